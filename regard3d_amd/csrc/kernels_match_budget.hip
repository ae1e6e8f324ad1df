// kernels_match_budget.hip -- the opt-in match budget (r3dm_set_match_budget, r3dm_budget_rows): a view of more
// than N rows is matched through a SUB-VIEW of its N highest-priority rows.
//
//   budget_select_kernel        one workgroup per view: the min(N, n) rows that come first under (priority descending, row ascending),
//                               written in ascending row index.  The key of a row is its priority's bit pattern -- priorities are finite
//                               and >= 0 with -0.0 stored as +0.0, so the unsigned order of the patterns is the order of the values.
//                               Four passes of an MSB-first radix select (256-bin histograms in LDS) find the exact N-th key from the top
//                               and how many rows EQUAL to it belong to the list; one order-preserving compaction then takes every row
//                               above the key and the lowest-indexed equal rows, kBudgetChunk rows per step: wave64 ballots give a lane its
//                               rank inside its wave, four wave counts in LDS its rank inside the step, two running counts the rest.  The
//                               list is a function of (priority, n, N) only: no atomics decide a position.
//   budget_gather_*_kernel      the listed rows out of the view's resident layout (fragment-order f32 tiles / word rows) and their
//                               positions -> row-major arrays of the view's own element type, which are staged like a registered view
//   budget_remap_kernel         one workgroup per pair of a finalised batch: match (i', j') of sub-views -> (S(I)[i'], S(J)[j']); S is
//                               ascending, so the (i, j) order of a pair's list survives
#include "kernels_match_common.hpp"

namespace r3dm {

static_assert(kBudgetChunk == 256u, "budget_select_kernel: one row per thread and step");

__global__ __launch_bounds__(256)
void budget_select_kernel(const BudgetSelectJob* __restrict__ jobs)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_remaining;
    __shared__ uint32_t wave_eq[4], wave_take[4];
    const BudgetSelectJob jb = jobs[blockIdx.x];
    const uint32_t tid = threadIdx.x, n = jb.n, hn = jb.N < n ? jb.N : n;
    if (hn == 0) return;
    const uint32_t* __restrict__ key = reinterpret_cast<const uint32_t*>(jb.priority);
    if (!key || hn == n) {                           // no priority, or a whole view: the first rows
        for (uint32_t r = tid; r < hn; r += 256u) jb.rows_out[r] = r;
        return;
    }
    // ---- radix select: after the pass of a digit, `prefix` holds the digits found so far of the hn-th largest key and `remaining`
    // counts from the top among the keys that share them
    uint32_t prefix = 0, mask = 0, remaining = hn;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        r3dm_syncthreads();
        for (uint32_t r = tid; r < n; r += 256u) {
            const uint32_t k = key[r];
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        r3dm_syncthreads();
        if (tid == 0) {
            uint32_t rem = remaining, d = 255u;
            for (;;) {
                const uint32_t cnt = hist[d];
                if (cnt >= rem || d == 0u) break;
                rem -= cnt; --d;
            }
            s_prefix = prefix | (d << shift); s_remaining = rem;
        }
        r3dm_syncthreads();
        prefix = s_prefix; remaining = s_remaining; mask |= 255u << shift;
    }
    const uint32_t T = prefix, need_eq = remaining;  // rows above T: all; rows equal to T: the need_eq lowest row indices
    // ---- compaction in row order
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t run_eq = 0, run_out = 0;                // equal rows / taken rows of the steps walked so far (the same in every thread)
    for (uint32_t base = 0; base < n && run_out < hn; base += kBudgetChunk) {
        const uint32_t r = base + tid;
        const uint32_t k = r < n ? key[r] : 0u;
        const bool gt = r < n && k > T, eq = r < n && k == T;
        const unsigned long long eq_mask = __ballot(eq);
        if (lane == 0) wave_eq[wave] = (uint32_t)__builtin_popcountll(eq_mask);
        r3dm_syncthreads();
        uint32_t eq_before = run_eq + (uint32_t)__builtin_popcountll(eq_mask & below), eq_step = 0;
        for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) eq_before += wave_eq[w]; eq_step += wave_eq[w]; }
        const bool take = gt || (eq && eq_before < need_eq);
        const unsigned long long take_mask = __ballot(take);
        if (lane == 0) wave_take[wave] = (uint32_t)__builtin_popcountll(take_mask);
        r3dm_syncthreads();
        uint32_t pos = run_out + (uint32_t)__builtin_popcountll(take_mask & below), take_step = 0;
        for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) pos += wave_take[w]; take_step += wave_take[w]; }
        if (take && pos < hn) jb.rows_out[pos] = r;
        run_eq += eq_step; run_out += take_step;
        r3dm_syncthreads();                          // the wave counts are rewritten by the next step
    }
}

hipError_t launch_budget_select(hipStream_t st, const BudgetSelectJob* jobs_dev, uint32_t n_jobs)
{
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(budget_select_kernel, dim3(n_jobs), dim3(256), 0, st, jobs_dev);
    return hipGetLastError();
}

// element (row, col) of the fragment-order f32 tiles: 32 rows per tile, D4 = 2 G float4 per padded row (head_gather_l2_kernel reads
// the same tiles a float4 at a time)
__device__ __forceinline__ float tiled_at(const float* __restrict__ tiled, uint32_t D4, uint32_t row, uint32_t col)
{
    return tiled[((size_t)(row >> 5) * (D4 * 32u) + (size_t)(col >> 2) * 32u + (row & 31u)) * 4u + (col & 3u)];
}

template <class T>
__global__ __launch_bounds__(256)
void budget_gather_l2_kernel(const float* __restrict__ tiled, const uint32_t* __restrict__ rows, uint32_t n, uint32_t hn, uint32_t dim, uint32_t D4, T* __restrict__ out)
{
    const size_t total = (size_t)hn * dim;
    for (size_t e = (size_t)blockIdx.x * 256u + threadIdx.x; e < total; e += (size_t)gridDim.x * 256u) {
        const uint32_t hr = (uint32_t)(e / dim), col = (uint32_t)(e % dim);
        const uint32_t row = rows[hr] < n ? rows[hr] : n - 1u;  // (a list is always inside its view; no read depends on that)
        out[e] = (T)tiled_at(tiled, D4, row, col);              // (U8 views hold the integers 0 .. 255 as floats: the conversion back is exact)
    }
}

__global__ __launch_bounds__(256)
void budget_gather_bin_kernel(const uint32_t* __restrict__ bin, const uint32_t* __restrict__ rows, uint32_t n, uint32_t hn, uint32_t nbytes, uint32_t W, uint8_t* __restrict__ out)
{
    const size_t total = (size_t)hn * nbytes;
    for (size_t e = (size_t)blockIdx.x * 256u + threadIdx.x; e < total; e += (size_t)gridDim.x * 256u) {
        const uint32_t hr = (uint32_t)(e / nbytes), b = (uint32_t)(e % nbytes);
        const uint32_t row = rows[hr] < n ? rows[hr] : n - 1u;
        out[e] = (uint8_t)(bin[(size_t)row * W + (b >> 2)] >> (8u * (b & 3u)));
    }
}

__global__ __launch_bounds__(256)
void budget_gather_xy_kernel(const float2* __restrict__ xy, const uint32_t* __restrict__ rows, uint32_t n, uint32_t hn, float2* __restrict__ out)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e < hn) out[e] = xy[rows[e] < n ? rows[e] : n - 1u];
}

hipError_t launch_budget_gather(hipStream_t st, const BudgetGatherArgs& A)
{
    if (A.hn == 0 || A.n == 0) return hipSuccess;
    const size_t total = (size_t)A.hn * A.dim;
    const dim3 grid((uint32_t)std::min<size_t>((total + 255u) / 256u, 65536u));
    if (A.dtype == 2) hipLaunchKernelGGL(budget_gather_bin_kernel, grid, dim3(256), 0, st, (const uint32_t*)A.src, A.rows, A.n, A.hn, A.dim, A.per_row, (uint8_t*)A.out);
    else if (A.dtype == 1) hipLaunchKernelGGL((budget_gather_l2_kernel<uint8_t>), grid, dim3(256), 0, st, (const float*)A.src, A.rows, A.n, A.hn, A.dim, A.per_row, (uint8_t*)A.out);
    else hipLaunchKernelGGL((budget_gather_l2_kernel<float>), grid, dim3(256), 0, st, (const float*)A.src, A.rows, A.n, A.hn, A.dim, A.per_row, (float*)A.out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !A.xy) return e;
    hipLaunchKernelGGL(budget_gather_xy_kernel, dim3((A.hn + 255u) / 256u), dim3(256), 0, st, (const float2*)A.xy, A.rows, A.n, A.hn, (float2*)A.xy_out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256)
void budget_remap_kernel(const BudgetRemapParams P)
{
    const uint2 pr = P.pairs[blockIdx.x];
    const BudgetMap mI = P.maps[pr.x], mJ = P.maps[pr.y];
    if (!mI.rows && !mJ.rows) return;
    const uint32_t cnt = P.pair_cnt[blockIdx.x];
    r3dm_match* __restrict__ m = P.matches + P.pair_off[blockIdx.x];
    for (uint32_t t = threadIdx.x; t < cnt; t += 256u) {
        r3dm_match v = m[t];
        if (mI.rows && v.i < mI.n) v.i = mI.rows[v.i];
        if (mJ.rows && v.j < mJ.n) v.j = mJ.rows[v.j];
        m[t] = v;
    }
}

hipError_t launch_budget_remap(hipStream_t st, const BudgetRemapParams& P, uint32_t n_pairs)
{
    if (n_pairs == 0) return hipSuccess;
    if (n_pairs > kMaxBlocksOf256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(budget_remap_kernel, dim3(n_pairs), dim3(256), 0, st, P);
    return hipGetLastError();
}

}  // namespace r3dm
