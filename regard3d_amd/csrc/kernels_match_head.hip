// kernels_match_head.hip -- the gate of opt-in preemptive matching (r3dm_set_preemptive_matching, r3dm_preselect_pairs; DESIGN.md
// section 4.25).  A view's HEAD is its min(h, n) largest-scale rows (chosen by the host, kept in ascending row index) gathered into a
// small row-major buffer of its own; the gate 2-NN-matches the head of J against the head of I and counts the queries that pass the
// ratio test.  A pair whose count stays below the threshold is never handed to a matcher.
//
// The distance is the reference's (exact_l2sq: 4-way unrolled, scalar tail, no FMA; the popcount Hamming distance for binary rows):
// its summation order decides the count and the count decides which pairs exist, so there is nothing to certify against -- both
// kernels are VALU work on purpose.  The L2 loop stays written out against the row-major stage, tail included: through the shared
// stage_l2sq of kernels_match_common.hpp the gate measured 0.1 - 0.3 % slower on 144-float rows (profiles/scan_steps_perf.txt).
//
//   head_gather_l2_kernel       rows out of the fragment-order f32 tiles -> f32 [hn][8 G], row-major (views registered from host
//                               or device pointers alike: the tiles are what every float / byte view holds)
//   head_gather_bin_kernel      rows out of the word rows -> u32 [hn][W]
//   l2_head_match_kernel<G>     padded lengths 64 / 128 / 144 / 256: one workgroup per pair, a lane holds one head row of J in registers,
//                               I's head is streamed through LDS 32 rows at a time and read wave-uniformly (LDS broadcast)
//   hamming_head_match_kernel<W>   the same frame over 8 / 16 words
//
// Only the two smallest distances of a query decide whether it counts, not the rows that gave them: ties need no order here, and the
// (d0, d1) of two disjoint sets of rows of I merge exactly.  A head of J of at most 128 (64) rows therefore occupies the first two
// (one) waves and the other waves take the SAME queries against every second (fourth) row of an LDS stage; the partial (d0, d1) are
// merged through LDS.  All four waves work at every h.
#include "kernels_match_common.hpp"

namespace r3dm {

__global__ __launch_bounds__(256)
void head_gather_l2_kernel(const float* __restrict__ tiled, const uint32_t* __restrict__ rows, uint32_t hn, uint32_t D4, f32x4* __restrict__ out)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= hn * D4) return;
    const uint32_t hr = e / D4, k = e % D4, row = rows[hr];
    out[e] = ((const f32x4*)tiled)[(size_t)(row >> 5) * (D4 * 32u) + k * 32u + (row & 31u)];
}

__global__ __launch_bounds__(256)
void head_gather_bin_kernel(const uint32_t* __restrict__ bin, const uint32_t* __restrict__ rows, uint32_t hn, uint32_t W, uint32_t* __restrict__ out)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= hn * W) return;
    out[e] = bin[(size_t)rows[e / W] * W + e % W];
}

hipError_t launch_head_gather(hipStream_t st, const void* src, const uint32_t* rows, uint32_t hn, uint32_t per_row, bool binary, void* out)
{
    if (hn == 0) return hipSuccess;
    const dim3 grid((hn * per_row + 255u) / 256u);
    if (binary) hipLaunchKernelGGL(head_gather_bin_kernel, grid, dim3(256), 0, st, (const uint32_t*)src, rows, hn, per_row, (uint32_t*)out);
    else hipLaunchKernelGGL(head_gather_l2_kernel, grid, dim3(256), 0, st, (const float*)src, rows, hn, per_row, (f32x4*)out);
    return hipGetLastError();
}

// how the 256 threads of a pair's workgroup are dealt: `part` takes query `q` against the rows part, part + parts, ... of every stage
struct HeadDeal { uint32_t parts, part, q; };
__device__ __forceinline__ HeadDeal head_deal(uint32_t nJ)
{
    HeadDeal d;
    d.parts = nJ <= 64u ? 4u : (nJ <= 128u ? 2u : 1u);
    const uint32_t span = 256u / d.parts;
    d.part = threadIdx.x / span; d.q = threadIdx.x % span;
    return d;
}

// merge of the parts' (d0, d1) in LDS and the count of the pair: `pass(d0, d1)` is the ratio test of one query.  Called by all threads.
template <class T, class Pass>
__device__ __forceinline__ void head_count(const HeadMatchParams& P, const HeadPair& hp, const HeadDeal& dl, uint32_t nJ, T d0, T d1,
                                           T* s0, T* s1, uint32_t* wave_cnt, Pass&& pass)
{
    s0[threadIdx.x] = d0; s1[threadIdx.x] = d1;
    r3dm_syncthreads();
    bool ok = false;
    if (dl.part == 0 && dl.q < nJ) {
        const uint32_t span = 256u / dl.parts;
        for (uint32_t p = 1; p < dl.parts; ++p) {
            const T b0 = s0[p * span + dl.q], b1 = s1[p * span + dl.q];
            const T lo = d0 < b0 ? d0 : b0, hi = d0 < b0 ? b0 : d0, m1 = d1 < b1 ? d1 : b1;
            d0 = lo; d1 = hi < m1 ? hi : m1;
        }
        ok = pass(d0, d1);
    }
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63u) == 0) wave_cnt[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(bal);
    r3dm_syncthreads();
    if (threadIdx.x == 0) P.counts[hp.out] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

template <int G>
__global__ __launch_bounds__(256)
void l2_head_match_kernel(const HeadMatchParams P)
{
    constexpr int D4 = G * 2;                        // float4 per (padded) row
    __shared__ f32x4 tile[32 * D4];                  // 32 head rows of I, row-major
    __shared__ float s0[256], s1[256];
    __shared__ uint32_t wave_cnt[4];
    const HeadPair hp = P.pairs[blockIdx.x];
    const HeadDev hI = P.heads[hp.sI], hJ = P.heads[hp.sJ];
    const uint32_t nI = hI.n, nJ = hJ.n;             // both <= 256
    const uint32_t d4 = hI.dim >> 2, tail = hI.dim & 3u;
    const gf4p irows = (gf4p)hI.rows, jrows = (gf4p)hJ.rows;
    const HeadDeal dl = head_deal(nJ);
    const bool active = dl.q < nJ;
    f32x4 jv[D4];
    {
        const gf4p jrow = jrows + (size_t)(active ? dl.q : 0u) * D4;
#pragma unroll
        for (int k = 0; k < D4; ++k) jv[k] = (k <= (int)d4 && k < D4) ? jrow[k] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float d0 = R3DM_INF, d1 = R3DM_INF;
    for (uint32_t t0 = 0; t0 < nI; t0 += 32) {
        r3dm_syncthreads();                          // every wave has finished with the previous stage
        const uint32_t rows_here = (nI - t0 < 32u) ? nI - t0 : 32u;
        {
            const gf4p src = irows + (size_t)t0 * D4;
            for (uint32_t e = threadIdx.x; e < rows_here * D4; e += 256) tile[e] = src[e];
        }
        r3dm_syncthreads();
        for (uint32_t r = dl.part; r < rows_here; r += dl.parts) {
            float result = 0.0f;
#pragma unroll
            for (int k = 0; k < D4; ++k) {
                if (k < (int)d4) {
                    const f32x4 a = tile[r * D4 + k];
                    const float e0 = a[0] - jv[k][0], e1 = a[1] - jv[k][1], e2 = a[2] - jv[k][2], e3 = a[3] - jv[k][3];
                    result += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
                } else if (k == (int)d4 && tail) {   // the scalar tail, one element at a time as exact_l2sq adds it
                    const f32x4 a = tile[r * D4 + k];
                    const float e0 = a[0] - jv[k][0], e1 = a[1] - jv[k][1], e2 = a[2] - jv[k][2];
                    result += e0 * e0;
                    if (tail > 1) result += e1 * e1;
                    if (tail > 2) result += e2 * e2;
                }
            }
            const float od0 = d0;
            d0 = result < od0 ? result : od0;
            d1 = result < od0 ? od0 : (result < d1 ? result : d1);
        }
    }
    const float R = P.ratio_R;
    head_count(P, hp, dl, nJ, d0, d1, s0, s1, wave_cnt, [&](float a, float b) { return nI >= 2u && a < R * b; });
}

template <int W>
__global__ __launch_bounds__(256)
void hamming_head_match_kernel(const HeadMatchParams P)
{
    __shared__ uint32_t tile[32 * W];
    __shared__ uint32_t s0[256], s1[256];
    __shared__ uint32_t wave_cnt[4];
    const HeadPair hp = P.pairs[blockIdx.x];
    const HeadDev hI = P.heads[hp.sI], hJ = P.heads[hp.sJ];
    const uint32_t nI = hI.n, nJ = hJ.n;
    const uint32_t* __restrict__ irows = (const uint32_t*)hI.rows;
    const uint32_t* __restrict__ jrows = (const uint32_t*)hJ.rows;
    const HeadDeal dl = head_deal(nJ);
    const bool active = dl.q < nJ;
    uint32_t jv[W];
#pragma unroll
    for (int w = 0; w < W; ++w) jv[w] = jrows[(size_t)(active ? dl.q : 0u) * W + w];
    constexpr uint32_t kFar = 0xFFFFFFFFu;
    uint32_t d0 = kFar, d1 = kFar;
    for (uint32_t t0 = 0; t0 < nI; t0 += 32) {
        r3dm_syncthreads();
        const uint32_t rows_here = (nI - t0 < 32u) ? nI - t0 : 32u;
        for (uint32_t e = threadIdx.x; e < rows_here * W; e += 256) tile[e] = irows[(size_t)t0 * W + e];
        r3dm_syncthreads();
        for (uint32_t r = dl.part; r < rows_here; r += dl.parts) {
            uint32_t d = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) d += (uint32_t)__builtin_popcount(jv[w] ^ tile[r * W + w]);
            const uint32_t od0 = d0;
            d0 = d < od0 ? d : od0;
            d1 = d < od0 ? od0 : (d < d1 ? d : d1);
        }
    }
    const float R = P.ratio_R;
    // NNdistanceRatio on unsigned distances converted to float
    head_count(P, hp, dl, nJ, d0, d1, s0, s1, wave_cnt, [&](uint32_t a, uint32_t b) { return nI >= 2u && (float)a < R * (float)b; });
}

hipError_t launch_head_match(hipStream_t st, const HeadMatchParams& P, uint32_t n_pairs, bool binary, uint32_t G_or_words)
{
    if (n_pairs == 0) return hipSuccess;
    if (n_pairs > kMaxBlocksOf256) return hipErrorInvalidValue;
    const dim3 grid(n_pairs);
    if (binary)
        return dispatch_words(G_or_words, [&](auto w) {
            hipLaunchKernelGGL((hamming_head_match_kernel<decltype(w)::value>), grid, dim3(256), 0, st, P);
            return hipGetLastError();
        });
    return dispatch_g(G_or_words, [&](auto g) {
        hipLaunchKernelGGL((l2_head_match_kernel<decltype(g)::value>), grid, dim3(256), 0, st, P);
        return hipGetLastError();
    });
}

}  // namespace r3dm
