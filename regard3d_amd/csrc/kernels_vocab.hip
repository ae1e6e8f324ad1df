// kernels_vocab.hip -- pair proposal from bag-of-words view signatures (r3dm_propose_pairs, r3dm_view_signatures; DESIGN.md section
// 4.28).  The word of a row is its first neighbour among the codebook's rows, found by the exhaustive matcher (api_vocab.cpp stages
// the codebook as a private dataset view): no distance is computed here.  Everything below is integer arithmetic, so the results do
// not depend on the order in which workgroups, waves or atomics arrive.
//
//   vocab_hist_kernel<LDS>      first-neighbour indices of a view's rows (the 2-lists the matcher leaves on the device) -> the view's
//                               word histogram.  LDS = true (n_words <= kVocabHistLdsWords): a workgroup counts its rows into a private
//                               histogram in LDS and flushes the bins it touched with one global atomic each; LDS = false: global
//                               atomics directly
//   vocab_intersect_kernel      s(i, j) = sum_w min(h_i[w], h_j[w]) for all pairs of the listed views: a workgroup owns a 64 x 64 tile
//                               of (view, view) and a slice of the word axis, streams the slice through LDS 32 words at a time, a lane
//                               holds a 4 x 4 block of the tile in registers (8 x ds_read_b128 per 64 min-adds), and adds its u32 sums
//                               to the score matrix with integer atomics.  Only tiles on or above the diagonal run: s is symmetric.
//                               <IDF>: every min is multiplied by the word's weight q[w] (r3dm_vocab_set_weighting), staged beside the tile
//   vocab_df_kernel             df[w] = the number of listed views with h[w] > 0: what the host turns into the weights
//   vocab_weight_sum_kernel     W_i = sum_w q[w] h_i[w] in u64: the normaliser vocab_select_kernel is handed under IDF, where it is
//                               handed the row counts otherwise
//   vocab_select_kernel         one workgroup per view: top_k times the smallest composite ((2^32 - key) << 31) | rank not yet taken,
//                               key = floor(s 2^32 / min(n_i, n_j)) in u64 (n = row counts, or the W under IDF), rank = the candidate's place in view-id order
#include "kernels_match_common.hpp"

namespace r3dm {

using u32x4 = uint32_t __attribute__((ext_vector_type(4)));

template <bool LDS>
__global__ __launch_bounds__(256)
void vocab_hist_kernel(const VocabHistJob* __restrict__ jobs, uint32_t n_words, uint32_t rows_per_block)
{
    __shared__ uint32_t bins[LDS ? kVocabHistLdsWords : 1];
    const VocabHistJob job = jobs[blockIdx.y];
    const uint32_t r0 = blockIdx.x * rows_per_block;
    if (r0 >= job.n) return;                                   // (block-uniform)
    const uint32_t r1 = (job.n - r0 < rows_per_block) ? job.n : r0 + rows_per_block;
    if (LDS) {
        for (uint32_t w = threadIdx.x; w < n_words; w += 256) bins[w] = 0;
        r3dm_syncthreads();
    }
    for (uint32_t q = r0 + threadIdx.x; q < r1; q += 256) {
        const uint32_t w = (uint32_t)job.idx[2 * (size_t)q];   // the first entry of the row's 2-list
        if (w >= n_words) continue;                            // (never: the codebook has at least two rows)
        if (LDS) atomicAdd(&bins[w], 1u); else atomicAdd(&job.hist[w], 1u);
    }
    if (LDS) {
        r3dm_syncthreads();
        for (uint32_t w = threadIdx.x; w < n_words; w += 256) { const uint32_t v = bins[w]; if (v) atomicAdd(&job.hist[w], v); }
    }
}

hipError_t launch_vocab_hist(hipStream_t st, const VocabHistJob* jobs, uint32_t n_jobs, uint32_t max_n, uint32_t n_words)
{
    if (n_jobs == 0 || max_n == 0) return hipSuccess;
    if (n_jobs > 65535u) return hipErrorInvalidValue;
    constexpr uint32_t kRowsPerBlock = 4096;
    const dim3 grid((max_n + kRowsPerBlock - 1) / kRowsPerBlock, n_jobs);
    if (n_words <= kVocabHistLdsWords) hipLaunchKernelGGL(vocab_hist_kernel<true>, grid, dim3(256), 0, st, jobs, n_words, kRowsPerBlock);
    else hipLaunchKernelGGL(vocab_hist_kernel<false>, grid, dim3(256), 0, st, jobs, n_words, kRowsPerBlock);
    return hipGetLastError();
}

template <bool IDF>
__global__ __launch_bounds__(256)
void vocab_intersect_kernel(const VocabScoreParams P)
{
    if (blockIdx.x < blockIdx.y) return;                       // below the diagonal: the mirror tile writes both halves
    // a row of a stage is 32 words + 4 of padding: 36 r mod 64 runs through the sixteen multiples of 4, so the sixteen rows a
    // ds_read_b128 lane group reads lie on disjoint banks
    constexpr uint32_t S = kVocabChunk + 4;
    __shared__ u32x4 a4[kVocabTile * S / 4], b4[kVocabTile * S / 4];
    __shared__ u32x4 q4[IDF ? kVocabChunk / 4 : 1];            // IDF: the weights of the stage's words
    uint32_t* a = reinterpret_cast<uint32_t*>(a4);
    uint32_t* b = reinterpret_cast<uint32_t*>(b4);
    const uint32_t V = P.n_views;
    const uint32_t ti = blockIdx.y * kVocabTile, tj = blockIdx.x * kVocabTile;
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t w_begin = blockIdx.z * P.words_per_z;
    const uint32_t w_end = (P.stride - w_begin < P.words_per_z) ? P.stride : w_begin + P.words_per_z;
    // the loader: a thread brings 4 words of two rows of each operand per stage
    const uint32_t lr = threadIdx.x >> 3, lc = (threadIdx.x & 7u) * 4u;
    const uint32_t* src[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = (k < 2 ? ti : tj) + lr + 32u * (uint32_t)(k & 1);
        src[k] = v < V ? P.sig + (size_t)P.sig_row[v] * P.stride : nullptr;
    }
    uint32_t acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    for (uint32_t w0 = w_begin; w0 < w_end; w0 += kVocabChunk) {
        r3dm_syncthreads();                                    // every wave has finished with the previous stage
        const bool in = w0 + lc < w_end;                       // (stride and slice bounds are multiples of 4: a quad is in or out as a whole)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32x4 v = (in && src[k]) ? *reinterpret_cast<const u32x4*>(src[k] + w0 + lc) : u32x4{0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>((k < 2 ? a : b) + (lr + 32u * (uint32_t)(k & 1)) * S + lc) = v;
        }
        if (IDF && threadIdx.x < kVocabChunk / 4)
            q4[threadIdx.x] = w0 + threadIdx.x * 4u < w_end ? *reinterpret_cast<const u32x4*>(P.q + w0 + threadIdx.x * 4u) : u32x4{0u, 0u, 0u, 0u};
        r3dm_syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kVocabChunk; k += 4) {
            u32x4 av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) av[r] = *reinterpret_cast<const u32x4*>(a + (ty + 16u * (uint32_t)r) * S + k);
#pragma unroll
            for (int c = 0; c < 4; ++c) bv[c] = *reinterpret_cast<const u32x4*>(b + (tx + 16u * (uint32_t)c) * S + k);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t m = av[r][e] < bv[c][e] ? av[r][e] : bv[c][e];
                        if (IDF) acc[r][c] += q4[k / 4][e] * m; else acc[r][c] += m;
                    }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t i = ti + ty + 16u * (uint32_t)r, j = tj + tx + 16u * (uint32_t)c;
            if (i >= V || j >= V || i == j || acc[r][c] == 0) continue;
            atomicAdd(&P.scores[(size_t)i * V + j], acc[r][c]);
            if (ti != tj) atomicAdd(&P.scores[(size_t)j * V + i], acc[r][c]);
        }
}

hipError_t launch_vocab_intersect(hipStream_t st, const VocabScoreParams& P, uint32_t n_slices)
{
    if (P.n_views == 0) return hipSuccess;
    const uint32_t nt = (P.n_views + kVocabTile - 1) / kVocabTile;
    if (nt > 65535u || n_slices == 0 || n_slices > 65535u || (P.stride & 3u) || (P.words_per_z % kVocabChunk)) return hipErrorInvalidValue;
    if (P.q) hipLaunchKernelGGL(vocab_intersect_kernel<true>, dim3(nt, nt, n_slices), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(vocab_intersect_kernel<false>, dim3(nt, nt, n_slices), dim3(256), 0, st, P);
    return hipGetLastError();
}

// one thread per word: df[w] = the number of listed views whose signature holds word w
__global__ __launch_bounds__(256)
void vocab_df_kernel(const uint32_t* __restrict__ sig, const uint32_t* __restrict__ sig_row, uint32_t stride, uint32_t n_views, uint32_t n_words,
                     uint32_t* __restrict__ df)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n_words) return;
    uint32_t n = 0;
    for (uint32_t v = 0; v < n_views; ++v) n += sig[(size_t)sig_row[v] * stride + w] != 0u;
    df[w] = n;
}

// one workgroup per view: W[v] = sum_w q[w] h_v[w] in u64 (integer adds: the order of the reduction does not matter)
__global__ __launch_bounds__(256)
void vocab_weight_sum_kernel(const uint32_t* __restrict__ sig, const uint32_t* __restrict__ sig_row, uint32_t stride, uint32_t n_words,
                             const uint32_t* __restrict__ q, unsigned long long* __restrict__ W)
{
    __shared__ unsigned long long wave_sum[4];
    const uint32_t* h = sig + (size_t)sig_row[blockIdx.x] * stride;
    unsigned long long s = 0;
    for (uint32_t w = threadIdx.x; w < n_words; w += 256) s += (unsigned long long)q[w] * h[w];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = s;
    r3dm_syncthreads();
    if (threadIdx.x == 0) W[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

hipError_t launch_vocab_df(hipStream_t st, const uint32_t* sig, const uint32_t* sig_row, uint32_t stride, uint32_t n_views, uint32_t n_words, uint32_t* df)
{
    if (n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(vocab_df_kernel, dim3((n_words + 255u) / 256u), dim3(256), 0, st, sig, sig_row, stride, n_views, n_words, df);
    return hipGetLastError();
}

hipError_t launch_vocab_weight_sums(hipStream_t st, const uint32_t* sig, const uint32_t* sig_row, uint32_t stride, uint32_t n_views, uint32_t n_words,
                                    const uint32_t* q, unsigned long long* W)
{
    if (n_views == 0) return hipSuccess;
    hipLaunchKernelGGL(vocab_weight_sum_kernel, dim3(n_views), dim3(256), 0, st, sig, sig_row, stride, n_words, q, W);
    return hipGetLastError();
}

__global__ __launch_bounds__(256)
void vocab_select_kernel(const VocabSelectParams P)
{
    __shared__ unsigned long long wave_min[4];
    constexpr unsigned long long kTaken = ~0ull;               // above every composite: (2^32 << 31) | rank < 2^64 - 1
    const uint32_t i = blockIdx.x, V = P.n_views;
    const uint32_t ni = P.n_rows[i];
    unsigned long long lower = 0;                              // composites are unique (rank is): the next pick is the smallest one >= lower
    for (uint32_t t = 0; t < P.top_k; ++t) {
        unsigned long long best = kTaken;
        if (ni)
            for (uint32_t j = threadIdx.x; j < V; j += 256) {
                const uint32_t nj = P.n_rows[j];
                if (j == i || nj == 0) continue;
                const unsigned long long m = ni < nj ? ni : nj;
                const unsigned long long key = ((unsigned long long)P.scores[(size_t)i * V + j] << 32) / m;      // <= 2^32: s <= min(n_i, n_j)
                const unsigned long long comp = (((1ull << 32) - key) << 31) | P.rank[j];
                if (comp >= lower && comp < best) best = comp;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(best, off); best = o < best ? o : best; }
        r3dm_syncthreads();                                    // the previous round's wave_min has been read by everybody
        if ((threadIdx.x & 63u) == 0) wave_min[threadIdx.x >> 6] = best;
        r3dm_syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) best = wave_min[w] < best ? wave_min[w] : best;
        if (threadIdx.x == 0) P.sel[(size_t)i * P.top_k + t] = best == kTaken ? kNone : (uint32_t)(best & 0x7FFFFFFFull);
        lower = best == kTaken ? kTaken : best + 1;            // (exhausted: every later round finds nothing and writes kNone)
    }
}

hipError_t launch_vocab_select(hipStream_t st, const VocabSelectParams& P)
{
    if (P.n_views == 0 || P.top_k == 0) return hipSuccess;
    if (P.n_views >= (1u << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vocab_select_kernel, dim3(P.n_views), dim3(256), 0, st, P);
    return hipGetLastError();
}

}  // namespace r3dm
