// kernels_vocab_train.hip -- Lloyd's update step for pair-proposal vocabularies (r3dm_vocab_train).  The
// assignment is the exhaustive matcher's (api_vocab.cpp stages the codebook as a private dataset view); the stable order of a word's
// members is the radix sort of kernels_tracks.hip.  What is here turns the matcher's lists and that order into the new words, in the
// arithmetic include/r3dm.h states: f64 sums on a fixed two-level tree (blocks of kVocabTrainBlock consecutive members summed in member
// order, the block sums added in block order), exact integer sums for byte rows and bit counts for binary rows.  No float atomics: a
// (block, dimension) and a (word, dimension) each belong to one thread.
//
//   vocab_assign_kernel         a batch's first-neighbour entries -> assign[g]; counts the rows whose word changed with one ballot and
//                               one integer atomic per wavefront
//   vocab_sort_keys_kernel      (assign[g], g) as the radix sort's (key, value) pairs
//   vocab_locate_kernel         sorted position p -> (view, local row) of member g = order[p]: the last view whose first global row is
//                               <= g, by bisection of the prefix table of the views' row counts
//   vocab_block_sum_kernel      float / byte views: a thread owns four dimensions (one float4 of the fragment-order tiles, addressed as
//                               head_gather_l2_kernel does) of one block and adds the block's members in member order from 0.0, in f64
//   vocab_block_bits_kernel     binary views: a thread owns one 32-bit word of the rows of one block and counts its 32 bits
//   vocab_update_kernel<T>      a thread owns one dimension (byte of a binary row) of one word: the word's block sums in block order
//                               from 0.0 (integers for bits), the division of the type, the new element.  A word without members is
//                               left alone
#include "kernels_match_common.hpp"

namespace r3dm {

__global__ __launch_bounds__(256)
void vocab_assign_kernel(const VocabAssignJob* __restrict__ jobs, uint32_t* __restrict__ assign, unsigned int* __restrict__ moved)
{
    const VocabAssignJob job = jobs[blockIdx.y];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    bool changed = false;
    if (q < job.n) {
        const uint32_t w = (uint32_t)job.idx[2 * (size_t)q];   // the first entry of the row's 2-list
        const uint32_t g = job.g0 + q;
        changed = assign[g] != w;
        assign[g] = w;
    }
    const unsigned long long bal = __ballot(changed);
    if ((threadIdx.x & 63u) == 0 && bal) atomicAdd(moved, (unsigned int)__builtin_popcountll(bal));
}

hipError_t launch_vocab_assign(hipStream_t st, const VocabAssignJob* jobs, uint32_t n_jobs, uint32_t max_n, uint32_t* assign, unsigned int* moved)
{
    if (n_jobs == 0 || max_n == 0) return hipSuccess;
    if (n_jobs > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vocab_assign_kernel, dim3((max_n + 255u) / 256u, n_jobs), dim3(256), 0, st, jobs, assign, moved);
    return hipGetLastError();
}

__global__ __launch_bounds__(256)
void vocab_sort_keys_kernel(const uint32_t* __restrict__ assign, uint32_t T, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= T) return;
    keys[g] = assign[g]; vals[g] = g;
}

__global__ __launch_bounds__(256)
void vocab_locate_kernel(const uint32_t* __restrict__ order, uint32_t T, const uint32_t* __restrict__ base, uint32_t n_views, uint2* __restrict__ loc)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= T) return;
    const uint32_t g = order[p];
    uint32_t lo = 0, hi = n_views;                             // last k with base[k] <= g (base[0] = 0 <= g; empty views repeat a base)
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (base[mid] <= g) lo = mid; else hi = mid; }
    loc[p] = make_uint2(lo, g - base[lo]);
}

hipError_t launch_vocab_sort_keys(hipStream_t st, const uint32_t* assign, uint32_t T, uint32_t* keys, uint32_t* vals)
{
    if (T == 0) return hipSuccess;
    hipLaunchKernelGGL(vocab_sort_keys_kernel, dim3((T + 255u) / 256u), dim3(256), 0, st, assign, T, keys, vals);
    return hipGetLastError();
}

hipError_t launch_vocab_locate(hipStream_t st, const uint32_t* order, uint32_t T, const uint32_t* base, uint32_t n_views, uint2* loc)
{
    if (T == 0 || n_views == 0) return hipSuccess;
    hipLaunchKernelGGL(vocab_locate_kernel, dim3((T + 255u) / 256u), dim3(256), 0, st, order, T, base, n_views, loc);
    return hipGetLastError();
}

__global__ __launch_bounds__(256)
void vocab_block_sum_kernel(const VocabTrainParams P)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t b = (uint32_t)(e / P.pieces), k = (uint32_t)(e % P.pieces);
    if (b >= P.n_blocks) return;
    const uint2 blk = P.blocks[b];                             // (first member, members)
    const uint2* __restrict__ loc = P.loc + blk.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (uint32_t m = 0; m < blk.y; ++m) {
        const uint2 l = loc[m];
        const f32x4 v = ((const f32x4*)P.views[l.x])[(size_t)(l.y >> 5) * (P.row_units * 32u) + k * 32u + (l.y & 31u)];
        s0 += (double)v[0]; s1 += (double)v[1]; s2 += (double)v[2]; s3 += (double)v[3];
    }
    double* out = P.block_sums + ((size_t)b * P.pieces + k) * 4u;
    out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3;
}

__global__ __launch_bounds__(256)
void vocab_block_bits_kernel(const VocabTrainParams P)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t b = (uint32_t)(e / P.pieces), k = (uint32_t)(e % P.pieces);
    if (b >= P.n_blocks) return;
    const uint2 blk = P.blocks[b];
    const uint2* __restrict__ loc = P.loc + blk.x;
    uint32_t ones[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) ones[i] = 0;
    for (uint32_t m = 0; m < blk.y; ++m) {
        const uint2 l = loc[m];
        const uint32_t x = ((const uint32_t*)P.views[l.x])[(size_t)l.y * P.row_units + k];
#pragma unroll
        for (int i = 0; i < 32; ++i) ones[i] += (x >> i) & 1u;
    }
    uint32_t* out = P.block_bits + ((size_t)b * P.pieces + k) * 32u;
#pragma unroll
    for (int i = 0; i < 32; ++i) out[i] = ones[i];
}

template <int DTYPE>
__global__ __launch_bounds__(256)
void vocab_update_kernel(const VocabTrainParams P)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t w = (uint32_t)(e / P.dim), d = (uint32_t)(e % P.dim);
    if (w >= P.n_words) return;
    const uint32_t count = P.counts[w];
    if (count == 0) return;                                    // a word without members keeps its row
    const uint32_t b0 = P.first_block[w], b1 = P.first_block[w + 1];
    if (DTYPE == (int)R3DM_BIN) {
        uint32_t ones[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const size_t per_block = (size_t)P.pieces * 32u;
        for (uint32_t b = b0; b < b1; ++b) {
            const uint32_t* src = P.block_bits + (size_t)b * per_block + (size_t)d * 8u;
#pragma unroll
            for (int i = 0; i < 8; ++i) ones[i] += src[i];
        }
        uint32_t byte = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) byte |= (2ull * ones[i] > (unsigned long long)count ? 1u : 0u) << i;
        ((unsigned char*)P.words)[(size_t)w * P.dim + d] = (unsigned char)byte;
    } else {
        const size_t per_block = (size_t)P.pieces * 4u;
        double s = 0.0;
        for (uint32_t b = b0; b < b1; ++b) s += P.block_sums[(size_t)b * per_block + d];
        if (DTYPE == (int)R3DM_F32) ((float*)P.words)[(size_t)w * P.dim + d] = (float)(s / (double)count);
        else {
            const unsigned long long S = (unsigned long long)s;  // byte sums are integers below 2^53: exact in f64
            ((unsigned char*)P.words)[(size_t)w * P.dim + d] = (unsigned char)((2ull * S + count) / (2ull * count));
        }
    }
}

hipError_t launch_vocab_block_sums(hipStream_t st, const VocabTrainParams& P, r3dm_dtype dtype)
{
    if (P.n_blocks == 0) return hipSuccess;
    const uint64_t threads = (uint64_t)P.n_blocks * P.pieces, grid = (threads + 255u) / 256u;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (dtype == R3DM_BIN) hipLaunchKernelGGL(vocab_block_bits_kernel, dim3((uint32_t)grid), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(vocab_block_sum_kernel, dim3((uint32_t)grid), dim3(256), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_vocab_update(hipStream_t st, const VocabTrainParams& P, r3dm_dtype dtype)
{
    const uint64_t threads = (uint64_t)P.n_words * P.dim, grid = (threads + 255u) / 256u;
    if (grid == 0 || grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (dtype == R3DM_BIN) hipLaunchKernelGGL(vocab_update_kernel<(int)R3DM_BIN>, dim3((uint32_t)grid), dim3(256), 0, st, P);
    else if (dtype == R3DM_U8) hipLaunchKernelGGL(vocab_update_kernel<(int)R3DM_U8>, dim3((uint32_t)grid), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(vocab_update_kernel<(int)R3DM_F32>, dim3((uint32_t)grid), dim3(256), 0, st, P);
    return hipGetLastError();
}

}  // namespace r3dm
