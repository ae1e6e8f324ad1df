// kernels_match_knn.hip -- exhaustive k-NN, k = 1 .. R3DM_KNN_MAX (8), of one (dataset, query) pair: what stands behind r3dm_knn /
// r3dm_index_knn for k >= 3 (ArrayMatcher::SearchNeighbours with any NN, /root/reference/src/utils/matcher_kgraph.h:205-251,
// matcher_hnsw.h:138-173).
//   l2_knnk_mfma_kernel<G, PF, KL>     the nominator on the f32 tiles, K-lists per lane half.  Its tile step is l2_tile_step<G, 1, PF, 3>
//                                      (kernels_match_tiles.hpp), the function template l2_knn2_mfma_kernel instantiates with Top2
//   (TopK<KL>, knnk_finish<KL>         its lists and its tail -- re-score the nominees in the reference arithmetic, order, certify
//                                      the k-th -- live in kernels_match_knn_lists.hpp, shared with kernels_match_knn16.hip)
//   l2_exact_knn_items_kernel<KL>      the exact scan behind it (uncertified queries; lengths without a tensor kernel)
//   hamming_knnk_kernel<W, KL, QL>     binary rows: xor + popcount with exact (distance, row) K-lists per lane
// KL is the list depth a kernel is built with: 4 for k <= 4, 8 above (dispatch_kl); k itself is a run-time value (k <= KL).
//
// Arithmetic contract as everywhere (kernels_match_common.hpp): the f32 4-way unrolled sum of squared differences without FMA, equal
// distances -> lowest dataset row.  This file is compiled with -ffp-contract=off; fused operations are spelled fmaf() / MFMA.
#include "kernels_match_tiles.hpp"

namespace r3dm {

// ------------------------------------------------------------------------------------------------
// The nominator.  One workgroup = 4 waves, each wave one query tile (32 queries, pre-scaled by -2) in registers as the MFMA B
// fragments; every 32-row dataset tile streams through as the A fragment from the fragment-order image (raw_buffer_load_b128, PF-deep
// rolling window).  C is initialised to ||a||^2, so the accumulator holds key = ||a||^2 - 2 a.q; lane (h, c) owns query column c and
// the 16 rows {(r & 3) + 8 (r >> 2) + 4 h} of a tile.  Ping-pong accumulators: the list updates of tile t - 1 issue in the shadow of
// tile t's MFMAs.  No LDS, no barriers.  One query tile per wave (NJ = 1): the K-list of a query tile costs 2 KL + 1 registers where
// Top2 costs 5, and the 2-NN kernel at NJ = 2 already sits near 256.
// ------------------------------------------------------------------------------------------------
template <int G, int PF, int KL>
__global__ __launch_bounds__(256, 2)
void l2_knnk_mfma_kernel(const KnnParams P)
{
    static_assert(G % PF == 0, "prefetch window must divide the group count");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t h = lane >> 5, c = lane & 31u;
    const ImgDev* __restrict__ Ip = P.imgs + P.sI;
    const ImgDev* __restrict__ Jp = P.imgs + P.sJ;
    const uint32_t ntI = Ip->n_tiles, ntJ = Jp->n_tiles;
    const uint32_t qt = blockIdx.x * 4u + wave;
    if (qt >= ntJ) return;                            // wave-uniform; no barriers in this kernel

    f32x4 bq[1][G];
    {
        const gf4p src = (gf4p)Jp->tiled + (size_t)qt * (G * 64) + lane;
#pragma unroll
        for (int g = 0; g < G; ++g) bq[0][g] = src[g * 64] * -2.0f;
    }
    TopK<KL> st[1];
    topk_init(st[0]);

    // dataset stream: float4 index = (t G + g) 64 + lane; norms of tile t, quad qd: float4 index 8 t + 2 qd + h
    const gf4p abase = (gf4p)Ip->tiled;
    const gf4p nbase = (gf4p)Ip->norms;
    f32x4 abuf[PF];
#pragma unroll
    for (int s = 0; s < PF; ++s) abuf[s] = abase[s * 64 + lane];
    f32x4 nrm[4];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) nrm[qd] = nbase[2 * qd + h];
    f32x16 accA[1], accB[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) accB[0][r] = R3DM_INF;       // "tile -1": keys that never enter a list
    const __amdgpu_buffer_rsrc_t ra = wave_uniform_rsrc(Ip->tiled), rn = wave_uniform_rsrc(Ip->norms);
    const uint32_t voffA = lane * 16u, voffN = h * 16u;
    const uint32_t tileB = (uint32_t)G * 1024u;                // bytes per tile (the launcher keeps n_tiles x tileB below 2^31)
    const uint32_t hb = 4u * h;
    uint32_t t = 0;
    for (; t + 1 < ntI; t += 2) {
        l2_tile_step<G, 1, PF, 3>(ra, rn, voffA, voffN, t * tileB + PF * 1024u, (t + 1) * 128u, abuf, nrm, bq, accA, accB, st, (t - 1) * 32u + hb);
        l2_tile_step<G, 1, PF, 3>(ra, rn, voffA, voffN, (t + 1) * tileB + PF * 1024u, (t + 2) * 128u, abuf, nrm, bq, accB, accA, st, t * 32u + hb);
    }
    if (t < ntI) {
        l2_tile_step<G, 1, PF, 3>(ra, rn, voffA, voffN, t * tileB + PF * 1024u, (t + 1) * 128u, abuf, nrm, bq, accA, accB, st, (t - 1) * 32u + hb);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (__builtin_amdgcn_ballot_w64(accA[0][r] < st[0].d[KL]) != 0ull) topk_push(st[0], accA[0][r], t * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (__builtin_amdgcn_ballot_w64(accB[0][r] < st[0].d[KL]) != 0ull) topk_push(st[0], accB[0][r], (ntI - 1) * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
    }
    knnk_finish<KL>(P, Ip, Jp, st[0], qt, h, c, (float)(G * 8));
}

template <int G, int PF>
static hipError_t launch_knnk_g(hipStream_t st, const KnnParams& P, uint32_t grid)
{
    return dispatch_kl(P.k, [&](auto kl) {
        hipLaunchKernelGGL((l2_knnk_mfma_kernel<G, PF, decltype(kl)::value>), dim3(grid), dim3(256), 0, st, P);
        return hipGetLastError();
    });
}

// hipErrorInvalidValue: no nominator for this launch (G without a tensor kernel, or a dataset whose tiles pass the 2^31-byte reach
// of the buffer offsets): the caller runs the exact scan over every query
hipError_t launch_l2_knnk(hipStream_t st, const KnnParams& P, uint32_t G, uint32_t n_tiles_dataset, uint32_t n_tiles_query)
{
    if (P.k < 1 || P.k > R3DM_KNN_MAX) return hipErrorInvalidValue;
    if (!tiles_within_reach(n_tiles_dataset, G * 1024u)) return hipErrorInvalidValue;
    const uint32_t grid = (n_tiles_query + 3u) / 4u;
    if (grid == 0) return hipSuccess;
    switch (G) {
        case 8:  return launch_knnk_g<8, 4>(st, P, grid);
        case 16: return launch_knnk_g<16, 4>(st, P, grid);
        case 18: return launch_knnk_g<18, 3>(st, P, grid);
        case 32: return launch_knnk_g<32, 4>(st, P, grid);
        default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------------------------------------
// The exact K scan: one workgroup per query, the reference arithmetic over every dataset row.  Thread t keeps the K-list of its rows
// t, t + 256, ... under (distance, row) -- its rows ascend, so a strict `<` keeps the lowest row of equal distances first -- and an
// LDS tree merges the 256 sorted lists.  Serves the uncertified queries of the nominator (from_list), descriptor lengths without a
// tensor kernel, and through exact_l2sq any length that is no multiple of 4, scalar tail included.
// ------------------------------------------------------------------------------------------------
template <int KL>
__global__ __launch_bounds__(256)
void l2_exact_knn_items_kernel(const KnnParams P, uint32_t count, int from_list)
{
    __shared__ float sd[KL * 256];
    __shared__ uint32_t si[KL * 256];
    const ImgDev* __restrict__ Ip = P.imgs + P.sI;
    const ImgDev* __restrict__ Jp = P.imgs + P.sJ;
    const uint32_t dim = Ip->dim, nI = Ip->n, k = P.k, tid = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {
        const uint32_t q = from_list ? P.fb_q[it] : it;
        if (q >= Jp->n) continue;                                 // block-uniform
        const float* qv = Jp->rows + (size_t)q * dim;
        float kd[KL]; uint32_t ki[KL];
#pragma unroll
        for (int j = 0; j < KL; ++j) { kd[j] = R3DM_INF; ki[j] = kNone; }
        for (uint32_t r = tid; r < nI; r += 256) {
            const float d = exact_l2sq(Ip->rows + (size_t)r * dim, qv, dim);
            if (d < kd[KL - 1]) {
                bool c[KL];
#pragma unroll
                for (int j = 0; j < KL; ++j) c[j] = d < kd[j];
#pragma unroll
                for (int j = KL - 1; j >= 1; --j) {
                    kd[j] = c[j - 1] ? kd[j - 1] : (c[j] ? d : kd[j]);
                    ki[j] = c[j - 1] ? ki[j - 1] : (c[j] ? r : ki[j]);
                }
                kd[0] = c[0] ? d : kd[0];
                ki[0] = c[0] ? r : ki[0];
            }
        }
#pragma unroll
        for (int j = 0; j < KL; ++j) { sd[j * 256 + tid] = kd[j]; si[j * 256 + tid] = ki[j]; }
        r3dm_syncthreads();
        for (uint32_t s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                // merge the sorted lists of slots tid and tid + s into slot tid (no other thread reads or writes slot tid in this stage)
                uint32_t pa = 0, pb = 0;
                float rd[KL]; uint32_t ri[KL];
#pragma unroll
                for (int j = 0; j < KL; ++j) {                    // pa + pb = j <= KL - 1: both cursors stay inside their lists
                    const float a = sd[pa * 256 + tid], b = sd[pb * 256 + tid + s];
                    const uint32_t x = si[pa * 256 + tid], y = si[pb * 256 + tid + s];
                    const bool tb = lex_less(b, y, a, x);
                    rd[j] = tb ? b : a; ri[j] = tb ? y : x;
                    pa += tb ? 0u : 1u; pb += tb ? 1u : 0u;
                }
#pragma unroll
                for (int j = 0; j < KL; ++j) { sd[j * 256 + tid] = rd[j]; si[j * 256 + tid] = ri[j]; }
            }
            r3dm_syncthreads();
        }
        if (tid < k) {
            P.out_idx[(size_t)q * k + tid] = (int32_t)si[tid * 256];
            P.out_dist[(size_t)q * k + tid] = sd[tid * 256];
        }
        r3dm_syncthreads();
    }
}

hipError_t launch_l2_exact_knn_items(hipStream_t st, const KnnParams& P, uint32_t count, int from_list)
{
    if (count == 0) return hipSuccess;
    if (P.k < 1 || P.k > R3DM_KNN_MAX) return hipErrorInvalidValue;
    const uint32_t grid = count < 16384u ? count : 16384u;
    return dispatch_kl(P.k, [&](auto kl) {
        hipLaunchKernelGGL((l2_exact_knn_items_kernel<decltype(kl)::value>), dim3(grid), dim3(256), 0, st, P, count, from_list);
        return hipGetLastError();
    });
}

// ------------------------------------------------------------------------------------------------
// Hamming k-NN (binary rows of 29..32 / 61..64 bytes in W = 8 / 16 words): the popcount kernel of hamming_knn2_kernel -- each lane
// owns QL query rows in registers, the dataset rows arrive wave-uniformly through the scalar cache -- with a K-list per query on packed
// keys (ham_key): their unsigned order IS the (distance, row) order, so the lists are exact and there is
// neither a bound nor a certificate.  A lane owns whole queries here (no lane halves to merge).
// ------------------------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) uint32_t* knn_cu32p;   // constant address space -> SMEM loads

template <int W, int KL, int QL>
__global__ __launch_bounds__(256)
void hamming_knnk_kernel(const KnnParams P)
{
    const ImgDev* __restrict__ Ip = P.imgs + P.sI;
    const ImgDev* __restrict__ Jp = P.imgs + P.sJ;
    const uint32_t nI = Ip->n, nJ = Jp->n, k = P.k;
    const uint32_t q0 = (blockIdx.x * 256u + threadIdx.x) * QL;
    const uint32_t wave_q0 = (blockIdx.x * 256u + (threadIdx.x & ~63u)) * QL;
    if (wave_q0 >= nJ) return;

    uint32_t qw[QL][W];
#pragma unroll
    for (int u = 0; u < QL; ++u) {
        uint32_t q = q0 + u; if (q >= nJ) q = nJ - 1;
        const uint32_t* src = Jp->bin + (size_t)q * W;
#pragma unroll
        for (int w = 0; w < W; ++w) qw[u][w] = src[w];
    }
    uint32_t kl[QL][KL];
#pragma unroll
    for (int u = 0; u < QL; ++u)
#pragma unroll
        for (int j = 0; j < KL; ++j) kl[u][j] = 0xFFFFFFFFu;

    const knn_cu32p base = (knn_cu32p)(uintptr_t)Ip->bin;
    for (uint32_t r = 0; r < nI; ++r) {
        const knn_cu32p row = base + (size_t)r * W;
        uint32_t a[W];
#pragma unroll
        for (int w = 0; w < W; ++w) a[w] = row[w];
#pragma unroll
        for (int u = 0; u < QL; ++u) {
            uint32_t d = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) d += (uint32_t)__builtin_popcount(qw[u][w] ^ a[w]);
            const uint32_t key = ham_key(d, r);
            if (__builtin_amdgcn_ballot_w64(key < kl[u][KL - 1]) != 0ull) {
#pragma unroll
                for (int j = KL - 1; j >= 1; --j) {               // min(kl[j], max(kl[j - 1], key))  (v_med3_u32)
                    const uint32_t hi = kl[u][j - 1] > key ? kl[u][j - 1] : key;
                    kl[u][j] = kl[u][j] < hi ? kl[u][j] : hi;
                }
                kl[u][0] = kl[u][0] < key ? kl[u][0] : key;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < QL; ++u) {
        const uint32_t q = q0 + u;
        if (q >= nJ) continue;
#pragma unroll
        for (int j = 0; j < KL; ++j)
            if ((uint32_t)j < k) {
                P.out_idx[(size_t)q * k + j] = (int32_t)ham_key_row(kl[u][j]);
                P.out_dist[(size_t)q * k + j] = (float)ham_key_dist(kl[u][j]);
            }
    }
}

template <int W>
static hipError_t launch_hamming_knnk_w(hipStream_t st, const KnnParams& P, uint32_t n_query)
{
    constexpr int QL = 2;
    const uint32_t grid = (n_query + 256u * QL - 1u) / (256u * QL);
    if (grid == 0) return hipSuccess;
    return dispatch_kl(P.k, [&](auto kl) {
        hipLaunchKernelGGL((hamming_knnk_kernel<W, decltype(kl)::value, QL>), dim3(grid), dim3(256), 0, st, P);
        return hipGetLastError();
    });
}

hipError_t launch_hamming_knnk(hipStream_t st, const KnnParams& P, uint32_t words, uint32_t n_query)
{
    if (P.k < 1 || P.k > R3DM_KNN_MAX) return hipErrorInvalidValue;
    return dispatch_words(words, [&](auto w) { return launch_hamming_knnk_w<decltype(w)::value>(st, P, n_query); });
}

}  // namespace r3dm
