// kernels_match_knn8.hip -- exhaustive Hamming k-NN (k <= R3DM_KNN_MAX) of binary rows on the i8 MFMA tiles, behind
// r3dm_set_knn_hamming_tiles:
//   hamming_knnk_mfma_kernel<GB, NJ, PF, WPS, KL>   bits as 0 / 1 bytes on v_mfma_i32_32x32x32_i8 (ImgDev::tiled8, biased popcounts in
//                                                   ImgDev::norms: stage_bin8_kernel), the dataset tiles shared by the four waves of a
//                                                   workgroup through LDS-DMA; exact keys, exact K-lists, nothing certified or scanned
// The frame is l2_knn2_int_lds_kernel<..., OPS = 1>'s (kernels_match_hamming.hip): three LDS buffers, one s_waitcnt vmcnt(0) + s_barrier
// per tile, a look-ahead of two tiles, ping-pong accumulators.  Where things live: the tile step (int_tile_step_lds, the function
// template that kernel instantiates with Top2) in kernels_match_tiles.hpp; the launchers' k -> KL dispatch in r3dm_internal.hpp;
// TopK<KL> and topk_push_exact in kernels_match_knn_lists.hpp; lex_less in kernels_match_common.hpp.  The popcount K-list kernel this one is measured against is
// hamming_knnk_kernel (kernels_match_knn.hip).  DESIGN.md 4.23.
//
// Arithmetic: key = popcount(a) - 2 a.q + kHamBias, an exact integer carried as the bits of a normal positive float (the float order
// IS the integer order: |key - kHamBias| <= 1024 steps of one ulp); distance = key - kHamBias + popcount(q); equal distances -> lowest
// dataset row.
#include "kernels_match_tiles.hpp"

namespace r3dm {

// ------------------------------------------------------------------------------------------------
// Finish of one query tile: lanes c and c + 32 hold the lexicographic (key, row) top-KL of the two lane halves' rows.  Every nominee is
// ranked among all 2 KL under (key, row) -- rows are distinct, so the ranks of real entries are too -- and the entries of rank < k are
// written at their rank.  Nothing else decides what is written: padding rows (key 0x7F000000, below the +inf of an empty entry) sit in
// the list of a half with fewer than KL real rows and rank behind every real row; n_dataset >= k (the API's rule) keeps them at rank >= k.
// ------------------------------------------------------------------------------------------------
template <int KL>
__device__ __forceinline__ void hamming_knnk_finish(const KnnParams& P, const ImgDev* __restrict__ Jp, const TopK<KL>& st, uint32_t qt,
                                                    uint32_t c)
{
    const uint32_t k = P.k;
    float pd[KL]; uint32_t pi[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) { pd[j] = __shfl_xor(st.d[j], 32); pi[j] = __shfl_xor(st.i[j], 32); }
    const uint32_t q = qt * 32u + c;
    if (!(qt < Jp->n_tiles && q < Jp->n)) return;
    const int pq = (int)(__float_as_uint(Jp->norms[q]) - kHamBias);                     // popcount of the query row
#pragma unroll
    for (int j = 0; j < KL; ++j) {
        uint32_t r = 0;
#pragma unroll
        for (int m = 0; m < KL; ++m) {
            if (m != j) r += lex_less(st.d[m], st.i[m], st.d[j], st.i[j]) ? 1u : 0u;
            r += lex_less(pd[m], pi[m], st.d[j], st.i[j]) ? 1u : 0u;
        }
        if (r < k) {
            P.out_idx[(size_t)q * k + r] = (int32_t)st.i[j];
            P.out_dist[(size_t)q * k + r] = (float)((int)(__float_as_uint(st.d[j]) - kHamBias) + pq);
        }
    }
}

// One workgroup = 4 waves, each wave NJ query tiles (32 queries each, bytes x -2) in registers as the B fragments.  Lane (h, c) owns
// query column c and the rows {(r & 3) + 8 (r >> 2) + 4 h} of a tile, ascending in r; tiles ascend too, so the strict comparison of
// topk_push_exact keeps the lexicographic (key, row) top-KL of the half.  KL >= k: the first k of the two halves' merge are the answer.
template <int GB, int NJ, int PF, int WPS, int KL>
__global__ __launch_bounds__(256, WPS)
void hamming_knnk_mfma_kernel(const KnnParams P)
{
    static_assert(GB % 4 == 0 && PF <= GB, "a tile is dealt to four waves in whole 1 KiB blocks");
    // ONE LDS array: [3 buffers][GB KiB tile] then [3 buffers][4 waves][256 B norms]
    extern __shared__ __attribute__((aligned(16))) unsigned char knn8_smem[];
    constexpr uint32_t tileB = (uint32_t)GB * 1024u;
    constexpr uint32_t nrm0 = 3u * tileB;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t h = lane >> 5, c = lane & 31u;
    const ImgDev* __restrict__ Ip = P.imgs + P.sI;
    const ImgDev* __restrict__ Jp = P.imgs + P.sJ;
    const uint32_t ntI = Ip->n_tiles, ntJ = Jp->n_tiles;
    const uint32_t qt0 = (blockIdx.x * 4u + wave) * NJ;
    // a wave without query tiles still takes part in the loads and barriers of its workgroup; its results are discarded
    const bool has_queries = qt0 < ntJ;

    f32x4 bq[NJ][GB];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        uint32_t qt = qt0 + nj; if (qt >= ntJ) qt = ntJ - 1;
        const gf4p src = (gf4p)(const void*)Jp->tiled8 + (size_t)qt * (GB * 64) + lane;
#pragma unroll
        for (int g = 0; g < GB; ++g) {
            const u32x4 w = __builtin_bit_cast(u32x4, src[g * 64]);
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = w[k] * 0xFEu;   // bytes 0 / 1 -> 0 / -2 as i8 (no carries between bytes)
            bq[nj][g] = __builtin_bit_cast(f32x4, o);
        }
    }
    TopK<KL> st[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) topk_init(st[nj]);     // d[KL] stays +inf: these lists carry no bound

    // per-lane global sources of this wave's share of a tile: blocks wave * GB/4 + i, and the tile's norms (row l & 31).  The loads run
    // up to two tiles past the dataset (a one-row dataset issues tiles 1 and 2): the slack behind tiled8 and norms holds them.
    const unsigned char* gA = reinterpret_cast<const unsigned char*>(Ip->tiled8) + (size_t)wave * (GB / 4) * 1024u + lane * 16u;
    const unsigned char* gN = reinterpret_cast<const unsigned char*>(Ip->norms) + (lane & 31u) * 4u;
    const uint32_t ldsA = wave * (GB / 4) * 1024u;         // + buffer * tileB + i * 1024   (the DMA adds lane * 16 itself)
    const uint32_t ldsN = nrm0 + wave * 256u;              // + buffer * 1024
    auto issue = [&](uint32_t tile, uint32_t buf) {
#pragma unroll
        for (int i = 0; i < GB / 4; ++i)
            __builtin_amdgcn_global_load_lds((glb_vp)(gA + (size_t)tile * tileB + i * 1024u), (lds_vp)(knn8_smem + buf * tileB + ldsA + i * 1024u), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_vp)(gN + (size_t)tile * 128u), (lds_vp)(knn8_smem + buf * 1024u + ldsN), 4, 0, 0);
    };
    issue(0, 0);
    issue(1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    issue(2, 2);
    const unsigned char* lane_lds = knn8_smem + lane * 16u;                    // fragment of block g of buffer b: + b * tileB + g * 1024
    const unsigned char* lane_nrm = knn8_smem + nrm0 + wave * 256u + h * 16u;  // quad qd of buffer b: + b * 1024 + qd * 32
    f32x4 abuf[PF];
#pragma unroll
    for (int s = 0; s < PF; ++s) abuf[s] = *reinterpret_cast<const f32x4*>(lane_lds + s * 1024);
    f32x16 nrmA, nrmB;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(lane_nrm + qd * 32);
#pragma unroll
        for (int k = 0; k < 4; ++k) nrmA[4 * qd + k] = v[k];
    }
    f32x16 accA[NJ], accB[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int r = 0; r < 16; ++r) accB[nj][r] = R3DM_INF;                  // "tile -1": keys that never enter a list
    const uint32_t hb = 4u * h;
    uint32_t bc = 0, bn = 1;                                                 // buffers of tile t and tile t + 1
    uint32_t t = 0;
    for (; t + 1 < ntI; t += 2) {
        if (t != 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            issue(t + 2, bc == 0 ? 2u : bc - 1u);                            // the buffer tile t - 1 occupied
        }
        int_tile_step_lds<GB, NJ, PF, 0, 1>(lane_lds + bc * tileB, lane_lds + bn * tileB, lane_nrm + bn * 1024u, abuf, nrmA, nrmB, bq, accA, accB, st, (t - 1) * 32u + hb);
        bc = bn; bn = bn == 2 ? 0u : bn + 1u;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        issue(t + 3, bc == 0 ? 2u : bc - 1u);
        int_tile_step_lds<GB, NJ, PF, 0, 1>(lane_lds + bc * tileB, lane_lds + bn * tileB, lane_nrm + bn * 1024u, abuf, nrmB, nrmA, bq, accB, accA, st, t * 32u + hb);
        bc = bn; bn = bn == 2 ? 0u : bn + 1u;
    }
    if (t < ntI) {
        if (t != 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        int_tile_step_lds<GB, NJ, PF, 0, 1>(lane_lds + bc * tileB, lane_lds + bn * tileB, lane_nrm + bn * 1024u, abuf, nrmA, nrmB, bq, accA, accB, st, (t - 1) * 32u + hb);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (__builtin_amdgcn_ballot_w64(accA[nj][r] < st[nj].d[KL - 1]) != 0ull)
                    topk_push_exact(st[nj], accA[nj][r], t * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
    } else {
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (__builtin_amdgcn_ballot_w64(accB[nj][r] < st[nj].d[KL - 1]) != 0ull)
                    topk_push_exact(st[nj], accB[nj][r], (ntI - 1) * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                          // drain the look-ahead loads before ordinary loads follow
    if (has_queries) {
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) hamming_knnk_finish<KL>(P, Jp, st[nj], qt0 + nj, c);
    }
}

template <int GB, int NJ, int PF, int WPS>
static hipError_t launch_hamming_knnk_mfma_g(hipStream_t st, const KnnParams& P, uint32_t n_tiles_query)
{
    const uint32_t grid = (n_tiles_query + 4u * NJ - 1u) / (4u * NJ);
    if (grid == 0) return hipSuccess;
    const size_t lds = 3 * (size_t)GB * 1024 + 3 * 1024;
    return dispatch_kl(P.k, [&](auto kl) {
        hipLaunchKernelGGL((hamming_knnk_mfma_kernel<GB, NJ, PF, WPS, decltype(kl)::value>), dim3(grid), dim3(256), lds, st, P);
        return hipGetLastError();
    });
}

// words = u32 per row: 8 (29 .. 32 bytes, 8 blocks of 32 bits) or 16 (61 .. 64 bytes).  hipErrorInvalidValue: no kernel for this launch
// (k out of range, another row length): the caller keeps the popcount K-list kernel.
// Query tiles per wave: two at 8 words (a fragment block then feeds two MFMAs); at 16 words the query fragments of one tile are 64
// registers and the K-lists of a second would not fit beside them without scratch.
hipError_t launch_hamming_knnk_mfma(hipStream_t st, const KnnParams& P, uint32_t words, uint32_t n_tiles_query)
{
    if (P.k < 1 || P.k > R3DM_KNN_MAX) return hipErrorInvalidValue;
    switch (words) {
        case 8:  return launch_hamming_knnk_mfma_g<8, 2, 4, 2>(st, P, n_tiles_query);
        case 16: return launch_hamming_knnk_mfma_g<16, 1, 4, 2>(st, P, n_tiles_query);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace r3dm
