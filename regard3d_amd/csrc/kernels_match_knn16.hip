// kernels_match_knn16.hip -- exhaustive k-NN (k <= R3DM_KNN_MAX) on the 16-bit tiles, behind r3dm_set_knn_narrow_tiles:
//   l2_knnk_int_kernel<GB, NJ, PF, KL>   integer-valued rows on v_mfma_f32_32x32x16_bf16 (ImgDev::tiled16): exact keys, exact lists
//   l2_knnk_split_kernel<GB, PF, KL>     real-valued rows on v_mfma_f32_32x32x16_f16 (ImgDev::tiledh: hi | lo planes), three MFMAs
//                                        per 16 dimensions; K-lists with a bound, the finish of the f32 K-list kernel with the
//                                        split planes' key scale and slack
// Where things live: the tile steps (int_tile_step, split_tile_step: one function template each, which l2_knn2_int_kernel and
// l2_knn2_split_kernel instantiate with Top2) and the descriptor in kernels_match_tiles.hpp, the launchers' k -> KL dispatch in
// r3dm_internal.hpp; TopK<KL> and knnk_finish in kernels_match_knn_lists.hpp; the exact scan behind both kernels is l2_exact_knn_items_kernel (kernels_match_knn.hip).
// A kernel body here reads: load the queries, initialise the lists, prologue loads, the ping-pong loop over the shared step, drain, finish.
// Which pair runs where is decided by the host alone (api_match.cpp: plan_batch); DESIGN.md 4.18.
//
// Arithmetic contract as everywhere (kernels_match_common.hpp): the f32 4-way unrolled sum of squared differences without FMA, equal
// distances -> lowest dataset row.  This file is compiled with -ffp-contract=off; fused operations are spelled fmaf() / MFMA.
#include "kernels_match_tiles.hpp"

namespace r3dm {

// ------------------------------------------------------------------------------------------------
// Integer tiles.  The keys ||a||^2 - 2 a.q are exact integers below 2^24 (the exact_pair condition, bf16 = true), so a lane half's
// list needs no bound: topk_push_exact keeps the lexicographic (key, row) top-KL of its rows, and knnk_finish<KL, kKnnKeysExact>
// merges the two halves into the exact top-k.  Nothing is re-scored, certified or scanned.
// One dataset tile is int_tile_step (kernels_match_tiles.hpp), the step of l2_knn2_int_kernel, folding into TopK<KL>.
// ------------------------------------------------------------------------------------------------
// One workgroup = 4 waves, each wave NJ query tiles (32 queries each, pre-scaled by -2 as bf16) in registers as the B fragments; the
// dataset's bf16 tiles stream through as the A fragment (raw_buffer_load_b128, PF-deep rolling window).  Ping-pong accumulators, no
// LDS, no barriers.  Lane (h, c) owns query column c and the rows {(r & 3) + 8 (r >> 2) + 4 h} of a tile, ascending in r.
template <int GB, int NJ, int PF, int KL>
__global__ __launch_bounds__(256, 2)
void l2_knnk_int_kernel(const KnnParams P)
{
    static_assert(GB % PF == 0, "prefetch window must divide the block count");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t h = lane >> 5, c = lane & 31u;
    const ImgDev* __restrict__ Ip = P.imgs + P.sI;
    const ImgDev* __restrict__ Jp = P.imgs + P.sJ;
    const uint32_t ntI = Ip->n_tiles, ntJ = Jp->n_tiles;
    const uint32_t qt0 = (blockIdx.x * 4u + wave) * NJ;
    if (qt0 >= ntJ) return;                                // wave-uniform; no barriers in this kernel

    f32x4 bq[NJ][GB];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        uint32_t qt = qt0 + nj; if (qt >= ntJ) qt = ntJ - 1;          // clamp: knnk_finish discards the tile (its queries are >= n)
        const gf4p src = (gf4p)(const void*)Jp->tiled16 + (size_t)qt * (GB * 64) + lane;
#pragma unroll
        for (int g = 0; g < GB; ++g) {
            const u32x4 w = __builtin_bit_cast(u32x4, src[g * 64]);     // -2 x (integer, |x| <= 256) is a bf16 again
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = bf16x2_times_m2(w[k]);
            bq[nj][g] = __builtin_bit_cast(f32x4, o);
        }
    }
    TopK<KL> st[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) topk_init(st[nj]);     // d[KL] stays +inf: these lists carry no bound

    const __amdgpu_buffer_rsrc_t ra = wave_uniform_rsrc(Ip->tiled16), rn = wave_uniform_rsrc(Ip->norms);
    const uint32_t voffA = lane * 16u, voffN = h * 16u;
    constexpr uint32_t tileB = (uint32_t)GB * 1024u;       // bytes per tile (the launcher keeps n_tiles x tileB below 2^31)
    const uint32_t hb = 4u * h;
    f32x4 abuf[PF];
#pragma unroll
    for (int s = 0; s < PF; ++s) abuf[s] = bload16(ra, voffA, (uint32_t)s * 1024u);
    f32x16 nrmA, nrmB;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const f32x4 v = bload16(rn, voffN, (uint32_t)qd * 32u);
#pragma unroll
        for (int k = 0; k < 4; ++k) nrmA[4 * qd + k] = v[k];
    }
    f32x16 accA[NJ], accB[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int r = 0; r < 16; ++r) accB[nj][r] = R3DM_INF;              // "tile -1": keys that never enter a list
    uint32_t t = 0;
    for (; t + 1 < ntI; t += 2) {
        int_tile_step<GB, NJ, PF, 0>(ra, rn, voffA, voffN, t * tileB + PF * 1024u, (t + 1) * 128u, abuf, nrmA, nrmB, bq, accA, accB, st, (t - 1) * 32u + hb);
        int_tile_step<GB, NJ, PF, 0>(ra, rn, voffA, voffN, (t + 1) * tileB + PF * 1024u, (t + 2) * 128u, abuf, nrmB, nrmA, bq, accB, accA, st, t * 32u + hb);
    }
    if (t < ntI) {
        int_tile_step<GB, NJ, PF, 0>(ra, rn, voffA, voffN, t * tileB + PF * 1024u, (t + 1) * 128u, abuf, nrmA, nrmB, bq, accA, accB, st, (t - 1) * 32u + hb);
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
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) knnk_finish<KL, kKnnKeysExact>(P, Ip, Jp, st[nj], qt0 + nj, h, c, (float)(GB * 16));
}

template <int GB, int NJ, int PF>
static hipError_t launch_knnk_int_g(hipStream_t st, const KnnParams& P, uint32_t n_tiles_query)
{
    const uint32_t grid = (n_tiles_query + 4u * NJ - 1u) / (4u * NJ);
    if (grid == 0) return hipSuccess;
    return dispatch_kl(P.k, [&](auto kl) {
        hipLaunchKernelGGL((l2_knnk_int_kernel<GB, NJ, PF, decltype(kl)::value>), dim3(grid), dim3(256), 0, st, P);
        return hipGetLastError();
    });
}

// G = padded dim / 8.  hipErrorNotSupported: no bf16 kernel for this G; hipErrorInvalidValue: k out of range, or a dataset whose bf16
// tiles pass the 2^31-byte reach of the buffer offsets.  Either way the caller keeps the f32 K-list kernel.
// Query tiles per wave: two where the registers allow it (a fragment block then feeds two MFMAs); the 256-dimensional kernel holds
// 64 registers of query fragments per tile and keeps one.
hipError_t launch_l2_knnk_int(hipStream_t st, const KnnParams& P, uint32_t G, uint32_t n_tiles_dataset, uint32_t n_tiles_query)
{
    if (P.k < 1 || P.k > R3DM_KNN_MAX) return hipErrorInvalidValue;
    if (G != 8 && G != 16 && G != 32) return hipErrorNotSupported;
    if (!tiles_within_reach(n_tiles_dataset, (G / 2) * 1024u)) return hipErrorInvalidValue;
#ifdef R3DM_DEVTOOLS
    if (r3dm_dev_knob("R3DM_KNN_INT_NJ1", 0)) {            // (developer build: A/B of the query tiles per wave)
        if (G == 8) return launch_knnk_int_g<4, 1, 4>(st, P, n_tiles_query);
        if (G == 16) return launch_knnk_int_g<8, 1, 4>(st, P, n_tiles_query);
    }
#endif
    switch (G) {
        case 8:  return launch_knnk_int_g<4, 2, 4>(st, P, n_tiles_query);
        case 16: return launch_knnk_int_g<8, 2, 4>(st, P, n_tiles_query);
        default: return launch_knnk_int_g<16, 1, 4>(st, P, n_tiles_query);
    }
}

// ------------------------------------------------------------------------------------------------
// Split-f16 planes.  x 2^split_k = hi + lo (two f16 pieces), a.q ~ al.qh + ah.ql + ah.qh: three MFMAs per 16 dimensions, keys in
// units of sI sJ with an error of at most err_scale (max||a||^2 + ||q||^2) + Dpad 2^-9 / (sI sJ) (kernels_match_16bit.hip,
// l2_knn2_split_kernel; host: err_scale = (3 Dpad + 36) 2^-22).  One query tile per wave: its hi fragments in registers, its lo
// fragments in the wave's own LDS slice (written once, read by the same wave only: no barrier).  The lists are TopK<KL> with the
// (KL + 1)-th key as the half's bound, folded by split_tile_step (kernels_match_tiles.hpp) behind the test-and-skip of the f32 step.
// ------------------------------------------------------------------------------------------------
template <int GB, int PF, int KL>
__global__ __launch_bounds__(256, 2)
void l2_knnk_split_kernel(const KnnParams P)
{
    static_assert(GB % PF == 0, "prefetch window must divide the block count");
    static_assert(GB >= 2, "the norms of the next tile are fetched in step 1");
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_split_smem[];     // [wave][GB][64 lanes] x 16 B: query lo fragments
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t h = lane >> 5, c = lane & 31u;
    const ImgDev* __restrict__ Ip = P.imgs + P.sI;
    const ImgDev* __restrict__ Jp = P.imgs + P.sJ;
    const uint32_t ntI = Ip->n_tiles, ntJ = Jp->n_tiles;
    const uint32_t qt = blockIdx.x * 4u + wave;
    if (qt >= ntJ) return;                                 // wave-uniform; no workgroup barriers in this kernel
    const int kI = Ip->split_k, kJ = Jp->split_k;
    const float cscale = pow2f(kI + kJ);               // key units: sI sJ (||a||^2 - 2 a.q)
    const float key_inv = pow2f(-(kI + kJ));

    // ---- query fragments (B operand), scaled by -2 (exact in f16): hi in registers, lo in this wave's LDS slice
    f32x4* bl_lds = reinterpret_cast<f32x4*>(knn_split_smem) + (size_t)wave * (GB * 64) + lane;
    f32x4 bqh[1][GB];
    const f16x8 m2 = {(_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f};
    {
        const gf4p src = (gf4p)(const void*)Jp->tiledh + (size_t)qt * (GB * 128) + lane;     // 128 float4 per block (hi | lo)
#pragma unroll
        for (int g = 0; g < GB; ++g) {
            bqh[0][g] = __builtin_bit_cast(f32x4, __builtin_bit_cast(f16x8, src[g * 128]) * m2);
            bl_lds[g * 64] = __builtin_bit_cast(f32x4, __builtin_bit_cast(f16x8, src[g * 128 + 64]) * m2);
        }
    }
    TopK<KL> st[1];
    topk_init(st[0]);

    const __amdgpu_buffer_rsrc_t ra = wave_uniform_rsrc(Ip->tiledh), rn = wave_uniform_rsrc(Ip->norms);
    const uint32_t voffA = lane * 16u, voffN = h * 16u;
    constexpr uint32_t tileB = (uint32_t)GB * 2048u;       // bytes per tile (the launcher keeps n_tiles x tileB below 2^31)
    const uint32_t hb = 4u * h;
    f32x4 ah[PF], al[PF];
#pragma unroll
    for (int s = 0; s < PF; ++s) { ah[s] = bload16(ra, voffA, (uint32_t)s * 2048u); al[s] = bload16(ra, voffA, (uint32_t)s * 2048u + 1024u); }
    f32x4 nrm[4];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) nrm[qd] = bload16(rn, voffN, (uint32_t)qd * 32u);
    f32x16 accA[1], accB[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) accB[0][r] = R3DM_INF;    // "tile -1": keys that never enter a list
    uint32_t t = 0;
    for (; t + 1 < ntI; t += 2) {
        split_tile_step<GB, 1, PF>(ra, rn, voffA, voffN, t * tileB + PF * 2048u, (t + 1) * 128u, ah, al, nrm, cscale, bqh, bl_lds, accA, accB, st, (t - 1) * 32u + hb);
        split_tile_step<GB, 1, PF>(ra, rn, voffA, voffN, (t + 1) * tileB + PF * 2048u, (t + 2) * 128u, ah, al, nrm, cscale, bqh, bl_lds, accB, accA, st, t * 32u + hb);
    }
    if (t < ntI) {
        split_tile_step<GB, 1, PF>(ra, rn, voffA, voffN, t * tileB + PF * 2048u, (t + 1) * 128u, ah, al, nrm, cscale, bqh, bl_lds, accA, accB, st, (t - 1) * 32u + hb);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (__builtin_amdgcn_ballot_w64(accA[0][r] < st[0].d[KL]) != 0ull) topk_push(st[0], accA[0][r], t * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (__builtin_amdgcn_ballot_w64(accB[0][r] < st[0].d[KL]) != 0ull) topk_push(st[0], accB[0][r], (ntI - 1) * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
    }
    // absolute part of the slack: pieces below the f16 normal range lose up to 2^-25 each (in scaled units), against an operand
    // of magnitude < 2^14 on the other side, two sides, key = -2 a.q  ->  Dpad 2^-9 in key units
    knnk_finish<KL, kKnnKeysSplit>(P, Ip, Jp, st[0], qt, h, c, (float)(GB * 16), key_inv, (float)(GB * 16) * 0.001953125f * key_inv);
}

template <int GB, int PF>
static hipError_t launch_knnk_split_g(hipStream_t st, const KnnParams& P, uint32_t n_tiles_query)
{
    const uint32_t grid = (n_tiles_query + 3u) / 4u;
    if (grid == 0) return hipSuccess;
    const size_t lds = (size_t)4 * GB * 1024;
    return dispatch_kl(P.k, [&](auto kl) {
        constexpr int KL = decltype(kl)::value;
        const hipError_t e = hipFuncSetAttribute((const void*)l2_knnk_split_kernel<GB, PF, KL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((l2_knnk_split_kernel<GB, PF, KL>), dim3(grid), dim3(256), lds, st, P);
        return hipGetLastError();
    });
}

// G = padded dim / 8 (8, 16, 18, 32).  hipErrorInvalidValue: no split kernel for this launch (unknown G, k out of range, or planes
// beyond the 2^31-byte reach of the buffer offsets): the caller keeps the f32 K-list kernel.
hipError_t launch_l2_knnk_split(hipStream_t st, const KnnParams& P, uint32_t G, uint32_t n_tiles_dataset, uint32_t n_tiles_query)
{
    if (P.k < 1 || P.k > R3DM_KNN_MAX) return hipErrorInvalidValue;
    if (G != 8 && G != 16 && G != 18 && G != 32) return hipErrorInvalidValue;
    if (!tiles_within_reach(n_tiles_dataset, (G / 2) * 2048u)) return hipErrorInvalidValue;
    switch (G) {
        case 8:  return launch_knnk_split_g<4, 4>(st, P, n_tiles_query);
        case 16: return launch_knnk_split_g<8, 4>(st, P, n_tiles_query);
        case 18: return launch_knnk_split_g<9, 3>(st, P, n_tiles_query);
        default: return launch_knnk_split_g<16, 4>(st, P, n_tiles_query);
    }
}

}  // namespace r3dm
