// kernels_match_knn16.hip -- exhaustive k-NN (k <= R3DM_KNN_MAX) on the 16-bit tiles, behind r3dm_set_knn_narrow_tiles:
//   l2_knnk_int_kernel<GB, NJ, PF, KL>   integer-valued rows on v_mfma_f32_32x32x16_bf16 (ImgDev::tiled16): exact keys, exact lists
//   l2_knnk_split_kernel<GB, PF, KL>     real-valued rows on v_mfma_f32_32x32x16_f16 (ImgDev::tiledh: hi | lo planes), three MFMAs
//                                        per 16 dimensions; K-lists with a bound, the finish of the f32 K-list kernel with the
//                                        split planes' key scale and slack
// The tile streams are those of l2_knn2_int_kernel / l2_knn2_split_kernel (kernels_match_16bit.hip), the lists and the finish those of
// l2_knnk_mfma_kernel (kernels_match_knn_lists.hpp); the exact scan behind both is l2_exact_knn_items_kernel (kernels_match_knn.hip).
// Which pair runs where is decided by the host alone (api_match.cpp: plan_batch); DESIGN.md 4.18.
//
// Arithmetic contract as everywhere (kernels_match_common.hpp): the f32 4-way unrolled sum of squared differences without FMA, equal
// distances -> lowest dataset row.  This file is compiled with -ffp-contract=off; fused operations are spelled fmaf() / MFMA.
#include "kernels_match_knn_lists.hpp"

namespace r3dm {

// descriptor of a wave-uniform base pointer (readfirstlane: no waterfall loop), 2^31 - 1 bytes of reach
__device__ __forceinline__ __amdgpu_buffer_rsrc_t knn16_rsrc(const void* p)
{
    const uint64_t a = (uint64_t)p;
    return __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a)),
        0, 0x7FFFFFFF, 0x00020000);
}

// ------------------------------------------------------------------------------------------------
// Integer tiles.  The keys ||a||^2 - 2 a.q are exact integers below 2^24 (the exact_pair condition, bf16 = true), so a lane half's
// list needs no bound: topk_push_exact keeps the lexicographic (key, row) top-KL of its rows, and knnk_finish<KL, kKnnKeysExact>
// merges the two halves into the exact top-k.  Nothing is re-scored, certified or scanned.
// One dataset tile: the MFMAs of tile t into `cur` (C operand of the first one = the norms) while the VALU folds tile t - 1 (`prev`)
// into the lists: one wave-wide test per FOUR keys of a list (their minimum against the list's last key), one more per key that is
// reached, and the insert only when some lane needs it.  The minimum is plain fminf in every step: the compiler's MFMA -> VALU hazard
// pass sees the read of the accumulator (kernels_match_16bit.hip, int_tile_step).
// ------------------------------------------------------------------------------------------------
template <int GB, int NJ, int PF, int KL>
__device__ __forceinline__ void knnk_int_tile_step(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                   uint32_t soffA, uint32_t soffN, f32x4 (&abuf)[PF], const f32x16& nrm_cur, f32x16& nrm_next,
                                                   const f32x4 (&bq)[NJ][GB], f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ],
                                                   TopK<KL> (&st)[NJ], uint32_t prev_rowbase)
{
    constexpr int NG = 4 * NJ;                             // (list, quad) groups of four keys per tile
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const f32x4 a = abuf[g % PF];
        abuf[g % PF] = bload16(ra, voffA, soffA + (uint32_t)g * 1024u);
        if (g == (GB > 2 ? 2 : GB - 1)) {                  // next tile's norms, element 4 qd + k = row 8 qd + 4 h + k: the accumulator layout
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const f32x4 v = bload16(rn, voffN, soffN + (uint32_t)qd * 32u);
#pragma unroll
                for (int k = 0; k < 4; ++k) nrm_next[4 * qd + k] = v[k];
            }
        }
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
            cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bq[nj][g]),
                                                              g == 0 ? nrm_cur : cur[nj], 0, 0, 0);
#pragma unroll
        for (int gi = (g * NG) / GB; gi < ((g + 1) * NG) / GB; ++gi) {
            const int nj = gi % NJ, qd = gi / NJ;
            const float p[4] = {prev[nj][4 * qd], prev[nj][4 * qd + 1], prev[nj][4 * qd + 2], prev[nj][4 * qd + 3]};
            const float m = __builtin_fminf(__builtin_fminf(p[0], p[1]), __builtin_fminf(p[2], p[3]));
            if (__builtin_amdgcn_ballot_w64(m < st[nj].d[KL - 1]) != 0ull) {
                const uint32_t rb = prev_rowbase + 8u * (uint32_t)qd;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (__builtin_amdgcn_ballot_w64(p[k] < st[nj].d[KL - 1]) != 0ull) topk_push_exact(st[nj], p[k], rb + (uint32_t)k);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

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
            for (int k = 0; k < 4; ++k) {
                const float lo = __uint_as_float(w[k] << 16) * -2.0f, hi = __uint_as_float(w[k] & 0xFFFF0000u) * -2.0f;
                o[k] = (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xFFFF0000u);
            }
            bq[nj][g] = __builtin_bit_cast(f32x4, o);
        }
    }
    TopK<KL> st[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) topk_init(st[nj]);     // d[KL] stays +inf: these lists carry no bound

    const __amdgpu_buffer_rsrc_t ra = knn16_rsrc(Ip->tiled16), rn = knn16_rsrc(Ip->norms);
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
        knnk_int_tile_step<GB, NJ, PF, KL>(ra, rn, voffA, voffN, t * tileB + PF * 1024u, (t + 1) * 128u, abuf, nrmA, nrmB, bq, accA, accB, st, (t - 1) * 32u + hb);
        knnk_int_tile_step<GB, NJ, PF, KL>(ra, rn, voffA, voffN, (t + 1) * tileB + PF * 1024u, (t + 2) * 128u, abuf, nrmB, nrmA, bq, accB, accA, st, t * 32u + hb);
    }
    if (t < ntI) {
        knnk_int_tile_step<GB, NJ, PF, KL>(ra, rn, voffA, voffN, t * tileB + PF * 1024u, (t + 1) * 128u, abuf, nrmA, nrmB, bq, accA, accB, st, (t - 1) * 32u + hb);
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
    if (P.k <= 4) hipLaunchKernelGGL((l2_knnk_int_kernel<GB, NJ, PF, 4>), dim3(grid), dim3(256), 0, st, P);
    else hipLaunchKernelGGL((l2_knnk_int_kernel<GB, NJ, PF, 8>), dim3(grid), dim3(256), 0, st, P);
    return hipGetLastError();
}

// G = padded dim / 8.  hipErrorNotSupported: no bf16 kernel for this G; hipErrorInvalidValue: k out of range, or a dataset whose bf16
// tiles pass the 2^31-byte reach of the buffer offsets.  Either way the caller keeps the f32 K-list kernel.
// Query tiles per wave: two where the registers allow it (a fragment block then feeds two MFMAs); the 256-dimensional kernel holds
// 64 registers of query fragments per tile and keeps one.
hipError_t launch_l2_knnk_int(hipStream_t st, const KnnParams& P, uint32_t G, uint32_t n_tiles_dataset, uint32_t n_tiles_query)
{
    if (P.k < 1 || P.k > R3DM_KNN_MAX) return hipErrorInvalidValue;
    if (G != 8 && G != 16 && G != 32) return hipErrorNotSupported;
    if ((uint64_t)n_tiles_dataset * (G / 2) * 1024ull + 2ull * kSlackBytes >= 0x7FFFFFFFull) return hipErrorInvalidValue;
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
// (KL + 1)-th key as the half's bound, folded behind the same test-and-skip as knnk_tile_step of the f32 kernel.
// ------------------------------------------------------------------------------------------------
typedef _Float16 knn_f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float knn_pow2f(int k) { return __uint_as_float((uint32_t)(127 + k) << 23); }    // -126 <= k <= 127

template <int GB, int PF, int KL>
__device__ __forceinline__ void knnk_split_tile_step(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                     uint32_t soffA, uint32_t soffN, f32x4 (&ah)[PF], f32x4 (&al)[PF], f32x4 (&nrm)[4], float cscale,
                                                     const f32x4 (&bqh)[GB], const f32x4* __restrict__ bl_lds, f32x16& cur, const f32x16& prev,
                                                     TopK<KL>& st, uint32_t prev_rowbase)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) cur[r] = nrm[r >> 2][r & 3] * cscale;      // ||a||^2 in key units (sI sJ); +inf for padding rows
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const knn_f16x8 a_hi = __builtin_bit_cast(knn_f16x8, ah[g % PF]);
        const knn_f16x8 a_lo = __builtin_bit_cast(knn_f16x8, al[g % PF]);
        ah[g % PF] = bload16(ra, voffA, soffA + (uint32_t)g * 2048u);
        al[g % PF] = bload16(ra, voffA, soffA + (uint32_t)g * 2048u + 1024u);
        if (g == 1) {
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) nrm[qd] = bload16(rn, voffN, soffN + (uint32_t)qd * 32u);
        }
        const f32x4 bl = bl_lds[g * 64];
        cur = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, __builtin_bit_cast(knn_f16x8, bqh[g]), cur, 0, 0, 0);
        cur = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, __builtin_bit_cast(knn_f16x8, bl), cur, 0, 0, 0);
        cur = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, __builtin_bit_cast(knn_f16x8, bqh[g]), cur, 0, 0, 0);
        // this block's share of the previous tile's 16 keys
        bool any = false;
#pragma unroll
        for (int r = (g * 16) / GB; r < ((g + 1) * 16) / GB; ++r) any |= prev[r] < st.d[KL];
        if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
#pragma unroll
            for (int r = (g * 16) / GB; r < ((g + 1) * 16) / GB; ++r)
                if (__builtin_amdgcn_ballot_w64(prev[r] < st.d[KL]) != 0ull)
                    topk_push(st, prev[r], prev_rowbase + (uint32_t)((r & 3) + 8 * (r >> 2)));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

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
    const float cscale = knn_pow2f(kI + kJ);               // key units: sI sJ (||a||^2 - 2 a.q)
    const float key_inv = knn_pow2f(-(kI + kJ));

    // ---- query fragments (B operand), scaled by -2 (exact in f16): hi in registers, lo in this wave's LDS slice
    f32x4* bl_lds = reinterpret_cast<f32x4*>(knn_split_smem) + (size_t)wave * (GB * 64) + lane;
    f32x4 bqh[GB];
    const knn_f16x8 m2 = {(_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f, (_Float16)-2.0f};
    {
        const gf4p src = (gf4p)(const void*)Jp->tiledh + (size_t)qt * (GB * 128) + lane;     // 128 float4 per block (hi | lo)
#pragma unroll
        for (int g = 0; g < GB; ++g) {
            bqh[g] = __builtin_bit_cast(f32x4, __builtin_bit_cast(knn_f16x8, src[g * 128]) * m2);
            bl_lds[g * 64] = __builtin_bit_cast(f32x4, __builtin_bit_cast(knn_f16x8, src[g * 128 + 64]) * m2);
        }
    }
    TopK<KL> st;
    topk_init(st);

    const __amdgpu_buffer_rsrc_t ra = knn16_rsrc(Ip->tiledh), rn = knn16_rsrc(Ip->norms);
    const uint32_t voffA = lane * 16u, voffN = h * 16u;
    constexpr uint32_t tileB = (uint32_t)GB * 2048u;       // bytes per tile (the launcher keeps n_tiles x tileB below 2^31)
    const uint32_t hb = 4u * h;
    f32x4 ah[PF], al[PF];
#pragma unroll
    for (int s = 0; s < PF; ++s) { ah[s] = bload16(ra, voffA, (uint32_t)s * 2048u); al[s] = bload16(ra, voffA, (uint32_t)s * 2048u + 1024u); }
    f32x4 nrm[4];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) nrm[qd] = bload16(rn, voffN, (uint32_t)qd * 32u);
    f32x16 accA, accB;
#pragma unroll
    for (int r = 0; r < 16; ++r) accB[r] = R3DM_INF;       // "tile -1": keys that never enter a list
    uint32_t t = 0;
    for (; t + 1 < ntI; t += 2) {
        knnk_split_tile_step<GB, PF, KL>(ra, rn, voffA, voffN, t * tileB + PF * 2048u, (t + 1) * 128u, ah, al, nrm, cscale, bqh, bl_lds, accA, accB, st, (t - 1) * 32u + hb);
        knnk_split_tile_step<GB, PF, KL>(ra, rn, voffA, voffN, (t + 1) * tileB + PF * 2048u, (t + 2) * 128u, ah, al, nrm, cscale, bqh, bl_lds, accB, accA, st, t * 32u + hb);
    }
    if (t < ntI) {
        knnk_split_tile_step<GB, PF, KL>(ra, rn, voffA, voffN, t * tileB + PF * 2048u, (t + 1) * 128u, ah, al, nrm, cscale, bqh, bl_lds, accA, accB, st, (t - 1) * 32u + hb);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (__builtin_amdgcn_ballot_w64(accA[r] < st.d[KL]) != 0ull) topk_push(st, accA[r], t * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (__builtin_amdgcn_ballot_w64(accB[r] < st.d[KL]) != 0ull) topk_push(st, accB[r], (ntI - 1) * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
    }
    // absolute part of the slack: pieces below the f16 normal range lose up to 2^-25 each (in scaled units), against an operand
    // of magnitude < 2^14 on the other side, two sides, key = -2 a.q  ->  Dpad 2^-9 in key units
    knnk_finish<KL, kKnnKeysSplit>(P, Ip, Jp, st, qt, h, c, (float)(GB * 16), key_inv, (float)(GB * 16) * 0.001953125f * key_inv);
}

template <int GB, int PF>
static hipError_t launch_knnk_split_g(hipStream_t st, const KnnParams& P, uint32_t n_tiles_query)
{
    const uint32_t grid = (n_tiles_query + 3u) / 4u;
    if (grid == 0) return hipSuccess;
    const size_t lds = (size_t)4 * GB * 1024;
    hipError_t e;
    if (P.k <= 4) {
        e = hipFuncSetAttribute((const void*)l2_knnk_split_kernel<GB, PF, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((l2_knnk_split_kernel<GB, PF, 4>), dim3(grid), dim3(256), lds, st, P);
    } else {
        e = hipFuncSetAttribute((const void*)l2_knnk_split_kernel<GB, PF, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((l2_knnk_split_kernel<GB, PF, 8>), dim3(grid), dim3(256), lds, st, P);
    }
    return hipGetLastError();
}

// G = padded dim / 8 (8, 16, 18, 32).  hipErrorInvalidValue: no split kernel for this launch (unknown G, k out of range, or planes
// beyond the 2^31-byte reach of the buffer offsets): the caller keeps the f32 K-list kernel.
hipError_t launch_l2_knnk_split(hipStream_t st, const KnnParams& P, uint32_t G, uint32_t n_tiles_dataset, uint32_t n_tiles_query)
{
    if (P.k < 1 || P.k > R3DM_KNN_MAX) return hipErrorInvalidValue;
    if (G != 8 && G != 16 && G != 18 && G != 32) return hipErrorInvalidValue;
    if ((uint64_t)n_tiles_dataset * (G / 2) * 2048ull + 2ull * kSlackBytes >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    switch (G) {
        case 8:  return launch_knnk_split_g<4, 4>(st, P, n_tiles_query);
        case 16: return launch_knnk_split_g<8, 4>(st, P, n_tiles_query);
        case 18: return launch_knnk_split_g<9, 3>(st, P, n_tiles_query);
        default: return launch_knnk_split_g<16, 4>(st, P, n_tiles_query);
    }
}

}  // namespace r3dm
