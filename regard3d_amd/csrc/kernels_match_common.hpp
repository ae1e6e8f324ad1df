// kernels_match_common.hpp -- device helpers shared by the matching kernels (kernels_match.hip: f32 tiles; kernels_match_16bit.hip:
// bf16 / f16 nominators; kernels_match_hamming.hip: binary descriptors; kernels_match_exact.hip: exact scans + finalisation;
// kernels_match_mutual.hip, kernels_match_head.hip, kernels_match_knn.hip, kernels_guided.hip: the other scans of every row):
// the reference metric, the (best, runner-up, bound) lists, the buffer load of a fragment, the steps of the exact-scan kernels
//   lex_less, lex_push, top2_lex_merge    the order (distance, row); (best, runner-up) lists kept and merged under it
//   stage_l2sq<D4>                        exact_l2sq's summation order against a row of a fragment-order LDS stage
//   ham_key, ham_key_row, ham_key_dist    the packed key distance << 22 | row of binary rows and its 22-bit row limit
//   wg_compact_rank                       one round of a 256-thread compaction: rank and total through wave_cnt[4], one barrier
// and the shared tail of every L2 tile kernel (merge the lane halves, re-score in the reference arithmetic, certify, ratio test).
// On top of it: kernels_match_knn_lists.hpp (the K-lists and their tail) and kernels_match_tiles.hpp (the tile steps of the MFMA
// nominators, for either kind of list).  The run-time value -> template argument dispatchers of the launchers are in r3dm_internal.hpp.
//
// Arithmetic contract (OpenMVG L2<float>; /root/reference/src/R3DComputeMatches.cpp:437-489): distances are the f32
// 4-way-unrolled sum of squared differences, NO fused multiply-add; equal distances -> lowest dataset row.  Every translation unit
// that includes this header is compiled with -ffp-contract=off; fused operations are spelled fmaf() / MFMA.
#pragma once
#include "r3dm_internal.hpp"

namespace r3dm {

typedef float f32x4  __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
// pointers read out of ImgDev are generic; the hot loops cast them to the global address space so
// the compiler emits global_load (vmcnt only, SGPR base + lane offset) instead of flat_load
typedef const __attribute__((address_space(1))) f32x4* gf4p;
typedef const __attribute__((address_space(1))) float* gf1p;

// ------------------------------------------------------------------------------------------------
// exact squared L2 in the reference's arithmetic (OpenMVG L2<float>): 4-way unrolled, float
// accumulator, ((d0^2 + d1^2) + d2^2) + d3^2 added to the running result, scalar tail, no FMA.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float exact_l2sq(const float* __restrict__ a, const float* __restrict__ b, uint32_t dim)
{
    float result = 0.0f;
    uint32_t k = 0;
    if ((dim & 3u) == 0) {
        const f32x4* a4 = (const f32x4*)a;
        const f32x4* b4 = (const f32x4*)b;
        for (; k < dim; k += 4) {
            const f32x4 x = a4[k >> 2], y = b4[k >> 2];
            const float d0 = x[0] - y[0], d1 = x[1] - y[1], d2 = x[2] - y[2], d3 = x[3] - y[3];
            result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        }
        return result;
    }
    for (; k + 3 < dim; k += 4) {
        const float d0 = a[k] - b[k], d1 = a[k + 1] - b[k + 1], d2 = a[k + 2] - b[k + 2], d3 = a[k + 3] - b[k + 3];
        result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (; k < dim; ++k) { const float d0 = a[k] - b[k]; result += d0 * d0; }
    return result;
}

// ------------------------------------------------------------------------------------------------
// running (best, runner-up, bound) list of one query column held by one lane
// ------------------------------------------------------------------------------------------------
struct Top2 {
    float d0, d1, d2;      // d0 <= d1 <= d2 ; d2 = smallest key NOT nominated (certification bound)
    uint32_t i0, i1;
};

__device__ __forceinline__ void top2_init(Top2& s)
{
    s.d0 = s.d1 = s.d2 = R3DM_INF; s.i0 = s.i1 = kNone;
}

__device__ __forceinline__ void top2_push(Top2& s, float key, uint32_t idx)
{
    // branch-free: locals first so every ?: is a plain select (v_cndmask), never control flow
    const float od0 = s.d0, od1 = s.d1, od2 = s.d2;
    const uint32_t oi0 = s.i0, oi1 = s.i1;
    const bool c0 = key < od0;
    const bool c1 = key < od1;
    const uint32_t t1 = c1 ? idx : oi1;
    s.d2 = __builtin_amdgcn_fmed3f(od1, od2, key);     // min(d2, max(d1, key))
    s.d1 = __builtin_amdgcn_fmed3f(od0, od1, key);     // min(d1, max(d0, key))
    s.d0 = __builtin_amdgcn_fmed3f(-R3DM_INF, od0, key);   // min(d0, key) as one v_med3_f32 (no canonicalising v_max)
    s.i1 = c0 ? oi0 : t1;
    s.i0 = c0 ? idx : oi0;
}

// write the verdict for one query: ratio test, optional 2-NN dump
__device__ __forceinline__ void emit_result(const MatchParams& P, uint32_t pair, uint32_t q,
                                            float ea, uint32_t ia, float eb, uint32_t ib)
{
    const size_t o = (size_t)pair * P.q_stride + q;
    P.nn_idx[o] = (ib != kNone && ea < P.ratio_R * eb) ? ia : kNone;
    if (P.knn_idx) {
        P.knn_idx[2 * o] = (int32_t)ia; P.knn_idx[2 * o + 1] = (int32_t)ib;
        P.knn_dist[2 * o] = ea;         P.knn_dist[2 * o + 1] = eb;
    }
}

// 16-byte buffer load: wave-uniform descriptor + SGPR byte offset + per-lane 32-bit offset -- no 64-bit
// per-lane address registers in the hot loop (the pointer form spilled at 256 VGPRs)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 bload16(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, uint32_t soff)
{
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0));
}

// ------------------------------------------------------------------------------------------------
// The steps the exact-scan kernels share (the exact 2-NN and k-NN scans, the mutual check, the head gate, guided matching, the
// finalisation).  Each carries one rule that makes a result bit-identical to the reference; a kernel that needs the rule calls the step.
// ------------------------------------------------------------------------------------------------
// THE ORDER: (distance, dataset row), the oracle's tie rule -- equal distances -> lowest row.  An empty entry (+inf, kNone) is last.
__device__ __forceinline__ bool lex_less(float da, uint32_t ia, float db, uint32_t ib)
{
    return da < db || (da == db && ia < ib);
}

// push into a (best, runner-up) list kept under that order (Top2::d2 is not used)
__device__ __forceinline__ void lex_push(Top2& s, float key, uint32_t idx)
{
    const float od0 = s.d0, od1 = s.d1;
    const uint32_t oi0 = s.i0, oi1 = s.i1;
    const bool c0 = lex_less(key, idx, od0, oi0);
    const bool c1 = lex_less(key, idx, od1, oi1);
    s.d1 = c0 ? od0 : (c1 ? key : od1);
    s.i1 = c0 ? oi0 : (c1 ? idx : oi1);
    s.d0 = c0 ? key : od0;
    s.i0 = c0 ? idx : oi0;
}

// THE MERGE of the (best, runner-up) of a second list of rows into a first under the order: what a scan over the union of both row
// sets would hold.  Both lists are sorted and hold distinct rows (or empty entries).
__device__ __forceinline__ void top2_lex_merge(Top2& s, float bd0, uint32_t bi0, float bd1, uint32_t bi1)
{
    lex_push(s, bd0, bi0);
    lex_push(s, bd1, bi1);
}

// THE L2 STEP against an LDS stage in fragment order (ImgDev::tiled: float4 chunk k of row r is stage[k * 32 + r]): the distance
// between a row held in registers (v: float4 chunks) and row r of the stage, over d4 = dim / 4 chunks.  The callers' launch
// conditions guarantee dim % 4 == 0: there is no tail here.  One written-out copy of this summation order remains, the only one
// with the scalar tail: l2_head_match_kernel's loop over its row-major stage (kernels_match_head.hip says why).
// Equal to exact_l2sq(row, v, dim) bit for bit: every chunk adds ((e0^2 + e1^2) + e2^2) + e3^2 to the running float in ascending k,
// and -ffp-contract=off keeps the compiler from fusing any of it.  Which operand is subtracted from which does not matter: a - b and
// b - a are exact negatives of each other in IEEE arithmetic, so their squares are the same float.
template <int D4>
__device__ __forceinline__ float stage_l2sq(const f32x4 (&v)[D4], const f32x4* stage, uint32_t r, uint32_t d4)
{
    float result = 0.0f;
#pragma unroll
    for (int k = 0; k < D4; ++k) {
        if (k < (int)d4) {
            const f32x4 a = stage[k * 32 + r];
            const float e0 = a[0] - v[k][0], e1 = a[1] - v[k][1], e2 = a[2] - v[k][2], e3 = a[3] - v[k][3];
            result += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
        }
    }
    return result;
}

// THE PACKED KEY of binary rows: distance << 22 | row.  A view has fewer than 2^22 rows (check_view in api_core.cpp refuses more; so
// do the index and k-NN entry points in api_match.cpp) and a distance is at most 512 bits, so the key fits 32 bits and the UNSIGNED
// order of the keys IS the order (distance, row): min / med3 on keys keep exact lists.  0xFFFFFFFF is the empty entry.
constexpr uint32_t kHamRowBits = 22;
__device__ __forceinline__ uint32_t ham_key(uint32_t dist, uint32_t row) { return (dist << kHamRowBits) | row; }
__device__ __forceinline__ uint32_t ham_key_row(uint32_t key) { return key & ((1u << kHamRowBits) - 1u); }
__device__ __forceinline__ uint32_t ham_key_dist(uint32_t key) { return key >> kHamRowBits; }

// THE COMPACTION ROUND of a 256-thread workgroup (4 waves): every thread brings a `keep` flag; returns the thread's rank among the
// kept threads of the workgroup (thread order) and their number in `total`, through wave_cnt[4] in LDS.  The round contains ONE
// barrier, between the waves' counts and their sum.  The caller puts a second barrier between two rounds (after the writes that use
// the rank): the next round's counts overwrite wave_cnt.  `before_barrier` runs between this wave's count and the barrier: the
// fence of a caller whose kept elements live in global memory (finalize_body).
template <class BeforeBarrier>
__device__ __forceinline__ uint32_t wg_compact_rank(bool keep, uint32_t* wave_cnt, uint32_t& total, BeforeBarrier&& before_barrier)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    const uint32_t before = (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = (uint32_t)__builtin_popcountll(bal);
    before_barrier();
    r3dm_syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) { const uint32_t cw = wave_cnt[w]; if (w < wave) woff += cw; tot += cw; }
    total = tot;
    return woff + before;
}
__device__ __forceinline__ uint32_t wg_compact_rank(bool keep, uint32_t* wave_cnt, uint32_t& total)
{
    return wg_compact_rank(keep, wave_cnt, total, [] {});
}

// whether the MFMA keys of a pair ARE the reference distances (the proof stands in l2_finish_queries, where it is used): both views
// integer-valued and every partial sum below 2^24; bf16 tiles also need |x| <= 256
__device__ __forceinline__ bool l2_pair_is_exact(const ImgDev* __restrict__ Ip, const ImgDev* __restrict__ Jp, float dpad, bool bf16_tiles)
{
    const float mI = __uint_as_float(Ip->max_abs_bits), mJ = __uint_as_float(Jp->max_abs_bits);
    const uint32_t fl = Ip->not_integer | Jp->not_integer;              // bit 0: non-integer, bit 1: negative elements
    return (fl & 1u) == 0u &&
           ((fl & 2u) ? dpad * (mI + mJ) * (mI + mJ) < 16777216.0f
                      : (2.0f * dpad * mI * mJ < 16777216.0f && dpad * mI * mI < 16777216.0f && dpad * mJ * mJ < 16777216.0f)) &&
           (!bf16_tiles || (mI <= 256.0f && mJ <= 256.0f));      // bf16 tiles hold the values exactly
}

// extra relative slack of the pruning kernel's keys over err_scale (l2_finish_queries<PRUNE>): 8 x 2^-24, for three roundings each
// below 2^-24 x 2 (maxnorm + ||q||^2).  The pair-norm filter of l2_knn2_half_kernel carries (err_scale + kPruneKeySlack) (maxnorm + ||q||^2)
// on EVERY pair: its keys are a 64-term f32 dot product of non-negative terms (products of rounded-up roots, never integers) started
// from the stored ||a||^2, off by at most (128 + 65 + 64) u of ||a||^2 + ||q||^2 on the key side and 256 u on the reference's side,
// 513 u <= err_scale = 544 u at D = 128; the 8 u here pay the roundings of the slack, of slack - ||q||^2 and of T (the derivation
// term by term: kernels_match.hip, above the kernel).  The nudge of the roots needs none: it only lowers the bound.
constexpr float kPruneKeySlack = 4.76837158203125e-07f;

// ---- per query: merge the two lane halves, re-score exactly, certify, ratio-test (tail of both L2 kernels).
// dpad = padded descriptor length, bf16_tiles = the keys come from the integer fast path
// LEX: the lists are exact lexicographic (distance, index) top-2 lists without a bound (l2_knn2_int_kernel)
// SPLIT: the keys come from the split-f16 nominator (l2_knn2_split_kernel) in units of key_inv^-1; a query whose merged
//        top-2 cannot be certified gets a second chance with all four nominees of its two lane halves before it is sent to
//        the exact scan
// lane_key_inv (count tiles, l2_knn2_counts_kernel): the keys of query tile nj are in units of lane_key_inv[nj]^-1, a value per QUERY
//        (both lane halves of a column hold the same one)
// PRUNE: the lists come from l2_knn2_half_kernel (or l2_knn2_prune_kernel), which left whole tiles out of them after their pair
//        norms or a prefix of their dimensions;
//        pruned_lb[nj] is this lane half's lower bound of the reference distance of every row it left out (+inf: none), and the
//        keys carry up to three more roundings than l2_tile_step's (prefix norm, suffix norm, their sum)
template <int NJ, bool LEX = false, bool SPLIT = false, bool PRUNE = false>
__device__ __forceinline__ void l2_finish_queries(const MatchParams& P, uint32_t pair, const ImgDev* __restrict__ Ip,
                                                  const ImgDev* __restrict__ Jp, const Top2 (&st)[NJ], uint32_t qt0,
                                                  uint32_t h, uint32_t c, float dpad, bool bf16_tiles,
                                                  float key_inv = 1.0f, float slack_abs = 0.0f, const float* lane_key_inv = nullptr,
                                                  const float* pruned_lb = nullptr)
{
    const uint32_t nI = Ip->n, nJ = Jp->n, ntJ = Jp->n_tiles;
    const float maxnorm = __uint_as_float(Ip->max_norm_bits);
    const uint32_t dim = Ip->dim;
    // Exactness proof for integer-valued descriptors (e.g. SIFT bins 0..255): when every element of
    // both views is an integer and all partial sums stay below 2^24, the MFMA pass (norm init, fma
    // chain, + ||q||^2) and the reference's sum of squared differences are BOTH exact, hence equal:
    // no rounding slack is needed and only true ties with an un-nominated row need the exact scan.
    // Non-negative data: ||a||^2 <= D mI^2 and the running ||a||^2 - 2 sum(a q) stays within [-2 D mI mJ, D mI^2]; the distance
    // itself is at most D max(mI, mJ)^2.  With negative elements the partial sums reach D mI^2 + 2 D mI mJ and the distance
    // D (mI + mJ)^2, where the reference's own sum starts to round: one bound on the latter covers both.
    const bool exact_pair = !SPLIT && l2_pair_is_exact(Ip, Jp, dpad, bf16_tiles);
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        Top2 s = st[nj];
        if constexpr (SPLIT) {
            const float ki = lane_key_inv ? lane_key_inv[nj] : key_inv;                 // positive scale: order unchanged
            s.d0 *= ki; s.d1 *= ki; s.d2 *= ki;
        }
        const Top2 own = s;                              // this lane half's list (rows 8 qd + 4 h + k of every tile)
        // partner half (same query column, the other 16 rows of every tile)
        const float pd0 = __shfl_xor(s.d0, 32), pd1 = __shfl_xor(s.d1, 32), pd2 = __shfl_xor(s.d2, 32);
        const uint32_t pi0 = __shfl_xor(s.i0, 32), pi1 = __shfl_xor(s.i1, 32);
        if constexpr (LEX) {
            lex_push(s, pd0, pi0);
            lex_push(s, pd1, pi1);
            s.d2 = R3DM_INF;                               // nothing un-nominated can tie or beat an exact top-2
        } else {
            top2_push(s, pd0, pi0);
            top2_push(s, pd1, pi1);
            s.d2 = fminf(s.d2, pd2);
        }
        // make both halves agree on the nominated pair (lane c's view)
        const uint32_t ci0 = __shfl(s.i0, (int)c), ci1 = __shfl(s.i1, (int)c);
        const float bound = __shfl(s.d2, (int)c);

        const uint32_t qt = qt0 + nj;
        const uint32_t q = qt * 32u + c;
        const bool valid = (qt < ntJ) && (q < nJ);
        const uint32_t cand = h ? ci1 : ci0;
        const float cd0 = __shfl(s.d0, (int)c), cd1 = __shfl(s.d1, (int)c);     // (both shuffles outside the lane-dependent select)
        const float ck = h ? cd1 : cd0;                                         // MFMA key ||a||^2 - 2 a.b of this lane's nominee
        float e = R3DM_INF;
        if (valid && cand != kNone) {
            // exact pairs (proof above): key + ||q||^2 IS the reference distance, bit for bit -- no need to fetch the two
            // nominated rows again (that re-read was 60 % of the kernel's HBM-side traffic: 3 x 512 B per query).
            // Otherwise re-score in the reference's summation order.
            if (exact_pair) e = ck + Jp->norms[q];
            else e = exact_l2sq(Ip->rows + (size_t)cand * dim, Jp->rows + (size_t)q * dim, dim);
        }
        const float eo = __shfl_xor(e, 32);
        float ea = h ? eo : e, eb = h ? e : eo;          // ea <-> ci0, eb <-> ci1
        uint32_t ia = ci0, ib = ci1;
        if (eb < ea || (eb == ea && ib < ia)) { const float tf = ea; ea = eb; eb = tf; const uint32_t tu = ia; ia = ib; ib = tu; }
        // certification (evaluated identically by both lane halves of a query)
        const float nb = valid ? Jp->norms[q] : 0.0f;
        float slack = exact_pair ? 0.0f : P.err_scale * (maxnorm + nb) + slack_abs;
        if constexpr (PRUNE) { if (!exact_pair) slack += kPruneKeySlack * (maxnorm + nb); }
        const float A3 = bound + nb;                        // distance of the best un-nominated row (exact if exact_pair)
        // certified: every un-nominated row is strictly farther than the runner-up.  With exact
        // arithmetic a runner-up that merely TIES an un-nominated row still fixes the best row (ea < eb)
        // and the runner-up DISTANCE, which is all the ratio test needs; only the raw 2-NN dump
        // (r3dm_knn2) needs the tie's index resolved by the exact scan.
        bool certified = (eb < A3 - slack) || (exact_pair && P.knn_idx == nullptr && ea < eb && eb <= A3);
        if (bf16_tiles && !exact_pair) certified = false;      // bf16 keys of a non-exact pair mean nothing: exact scan
        // PRUNE (match mode only: the launcher sees to P.knn_idx == nullptr and 0 < R < 1).  `certified` so far speaks of the rows the
        // lists have SEEN: (ea, ia), (eb, ib) are their two nearest.  Every row of a pruned tile was left out because its prefix
        // distance, a lower bound of its reference distance d (the reference adds non-negative terms in dimension order: its partial
        // sums only grow), lay strictly above the lane half's threshold T, and T >= fl(R e1) for the runner-up distance e1 the half
        // held at that moment, rounded up and widened by the slack.  Let t1 <= t2 be the true two smallest distances over ALL rows.
        //   * t2 <= eb, and t2 <= e1 of either half at any moment (two seen rows lie no farther): fl(R x) is monotone in x, so
        //     d > T >= fl(R e1) >= fl(R t2) for every pruned row: a pruned row is never a best row that passes the ratio test.
        //   * not ea < fl(R eb): if the true best is a seen row it is ia, and ea >= fl(R eb) >= fl(R t2); if it is a pruned row, the
        //     line above.  No match either way: emit_result says so from (ea, eb).
        //   * ea < fl(R eb) and ea < fl(R PL), PL = the smaller pruned_lb of the two halves: d > PL >= fl(R PL) > ea (R < 1), so
        //     ia is the true best row; the true runner-up is eb or a pruned row, and ea is below fl(R .) of both.  Emit ia.
        //   * ea < fl(R eb) but not ea < fl(R PL): a pruned row may be the best row or spoil the ratio.  Exact scan.
        // An uncertified query keeps its shortcut with PL folded into the lower bound of everything un-nominated.
        // The cascade (l2_knn2_half_kernel) prunes a tile on EITHER of two lower bounds of d, the prefix distance or the pair-norm
        // bound |a|^2 + |b|^2 - 2 sum_k sa_k sb_k less its slack (Cauchy-Schwarz per pair of dimensions: kernels_match.hip).  The
        // argument above uses of a pruned row only d > T for the T its lane half held at that moment, which holds for both, and of
        // pruned_lb only that it is at most every such T: the cascade hands over the smallest T itself.
        float PL = R3DM_INF;
        if constexpr (PRUNE) {
            PL = fminf(pruned_lb[nj], __shfl_xor(pruned_lb[nj], 32));
            if (certified && ea < P.ratio_R * eb && !(ea < P.ratio_R * PL)) certified = false;
        }
        // Match mode only needs the VERDICT of the ratio test.  The two re-scored nominees bound the true runner-up distance from
        // above (d2 <= eb: two rows are no farther than eb) and, with the un-nominated rows' lower bound L = bound + ||q||^2 -
        // slack, the true best distance from below (d1 >= min(ea, L)).  If min(ea, L) >= R eb then d1 >= R d2 whatever the exact
        // top-2 is: the query has no match, exactly as the exact scan would find -- and that is the fate of nearly every
        // uncertifiable query (descriptors without a counterpart sit at almost equal distances from their nearest rows).
        bool no_match = false;
        if (!certified && !exact_pair && !bf16_tiles && P.knn_idx == nullptr && valid && nI >= 2 && ib != kNone) {
            float L = A3 - slack;
            L -= fabsf(L) * 9.5367431640625e-07f;            // 2^-20: the float evaluation of L itself
            if constexpr (PRUNE) L = fminf(L, PL);
            no_match = fminf(ea, L) >= P.ratio_R * eb;
        }
        if constexpr (SPLIT) {
            // second chance: the two lane halves of a query nominated up to four rows between them.  Re-score all four in the
            // reference arithmetic and certify against the smallest key that NONE of them holds (each half's third key):
            // the gap from the runner-up to the fifth-best row is what has to exceed the slack now, not the gap to the third.
            const bool need = valid && nI >= 2 && !certified && !no_match;
            if (__builtin_amdgcn_ballot_w64(need) != 0ull) {
                float f0 = R3DM_INF, f1 = R3DM_INF;
                if (need) {
                    const float* qrow = Jp->rows + (size_t)q * dim;
                    if (own.i0 != kNone) f0 = exact_l2sq(Ip->rows + (size_t)own.i0 * dim, qrow, dim);
                    if (own.i1 != kNone) f1 = exact_l2sq(Ip->rows + (size_t)own.i1 * dim, qrow, dim);
                }
                Top2 m4; top2_init(m4);
                lex_push(m4, f0, own.i0); lex_push(m4, f1, own.i1);
                const float g0 = __shfl_xor(f0, 32), g1 = __shfl_xor(f1, 32);
                const uint32_t j0 = __shfl_xor(own.i0, 32), j1 = __shfl_xor(own.i1, 32);
                lex_push(m4, g0, j0); lex_push(m4, g1, j1);
                const float bound4 = fminf(own.d2, __shfl_xor(own.d2, 32));
                if (need && m4.i1 != kNone && m4.d1 < (bound4 + nb) - slack) {
                    ea = m4.d0; ia = m4.i0; eb = m4.d1; ib = m4.i1; certified = true;
                }
            }
        }
        if (valid && h == 0) {
            if (nI < 2) {
                emit_result(P, pair, q, R3DM_INF, kNone, R3DM_INF, kNone);
            } else if (certified) {
                emit_result(P, pair, q, ea, ia, eb, ib);
            } else if (no_match) {
                P.nn_idx[(size_t)pair * P.q_stride + q] = kNone;
            } else {
                P.nn_idx[(size_t)pair * P.q_stride + q] = kFallback;
                const uint32_t pos = atomicAdd(P.fb_cnt + pair, 1u);
                atomicAdd(P.fb_total, 1u);
                if (pos < kFbPerPair) P.fb_q[(size_t)pair * kFbPerPair + pos] = q;
                else atomicAdd(P.fb_total + 1, 1u);
            }
        }
    }
}

// ---- helpers of the exact-key kernels (bf16 / i8 tiles): keys ARE distances' ranks, lists hold (best, runner-up) only
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ float vmin2(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

__device__ __forceinline__ void tope_push(Top2& s, float key, uint32_t idx)
{
    const float od0 = s.d0, od1 = s.d1;
    const uint32_t oi0 = s.i0, oi1 = s.i1;
    const bool c0 = key < od0;
    const bool c1 = key < od1;
    const uint32_t t1 = c1 ? idx : oi1;
    s.d1 = __builtin_amdgcn_fmed3f(od0, od1, key);
    s.d0 = vmin2(od0, key);
    s.i1 = c0 ? oi0 : t1;
    s.i0 = c0 ? idx : oi0;
}

}  // namespace r3dm
