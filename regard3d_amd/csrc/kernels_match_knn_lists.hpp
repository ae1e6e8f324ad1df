// kernels_match_knn_lists.hpp -- the K-lists of the exhaustive k-NN kernels and their shared tail, included by kernels_match_knn.hip
// (f32 tiles) and kernels_match_knn16.hip (bf16 tiles, split-f16 planes):
//   TopK<KL>, topk_init, topk_push     the KL smallest keys of a lane half with their rows, and the (KL + 1)-th key as its bound
//   topk_push_exact                    the same list on exact keys: no bound is kept (kernels_match_knn16.hip, integer tiles;
//                                      kernels_match_knn8.hip, i8 tiles)
//   topk_push_lex, topk_wave_select    the same list for rows in any order, and the k smallest entries of a wavefront's 64 lists
//                                      (kernels_mrpt.hip: the exact re-rank of the elected rows)
//   knnk_finish<KL, MODE>              merge the two lane halves, re-score, rank, certify the k-th, write or list for the exact scan
// The tile steps that fold keys into these lists, and into Top2, are in kernels_match_tiles.hpp (which includes this header).
#pragma once
#include "kernels_match_common.hpp"

namespace r3dm {

// ------------------------------------------------------------------------------------------------
// K-list of one query column held by one lane HALF (16 of a tile's 32 rows): the KL smallest keys with their rows, ascending, and
// the (KL + 1)-th smallest key d[KL] -- the smallest key this half did NOT nominate, its bound.  The depth is KL per half, not in
// total: all k neighbours of a query may sit in rows of one half.
// ------------------------------------------------------------------------------------------------
template <int KL>
struct TopK {
    float d[KL + 1];
    uint32_t i[KL];
};

template <int KL>
__device__ __forceinline__ void topk_init(TopK<KL>& s)
{
#pragma unroll
    for (int j = 0; j <= KL; ++j) s.d[j] = R3DM_INF;
#pragma unroll
    for (int j = 0; j < KL; ++j) s.i[j] = kNone;
}

// sorted insert, branch-free (v_med3 / v_cndmask): new d[j] = min(d[j], max(d[j - 1], key)).  Runs only behind a wave-wide test.
template <int KL>
__device__ __forceinline__ void topk_push(TopK<KL>& s, float key, uint32_t idx)
{
    bool c[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) c[j] = key < s.d[j];
    s.d[KL] = __builtin_amdgcn_fmed3f(s.d[KL - 1], s.d[KL], key);
#pragma unroll
    for (int j = KL - 1; j >= 1; --j) {                 // downwards: d[j - 1], i[j - 1] are still the old ones
        s.d[j] = __builtin_amdgcn_fmed3f(s.d[j - 1], s.d[j], key);
        const uint32_t t = c[j] ? idx : s.i[j];
        s.i[j] = c[j - 1] ? s.i[j - 1] : t;
    }
    s.d[0] = __builtin_amdgcn_fmed3f(-R3DM_INF, s.d[0], key);
    s.i[0] = c[0] ? idx : s.i[0];
}

// The same insert for EXACT keys (integer tiles): d[KL] is never written and stays +inf -- such a list carries no bound.  A lane sees
// its rows in ascending order and the comparison is strict, so a key equal to a listed one goes behind it: the list is the
// lexicographic (key, row) top-KL of the lane half's rows.
template <int KL>
__device__ __forceinline__ void topk_push_exact(TopK<KL>& s, float key, uint32_t idx)
{
    bool c[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) c[j] = key < s.d[j];
#pragma unroll
    for (int j = KL - 1; j >= 1; --j) {
        s.d[j] = __builtin_amdgcn_fmed3f(s.d[j - 1], s.d[j], key);
        const uint32_t t = c[j] ? idx : s.i[j];
        s.i[j] = c[j - 1] ? s.i[j - 1] : t;
    }
    s.d[0] = __builtin_amdgcn_fmed3f(-R3DM_INF, s.d[0], key);
    s.i[0] = c[0] ? idx : s.i[0];
}

// The same list for rows that arrive in ANY order (kernels_mrpt.hip: the elected rows of a query, in the order their votes came in):
// the insert compares (key, row) pairs, so the list is the lexicographic top-KL whatever the order.  No bound is kept either.
template <int KL>
__device__ __forceinline__ void topk_push_lex(TopK<KL>& s, float key, uint32_t idx)
{
    bool c[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) c[j] = lex_less(key, idx, s.d[j], s.i[j]);
#pragma unroll
    for (int j = KL - 1; j >= 1; --j) {                 // downwards: d[j - 1], i[j - 1] are still the old ones
        const float td = c[j] ? key : s.d[j];
        const uint32_t ti = c[j] ? idx : s.i[j];
        s.d[j] = c[j - 1] ? s.d[j - 1] : td;
        s.i[j] = c[j - 1] ? s.i[j - 1] : ti;
    }
    s.d[0] = c[0] ? key : s.d[0];
    s.i[0] = c[0] ? idx : s.i[0];
}

// The k smallest entries, under (key, row), of the lists the 64 lanes of a wavefront hold (rows distinct across lanes; lists ascending):
// k rounds of a wave-wide minimum over the lists' heads, the owner of a round's minimum moves its list up.  emit(j, key, row) runs in
// every lane with the j-th smallest entry, (+inf, kNone) once the lists are exhausted.  The lists are consumed.
template <int KL, class Emit>
__device__ __forceinline__ void topk_wave_select(TopK<KL>& s, uint32_t k, Emit&& emit)
{
#pragma unroll
    for (int j = 0; j < KL; ++j) {
        if ((uint32_t)j >= k) break;                     // wave-uniform
        float bd = s.d[0]; uint32_t bi = s.i[0];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const float od = __shfl_xor(bd, m); const uint32_t oi = (uint32_t)__shfl_xor((int)bi, m);
            const bool take = lex_less(od, oi, bd, bi);
            bd = take ? od : bd; bi = take ? oi : bi;
        }
        if (bi != kNone && s.i[0] == bi) {
#pragma unroll
            for (int t = 0; t + 1 < KL; ++t) { s.d[t] = s.d[t + 1]; s.i[t] = s.i[t + 1]; }
            s.d[KL - 1] = R3DM_INF; s.i[KL - 1] = kNone;
        }
        emit((uint32_t)j, bd, bi);
    }
}

// ------------------------------------------------------------------------------------------------
// Finish and certificate of one query column (lanes c and c + 32 hold its two halves' lists).
//   1. nominees = the union of both lists (up to 2 KL rows); bound = min of the two halves' (KL + 1)-th keys
//   2. every nominee is re-scored with exact_l2sq on the row-major rows, KL per lane half (on an exact pair -- the integer proof of
//      l2_finish_queries -- key + ||q||^2 IS that distance and nothing is read again)
//   3. the nominees are ranked under (distance, row); the first k are e_1 .. e_k
//   4. certified iff e_k < (bound + ||q||^2) - slack, slack = err_scale (max||a||^2 + ||q||^2), 0 on exact pairs (comparison strict:
//      a k-th neighbour that TIES an un-nominated row needs its index resolved)
//   5. otherwise the query is listed for the exact scan.
// Why a certified answer is the reference's: every un-nominated row has key >= bound (it lost against KL + 1 keys of its own half),
// so its reference distance is >= bound + ||q||^2 - slack > e_k (|key + ||q||^2 - reference distance| <= slack for every row:
// DESIGN.md "Certification").  k nominees are at most e_k away, every other row is strictly farther: the true top-k under
// (distance, row) is a subset of the nominees, and all of those carry their reference distance, so their order -- ties included --
// is the answer.  This is the split path's "second chance" rule (l2_finish_queries) made the only rule.
//
// MODE says where the keys come from:
//   kKnnKeysF32    the f32 tiles (l2_knnk_mfma_kernel): the rule above as it stands
//   kKnnKeysExact  the bf16 tiles (l2_knnk_int_kernel): lists of topk_push_exact.  Under the exact_pair condition -- re-checked here
//                  with the bf16 bound on the magnitudes -- key + ||q||^2 is the reference distance of EVERY row, both lists are
//                  lexicographic, and the first k of their merge are the answer: no bound, no slack, nothing to certify.  A pair
//                  that fails the re-check (the host's predicate admits none) lists every query for the exact scan.
//   kKnnKeysSplit  the split-f16 planes (l2_knnk_split_kernel): keys in units of key_inv^-1 (the two views' powers of two), never
//                  exact; certified iff e_k < (bound key_inv + ||q||^2) - (err_scale (max||a||^2 + ||q||^2) + slack_abs), the
//                  quantities l2_knn2_split_kernel hands to l2_finish_queries.
// ------------------------------------------------------------------------------------------------
enum { kKnnKeysF32 = 0, kKnnKeysExact = 1, kKnnKeysSplit = 2 };

template <int KL, int MODE = kKnnKeysF32>
__device__ __forceinline__ void knnk_finish(const KnnParams& P, const ImgDev* __restrict__ Ip, const ImgDev* __restrict__ Jp,
                                            const TopK<KL>& st, uint32_t qt, uint32_t h, uint32_t c, float dpad,
                                            float key_inv = 1.0f, float slack_abs = 0.0f)
{
    const uint32_t nJ = Jp->n, dim = Ip->dim, k = P.k;
    const float maxnorm = __uint_as_float(Ip->max_norm_bits);
    const float mI = __uint_as_float(Ip->max_abs_bits), mJ = __uint_as_float(Jp->max_abs_bits);
    const uint32_t fl = Ip->not_integer | Jp->not_integer;              // bit 0: non-integer, bit 1: negative elements
    const bool exact_f32 = (fl & 1u) == 0u &&
                           ((fl & 2u) ? dpad * (mI + mJ) * (mI + mJ) < 16777216.0f
                                      : (2.0f * dpad * mI * mJ < 16777216.0f && dpad * mI * mI < 16777216.0f && dpad * mJ * mJ < 16777216.0f));
    // split keys are never exact; the bf16 tiles hold magnitudes up to 256 exactly
    const bool exact_pair = MODE == kKnnKeysSplit ? false : (MODE == kKnnKeysExact ? exact_f32 && mI <= 256.0f && mJ <= 256.0f : exact_f32);
    // (the nominees of exact lists carry key + ||q||^2 whatever the re-check says: a failed re-check discards them)
    const bool keyed = MODE == kKnnKeysExact ? true : exact_pair;
    const uint32_t q = qt * 32u + c;
    const bool valid = q < nJ;
    const float nb = valid ? Jp->norms[q] : 0.0f;
    float e[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) {
        e[j] = R3DM_INF;
        if (valid && st.i[j] != kNone)
            e[j] = keyed ? st.d[j] + nb : exact_l2sq(Ip->rows + (size_t)st.i[j] * dim, Jp->rows + (size_t)q * dim, dim);
    }
    // rank of every own nominee among all 2 KL (rows are distinct: a row belongs to one half; empty entries are (inf, kNone) and
    // rank behind every row)
    float pe[KL]; uint32_t pi[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) { pe[j] = __shfl_xor(e[j], 32); pi[j] = __shfl_xor(st.i[j], 32); }
    uint32_t rank[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) {
        uint32_t r = 0;
#pragma unroll
        for (int m = 0; m < KL; ++m) {
            if (m != j) r += lex_less(e[m], st.i[m], e[j], st.i[j]) ? 1u : 0u;
            r += lex_less(pe[m], pi[m], e[j], st.i[j]) ? 1u : 0u;
        }
        rank[j] = r;
    }
    float mine = R3DM_INF;
#pragma unroll
    for (int j = 0; j < KL; ++j) if (rank[j] == k - 1u && st.i[j] != kNone) mine = e[j];
    const float ek = fminf(mine, __shfl_xor(mine, 32));
    const float bound = MODE == kKnnKeysSplit ? fminf(st.d[KL], __shfl_xor(st.d[KL], 32)) * key_inv : fminf(st.d[KL], __shfl_xor(st.d[KL], 32));
    const float slack = exact_pair ? 0.0f : (MODE == kKnnKeysSplit ? P.err_scale * (maxnorm + nb) + slack_abs : P.err_scale * (maxnorm + nb));
    const bool certified = MODE == kKnnKeysExact ? exact_pair : ek < (bound + nb) - slack;         // (evaluated identically by both lane halves)
    if (!valid) return;
    if (certified) {
#pragma unroll
        for (int j = 0; j < KL; ++j)
            if (rank[j] < k && st.i[j] != kNone) {
                P.out_idx[(size_t)q * k + rank[j]] = (int32_t)st.i[j];
                P.out_dist[(size_t)q * k + rank[j]] = e[j];
            }
    } else if (h == 0) {                                      // lane half 0 lists the query (fb_q holds n_query entries: no overflow)
        P.fb_q[atomicAdd(P.fb_cnt, 1u)] = q;
    }
}

}  // namespace r3dm
