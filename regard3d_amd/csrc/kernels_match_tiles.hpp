// kernels_match_tiles.hpp -- the tile machinery of the MFMA nominators, written once for the 2-NN kernels (Top2 lists:
// kernels_match.hip, kernels_match_16bit.hip) and the k-NN kernels (TopK<KL> lists: kernels_match_knn.hip, kernels_match_knn16.hip):
//   wave_uniform_rsrc                  the buffer descriptor of a wave-uniform base pointer
//   pow2f, f16x8                       2^k as a float; the f16 MFMA operand type
//   list_bound / list_push             the interface a tile step folds keys through: lists that keep a bound (Top2::d2, TopK::d[KL])
//   list_last / list_push_exact        ... and lists of exact keys without one (integer tiles: Top2::d1, TopK::d[KL - 1])
//   kTestsEachKey, kTestsEachKeyExact  whether a list policy guards every single push with a ballot of its own
//   l2_tile_step                       one dataset tile on the f32 tiles          (v_mfma_f32_32x32x2_f32)
//   l2_prune_tile_prefix / _finish     ... stopped after a prefix of its dimensions when no lane needs the rest (match mode)
//   l2_pairnorm_tile_filter / l2_prune_tile_restart   ... ruled out on its pair norms first; a tile that is not starts over
//   l2_halfnorm_tile_filter / l2_pairnorm_tile_stream ... ruled out on its pair norms in f16 before that (v_mfma_f32_32x32x16_f16)
//   l2_prefix16_tile_stream            ... the restart's prefix test on the rows rounded to f16, in front of the restart
//   tile_key_min                       the minimum of a lane's 16 keys per query tile, a v_min3_f32 tree (the min form of those tile tests)
//   int_tile_step                      ... on the bf16 tiles of integer rows      (v_mfma_f32_32x32x16_bf16)
//   int_tile_step_lds                  ... on bf16 / i8 tiles shared through LDS  (v_mfma_f32_32x32x16_bf16 / v_mfma_i32_32x32x32_i8)
//   split_tile_step                    ... on the split-f16 planes                (3 x v_mfma_f32_32x32x16_f16)
//   bf16x2_times_m2                    -2 x a packed pair of bf16 integers (the query fragments of the integer tiles)
//   workgroup_pair                     the workgroup -> (pair, query block) decode of every 2-NN nominator
//   pair_grid, launch_pair_kernel      host: qb_per_pair, xcd_map, the grid of a 2-NN launch and its bound; the launch itself
//   tiles_within_reach                 host: the 2^31-byte reach of the buffer offsets (dispatch_kl is in r3dm_internal.hpp)
// Every step is templated on the list type and on NJ, the query tiles a wave holds; the K-list kernels that hold one tile keep arrays
// of one.
// What is NOT here, on purpose: the ping-pong loop around the steps (two steps, the odd tail, the drain of the last tile) and the load
// of a wave's query fragments stay written out in every kernel.  Each of them was tried as a function of this header and changed the
// machine code of the kernels that called it; a kernel's bytes decide.  What holds is what was a function before (the
// steps), pure expressions on values (the descriptor, the bf16 repacking) and the workgroup's decode in the very shape it had.
//
// Arithmetic contract as everywhere (kernels_match_common.hpp); every unit that includes this header is compiled with
// -ffp-contract=off, fused operations are spelled fmaf() / MFMA.
#pragma once
#include "kernels_match_knn_lists.hpp"

#include <type_traits>

namespace r3dm {

// descriptor from wave-uniform values only (readfirstlane) so no waterfall loop is emitted; 2^31 - 1 bytes of reach
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_uniform_rsrc(const void* p)
{
    const uint64_t a = (uint64_t)p;
    return __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a)),
        0, 0x7FFFFFFF, 0x00020000);
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float pow2f(int k) { return __uint_as_float((uint32_t)(127 + k) << 23); }    // -126 <= k <= 127

// ------------------------------------------------------------------------------------------------
// What a tile step needs of a list.  Bounded lists (f32 tiles, split planes): a key can change the list only below list_bound -- the
// smallest key the lane half did NOT nominate.  Exact lists (integer tiles): keys are exact and a lane sees its rows in ascending
// order, so the list is the lexicographic (key, row) top of its rows and carries no bound; a key enters only below list_last.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float list_bound(const Top2& s) { return s.d2; }
template <int KL> __device__ __forceinline__ float list_bound(const TopK<KL>& s) { return s.d[KL]; }
__device__ __forceinline__ void list_push(Top2& s, float key, uint32_t idx) { top2_push(s, key, idx); }
template <int KL> __device__ __forceinline__ void list_push(TopK<KL>& s, float key, uint32_t idx) { topk_push(s, key, idx); }

__device__ __forceinline__ float list_last(const Top2& s) { return s.d1; }
template <int KL> __device__ __forceinline__ float list_last(const TopK<KL>& s) { return s.d[KL - 1]; }
__device__ __forceinline__ void list_push_exact(Top2& s, float key, uint32_t idx) { tope_push(s, key, idx); }
template <int KL> __device__ __forceinline__ void list_push_exact(TopK<KL>& s, float key, uint32_t idx) { topk_push_exact(s, key, idx); }

// Does the policy test each key with a ballot of its own before the push?  A K-list insert is 3 KL instructions and always is;
// Top2's 8-instruction push runs unconditionally behind the slice test -- except on the integer tiles up to 128 dimensions, where
// usually ONE of four keys improves (the 16-step body of D = 256 stays with unconditional pushes: the compiler gives up unrolling the
// larger one).  The drain of the last tile, written out in each kernel, tests as the list does on the f32 tiles.
template <class L> inline constexpr bool kTestsEachKey = true;
template <> inline constexpr bool kTestsEachKey<Top2> = false;
template <class L, int GB> inline constexpr bool kTestsEachKeyExact = true;
template <int GB> inline constexpr bool kTestsEachKeyExact<Top2, GB> = GB <= 8;
// The minimum of four accumulator values may take the two-instruction asm form (vmin2 / vmin3) from step 1 on: Top2 on the integer
// tiles, measured; the K-lists keep plain fminf in every step (int_tile_step)
template <class L> inline constexpr bool kQuadMinAsm = false;
template <> inline constexpr bool kQuadMinAsm<Top2> = true;

// ------------------------------------------------------------------------------------------------
// f32 tiles.
// One dataset tile: MFMAs of tile t into `cur`, while the VALU folds the finished accumulators of
// tile t-1 (`prev`) into the running lists -- software pipelining inside the wave, so the
// epilogue issues in the shadow of the 64-cycle MFMAs instead of after them.
// PIPE (developer A/B, tools/ab_l2.py; the product and every K-list kernel run 3): 1 pipelined epilogue | 2 the same with the issue
// order pinned | 3 pipelined + wave-wide test-and-skip | 4 = 1 with raised priority around the MFMAs | 9 ablation without epilogue.
// ------------------------------------------------------------------------------------------------
template <int G, int NJ, int PF, int PIPE, class L>
__device__ __forceinline__ void l2_tile_step(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                             uint32_t soffA, uint32_t soffN, f32x4 (&abuf)[PF], f32x4 (&nrm)[4],
                                             const f32x4 (&bq)[NJ][G], f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ],
                                             L (&st)[NJ], uint32_t prev_rowbase)
{
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int r = 0; r < 16; ++r) cur[nj][r] = nrm[r >> 2][r & 3];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const f32x4 a = abuf[g % PF];
        abuf[g % PF] = bload16(ra, voffA, soffA + (uint32_t)g * 1024u);
        if (g == 2) {   // next tile's norms: early, so the wait at the tile boundary finds them landed
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) nrm[qd] = bload16(rn, voffN, soffN + (uint32_t)qd * 32u);
        }
        if constexpr (PIPE == 4) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], bq[nj][g][cc], cur[nj], 0, 0, 0);
        if constexpr (PIPE == 4) __builtin_amdgcn_s_setprio(0);
        // this group's share of the previous tile's 16 accumulator values per query tile
        if constexpr (PIPE == 9) {
            // ablation (timing only, results meaningless): keep the accumulators alive, skip the epilogue
#pragma unroll
            for (int r = (g * 16) / G; r < ((g + 1) * 16) / G; ++r)
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj) asm volatile("" ::"v"(prev[nj][r]));
        } else if constexpr (PIPE == 3) {
            // test-and-skip: a value can only change a list if it is below that lane's bound; once the
            // lists have warmed up that is rare, so one wave-wide test guards the whole slice (and, where the policy says so, one
            // more each key: the insert then runs only when some lane needs it)
            bool any = false;
#pragma unroll
            for (int r = (g * 16) / G; r < ((g + 1) * 16) / G; ++r)
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj) any |= prev[nj][r] < list_bound(st[nj]);
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
#pragma unroll
                for (int r = (g * 16) / G; r < ((g + 1) * 16) / G; ++r)
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj)
                        if (!kTestsEachKey<L> || __builtin_amdgcn_ballot_w64(prev[nj][r] < list_bound(st[nj])) != 0ull)
                            list_push(st[nj], prev[nj][r], prev_rowbase + (uint32_t)((r & 3) + 8 * (r >> 2)));
            }
        } else {
#pragma unroll
            for (int r = (g * 16) / G; r < ((g + 1) * 16) / G; ++r)
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj)
                    list_push(st[nj], prev[nj][r], prev_rowbase + (uint32_t)((r & 3) + 8 * (r >> 2)));
        }
        if constexpr (PIPE == 2) {
            // issue order inside the step: MFMA, 3 VALU, MFMA, 3 VALU, ... so the epilogue slice hides
            // behind the 64-cycle matrix instructions instead of in front of them
#pragma unroll
            for (int i = 0; i < 4 * NJ; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);   // 3 VALU
            }
        }
        __builtin_amdgcn_sched_barrier(0);                // keep each prefetch / epilogue slice in its own step
    }
}

// ------------------------------------------------------------------------------------------------
// f32 tiles, match mode: the step that stops a tile after GP of its G groups (l2_knn2_prune_kernel; Top2 lists only).
// The accumulators start from the rows' PREFIX norms (|a_P|^2 over the first 8 GP dimensions, ImgDev::norms' second half), so after
// GP groups they hold kp = |a_P|^2 - 2 a_P.b_P, and kp + |b_P|^2 = d_P <= d.  One wave-wide test against the lane's threshold
// `thr` (PruneLane, kernels_match.hip says what it is) decides: no lane objects -> the tile is done (the kernel remembers its rows
// through pl, the smallest threshold it pruned under); else the suffix norms (norms - prefix norms) are added, groups GP .. G-1 run and the keys are those of
// l2_tile_step (for integer-valued pairs the same floats: every sum is exact).
// The epilogue of tile t-1 is spread over the GP prefix groups (prev_live says whether there is one: a pruned tile leaves none).
// The A window: during the prefix it runs on into the NEXT tile's prefix (GP % PF == 0 keeps a group in slot g % PF), so a pruned
// tile costs no load latency; a continuing tile fetches its groups GP .. GP+PF-1 at the decision and waits for them once -- the
// other wave of the SIMD has the matrix pipe meanwhile -- then streams in order into the next tile as l2_tile_step does.
// Two functions, l2_prune_tile_prefix and l2_prune_tile_finish; the second returns whether `cur` holds the keys of a finished tile
// (wave-uniform).
// ------------------------------------------------------------------------------------------------
template <int G, int GP, int NJ, int PF>
__device__ __forceinline__ void l2_prune_tile_prefix(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                     uint32_t soffA, uint32_t soffP, f32x4 (&abuf)[PF], f32x4 (&pnrm)[4],
                                                     const f32x4 (&bq)[NJ][GP], f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ],
                                                     Top2 (&st)[NJ], uint32_t prev_rowbase, bool prev_live)
{
    static_assert(GP > 2 && GP < G && GP % PF == 0 && G % PF == 0, "the window keeps group g in slot g % PF across a pruned tile");
    // soffA: byte offset of this tile's group 0; soffP: of this tile's prefix norms (soffN in the second half: of its norms)
    constexpr uint32_t tileB = (uint32_t)G * 1024u;
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int r = 0; r < 16; ++r) cur[nj][r] = pnrm[r >> 2][r & 3];
#pragma unroll
    for (int g = 0; g < GP; ++g) {
        const f32x4 a = abuf[g % PF];
        abuf[g % PF] = bload16(ra, voffA, soffA + (g + PF < GP ? (uint32_t)(g + PF) * 1024u : tileB + (uint32_t)(g + PF - GP) * 1024u));
        if (g == 2) {   // next tile's prefix norms
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) pnrm[qd] = bload16(rn, voffN, soffP + 128u + (uint32_t)qd * 32u);
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], bq[nj][g][cc], cur[nj], 0, 0, 0);
        if (prev_live) {
            // this group's share of the previous tile's keys: test-and-skip as in l2_tile_step<PIPE 3>
            bool any = false;
#pragma unroll
            for (int r = (g * 16) / GP; r < ((g + 1) * 16) / GP; ++r)
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj) any |= prev[nj][r] < st[nj].d2;
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
#pragma unroll
                for (int r = (g * 16) / GP; r < ((g + 1) * 16) / GP; ++r)
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj)
                        top2_push(st[nj], prev[nj][r], prev_rowbase + (uint32_t)((r & 3) + 8 * (r >> 2)));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the second half of the step: the decision on the prefix keys and, for a tile that goes on, its suffix.  Split from the first so
// that the caller refreshes `thr` between them (the lists are final once the epilogue above has run).
template <int G, int GP, int NJ, int PF>
__device__ __forceinline__ bool l2_prune_tile_finish(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                     uint32_t soffA, uint32_t soffN, uint32_t soffP, f32x4 (&abuf)[PF],
                                                     __amdgpu_buffer_rsrc_t rq, const uint32_t (&soffQ)[NJ], f32x16 (&cur)[NJ],
                                                     const float (&thr)[NJ])
{
    constexpr uint32_t tileB = (uint32_t)G * 1024u;
    // a lane objects when one of its prefix keys is not above its threshold (written so that a NaN key objects)
    bool obj = false;
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int r = 0; r < 16; ++r) obj |= !(cur[nj][r] > thr[nj]);
    if (__builtin_amdgcn_ballot_w64(obj) == 0ull) return false;
    // the tile goes on.  The wave keeps only the PREFIX of its query fragments in registers (the tile loop has no room for more
    // beside the thresholds): the suffix fragments come from the query view's tiles again, soffQ[nj] = the byte offset of query tile
    // nj's group 0, scaled by -2 like the others.  Its groups GP .. GP+PF-1 replace the next tile's first groups in the window (fetched again below, in order)
#pragma unroll
    for (int s = 0; s < PF; ++s) abuf[(GP + s) % PF] = bload16(ra, voffA, soffA + (uint32_t)(GP + s) * 1024u);
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const f32x4 nf = bload16(rn, voffN, soffN + (uint32_t)qd * 32u), np = bload16(rn, voffN, soffP + (uint32_t)qd * 32u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // |a|^2 - |a_P|^2; a padding row (both +inf) keeps its +inf key
            const float sn = np[k] < R3DM_INF ? nf[k] - np[k] : 0.0f;
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) cur[nj][4 * qd + k] += sn;
        }
    }
    f32x4 bqs[NJ][G - GP];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int g = GP; g < G; ++g) bqs[nj][g - GP] = bload16(rq, voffA, soffQ[nj] + (uint32_t)g * 1024u) * -2.0f;
#pragma unroll
    for (int g = GP; g < G; ++g) {
        const f32x4 a = abuf[g % PF];
        abuf[g % PF] = bload16(ra, voffA, soffA + (g + PF < G ? (uint32_t)(g + PF) * 1024u : tileB + (uint32_t)(g + PF - G) * 1024u));
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], bqs[nj][g - GP][cc], cur[nj], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// The minimum of a lane's 16 keys, per query tile, as a tree of v_min3_f32: five over 15 keys, two over their results and the 16th
// key, one v_min_f32 -- 8 VALU instructions three deep, no scalar unit, where 16 compares alternate with 16 s_or.  For the tile tests
// of the min form of l2_knn2_half_kernel, whose keys are never NaN (kernels_match.hip above the kernel: v_min3_f32 returns the
// operand that is no NaN, so a NaN key would be lost).
// Written as inline assembly: fminf() on an MFMA result gets a canonicalising v_max_f32 x, x in front of every input (the compiler
// cannot know the result to be quiet), which doubles the count.  The hazard recogniser does not look into inline assembly, and a
// VALU read of an MFMA result needs wait states; so one key of the LAST query tile passes through an instruction the compiler sees
// (v_max_f32 x, x, the value itself), every first-level instruction names its result as an input, and the matrix pipe retires in
// order: the wait the compiler puts in front of that one instruction covers every read below (int_tile_step does the same with its
// block 0).
// ------------------------------------------------------------------------------------------------
// v_min3_f32 (vmin3, kernels_match_common.hpp) that the compiler may not move in front of `after`
__device__ __forceinline__ float vmin3_after(float a, float b, float c, float after)
{
    float m;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c), "v"(after));
    return m;
}
template <int NJ>
__device__ __forceinline__ void tile_key_min(const f32x16 (&k)[NJ], float (&m)[NJ])
{
    const float first = __builtin_canonicalizef(k[NJ - 1][0]);      // v_max_f32 x, x: the key itself (no key is a NaN)
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        const f32x16& x = k[nj];
        const float t0 = vmin3_after(nj == NJ - 1 ? first : x[0], x[1], x[15], first);
        const float t1 = vmin3_after(x[2], x[3], x[4], first), t2 = vmin3_after(x[5], x[6], x[7], first);
        const float t3 = vmin3_after(x[8], x[9], x[10], first), t4 = vmin3_after(x[11], x[12], x[13], first);
        m[nj] = vmin2(vmin3(t0, t1, t2), vmin3(t3, t4, x[14]));
    }
}

// ------------------------------------------------------------------------------------------------
// f32 tiles, match mode: the pair-norm filter in front of the prefix test (l2_knn2_half_kernel; Top2 lists only).
// The same contraction over the REDUCED rows (the table behind MatchParams::prune_cnt: GR = G / 2 groups of 8 pair norms per tile,
// tiles contiguous), accumulators started from the rows' FULL norms: after GR groups they hold kf = |a|^2 - 2 sum_k sa_k sb_k, and
// kf + |b|^2 <= |a - b|^2 (Cauchy-Schwarz per pair; the proof and the slack: kernels_match.hip above the kernel).  The epilogue of
// tile t-1 is spread over the GR groups as in l2_prune_tile_prefix; the A window simply runs on (reduced tiles follow one another),
// so a filtered tile exposes no load latency.  The caller decides on `cur`.
// ------------------------------------------------------------------------------------------------
template <int GR, int NJ, int PF>
__device__ __forceinline__ void l2_pairnorm_tile_filter(__amdgpu_buffer_rsrc_t rr, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                        uint32_t soffR, uint32_t soffN, f32x4 (&abuf)[PF], f32x4 (&nrm)[4],
                                                        const f32x4 (&bqr)[NJ][GR], f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ],
                                                        Top2 (&st)[NJ], uint32_t prev_rowbase, bool prev_live)
{
    static_assert(GR > 2 && GR % PF == 0, "the window keeps group g in slot g % PF from tile to tile");
    // soffR: byte offset of this tile's reduced group 0; soffN: of the NEXT tile's norms
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
        for (int r = 0; r < 16; ++r) cur[nj][r] = nrm[r >> 2][r & 3];
#pragma unroll
    for (int g = 0; g < GR; ++g) {
        const f32x4 a = abuf[g % PF];
        abuf[g % PF] = bload16(rr, voffA, soffR + (uint32_t)(g + PF) * 1024u);
        if (g == 2) {   // next tile's norms
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) nrm[qd] = bload16(rn, voffN, soffN + (uint32_t)qd * 32u);
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], bqr[nj][g][cc], cur[nj], 0, 0, 0);
        if (prev_live) {
            // this group's share of the previous tile's keys: test-and-skip as in l2_tile_step<PIPE 3>
            bool any = false;
#pragma unroll
            for (int r = (g * 16) / GR; r < ((g + 1) * 16) / GR; ++r)
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj) any |= prev[nj][r] < st[nj].d2;
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
#pragma unroll
                for (int r = (g * 16) / GR; r < ((g + 1) * 16) / GR; ++r)
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj)
                        top2_push(st[nj], prev[nj][r], prev_rowbase + (uint32_t)((r & 3) + 8 * (r >> 2)));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------------------------------------------------------------
// f32 tiles, match mode: the f16 level in front of the pair-norm filter (l2_knn2_half_kernel; Top2 lists only).
// The filter's contraction once more on the pair norms rounded UP to f16 (the second table behind MatchParams::prune_cnt:
// [tile][4 blocks of 16 pair norms][lane half][32 rows][8 f16], 4 KiB per tile, tiles contiguous): four v_mfma_f32_32x32x16_f16 per
// query tile instead of 32 v_mfma_f32_32x32x2_f32, accumulators started from the rows' FULL norms, so they end as
// kh = |a|^2 - 2 sum_k ha_k hb_k <= kf in exact arithmetic (ha >= sa, hb >= sb).  The epilogue of tile t-1 is spread over the four
// blocks; the A window runs on from tile to tile.  The caller decides on `cur`.
//   v_mfma_f32_32x32x16_f16: A lane l = A[i = l&31][k = 8 (l>>5) .. + 7], B lane l = B[k = 8 (l>>5) .. + 7][j = l&31], D as the f32 form.
// ------------------------------------------------------------------------------------------------
// CSTART (the min form of the kernel): every query tile's first MFMA takes the norms as its C operand -- one 16-register tuple, filled
// by the four norm loads -- and the next tile's norms are fetched behind those MFMAs, so no accumulator is started by a copy.  The keys
// are the same floats: C enters the contraction exactly as a started accumulator does.
template <int GH, int NJ, int PF, bool CSTART = false>
__device__ __forceinline__ void l2_halfnorm_tile_filter(__amdgpu_buffer_rsrc_t rh, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                        uint32_t soffH, uint32_t soffN, f32x4 (&abuf)[PF], f32x4 (&nrm)[4],
                                                        const f32x4 (&bqh)[NJ][GH], f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ],
                                                        Top2 (&st)[NJ], uint32_t prev_rowbase, bool prev_live)
{
    static_assert(GH % PF == 0, "the window keeps block g in slot g % PF from tile to tile");
    // soffH: byte offset of this tile's f16 block 0; soffN: of the NEXT tile's norms
    if constexpr (!CSTART) {
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
            for (int r = 0; r < 16; ++r) cur[nj][r] = nrm[r >> 2][r & 3];
    }
#pragma unroll
    for (int g = 0; g < GH; ++g) {
        const f16x8 a = __builtin_bit_cast(f16x8, abuf[g % PF]);
        abuf[g % PF] = bload16(rh, voffA, soffH + (uint32_t)(g + PF) * 1024u);
        if (CSTART && g == 0) {
            const f32x16 n16 = __builtin_shufflevector(__builtin_shufflevector(nrm[0], nrm[1], 0, 1, 2, 3, 4, 5, 6, 7),
                                                       __builtin_shufflevector(nrm[2], nrm[3], 0, 1, 2, 3, 4, 5, 6, 7),
                                                       0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(f16x8, bqh[nj][g]), n16, 0, 0, 0);
            // (the tuple stays live behind the last MFMA, or that one is tied to it and gets a copy; and no norm load moves in front)
            asm volatile("" : : "v"(n16));
            __builtin_amdgcn_sched_barrier(0);
        }
        if (g == 0) {   // next tile's norms: as early as the accumulators' start allows
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) nrm[qd] = bload16(rn, voffN, soffN + (uint32_t)qd * 32u);
        }
        if (!(CSTART && g == 0)) {
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(f16x8, bqh[nj][g]), cur[nj], 0, 0, 0);
        }
        if (prev_live) {
            // this block's share of the previous tile's keys: test-and-skip as in l2_tile_step<PIPE 3>
            bool any = false;
#pragma unroll
            for (int r = (g * 16) / GH; r < ((g + 1) * 16) / GH; ++r)
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj) any |= prev[nj][r] < st[nj].d2;
            if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
#pragma unroll
                for (int r = (g * 16) / GH; r < ((g + 1) * 16) / GH; ++r)
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj)
                        top2_push(st[nj], prev[nj][r], prev_rowbase + (uint32_t)((r & 3) + 8 * (r >> 2)));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The pair-norm filter on a tile the f16 level let through: the MFMAs of l2_pairnorm_tile_filter in the same order on the same
// operands (the keys are the same floats), but nothing of it is in registers when it starts -- the tile's norms, its reduced groups
// and the query view's reduced groups stream through a W-deep window as in l2_prune_tile_restart below.  The f16 level's window and
// norms stay untouched.  The caller decides on `cur`.
template <int GR, int NJ>
__device__ __forceinline__ void l2_pairnorm_tile_stream(__amdgpu_buffer_rsrc_t rr, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                        uint32_t soffR, uint32_t soffN, __amdgpu_buffer_rsrc_t rqr,
                                                        const uint32_t (&soffQR)[NJ], f32x16 (&cur)[NJ])
{
    constexpr int W = 2;
    static_assert(GR % W == 0, "window slots");
    // soffR: byte offset of this tile's reduced group 0; soffN: of THIS tile's norms
    f32x4 wa[W], wb[NJ][W];
#pragma unroll
    for (int s = 0; s < W; ++s) {
        wa[s] = bload16(rr, voffA, soffR + (uint32_t)s * 1024u);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) wb[nj][s] = bload16(rqr, voffA, soffQR[nj] + (uint32_t)s * 1024u);
    }
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const f32x4 nf = bload16(rn, voffN, soffN + (uint32_t)qd * 32u);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) cur[nj][4 * qd + k] = nf[k];
    }
#pragma unroll
    for (int g = 0; g < GR; ++g) {
        const f32x4 a = wa[g % W];
        f32x4 b[NJ];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) b[nj] = wb[nj][g % W] * -2.0f;
        if (g + W < GR) {
            wa[g % W] = bload16(rr, voffA, soffR + (uint32_t)(g + W) * 1024u);
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) wb[nj][g % W] = bload16(rqr, voffA, soffQR[nj] + (uint32_t)(g + W) * 1024u);
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], b[nj][cc], cur[nj], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The restart's prefix test on a tile that is about to enter the restart, on the rows rounded to f16 (the third table behind
// MatchParams::prune_cnt, stage_pairnorm_kernel: [tile][GB = GP / 2 blocks of 16 dimensions][lane half][32 rows][8 f16], 6 KiB per tile,
// tiles contiguous): GB v_mfma_f32_32x32x16_f16 per query tile instead of 4 GP v_mfma_f32_32x32x2_f32, the accumulators started from the
// same stored prefix norms -- through the C operand of each query tile's first MFMA, one 16-register tuple the four norm loads fill, as
// in l2_halfnorm_tile_filter<CSTART>.  Built like l2_pairnorm_tile_stream: nothing of it is in registers when it starts, the dataset
// view's blocks and the query view's blocks (x -2 in f16: exact for every stored finite value, row_to_half) stream through a W-deep
// window.  Level 1's window and norms stay untouched.  The caller decides on `cur`.
template <int GB, int NJ>
__device__ __forceinline__ void l2_prefix16_tile_stream(__amdgpu_buffer_rsrc_t rp, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                        uint32_t soffB, uint32_t soffP, __amdgpu_buffer_rsrc_t rqp,
                                                        const uint32_t (&soffQB)[NJ], f32x16 (&cur)[NJ])
{
    constexpr int W = 2;
    static_assert(GB % W == 0, "window slots");
    // soffB: byte offset of this tile's f16 block 0; soffP: of THIS tile's prefix norms
    f32x4 wa[W], wb[NJ][W];
#pragma unroll
    for (int s = 0; s < W; ++s) {
        wa[s] = bload16(rp, voffA, soffB + (uint32_t)s * 1024u);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) wb[nj][s] = bload16(rqp, voffA, soffQB[nj] + (uint32_t)s * 1024u);
    }
    f32x4 np[4];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) np[qd] = bload16(rn, voffN, soffP + (uint32_t)qd * 32u);
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const f16x8 a = __builtin_bit_cast(f16x8, wa[g % W]);
        f16x8 b[NJ];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) b[nj] = __builtin_bit_cast(f16x8, wb[nj][g % W]) * (_Float16)-2.0f;
        if (g + W < GB) {
            wa[g % W] = bload16(rp, voffA, soffB + (uint32_t)(g + W) * 1024u);
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) wb[nj][g % W] = bload16(rqp, voffA, soffQB[nj] + (uint32_t)(g + W) * 1024u);
        }
        if (g == 0) {
            const f32x16 n16 = __builtin_shufflevector(__builtin_shufflevector(np[0], np[1], 0, 1, 2, 3, 4, 5, 6, 7),
                                                       __builtin_shufflevector(np[2], np[3], 0, 1, 2, 3, 4, 5, 6, 7),
                                                       0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b[nj], n16, 0, 0, 0);
            asm volatile("" : : "v"(n16));                // (the tuple stays live behind the last MFMA: none is tied to it)
        } else {
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b[nj], cur[nj], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// A tile the filter let through, from its group 0: the prefix norms, GP groups, the prefix test against `thr`, then the suffix norms
// and groups GP .. G-1 -- the MFMAs of l2_prune_tile_prefix / _finish in the same order on the same operands, so the keys of a tile
// that finishes are the same floats.  Nothing of it is in registers when it starts (the wave holds the reduced query fragments
// only): dataset and query fragments of all G groups stream through a W-deep window of their own, from the dataset's and the query
// view's tiles; the first W groups' latency is exposed once per such tile -- the other wave of the SIMD has the matrix pipe meanwhile.
// The filter's window (next reduced tile) and norms stay untouched.  Returns whether `cur` holds the keys of a finished tile
// (wave-uniform).  TEST_PREFIX = false (developer ablation): the tile always finishes.
// MIN (the min form of the kernel): the prefix test on tile_key_min's minimum -- the same verdict where no key is a NaN.
template <int G, int GP, int NJ, bool TEST_PREFIX, bool MIN = false>
__device__ __forceinline__ bool l2_prune_tile_restart(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                      uint32_t soffA, uint32_t soffN, uint32_t soffP, __amdgpu_buffer_rsrc_t rq,
                                                      const uint32_t (&soffQ)[NJ], f32x16 (&cur)[NJ], const float (&thr)[NJ])
{
    constexpr int W = 2;
    static_assert(GP > 2 && GP < G && G % W == 0, "window slots");
    f32x4 wa[W], wb[NJ][W];
#pragma unroll
    for (int s = 0; s < W; ++s) {
        wa[s] = bload16(ra, voffA, soffA + (uint32_t)s * 1024u);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) wb[nj][s] = bload16(rq, voffA, soffQ[nj] + (uint32_t)s * 1024u);
    }
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const f32x4 np = bload16(rn, voffN, soffP + (uint32_t)qd * 32u);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) cur[nj][4 * qd + k] = np[k];
    }
    auto group = [&](int g) __attribute__((always_inline)) {
        const f32x4 a = wa[g % W];
        f32x4 b[NJ];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) b[nj] = wb[nj][g % W] * -2.0f;
        if (g + W < G) {
            wa[g % W] = bload16(ra, voffA, soffA + (uint32_t)(g + W) * 1024u);
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) wb[nj][g % W] = bload16(rq, voffA, soffQ[nj] + (uint32_t)(g + W) * 1024u);
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], b[nj][cc], cur[nj], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll
    for (int g = 0; g < GP; ++g) group(g);
    if constexpr (TEST_PREFIX) {
        // a lane objects when one of its prefix keys is not above its threshold (written so that a NaN key objects)
        bool obj = false;
        if constexpr (MIN) {
            float m[NJ];
            tile_key_min<NJ>(cur, m);
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) obj |= !(m[nj] > thr[nj]);
        } else {
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                for (int r = 0; r < 16; ++r) obj |= !(cur[nj][r] > thr[nj]);
        }
        if (__builtin_amdgcn_ballot_w64(obj) == 0ull) return false;
    }
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const f32x4 nf = bload16(rn, voffN, soffN + (uint32_t)qd * 32u), np = bload16(rn, voffN, soffP + (uint32_t)qd * 32u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // |a|^2 - |a_P|^2; a padding row (both +inf) keeps its +inf key
            const float sn = np[k] < R3DM_INF ? nf[k] - np[k] : 0.0f;
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) cur[nj][4 * qd + k] += sn;
        }
    }
#pragma unroll
    for (int g = GP; g < G; ++g) group(g);
    return true;
}

// ------------------------------------------------------------------------------------------------
// integer fast path (r3dm_set_integer_mfma): the same contraction on v_mfma_f32_32x32x16_bf16.
// Views whose descriptors are integers of magnitude <= 256 (SIFT bins) are staged a second time as bf16 tiles
// (ImgDev::tiled16, [tile][16-dim block][lane half][32 rows][8 bf16] -- 16 bytes per lane and step like the f32
// tiles, half as many steps).  Every value is a bf16, every product and partial sum an integer below 2^24, so the f32
// accumulators hold exactly the values of the f32 path and of the reference's sum of squared differences
// (l2_finish_queries re-checks the condition per pair; anything else goes to the exact scan).
// At 32 cycles per MFMA (16x fewer matrix cycles) the VALU side of l2_tile_step -- 10.7 VALU instructions per MFMA:
// accumulator init, one compare per key, 8-instruction pushes into (best, runner-up, bound) lists -- would hold the
// issue port longer than the matrix pipe runs.  Exact keys allow less:
//   * lists hold (best, runner-up) only.  Keys are exact and every lane sees its rows in increasing index order, so
//     strict '<' keeps the lexicographic (distance, index) top-2 of the lane's rows, and a lexicographic merge of the
//     two lane halves IS the exact top-2 -- no certification bound, a third fewer list updates;
//   * one wave-wide test per FOUR keys of a list (v_min3 + v_min + v_cmp instead of four v_cmp);
//   * the accumulators start from the norm vector through the MFMA's C operand (8 v_mov_b64 per tile instead of 32 v_mov).
// Measured (780 pairs of 8192 x 8192 rows): f32 tiles 95.0 ms; this kernel 12.4 ms (12.96 before the per-key tests in the
// update path) (the f32 kernel's structure on bf16
// tiles: 14.97 ms; without any epilogue: 11.4 ms).  The shader clock drops from 2.32 GHz (f32 kernel) to 1.84 GHz under
// the bf16 matrix load (GRBM_GUI_ACTIVE / duration), so 12.4 ms is 56 % of the clocked bf16 peak.  Sharing the dataset
// tiles of a workgroup through LDS (a quarter of the L1 traffic) measured 16.0 ms against 15.0 ms and was dropped.
// The K-lists (l2_knnk_int_kernel) fold through the same step: topk_push_exact keeps the lexicographic (key, row) top-KL of a lane
// half's rows, one wave-wide test per four keys of a list (their minimum against the list's last key), one more per key that is
// reached, and the insert only when some lane needs it.
// ABL (developer ablations, timing only): bit 0 = no epilogue, bit 1 = no tile / norm loads.
// ------------------------------------------------------------------------------------------------
template <int GB, int NJ, int PF, int ABL, class L>
__device__ __forceinline__ void int_tile_step(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                              uint32_t soffA, uint32_t soffN, f32x4 (&abuf)[PF], const f32x16& nrm_cur, f32x16& nrm_next,
                                              const f32x4 (&bq)[NJ][GB], f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ],
                                              L (&st)[NJ], uint32_t prev_rowbase)
{
    constexpr int NG = 4 * NJ;                             // (list, quad) groups of four keys per tile
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const f32x4 a = abuf[g % PF];
        if (ABL < 2) abuf[g % PF] = bload16(ra, voffA, soffA + (uint32_t)g * 1024u);
        if (ABL < 2 && g == (GB > 2 ? 2 : GB - 1)) {   // next tile's norms, element 4 qd + k = row 8 qd + 4 h + k: the accumulator layout
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
            const float p0 = prev[nj][4 * qd], p1 = prev[nj][4 * qd + 1], p2 = prev[nj][4 * qd + 2], p3 = prev[nj][4 * qd + 3];
            if constexpr ((ABL & 1) != 0) {
                asm volatile("" ::"v"(p0), "v"(p1), "v"(p2), "v"(p3));
            } else {
                // Step 0 may follow the previous tile's last MFMAs (the writers of p0..p3) closely: its minimum goes through
                // ordinary fminf so that the compiler's MFMA -> VALU hazard pass sees the read; from step 1 on at least NJ
                // MFMAs and a sched_barrier lie in between and the two-instruction asm form is safe.  (Measured for Top2 only:
                // the K-lists take plain fminf in every step.)
                const float m = (g == 0 || !kQuadMinAsm<L>) ? __builtin_fminf(__builtin_fminf(p0, p1), __builtin_fminf(p2, p3)) : vmin2(vmin3(p0, p1, p2), p3);
                if (__builtin_amdgcn_ballot_w64(m < list_last(st[nj])) != 0ull) {
                    // some lane improves on one of the four keys: usually ONE key does, so test each before its push
                    // (7 instructions for Top2, 3 KL for a K-list) where the policy says so (kTestsEachKeyExact)
                    constexpr bool each = kTestsEachKeyExact<L, GB>;
                    const uint32_t rb = prev_rowbase + 8u * (uint32_t)qd;
                    if (!each || __builtin_amdgcn_ballot_w64(p0 < list_last(st[nj])) != 0ull) list_push_exact(st[nj], p0, rb);
                    if (!each || __builtin_amdgcn_ballot_w64(p1 < list_last(st[nj])) != 0ull) list_push_exact(st[nj], p1, rb + 1u);
                    if (!each || __builtin_amdgcn_ballot_w64(p2 < list_last(st[nj])) != 0ull) list_push_exact(st[nj], p2, rb + 2u);
                    if (!each || __builtin_amdgcn_ballot_w64(p3 < list_last(st[nj])) != 0ull) list_push_exact(st[nj], p3, rb + 3u);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------------------------------------------------------------
// The integer step on dataset tiles SHARED by the four waves of a workgroup through LDS (l2_knn2_int_lds_kernel and
// l2_knn2_int_ring_kernel, kernels_match_hamming.hip, with Top2; hamming_knnk_mfma_kernel, kernels_match_knn8.hip, with TopK<KL>):
// the fragments of tile t come from lds_cur through a PF-deep register window that runs on into lds_nxt, the next tile's norms from
// nrm_nxt; nothing is loaded from global memory here.  The list side is int_tile_step's.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_vp;
typedef const __attribute__((address_space(1))) void* glb_vp;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// OPS 0: bf16 operands (16 dims per block, v_mfma_f32_32x32x16_bf16).  OPS 1: i8 operands holding the BITS of binary
// descriptors as 0 / 1 (32 bits per block, v_mfma_i32_32x32x32_i8): with C = popcount(a) and B = -2 b the accumulator is
// popcount(a) - 2 a.b = Hamming(a, b) - popcount(b), an exact integer.  The accumulators are biased by 0x3F800000 (the bits of
// 1.0f) through the C operand: the int32 key k and the float with the bits k + 0x3F800000 order identically (normal positive
// floats, |k| <= 2048 steps of one ulp), so the float list machinery below runs on them unchanged.
template <int GB, int NJ, int PF, int ABL, int OPS, class L>
__device__ __forceinline__ void int_tile_step_lds(const unsigned char* __restrict__ lds_cur, const unsigned char* __restrict__ lds_nxt,
                                                  const unsigned char* __restrict__ nrm_nxt, f32x4 (&abuf)[PF], const f32x16& nrm_cur,
                                                  f32x16& nrm_next, const f32x4 (&bq)[NJ][GB], f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ],
                                                  L (&st)[NJ], uint32_t prev_rowbase)
{
    constexpr int NG = 4 * NJ;
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const f32x4 a = abuf[g % PF];
        // block g + PF of the tile stream: this tile's, or the first blocks of the next one (landed with this step's barrier)
        abuf[g % PF] = (g + PF < GB) ? *reinterpret_cast<const f32x4*>(lds_cur + (g + PF) * 1024)
                                     : *reinterpret_cast<const f32x4*>(lds_nxt + (g + PF - GB) * 1024);
        if (g == (GB > 2 ? 2 : GB - 1)) {   // next tile's norms, element 4 qd + k = row 8 qd + 4 h + k: the accumulator layout
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(nrm_nxt + qd * 32);
#pragma unroll
                for (int k = 0; k < 4; ++k) nrm_next[4 * qd + k] = v[k];
            }
        }
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) {
            if constexpr (OPS == 0)
                cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bq[nj][g]),
                                                                  g == 0 ? nrm_cur : cur[nj], 0, 0, 0);
            else
                cur[nj] = __builtin_bit_cast(f32x16, __builtin_amdgcn_mfma_i32_32x32x32_i8(
                              __builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, bq[nj][g]),
                              __builtin_bit_cast(i32x16, g == 0 ? nrm_cur : cur[nj]), 0, 0, 0));
        }
#pragma unroll
        for (int gi = (g * NG) / GB; gi < ((g + 1) * NG) / GB; ++gi) {
            const int nj = gi % NJ, qd = gi / NJ;
            const float p0 = prev[nj][4 * qd], p1 = prev[nj][4 * qd + 1], p2 = prev[nj][4 * qd + 2], p3 = prev[nj][4 * qd + 3];
            if constexpr (ABL != 0) {
                asm volatile("" ::"v"(p0), "v"(p1), "v"(p2), "v"(p3));
            } else {
                // (the minimum and the per-key tests: as in int_tile_step)
                const float m = (g == 0 || !kQuadMinAsm<L>) ? __builtin_fminf(__builtin_fminf(p0, p1), __builtin_fminf(p2, p3)) : vmin2(vmin3(p0, p1, p2), p3);
                if (__builtin_amdgcn_ballot_w64(m < list_last(st[nj])) != 0ull) {
                    constexpr bool each = kTestsEachKeyExact<L, GB>;
                    const uint32_t rb = prev_rowbase + 8u * (uint32_t)qd;
                    if (!each || __builtin_amdgcn_ballot_w64(p0 < list_last(st[nj])) != 0ull) list_push_exact(st[nj], p0, rb);
                    if (!each || __builtin_amdgcn_ballot_w64(p1 < list_last(st[nj])) != 0ull) list_push_exact(st[nj], p1, rb + 1u);
                    if (!each || __builtin_amdgcn_ballot_w64(p2 < list_last(st[nj])) != 0ull) list_push_exact(st[nj], p2, rb + 2u);
                    if (!each || __builtin_amdgcn_ballot_w64(p3 < list_last(st[nj])) != 0ull) list_push_exact(st[nj], p3, rb + 3u);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the bias of the i8 tiles' keys (OPS 1): the bits of 1.0f
constexpr uint32_t kHamBias = 0x3F800000u;

// ------------------------------------------------------------------------------------------------
// split-f16 planes (the format and its error bound: kernels_match_16bit.hip, above stage_split_kernel).  x 2^split_k = hi + lo,
// a.q ~ al.qh + ah.ql + ah.qh: three MFMAs per 16 dimensions, keys in units of sI sJ (cscale).  The wave's query hi fragments sit
// in registers (bqh), their lo fragments in its own LDS slice (bl_lds: written once, read by the same wave only).
// ------------------------------------------------------------------------------------------------
template <int GB, int NJ, int PF, class L>
__device__ __forceinline__ void split_tile_step(__amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rn, uint32_t voffA, uint32_t voffN,
                                                uint32_t soffA, uint32_t soffN, f32x4 (&ah)[PF], f32x4 (&al)[PF], f32x4 (&nrm)[4], float cscale,
                                                const f32x4 (&bqh)[NJ][GB], const f32x4* __restrict__ bl_lds, f32x16 (&cur)[NJ],
                                                const f32x16 (&prev)[NJ], L (&st)[NJ], uint32_t prev_rowbase)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = nrm[r >> 2][r & 3] * cscale;       // ||a||^2 in key units (sI sJ); +inf for padding rows
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) cur[nj][r] = v;
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const f16x8 a_hi = __builtin_bit_cast(f16x8, ah[g % PF]);
        const f16x8 a_lo = __builtin_bit_cast(f16x8, al[g % PF]);
        ah[g % PF] = bload16(ra, voffA, soffA + (uint32_t)g * 2048u);
        al[g % PF] = bload16(ra, voffA, soffA + (uint32_t)g * 2048u + 1024u);
        if (g == 1) {
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) nrm[qd] = bload16(rn, voffN, soffN + (uint32_t)qd * 32u);
        }
        f32x4 bl[NJ];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) bl[nj] = bl_lds[(nj * GB + g) * 64];
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
            cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, __builtin_bit_cast(f16x8, bqh[nj][g]), cur[nj], 0, 0, 0);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
            cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, __builtin_bit_cast(f16x8, bl[nj]), cur[nj], 0, 0, 0);
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
            cur[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, __builtin_bit_cast(f16x8, bqh[nj][g]), cur[nj], 0, 0, 0);
        // this block's share of the previous tile's keys: wave-wide test-and-skip, as in l2_tile_step<PIPE 3>
        bool any = false;
#pragma unroll
        for (int r = (g * 16) / GB; r < ((g + 1) * 16) / GB; ++r)
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) any |= prev[nj][r] < list_bound(st[nj]);
        if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
#pragma unroll
            for (int r = (g * 16) / GB; r < ((g + 1) * 16) / GB; ++r)
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj)
                    if (!kTestsEachKey<L> || __builtin_amdgcn_ballot_w64(prev[nj][r] < list_bound(st[nj])) != 0ull)
                        list_push(st[nj], prev[nj][r], prev_rowbase + (uint32_t)((r & 3) + 8 * (r >> 2)));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// -2 x (integer, |x| <= 256) is a bf16 again: both halves of a packed pair
__device__ __forceinline__ uint32_t bf16x2_times_m2(uint32_t w)
{
    const float lo = __uint_as_float(w << 16) * -2.0f, hi = __uint_as_float(w & 0xFFFF0000u) * -2.0f;
    return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xFFFF0000u);
}

// ------------------------------------------------------------------------------------------------
// workgroup -> (pair, query block) of every 2-NN nominator; false: the workgroup has no pair (the whole workgroup returns).
// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2; with xcd_map every workgroup of a pair runs on ONE XCD
// (pair p on XCD p % 8), so image I and the query tiles are pulled into one L2 instead of eight (pairs are sorted by I: an XCD's
// consecutive pairs mostly share their dataset image).  The two branches keep the shape they had when every kernel wrote them out:
// in this shape the kernels' machine code is what it was (profiles/levels_frame_isa.txt); a kernel's bytes decide.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool workgroup_pair(const MatchParams& P, uint32_t& pair, uint32_t& qb)
{
    if (P.xcd_map) {
        const uint32_t xcd = blockIdx.x & 7u, j = blockIdx.x >> 3;
        pair = (j / P.qb_per_pair) * 8u + xcd;
        qb = j % P.qb_per_pair;
        if (pair >= P.n_pairs) return false;
    } else {
        pair = blockIdx.x / P.qb_per_pair;
        qb = blockIdx.x % P.qb_per_pair;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// Grid of a 2-NN launch, the host mirror of workgroup_pair:
// 4 waves x nj query tiles x 32 queries per workgroup; with xcd_map the pair count is rounded up to the 8 XCDs.  Fills P.qb_per_pair
// and P.xcd_map and returns true with the grid to launch; false with `status` = hipSuccess (an empty launch) or hipErrorInvalidValue
// (a grid beyond 2^32 work-items).
// ------------------------------------------------------------------------------------------------
inline bool pair_grid(MatchParams& P, uint32_t max_nj_tiles, uint32_t nj, uint32_t xcd_map, uint32_t& grid, hipError_t& status)
{
    const uint32_t tiles_per_wg = 4u * nj;
    P.qb_per_pair = (max_nj_tiles + tiles_per_wg - 1) / tiles_per_wg;
    P.xcd_map = xcd_map;
    const uint64_t grid64 = (uint64_t)(xcd_map ? (P.n_pairs + 7u) / 8u * 8u : P.n_pairs) * P.qb_per_pair;
    status = grid64 > kMaxBlocksOf256 ? hipErrorInvalidValue : hipSuccess;
    if (grid64 == 0 || grid64 > kMaxBlocksOf256) return false;
    grid = (uint32_t)grid64;
    return true;
}

// One 2-NN launch: `kernel` with nj query tiles per wave and `lds` bytes of dynamic LDS on a copy of the parameters that carries the
// grid's mapping.  xcd_knob: the launch follows R3DM_XCD_MAP (developer build; the product's constant is 1); the others always map.
inline hipError_t launch_pair_kernel(void (*kernel)(MatchParams), uint32_t nj, bool xcd_knob, hipStream_t st, const MatchParams& Pin,
                                     uint32_t max_nj_tiles, size_t lds = 0)
{
    MatchParams P = Pin;
    static const int xcd_map = r3dm_dev_knob("R3DM_XCD_MAP", 1);
    uint32_t grid; hipError_t status;
    if (!pair_grid(P, max_nj_tiles, nj, xcd_knob ? (uint32_t)xcd_map : 1u, grid, status)) return status;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, st, P);
    return hipGetLastError();
}

// the nominators address a dataset through 32-bit buffer offsets: its tiles and both slacks must end below 2^31 - 1 bytes
inline bool tiles_within_reach(uint32_t n_tiles, uint32_t tile_bytes)
{
    return (uint64_t)n_tiles * tile_bytes + 2ull * kSlackBytes < 0x7FFFFFFFull;
}

}  // namespace r3dm
