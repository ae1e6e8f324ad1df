// kernels_match_mutual.hip -- the opt-in mutual nearest-neighbour check (r3dm_set_mutual_matching).  It runs on
// nn_idx[pair][*] after the matcher and its exact scans have finished and before the finalisation: an accepted match (i, j) -- j's
// nearest row of I is i and the ratio test passed -- stays iff j is the nearest row of J to row i under the order (distance, row);
// anything else becomes kNone, so the (i, j) ordering and both de-duplications never see it.
//
// The distance is the reference's (exact_l2sq: 4-way unrolled, scalar tail, no FMA -- symmetric in its operands bit for bit; over
// the tiles stage_l2sq, the same order for lengths without a tail; the popcount Hamming distance for binary rows) and the scan is
// exhaustive over J whatever arm nominated the match, so the result is a deterministic subset of the switch-off result.  Only
// accepted matches are checked: tens to hundreds of rows of I against one view.  The L2 step, the order, the packed key and the
// gather's compaction round are the shared steps of kernels_match_common.hpp.
//
//   l2_mutual_batch_kernel<RATIO, G>   padded lengths with a tensor kernel, dim % 4 == 0: one workgroup per pair, lane = one accepted
//                                      match (its row of I in registers), J's fragment-order f32 tiles streamed through LDS as
//                                      l2_exact_batch_kernel streams I's (row reads are wave-uniform -> LDS broadcast)
//   l2_mutual_items_kernel<RATIO>      any other length: one workgroup per accepted match over the row-major rows
//   hamming_mutual_kernel<RATIO, W>    binary rows of 8 / 16 words: the batch kernel's shape over the word rows, packed integer keys
//
// The symmetric ratio test (r3dm_set_symmetric_ratio; MutualParams::ratio_form != 0) is the same scan keeping TWO minima: a match stays
// iff j is nearest AND f(d1) < R f(d2), d2 = the smallest distance from row i to a row of J other than j -- the forward 2-NN + ratio
// rule with the views swapped.  It is the RATIO instantiation of each kernel: the two differ in what a scan keeps (L2Scan<RATIO>,
// HammingScan<RATIO>), in the items kernel's tree merge and in what the frame does with the answer, and in nothing else.
#include "kernels_match_common.hpp"

namespace r3dm {

// MutualParams::ratio_form -> the RATIO template argument of a launch, as dispatch_g / dispatch_words (r3dm_internal.hpp)
template <class F>
inline hipError_t dispatch_ratio(const MutualParams& P, F&& f)
{
    return P.ratio_form != 0 ? f(std::integral_constant<bool, true>{}) : f(std::integral_constant<bool, false>{});
}

// ------------------------------------------------------------------------------------------------
// the frame of the one-workgroup-per-pair kernels: gather the accepted (i, j) of the pair in query order into `cand`
// (i << 32 | j), 256 per round; best_row(i, j, active) -> the row of J nearest to row i (it is called by ALL 256 threads and may
// synchronise the workgroup); a candidate whose nearest row is not j loses its entry of nn_idx.
// `cand` holds 512 keys: a round starts with fewer than 256 left over and gathers at most 256 more.
// RATIO (the symmetric ratio test): best_row returns a Nearest2 -- the row, its distance d1 and the smallest distance d2 to any OTHER
// row of J.  A candidate that is nearest stays only if reverse_ratio_passes, and never when J has fewer than two rows (no second
// neighbour: the matcher with the views swapped returns nothing).  A third counter holds what the ratio alone removed.
// ------------------------------------------------------------------------------------------------
struct Nearest2 { uint32_t row; float d1, d2; };

// the reverse ratio test, the forward test of the arm that accepted the match operation for operation: one f32 multiply, a strict <,
// no FMA (-ffp-contract=off).  ratio_form 2 is the MRPT arm's, whose forward test runs on the square roots it returns.
__device__ __forceinline__ bool reverse_ratio_passes(const MutualParams& P, float d1, float d2)
{
    return P.ratio_form == 2u ? sqrtf(d1) < P.ratio_R * sqrtf(d2) : d1 < P.ratio_R * d2;
}

template <bool RATIO, class BestRow>
__device__ __forceinline__ void mutual_pair_rounds(const MutualParams& P, uint32_t pair, uint32_t nJ, unsigned long long* cand,
                                                   uint32_t* wave_cnt, BestRow&& best_row)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* nn = P.nn_idx + (size_t)pair * P.q_stride;
    uint32_t held = 0, qpos = 0;                     // block-uniform: keys in cand, first query not gathered yet
    uint32_t checked = 0, dropped = 0;               // per wave, kept by its lane 0
    uint32_t dropped_ratio = 0;                      // (RATIO) ... nearest, and removed by the reverse ratio test
    for (;;) {
        while (held < 256u && qpos < nJ) {
            const uint32_t q = qpos + threadIdx.x;
            const uint32_t v = (q < nJ) ? nn[q] : kNone;
            const bool keep = (v < kFallback);
            uint32_t tot;
            const uint32_t rank = wg_compact_rank(keep, wave_cnt, tot);
            if (keep) cand[held + rank] = ((unsigned long long)v << 32) | q;
            held += tot; qpos += 256u;
            r3dm_syncthreads();
        }
        if (held == 0) break;                        // a pair without an accepted match leaves here, having read nn_idx once
        const uint32_t cnt = held < 256u ? held : 256u;
        const bool active = threadIdx.x < cnt;
        const unsigned long long key = cand[active ? threadIdx.x : 0u];
        const uint32_t i = (uint32_t)(key >> 32), j = (uint32_t)key;
        const auto best = best_row(i, j, active);
        uint32_t bj;
        if constexpr (RATIO) bj = best.row; else bj = best;
        const bool drop = active && bj != j;
        bool drop_ratio = false;
        if constexpr (RATIO) drop_ratio = active && !drop && !(nJ >= 2u && reverse_ratio_passes(P, best.d1, best.d2));
        if (drop || drop_ratio) nn[j] = kNone;       // (j < qpos: the gather never reads this entry again)
        const unsigned long long ba = __ballot(active), bd = __ballot(drop);
        checked += (uint32_t)__builtin_popcountll(ba); dropped += (uint32_t)__builtin_popcountll(bd);
        if constexpr (RATIO) dropped_ratio += (uint32_t)__builtin_popcountll(__ballot(drop_ratio));
        // the keys beyond this round move to the front: read, barrier, write
        r3dm_syncthreads();
        const uint32_t rest = held - cnt;            // < 256
        const unsigned long long moved = (threadIdx.x < rest) ? cand[256u + threadIdx.x] : 0ull;
        r3dm_syncthreads();
        if (threadIdx.x < rest) cand[threadIdx.x] = moved;
        r3dm_syncthreads();
        held = rest;
    }
    if (lane == 0 && checked) {
        atomicAdd(P.counters, (unsigned long long)checked);
        if (dropped) atomicAdd(P.counters + 1, (unsigned long long)dropped);
        if (dropped_ratio) atomicAdd(P.counters + 2, (unsigned long long)dropped_ratio);
    }
}

// ------------------------------------------------------------------------------------------------
// what a scan keeps while the rows of J go by in ASCENDING order, one type per metric, specialised on RATIO by if constexpr.  The
// mutual check keeps the minimum: a strict <, so an equal distance keeps the lower row.  The ratio form keeps two: an equal distance
// never replaces the best and becomes d2 -- a duplicate of row j gives d2 = d1.  When the best row is j, d2 is the minimum over every
// other row; when it is not, the match is gone whatever d2 holds.  result() is what the frame's best_row returns: the row, or a
// Nearest2.
// The states are VALUES: push takes one and returns the next (scan = push(scan, ...)), and nothing takes a state's address.  A
// member function would -- and the compiler then keeps the state in memory until it has inlined the call, which is later than it
// puts the loop counters around it into registers; the kernels that come out of that are longer and, for G = 32, take more registers
// (tools/kernel_isa_diff.py, profiles/mutual_fold_isa.txt).  For the same reason push gets the row as base + offset and adds the two
// where it keeps the row, and the members stand in this order.
// ------------------------------------------------------------------------------------------------
template <bool RATIO> struct L2Scan {
    uint32_t bj = kNone; float d2 = R3DM_INF, bd = R3DM_INF;     // nearest row, (RATIO) second distance, nearest distance
    static __device__ __forceinline__ L2Scan push(L2Scan s, float d, uint32_t base, uint32_t offset = 0)
    {
        if (d < s.bd) { if constexpr (RATIO) s.d2 = s.bd; s.bd = d; s.bj = base + offset; }
        else if constexpr (RATIO) { if (d < s.d2) s.d2 = d; }
        return s;
    }
    static __device__ __forceinline__ auto result(L2Scan s)
    {
        if constexpr (RATIO) return Nearest2{s.bj, s.bd, s.d2}; else return s.bj;
    }
};

// binary rows: the unsigned minimum of the packed keys (ham_key) IS the nearest row under the (distance, row) order.  The ratio form
// keeps the two smallest keys.  Keys of distinct rows are distinct, so when the smallest is row j's the second is the minimum over
// every other row and its distance field is d2 (a duplicate of row j: the same distance, a higher row).  The distances go into the
// test as floats, as the forward test takes them.
template <bool RATIO> struct HammingScan {
    uint32_t best = 0xFFFFFFFFu, second = 0xFFFFFFFFu;           // second: RATIO only
    static __device__ __forceinline__ HammingScan push(HammingScan s, uint32_t key)
    {
        if constexpr (RATIO) {
            const uint32_t loser = s.best < key ? key : s.best;
            s.second = s.second < loser ? s.second : loser;
        }
        s.best = s.best < key ? s.best : key;
        return s;
    }
    static __device__ __forceinline__ auto result(HammingScan s)
    {
        const uint32_t row = s.best == 0xFFFFFFFFu ? kNone : ham_key_row(s.best);
        if constexpr (RATIO) return Nearest2{row, (float)ham_key_dist(s.best), (float)ham_key_dist(s.second)}; else return row;
    }
};

template <bool RATIO, int G>
__global__ __launch_bounds__(256)
void l2_mutual_batch_kernel(const MutualParams P)
{
    constexpr int D4 = G * 2;                        // float4 per (padded) row
    __shared__ f32x4 tile[32 * D4];                  // 32 rows of J x Dpad floats, fragment order: [chunk k][row r]
    __shared__ unsigned long long cand[512];
    __shared__ uint32_t wave_cnt[4];
    const uint32_t pair = blockIdx.x;
    const uint2 pr = P.pairs[pair];
    const ImgDev* __restrict__ Ip = P.imgs + pr.x;
    const ImgDev* __restrict__ Jp = P.imgs + pr.y;
    const uint32_t nJ = Jp->n, d4 = Ip->dim >> 2;    // dim % 4 == 0 guaranteed by the caller
    const gf4p itiles = (gf4p)Ip->tiled, jtiles = (gf4p)Jp->tiled;
    mutual_pair_rounds<RATIO>(P, pair, nJ, cand, wave_cnt, [&](uint32_t i, uint32_t, bool) {
        f32x4 iv[D4];
        const gf4p irow = itiles + (size_t)(i >> 5) * (D4 * 32) + (i & 31u);
#pragma unroll
        for (int k = 0; k < D4; ++k) iv[k] = (k < (int)d4) ? irow[k * 32] : f32x4{0.f, 0.f, 0.f, 0.f};
        L2Scan<RATIO> scan{};
        for (uint32_t t0 = 0; t0 < nJ; t0 += 32) {
            r3dm_syncthreads();                      // every wave has finished with the previous tile
            {
                const gf4p src = jtiles + (size_t)(t0 >> 5) * (D4 * 32);
                for (uint32_t e = threadIdx.x; e < 32u * D4; e += 256) tile[e] = src[e];
            }
            r3dm_syncthreads();
            const uint32_t rows_here = (nJ - t0 < 32u) ? nJ - t0 : 32u;
            for (uint32_t r = 0; r < rows_here; ++r) scan = L2Scan<RATIO>::push(scan, stage_l2sq<D4>(iv, tile, r, d4), t0, r);
        }
        return L2Scan<RATIO>::result(scan);
    });
}

hipError_t launch_l2_mutual_batch(hipStream_t st, const MutualParams& P, uint32_t G)
{
    if (P.n_pairs == 0) return hipSuccess;
    if (P.n_pairs > kMaxBlocksOf256) return hipErrorInvalidValue;
    const dim3 grid(P.n_pairs);
    return dispatch_g(G, [&](auto g) {
        return dispatch_ratio(P, [&](auto ratio) {
            hipLaunchKernelGGL((l2_mutual_batch_kernel<decltype(ratio)::value, decltype(g)::value>), grid, dim3(256), 0, st, P);
            return hipGetLastError();
        });
    });
}

// ------------------------------------------------------------------------------------------------
// rows-based form (lengths without a tensor kernel, lengths with a scalar tail): one workgroup per accepted match, the rows of J
// dealt to its threads, the per-thread bests merged under the (distance, row) order -- the shape of l2_exact_items_kernel.
// The ratio form's tree merges 2-LISTS (best, its row, second distance): the second minimum of a union is the loser's best or the
// winner's second -- it may be the second entry of one thread's list, which a merge of bests alone would lose.  The winner is chosen
// under the (distance, row) order; the row of d2 does not matter.
// ------------------------------------------------------------------------------------------------
template <bool RATIO>
__global__ __launch_bounds__(256)
void l2_mutual_items_kernel(const MutualParams P, uint32_t count)
{
    __shared__ float sd[256];
    __shared__ float s2[256];                        // (RATIO: every use is under if constexpr, so the mutual check has no such array)
    __shared__ uint32_t si[256];
    uint32_t checked = 0, dropped = 0, dropped_ratio = 0;         // kept by thread 0
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {
        const uint32_t pair = it / P.q_stride, j = it % P.q_stride;
        const uint2 pr = P.pairs[pair];
        const ImgDev* __restrict__ Ip = P.imgs + pr.x;
        const ImgDev* __restrict__ Jp = P.imgs + pr.y;
        const uint32_t nJ = Jp->n;
        if (j >= nJ) continue;                                    // block-uniform
        const uint32_t i = P.nn_idx[it];                          // block-uniform: every thread reads it before the barriers below
        if (i >= kFallback) continue;
        const uint32_t dim = Ip->dim;
        const float* iv = Ip->rows + (size_t)i * dim;
        L2Scan<RATIO> scan{};
        for (uint32_t r = threadIdx.x; r < nJ; r += 256) scan = L2Scan<RATIO>::push(scan, exact_l2sq(iv, Jp->rows + (size_t)r * dim, dim), r);
        sd[threadIdx.x] = scan.bd;
        if constexpr (RATIO) s2[threadIdx.x] = scan.d2;
        si[threadIdx.x] = scan.bj;
        r3dm_syncthreads();
        for (uint32_t s = 128; s > 0; s >>= 1) {
            if (threadIdx.x < s) {
                if constexpr (RATIO) {
                    const float a0 = sd[threadIdx.x], a1 = s2[threadIdx.x]; const uint32_t x = si[threadIdx.x];
                    const float b0 = sd[threadIdx.x + s], b1 = s2[threadIdx.x + s]; const uint32_t y = si[threadIdx.x + s];
                    if (lex_less(b0, y, a0, x)) { sd[threadIdx.x] = b0; si[threadIdx.x] = y; s2[threadIdx.x] = a0 < b1 ? a0 : b1; }
                    else s2[threadIdx.x] = b0 < a1 ? b0 : a1;
                } else {
                    const float b = sd[threadIdx.x + s]; const uint32_t y = si[threadIdx.x + s];
                    if (lex_less(b, y, sd[threadIdx.x], si[threadIdx.x])) { sd[threadIdx.x] = b; si[threadIdx.x] = y; }
                }
            }
            r3dm_syncthreads();
        }
        if (threadIdx.x == 0) {
            checked += 1;
            if (si[0] != j) { P.nn_idx[it] = kNone; dropped += 1; }
            else if constexpr (RATIO) {
                if (!(nJ >= 2u && reverse_ratio_passes(P, sd[0], s2[0]))) { P.nn_idx[it] = kNone; dropped_ratio += 1; }
            }
        }
        r3dm_syncthreads();
    }
    if (threadIdx.x == 0 && checked) {
        atomicAdd(P.counters, (unsigned long long)checked);
        if (dropped) atomicAdd(P.counters + 1, (unsigned long long)dropped);
        if (dropped_ratio) atomicAdd(P.counters + 2, (unsigned long long)dropped_ratio);
    }
}

hipError_t launch_l2_mutual_items(hipStream_t st, const MutualParams& P, uint32_t count)
{
    if (count == 0) return hipSuccess;
    const uint32_t grid = count < 16384u ? count : 16384u;
    return dispatch_ratio(P, [&](auto ratio) {
        hipLaunchKernelGGL(l2_mutual_items_kernel<decltype(ratio)::value>, dim3(grid), dim3(256), 0, st, P, count);
        return hipGetLastError();
    });
}

// ------------------------------------------------------------------------------------------------
// binary rows (ImgDev::bin: row-major u32 [n][W]): lane = one accepted match, its row of I in registers, 32 rows of J per LDS stage
// ------------------------------------------------------------------------------------------------
template <bool RATIO, int W>
__global__ __launch_bounds__(256)
void hamming_mutual_kernel(const MutualParams P)
{
    __shared__ uint32_t tile[32 * W];
    __shared__ unsigned long long cand[512];
    __shared__ uint32_t wave_cnt[4];
    const uint32_t pair = blockIdx.x;
    const uint2 pr = P.pairs[pair];
    const ImgDev* __restrict__ Ip = P.imgs + pr.x;
    const ImgDev* __restrict__ Jp = P.imgs + pr.y;
    const uint32_t nJ = Jp->n;
    const uint32_t* __restrict__ ibin = Ip->bin;
    const uint32_t* __restrict__ jbin = Jp->bin;
    mutual_pair_rounds<RATIO>(P, pair, nJ, cand, wave_cnt, [&](uint32_t i, uint32_t, bool) {
        uint32_t a[W];
#pragma unroll
        for (int w = 0; w < W; ++w) a[w] = ibin[(size_t)i * W + w];
        HammingScan<RATIO> scan{};
        for (uint32_t t0 = 0; t0 < nJ; t0 += 32) {
            r3dm_syncthreads();
            for (uint32_t e = threadIdx.x; e < 32u * W; e += 256)
                tile[e] = (t0 + e / W < nJ) ? jbin[(size_t)t0 * W + e] : 0u;
            r3dm_syncthreads();
            const uint32_t rows_here = (nJ - t0 < 32u) ? nJ - t0 : 32u;
            for (uint32_t r = 0; r < rows_here; ++r) {
                uint32_t d = 0;
#pragma unroll
                for (int w = 0; w < W; ++w) d += (uint32_t)__builtin_popcount(a[w] ^ tile[r * W + w]);
                scan = HammingScan<RATIO>::push(scan, ham_key(d, t0 + r));
            }
        }
        return HammingScan<RATIO>::result(scan);
    });
}

hipError_t launch_hamming_mutual(hipStream_t st, const MutualParams& P, uint32_t words)
{
    if (P.n_pairs == 0) return hipSuccess;
    if (P.n_pairs > kMaxBlocksOf256) return hipErrorInvalidValue;
    const dim3 grid(P.n_pairs);
    return dispatch_words(words, [&](auto w) {
        return dispatch_ratio(P, [&](auto ratio) {
            hipLaunchKernelGGL((hamming_mutual_kernel<decltype(ratio)::value, decltype(w)::value>), grid, dim3(256), 0, st, P);
            return hipGetLastError();
        });
    });
}

}  // namespace r3dm
