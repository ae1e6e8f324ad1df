// r3dm_internal.hpp -- structures shared by the host library (api_*.cpp, r3dm_ctx.hpp) and the HIP kernels
// (kernels_*.hip).  Not part of the public ABI (include/r3dm.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/r3dm.h"

// Developer knobs -- A/B kernel variants (two of them ablations whose results are meaningless), traces, invariant checks, the
// launch-order switches -- exist only in the developer build: `build.sh dev` compiles the same sources with -DR3DM_DEVTOOLS
// plus tools/devtools/dev_knobs.cpp (the one place that calls getenv) into regard3d_amd/libr3dm_dev.so for tools/ and the
// fallback-path tests.  The product library (libr3dm.so) resolves every knob to its default at compile time and never reads
// the environment: a stray variable cannot change what a product call computes.
#ifdef R3DM_DEVTOOLS
int r3dm_dev_knob(const char* name, int dflt);
const char* r3dm_dev_str(const char* name);
#else
constexpr int r3dm_dev_knob(const char*, int dflt) { return dflt; }
constexpr const char* r3dm_dev_str(const char*) { return nullptr; }
#endif

namespace r3dm {

constexpr uint32_t kNone = 0xFFFFFFFFu;       // "no match" / invalid row
constexpr uint32_t kTileRows = 32;            // rows per MFMA tile (32x32x2 f32)
constexpr uint32_t kSlackBytes = 32768;
// l2_knn2_prune_kernel tests a tile after GP = kPrefixGroups of its 16 groups of 8 dimensions (DESIGN.md, f32 kernel section)
constexpr uint32_t kPrefixGroups = 12;
// the min form of l2_knn2_half_kernel's tile tests serves views whose ImgDev::max_norm_bits lies below the bits of 2^28 (compared as
// unsigned integers, so a NaN norm lies above): then no key of any level is a NaN or -inf (kernels_match.hip above the kernel)
constexpr uint32_t kMinTileTestNormBits = 0x4D800000u;
__host__ __device__ inline uint32_t prefix_norm_offset(uint32_t n_tiles) { return n_tiles * 32u + kSlackBytes / 4u; }      // in floats
__host__ __device__ inline size_t norms_bytes(uint32_t n_tiles) { return 2 * ((size_t)n_tiles * 128 + kSlackBytes); }
// the prefix groups of the build that runs: the product's constant; the developer build's R3DM_L2_VARIANT 109 .. 112 pick 9 .. 12
uint32_t l2_prefix_groups();
// A dispatch carries its global size (workgroups x threads per workgroup) as a 32-bit number of work-items: a launch of more
// than 2^32 - 1 threads is not rejected by the runtime, it WRAPS (found on the first C5-sized graph search: 4560 pairs x 4096
// workgroups x 256 threads ran only the first 464 pairs).  Launchers refuse such grids; callers batch below the limit.
constexpr uint64_t kMaxBlocksOf256 = 0xFFFFFFFFull / 256ull;       // zero slack behind every tiled / norm array (prefetch runs past the end)

// One registered view, resident in HBM.  Layouts (DESIGN.md "Data layout in HBM"):
//   rows  : row-major f32 [n][dim]            -- exact re-scoring in the reference's summation order
//   tiled : [n_tiles][G][2][32][4] f32        -- MFMA fragment order: float4 (g, h, r) = row 32t+r,
//                                                dims 8g+4h .. 8g+4h+3; one 1 KiB line per wave load
//   norms : f32 [n_tiles*32], ||row||^2, +inf for padding rows; behind its zeroed slack the PREFIX norms in the same form (the sum
//           over the first kPrefixDims dimensions, then slack again): prefix_norm_offset floats on.  One buffer and no pointer of its
//           own, so that the entry keeps the size and the offsets the other kernels' machine code was compiled with.
//   bin   : row-major u32 [n_pad][words]      -- binary descriptors, zero padded
struct ImgDev {
    const float*    rows;
    const float*    tiled;
    const float*    norms;
    const uint32_t* bin;
    const float*    xy;        // [n][2] pixel coordinates or nullptr
    const uint32_t* canon;     // position-class id per feature (smallest index with identical xy) or nullptr
    uint32_t n;
    uint32_t n_tiles;
    uint32_t dim;              // floats per row (F32/U8) or bytes per row (BIN)
    uint32_t G;                // dim padded to 8, / 8   (F32/U8)
    uint32_t words;            // u32 words per row (BIN)
    uint32_t width, height;
    uint32_t max_norm_bits;    // float bits of max ||row||^2 (filled by the staging kernel)
    uint32_t max_abs_bits;     // float bits of max |element|   (filled by the staging kernel)
    uint32_t not_integer;      // bit 0: some element is not an integer, bit 1: some element is negative (filled by the staging kernel)
    // graph index of the view (kernels_ann.hip), nullptr until r3dm_match_pairs_kgraph builds it
    const uint32_t* ann_adj;   // [n][kAnnDeg] neighbour rows ordered by (distance, id), kNone padded
    const uint32_t* ann_deg;   // [n] valid entries of each adjacency row
    // part of the index: the rows once more as bf16 ([n][dim], row-major) when every element is a bf16 (integers of magnitude
    // <= 256: SIFT bins), else nullptr.  The graph search is bound by its row gathers; this halves their bytes and converts back to
    // the SAME f32 values, so the search computes exactly what it computes on `rows`.  (Keep the three pointers adjacent: one copy sets them.)
    const uint16_t* ann_rows16;
    // ... or as bytes ([n][dim] u8) when every element is an integer in 0 .. 255 (what SIFT descriptors are on disk): one 128-byte
    // line per 128-dimensional row.  A view has at most one of the two copies.
    const uint8_t* ann_rows8;
    // bf16 fragment-order tiles for the integer fast path (r3dm_set_integer_mfma): [n_tiles][G/2][2][32][8] bf16,
    // lane half h of 16-dim block kb holds dims 16 kb + 8 h .. + 7 of row 32 t + r.  Exact iff the view is
    // integer-valued with |x| <= 256 (every such value is a bf16); the kernel checks that itself.
    const uint16_t* tiled16;
    // f16 hi / lo fragment-order tiles for the split nominator (r3dm_set_split_mfma): [n_tiles][G/2][hi | lo][2][32][8] f16 of the
    // values scaled by 2^split_k (max|x| 2^split_k in [2^13, 2^14); both filled by stage_split_kernel)
    const uint16_t* tiledh;
    int32_t split_k;
    // (in the 4 bytes of padding that followed split_k: the size of the entry and the offsets of its other fields stay what the
    // profiled machine code of the matching kernels was compiled with, profiles/pmc_traffic.json)
    uint32_t has_dup;          // != 0: some feature of the view shares its position with an earlier one (filled by the staging kernel)
    // count tiles (kernels_match.hip, l2_knn2_counts_kernel): rows that are small integers times a per-row scale (LIOP) as f16 integers
    // in fragment order [n_tiles][G/2][2][32][8], the row scales, and whether EVERY row of the view is of that form
    const uint16_t* tiledc;    // keypoint order: the QUERY side of the nominator
    const float* cscale;       // [n] row scales, keypoint order
    const uint16_t* tiledp;    // the same tiles with the rows in the order of their scales: the DATASET side
    const float* cquad;        // [n_tiles][64] the row line of an ordered tile: ||a||^2 of its 32 rows, then their negated scales
    const uint32_t* cperm;     // [n_tiles * 32] row of the ordered image -> keypoint index (kNone on padding)
    uint32_t counts_fail;      // != 0: some row is not (filled by the staging kernel)
    // binary views, opt-in MFMA Hamming (r3dm_set_hamming_mfma): one byte (0 / 1) per bit in i8 fragment order,
    // [n_tiles][words][2][32][16]; `norms` then holds popcount + 0x3F800000 as float bits
    const uint8_t* tiled8;
};
#ifndef R3DM_INF
#define R3DM_INF __builtin_huge_valf()
#endif
constexpr uint32_t kAnnDeg = 64;        // adjacency slots per row
constexpr uint32_t kAnnMaxK = 32;       // forward (exact nearest) neighbours per row
constexpr uint32_t kAnnMinRows = 128;   // views with fewer rows are matched exhaustively

struct AnnBuildJob {
    uint32_t slot;
    unsigned long long* fwd;      // [n][K] keys (distance bits << 32 | row), ascending, ~0 padded
    uint32_t* rev_cnt;            // [n]   reverse edges received
    uint32_t* rev_cur;            // [n]   fill cursor
    uint32_t* rev_off;            // [n+1] exclusive scan of rev_cnt
    unsigned long long* rev;      // [<= n*K] reverse keys, grouped by receiving row
    uint32_t* adj;                // -> ImgDev::ann_adj
    uint32_t* deg;                // -> ImgDev::ann_deg
    const uint8_t* rows8;         // the view's byte rows (ImgDev::ann_rows8 once the index is published) or nullptr
};
struct AnnBuildParams {
    const ImgDev* imgs;
    const AnnBuildJob* jobs;
    uint32_t K;
};
struct AnnSearchParams {
    const ImgDev* imgs;
    const uint2*  pairs;          // slot indices (I, J)
    const uint2*  pair_ids;       // view ids (I, J): keys of the start-row stream
    uint32_t      n_pairs;
    uint32_t      qb_per_pair;    // workgroups (4 queries each) per pair
    uint32_t      q_stride;
    uint32_t      flag_words;     // u32 words of the visited bitset of one query
    uint32_t      P, S, pool_cap; // start rows, neighbours expanded per step, K + P
    uint64_t      seed;
    float         ratio_R;
    uint32_t*     nn_idx;
    int32_t*      knn_idx;        // optional
    float*        knn_dist;       // optional
    unsigned long long* n_comps;  // distance evaluations (atomic)
};

// ---- HNSW plugin path (kernels_hnsw.hip): an index is three arrays in hnswlib's own shape
struct HnswView {
    const float*   rows;          // [n][dim] f32, row-major
    const uint8_t* rows8;         // the same rows as bytes when every element is an integer 0 .. 255 (ImgDev::ann_rows8), else nullptr
    const int32_t* l0;            // [n][1 + 2M]: count, links (farthest first, -1 padded)
    const int32_t* up_off;        // [n + 1]: first upper-layer row of a node (layer L of node i: row up_off[i] + L - 1)
    const int32_t* up;            // [rows][1 + M]
    uint32_t n, dim, M;
    int32_t enter, maxlevel;
};
struct HnswSearchJob {
    HnswView     ix;
    const float* query;           // [nq][dim]
    uint32_t     nq;
    uint32_t     out_base;        // first slot of the pair in nn_idx / knn_*
};
struct HnswSearchParams {
    const HnswSearchJob* jobs;
    uint32_t n_jobs, ef, cand_cap, flag_words;
    uint32_t rows8;               // != 0: every job's index view holds its byte rows; the search gathers those (a quarter of the bytes, the same float values)
    float    ratio_R;
    uint32_t* nn_idx;
    int32_t*  knn_idx;            // optional
    float*    knn_dist;           // optional
    unsigned long long* n_comps;  // distance evaluations (atomic)
    uint32_t* n_overflow;         // queries whose candidate heap did not fit cand_cap (their nn_idx slot holds 0xFFFFFFFE)
    uint32_t dense_steps;         // developer build: != 0 measures every link of a hop, visited or not, eight LINKS per step (the round-3 stepping; wavefront-per-query kernel only)
    uint32_t queries_per_wave;    // developer build: 2 / 4 / 8 run hnsw_search_group_kernel (measured, not adopted); else a wavefront per query
    uint32_t per_query;           // set by the launcher: LDS bytes of one query's state
};
// ---- MRPT plugin path (kernels_mrpt.hip): random projection trees of a view in the shape of /root/reference/src/thirdparty/mrpt/mrpt.h
struct MrptView {
    const float*   rows;          // [n][dim] f32, row-major
    const float*   RT;            // [dim][n_trees * depth]: the random matrix, transposed (zeros where the sparse matrix has no entry)
    const float*   splits;        // [n_trees][2^depth - 1], heap order
    const int32_t* leaves;        // [n_trees][n]: rows of a tree, leaf after leaf
    const int32_t* leaf_first;    // [2^depth + 1]
    uint32_t n, dim, n_trees, depth;
};
struct MrptQueryJob {
    MrptView     ix;
    const float* query;           // [nq][dim]
    uint32_t     nq;
    uint32_t     out_base;        // first slot of the pair in nn_idx / knn_*
};
struct MrptQueryParams {
    const MrptQueryJob* jobs;
    uint32_t n_jobs, votes, elected_cap;
    uint32_t max_n, pool_pad, per_wave, waves;   // set by the launcher
    float    ratio;               // UN-squared: the test runs on sqrt distances (RegionsMatcherT(regions, false))
    uint32_t* nn_idx;
    int32_t*  knn_idx;            // optional
    float*    knn_dist;           // optional: sqrtf of the squared L2 distances, -1 for a query without two elected rows
    unsigned long long* n_comps;  // distance evaluations (atomic)
};
hipError_t launch_mrpt_project(hipStream_t st, const float* rows, uint32_t n, uint32_t dim, const float* R, uint32_t n_trees, uint32_t depth, float* proj);
hipError_t launch_mrpt_trees(hipStream_t st, const float* proj, uint32_t n, uint32_t n_trees, uint32_t depth, uint32_t cap, unsigned long long* keys,
                             int32_t* leaves, float* splits);
// knn_k = 0: the 2-NN kernel (nn_idx, optional 2-lists); 1 .. R3DM_KNN_MAX: the k-list kernel (knn_idx / knn_dist [slot][knn_k], no ratio test)
hipError_t launch_mrpt_query(hipStream_t st, const MrptQueryParams& P, uint32_t max_nq, uint32_t max_n, uint32_t max_pool, uint32_t knn_k = 0);

struct HnswBuildJob {
    const float*    rows;
    const uint32_t* adj;          // ImgDev::ann_adj of the view (exact 32-NN graph + reverse edges)
    const uint32_t* adj_deg;
    const uint32_t* up_node;      // [up_rows] node of an upper-layer row
    const uint32_t* up_level;     // [up_rows] its layer (1 ..)
    const uint32_t* members;      // rows of layer 1, then layer 2, ... each ascending
    const uint32_t* mem_off;      // [maxlevel + 1] offsets into members
    int32_t* l0;
    int32_t* up;
    uint32_t n, dim, M, up_rows;
};
struct HnswBuildParams {
    const HnswBuildJob* jobs;
};

// What the pruning kernels keep behind MatchParams::prune_cnt (l2_knn2_prune_kernel: the first two counters; l2_knn2_half_kernel:
// all of it): counters of wave tiles (32 rows x 64 queries; atomic, zeroed by the host) and the addresses of two tables by slot of
// MatchParams::imgs, scratch of the call (run_match_batch), written by the host when the launch may prune.  Behind a pointer and in
// no field of ImgDev or MatchParams: their sizes and offsets are what every other kernel's machine code and kernel arguments were
// compiled with.  The order is the order the fields came in; the asserts below hold it.
struct PruneHeader {
    unsigned long long      n_tested;     // wave tiles tested
    unsigned long long      n_pruned;     // ... pruned by any test
    unsigned long long      n_filtered;   // ... pruned by the pair-norm filter, at either precision (part of n_pruned)
    const float* const*     pairnorm;     // pair-norm tiles per slot: [n_tiles][G / 2][2][32][4] f32 in the fragment order of `tiled`, half its bytes
    unsigned long long      n_half;       // ... pruned by the f16 level (part of n_filtered)
    const uint16_t* const*  halfnorm;     // f16 pair-norm tiles per slot: [n_tiles][G / 4][2][32][8] f16; set when MatchParams::prune bit 1 is
    unsigned long long      n_skip;       // tiles the f16 level sent straight to the restart, the filter unable to prune them (part of
                                          // no count above: these tiles go on)
    const uint16_t* const*  prefix16;     // the rows' first 8 GP dimensions as f16, per slot: [n_tiles][GP / 2][2][32][8] f16; set when MatchParams::prune bit 3 is
    unsigned long long      n_prefix16;   // tiles the f16 prefix test pruned in front of the restart (part of n_pruned)
};
// the header of a batch's fallback lists (r3dm_ctx::d_fb): zeroed per batch, [fb_cnt: P][fb_q: P x kFbPerPair] behind it
struct FbHeader {
    uint32_t    fb_total[2];              // MatchParams::fb_total
    uint32_t    pad0[2];
    PruneHeader prune;                    // MatchParams::prune_cnt
    uint32_t    pad1[2];
};

struct MatchParams {
    const ImgDev* imgs;
    const uint2*  pairs;          // slot indices (I, J)
    uint32_t      n_pairs;
    uint32_t      qb_per_pair;    // workgroups per pair
    uint32_t      xcd_map;        // != 0: all workgroups of a pair on one XCD (blockIdx & 7)
    uint32_t      q_stride;       // entries per pair in nn_idx / knn_* (>= max n_J)
    float         ratio_R;        // ratio^2 (squared metric) or ratio
    float         err_scale;      // certification slack factor: 4.25 Dpad 2^-24 (f32 tiles), (3 Dpad + 36) 2^-22 (split / count tiles)
    uint32_t*     nn_idx;         // [n_pairs][q_stride] matched I row, kNone, or kFallback
    int32_t*      knn_idx;        // optional [n_pairs][q_stride][2]
    float*        knn_dist;       // optional [n_pairs][q_stride][2]
    // queries whose nominated pair could not be certified are redone exactly; they are collected per
    // pair (fb_q[pair][0..kFbPerPair)) so one workgroup can stream image I once for all of them
    uint32_t*     fb_q;           // [n_pairs][kFbPerPair] query rows
    uint32_t*     fb_cnt;         // [n_pairs] number collected (may exceed kFbPerPair: overflow -> global rescan)
    uint32_t*     fb_total;       // [2]: total uncertified queries, number that overflowed their pair's list
    // the exact scan of a pair's uncertified queries split over fb_slices workgroups (row ranges of image I): per-slice results in
    // fb_part, the last workgroup of a pair to finish merges them (fb_done: tickets, zeroed by the host)
    float4*       fb_part;        // [n_pairs][kFbPerPair][fb_slices] (d0, bits of i0, d1, bits of i1)
    uint32_t*     fb_done;        // [n_pairs]
    uint32_t      fb_slices;      // 1: one workgroup per pair, results emitted directly
    // prefix pruning of the f32 2-NN tiles in match mode (r3dm_set_prefix_pruning; l2_knn2_prune_kernel).  Behind every older field:
    // their offsets are what the other kernels' machine code was compiled with.
    uint32_t      prune;          // != 0: launch_l2_knn2 may pick the pruning kernel; bit 1: with the f16 level in front (r3dm_set_half_filter);
                                  // bit 2: ... and its tile tests in the min form (r3dm_set_min_tile_test; every norm below kMinTileTestNormBits);
                                  // bit 3: ... and the f16 prefix test in front of the restart (r3dm_set_half_prefix)
    PruneHeader*  prune_cnt;      // the pruning kernels' counters and tables (FbHeader::prune)
};
static_assert(sizeof(MatchParams) == 120 && offsetof(MatchParams, prune_cnt) == 112, "kernel arguments: every 2-NN kernel was compiled with this layout");
static_assert(offsetof(PruneHeader, n_tested) == 0 && offsetof(PruneHeader, n_pruned) == 8 && offsetof(PruneHeader, n_filtered) == 16 &&
              offsetof(PruneHeader, pairnorm) == 24 && offsetof(PruneHeader, n_half) == 32 && offsetof(PruneHeader, halfnorm) == 40 &&
              offsetof(PruneHeader, n_skip) == 48 && offsetof(PruneHeader, prefix16) == 56 && offsetof(PruneHeader, n_prefix16) == 64 &&
              sizeof(PruneHeader) == 72, "the slots the pruning kernels were compiled with");
static_assert(offsetof(FbHeader, fb_total) == 0 && offsetof(FbHeader, prune) == 16 && sizeof(FbHeader) == 96, "24 words, the counters 8-byte aligned");
constexpr uint32_t kFbPerPair = 256;
constexpr uint32_t kFallback = 0xFFFFFFFEu;

struct FinalizeParams {
    const ImgDev* imgs;
    const uint2*  pairs;
    uint32_t      n_pairs;
    uint32_t      q_stride;
    const uint32_t* nn_idx;
    uint32_t      sort_cap;       // LDS sort capacity: power of two, >= q_stride unless the spill buffers are set
    unsigned long long* spill_keys;   // optional [n_pairs][spill_stride]: sort buffer of pairs keeping more than sort_cap matches
    unsigned char*      spill_drop;   // optional [n_pairs][spill_stride]
    uint32_t      spill_stride;   // power of two >= q_stride
    r3dm_match*   out;            // compacted matches
    uint64_t      out_cap;
    unsigned long long* total;    // running total (atomic)
    uint64_t*     pair_off;       // [n_pairs]
    uint32_t*     pair_cnt;       // [n_pairs]
};

// the mutual nearest-neighbour check (kernels_match_mutual.hip: l2_mutual_batch_kernel<RATIO, G>, l2_mutual_items_kernel<RATIO>,
// hamming_mutual_kernel<RATIO, W>; r3dm_set_mutual_matching): runs on nn_idx between the matcher and the finalisation; an accepted
// entry whose row of I has a nearer row of J (order: distance, row) becomes kNone.  RATIO is ratio_form != 0
struct MutualParams {
    const ImgDev* imgs;
    const uint2*  pairs;          // slot indices (I, J)
    uint32_t      n_pairs;
    uint32_t      q_stride;
    uint32_t*     nn_idx;         // [n_pairs][q_stride]
    unsigned long long* counters; // [3]: matches checked, dropped because not nearest, dropped by the reverse ratio (atomic; zeroed by the host)
    // the symmetric ratio test (r3dm_set_symmetric_ratio): a match that is nearest must also pass f(d1) < ratio_R * f(d2), d2 = the
    // smallest distance from its row of I to any other row of J.  ratio_form 0: mutual check only; 1: f = identity (ratio_R = the
    // forward test's R: ratio^2 on squared distances, ratio on Hamming distances); 2: f = sqrtf, ratio_R = ratio (the MRPT arm)
    float         ratio_R;
    uint32_t      ratio_form;
};
// the forward ratio test of the batch a finalisation collects, for the reverse one: R as the arm's kernels got it, on_roots = the arm
// compares square roots (MRPT's indexed pairs)
struct ForwardRatio { float R = 0.0f; bool on_roots = false; };

// the gate of preemptive matching (kernels_match_head.hip; r3dm_set_preemptive_matching, r3dm_preselect_pairs): a view's head is its
// min(h, n) largest-scale rows in a row-major buffer of its own; the table of a gate call is indexed by slot
struct HeadDev {
    const void* rows;             // f32 [n][8 G] (F32 / U8 views) or u32 [n][words] (BIN views)
    uint32_t    n;                // head rows, <= 256
    uint32_t    dim;              // floats per row as registered (F32 / U8); unused for BIN
};
struct HeadPair { uint32_t sI, sJ, out; };      // slots of the pair, entry of `counts` that receives its count
struct HeadMatchParams {
    const HeadDev*  heads;
    const HeadPair* pairs;        // the launch's pairs (one workgroup each): one length class
    uint32_t*       counts;
    float           ratio_R;      // ratio^2 (squared metric) or ratio
};

// the match budget (kernels_match_budget.hip; r3dm_set_match_budget, r3dm_budget_rows): a view of more than N rows is matched through
// a sub-view of its N highest-priority rows, staged in a slot of its own; matches come back through the sub-view's row list
constexpr uint32_t kBudgetChunk = 256;              // rows per step of the selection's compaction; R3DM_BUDGET_SELECT_CHUNK
struct BudgetSelectJob {
    const float* priority;        // one per row, finite and >= 0 (-0.0 stored as +0.0); null: the first rows
    uint32_t     n, N;            // rows of the view, the budget
    uint32_t*    rows_out;        // [min(N, n)] ascending
};
struct BudgetGatherArgs {
    const void*     src;          // fragment-order f32 tiles (F32 / U8 views) or word rows (BIN views)
    const uint32_t* rows;         // the listed rows
    uint32_t        n, hn, dim;   // rows of the view, rows listed, elements per row as registered (BIN: bytes)
    uint32_t        per_row;      // float4 per padded row (2 G) / words per row
    int             dtype;        // r3dm_dtype of the view: the element type of `out`
    void*           out;          // [hn][dim] row-major
    const float*    xy; float* xy_out;      // positions of the view (null: none) -> [hn][2]
};
struct BudgetMap { const uint32_t* rows; uint32_t n; };      // by slot: the row list of a sub-view slot, null for every other slot
struct BudgetRemapParams {
    const BudgetMap* maps;
    const uint2*     pairs;       // slots of the batch's pairs (one workgroup each)
    const uint64_t*  pair_off;    // FinalizeParams::pair_off / pair_cnt
    const uint32_t*  pair_cnt;
    r3dm_match*      matches;     // FinalizeParams::out
};

// pair proposal from bag-of-words view signatures (kernels_vocab.hip; r3dm_propose_pairs, r3dm_view_signatures)
constexpr uint32_t kVocabHistLdsWords = 8192;      // largest vocabulary whose histogram a workgroup privatises in LDS (32 KiB); R3DM_VOCAB_HIST_LDS_WORDS
constexpr uint32_t kVocabTile = 64;                 // views per side of a score tile
constexpr uint32_t kVocabChunk = 32;                // words of a score tile's LDS stage; R3DM_VOCAB_WORD_CHUNK
struct VocabHistJob {
    const int32_t* idx;           // the view's 2-lists as the matcher leaves them: [n][2], entry 0 = the row's word
    uint32_t       n;             // rows of the view
    uint32_t*      hist;          // [n_words], zeroed by the host
};
struct VocabScoreParams {
    const uint32_t* sig;          // signatures, `stride` words apart (a multiple of 4; the words past n_words are zero)
    const uint32_t* sig_row;      // [n_views]: the signature of every listed view
    uint32_t        stride, n_views;
    uint32_t        words_per_z;  // words of a workgroup's slice of the word axis (a multiple of kVocabChunk)
    uint32_t*       scores;       // [n_views][n_views], zeroed by the host; the diagonal stays 0
    const uint32_t* q;            // [stride] word weights (R3DM_VOCAB_WEIGHT_IDF; zero past n_words), or nullptr: plain counts
};
// vocabulary training (kernels_vocab_train.hip; r3dm_vocab_train)
constexpr uint32_t kVocabTrainBlock = 256;          // members of a word summed sequentially before the block sums are; R3DM_VOCAB_TRAIN_BLOCK
struct VocabAssignJob {
    const int32_t* idx;           // a view's 2-lists as the matcher leaves them: [n][2], entry 0 = the row's word
    uint32_t       n;             // rows of the view
    uint32_t       g0;            // global row of the view's first row
};
struct VocabTrainParams {
    const void* const* views;     // [n_views]: fragment-order f32 tiles (float / byte views) or word rows (binary views)
    const uint2*    loc;          // [T]: (view, local row) of the members in sorted order
    const uint2*    blocks;       // [n_blocks]: (first member, members <= kVocabTrainBlock) of a block
    const uint32_t* first_block;  // [n_words + 1]: the first block of every word
    const uint32_t* counts;       // [n_words]: members of every word
    uint32_t        n_blocks, n_words, dim;
    uint32_t        row_units;    // float4 per padded row of the tiles (2 G), or u32 words per binary row
    uint32_t        pieces;       // of them, those that hold elements: ceil(dim / 4) float4, or all words
    double*         block_sums;   // [n_blocks][pieces * 4]
    uint32_t*       block_bits;   // [n_blocks][pieces * 32] (binary)
    void*           words;        // [n_words][dim] of the vocabulary's type
};
struct VocabSelectParams {
    const uint32_t* scores;       // [n_views][n_views]
    const uint32_t* n_rows;       // [n_views]: rows of every listed view (R3DM_VOCAB_WEIGHT_IDF: its W = sum_w q[w] h[w])
    const uint32_t* rank;         // [n_views]: place of every listed view in view-id order
    uint32_t        n_views, top_k;
    uint32_t*       sel;          // [n_views][top_k]: ranks of the picks in order, kNone behind the last candidate
};

constexpr int kCoopB = 32;                  // models per batch of the cooperative AC-RANSAC kernel, at most
constexpr uint32_t kCoopMaxG = 30;          // slices per pair, at most (5-bit slice code of a task, 31 = start-up)

struct FilterParams {
    const ImgDev* imgs;
    const uint2*  pairs;          // slot indices, one per work item
    const uint2*  pair_ids;       // view ids (I, J): keys of the sample stream
    const uint64_t* offsets;      // per work item: [2k] = begin, [2k+1] = end of its putative list inside `matches`
    const uint32_t* order;        // launch order: workgroup b runs item order[b] (longest putative lists first), nullptr = identity
    const uint64_t* soff;         // per work item: start of its slice in the work arrays (multiples of 32 elements, m + 1 <= slice)
    const r3dm_match* matches;
    uint32_t      n_items;
    uint32_t      m_cap;          // LDS sort capacity (power of two); items with more putatives use the spill buffers
    uint32_t      wide;           // != 0: the 512-thread variant of the kernel (long match lists: one workgroup per CU, half the trips per pass)
    unsigned long long* spill_keys;  // optional global sort buffers for those items
    uint32_t*     spill_idx;
    const uint64_t* spill_off;    // [n_items] element offset of the item's slice (next_pow2(m) elements)
    double        precision_px;
    uint32_t      max_iter;
    uint64_t      seed;
    int           err_kind;
    int           model_kind;     // 0 = fundamental matrix (7-point), 1 = homography (4-point), 2 = essential matrix (5-point)
    uint32_t*     dbg;            // optional [4]: first violated invariant (code, item, a, b); R3DM_FILTER_CHECK=1
    const double* kinv;           // [slots][9] inverse intrinsics K^-1 of every view (essential matrix only)
    const float*  log10_tab;      // log10f(k), k = 0..max_m  (host-computed: same libm as the reference build)
    const float*  logc_k;         // logcombi(sample size, n), n = 0..max_m (host-computed)
    // outputs
    uint32_t*     inl_count;      // [n_items] inliers kept (0 if rejected)
    uint32_t*     inl_idx;        // [slices] inlier positions into the pair's putative list, AC-RANSAC order (indexed by soff)
    double*       F_out;          // [n_items][9]
    double*       thr_nfa;        // [n_items][2]  threshold px, nfa
    uint32_t*     iters;          // [n_items][2]  iterations, models
    // scratch (global memory, sliced per item by its `begin` offset)
    double*       pts_scratch;    // [slices][4] normalised (x1, y1, x2, y2)
    uint32_t*     pool_scratch;   // [n_matches]    current sampling pool
    float*        scratch_logc;   // [n_matches + n_items + 1] logcombi(k, m) table of each item
    double*       la_tab;         // [n_items][1024] NFA slope of every residual-histogram bin of the item (the one-workgroup kernel's scout pass)
    uint32_t      scout;          // != 0: the one-workgroup kernel scouts its models a wavefront each ahead of the walk (filter_acransac.inc)
    // ---- long pairs: the cooperative kernel (kernels_filter_coop.hip).  Items order[0 .. n_short) run on the one-workgroup-per-pair
    // kernel, the n_coop items of coop_items on a pool of workers over a task queue.
    uint32_t      n_short;
    uint32_t      n_coop;
    uint32_t      coop_workers;   // workgroups of the cooperative launch
    const uint32_t* coop_items;   // [n_coop] work item of every cooperative pair
    const uint32_t* coop_G;       // [n_coop] slices (workgroups per batch) of the pair, 1 .. kCoopMaxG
    const uint32_t* coop_slice;   // [n_coop] matches per slice (< 65536: the slice histograms count in 16 bits)
    const uint32_t* coop_hoff;    // [n_coop] first histogram slot of the pair
    unsigned char* coop_pub;      // [n_coop] 64-byte records a slice task reads about its pair (kernels_filter_coop.hip: CoopPub)
    double*       coop_models;    // [n_coop][chunk x 9 x MAX_MODELS] models of the current chunk of minimal samples
    double*       coop_bm;        // [n_coop][kCoopB][9] matrices the residuals of the batch in flight are taken with
    uint32_t*     coop_hist;      // [slots][kCoopB][512] residual histograms of a slice (1024 u16 bins per model)
    uint32_t*     coop_cnt;       // [slots][kCoopB] matches within the bound
    double*       coop_tstar;     // [slices] T*(k) of every item (indexed by soff), k = 0 .. m
    double*       coop_la;        // [n_coop][1024] NFA slope of every histogram bin
    unsigned long long* coop_prof; // developer build: [n_coop][16] wall-clock ticks per phase (kernels_filter_coop.hip), or nullptr
    uint32_t*     coop_q;         // task queue: [head, tail, done, potential, active, n_pairs, cap - 1, next pair to start] + seq[cap] + data[cap]
    // debug trace (R3DM_TRACE_PAIR): rows of (iter, model, #<=bound, NFA, improved) for one item
    double*       trace;
    uint32_t      trace_item, trace_cap, trace_iter;
    uint32_t*     trace_rows;
};

// Workgroup barrier for waves that exchange data through LDS, with an EXPLICIT `s_waitcnt lgkmcnt(0)`.  hipcc (ROCm 7.2) was
// seen to emit a bare s_barrier -- dropping the wait that __syncthreads' release fence implies -- when the barrier opens a loop
// header and the pending ds_write sits in the latch block (filter_acransac.inc, chunk loop: other waves then read a stale loop
// counter).  The builtin cannot be optimised away and costs nothing when nothing is pending.
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__device__ __forceinline__ void r3dm_syncthreads()
{
    __builtin_amdgcn_s_waitcnt(0xc07f);          // vmcnt = max, expcnt = max, lgkmcnt = 0
    __syncthreads();
}
#endif

// ---- Fast-A-KAZE detector (kernels_akaze.hip) ----
struct AkTaps { int n; float k[31]; };                  // Gaussian taps (host: getGaussianKernel restated), n <= 31
struct AkAreaTab { int si; float alpha; };              // one source cell of an INTER_AREA destination cell
struct AkLevelDev {
    int w, h, border;
    float ratio, psize;                                  // octave ratio; keypoint size before the final doubling (esigma * 1.5)
    const float* Ldet; const float* Lx; const float* Ly; const float* Lt;
    uint32_t* row_cnt; uint32_t* row_off;                // [h - 2 border] extrema per image row / exclusive scan
    unsigned long long* mask; uint32_t mask_words;       // [h - 2 border][mask_words] one bit per interior pixel: is a scale-space extremum (64-pixel ballots)
    uint32_t* counts;                                    // [0] candidates, [1] list entries after the in-level pruning
    float4* cand;                                        // raster-ordered candidates (x, y, response, -)
    float4* list;                                        // kept points (x, y, response, -), in insertion order
    float*  live;                                        // scratch for the live set of large levels (4 x capacity)
    unsigned char* dead_lower; unsigned char* dead_upper;
    float4* out0; float2* out1; uint32_t* out_valid;     // refined (x, y, size, response), dominant gradient vector, kept?
};
struct AkMldbItem { uint32_t level; float xf, yf, co, si, scale; };   // keypoint in level coordinates (level = image * n_levels + level), cos / sin of its angle, sigma_size
struct AkMsurfItem { uint32_t level; float xf, yf, co, si; int32_t scale; };   // the same for M-SURF-64: scale is the reference's int (fRound(size / 2 / ratio) = sigma_size)
// per image of a batch, written by the device: candidates the count pass found, whether they exceeded the slot capacity (then the
// image's lists were not built and the host repeats the detection phase with larger slot arrays), keypoints compacted
struct AkBatchMeta { uint32_t need, overflow, n_kp, pad; };
// one surviving keypoint as it crosses to the host: refined position, size (diameter), response, dominant gradient vector, level
struct AkKpRec { float x, y, size, response, max_x, max_y; uint32_t level, pad; };
// All launchers: B = images of the batch (same size); image buffers hold B planes back to back; levels = [B][n_levels].
hipError_t ak_mldb(hipStream_t st, const AkLevelDev* levels, const AkMldbItem* items, uint32_t n, const unsigned char* pairs, unsigned char* out);
// M-SURF-64 rows (64 floats each, 16-byte aligned) of n keypoints; `levels` must carry the M-SURF border (kAkSmaxMsurf)
hipError_t ak_msurf(hipStream_t st, const AkLevelDev* levels, const AkMsurfItem* items, uint32_t n, float* out);
hipError_t ak_bgr_to_gray(hipStream_t st, const unsigned char* bgr, float* gray, size_t n);
hipError_t ak_gaussian(hipStream_t st, const float* src, float* tmp, float* dst, int w, int h, int B, const AkTaps& kf);
hipError_t ak_scharr(hipStream_t st, const float* src, float* rd, float* rs, float* Lx, float* Ly, int w, int h, int B);
hipError_t ak_scharr_g2(hipStream_t st, const float* src, float* dst, int w, int h, int B, const float* inv_k2);
hipError_t ak_kcontrast(hipStream_t st, const uint32_t* hmax_bits, const uint32_t* hist, int nbins, uint32_t total, int have_hist, float* inv_k2, int B);
hipError_t ak_scaled_deriv_xy(hipStream_t st, const float* src, float* dst_x, float* dst_y, int w, int h, int B, int s);
hipError_t ak_scaled_deriv_det(hipStream_t st, const float* lx, const float* ly, float* ldet, int w, int h, int B, int s);
hipError_t ak_modg_max(hipStream_t st, const float* src, int w, int h, int B, uint32_t* out_max);
hipError_t ak_modg_hist(hipStream_t st, const float* src, int w, int h, int B, const uint32_t* hmax_bits, int nbins, uint32_t* hist);
hipError_t ak_fed_step(hipStream_t st, const float* Lt, const float* Lf, float* out, int w, int h, int B, float step_size);
hipError_t ak_fed_multi(hipStream_t st, const float* Lt, const float* Lf, float* out, int w, int h, int B, const float* tau, int n_steps);
hipError_t ak_level_head(hipStream_t st, const float* src, float* Lx, float* Ly, float* Ldet, float* flow, int w, int h, int B, const AkTaps& kf, int s,
                         const float* inv_k2, int rows_per_band);
hipError_t ak_fed_march(hipStream_t st, const float* Lt, const float* Lf, float* out, int w, int h, int B, const float* tau, int n_steps, int rows_per_band);
hipError_t ak_halfsample(hipStream_t st, const float* src, float* dst, int w, int h, int B, const AkAreaTab* xt, const int* xb,
                         const AkAreaTab* yt, const int* yb);
hipError_t ak_extrema(hipStream_t st, const AkLevelDev* levels, int n_levels, int B, int max_rows, float thr, int pass);
struct AkTileTable { uint32_t begin[17]; };            // first tile of every level in the extremum count pass (0xFFFFFFFF beyond the last level)
hipError_t ak_extrema_mask(hipStream_t st, const AkLevelDev* levels, int n_levels, int B, const AkTileTable& tt, uint32_t n_tiles, float thr);
hipError_t ak_scan_rows(hipStream_t st, const AkLevelDev* levels, int n_levels, int B);
hipError_t ak_layout(hipStream_t st, AkLevelDev* levels, int n_levels, int B, unsigned char* slots, uint32_t cap, AkBatchMeta* meta);
hipError_t ak_prune_levels(hipStream_t st, const AkLevelDev* levels, int n_levels, int B);
hipError_t ak_list_ranges(hipStream_t st, const AkLevelDev* levels, int n_levels, int B);
hipError_t ak_cross(hipStream_t st, const AkLevelDev* levels, int n_levels, int B, int mode);
hipError_t ak_refine(hipStream_t st, const AkLevelDev* levels, int n_levels, int B);
hipError_t ak_compact(hipStream_t st, const AkLevelDev* levels, int n_levels, int B, AkKpRec* recs, uint32_t cap, AkBatchMeta* meta);

// ---- classic A-KAZE detector (kernels_akaze_classic.hip) ----
constexpr int kAcMaxLevels = 16;                        // 4 octaves x 4 sublevels
struct AcCand { uint32_t x, y, level; float value; };   // a 3 x 3 maximum of one level, in the reference's scan order
struct AcSlot { float x, y, size, resp; uint32_t cls, pad; };   // an entry of kpts_aux (x, y in image coordinates)
struct AcOut { float x, y, size, angle, resp; uint32_t ok, pad0, pad1; };   // a slot after the upper-level filter, refinement, orientation
struct AcLevelTab {
    int n_levels;
    int w[kAcMaxLevels], h[kAcMaxLevels], octave[kAcMaxLevels];
    float esigma[kAcMaxLevels], ratio[kAcMaxLevels], off[kAcMaxLevels];   // off = .5 (ratio - 1)
    float smax;                                          // 10 sqrt(2) as the reference forms it
    uint32_t row0[kAcMaxLevels];                         // first row of each level in the per-image row-offset array of ac_scan_rows
};
// the parallel kpts_aux walk (ac_aux_parallel): per-candidate arrays of B x stride words, as kernels_akaze_classic.hip describes them
struct AcCc {
    uint32_t *par, *csz, *boff, *cur, *memb, *fin, *opn, *big, *bopen;
    uint32_t* n_big;                                     // [B] members of the handed-back components
    uint32_t* scratch;                                   // [B] (scan totals nobody reads)
    uint32_t* hist;                                      // [B x 32] component-size histogram (bin k: sizes in [2^k, 2^(k+1))), or null
    const uint32_t* rows;                                // row offsets of ac_scan_rows, rows_stride per image
    uint32_t rows_stride;
};
// the upper-level filter's buckets: per image cells_stride heads (-1 = empty), class k's cells at cell_off[k], side G[k]; next: stride per image
struct AcUpGrid { int* heads; int* next; size_t cells_stride; int img_w, img_h; uint32_t cell_off[kAcMaxLevels]; int G[kAcMaxLevels]; };
// the spatial grid of the kpts_aux walk, per image: cells_stride heads (-1 = empty) and ent_stride entries (slot, cell, next)
struct AcGrid { int* heads; uint32_t* ent_slot; uint32_t* ent_cell; int* ent_next; size_t cells_stride, ent_stride; int img_w, img_h; };
struct AcPlanes { const float* ldet[kAcMaxLevels]; const float* lx[kAcMaxLevels]; const float* ly[kAcMaxLevels]; };
hipError_t ac_kcontrast(hipStream_t st, const float* smooth1, int w, int h, int B, uint32_t* small);
hipError_t ac_fed_step(hipStream_t st, const float* Lt, const float* Lf, float* out, int w, int h, int B, float half_step);
hipError_t ac_hessian(hipStream_t st, const float* smooth, float* Lx, float* Ly, float* Ldet, int w, int h, int B, int s, float norm, float kc);
hipError_t ac_extrema(hipStream_t st, const float* ldet, int w, int h, int B, float thr, uint32_t* row_counts, uint32_t rows_stride,
                      uint32_t row0, AcCand* cand, uint32_t cand_stride, int level, int pass);
hipError_t ac_scan_rows(hipStream_t st, uint32_t* row_counts, uint32_t rows_stride, uint32_t n_rows, int B, uint32_t* totals);
hipError_t ac_aux(hipStream_t st, const AcCand* cand, uint32_t cand_stride, const uint32_t* totals, const AcLevelTab& tab, AcSlot* slots,
                  const AcGrid& grid, uint32_t* n_slots, int B);
// bound: components of at most this many candidates (<= 64) are walked by one wavefront each, larger ones by ac_aux_kernel<true>
hipError_t ac_aux_parallel(hipStream_t st, const AcCand* cand, uint32_t stride, const uint32_t* totals, const AcLevelTab& tab, AcSlot* slots,
                           const AcGrid& grid, uint32_t* n_slots, const AcCc& cc, uint32_t bound, int B);
// ug.heads == null: the upper-level filter compares every later slot (the developer build's R3DM_AC_AUX=0)
hipError_t ac_finish(hipStream_t st, const AcSlot* slots, uint32_t stride, const uint32_t* n_slots, const AcLevelTab& tab, const AcPlanes& pl,
                     AcOut* out, uint32_t max_slots, int B, const AcUpGrid& ug);
constexpr uint32_t kAkSlotBytes = 80;                  // per candidate slot: cand 16 + list 16 + live 16 + out0 16 + out1 8 + valid 4 + dead 2 (+ 2 spare)

// ---- run-time value -> template argument of a launch.  f(std::integral_constant<int, V>{}) launches and returns the status; a value
// without a kernel is hipErrorInvalidValue.  Each list is written here and nowhere else: the kernels that exist are the instantiations
// these functions make.  (Launchers whose cases carry further per-value template arguments -- prefetch depth, tile variants -- keep
// their own switch.)
// G: 8-float groups of a padded row with a tensor kernel, i.e. padded lengths 64 / 128 / 144 / 256
template <class F>
inline hipError_t dispatch_g(uint32_t G, F&& f)
{
    switch (G) {
        case 8:  return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 18: return f(std::integral_constant<int, 18>{});
        case 32: return f(std::integral_constant<int, 32>{});
        default: return hipErrorInvalidValue;
    }
}
// words: u32 words of a binary row with a kernel of its own (29 .. 32 / 61 .. 64 bytes)
template <class F>
inline hipError_t dispatch_words(uint32_t words, F&& f)
{
    switch (words) {
        case 8:  return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        default: return hipErrorInvalidValue;
    }
}
// KL is the list depth a K-list kernel is built with: 4 for k <= 4, 8 above (k <= R3DM_KNN_MAX is the caller's check)
template <class F>
inline hipError_t dispatch_kl(uint32_t k, F&& f)
{
    return k <= 4 ? f(std::integral_constant<int, 4>{}) : f(std::integral_constant<int, 8>{});
}
inline bool has_tensor_kernel(uint32_t G) { return dispatch_g(G, [](auto) { return hipSuccess; }) == hipSuccess; }

// ---- launch of a kernel whose dynamic LDS may pass the 64 KiB a kernel gets by default (the KGraph, HNSW and MRPT searches: their
// visited sets grow with the view).  The limit is raised on the kernel that is launched: one name, so the two cannot differ.
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
template <class... KArgs, class... Args>
inline hipError_t launch_with_lds(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}
#endif

// ---- launchers implemented in the .hip files (host side) ----
// registration of one float view (kernels_match.hip: stage_view_kernel): raw descriptors -> fragment-order tiles + norms + statistics
// (+ the row-major f32 copy when `rows` is given), the positions copied / entered into the position-class table by role blocks of the
// same launch, the classes read back by a second small launch
struct StageViewArgs {
    const void* raw;               // [n][dim] f32 or u8, row-major: device memory, or page-locked host memory read over the link
    int raw_is_u8;
    uint32_t n, dim, G, n_tiles;
    float* tiled; float* norms;        // norms: both halves (ImgDev::norms)
    uint32_t prefix_dims;              // the prefix norms' dimensions (8 l2_prefix_groups())
    float* rows;                   // optional
    uint32_t* img_stats;           // &ImgDev::max_norm_bits: 3 consecutive words (zeroed by the table entry's upload)
    const float* xy_src; float* xy_dst;         // optional positions (xy_src == xy_dst: already in place)
    unsigned long long* canon_keys; uint32_t* canon_vals; uint32_t canon_bits;     // hash table of 2^bits slots, all bytes 0xFF
    uint32_t* canon_dst; uint32_t* has_dup;     // -> ImgDev::canon's array, &ImgDev::has_dup
};
hipError_t launch_stage_view(hipStream_t st, const StageViewArgs& A);
hipError_t launch_stage_positions(hipStream_t st, const StageViewArgs& A);      // the position part alone (binary views)
hipError_t launch_untile_rows(hipStream_t st, const float* tiled, uint32_t n, uint32_t dim, uint32_t G, uint32_t n_tiles, float* rows);
hipError_t launch_stage_bf16(hipStream_t st, const float* tiled, uint32_t G, uint32_t n_tiles, uint16_t* tiled16);
// tiledrh: null, or the f16 tiles of the same pair norms (the f16 level of l2_knn2_half_kernel), n_tiles x G x 256 bytes
hipError_t launch_stage_pairnorm(hipStream_t st, const float* tiled, uint32_t G, uint32_t n_tiles, float* tiledr, uint16_t* tiledrh,
                                 uint16_t* tiledp16 = nullptr);
// whether launch_l2_knn2 takes the pruning kernel for such a launch (which reads the pair-norm tiles behind MatchParams::prune_cnt: the caller makes them, run_match_batch)
bool l2_prune_serves(uint32_t G, bool prune, bool raw_knn, float ratio_R);
hipError_t launch_stage_bin(hipStream_t st, const uint8_t* raw, uint32_t n, uint32_t nbytes,
                            uint32_t* bin, uint32_t words, uint32_t n_pad);
// returns hipErrorInvalidValue when (G, dtype) has no tensor kernel; caller falls back to the exact scan
hipError_t launch_l2_knn2(hipStream_t st, const MatchParams& P, uint32_t G, uint32_t max_nj_tiles, bool integer_mfma = false);
// (between the translation units of the matcher: the bf16 launcher, hipErrorNotSupported = no such kernel for this G; the LDS-shared developer variants)
hipError_t launch_l2_knn2_int(hipStream_t st, const MatchParams& P, uint32_t G, uint32_t max_nj_tiles);
hipError_t launch_l2_int_lds_variant(hipStream_t st, const MatchParams& P, uint32_t max_nj_tiles, int iv);
hipError_t launch_hamming_mfma(hipStream_t st, const MatchParams& P, uint32_t words, uint32_t max_nj_tiles);
hipError_t launch_stage_bin8(hipStream_t st, const uint32_t* bin, uint32_t n, uint32_t words, uint32_t n_tiles, uint8_t* tiled8, float* norms);
hipError_t launch_l2_knn2_split(hipStream_t st, const MatchParams& P, uint32_t G, uint32_t max_nj_tiles);
// ImgDev::cquad holds [n_tiles][64] row-line floats, slack, then [n_tiles + 1][16] quad summaries (the extra line: +inf / scale 1, the
// "tile before the first"): offset of the summaries in floats
__host__ __device__ inline size_t counts_summary_offset(uint32_t n_tiles) { return (size_t)n_tiles * 64u + 8192u; }
hipError_t launch_l2_knn2_counts(hipStream_t st, const MatchParams& P, uint32_t G, uint32_t max_nj_tiles, int variant = 0);   // variant 1: the two-list kernel for every G (l2_knn2_counts_kernel: float keys -- dataset views beyond 65,536 rows, and R3DM_COUNTS_TWO_LISTS in the developer build)
hipError_t launch_stage_counts(hipStream_t st, const float* rows, uint32_t n, uint32_t dim, uint32_t GB, uint32_t n_tiles,
                               uint16_t* tiledc, float* cscale, const float* norms, uint16_t* tiledp, float* crow, uint32_t* cperm,
                               uint32_t* fail_dev);
hipError_t launch_stage_split(hipStream_t st, const float* rows, uint32_t n, uint32_t dim, uint32_t GB, uint32_t n_tiles,
                              uint16_t* tiledh, const uint32_t* img_stats_dev, int32_t* split_k_dev);
hipError_t launch_l2_exact_items(hipStream_t st, const MatchParams& P, uint32_t count, int scan_all);
// exact scan of the per-pair fallback lists (one workgroup per pair); false return -> no kernel for this G
hipError_t launch_l2_exact_batch(hipStream_t st, const MatchParams& P, uint32_t G);
hipError_t launch_hamming_knn2(hipStream_t st, const MatchParams& P, uint32_t words, uint32_t max_n);
// the mutual check, each with P.ratio_form != 0 as its kernel's RATIO: l2_mutual_batch_kernel<RATIO, G>, one workgroup per pair over
// J's f32 tiles (G with a tensor kernel, dim % 4 == 0); hamming_mutual_kernel<RATIO, W> over the word rows of binary views (8 or 16
// words); l2_mutual_items_kernel<RATIO>, one workgroup per accepted match over the row-major rows for every other length (count =
// n_pairs x q_stride)
hipError_t launch_l2_mutual_batch(hipStream_t st, const MutualParams& P, uint32_t G);
hipError_t launch_l2_mutual_items(hipStream_t st, const MutualParams& P, uint32_t count);
hipError_t launch_hamming_mutual(hipStream_t st, const MutualParams& P, uint32_t words);
// preemptive matching: `hn` listed rows of a view -> its head buffer (per_row: float4 per padded row / words per row); the gate itself,
// one workgroup per pair (G of 8 / 16 / 18 / 32, or 8 / 16 words)
hipError_t launch_head_gather(hipStream_t st, const void* src, const uint32_t* rows, uint32_t hn, uint32_t per_row, bool binary, void* out);
hipError_t launch_head_match(hipStream_t st, const HeadMatchParams& P, uint32_t n_pairs, bool binary, uint32_t G_or_words);
// the match budget: one workgroup per job selects a view's rows; the listed rows and positions of one view -> row-major arrays; the
// matches of a finalised batch back into the views' own row numbers (one workgroup per pair)
hipError_t launch_budget_select(hipStream_t st, const BudgetSelectJob* jobs_dev, uint32_t n_jobs);
hipError_t launch_budget_gather(hipStream_t st, const BudgetGatherArgs& A);
hipError_t launch_budget_remap(hipStream_t st, const BudgetRemapParams& P, uint32_t n_pairs);
hipError_t launch_vocab_hist(hipStream_t st, const VocabHistJob* jobs, uint32_t n_jobs, uint32_t max_n, uint32_t n_words);
hipError_t launch_vocab_intersect(hipStream_t st, const VocabScoreParams& P, uint32_t n_slices);
hipError_t launch_vocab_select(hipStream_t st, const VocabSelectParams& P);
hipError_t launch_vocab_df(hipStream_t st, const uint32_t* sig, const uint32_t* sig_row, uint32_t stride, uint32_t n_views, uint32_t n_words, uint32_t* df);
hipError_t launch_vocab_weight_sums(hipStream_t st, const uint32_t* sig, const uint32_t* sig_row, uint32_t stride, uint32_t n_views, uint32_t n_words,
                                    const uint32_t* q, unsigned long long* W);
hipError_t launch_vocab_assign(hipStream_t st, const VocabAssignJob* jobs, uint32_t n_jobs, uint32_t max_n, uint32_t* assign, unsigned int* moved);
hipError_t launch_vocab_sort_keys(hipStream_t st, const uint32_t* assign, uint32_t T, uint32_t* keys, uint32_t* vals);
hipError_t launch_vocab_locate(hipStream_t st, const uint32_t* order, uint32_t T, const uint32_t* base, uint32_t n_views, uint2* loc);
hipError_t launch_vocab_block_sums(hipStream_t st, const VocabTrainParams& P, r3dm_dtype dtype);
hipError_t launch_vocab_update(hipStream_t st, const VocabTrainParams& P, r3dm_dtype dtype);
hipError_t launch_finalize(hipStream_t st, const FinalizeParams& P);
hipError_t launch_filter_F(hipStream_t st, const FilterParams& P);
hipError_t launch_filter_E(hipStream_t st, const FilterParams& P, size_t lds);   // the E kernels of launch_filter_F (kernels_filter_e.hip)
// one pool of workers for the long pairs of up to three filters: dev_params = FilterParams[3] in device memory indexed by model kind,
// q = the scheduling words, start = kind << 30 | pair in the order pairs are started
hipError_t launch_filter_coop(hipStream_t st, const FilterParams* dev_params, uint32_t* q, const uint32_t* start, uint32_t n_workers);
size_t     filter_coop_lds_bytes();
inline size_t filter_coop_model_doubles(int model_kind) { return model_kind == 2 ? 32u * 90u : 64u * 27u; }   // chunk x 9 x MAX_MODELS
size_t     filter_F_lds_bytes(uint32_t m_cap, int model_kind);
// rows8: every job carries byte rows -> the all-pairs scan runs on integer dot products (same keys)
// bin_words != 0: every job is a binary view of that many words per row (8 / 16) -> the Hamming scan of ImgDev::bin (dim unused)
hipError_t launch_ann_build(hipStream_t st, const AnnBuildParams& P, uint32_t n_jobs, uint32_t max_n, uint32_t dim, bool rows8, uint32_t bin_words = 0);
// rows_mode: 0 = f32 rows, 1 = ImgDev::ann_rows16 (bf16), 2 = ImgDev::ann_rows8 (u8) -- every indexed view of the batch must hold that copy;
// 3 = u8 rows on both sides (the query views hold ann_rows8 too): distances as integer dot products
// 4 = binary views on both sides (ImgDev::bin, 8 / 16 words per row; dim = their bytes): Hamming distances
// knn_k = 0: the 2-NN search kernels (nn_idx, optional 2-lists); 1 .. R3DM_KNN_MAX: their k-list instantiations, which write
// knn_idx / knn_dist [slot][knn_k] and no ratio test (pool_cap = knn_k + P; the caller sets ef = max(ef, knn_k))
hipError_t launch_ann_search(hipStream_t st, const AnnSearchParams& P, uint32_t max_nJ, uint32_t max_nI, uint32_t dim, int rows_mode, uint32_t knn_k = 0);
hipError_t launch_hnsw_search(hipStream_t st, const HnswSearchParams& P, uint32_t max_nq, uint32_t max_n, uint32_t dim, uint32_t knn_k = 0);
hipError_t launch_hnsw_link(hipStream_t st, const HnswBuildParams& P, uint32_t n_jobs, uint32_t max_items, uint32_t dim);
hipError_t launch_ann_rows16(hipStream_t st, const float* rows, uint16_t* rows16, size_t n_elems);
hipError_t launch_ann_rows8(hipStream_t st, const float* rows, uint8_t* rows8, size_t n_elems);
// img_of (optional): image of the batch each keypoint belongs to -- its pixels start img_of[k] * w * h floats into `image`
hipError_t launch_liop_extract(hipStream_t st, const float* image, int w, int h, const float* M6, const float* kern,
                               uint32_t n, float* patches, const uint32_t* img_of = nullptr);
// one contiguous run of matches of the graph gather kernel (kernels_graph.hip): element offsets into src / idx / dst
struct GraphSeg { uint64_t src, idx, dst; uint32_t cnt, pad; };
hipError_t launch_graph_gather(hipStream_t st, const r3dm_match* src, const uint32_t* idx, const GraphSeg* segs, uint32_t n_segs, r3dm_match* dst);

// ---- feature tracks (kernels_tracks.hip, api_tracks.cpp; r3dm_build_tracks).  A node (view, feature) is the
// slot base[rank of the view] + feature; all per-slot arrays hold N = base[V] entries, all per-match arrays M
struct TrkParams {
    const r3dm_match* matches;    // [M] the graph's matches, graph order
    const uint64_t* offsets;      // [P + 1]
    const uint32_t* pair_rank;    // [2 P] ranks of the two views of every pair
    uint32_t P, V, N, min_length;
    uint64_t M;
    const uint32_t* view_ids;     // [V] ascending
    const uint32_t* base;         // [V + 1] first slot of every view
    uint32_t* smax;               // [V] largest feature index (zeroed by the host)
    uint32_t* par;                // [N] union-find parent; after flatten the root (a component's smallest slot) of every touched slot
    uint32_t* csz;                // [N] nodes of the component, at its root (zeroed)
    uint8_t* touched;             // [N] the slot is a node of the graph (zeroed)
    uint8_t* conf;                // [N] at a root: two nodes of one view (zeroed)
    uint8_t* surv;                // [N] at a root: the component is a track
    uint32_t* ma;                 // [M] slot of the match's first node
    uint32_t* rel;                // [M] position of the match in its pair's list
    uint8_t* keep;                // [M] the match's component is a track
    uint32_t* pair_kept;          // [P] such matches of every pair (zeroed)
    uint32_t* nodes;              // [n_nodes] the touched slots, ascending
    uint32_t* keys;               // [n_nodes] their roots
    uint32_t* skey; uint32_t* sval;   // [n_nodes] (root, slot) sorted by root, stable: components in root order, members ascending
    uint8_t* nodeflag;            // [n_nodes] the sorted node is an observation
    uint64_t n_nodes, n_obs;
    uint32_t* oslots;             // [n_obs] slots of the observations in output order
    r3dm_observation* obs;        // [n_obs]
    uint8_t* hflag;               // [n_obs] first observation of its track
    unsigned long long* ctr;      // [8] counters (kernels_tracks.hip: trk_classify_kernel), zeroed
};
enum class TrkStep { kExtent, kInit, kLink, kFlatten, kKeys, kMark, kClassify, kEmit, kKeep };
hipError_t launch_tracks(hipStream_t st, const TrkParams& T, TrkStep step);
// order-preserving selection and stable radix sort (kernels_tracks.hip).  scratch: tracks_scratch_words(n, sort) words
size_t tracks_scratch_words(uint64_t n, bool sort);
// out = the positions i < n with flags[i] != 0, ascending (vals == nullptr), or vals[i] of those positions; *count = how many
hipError_t tracks_select(hipStream_t st, uint32_t* scratch, const uint8_t* flags, uint64_t n, const uint32_t* vals, uint32_t* out, unsigned long long* count);
hipError_t tracks_select64(hipStream_t st, uint32_t* scratch, const uint8_t* flags, uint64_t n, uint64_t* out, unsigned long long* count);
// (keys, vals) sorted by the low `bits` bits of the keys, stable; both pairs of arrays are work space; *in_second: the result is in
// (keys2, vals2), else in (keys, vals)
hipError_t tracks_sort_by_root(hipStream_t st, uint32_t* scratch, uint32_t* keys, uint32_t* vals, uint32_t* keys2, uint32_t* vals2, uint64_t n,
                               uint32_t bits, bool* in_second);

// guided matching (kernels_guided.hip; OpenMVG's geometry_aware::GuidedMatching): one job per pair, the queries are the rows of I
struct GuidedJob {
    double M[9];               // kind 0: F (for E: K_J^-T E K_I^-1), kind 1: H (x_J ~ H x_I)
    double errTh;              // a candidate passes iff err < errTh (f64, strict)
    double R;                  // ratio^2 of the descriptor mode
    uint32_t sI, sJ;           // slots of the two views
    uint32_t kind;             // 0 = EpipolarDistanceError, 1 = homography AsymmetricError
    uint32_t flags;            // kGuidedDesc: descriptor mode (else geometry only); kGuidedDedup: coordinate de-duplication; kGuidedBin: Hamming on bin rows
    uint32_t q0;               // first query of the job in the call's query numbering
    uint32_t b0;               // first workgroup of the job
    uint32_t nI, pad;
};
constexpr uint32_t kGuidedDesc = 1u, kGuidedDedup = 2u, kGuidedBin = 4u;
struct GuidedParams {
    const ImgDev* imgs;
    const GuidedJob* jobs;
    uint32_t n_jobs, n_blocks;
    uint32_t b_lo;             // the launch covers workgroups [b_lo, b_lo + n_blocks) of the call (chunks of the descriptor passes)
    uint32_t* res;             // [queries] matched row of J or kNone
    uint32_t* q_cnt;           // [queries] candidates (gate passed) of a descriptor-mode query
    unsigned long long* q_off; // [queries] their offset in cand (written by pass 1, relative to the chunk)
    unsigned long long* blk_cnt;         // [workgroups] candidates of a workgroup's descriptor-mode queries (pass 0)
    const unsigned long long* blk_base;  // [workgroups] where a workgroup's candidates start in cand, relative to its chunk
    uint32_t* cand;            // candidate rows of J, ascending per query: the lists of one chunk of workgroups
    unsigned long long* ctr;   // [0] candidates of every query (all modes)
    r3dm_match* out;           // [queries]: job k's list at [q0, q0 + out_cnt[k])
    uint32_t* out_cnt;         // [jobs]
};
constexpr uint32_t kGuidedTile = 4096;     // positions of J per LDS stage (32 KiB)
// pass 0: gate every (i, j), resolve geometry-only queries, count the candidates of descriptor-mode queries; pass 1: write them
hipError_t launch_guided_sweep(hipStream_t st, const GuidedParams& P, int pass);
hipError_t launch_guided_desc(hipStream_t st, const GuidedParams& P);
hipError_t launch_guided_compact(hipStream_t st, const GuidedParams& P);

// geometry tables of the 41 x 41 LIOP patch (api_liop.cpp: liop_prepare), all in device memory
struct LiopTables {
    const int* pix;            // [n_pix] support pixels in scan order, as offsets into the zero-ringed 43 x 43 patch
    const double* samp_w;      // [n_pix][4][2] fractional parts (wx, wy) of the four sample positions
    const int* samp_off;       // [n_pix][4] ringed-patch offset of every sample's top-left tap
    uint32_t n_pix;
};
hipError_t launch_liop(hipStream_t st, const LiopTables& T, const float* patches, uint32_t n, float* desc, uint32_t* n_tie_patches, uint32_t* tie_list);
// keypoints -> descriptors without the patches ever reaching HBM (the warp + blur runs inside the descriptor's wavefront)
hipError_t launch_liop_fused(hipStream_t st, const LiopTables& T, const float* image, int w, int h, const float* M6, const float* kern,
                             const uint32_t* img_of, uint32_t n, float* desc, uint32_t* n_tie_patches, uint32_t* tie_list);

// ---- exhaustive k-NN of one (dataset, query) pair, k = 1 .. R3DM_KNN_MAX (kernels_match_knn.hip; r3dm_knn / r3dm_index_knn)
struct KnnParams {
    const ImgDev* imgs;
    uint32_t      sI, sJ;         // slots of the dataset and of the query set
    uint32_t      k;              // neighbours per query, 1 .. R3DM_KNN_MAX
    float         err_scale;      // certification slack factor of the launch's tiles: 4.25 Dpad 2^-24 on the f32 tiles, (3 Dpad + 36) 2^-22 on the split planes (as MatchParams::err_scale)
    int32_t*      out_idx;        // [n_query][k] dataset rows, ascending under (distance, row)
    float*        out_dist;       // [n_query][k]
    uint32_t*     fb_q;           // [n_query] queries the nominator could not certify
    uint32_t*     fb_cnt;         // [1] how many (zeroed by the host)
};
// hipErrorInvalidValue: no nominator for this (G, dataset size); the caller scans every query exactly
hipError_t launch_l2_knnk(hipStream_t st, const KnnParams& P, uint32_t G, uint32_t n_tiles_dataset, uint32_t n_tiles_query);
// from_list != 0: the `count` queries of fb_q; else queries 0 .. count - 1
hipError_t launch_l2_exact_knn_items(hipStream_t st, const KnnParams& P, uint32_t count, int from_list);
hipError_t launch_hamming_knnk(hipStream_t st, const KnnParams& P, uint32_t words, uint32_t n_query);
// the K-list nominators on the 16-bit tiles (kernels_match_knn16.hip; r3dm_set_knn_narrow_tiles).  hipErrorInvalidValue /
// hipErrorNotSupported: no such kernel for this (G, dataset size) -- the caller keeps the f32 K-list kernel.  P.err_scale of the split
// launch is the split planes' factor, (3 Dpad + 36) 2^-22
hipError_t launch_l2_knnk_int(hipStream_t st, const KnnParams& P, uint32_t G, uint32_t n_tiles_dataset, uint32_t n_tiles_query);
hipError_t launch_l2_knnk_split(hipStream_t st, const KnnParams& P, uint32_t G, uint32_t n_tiles_dataset, uint32_t n_tiles_query);
// the K-list nominator of binary rows on the i8 tiles (kernels_match_knn8.hip; r3dm_set_knn_hamming_tiles): both views hold kLayBin8.
// hipErrorInvalidValue: no such kernel for this launch -- the caller keeps the popcount K-list kernel
hipError_t launch_hamming_knnk_mfma(hipStream_t st, const KnnParams& P, uint32_t words, uint32_t n_tiles_query);

}  // namespace r3dm
