/*
 * r3dm.h -- C ABI of the MI355X-native compute-matches hot path (libr3dm.so).
 *
 * Drop-in boundary for Regard3D's "Compute matches" stage.  Each entry point replaces one
 * interface of the reference (rhiestan/Regard3D, paths relative to /root/reference):
 *
 *   r3dm_set_image          <- Regions_Provider::load + regions_provider->get(I)
 *                              (src/R3DComputeMatches.cpp:2040, 443-472): one call per view with the
 *                              view's DescriptorRawData() / RegionCount() / DescriptorLength() and its
 *                              feature positions (Features_Provider::load, :2094-2095)
 *   r3dm_match_pairs        <- Matcher_Regions(fDistRatio, BRUTE_FORCE_L2).Match(regions_provider,
 *                              pairs, map_PutativesMatches) (src/R3DComputeMatches.cpp:2037-2039,2048)
 *                              and its in-tree clones kgraph_match / hnsw_match / mrpt_match
 *                              (:808-902, :502-597, :423-491): a new "matchingAlgorithm == 9" arm
 *   r3dm_filter_F           <- ImageCollectionGeometricFilter::Robust_model_estimation(
 *                              GeometricFilter_FMatrix_AC(4.0, 2048), putative, false) +
 *                              Get_geometric_matches() (src/R3DComputeMatches.cpp:2099,2113-2115)
 *   r3dm_knn2               <- openMVG::matching::ArrayMatcher<Scalar,Metric>::Build +
 *                              SearchNeighbours(query, nbQuery, &idx, &dist, NN=2)
 *                              (plugin contract: src/utils/matcher_kgraph.h:120-125,205-211)
 *   r3dm_save_matches /     <- openMVG::matching::Save / Load(PairWiseMatches, "matches.*.txt|.bin")
 *   r3dm_load_matches          (src/R3DComputeMatches.cpp:2064,2120; names src/R3DProject.cpp:858-871)
 *   r3dm_graph_*            <- openMVG::matching::PairWiseMatches accessors
 *                              (R3DComputeMatchesStatistics, src/R3DComputeMatches.h:59-66)
 *
 * Conventions: every function returns 0 on success or a negative r3dm_status; nothing throws;
 * all state lives in the opaque context; buffers passed in stay owned by the caller (they are
 * copied -- host or device pointers are both accepted, the copy is hipMemcpyDefault); objects
 * returned by the library are released only with the matching *_free.  One context per host
 * thread (or serialise externally); one context drives one GPU (one process per GPU, or r3dm_multi_* below for one
 * process driving several GPUs).
 * There is NO CPU fallback: if no gfx950 device is visible r3dm_create fails with
 * R3DM_ERR_NO_DEVICE.
 */
#ifndef R3DM_H
#define R3DM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct r3dm_ctx r3dm_ctx;
typedef struct r3dm_graph r3dm_graph;

typedef enum {
    R3DM_OK = 0,
    R3DM_ERR_INVALID = -1,     /* bad argument                                   */
    R3DM_ERR_NO_DEVICE = -2,   /* no usable gfx950 GPU / HIP runtime failure      */
    R3DM_ERR_HIP = -3,         /* a HIP call failed (see r3dm_last_error)         */
    R3DM_ERR_IO = -4,          /* file could not be read / written                */
    R3DM_ERR_UNSUPPORTED = -5, /* descriptor type / metric combination            */
    R3DM_ERR_NOMEM = -6
} r3dm_status;

typedef enum {
    R3DM_F32 = 0,   /* Scalar_Regions<.., float, D>: D floats per row (SIFT-128 f32, LIOP-144) */
    R3DM_U8 = 1,    /* Scalar_Regions<.., unsigned char, D>: D bytes per row, L2 metric        */
    R3DM_BIN = 2    /* Binary_Regions<.., NB>: NB bytes per row, Hamming metric                 */
} r3dm_dtype;

typedef struct { uint32_t i, j; } r3dm_match;   /* IndMatch{i_, j_}: i_ = row in I, j_ = row in J */

/* which squared epipolar error the AC kernel binds (default symmetric) */
typedef enum { R3DM_ERR_SYMMETRIC_EPIPOLAR = 0, R3DM_ERR_SAMPSON = 1, R3DM_ERR_EPIPOLAR_ONE_SIDED = 2 } r3dm_ferror;

/* ---- context ---- */
int  r3dm_create(int device_id, r3dm_ctx** out);
void r3dm_destroy(r3dm_ctx* ctx);
const char* r3dm_last_error(const r3dm_ctx* ctx);
/* "gfx950", CU count, bytes of HBM -- for reports */
int  r3dm_device_info(const r3dm_ctx* ctx, char* arch, size_t arch_cap, int* n_cu, uint64_t* hbm_bytes);

/* ---- views ----
 * Register (or replace) view `view_id`: n descriptors of `dim` elements (floats for F32, bytes for
 * U8/BIN), row-major, plus optional feature positions xy (n x 2 floats, pixel coordinates; NULL if
 * no coordinate de-duplication / geometric filter is wanted).  The data is copied to HBM and
 * re-laid-out there (MFMA fragment-order tiles + row norms).
 * What the reference does before it matches (Regions_Provider::load / Features_Provider::load, src/R3DComputeMatches.cpp:2040,2094-2095).
 * The call returns when the caller's buffers are consumed, NOT when the view is laid out: rows in pageable host memory are copied
 * into a ring of page-locked slots and travel from there (one DMA + one kernel per view, queued on the context's streams); rows
 * behind device pointers (this device's or a peer's) and page-locked host pointers are copied by the copy engine into the ring's
 * device slot, and only that copy is waited for.  A device buffer must be COMPLETE when the call is made: the library's streams are
 * not ordered behind the caller's, so the stream that produced the buffer has to be synchronised first (the features workers of
 * r3dm_multi_extract_features hand their batches over that way).  Every later call of the context is ordered behind
 * the registration; r3dm_images_wait waits for it explicitly.  A view costs its f32 tiles + norms in HBM (1.0 x its f32 size); the
 * layouts only some paths read (row-major rows for real-valued views and the approximate matchers, bf16 / split-f16 / count /
 * byte tiles of the opt-in paths) are made by the first call that needs them, or here when the path's switch is already on. */
int r3dm_set_image(r3dm_ctx* ctx, uint32_t view_id, uint32_t width, uint32_t height,
                   const void* desc, uint32_t n, uint32_t dim, r3dm_dtype dtype, const float* xy);
/* ... a whole collection in one call (the reference loads all regions in one Regions_Provider::load): helper threads of the host
 * fill the ring with the next views while the DMA and the kernels of the previous ones run.  dtype: r3dm_dtype. */
typedef struct r3dm_view_desc {
    uint32_t view_id, width, height;
    uint32_t n, dim;
    int32_t dtype;
    const void* desc;
    const float* xy;
} r3dm_view_desc;
int r3dm_set_images(r3dm_ctx* ctx, const r3dm_view_desc* views, uint32_t n_views);
int r3dm_images_wait(r3dm_ctx* ctx);
/* What a registered view holds in HBM (reports, tests): *layouts = the on-demand layouts staged so far, bits R3DM_LAYOUT_*;
 * *bytes = device memory of every layout and index of the view; *ring_uploads / *direct_uploads (context-wide, may be NULL) = views that
 * travelled through the page-locked ring / were copied straight from the caller's device or page-locked buffers (and empty views),
 * since r3dm_create. */
#define R3DM_LAYOUT_ROWS   1u   /* row-major f32 rows */
#define R3DM_LAYOUT_BF16   2u   /* bf16 tiles (r3dm_set_integer_mfma) */
#define R3DM_LAYOUT_SPLIT  4u   /* split-f16 planes (r3dm_set_split_mfma) */
#define R3DM_LAYOUT_COUNTS 8u   /* count tiles + scale order (r3dm_set_split_mfma, votes x scale rows) */
#define R3DM_LAYOUT_BIN8   16u  /* byte-per-bit tiles (r3dm_set_hamming_mfma) */
#define R3DM_LAYOUT_HEAD   32u  /* the head rows of preemptive matching (r3dm_set_preemptive_matching, r3dm_preselect_pairs) */
#define R3DM_LAYOUT_BUDGET 64u  /* the sub-view of the match budget (r3dm_set_match_budget) */
int r3dm_view_info(r3dm_ctx* ctx, uint32_t view_id, uint32_t* layouts, uint64_t* bytes, uint64_t* ring_uploads, uint64_t* direct_uploads);
/* device memory the context holds for its registered views (the slabs their layouts are cut from, live and recycled blocks alike),
 * for the upload ring (device slots + position-class tables), and the ring's page-locked host memory; any pointer may be NULL */
int r3dm_memory_info(const r3dm_ctx* ctx, uint64_t* views_device_bytes, uint64_t* ring_device_bytes, uint64_t* ring_host_bytes);
int r3dm_clear_images(r3dm_ctx* ctx);
/* r3dm_clear_images keeps the staging buffers of up to 256 cleared views for the next collection (the index buffers of a view are
 * always released); r3dm_trim gives those spares back to the device as well. */
int r3dm_trim(r3dm_ctx* ctx);

/* Opt-in integer fast path of the L2 matcher (default off; no reference counterpart -- the reference has one L2 loop,
 * openMVG/matching/metric.hpp L2_Vectorized via ArrayMatcherBruteForce).  When every view of a batch holds
 * integer-valued descriptors of magnitude <= 256 (SIFT bins 0..255 stored as float or u8), the all-pairs contraction
 * runs on v_mfma_f32_32x32x16_bf16 instead of v_mfma_f32_32x32x2_f32: every such value is a bf16, every product and
 * partial sum an integer below 2^24, so the f32 accumulators -- and therefore the matches -- are bit-identical to the
 * f32 path and to the reference; the kernel re-checks the condition per pair and sends anything else to the exact
 * scan.  Batches with any other view (LIOP, normalised SIFT) keep the f32 tiles.  r3dm_stats.n_integer_mfma reports
 * which path ran. */
int r3dm_set_integer_mfma(r3dm_ctx* ctx, int enable);

/* Prefix pruning of the f32 L2 matcher in match mode (default ON; no reference counterpart).  r3dm_match_pairs returns, per query,
 * its nearest row if d1 < R d2 and nothing else, so a dataset row matters to a query only below R x (the runner-up distance seen so
 * far).  On 128-dimensional rows with 0 < R <= 0.5 (a ratio up to 0.7 on
 * squared distances) the f32 kernel therefore tests every 32-row x 64-query tile after 96 of its 128
 * dimensions -- the squared distance over a prefix of the dimensions is a lower bound of the whole -- and skips the rest of a tile
 * that no query needs.  A query whose verdict could depend on a skipped row goes to the exact scan, so graphs are bit-identical
 * with the switch on or off (DESIGN.md, f32 kernel section, states the rule and its proof).  Everything else runs the kernel it ran
 * before: raw neighbour lists (r3dm_knn2, r3dm_knn, r3dm_index_*), other descriptor lengths, larger R, the opt-in
 * nominators.  r3dm_get_prefix_pruning_counts returns the tiles tested and the tiles skipped in the last r3dm_match_pairs call
 * (0 / 0 when the pruning kernel did not run); it costs a view 4 more bytes per row. */
int r3dm_set_prefix_pruning(r3dm_ctx* ctx, int enable);
int r3dm_get_prefix_pruning_counts(r3dm_ctx* ctx, uint64_t out[2]);
/* In front of the prefix test the kernel runs a cheaper one on every tile: the same contraction over 64 PAIR NORMS per row
 * (sqrt(x[2k]^2 + x[2k+1]^2), rounded up; Cauchy-Schwarz per pair bounds the distance from below), half of a tile's work instead of
 * three quarters.  A tile is skipped if either test rules it out; one that is not starts over and runs as before.  The pair norms are
 * scratch of the call (2 bytes per dimension and row of the batch's views, in one buffer of the context), made from the views' f32
 * tiles by every match call that prunes: a view holds no layout for them (r3dm_view_info reports what it reported).
 * r3dm_get_pair_filter_counts: the tiles of the last r3dm_match_pairs call that this first test skipped (part of out[1] above). */
int r3dm_get_pair_filter_counts(r3dm_ctx* ctx, uint64_t* out);
/* In front of that filter, a cheaper one still (default on): the same contraction on the pair norms rounded UP to f16, on the f16
 * matrix instructions -- a sixteenth of the filter's matrix cycles.  Its threshold carries a margin for the arithmetic of both, so
 * it skips a tile only if the filter would: the tiles skipped, both counters above and every result are the same with the switch
 * on or off, on any data (pair norms beyond f16's range just get nothing from it); only the time differs.  Off runs the kernel the
 * library ran before.  The f16 pair norms are scratch of the call too (half a byte more per dimension and row).
 * r3dm_get_half_filter_counts: the tiles of the last r3dm_match_pairs call that this level skipped (part of the filter's count). */
int r3dm_set_half_filter(r3dm_ctx* ctx, int enable);
int r3dm_get_half_filter_counts(r3dm_ctx* ctx, uint64_t* out);
/* A tile the f16 level cannot skip goes to the filter -- unless one of its f16 keys lies so far below the filter's threshold that
 * the filter provably cannot skip the tile either (the f16 rounding loses a bounded amount); then it starts over at once.  No tile
 * is treated differently by it, only the filter's work on such a tile is saved.  r3dm_get_level2_skip_counts: the tiles of the last
 * r3dm_match_pairs call that went from the f16 level straight to the restart (0 with the f16 level off). */
int r3dm_get_level2_skip_counts(r3dm_ctx* ctx, uint64_t* out);
/* The tests that decide a tile at these levels ask whether ONE of a lane's 16 keys lies at or below a threshold.  Where no key can
 * be a NaN or -inf, the minimum of the keys answers that (default on): a batch whose views all have max |row|^2 below 2^28 -- known on
 * the host, no synchronisation -- runs the kernel with its tile tests in that form, every other batch the general form.  Every tile
 * is decided as before, so the tiles skipped, all counters above and every result are the same with the switch on or off, on any
 * data; only the time differs.  Off runs the kernel the library ran before.  r3dm_get_min_tile_test_counts: the pairs of the last
 * r3dm_match_pairs call that the three-level kernel matched in the min form (out[0]) and in the general form (out[1]). */
int r3dm_set_min_tile_test(r3dm_ctx* ctx, int enable);
int r3dm_get_min_tile_test_counts(r3dm_ctx* ctx, uint64_t out[2]);
/* A tile none of these levels rules out starts over on its f32 rows, and that restart first tests a 96-dimension prefix distance --
 * which prunes most of the tiles that get there.  In front of it (default on, where the f16 level serves): the same prefix test on
 * the rows rounded to f16, on the f16 matrix instructions -- a sixteenth of its matrix cycles, half its bytes.  Its threshold carries
 * a margin for the rounding of the rows and the arithmetic of both, so it prunes a tile only if the restart's prefix test would: the
 * tiles pruned, all counters above and every result are the same with the switch on or off, on any data (elements beyond 32,752 in
 * magnitude get nothing from it); only the time differs.  Off runs the kernel the library ran before.  The f16 rows are scratch of
 * the call too (192 bytes more per row).  r3dm_get_half_prefix_counts: the tiles of the last
 * r3dm_match_pairs call that reached this test (out[0]) and that it pruned (out[1], part of the pruned tiles above). */
int r3dm_set_half_prefix(r3dm_ctx* ctx, int enable);
int r3dm_get_half_prefix_counts(r3dm_ctx* ctx, uint64_t out[2]);

/* Opt-in split-f16 nominator of the L2 matcher for REAL-valued descriptors (default off; no reference counterpart) -- LIOP-144,
 * normalised SIFT: what Regard3D actually matches (src/Regard3DFeatures.h:44-48).  Their matching is always "nominate on
 * MFMA keys, re-score the nominees with the reference's own summation (L2_Vectorized order, no FMA), certify against a
 * rounding slack, exact scan for what cannot be certified".  With this switch the nomination runs on
 * v_mfma_f32_32x32x16_f16 with every value split into two f16 pieces (a.b ~ ah.bh + al.bh + ah.bl, 3/16 of the matrix
 * cycles of the f32 tiles) and a slack that covers the split; the distances that are compared, ratio-tested and returned
 * are still the reference's f32 sums, so results are bit-identical to the default path and to the CPU restatement.
 * Batches of integer-valued views keep the f32 tiles (or r3dm_set_integer_mfma).  r3dm_stats.n_split_mfma reports which path ran. */
int r3dm_set_split_mfma(r3dm_ctx* ctx, int enable);

/* Opt-in exact MFMA formulation of the Hamming matcher for binary descriptors (default off: the default is the plain
 * xor + popcount kernel BASELINE config C3 names; no reference counterpart -- OpenMVG has one Hamming loop).  The bits of a
 * row become bytes 0 / 1, Hamming(a, b) = popcount(a) + popcount(b) - 2 a.b, and a.b runs on v_mfma_i32_32x32x32_i8 with
 * the dataset tiles shared by a workgroup through LDS; every quantity is a small integer, so indices, distances and
 * matches are bit-identical to the popcount kernel and to the CPU restatement (ties -> lowest row).
 * r3dm_stats.n_hamming_mfma reports which path ran. */
int r3dm_set_hamming_mfma(r3dm_ctx* ctx, int enable);

/* Opt-in mutual nearest-neighbour matching (default off; no reference counterpart -- SURVEY.md App. A.3 / App. C: "several queries of
 * J may map to the same row of I -- they are all kept (no cross-check / mutual-NN)", and parity with the reference depends on that
 * default).  Let (i, j) be a match a matcher would return: j's nearest row of I is i and the ratio test accepted it.  With the switch
 * on, (i, j) is kept iff j is the nearest row of J to row i under the order (distance, row index): there is no j' in J with
 * d(i, j') < d(i, j), or d(i, j') == d(i, j) and j' < j.  d is the reference distance for every arm and every tile format -- the f32
 * 4-way unrolled sum of squared differences with its scalar tail and no FMA for F32 / U8 rows (symmetric in its operands bit for bit,
 * so the forward and the reverse direction agree), the popcount Hamming distance for BIN rows; the MRPT arm applies its ratio to square
 * roots, the check still compares squared distances.  The approximate arms nominate approximately; the check is always the exhaustive
 * one over all rows of J, so the result is a deterministic subset of what the arm returns without it.  It runs after the ratio test
 * and BEFORE the (i_, j_) ordering and both de-duplications: a match that fails it is gone before the coordinate de-duplication looks at
 * its neighbours.  Consequences: a row of I appears at most once per pair; a view J with one row is always mutual; of two identical
 * rows of J the lower index survives.  The reverse ratio test is a switch of its own: r3dm_set_symmetric_ratio, below.
 * Honoured by r3dm_match_pairs, r3dm_match_pairs_kgraph / _hnsw / _mrpt, their r3dm_multi_* forms and the stage (R3DComputeMatches::
 * setMutualMatching, R3DM_STAGE_MUTUAL_MATCHING).  IGNORED by the entries that return raw neighbour lists -- r3dm_knn2, r3dm_knn, the
 * r3dm_index_* family, the *_knn2 / *_knn entries of the approximate matchers -- and by guided matching, which replaces lists after
 * the filters.  Cost: one more read of view J per pair that has accepted matches (kernels_match_mutual.hip); while the switch is off
 * nothing is allocated or launched for it.  r3dm_stats.n_mutual_checked / n_mutual_dropped report the last call. */
int r3dm_set_mutual_matching(r3dm_ctx* ctx, int enable);

/* Opt-in symmetric ratio test ("mutual + ratio", SMNN; default off; no reference counterpart -- SURVEY.md App. A.3 / App. C).  Let
 * (i, j) be a match a matcher would return: j's nearest row of I is i and the forward ratio test accepted it.  With the switch on,
 * (i, j) is kept iff the same 2-NN + ratio rule, applied with the two views swapped, accepts it:
 *   1. Nearest.  j is the nearest row of J to row i under the order (distance, row index) -- the rule of r3dm_set_mutual_matching,
 *      with the same distance d (the reference's f32 sum for F32 / U8 rows, the popcount distance for BIN rows).
 *   2. Reverse ratio.  Let d1 = d(i, j) and d2 = the smallest d(i, j') over all rows j' != j of J; which row gives d2 does not matter,
 *      and a duplicate of row j in J gives d2 = d1.  The match stays iff f(d1) < R * f(d2), evaluated in f32 with one multiply, a
 *      strict < and no FMA, where R and f are those of the forward test that accepted it: R = dist_ratio * dist_ratio (the f32
 *      product) and f the identity where the call compares squared distances (squared_metric != 0; the KGraph and HNSW matchers; the
 *      pairs an approximate matcher scans exhaustively); R = dist_ratio and f the identity otherwise, Hamming distances converted to
 *      float; R = dist_ratio and f = sqrtf for the pairs the MRPT matcher answers through its index, whose forward test runs on
 *      square roots.
 *   3. Fewer than two rows.  A view J with fewer than two rows has no second neighbour: the matcher with the views swapped returns
 *      nothing (SearchNeighbours fails for NN > rows), so NO match of such a pair survives.  This differs from the mutual rule on
 *      purpose, under which a view J with one row is always mutual.
 * Non-finite distances follow from the comparisons: a NaN is never less than anything, so it never becomes a minimum -- a row of I
 * whose distances are all NaN has no nearest row and its match is dropped as not nearest; a comparison with a NaN on either side of
 * the ratio test fails.
 * The two switches are independent: this one alone still applies part 1, and both together give what this one alone gives.  The check
 * runs where the mutual check runs -- after the forward ratio test, before the (i_, j_) ordering and both de-duplications -- on the
 * same exhaustive scan of J (kernels_match_mutual.hip keeps the second minimum of it), so the result is a deterministic subset of the
 * mutual result.  Honoured and ignored by the same entries as r3dm_set_mutual_matching (stage: R3DComputeMatches::setSymmetricRatio,
 * R3DM_STAGE_SYMMETRIC_RATIO); also ignored by the head match of preemptive matching and the quantisation of pair proposal.  While the
 * switch is off nothing is allocated or launched for it.  r3dm_stats.n_mutual_checked / n_mutual_dropped keep their meaning
 * (candidates looked at / dropped because not nearest: what the mutual switch alone would report); the matches the reverse ratio
 * alone removed are read through r3dm_symmetric_ratio_report. */
int r3dm_set_symmetric_ratio(r3dm_ctx* ctx, int enable);
/* The symmetric ratio test's counters of the last call that collected matches (r3dm_match_pairs and the three approximate matchers):
 * candidates checked, dropped because not nearest, dropped by the reverse ratio (every candidate of a pair whose view J has fewer than
 * two rows counts here).  Any pointer may be null.  All three are 0 after a call with the switch off. */
int r3dm_symmetric_ratio_report(const r3dm_ctx* ctx, uint64_t* checked, uint64_t* dropped_not_nearest, uint64_t* dropped_ratio);

/* Opt-in preemptive matching (default off; no reference counterpart -- the reference matches exhaustivePairs, SURVEY.md section 5, and
 * parity with it depends on that default): match only the largest-scale features of each view first, and run the full match of a pair
 * only if that small match finds enough correspondences (Wu, "Towards linear-time incremental structure from motion", 3DV 2013).
 * DROPPED PAIRS LOSE REAL MATCHES: the gate trades recall of the pair graph for time.
 *
 * Priority.  A view may carry one float per row: its feature scale, the third column of its .feat line.  Priorities must be finite
 * and >= 0; -0.0 is stored as +0.0.  Anything else is R3DM_ERR_INVALID; so is a count different from the view's rows, or an unknown
 * view.  A priority belongs to the registration: r3dm_set_image(s) on that id and r3dm_clear_images remove it.
 *
 * Head of a view for head size h (2 <= h <= 256).  The head is the min(h, n) rows that come first under the order (priority
 * descending, row index ascending).  The head is kept in ascending row index: a tie between two equally distant head rows therefore
 * resolves to the lower original row, as everywhere else.  A view without priorities has its first min(h, n) rows as head.
 *
 * Count of a pair (I, J).  Compute the 2-NN of every head row of J among the head rows of I, with the reference's distance:
 * exact_l2sq for F32 / U8 rows (4-way unrolled, scalar tail, no FMA) and popcount Hamming for BIN rows; ties go to the lowest row.
 * A query counts iff d0 < R * d1 in float.  R is what the calling entry uses: r3dm_match_pairs uses ratio^2 or ratio by its
 * squared_metric; the KGraph / HNSW / MRPT collection entries use ratio^2 on squared distances.  A head of I with fewer than two rows
 * gives count 0.  There is no de-duplication and no mutual rule: the count is the number of accepted queries.
 *
 * Keep.  A pair is kept iff its count >= t, with t >= 1.  A kept pair is then matched by the entry exactly as it is today, on the
 * whole views; a dropped pair does not enter the graph.  So the graph with the switch on is the graph with the switch off, restricted
 * to the kept pairs -- bit for bit, on every arm and tile format.
 *
 * Lengths.  F32 / U8 rows of any length up to 256 elements are served, lengths with a scalar tail (37, 61 ...) included: the tail is
 * summed as exact_l2sq sums it, not zero-padded into a group of four.  BIN rows of 29..32 and 61..64 bytes are served.  Longer L2 rows
 * are R3DM_ERR_UNSUPPORTED: r3dm_preselect_pairs returns it, and the match entries return it when the switch is on and such a view is
 * in the call.
 *
 * r3dm_set_view_priority: priority = n floats in host memory, NULL removes the view's priority (n is then ignored).
 * r3dm_preselect_pairs: the primitive, whatever the switch says: counts_out[p] = the count of pair p, in the caller's order (a pair
 *   with an empty view or views of different types has count 0; an unregistered view is R3DM_ERR_INVALID).
 * r3dm_set_preemptive_matching: the switch.  While it is on, r3dm_match_pairs and r3dm_match_pairs_kgraph / _hnsw / _mrpt (and their
 *   r3dm_multi_* forms, each context gating its own shard) gate their resolved pair list before they batch it.  IGNORED by the entries
 *   that return raw neighbour lists -- r3dm_knn2, r3dm_knn, the r3dm_index_* family, the *_knn2 / *_knn entries -- and by guided matching.
 *   head_rows outside 2..256 or min_matches of 0 is R3DM_ERR_INVALID (also when enable is 0: the values are stored either way).
 * Heads are made by the first gate that needs them (host selection, one small gather kernel per view: kernels_match_head.hip) and
 * cached per view with the h they were made for; a head is remade when h, the priority or the view changes.  r3dm_view_info shows
 * R3DM_LAYOUT_HEAD and counts its bytes.  While the switch is off and the primitive is not called nothing is allocated or launched.
 * r3dm_preselect_report: the last match call (the switch on) or r3dm_preselect_pairs call; all zero after a match call with the switch
 * off.  n_kept of r3dm_preselect_pairs counts against the min_matches last set (default 4). */
int r3dm_set_view_priority(r3dm_ctx* ctx, uint32_t view_id, const float* priority /* host */, uint32_t n);
int r3dm_preselect_pairs(r3dm_ctx* ctx, const uint32_t* pairs_ij, uint64_t n_pairs, uint32_t head_rows, float dist_ratio,
                         int squared_metric, uint32_t* counts_out /* [n_pairs], caller's order */);
int r3dm_set_preemptive_matching(r3dm_ctx* ctx, int enable, uint32_t head_rows, uint32_t min_matches);
typedef struct {
    double ms_kernels;                 /* HIP-event time of the gather and gate kernels */
    double ms_wall;                    /* host time of the gate: selection, uploads, kernels, the counts' way back */
    uint64_t n_pairs;                  /* pairs the gate looked at: pairs with an empty view or views of different types are skipped, in both entries */
    uint64_t n_kept;                   /* ... of those, pairs with count >= min_matches */
    uint64_t n_heads_built;            /* heads made by this call (the others were cached) */
    uint64_t n_views_without_priority; /* views of the call whose head is their first rows */
} r3dm_preselect_stats;
int r3dm_preselect_report(const r3dm_ctx* ctx, r3dm_preselect_stats* out);

/* Opt-in match budget (default off; no reference counterpart -- the reference matches every row of every view, and parity with it
 * depends on that default): only the N highest-priority rows of each view take part in putative matching (VisualSFM matches each
 * image's 8,192 largest-scale features: Wu, 3DV 2013; COLMAP bounds the features per image).  ROWS OUTSIDE THE BUDGET LOSE THEIR
 * MATCHES: the budget trades recall for time.  Nothing below carries a tolerance; every statement is bit for bit.
 *
 * Selected rows of a view of n rows for budget N (N >= 2).  S = the min(N, n) rows that come first under the order (priority
 * descending, row index ascending) -- the priority and the order of r3dm_set_view_priority above: finite, >= 0, -0.0 stored as +0.0 --
 * kept in ASCENDING ROW INDEX.  A view without priority takes its first min(N, n) rows.  A view with n <= N is WHOLE: nothing is copied,
 * no kernel runs for it, and it is matched as registered.
 *
 * Graph.  For a pair (I, J) the collection entry runs exactly as it does with the switch off on the view I' = the rows S(I) of I in that
 * order with their positions, and on J' likewise; every match (i', j') is returned as (S(I)[i'], S(J)[j']).  Put another way: the graph
 * equals the graph of a fresh context in which the caller registered the sub-arrays under the same view ids, with every index mapped
 * back through S -- on every arm and every tile format that collects matches into a graph (f32 tiles, r3dm_set_integer_mfma,
 * r3dm_set_split_mfma with its count tiles, the popcount Hamming kernel, r3dm_set_hamming_mfma; r3dm_match_pairs_kgraph / _hnsw / _mrpt,
 * whose indices are built on the sub-views and whose choice between index and scan looks at the sub-view), with the mutual and the
 * symmetric-ratio check on top, the coordinate de-duplication, the order of pairs and of matches within a pair, and the device mirror
 * under r3dm_set_device_graphs.  The ratio test sees the sub-view's second neighbour.  The budgeted graph is therefore NOT the full
 * graph restricted to S: a query whose runner-up lies outside S may be accepted here and refused there.
 *
 * Honoured by r3dm_match_pairs, r3dm_match_pairs_kgraph / _hnsw / _mrpt and their r3dm_multi_* forms (each context budgets its own
 * shard; the switch is r3dm_multi_set_match_budget; stage: R3DComputeMatches::setMatchBudget, R3DM_STAGE_MATCH_BUDGET).  IGNORED by the
 * entries that return raw neighbour lists -- r3dm_knn2, r3dm_knn, the r3dm_index_* family, the *_knn2 / *_knn entries --, by the
 * vocabulary entries, by r3dm_kgraph_index / r3dm_hnsw_index / r3dm_mrpt_index, which report on the whole view, and by guided matching
 * and the filters, which read the registered positions through original indices: with guided matching on, the budgeted putatives
 * decide which pairs and models survive and the guided step re-matches over ALL features.
 *
 * The preemptive gate is unchanged: it builds its heads from the whole views and runs before the budget.  With both switches on the
 * graph is the budgeted graph restricted to the gate's kept pairs.
 *
 * r3dm_set_match_budget: the switch.  max_rows < 2 is R3DM_ERR_INVALID (also when enable is 0: the value is stored either way).  While
 *   the switch is off and the primitive is not called nothing is allocated, uploaded or launched, and every entry returns what it
 *   returns without it.
 * r3dm_budget_rows: the primitive, whatever the switch says: S of the view from the device selection, ascending, in rows_out (room for
 *   min(max_rows, n) entries); *n_out = min(max_rows, n); a whole view returns 0 .. n - 1.  An unregistered view or max_rows < 2 is
 *   R3DM_ERR_INVALID.
 * Cache.  A budgeted view holds its sub-view as one more on-demand layout, R3DM_LAYOUT_BUDGET in r3dm_view_info, whose bytes -- the
 *   row list, the sub-view's layouts and the indices built on it -- are counted there and in r3dm_memory_info.  It is made by the first
 *   collection call that needs it (selection: one workgroup per view, all views of the call in one launch; priorities reach the device
 *   then; gather; staging as a registered view is staged) and remade when N, the priority or the registration changes;
 *   r3dm_set_image(s) on the id and r3dm_clear_images release it; r3dm_drop_indices also drops the indices built on sub-views.
 *   The selection walks a view R3DM_BUDGET_SELECT_CHUNK rows at a time -- it only matters to tests that straddle it.
 * r3dm_budget_report: the last collection call or the last r3dm_budget_rows call; all zero after a collection call with the switch off. */
#define R3DM_BUDGET_SELECT_CHUNK 256u
int r3dm_set_match_budget(r3dm_ctx* ctx, int enable, uint32_t max_rows);
int r3dm_budget_rows(r3dm_ctx* ctx, uint32_t view_id, uint32_t max_rows, uint32_t* rows_out, uint32_t* n_out);
typedef struct {
    double ms_select;                  /* HIP-event time of the selection kernel */
    double ms_gather;                  /* ... of the gather kernels */
    double ms_remap;                   /* ... of the remap kernels of the call's batches */
    double ms_wall;                    /* host time of the budget's share: substitution (selection, gather, staging) and remaps */
    uint64_t n_views_budgeted;         /* views of the call with more rows than the budget */
    uint64_t n_views_whole;            /* views of the call matched as registered */
    uint64_t n_subviews_built;         /* sub-views made by this call (the others were cached) */
    uint64_t n_rows_selected;          /* rows of the budgeted views that take part: max_rows each */
    uint64_t n_matches_remapped;       /* matches of pairs with a budgeted view, sent back through the row lists */
} r3dm_budget_stats;
int r3dm_budget_report(const r3dm_ctx* ctx, r3dm_budget_stats* out);

/* Pair proposal from bag-of-words view signatures (no reference counterpart -- the reference matches exhaustivePairs, SURVEY.md section
 * 5, and parity with it depends on that: nothing proposes pairs unless a caller asks).  Instead of matching all n (n - 1) / 2 pairs of a
 * collection, quantise every descriptor to a visual word, describe a view by its word histogram, score every pair of views by histogram
 * intersection and match only each view's top_k best partners.  PAIRS THAT ARE NOT PROPOSED ARE NEVER MATCHED: retrieval trades recall of
 * the pair graph for time.  Every quantity below is an integer, so a result depends on (rows, vocabulary, view list, top_k) only.
 *
 * Vocabulary.  n_words rows of one type and length, 2 <= n_words <= 65,536: F32 or U8 rows of any length the exhaustive matcher serves,
 * BIN rows of the byte lengths it serves (29..32, 61..64; others R3DM_ERR_UNSUPPORTED).  It belongs to the device of the context that
 * made it and may be used with any context of that device.
 *   r3dm_vocab_sample: a deterministic even sample of registered views -- no RNG, no k-means.  All listed views must be registered, of
 *     one type and one length, and listed once; otherwise R3DM_ERR_INVALID.  Let T be the total row count of the listed views and their
 *     rows be concatenated in list order: word t is row floor((2 t + 1) T / (2 n_words)), in 64-bit integer arithmetic, t = 0 ..
 *     n_words - 1.  T < n_words is R3DM_ERR_INVALID.  The rows are gathered on the device from the views' resident layouts.
 *   r3dm_vocab_from_rows: the caller's own words, n_words x dim elements in host memory (floats for F32, bytes for U8 / BIN).
 *   r3dm_vocab_words: copies the words back (n_words x dim elements of the vocabulary's type): tests, callers that save a codebook.
 *   r3dm_vocab_free: releases the vocabulary and its signatures.  A failed creation leaves *out NULL and nothing behind.
 *
 * Word of a row.  Its nearest word under the reference's distance -- exact_l2sq for F32 / U8 rows (4-way unrolled, scalar tail, no FMA),
 * popcount Hamming for BIN rows -- ties to the lowest word index.  It is the first neighbour the exhaustive matcher returns with the
 * codebook staged as a private dataset view and the registered view as the query side (as r3dm_knn2 stages its arrays), so whichever
 * exact tile path the context's switches select (f32, r3dm_set_integer_mfma, r3dm_set_split_mfma, r3dm_set_hamming_mfma) gives the
 * same words.  r3dm_stats is left as the call found it.
 *
 * Signature of a view.  h[w] = the number of the view's rows whose word is w, u32; an empty view has an all-zero signature.  Signatures
 * live in the vocabulary, keyed by view id and by the view's registration: r3dm_set_image(s) on that id, or r3dm_clear_images, makes a
 * signature stale, and a stale or missing signature is rebuilt by the next call that needs it.
 *
 * Score of a pair.  s(i, j) = sum over w of min(h_i[w], h_j[w]), u32; s <= min(n_i, n_j).  s(i, i) is not used.
 *
 * Rank.  For view i the candidates are the other listed views j with n_j > 0; a view with n_i = 0 proposes nothing and is proposed by
 * nobody.  Candidates are ordered by key(i, j) = floor(s(i, j) * 2^32 / min(n_i, n_j)), computed in u64, descending, then by view id
 * ascending.  An integer key on purpose: a float division would make the order depend on rounding.
 *
 * r3dm_propose_pairs: builds the missing signatures, takes the first min(top_k, candidates) of every listed view's rank and returns the
 *   union as pairs (min id, max id), unique, sorted by (I, J), in pairs_out (2 ids per pair); *n_pairs_out = their number.  top_k >= 1.
 *   cap_pairs (the room of pairs_out, in pairs) below n_views * top_k is R3DM_ERR_INVALID: the union never exceeds that.  scores_out may
 *   be NULL; otherwise [n_views][n_views] u32 in list order, the diagonal 0.  R3DM_ERR_INVALID as well: an unregistered view, an id listed
 *   twice, a view whose type or length differs from the vocabulary's, n_views of 0.
 * r3dm_view_signatures: the primitive -- the histograms of the listed views, [n_views][n_words] u32 in list order; same refusals.
 * r3dm_vocab_report: the last r3dm_propose_pairs or r3dm_view_signatures call on the vocabulary.
 *
 * Cost.  Signatures: n_words * 4 bytes per view (rounded up to 16), in the vocabulary; a call's scratch is the matcher's own.  A view's
 * r3dm_view_info changes only as a match call on it would change it (layouts staged on first use).  While no vocabulary exists nothing is
 * allocated or launched; r3dm_stats gains no field.  The matchers know nothing of vocabularies: hand the proposed pairs to r3dm_match_pairs
 * or any other collection entry (r3dm_shard_pairs for a device list), and the graph is that of all pairs restricted to the proposed ones,
 * bit for bit; with r3dm_set_preemptive_matching on, the gate sees the proposed pairs.  The kernels are in kernels_vocab.hip; the
 * histogram kernel counts in LDS up to R3DM_VOCAB_HIST_LDS_WORDS words and with global atomics beyond, the score kernel streams the word
 * axis in chunks of R3DM_VOCAB_WORD_CHUNK -- both only matter to tests that straddle them. */
#define R3DM_VOCAB_MAX_WORDS 65536u
#define R3DM_VOCAB_HIST_LDS_WORDS 8192u
#define R3DM_VOCAB_WORD_CHUNK 32u
typedef struct r3dm_vocab r3dm_vocab;
int  r3dm_vocab_sample(r3dm_ctx* ctx, const uint32_t* view_ids, uint32_t n_views, uint32_t n_words, r3dm_vocab** out);
int  r3dm_vocab_from_rows(r3dm_ctx* ctx, const void* rows /* host */, uint32_t n_words, uint32_t dim, r3dm_dtype dtype, r3dm_vocab** out);
int  r3dm_vocab_info(const r3dm_vocab* vocab, uint32_t* n_words, uint32_t* dim, int32_t* dtype);      /* any pointer may be NULL */
int  r3dm_vocab_words(const r3dm_vocab* vocab, void* rows_out /* host */);
void r3dm_vocab_free(r3dm_vocab* vocab);
int  r3dm_view_signatures(r3dm_ctx* ctx, r3dm_vocab* vocab, const uint32_t* view_ids, uint32_t n_views, uint32_t* hist_out /* host */);
int  r3dm_propose_pairs(r3dm_ctx* ctx, r3dm_vocab* vocab, const uint32_t* view_ids, uint32_t n_views, uint32_t top_k,
                        uint32_t* pairs_out /* host, 2 x cap_pairs */, uint64_t cap_pairs, uint64_t* n_pairs_out, uint32_t* scores_out /* host, or NULL */);
typedef struct {
    double   ms_quantise;              /* HIP-event time of staging the codebook and the matcher's batches */
    double   ms_histogram, ms_score, ms_select;      /* ... of the histogram, score and selection kernels */
    uint64_t n_rows_quantised;         /* rows sent through the matcher by the call */
    uint64_t n_signatures_built;       /* signatures the call made (missing or stale) */
    uint64_t n_signatures_cached;      /* ... and found valid */
} r3dm_vocab_stats;
int  r3dm_vocab_report(const r3dm_vocab* vocab, r3dm_vocab_stats* out);

/* Trained vocabularies: Lloyd's k-means iterations on the device (opt-in like everything above: with neither
 * r3dm_vocab_train nor r3dm_vocab_set_weighting called, nothing new is allocated or launched and every result is what it was).
 *
 * r3dm_vocab_train: `init` is any vocabulary of the context's device and is not modified; *out is a new vocabulary of the same type,
 *   length and word count, without signatures.  The training set is every row of the listed views; global row g is the row's position in
 *   the concatenation of the views in list order (as in r3dm_vocab_sample; empty views are allowed), T their number.  Refusals: those of
 *   r3dm_vocab_sample (unregistered id, id listed twice, views of mixed type or length), a view unlike the vocabulary, another device's
 *   vocabulary, max_iterations == 0, T == 0 (R3DM_ERR_INVALID), T >= 2^32 (R3DM_ERR_UNSUPPORTED).  A failed call leaves *out NULL and
 *   nothing behind.  r3dm_stats is left as the call found it.
 *
 * Assignment.  a[g] = the word of row g under "Word of a row" above (first neighbour under the reference's distance, ties to the lowest
 *   word), against the current words; it does not depend on how the rows are batched or on the tile path the context's switches select.
 * Stop.  Iteration t = 0, 1, ... assigns and counts moved_t = #{g : a_t[g] != a_(t-1)[g]}, moved_0 = T.  If t > 0 and moved_t = 0 the
 *   call stops there: converged, no update.  Otherwise the words are updated; after max_iterations updates the call stops.
 * Members of word w.  The rows g with a[g] = w in ascending g; count = their number.
 * Update, F32.  Per dimension the members are summed in double on a fixed tree: blocks of R3DM_VOCAB_TRAIN_BLOCK consecutive members are
 *   each summed sequentially in member order starting from 0.0, then the block sums are added sequentially in block order starting from
 *   0.0.  New element = (float)(sum / (double)count): an IEEE double division, rounded to nearest-even into f32.  There is no product, so
 *   no FMA can enter.  (A restatement must add in this order: numpy's sum is pairwise, cumsum is sequential.)
 * Update, U8.  Exact integer sums; byte = floor((2 sum + count) / (2 count)): a half rounds up.
 * Update, BIN.  Per bit, ones = the members with the bit set; the bit is 1 iff 2 ones > count (a tie gives 0).
 * Empty words.  A word without members keeps its row.
 *
 * r3dm_vocab_train_report: of the r3dm_vocab_train call that made this vocabulary (all zero for any other vocabulary). */
#define R3DM_VOCAB_TRAIN_BLOCK 256u
typedef struct {
    uint32_t n_updates;                /* updates run: <= max_iterations */
    uint32_t converged;                /* 1: an assignment moved no row; 0: stopped by max_iterations */
    uint64_t n_moved;                  /* moved_t of the last assignment */
    uint64_t n_empty;                  /* words without members under the last assignment */
    uint64_t max_members;              /* the largest member count under the last assignment */
    uint64_t n_rows_assigned;          /* rows sent through the matcher, all assignments together */
    double   ms_assign, ms_sort, ms_update;          /* HIP-event times of the three phases, summed over the iterations */
} r3dm_vocab_train_stats;
int  r3dm_vocab_train(r3dm_ctx* ctx, const r3dm_vocab* init, const uint32_t* view_ids, uint32_t n_views, uint32_t max_iterations, r3dm_vocab** out);
int  r3dm_vocab_train_report(const r3dm_vocab* vocab, r3dm_vocab_train_stats* out);

/* idf-weighted scores.  r3dm_vocab_set_weighting(vocab, R3DM_VOCAB_WEIGHT_IDF) changes how r3dm_propose_pairs on that vocabulary scores
 * and ranks (r3dm_view_signatures is unaffected); R3DM_VOCAB_WEIGHT_COUNTS, the default, is the rule above.  Under IDF every call computes,
 * from its own list of views:
 *   N = the listed views with rows;  df[w] = those of them with h[w] > 0;  q[w] = 0 if df[w] = 0, else log2_q8(N, df[w])
 *   log2_q8(N, df), an integer procedure for 256 log2(N / df), N >= df >= 1:
 *     e = the largest integer with df 2^e <= N;  x = floor(N 2^(62 - e) / df) (Q1.62 in [2^62, 2^63), 128-bit numerator);  q = e;
 *     eight times: x = (x x) >> 62 on the 128-bit product;  q = 2 q;  if x >= 2^63 then x >>= 1 and q += 1.
 *     (q(N, N) = 0, q(8, 1) = 768, q(3, 2) = 149; a word present in every listed view weighs nothing.)
 *   s(i, j) = sum_w q[w] min(h_i[w], h_j[w]);  W_i = sum_w q[w] h_i[w];  key(i, j) = floor(s 2^32 / min(W_i, W_j)) in u64
 *   candidates: the listed views with W > 0; a view with W_i = 0 proposes nothing and is proposed by nobody.  Rank, union and scores_out
 *   (u32) as above.  If any W_i >= 2^32 the call returns R3DM_ERR_UNSUPPORTED (this keeps s in u32 and s 2^32 in u64).
 * r3dm_vocab_weights: q of the last r3dm_propose_pairs call on the vocabulary, n_words u32; all 1 under COUNTS or before any call. */
#define R3DM_VOCAB_WEIGHT_COUNTS 0
#define R3DM_VOCAB_WEIGHT_IDF    1
int  r3dm_vocab_set_weighting(r3dm_vocab* vocab, int mode);
int  r3dm_vocab_weights(const r3dm_vocab* vocab, uint32_t* q_out /* host, n_words */);

/* ---- putative matching ----
 * pairs_ij: n_pairs x 2 view ids (I, J); J's rows are the queries, I's rows the dataset.
 * Descriptor lengths and speed: the tensor kernels serve float / byte rows of up to 64, 128, 144 and 256 elements (rows are padded
 * to the next of these: SIFT-128, LIOP-144, SURF-64, 256-D learned descriptors) and binary rows of 29..32 / 61..64 bytes.  Any other
 * L2 length (> 256 elements) is matched by the exact scan alone -- one workgroup per query row streaming the dataset: the same
 * results, two to three orders of magnitude slower; r3dm_stats.n_exact_fallback then equals n_queries.  Lengths that are not a
 * multiple of 4 (37, 61 ...) run on the tensor kernels like any other; only their uncertified queries (a handful per million) are
 * re-done by that per-query scan instead of the batched one, because the reference's 4-way unrolled sum ends in a scalar tail.
 * dist_ratio: Lowe ratio (0.6 default in the reference, src/Regard3DFeatures.cpp:129);
 * squared_metric != 0 applies ratio^2 (RegionsMatcherT ctor flag, true for L2).
 * The result holds only non-empty pairs, ordered by (I, J), matches ordered by (i_, j_). */
int r3dm_match_pairs(r3dm_ctx* ctx, const uint32_t* pairs_ij, uint64_t n_pairs,
                     float dist_ratio, int squared_metric, r3dm_graph** out);

/* ---- geometric filter ----
 * AC-RANSAC fundamental-matrix filter over every pair of `putative`.  F_out (may be NULL) receives
 * 9 doubles (row-major F) per KEPT pair, in the order of the returned graph. */
int r3dm_filter_F(r3dm_ctx* ctx, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                  uint64_t seed, r3dm_ferror err_kind, r3dm_graph** out, double* F_out);

/* Homography AC-RANSAC filter: ImageCollectionGeometricFilter::Robust_model_estimation(
 * GeometricFilter_HMatrix_AC(4.0, 2048), putative, false) (src/R3DComputeMatches.cpp:2216-2221; run by default,
 * src/Regard3DFeatures.cpp:129-131) -- 4-point DLT, asymmetric transfer error, point-to-point NFA scale,
 * accept iff #inliers > 2.5 * 4.  H_out: 9 doubles (row-major H, x_J ~ H x_I) per KEPT pair. */
int r3dm_filter_H(r3dm_ctx* ctx, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                  uint64_t seed, r3dm_graph** out, double* H_out);

/* Essential-matrix variant (GeometricFilter_EMatrix_AC(4.0, imax_iteration), src/R3DComputeMatches.cpp:2169, default on
 * via computeEssentialMatrix_) -- 5-point solver on K^-1 x, epipolar distance in pixels through F = K2^-T E K1^-1,
 * accept iff #inliers > 2.5 * 5 -- followed by Regard3D's own overlap rule (:2175-2192): a pair is dropped when it keeps
 * fewer than min_count (50) matches or less than min_ratio (0.3) of its putative matches; pass 0 / 0 for the bare
 * OpenMVG filter.  Needs r3dm_set_intrinsics for both views of a pair; pairs without are not estimated, as in
 * E_ACRobust.hpp.  E_out: 9 doubles (row-major E, x_J^T E x_I = 0 in camera coordinates) per KEPT pair.
 * K: row-major 3x3 pinhole matrix of the view (Pinhole_Intrinsic::K()), NULL to remove; call after r3dm_set_image. */
int r3dm_set_intrinsics(r3dm_ctx* ctx, uint32_t view_id, const double* K);
int r3dm_filter_E(r3dm_ctx* ctx, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                  uint64_t seed, uint32_t min_count, float min_ratio, r3dm_graph** out, double* E_out);

/* Per-pair outcome of the last r3dm_filter_F / r3dm_filter_H call -- what OpenMVG's ACRANSAC returns besides the inliers
 * (std::pair<errorMax, minNFA>) plus work counters.  One entry per pair of the putative graph, in its
 * order; pairs with too few putatives (<= 7 for F, <= 4 for H) are all-zero.  Returns the number of entries available. */
typedef struct {
    double   threshold_px;   /* AC-RANSAC inlier threshold (pixels); 0 when no meaningful model     */
    double   nfa;            /* minimum log10 NFA (+inf when nothing was evaluated)                  */
    uint32_t iterations;     /* iterations executed                                                  */
    uint32_t models;         /* models evaluated                                                     */
    uint32_t inliers;        /* inliers found (before the > 2.5*7 acceptance rule)                   */
    uint32_t reserved;
} r3dm_pair_report;
int r3dm_filter_report(const r3dm_ctx* ctx, r3dm_pair_report* out, uint64_t cap);
/* The three filters of one putative graph side by side -- what the reference runs one after the other at src/R3DComputeMatches.cpp:
 * 2113-2120 (F), :2130-2204 (E + overlap rule) and :2216-2233 (H); they only read the putative graph.  which: bit 0 F, bit 1 E, bit 2 H
 * (the out_* of a requested filter must not be NULL).  Pairs with >= 4096 putatives of all requested filters share ONE cooperative
 * kernel (a pool of persistent workgroups; a pair's residual passes are row slices run by idle workers), shorter pairs run one
 * workgroup per pair on a stream per filter; one filter alone is served the same way (r3dm_filter_F / _E / _H).  Results are those of
 * r3dm_filter_F / _E / _H whatever the split (inlier sets, models, iteration counts: tests/test_gpu_filter_coop.py).  ms_kernels3 /
 * ms_wall3 (optional): HIP-event time of the kernels and wall time of each call in the order F, E, H (they overlap; a filter with
 * long pairs ends when the cooperative kernel does).  r3dm_filter_report afterwards: the E call's, else the last requested kind's.
 * r3dm_stats: n_filter_workgroups / n_filter_coop_pairs. */
int r3dm_filter_FEH(r3dm_ctx* ctx, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter, uint64_t seed, int which,
                    uint32_t e_min_count, float e_min_ratio, r3dm_graph** out_F, r3dm_graph** out_E, r3dm_graph** out_H,
                    double* ms_kernels3, double* ms_wall3);

/* ---- guided matching (OpenMVG's bGuided_matching) ----
 * The reference runs every filter as Robust_model_estimation(functor, putatives, bGuided_matching, dDistanceRatio) with
 * bGuided_matching = false (src/R3DComputeMatches.cpp:2101,2113-2114 F; :2169-2170 E; :2215-2218 H, which already passes the
 * geometry-only ratio -1.0).  With true, OpenMVG re-matches every ACCEPTED pair over all features of both views and the result
 * replaces the pair's inlier list ("Guided matching"):
 *   - the queries are the features of I, the candidates all features of J; a candidate passes the geometric gate iff err < errTh
 *     (f64, strict) with errTh = threshold_px^2 and err the filter's own error with positions promoted to double: F
 *     EpipolarDistanceError(F, x_i, x_j), E the same on F = K_J^-T E K_I^-1 (r3dm_set_intrinsics of both views), H AsymmetricError
 *     (transfer error in J).  E's threshold_px is ALREADY the squared pixel bound (r3dm_pair_report of the E filter), so its
 *     effective gate is that value squared once more -- what OpenMVG's Square(m_dPrecision_robust) does with it; reproduced as is;
 *   - ratio >= 0 (descriptor mode; the reference's F and E default 0.6): among the candidates in ascending j, OpenMVG's
 *     distanceRatio update on SquaredDescriptorDistance (squared L2 in the reference arithmetic for float / byte rows, the Hamming
 *     distance for binary rows); a match (i, j_best) iff there were two candidates and (double)best < ratio^2 * (double)second;
 *   - ratio < 0 (geometry only; the reference's H): the j of smallest error (the first one on ties); for H the matches are then
 *     de-duplicated by coordinates (IndMatchDecorator: the smallest (i, j) of equal (xI, yI, xJ, yJ) stays);
 *   - matches are (i in I, j in J), ascending i, at most one per i.  A pair whose guided list is empty does not enter the graph
 *     (graphs here never hold empty entries; OpenMVG would insert it empty).
 * r3dm_guided_match is the primitive: it reads only the pair list of `pairs` and takes the caller's models (9 doubles per pair: F, E or
 * H as the filters return them) and thresholds (one per pair, as r3dm_pair_report.threshold_px reports them).  kind R3DM_GUIDED_*. */
#define R3DM_GUIDED_F 0
#define R3DM_GUIDED_E 1
#define R3DM_GUIDED_H 2
int r3dm_guided_match(r3dm_ctx* ctx, const r3dm_graph* pairs, int kind, const double* models, const double* threshold_px, double ratio,
                      r3dm_graph** out);
/* Context switch (default off: every filter returns what it returns without it, byte for byte).  While on, r3dm_filter_F / _E / _H /
 * _FEH (and r3dm_multi_filter_* through r3dm_multi_set_guided_matching) return the guided lists of their accepted pairs, one guided
 * launch per call for all its filters; E's overlap rule (min_count / min_ratio) is applied to the guided list, as Regard3D applies it
 * after Get_geometric_matches() (src/R3DComputeMatches.cpp:2175-2192).  F_out / E_out / H_out and r3dm_filter_report stay what
 * AC-RANSAC found (one model per pair of the returned graph).  ratio_*: the dDistanceRatio of each filter; the reference's own
 * arguments are 0.6, 0.6, -1.0 (R3DComputeMatches::setGuidedMatching). */
int r3dm_set_guided_matching(r3dm_ctx* ctx, int enable, double ratio_F, double ratio_E, double ratio_H);
/* The last guided step of the context (r3dm_guided_match, or a filter call with the switch on): HIP-event time of its kernels, wall
 * time, pairs re-matched (accepted pairs), queries (features of the I views), candidates that passed the geometric gate (candidates
 * per query = n_candidates / n_queries), matches before the graph's pair rules, and the chunks the descriptor mode ran in.
 * Memory: the descriptor mode holds the candidate lists of at most 2^28 candidates (1 GiB) at a time -- the queries are processed in
 * chunks of 256-query blocks below that budget, so a wide threshold costs time, not memory; a single block of 256 queries whose lists
 * alone exceed it is a chunk of its own (at most 256 x |J| candidates).  Everything else is O(queries of the call). */
typedef struct {
    double   ms_kernels, ms_wall;
    uint64_t n_pairs, n_queries, n_candidates, n_matches, n_desc_chunks;
} r3dm_guided_stats;
int r3dm_guided_report(const r3dm_ctx* ctx, r3dm_guided_stats* out);

/* ---- ArrayMatcher-shaped low level call: 2-NN of each query row among the dataset rows ----
 * out_idx / out_dist: 2 entries per query, ascending distance (dist: float squared L2 for F32/U8,
 * Hamming distance converted to float for BIN).  Fails (R3DM_ERR_INVALID) when n_query < 1 or
 * n_dataset < 2, like ArrayMatcherBruteForce::SearchNeighbours with NN = 2. */
int r3dm_knn2(r3dm_ctx* ctx, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query,
              uint32_t dim, r3dm_dtype dtype, int32_t* out_idx, float* out_dist);

/* The same with the dataset staged ONCE, the way the reference uses its plugins: Build per first view I, SearchNeighbours per
 * J from an OpenMP loop (src/R3DComputeMatches.cpp:462-479; ArrayMatcher_kgraph::Build / SearchNeighbours,
 * src/utils/matcher_kgraph.h:120-166,205-251).  r3dm_index_create copies and re-lays-out `dataset` (it need not outlive the
 * call); the index belongs to the context's DEVICE, not to the context: r3dm_index_knn2 may be called with any context of
 * that device, so a host can keep a small pool of contexts and run its searches concurrently (include/r3dm_array_matcher.hpp
 * does).  Each search uploads the query rows only; r3dm_stats.n_views_staged counts the copies + re-layouts a context made. */
typedef struct r3dm_index r3dm_index;
int  r3dm_index_create(r3dm_ctx* ctx, const void* dataset, uint32_t n_dataset, uint32_t dim, r3dm_dtype dtype, r3dm_index** out);
int  r3dm_index_knn2(r3dm_ctx* ctx, const r3dm_index* index, const void* query, uint32_t n_query, int32_t* out_idx, float* out_dist);
void r3dm_index_destroy(r3dm_index* index);

/* ---- the same two calls for k neighbours, k = 1 .. R3DM_KNN_MAX: ArrayMatcher::SearchNeighbours(query, nbQuery, &idx, &dist, NN)
 * with any NN, as the reference's plugins serve it (src/utils/matcher_kgraph.h:205-251, matcher_hnsw.h:138-173) ----
 * out_idx / out_dist: k entries per query at [q * k + j], ascending under (distance, dataset row): equal distances, lowest row
 * first.  F32 / U8 distances are the reference's f32 sums (4-way unrolled, no FMA), Hamming distances exact integers as float.
 * R3DM_ERR_INVALID: k < 1, k > R3DM_KNN_MAX, n_query < 1, n_dataset < k (the plugins' "NN > rows" rule), null pointers (a null
 * context is refused before any GPU is touched).  R3DM_ERR_UNSUPPORTED: the BIN byte-length rule of r3dm_knn2.
 * k <= 2 with n_dataset >= 2 runs the 2-NN path of r3dm_knn2 (bit-identical to it by construction; k = 1 is its first column).
 * Everything else -- k >= 3, and k = 1 on a one-row dataset -- runs on k-list kernels of its own: by default the f32 tiles (F32 / U8)
 * or the popcount kernel (BIN).
 *   IGNORED there: r3dm_set_integer_mfma / _split_mfma / _hamming_mfma (those nominators keep 2-lists).  None of their counters
 *     (n_integer_mfma, n_split_mfma, n_hamming_mfma, n_counts_mfma) moves on such a call, whatever any switch says.
 *   NOT ignored: r3dm_set_knn_narrow_tiles and r3dm_set_knn_hamming_tiles, the k-list kernels' own switches (below).
 * Lengths without a tensor kernel (> 256 elements) are scanned exactly, as in r3dm_match_pairs.  r3dm_stats.n_queries and
 * .n_exact_fallback (queries answered by the exact scan) describe the call. */
#define R3DM_KNN_MAX 8
/* Opt-in (default off), same results bit for bit: while on, a call that runs on the k-list kernels (k >= 3; k = 1 on a one-row
 * dataset) picks its nominator from the two views' statistics, under the conditions the 2-NN switches use:
 *   - both views integer-valued with magnitudes <= 256 and every partial sum below 2^24 (SIFT bins, any unsigned char rows), padded
 *     length 64, 128 or 256: the bf16 tiles of r3dm_set_integer_mfma with exact k-lists -- nothing is certified or scanned
 *     (r3dm_stats.n_knn_integer_tiles counts the launch; .n_exact_fallback is 0);
 *   - otherwise both views finite and non-zero, scales within reach of one another, not both integer-valued: the split-f16 planes of
 *     r3dm_set_split_mfma (r3dm_stats.n_knn_split_tiles); uncertified queries go to the exact scan as on the f32 tiles;
 *   - anything else (integer views beyond those bounds, 144-element integer views, lengths without a tensor kernel, BIN rows, a
 *     dataset whose tiles pass 2 GiB) runs exactly what it runs with the switch off, and neither counter moves.
 * The layouts are staged on first use; on an r3dm_index that is once per index, under its lock, whichever context asks first.
 * k <= 2 (the 2-NN path) does not consult this switch. */
int r3dm_set_knn_narrow_tiles(r3dm_ctx* ctx, int enable);
/* Opt-in (default off), same results bit for bit: the switch of BIN rows, which r3dm_set_knn_narrow_tiles leaves alone.  While on, a
 * call that runs on the k-list kernels (k >= 3; k = 1 on a one-row dataset) with BIN views runs on the i8 MFMA tiles of
 * r3dm_set_hamming_mfma -- one byte per bit, keys popcount(a) - 2 a.b -- with exact k-lists: the keys are integers, so nothing is
 * certified or scanned (r3dm_stats.n_knn_hamming_tiles counts the launch; .n_exact_fallback is 0; n_hamming_mfma, the 2-NN kernel's
 * counter, does not move).  With the switch off such a call runs the popcount k-list kernel, as before.  F32 / U8 views and k <= 2
 * never consult it.  The byte-per-bit tiles are staged on first use; on an r3dm_index that is once per index, under its lock,
 * whichever context asks first. */
int r3dm_set_knn_hamming_tiles(r3dm_ctx* ctx, int enable);
int r3dm_knn(r3dm_ctx* ctx, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query,
             uint32_t dim, r3dm_dtype dtype, uint32_t k, int32_t* out_idx, float* out_dist);
/* same mounting, locking and "any context of the index's device" rules as r3dm_index_knn2 */
int r3dm_index_knn(r3dm_ctx* ctx, const r3dm_index* index, const void* query, uint32_t n_query, uint32_t k,
                   int32_t* out_idx, float* out_dist);

/* ---- approximate matching: the KGraph plugin path (BASELINE config C5) ----
 * Replaces kgraph_match (src/R3DComputeMatches.cpp:808-902): per first view I an index over its descriptors
 * (ArrayMatcher_kgraph::Build, src/utils/matcher_kgraph.h:138-153), per query row of J a graph search for its 2
 * nearest rows (SearchNeighbours, :204-251 -> KGraphImpl::search, src/thirdparty/kgraph/kgraph.cpp:411-552), then
 * the same ratio test / de-duplication / pair rules as r3dm_match_pairs.  F32 (and U8) descriptors with
 * dim % 4 == 0 only, squared-L2 metric (kgraph_match constructs its matcher with b_squared_metric = true, :842); binary views under
 * the Hamming metric behind r3dm_set_kgraph_hamming (below), refused otherwise.
 * The index is the exact index_K-nearest-neighbour graph completed with reverse edges (DESIGN.md "ANN"); it is
 * built on first use and cached with the view.  Views with fewer than 128 rows are matched exhaustively.
 * Results are deterministic: they depend on (descriptors, parameters, view ids) only. */
typedef struct {
    uint32_t index_K;    /* forward neighbours per row, 1..32  (reference: IndexParams K/L, presets 2/20 .. 16/24) */
    uint32_t search_P;   /* random start rows per query, 2..61 (reference: SearchParams P, presets 2 / 6 / 12 / 10) */
    uint32_t search_S;   /* neighbours expanded per step, 1..16 (reference: SearchParams S, default 10)              */
    uint32_t reserved;
    uint64_t seed;       /* start-row stream (reference: SearchParams seed, 1998)                                    */
} r3dm_kgraph_params;
/* preset = matchingAlgorithm of the reference: 0 "KGraph fast", 1 "medium", 2 "precise", anything else its default
 * block (src/R3DComputeMatches.cpp:844-873) */
int r3dm_kgraph_preset(int preset, r3dm_kgraph_params* out);
/* parameters with which the graph matcher serves an approximate arm of the reference's dispatch (matchingAlgorithm,
 * src/R3DComputeMatches.cpp:2035-2062: 0 FLANN kd-trees, 1..3 KGraph, 5 MRPT, 6..8 HNSW) with a recall at least that of the arm;
 * R3DM_ERR_INVALID for the exhaustive arms 4 / 9 and unknown values.  The KGraph arms are the reference's algorithm.  The HNSW
 * arms have their own entry points (r3dm_match_pairs_hnsw below: hnswlib's search on an HNSW index) -- this mapping is what a host
 * uses for them only when it wants the FASTEST matcher of at least the arm's recall, or for a descriptor length hnswlib's SIMD16
 * distance does not serve.  The MRPT arm (5) has its own entry points too since round 4 (r3dm_match_pairs_mrpt below: random
 * projection trees built and queried on the device); this mapping serves it only under the fastest-matcher policy.  FLANN (arm 0)
 * is PERMANENTLY SUBSTITUTED: no kd-tree index is built here, the deterministic graph matcher answers for it and its matches are not
 * those the reference's arm would return (both are approximate) -- FLANN is an external library that is not in the reference tree,
 * so there is nothing to restate or pin, and every approximate arm measured on this GPU is slower than the exact fast paths, under
 * which the facade's default policy serves these arms at recall 1.  The arm numbers are accepted and mapped, never rejected.
 * See the table in api_match.cpp and DESIGN.md sections 4.7 and 7. */
int r3dm_ann_params_for_algorithm(int matching_algorithm, r3dm_kgraph_params* out);
int r3dm_match_pairs_kgraph(r3dm_ctx* ctx, const uint32_t* pairs_ij, uint64_t n_pairs, float dist_ratio,
                            const r3dm_kgraph_params* params, r3dm_graph** out);
/* 1 when, for the views registered in ctx, the EXHAUSTIVE matcher (r3dm_match_pairs) is expected to be at least as fast as the
 * graph matcher -- and it is exact: the views hold real-valued descriptors (LIOP-144, the descriptor Regard3D matches: the graph
 * search then gathers f32 rows and runs at 937 pairs/s on 16,384-row views where the exhaustive f32 kernel runs at 2,017 and the
 * split-f16 path at ~5,000, profiles/r02_p_ann_perf_f32rows.txt) of a length the tensor kernels serve (64 / 128 / 144 / 256) and no
 * view has more than 32,768 rows.  0 otherwise (integer-valued byte rows, where the v_dot4 graph search beats the f32 tiles; very
 * large views, where n log n beats n^2).  Binary views: 1 while no view exceeds 32,768 rows, the largest measured size at which the
 * faster of the two exhaustive Hamming paths is at least as fast as the Hamming graph matcher's default preset
 * (profiles/ann_hamming_perf.txt, 16 views: 3,084 against 2,476 pairs/s at 32,768 rows, lines 19 / 20; 816 against 829 at 65,536,
 * lines 26 / 27).  A host that only wants the arm's RESULT QUALITY (the reference's approximate arms 0-3,
 * 5-8 exist to save CPU time, not to lose matches) can use this to serve them with the exact matcher: the facade's default. */
int r3dm_exhaustive_is_faster(const r3dm_ctx* ctx);
/* ArrayMatcher_kgraph-shaped call: index `dataset`, 2 approximate nearest rows of every query row.  pair_i / pair_j
 * key the start-row stream (view ids in r3dm_match_pairs_kgraph).  out_idx -1 / out_dist +inf where the search
 * found fewer than two rows. */
int r3dm_kgraph_knn2(r3dm_ctx* ctx, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query,
                     uint32_t dim, const r3dm_kgraph_params* params, uint32_t pair_i, uint32_t pair_j,
                     int32_t* out_idx, float* out_dist);
/* Rows per view the graph matcher indexes: its index is the exact K-NN graph, built by an all-pairs scan of the view (quadratic in the
 * rows: 1-4 ms at 16 k rows, ~0.3 s at this bound).  r3dm_kgraph_index / r3dm_match_pairs_kgraph / r3dm_kgraph_knn2 return
 * R3DM_ERR_UNSUPPORTED for a larger view instead of indexing it in quadratic time (the reference's NN-descent builder,
 * src/thirdparty/kgraph/kgraph.cpp:703-999, is not built); the exhaustive matcher has no such bound. */
#define R3DM_KGRAPH_MAX_ROWS 131072u
/* the index of a registered view (built if necessary): adj_out = n x 64 rows (0xFFFFFFFF padded), deg_out = n.  Binary views: only
 * while r3dm_set_kgraph_hamming is on (the Hamming index). */
int r3dm_kgraph_index(r3dm_ctx* ctx, uint32_t view_id, uint32_t index_K, uint32_t* adj_out, uint32_t* deg_out);
/* forget the graph indices of all registered views, binary ones included (they are rebuilt on the next r3dm_match_pairs_kgraph); the reference builds
 * the index of image I inside every kgraph_match call (src/R3DComputeMatches.cpp:826-841), so a measurement that wants the same
 * accounting calls this between passes.  The registered descriptors stay. */
int r3dm_drop_indices(r3dm_ctx* ctx);

/* ---- binary views on the graph matcher: ArrayMatcher_kgraph<unsigned char, Hamming<unsigned char>> (the reference's plugin is generic
 * in its metric: src/utils/matcher_kgraph.h:33-37,60,90) ----
 * r3dm_set_kgraph_hamming: per-context switch, default 0.  While it is on, r3dm_match_pairs_kgraph (and its r3dm_multi_ form),
 * r3dm_kgraph_index, r3dm_index_kgraph_knn (the context passed is the one consulted) and r3dm_drop_indices serve R3DM_BIN views (29..32
 * or 61..64 bytes per row, the lengths a binary view can be registered with) as they serve float views: the index is the exact
 * index_K-nearest-neighbour graph under the Hamming distance, completed, ordered by (distance, row) and cut as for float rows; the search
 * is the same pool expansion with xor + popcount distances.  Both read the view's packed rows; no unpacked copy is made.  A Hamming
 * distance equals the squared L2 distance of the rows unpacked to 0 / 1 floats, so index and search are bit for bit those of the float
 * graph matcher on the unpacked rows.  Only the ratio rule differs: binary views take dist_ratio UNSQUARED (RegionsMatcherT's
 * b_squared_metric = false), in the search, in the exhaustively scanned part (views below 128 rows, search_P >= rows) and in the
 * preemptive gate alike.  A list that mixes float and binary views is cut into chunks by (type, length); pairs of different types are
 * skipped as ever.  While the switch is off every entry refuses binary views as before.  r3dm_stats counts the path as it counts the
 * float one (n_ann_built, n_ann_dist, ms_ann_build, ms_ann_search, n_match_launches, n_pairs; n_ann_rows16 / _rows8 / _dot8 stay 0).
 * HNSW and MRPT keep refusing binary views: hnswlib's L2Space is hard-wired in matcher_hnsw.h:70, MRPT projects floats. */
int r3dm_set_kgraph_hamming(r3dm_ctx* ctx, int enable);
/* what the packed-row kernels did since the context was created: indices built by the Hamming index kernel, launches of the Hamming
 * search (both tails) */
typedef struct {
    uint64_t n_index_builds;
    uint64_t n_search_launches;
} r3dm_kgraph_hamming_stats;
int r3dm_kgraph_hamming_report(const r3dm_ctx* ctx, r3dm_kgraph_hamming_stats* out);
/* r3dm_kgraph_knn2 / r3dm_kgraph_knn (below) for packed binary rows of n_bytes bytes (29..32 or 61..64), Hamming metric: same pair_i /
 * pair_j, parameters, outputs and bounds (k + search_P <= 63, R3DM_KGRAPH_MAX_ROWS); distances are the Hamming counts as floats, as
 * r3dm_knn2 reports them.  A dataset below 128 rows, or with search_P >= n_dataset, goes to the exhaustive Hamming 2-NN / k-list.
 * Their own opt-in: they need no switch. */
int r3dm_kgraph_knn2_bits(r3dm_ctx* ctx, const uint8_t* dataset, uint32_t n_dataset, const uint8_t* query, uint32_t n_query,
                          uint32_t n_bytes, const r3dm_kgraph_params* params, uint32_t pair_i, uint32_t pair_j,
                          int32_t* out_idx, float* out_dist);
int r3dm_kgraph_knn_bits(r3dm_ctx* ctx, const uint8_t* dataset, uint32_t n_dataset, const uint8_t* query, uint32_t n_query,
                         uint32_t n_bytes, const r3dm_kgraph_params* params, uint32_t pair_i, uint32_t pair_j, uint32_t k,
                         int32_t* out_idx, float* out_dist);

/* ---- approximate matching: the HNSW plugin path (matchingAlgorithm 6 / 7 / 8) ----
 * Replaces hnsw_match (src/R3DComputeMatches.cpp:497-593): per first view I an HNSW index over its descriptors
 * (ArrayMatcher_hnsw::Build, src/utils/matcher_hnsw.h:53-83 -> hnswlib::HierarchicalNSW, src/thirdparty/hnswlib/hnswlib/hnswalg.h),
 * per query row of J hnswlib's searchKnn(row, 2) with setEf(ef) (SearchNeighbours, matcher_hnsw.h:150-190), then the same ratio
 * test / de-duplication / pair rules as r3dm_match_pairs.  F32 / U8 descriptors of length 64, 128, 144 or 256 (hnswlib's
 * L2SqrSIMD16Ext, dim % 16 == 0), squared-L2 metric, at most 262,144 rows per view; views with fewer than 128 rows are scanned.
 *
 * SEARCH: hnswlib's algorithm step for step -- greedy descent through the upper layers, searchBaseLayerST on layer 0 with the two
 * priority queues moved as libstdc++'s heaps move them (ties between equally distant rows included), distances summed in the order
 * of hnswlib's AVX kernel.  On an index written by the reference-built library r3dm_hnsw_knn2_on_index returns hnswlib's own
 * rows and distances BIT FOR BIT (tests/test_gpu_hnsw.py against tests/golden/hnsw_ref_index.npz).
 * BUILD: hnswlib inserts rows one after another, each insertion searching the graph so far, and the reference adds rows 1 .. n-1
 * from an OpenMP loop -- its index differs from run to run.  Here the index is built in one batch, deterministically: hnswlib's
 * level draw (same engine and seed), per layer exact candidates (layer 0: the 64 closest of the exact 32-NN graph with reverse
 * edges; above: the 32 nearest members), hnswlib's neighbour-selection heuristic over them (at most 2M links on layer 0, M above),
 * free places refilled with the closest rejected candidates.  ef_construction has no role in it (accepted, ignored).  At the
 * reference's ef the batch-built index finds the true nearest row at least as often as the reference-built one (same tests;
 * CPU model: oracle/hnsw.c orc_hnsw_build_batch, GPU parity with it bit-exact). */
typedef struct {
    uint32_t M;                /* links per row above layer 0 (2M on layer 0), 2..32   (reference presets 5 / 15 / 19)        */
    uint32_t ef_construction;  /* the reference's build beam (112 / 112 / 100): unused by the batch construction             */
    uint32_t ef;               /* search beam, 1..512 (searchKnn uses max(ef, 2))      (reference presets 5 / 10 / 15)        */
    uint32_t seed;             /* level draw (hnswlib: random_seed = 100)                                                    */
} r3dm_hnsw_params;
/* preset = matchingAlgorithm - 6 of the reference: 0 "HNSW fast", 1 "medium", anything else "precise" */
int r3dm_hnsw_preset(int preset, r3dm_hnsw_params* out);
int r3dm_match_pairs_hnsw(r3dm_ctx* ctx, const uint32_t* pairs_ij, uint64_t n_pairs, float dist_ratio,
                          const r3dm_hnsw_params* params, r3dm_graph** out);
/* ArrayMatcher_hnsw-shaped call: index `dataset` (>= 128 rows), searchKnn(row, 2) of every query row.  out_idx -1 / out_dist +inf
 * where the search found fewer than two rows. */
int r3dm_hnsw_knn2(r3dm_ctx* ctx, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query,
                   uint32_t dim, const r3dm_hnsw_params* params, int32_t* out_idx, float* out_dist);
/* An HNSW index as arrays in hnswlib's own shape: links0 = n x (1 + 2M) ints (count, then links, -1 padded), up_off = n + 1 ints
 * (first upper-layer row of a node; layer L >= 1 of node i is row up_off[i] + L - 1), up_links = up_rows x (1 + M) ints. */
typedef struct {
    uint32_t M;
    const int32_t* links0;
    const int32_t* up_off;
    const int32_t* up_links;
    uint32_t up_rows;
    int32_t enterpoint, maxlevel;
} r3dm_hnsw_arrays;
/* searchKnn(row, 2) with setEf(ef) on an index handed over as arrays -- e.g. one written by hnswlib itself (any n_dataset >= 2).
 * The arrays are validated (R3DM_ERR_INVALID when a link or an offset is out of range). */
int r3dm_hnsw_knn2_on_index(r3dm_ctx* ctx, const float* dataset, uint32_t n_dataset, uint32_t dim, const r3dm_hnsw_arrays* index,
                            const float* query, uint32_t n_query, uint32_t ef, int32_t* out_idx, float* out_dist);
/* the index of a registered view (built if necessary) in that shape; up_links holds up_cap rows, *up_rows receives the number needed */
int r3dm_hnsw_index(r3dm_ctx* ctx, uint32_t view_id, const r3dm_hnsw_params* params, int32_t* links0, int32_t* up_off,
                    int32_t* up_links, uint32_t up_cap, uint32_t* up_rows, int32_t* enterpoint, int32_t* maxlevel);

/* ---- MRPT plugin path (matchingAlgorithm 5) ----
 * mrpt_match (src/R3DComputeMatches.cpp:423-491): per first view I an index of n_trees random projection trees of depth `depth` over
 * its descriptors (ArrayMatcher_mrpt::Build, src/utils/matcher_mrpt.h:76-128 -> Mrpt::grow, src/thirdparty/mrpt/mrpt.h:84-137: sparse
 * random vectors of density 1 / sqrt(dim), every tree level splits its nodes at the median projection), per query row of J
 * Mrpt::query(row, 2, votes) (mrpt.h:661-728: one leaf per tree, the rows that collect >= votes votes are measured exactly, the two
 * nearest kept; once more with votes - 1 when fewer than two rows were elected, matcher_mrpt.h:224-232; a query that still has none is
 * dropped), then the ratio test ON THE SQUARE ROOTS the index returns with the un-squared ratio (RegionsMatcherT(regions, false),
 * src/R3DComputeMatches.cpp:461) and the de-duplication / pair rules every arm shares.  The index is built on the device
 * (kernels_mrpt.hip); parity is with the CPU model oracle/mrpt.c bit for bit.  What cannot match a reference build -- and could not
 * be pinned to one, mrpt.h being Eigen code: the random vectors are drawn from a counter-based stream instead of std::mt19937 with
 * implementation-defined distributions (same density, same N(0, 1) values), rows whose projection EQUALS a node's median go left in
 * (projection, row) order where std::nth_element leaves them anywhere, candidates are measured with the reference's brute-force
 * metric in its summation order.  Views with fewer than 128 rows are scanned exhaustively; descriptor lengths: any multiple of 4
 * up to 512; at most 131,072 rows per indexed view. */
typedef struct {
    uint32_t n_trees;          /* 1..255                                   (reference: 26)                                         */
    uint32_t depth;            /* 1..6; clamped per view to max(2, min(depth, floor(log2 n) - 1)) as ArrayMatcher_mrpt::Build does   (6) */
    uint32_t votes;            /* rows with at least this many of the n_trees votes are candidates, 1..n_trees   (5)               */
    float    density;          /* share of non-zero entries of a random vector; <= 0: 1 / sqrt(dim), mrpt.h's default   (0.088: set but never passed on by the reference) */
    uint64_t seed;             /* of the counter-based stream the random vectors are drawn from                                     */
} r3dm_mrpt_params;
int r3dm_mrpt_preset(r3dm_mrpt_params* out);               /* 26 / 6 / 5 / default density / seed 0 */
int r3dm_match_pairs_mrpt(r3dm_ctx* ctx, const uint32_t* pairs_ij, uint64_t n_pairs, float dist_ratio,
                          const r3dm_mrpt_params* params, r3dm_graph** out);
/* ArrayMatcher_mrpt-shaped call: index `dataset` (>= 128 rows), the two nearest elected rows of every query row.  out_dist = the
 * SQUARE ROOTS of the squared L2 distances, as Mrpt::query returns them; out_idx -1 / out_dist -1 for a query the reference drops. */
int r3dm_mrpt_knn2(r3dm_ctx* ctx, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query,
                   uint32_t dim, const r3dm_mrpt_params* params, int32_t* out_idx, float* out_dist);
/* the index of a registered view (built if necessary): R = n_trees * depth x dim (zeros where the sparse matrix has no entry),
 * splits = n_trees x (2^depth - 1) in heap order, leaves = n_trees x n rows leaf after leaf, leaf_first = 2^depth + 1 offsets;
 * *depth_out = the clamped depth.  Any output may be NULL.  The arrays must hold the sizes of depth = params->depth. */
int r3dm_mrpt_index(r3dm_ctx* ctx, uint32_t view_id, const r3dm_mrpt_params* params, float* R, float* splits, int32_t* leaves,
                    int32_t* leaf_first, uint32_t* depth_out);

/* ---- k neighbours, k = 1 .. R3DM_KNN_MAX, through the three approximate matchers: ArrayMatcher::SearchNeighbours(.., NN) of
 * ArrayMatcher_kgraph / _hnsw / _mrpt with any NN (sparams.K = NN, matcher_kgraph.h:205-251; searchKnn(q, NN), matcher_hnsw.h:138-173;
 * Mrpt::query(q, NN, votes), matcher_mrpt.h:186-251) ----
 * Each entry takes the arguments of its *_knn2 sibling plus k and follows the sibling's rules for lengths, row counts and small
 * datasets; out_idx / out_dist hold k entries per query at [q * k + j].  R3DM_ERR_INVALID: k < 1, k > R3DM_KNN_MAX, n_dataset < k
 * (the plugins' "NN > rows" rule), null pointers.  k = 2 returns the sibling's bits.  The search itself depends on k:
 *   KGraph  the pool holds k + search_P entries (KGraphImpl::search, kgraph.cpp:418), one per lane of a wavefront: k + search_P > 63
 *           is R3DM_ERR_INVALID.  Output: the first min(L, k) pool entries, ascending; -1 / +inf behind them.
 *   HNSW    the beam is max(ef, k) (hnswalg.h:765) -- the "fast" preset (ef 5) searches a wider beam at k = 8.  Output: the beam popped
 *           down to k, ascending by (distance, row); -1 / +inf for rows the search did not find.
 *   MRPT    the election is the sibling's; the k nearest elected rows by (distance, row) are kept, the retry with votes - 1 runs when
 *           fewer than k rows were elected, and a query still short of k is dropped: all k entries -1 / -1.  Distances are square
 *           roots.  (The reference's autotune mode is not served.)
 * The r3dm_match_pairs_* ratio rule stays on 2-lists.  The ANN counters of r3dm_stats (n_ann_dist, ms_ann_build, ms_ann_search,
 * n_hnsw_launches, n_hnsw_retries, ...) describe these calls as they describe the siblings. */
int r3dm_kgraph_knn(r3dm_ctx* ctx, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query,
                    uint32_t dim, const r3dm_kgraph_params* params, uint32_t pair_i, uint32_t pair_j, uint32_t k,
                    int32_t* out_idx, float* out_dist);
int r3dm_hnsw_knn(r3dm_ctx* ctx, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query,
                  uint32_t dim, const r3dm_hnsw_params* params, uint32_t k, int32_t* out_idx, float* out_dist);
int r3dm_hnsw_knn_on_index(r3dm_ctx* ctx, const float* dataset, uint32_t n_dataset, uint32_t dim, const r3dm_hnsw_arrays* index,
                           const float* query, uint32_t n_query, uint32_t ef, uint32_t k, int32_t* out_idx, float* out_dist);
int r3dm_mrpt_knn(r3dm_ctx* ctx, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query,
                  uint32_t dim, const r3dm_mrpt_params* params, uint32_t k, int32_t* out_idx, float* out_dist);
/* "Build once, search per query block" for the three matchers: the arm's structure lives on an r3dm_index (F32 / U8 rows).
 * It is built on FIRST USE, under the index's lock, from that call's build parameters -- KGraph: index_K; HNSW: M, ef_construction,
 * seed; MRPT: n_trees, depth, density, seed -- and never again: a later call whose build parameters differ is R3DM_ERR_INVALID (nothing
 * is rebuilt under another context's search).  Search parameters (search_P, search_S, seed; ef; votes) are free per call.  Any context
 * of the index's device may search, several at a time, as for r3dm_index_knn; an index may hold all three structures.  An index of
 * fewer than 128 rows (KGraph: or of at most search_P rows) is answered by r3dm_index_knn, exactly, as r3dm_match_pairs_* scans such
 * views (MRPT too: such an answer holds squared distances and drops no query).  r3dm_stats.ms_ann_build / n_ann_built are 0 for every call but the one that built. */
/* (a binary index: served by r3dm_index_kgraph_knn while r3dm_set_kgraph_hamming is on in the context passed; queries are packed rows) */
int r3dm_index_kgraph_knn(r3dm_ctx* ctx, const r3dm_index* index, const r3dm_kgraph_params* params, const void* query, uint32_t n_query,
                          uint32_t pair_i, uint32_t pair_j, uint32_t k, int32_t* out_idx, float* out_dist);
int r3dm_index_hnsw_knn(r3dm_ctx* ctx, const r3dm_index* index, const r3dm_hnsw_params* params, const void* query, uint32_t n_query,
                        uint32_t k, int32_t* out_idx, float* out_dist);
int r3dm_index_mrpt_knn(r3dm_ctx* ctx, const r3dm_index* index, const r3dm_mrpt_params* params, const void* query, uint32_t n_query,
                        uint32_t k, int32_t* out_idx, float* out_dist);

/* ---- keypoint detection: Fast-A-KAZE ----
 * The "Fast-AKAZE" arm of Regard3DFeatures::detectKeypoints (src/Regard3DFeatures.cpp:596-617): cv::AKAZE2::create() with its
 * defaults (src/thirdparty/fast-akaze/AKAZEConfig.h:18-43: 4 octaves x 4 sublevels, PM_G2 diffusivity), setThreshold(threshold),
 * detect() = nonlinear scale space by fast explicit diffusion + determinant-of-Hessian extrema + sub-pixel refinement + main
 * orientation (src/thirdparty/fast-akaze/AKAZEFeatures.cpp:245-382), then the angle conversion of :604-613.
 * image: height x width floats in [0, 1] (gray / 255, as R3DFeaturesThread.cpp:163-191 prepares it), host or device pointer.
 * keypoints_out: cap x 4 floats (x, y, size, angle in degrees) -- exactly what r3dm_extract_liop takes; responses_out optional.
 * *n_out = number detected (may exceed cap; only the first cap are written, in the reference's order: by evolution level, then
 * by detection order).  The reference serialises this stage with a semaphore (one image at a time). */
int r3dm_detect_akaze(r3dm_ctx* ctx, const float* image, uint32_t width, uint32_t height, float threshold,
                      float* keypoints_out, float* responses_out, uint32_t cap, uint32_t* n_out);

/* The same over a BATCH of n_images same-size images in ONE pass of the detector (no reference counterpart: the reference admits one
 * image at a time into this stage, src/Regard3DFeatures.cpp:71-125).  The ~550 dependent launches of the scale space depend on the
 * image size only, so they serve all images at once (one image alone waits for launch latency below the first octave), and nothing
 * in the chain visits the host.  images[b]: height x width floats, host or device; keypoints_out[b]: cap x 4
 * floats; responses_out: NULL, or n_images pointers (each may be NULL); n_out[b] as above.  Results per image are bit-identical
 * to r3dm_detect_akaze on that image. */
int r3dm_detect_akaze_batch(r3dm_ctx* ctx, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                            float threshold, float* const* keypoints_out, float* const* responses_out, uint32_t cap, uint32_t* n_out);

/* cv::AKAZE2::detectAndCompute with DESCRIPTOR_MLDB (src/thirdparty/fast-akaze/akaze.cpp:171-221; the binary descriptors of
 * BASELINE config C3): keypoints as above plus the full MLDB descriptor of each -- 3 grids (2x2, 3x3, 4x4) x 3 channels, all
 * pairwise comparisons = 486 bits packed LSB first into 61 bytes (AKAZEFeatures.cpp:1790-1909).  descriptors_out: cap x 61
 * bytes, ready for r3dm_set_image(..., dim 61, R3DM_BIN). */
int r3dm_detect_akaze_mldb(r3dm_ctx* ctx, const float* image, uint32_t width, uint32_t height, float threshold,
                           float* keypoints_out, unsigned char* descriptors_out, uint32_t cap, uint32_t* n_out);

/* The same over a BATCH of n_images same-size images: one pass of the detector (r3dm_detect_akaze_batch), then ONE MLDB launch over the
 * keypoints of all images (a keypoint names its evolution level as image x levels + level; the level planes of every image stay on
 * the device until the launch).  keypoints_out[b]: cap x 4 floats, descriptors_out[b]: cap x 61 bytes; min(count, cap) rows are written
 * per image, n_out[b] = number detected (may exceed cap).  Results per image are bit-identical to r3dm_detect_akaze_mldb on that
 * image, for any n_images, images without keypoints included. */
int r3dm_detect_akaze_mldb_batch(r3dm_ctx* ctx, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                                 float threshold, float* const* keypoints_out, unsigned char* const* descriptors_out, uint32_t cap,
                                 uint32_t* n_out);

/* Fast-A-KAZE keypoints with their M-SURF-64 rows, the float descriptor of the vendored Fast-A-KAZE (MSURF_Descriptor_64_InvokerV2,
 * src/thirdparty/fast-akaze/AKAZEFeatures.cpp:1431-1544; OpenMVG's AKAZE_FLOAT): 64 floats per keypoint, unit length.  Shapes as the
 * MLDB entries above; descriptors_out (descriptors_out[b]) holds cap x 64 floats.
 * THE BORDER IS THE DESCRIPTOR'S: as the reference does when it is configured for the KAZE descriptors (:78-84,105,112), the detector
 * of these entries runs on a level table whose borders are fRound(12 sqrt(2) sigma_size) + 1, not MLDB's 10 sqrt(2): levels are cut
 * sooner on small images and keypoints near the frame are not found, so the keypoints are NOT those of r3dm_detect_akaze(_mldb) there.
 * The exponential of the Gaussian weights is the library's own (evaluated in double, within 0.5 + 2^-28 ulp of exp; the reference
 * calls libm's expf, which a device cannot reproduce bit for bit): rows differ from a CPU run of the reference in the last bits only
 * (DESIGN.md section 4.8).  A keypoint whose window holds no gradient has length 0 and a row of NaN, as in the reference. */
int r3dm_detect_akaze_msurf(r3dm_ctx* ctx, const float* image, uint32_t width, uint32_t height, float threshold,
                            float* keypoints_out, float* descriptors_out, uint32_t cap, uint32_t* n_out);
int r3dm_detect_akaze_msurf_batch(r3dm_ctx* ctx, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                                  float threshold, float* const* keypoints_out, float* const* descriptors_out, uint32_t cap,
                                  uint32_t* n_out);

/* ---- keypoint detection: classic A-KAZE ----
 * The "AKAZE" arm of Regard3DFeatures::detectKeypoints (src/Regard3DFeatures.cpp:578-589), the GUI's default detector:
 * cv::AKAZE::create(DESCRIPTOR_MLDB, 0, 3, threshold, 4, 4, DIFF_PM_G2) + detect(), restated as libAKAZE, the classic code of the
 * reference tree (src/thirdparty/akaze/lib/, AKAZEConfig.h defaults): nonlinear scale space by FED, scale-normalised multiscale
 * derivatives, determinant-of-Hessian extrema with libAKAZE's sequential kpts_aux rule, the upper-level filter, sub-pixel refinement.
 * Orientation: libAKAZE's Feature_Detection leaves the angle 0, OpenCV 4's detect() assigns one; this arm computes
 * Compute_Main_Orientation on the level's multiscale Lx / Ly and returns it in DEGREES in [0, 360) with NO + 90 (Regard3D converts
 * the Fast arm's angle only).  Parity with OpenCV is UNPINNED (its 4.x extrema search is a reworked parallel form): DESIGN.md section 7.
 * Arguments and output layout as r3dm_detect_akaze: keypoints_out cap x 4 floats (x, y, size, angle in degrees), responses_out optional,
 * *n_out may exceed cap, output in the reference's order (kpts_aux slot order). */
int r3dm_detect_akaze_classic(r3dm_ctx* ctx, const float* image, uint32_t width, uint32_t height, float threshold,
                              float* keypoints_out, float* responses_out, uint32_t cap, uint32_t* n_out);

/* The same over a batch of n_images same-size images in one pass (arguments as r3dm_detect_akaze_batch); results per image are
 * bit-identical to r3dm_detect_akaze_classic on that image. */
int r3dm_detect_akaze_classic_batch(r3dm_ctx* ctx, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                                    float threshold, float* const* keypoints_out, float* const* responses_out, uint32_t cap,
                                    uint32_t* n_out);

/* Component-size histogram of the classic arm's parallel kpts_aux walk since r3dm_create: hist[k] (32 entries) counts the connected
 * components of "same or adjacent level and within size" with 2^k .. 2^(k+1) - 1 candidates. */
int r3dm_akaze_classic_components(const r3dm_ctx* ctx, uint64_t* hist);

/* The detector arm of the features entries (r3dm_extract_features_to_files, r3dm_extract_features_batch, r3dm_multi_extract_features
 * and _ex): Regard3D's keypointDetectorList_ of one entry.  R3DM_DETECTOR_FAST_AKAZE (the default) is r3dm_detect_akaze,
 * R3DM_DETECTOR_AKAZE the classic arm r3dm_detect_akaze_classic (the GUI's default, keypointDetectorType 0).  Both feed LIOP with
 * kpSizeFactor 8 (getKpSizeFactor, src/Regard3DFeatures.cpp:691-717); the classic arm's angle is written as it detects it (degrees, no
 * + 90).  Everything after the detector -- files, sink, deferred files, skip rule -- is the same.  Other values: R3DM_ERR_INVALID. */
#define R3DM_DETECTOR_FAST_AKAZE 0
#define R3DM_DETECTOR_AKAZE 1
int r3dm_set_keypoint_detector(r3dm_ctx* ctx, int arm);

/* The descriptor arm of the same features entries.  R3DM_DESCRIPTOR_LIOP (the default) is what Regard3D computes: LIOP, 144 floats per
 * keypoint.  R3DM_DESCRIPTOR_MLDB is the second descriptor of the vendored Fast-A-KAZE, which Regard3D itself never computes: the full
 * MLDB-486 of r3dm_detect_akaze_mldb, for BASELINE config C3 (binary rows, Hamming brute force) from photographs.  Under it the .feat
 * of an image is byte for byte the one the LIOP arm writes (same detector, same angle conversion, same text) and its .desc is the
 * 8-byte count followed by count x 61 bytes (KeypointSet::saveToBinFile with Descriptor<unsigned char, 61>) -- what the facade reads
 * under setRegionsType(R3DM_BIN, 61).  Skip rule, sink, deferred files and scheduling are shared.  MLDB needs the Fast arm's level
 * planes: together with R3DM_DETECTOR_AKAZE a features call returns R3DM_ERR_UNSUPPORTED (r3dm_last_error names the arm), computes
 * nothing and leaves both switches as they are.
 * R3DM_DESCRIPTOR_MSURF is the M-SURF-64 of r3dm_detect_akaze_msurf: same .feat text format, a .desc of the 8-byte count followed by
 * count x 64 floats (the LIOP layout with 64 columns: what the facade reads under setRegionsType(R3DM_F32, 64)), the sink's pointer
 * at n_features x 64 floats.  The detector then runs on the M-SURF level table (wider borders, see r3dm_detect_akaze_msurf), so the
 * .feat of an image near whose frame keypoints lie differs from the other arms'.  With R3DM_DETECTOR_AKAZE it is refused exactly as
 * MLDB is.  Its value is 3: 2 stays unassigned and refused (it is the value the suite holds to R3DM_ERR_INVALID).
 * Other values: R3DM_ERR_INVALID. */
#define R3DM_DESCRIPTOR_LIOP 0
#define R3DM_DESCRIPTOR_MLDB 1
#define R3DM_DESCRIPTOR_MSURF 3
int r3dm_set_descriptor_arm(r3dm_ctx* ctx, int arm);

/* ---- the per-image work item of the features stage ----
 * R3DFeaturesThread::processWorkItem (src/threads/R3DFeaturesThread.cpp:123-210) after cv::imread: 8-bit BGR -> float / 255 ->
 * BGR2GRAY (r3dm_gray_from_bgr8; bgr = height x width x 3 bytes, gray_out = height x width floats, host or device), then
 * Regard3DFeatures::detectAndExtract with the "Fast-AKAZE" detector + LIOP and KeypointSet::saveToBinFile
 * (src/keypointSet.hpp:61-67): <feat_path> gets one "x y scale orientation" line per feature (scale = size / 2), <desc_path>
 * an 8-byte count followed by count x 144 floats -- the files r3dm_compute_matches_dir / the facade read back.  (Under
 * R3DM_DESCRIPTOR_MLDB: count x 61 bytes, under R3DM_DESCRIPTOR_MSURF: count x 64 floats, r3dm_set_descriptor_arm.)
 * As in the reference (:139-142) the work item does nothing when BOTH files already exist (n_features = rows of the existing .desc).
 * Image decoding (cv::imread) stays with the caller. */
int r3dm_gray_from_bgr8(r3dm_ctx* ctx, const unsigned char* bgr, uint32_t width, uint32_t height, float* gray_out);
int r3dm_extract_features_to_files(r3dm_ctx* ctx, const float* gray, uint32_t width, uint32_t height, float threshold,
                                   const char* feat_path, const char* desc_path, uint32_t* n_features);

/* n_images same-size images through the work item in one pass: detector batch (above) -> the angle and LIOP patch map of every
 * keypoint on the host (atan2f / cos / sin of the host libm, as the reference; 32 bytes per keypoint up, 24 down) -> ONE patch
 * extraction launch and ONE LIOP launch over the keypoints of all images -> files.  grays: n_images pointers to height x width
 * floats, or NULL and bgrs: n_images pointers to height x width x 3 bytes (BGR as cv::imread decodes; converted on the device as
 * r3dm_gray_from_bgr8 does); host or device.  No skip rule here: every image is computed and its two files (re)written. */
int r3dm_extract_features_batch(r3dm_ctx* ctx, uint32_t n_images, const float* const* grays, const unsigned char* const* bgrs,
                                uint32_t width, uint32_t height, float threshold, const char* const* feat_paths,
                                const char* const* desc_paths, uint32_t* n_features);

/* ---- descriptor extraction: LIOP on pre-extracted patches ----
 * r3d_vl_liopdesc_process of the vendored VLFeat copy (src/thirdparty/liop/vl_liop.c:465-580) as Regard3D
 * calls it per keypoint (src/Regard3DFeatures.cpp:727-752,827: new_basic(41) -> 4 neighbours, 6 bins, radius 6):
 * patches = n x 41 x 41 floats (the warped + blurred patch of every keypoint, row-major), desc_out = n x 144
 * floats, non-negative, unit L2 norm (all-zero for a constant patch).  Host or device pointers.
 * n_resorted (optional) receives the number of patches with equal intensities that went through the exact
 * re-sort.  Results are bit-identical to the reference routine. */
int r3dm_liop_describe_patches(r3dm_ctx* ctx, const float* patches, uint32_t n, uint32_t side, float* desc_out,
                               uint32_t* n_resorted);

/* ---- descriptor extraction: keypoints -> LIOP descriptors ----
 * The per-keypoint loop of Regard3DFeatures::extractLIOPFeatures (src/Regard3DFeatures.cpp:719-861; serial in the
 * reference): for every keypoint a 41x41 patch by inverse affine warp (scale = size/41 * kpSizeFactor,
 * angle = -90 - kp.angle, :768-803) + Gaussian blur sigma 1.2 (:807), then LIOP.  image: h x w floats (gray / 255,
 * as R3DFeaturesThread.cpp:163-191 prepares it); keypoints: n x 4 floats (x, y, size, angle in degrees) as left by
 * detectKeypoints (:574-684); kp_size_factor: getKpSizeFactor(detector) (:691-717, 8.0 for A-KAZE).
 * desc_out: n x 144 floats.  patches_out (optional): n x 41 x 41 floats.  Host or device pointers. */
int r3dm_extract_liop(r3dm_ctx* ctx, const float* image, uint32_t width, uint32_t height,
                      const float* keypoints, uint32_t n, float kp_size_factor, float* desc_out, float* patches_out);

/* ---- match graph (PairWiseMatches) ---- */
uint64_t          r3dm_graph_num_pairs(const r3dm_graph* g);
uint64_t          r3dm_graph_num_matches(const r3dm_graph* g);
const uint32_t*   r3dm_graph_pairs(const r3dm_graph* g);     /* n_pairs x 2                        */
const uint64_t*   r3dm_graph_offsets(const r3dm_graph* g);   /* n_pairs + 1 (CSR into matches)     */
const r3dm_match* r3dm_graph_matches(const r3dm_graph* g);
void              r3dm_graph_free(r3dm_graph* g);
/* build a graph from host CSR arrays (copied); used to re-assemble shards after the all-gather */
int r3dm_graph_from_csr(const uint32_t* pairs_ij, uint64_t n_pairs, const uint64_t* offsets,
                        const r3dm_match* matches, r3dm_graph** out);
/* merge several graphs (e.g. one per rank) into one ordered by (I, J) */
int r3dm_graph_merge(const r3dm_graph* const* parts, uint32_t n_parts, r3dm_graph** out);

/* ---- multi-GPU, single process: one context per device, one host thread per device ----
 * For a C++ host like Regard3D itself (one process, /root/reference/src/R3DComputeMatches.cpp:437-489 treats the pairs of the
 * collection as independent OpenMP iterations; so does OpenMVG's filter loop, :2099).  r3dm_multi_create opens one context per
 * entry of device_ids (an id may repeat: two contexts on one GPU); r3dm_multi_set_image replicates a view on every device;
 * r3dm_multi_match_pairs deals the pair list to the devices by rows of I in snake order (r3dm_shard_pairs: rows sorted by
 * decreasing pair count, dealt 0..W-1, W-1..0, ... -- cost-balanced, the pairs of one I stay on one device), runs
 * r3dm_match_pairs on every device from its own host thread and merges the graphs; the filters deal the putative pairs
 * longest list first.  No collective is involved (the graph is reassembled in host memory, where PairWiseMatches lives);
 * the multi-PROCESS route -- one rank per GPU, one RCCL all-gather -- is regard3d_amd/dist.py.  Results are identical to a
 * single-device run (every per-pair computation is independent of the device that runs it). */
typedef struct r3dm_multi r3dm_multi;
int  r3dm_multi_create(const int* device_ids, int n_dev, r3dm_multi** out);
void r3dm_multi_destroy(r3dm_multi* m);
int  r3dm_multi_num_devices(const r3dm_multi* m);
r3dm_ctx* r3dm_multi_ctx(r3dm_multi* m, int k);            /* the k-th device's context (statistics, reports) */
const char* r3dm_multi_last_error(const r3dm_multi* m);
int r3dm_multi_set_image(r3dm_multi* m, uint32_t view_id, uint32_t width, uint32_t height,
                         const void* desc, uint32_t n, uint32_t dim, r3dm_dtype dtype, const float* xy);
/* how the views registered so far travelled: a view crosses PCIe once (host -> the first context's device; not at all when the
 * caller's buffers are device memory) and reaches the other devices by hipMemcpyPeerAsync (xGMI where peer access exists) */
int r3dm_multi_transfer_counts(const r3dm_multi* m, uint64_t* host_uploads, uint64_t* peer_copies);
int r3dm_multi_set_intrinsics(r3dm_multi* m, uint32_t view_id, const double* K);
int r3dm_multi_clear_images(r3dm_multi* m);
int r3dm_multi_set_integer_mfma(r3dm_multi* m, int enable);
int r3dm_multi_set_mutual_matching(r3dm_multi* m, int enable);      /* r3dm_set_mutual_matching on every context */
int r3dm_multi_set_symmetric_ratio(r3dm_multi* m, int enable);      /* r3dm_set_symmetric_ratio on every context (r3dm_symmetric_ratio_report: per context, through r3dm_multi_ctx) */
int r3dm_multi_set_kgraph_hamming(r3dm_multi* m, int enable);       /* r3dm_set_kgraph_hamming on every context */
int r3dm_multi_set_prefix_pruning(r3dm_multi* m, int enable);       /* r3dm_set_prefix_pruning on every context */
int r3dm_multi_get_prefix_pruning_counts(r3dm_multi* m, uint64_t out[2]);      /* summed over the contexts' last calls */
int r3dm_multi_get_pair_filter_counts(r3dm_multi* m, uint64_t* out);           /* summed over the contexts' last calls */
int r3dm_multi_set_half_filter(r3dm_multi* m, int enable);          /* r3dm_set_half_filter on every context */
int r3dm_multi_get_half_filter_counts(r3dm_multi* m, uint64_t* out);           /* summed over the contexts' last calls */
int r3dm_multi_get_level2_skip_counts(r3dm_multi* m, uint64_t* out);           /* summed over the contexts' last calls */
int r3dm_multi_set_min_tile_test(r3dm_multi* m, int enable);        /* r3dm_set_min_tile_test on every context */
int r3dm_multi_get_min_tile_test_counts(r3dm_multi* m, uint64_t out[2]);       /* summed over the contexts' last calls */
int r3dm_multi_set_half_prefix(r3dm_multi* m, int enable);          /* r3dm_set_half_prefix on every context */
int r3dm_multi_get_half_prefix_counts(r3dm_multi* m, uint64_t out[2]);         /* summed over the contexts' last calls */
int r3dm_multi_set_view_priority(r3dm_multi* m, uint32_t view_id, const float* priority, uint32_t n);      /* on every context, as r3dm_multi_set_image replicates the view */
int r3dm_multi_set_preemptive_matching(r3dm_multi* m, int enable, uint32_t head_rows, uint32_t min_matches);   /* on every context: each gates its own shard */
int r3dm_multi_set_match_budget(r3dm_multi* m, int enable, uint32_t max_rows);                                 /* on every context: each budgets its own shard */
int r3dm_multi_match_pairs(r3dm_multi* m, const uint32_t* pairs_ij, uint64_t n_pairs,
                           float dist_ratio, int squared_metric, r3dm_graph** out);
/* the same deal for the graph matcher (kgraph_match, config C5): a device builds the index of every image I whose row it owns */
int r3dm_multi_match_pairs_kgraph(r3dm_multi* m, const uint32_t* pairs_ij, uint64_t n_pairs, float dist_ratio,
                                  const r3dm_kgraph_params* params, r3dm_graph** out);
/* ... and for the HNSW matcher (hnsw_match, matchingAlgorithm 6..8) */
int r3dm_multi_match_pairs_hnsw(r3dm_multi* m, const uint32_t* pairs_ij, uint64_t n_pairs, float dist_ratio,
                                const r3dm_hnsw_params* params, r3dm_graph** out);
/* ... and for the MRPT matcher (mrpt_match, matchingAlgorithm 5) */
int r3dm_multi_match_pairs_mrpt(r3dm_multi* m, const uint32_t* pairs_ij, uint64_t n_pairs, float dist_ratio,
                                const r3dm_mrpt_params* params, r3dm_graph** out);
int r3dm_multi_filter_F(r3dm_multi* m, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                        uint64_t seed, r3dm_graph** out, double* F_out);
int r3dm_multi_filter_H(r3dm_multi* m, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                        uint64_t seed, r3dm_graph** out, double* H_out);
int r3dm_multi_filter_E(r3dm_multi* m, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                        uint64_t seed, uint32_t min_count, float min_ratio, r3dm_graph** out, double* E_out);
/* r3dm_set_guided_matching on every device context: r3dm_multi_filter_* then return guided lists */
int r3dm_multi_set_guided_matching(r3dm_multi* m, int enable, double ratio_F, double ratio_E, double ratio_H);
/* r3dm_set_keypoint_detector on every device context: the arm of r3dm_multi_extract_features and _ex */
int r3dm_multi_set_keypoint_detector(r3dm_multi* m, int arm);
/* r3dm_set_descriptor_arm on every device context: what r3dm_multi_extract_features and _ex describe the keypoints with */
int r3dm_multi_set_descriptor_arm(r3dm_multi* m, int arm);
/* The features stage over an image list: R3DFeaturesThread::extractFeaturesAndDescriptors (src/threads/R3DFeaturesThread.cpp:38-121),
 * whose worker pool pulls images off a work list and runs processWorkItem on each.  Here every context of `m` is a worker that pulls
 * BATCHES of same-size images (r3dm_extract_features_batch: up to 8 per detector pass): create
 * the r3dm_multi with one device id repeated K times to keep K batches in flight on that GPU (K streams + K sets of work buffers;
 * the reference admits one image at a time into the A-KAZE scale space, src/Regard3DFeatures.cpp:71-125 -- HBM does not need that),
 * or with several device ids to spread the list over the GPUs of a node.  Images whose <feat> AND <desc> files already exist are
 * skipped like processWorkItem does (:139-142); skipped[i] (optional) says so and n_features[i] (optional) then carries the row
 * count of the existing .desc.  grays[i]: height x width floats, host or device.  err (optional) receives the first failure. */
int r3dm_multi_extract_features(r3dm_multi* m, uint32_t n_images, const float* const* grays, const uint32_t* widths,
                                const uint32_t* heights, float threshold, const char* const* feat_paths,
                                const char* const* desc_paths, uint32_t* n_features, uint32_t* skipped, char* err, size_t err_cap);
/* the general form: per image either grays[i] (gray / 255 floats) or bgrs[i] (decoded 8-bit BGR, what cv::imread hands
 * processWorkItem, src/threads/R3DFeaturesThread.cpp:163-165: the float / 255 -> BGR2GRAY conversion then runs on the device);
 * either array may be NULL as a whole.  batch: images per detector pass of a worker, 0 = the default (8; fewer when HBM or the list
 * is short).  A worker's batch is a run of images of one size and one kind. */
int r3dm_multi_extract_features_ex(r3dm_multi* m, uint32_t n_images, const float* const* grays, const unsigned char* const* bgrs,
                                   const uint32_t* widths, const uint32_t* heights, float threshold, const char* const* feat_paths,
                                   const char* const* desc_paths, uint32_t* n_features, uint32_t* skipped, uint32_t batch,
                                   char* err, size_t err_cap);
/* owner_out[p] = the device / rank (0..world-1) that the snake deal gives pair p.  Pure host code (no GPU needed). */
int r3dm_shard_pairs(const uint32_t* pairs_ij, uint64_t n_pairs, uint32_t world, uint32_t* owner_out);

/* ---- multi-GPU, one process per GPU: the ONE collective of the path ----
 * Every rank matches and filters its share of the pair list (r3dm_shard_pairs) and then calls r3dm_allgather_graphs: one
 * ncclAllGather of the per-rank sizes (8 bytes each) and one of the packed graphs padded to the largest rank, over RCCL (xGMI between
 * the GPUs of a node); every rank ends up with the graphs of the whole collection, ordered by (I, J) -- the std::map the reference's
 * OpenMP threads fill under `omp critical` (/root/reference/src/R3DComputeMatches.cpp:465,481-487).  The communicator is RCCL's own:
 * rank 0 draws an id (r3dm_comm_unique_id, 128 bytes) and hands it to the other ranks by whatever the host has (MPI_Bcast, a file,
 * torch.distributed), every rank calls r3dm_comm_create(id, rank, world, device).  RCCL is bound at run time (dlopen): without
 * librccl.so these calls return R3DM_ERR_UNSUPPORTED, they never fall back to another transport.
 * r3dm_graphs_pack / r3dm_graphs_unpack_merge expose the wire format (uint32 words: [n_graphs, len_k ..] then per graph
 * [P, M_lo, M_hi, pairs, counts, matches]) for hosts that bring their own transport; words from r3dm_graphs_pack are released with
 * r3dm_words_free. */
typedef struct r3dm_comm r3dm_comm;
int  r3dm_comm_unique_id(void* id_out_128);
int  r3dm_comm_create(const void* id_128, int rank, int world, int device_id, r3dm_comm** out);
void r3dm_comm_destroy(r3dm_comm* comm);
int  r3dm_comm_rank(const r3dm_comm* comm);
int  r3dm_comm_world(const r3dm_comm* comm);
const char* r3dm_comm_last_error(const r3dm_comm* comm);
int  r3dm_allgather_graphs(r3dm_comm* comm, const r3dm_graph* const* local, uint32_t n_graphs, r3dm_graph** merged_out /* [n_graphs] */);
/* Device-resident graphs for that exchange.  With r3dm_set_device_graphs(ctx, 1) every graph the context produces from then on
 * (r3dm_match_pairs*, r3dm_filter_F / _E / _H / _FEH) keeps, beside its host vectors, the same CSR in the memory of the context's GPU,
 * laid out by gather kernels where the matches already are (the finalisation's output array; the putative matches through the filters'
 * inlier indices).  r3dm_allgather_graphs sends such a graph from device memory -- its payload does not cross PCIe on the way out --
 * when the mirror lives on the communicator's device; other graphs are packed on the host as before (r3dm_graph_from_csr, loaded or
 * merged graphs have no mirror).  r3dm_graph_on_device: the device id of a graph's mirror, -1 without one;
 * r3dm_comm_last_device_graphs: how many local graphs of the last exchange went out that way.  The approximate matchers
 * (r3dm_match_pairs_kgraph / _hnsw / _mrpt) merge two part graphs on the host -- graph-searched pairs and exhaustively scanned small
 * ones: their result keeps a mirror when all of its pairs are of one kind (the usual case), none otherwise.
 * A rank takes part in every collective of an exchange whatever happened while it prepared its share -- graphs it cannot pack, buffers
 * it cannot allocate, copies into its send buffer that fail are reported in the words it contributes -- so all ranks return together;
 * not covered: a device that is gone (hipSetDevice, the size collective's own 16 (W + 1) bytes, a failing collective). */
int  r3dm_set_device_graphs(r3dm_ctx* ctx, int enable);
int  r3dm_graph_on_device(const r3dm_graph* g);
int  r3dm_comm_last_device_graphs(const r3dm_comm* comm);
int  r3dm_graphs_pack(const r3dm_graph* const* local, uint32_t n_graphs, uint32_t** words_out, uint64_t* n_words_out);
void r3dm_words_free(uint32_t* words);
int  r3dm_graphs_unpack_merge(const uint32_t* const* rank_words, const uint64_t* rank_n_words, uint32_t world, uint32_t n_graphs,
                              r3dm_graph** merged_out /* [n_graphs] */);

/* ---- feature tracks of a match graph: OpenMVG's TracksBuilder (Build, Filter, ExportToSTL, GetTracksInImages) on the GPU ----
 * Nodes and edges.  For pair p = (I, J) of g and match (i, j) of that pair the nodes are (I, i) and (J, j), and the match is an edge
 *   between them.  No special cases: duplicate edges are edges; the same two views listed as (I, J) and as (J, I) contribute alike; a
 *   pair with I == J contributes like any other (i != j joins two features of one view, i == j is a loop on one node).  View ids are
 *   arbitrary uint32 values, sparse or huge.
 * Components and the filter.  Components are the connected components over all nodes that appear in g.  The filter is
 *   TracksBuilder::Filter(nLengthSupTo): a component that contains two different nodes of one view is CONFLICTING and is removed
 *   whatever its size; of the rest, a component with fewer than min_length nodes is SHORT and is removed.  min_length >= 2; smaller
 *   values are R3DM_ERR_INVALID.  What remains are the tracks.
 * Canonical output.  A track's observations are sorted by view id ascending (one per view).  Tracks are sorted by their first
 *   observation, (view id, feature) ascending.  Track t is observations[offsets[t] .. offsets[t + 1]).  The output is a pure function
 *   of g and min_length: it does not depend on the order in which unions land on the device.  (OpenMVG numbers tracks by union-find
 *   root; the set of tracks is the same, the numbering is this library's.)
 * Size limit.  With s(v) = 1 + the largest feature index view v has in g, a graph whose sum of s(v) exceeds R3DM_TRACKS_MAX_SLOTS is
 *   R3DM_ERR_UNSUPPORTED: returned before anything sized by that sum is allocated.  So is a graph of 2^32 - 1 matches or more.
 * Trivial cases.  An empty graph gives zero tracks (offsets = {0}) and success.
 * kept_out (may be NULL): the track filter applied to the graph itself -- g restricted to the matches whose component is a track, order
 *   of pairs and of matches unchanged, pairs left empty dropped.  It gets a device mirror under the rule of every produced graph
 *   (r3dm_set_device_graphs).
 * Inputs.  A graph with a device mirror on the context's device is read where it is; any other graph (r3dm_graph_from_csr, loaded,
 *   merged) is uploaded.  NULL handles are R3DM_ERR_INVALID.  Nothing is allocated or launched for this feature before the first call.
 * r3dm_tracks_in_pair: GetTracksInImages({a, b}) as Regard3D's match preview uses it -- for every track, in track order, that observes
 *   both views: (feature in view_a, feature in view_b).  Not only direct matches: transitive ones appear too.  At most cap entries are
 *   written (out may be NULL when cap is 0); *n_out is the full count.  view_a == view_b is R3DM_ERR_INVALID; an unknown view gives
 *   zero results.  Host code over the arrays above.
 * r3dm_tracks_phase_ms: ms_kernels split into the call's four phases, each between two counts the host reads back: [0] the views'
 *   extents, [1] link + flatten + the selection of the nodes, [2] the sort by root + conflicts + the filter + the selection of the
 *   observations, [3] observations, offsets, kept matches.
 * Memory.  The work buffers are the context's and serve its next call; those above 64 MiB each are given back to the device when the
 *   call returns, so a graph near the slot limit (11 bytes per slot) does not pin gigabytes until r3dm_destroy.
 * The arrays of an r3dm_tracks live until r3dm_tracks_free. */
#define R3DM_TRACKS_MAX_SLOTS (1ull << 28)
typedef struct r3dm_tracks r3dm_tracks;
typedef struct { uint32_t view, feature; } r3dm_observation;
typedef struct {
    uint64_t n_matches, n_nodes, n_components, n_conflicting, n_short, n_tracks, n_observations;
    uint64_t n_matches_kept;          /* matches of g whose component is a track */
    uint32_t longest;                 /* observations of the longest track */
    uint32_t largest_component;       /* nodes of the largest component, removed ones included */
    double   ms_kernels, ms_wall;     /* HIP-event time of the device work (uploads excluded); the whole call */
} r3dm_tracks_stats;
int r3dm_build_tracks(r3dm_ctx* ctx, const r3dm_graph* g, uint32_t min_length, r3dm_tracks** out, r3dm_graph** kept_out /* may be NULL */);
uint64_t                r3dm_tracks_count(const r3dm_tracks* t);
const uint64_t*         r3dm_tracks_offsets(const r3dm_tracks* t);       /* n_tracks + 1 */
const r3dm_observation* r3dm_tracks_observations(const r3dm_tracks* t);
int  r3dm_tracks_report(const r3dm_tracks* t, r3dm_tracks_stats* out);
int  r3dm_tracks_phase_ms(const r3dm_tracks* t, double* out4);
int  r3dm_tracks_in_pair(const r3dm_tracks* t, uint32_t view_a, uint32_t view_b, r3dm_match* out, uint64_t cap, uint64_t* n_out);
void r3dm_tracks_free(r3dm_tracks* t);

/* ---- files: ".txt" (what Regard3D's consumers read) or ".bin" (cereal portable binary) ---- */
int r3dm_save_matches(const r3dm_graph* g, const char* path);
int r3dm_load_matches(const char* path, r3dm_graph** out);

/* ---- run statistics of the last r3dm_match_pairs / r3dm_filter_F call ---- */
typedef struct {
    double   ms_match_kernels;     /* HIP-event time of the 2-NN kernels (dominant kernel)        */
    uint64_t n_match_launches;     /* launches of the dominant kernel                              */
    double   ms_filter_kernels;    /* HIP-event time of the AC-RANSAC kernel                       */
    uint64_t n_pairs;              /* pairs processed                                              */
    uint64_t n_queries;            /* query rows processed                                         */
    uint64_t n_exact_fallback;     /* queries re-done by the exact scan (uncertified top-2)        */
    double   algorithmic_flops;    /* 2 * nI * nJ * D summed over pairs (L2) / lane-ops (Hamming)   */
    double   algorithmic_bytes;    /* compulsory HBM bytes: both descriptor sets once + results     */
    /* host wall-clock breakdown of the last calls (milliseconds) */
    double   ms_wall_match;        /* whole r3dm_match_pairs call                                   */
    double   ms_wall_match_post;   /* of which: exact scans + finalisation + copies back + assembly */
    double   ms_wall_filter;       /* whole r3dm_filter_F call                                      */
    double   ms_liop_kernel;       /* HIP-event time of the last r3dm_liop_describe_patches kernel (a features pass under R3DM_DESCRIPTOR_MLDB / _MSURF: of its MLDB / M-SURF launch) */
    /* r3dm_match_pairs_kgraph */
    double   ms_ann_build;         /* HIP-event time of the index builds triggered by the call      */
    double   ms_ann_search;        /* HIP-event time of the search kernel                           */
    uint64_t n_ann_built;          /* indices built by the call                                     */
    uint64_t n_ann_dist;           /* descriptor distances evaluated by the searches                */
    double   ms_detect;            /* wall time of the last r3dm_detect_akaze call                  */
    uint64_t n_integer_mfma;       /* launches of the dominant kernel that ran as the integer fast path  */
    uint64_t n_split_mfma;         /* launches of the dominant kernel that ran as the split-f16 nominator */
    uint64_t n_views_staged;       /* views / datasets / query sets copied + re-laid-out by this context since r3dm_create */
    uint64_t n_hamming_mfma;       /* launches of the Hamming matcher that ran as the MFMA formulation */
    uint64_t n_detect_images;      /* images of the last detector pass (r3dm_detect_akaze: 1; the batch entries: B)                   */
    uint64_t n_ann_rows16;         /* graph-search launches that gathered the bf16 row copy (integer-valued views: same distances, half the bytes) */
    uint64_t n_ann_rows8;          /* ... the u8 row copy (integers 0 .. 255: a quarter of the bytes)                                          */
    uint64_t n_ann_dot8;           /* ... of those, launches whose query views are bytes too: distances as exact integer dot products (v_dot4_u32_u8) */
    /* the last detector pass (r3dm_detect_akaze*, r3dm_extract_features_*) */
    double   ms_detect_kernels;    /* HIP-event time from the first scale-space launch to the keypoint compaction, all images of the pass */
    double   detect_algorithmic_bytes; /* HBM bytes the pass structure implies: every stencil pass reads / writes whole image planes once */
    double   ms_liop_wall;         /* host + device time of the LIOP half of the last features pass (patch maps, two launches, copy back); under R3DM_DESCRIPTOR_MLDB / _MSURF: of that descriptor's half */
    double   ms_feature_files;     /* time spent writing the .feat / .desc files of the last features pass                              */
    /* r3dm_match_pairs_hnsw (ms_ann_build / ms_ann_search / n_ann_built / n_ann_dist are shared with the KGraph path) */
    uint64_t n_hnsw_launches;      /* launches of the HNSW search kernel                                                                */
    uint64_t n_hnsw_retries;       /* ... of those, repeats because a query's candidate heap outgrew its LDS room                       */
    uint64_t n_counts_mfma;        /* launches of the split nominator that ran on COUNT tiles (rows = small integers x a row scale: LIOP; one f16 MFMA per 16 dimensions instead of three) */
    double   detect_compulsory_bytes; /* the last detector pass: bytes a perfectly fused level would still move (smoothed plane in + out, determinant out,
                                       * conductivity out, 8 bytes per pixel and FED step); detect_algorithmic_bytes is the as-structured count            */
    uint64_t n_filter_workgroups;  /* workgroups of the last AC-RANSAC call (all its filters): pool workers of the cooperative kernel + one per short pair */
    uint64_t n_filter_coop_pairs;  /* ... (pair, filter) items that ran on the cooperative kernel                                                          */
    /* r3dm_knn / r3dm_index_knn with r3dm_set_knn_narrow_tiles on */
    uint64_t n_knn_integer_tiles;  /* launches of the K-list nominator on the bf16 tiles (integer-valued rows: exact lists, nothing certified or scanned)  */
    uint64_t n_knn_split_tiles;    /* launches of the K-list nominator on the split-f16 planes (real-valued rows)                                          */
    /* r3dm_set_mutual_matching (both 0 while the switch is off).  They stand in front of the last k-NN counter: the interface test of
     * r3dm_set_knn_hamming_tiles holds that one to the end of the structure */
    uint64_t n_mutual_checked;     /* accepted matches the mutual check looked at                                                                          */
    uint64_t n_mutual_dropped;     /* ... of those, matches it removed: their row of I has a nearer row of J                                               */
    /* r3dm_knn / r3dm_index_knn with r3dm_set_knn_hamming_tiles on */
    uint64_t n_knn_hamming_tiles;  /* launches of the K-list nominator on the i8 tiles (BIN rows: exact lists, nothing certified or scanned)               */
} r3dm_stats;
int r3dm_get_stats(const r3dm_ctx* ctx, r3dm_stats* out);

/* ---- totals of the features work this context has done since r3dm_create (never reset: a stage that runs many batches on several
 * contexts adds them up; R3DFeaturesThread keeps doneCount_ / numberOfKeypoints_ the same way, src/threads/R3DFeaturesThread.cpp:32-36) ---- */
typedef struct {
    uint64_t n_images;                 /* images through the detector                                                         */
    uint64_t n_passes;                 /* detector passes (batches)                                                            */
    uint64_t n_keypoints;              /* keypoints found                                                                      */
    uint64_t n_regrows;                /* detection phases repeated because an image had more candidates than slots            */
    double   ms_detect_kernels;        /* HIP-event time, first scale-space launch .. keypoint compaction                      */
    double   detect_algorithmic_bytes; /* HBM bytes the pass structure implies (every stencil pass moves whole planes once)    */
    double   ms_liop_kernels;          /* HIP-event time of the LIOP patch extraction + descriptor launches (+ the MLDB / M-SURF launches of passes under those arms) */
    double   ms_wall;                  /* wall time inside the features entry points (detector + LIOP + copies + files)        */
    double   ms_files;                 /* of which: writing .feat / .desc                                                      */
} r3dm_features_totals;
int r3dm_get_features_totals(const r3dm_ctx* ctx, r3dm_features_totals* out);
/* How many helper threads a host should start beside this library: half of the cores the process may really use -- the affinity mask
 * AND the cgroup CPU quota (a container can show 256 processors and own 16; more runnable threads than that are throttled for the rest
 * of the scheduler period, which looks like random 60-100 ms stalls) -- at most `want`.  The library sizes its own teams with it. */
int r3dm_host_threads(int want);

/* A sink for the features entry points (r3dm_extract_features_batch, r3dm_multi_extract_features*): called once per COMPUTED image
 * (not for skipped ones), from a helper thread of the library (several images of a batch may arrive concurrently: the sink must be
 * thread-safe), after the image's two files are written.  desc_device = n_features x 144 floats
 * in DEVICE memory of the computing context (valid until the sink returns) -- under R3DM_DESCRIPTOR_MLDB it points at n_features x 61
 * BYTES there instead (the type of the argument stays; r3dm_set_image(dim 61, R3DM_BIN) takes the pointer as it is), under R3DM_DESCRIPTOR_MSURF at n_features x 64 floats (r3dm_set_image(dim 64, R3DM_F32)); xy_as_written = n_features x 2 floats exactly as a reader
 * of the .feat file parses them (the file holds 6 significant digits).  What Regions_Provider::load would read back from the files
 * (src/R3DComputeMatches.cpp:2040) is thus handed over without the round trip through the file system and the PCIe bus: the facade
 * registers the view with the matcher straight from it (r3dm_set_image accepts device pointers).  image_index = the index in the
 * arrays of the call.  A non-zero return fails the features call with R3DM_ERR_INVALID.  NULL removes the sink. */
typedef int (*r3dm_features_sink)(void* user, uint32_t image_index, uint32_t n_features, const float* desc_device, const float* xy_as_written);
int r3dm_set_features_sink(r3dm_ctx* ctx, r3dm_features_sink sink, void* user);
int r3dm_multi_set_features_sink(r3dm_multi* m, r3dm_features_sink sink, void* user);

/* Deferred feature files.  The reference's feature thread returns when KeypointSet::saveToBinFile has written the image's .feat /
 * .desc (src/threads/R3DFeaturesThread.cpp:139-170, src/keypointSet.hpp:61-67); with on != 0 a features call of this context returns
 * when the images are COMPUTED and handed to the sink -- the two fwrites of every image of a batch (16 MB of descriptors per 28 k
 * keypoints) run on a writer thread of the context, beside the caller's next step (the facade: the match phase) and beside the
 * context's next batch.  r3dm_features_files_wait joins the writer and reports its I/O error, if any (R3DM_ERR_IO; the message in
 * r3dm_last_error); a context joins its writer by itself before it needs the landing buffer again, when the mode is switched
 * off, and in r3dm_destroy.  The files are complete when the wait returns R3DM_OK -- call it before anything reads them.
 * Off by default: without it every features entry point returns with its files written, as before. */
int r3dm_set_deferred_feature_files(r3dm_ctx* ctx, int on);
/* The library's background host threads (the deferred feature-file writers of a context; the facade's match-file writers and map
 * builders) run at the host's default priority unless asked: nice_value 1 .. 19 makes them stand back behind the caller's own threads
 * (Linux per-thread nice; useful when the process lives under a CPU quota it can exhaust), 0 (default) leaves priorities alone. */
int r3dm_set_background_nice(r3dm_ctx* ctx, int nice_value);
int r3dm_multi_set_background_nice(r3dm_multi* m, int nice_value);
int r3dm_features_files_wait(r3dm_ctx* ctx);
int r3dm_multi_set_deferred_feature_files(r3dm_multi* m, int on);
int r3dm_multi_features_files_wait(r3dm_multi* m, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif
