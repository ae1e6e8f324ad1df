// api_match.cpp -- part of the host side of libr3dm.so: the C ABI declared in include/r3dm.h (see r3dm_ctx.hpp for the file map).
//
// Mirrors, for the compute-matches hot path only, what the reference does in
// /root/reference/src/R3DComputeMatches.cpp:2035-2129 and src/Regard3DFeatures.cpp -- with every arithmetic stage running as
// HIP kernels on one MI355X.  There is no CPU fallback in this file: when HIP fails, the call fails.
#include "r3dm_ctx.hpp"

// ------------------------------------------------------------------------------------------------
// putative matching
// ------------------------------------------------------------------------------------------------
// r3dm_set_mutual_matching: the mutual nearest-neighbour check on nn_idx[pair][*] (kernels_match_mutual.hip), after the ratio test and
// before the (i, j) ordering and both de-duplications.  Whatever arm nominated the matches, the check is the exhaustive one in the
// reference's arithmetic: over J's f32 tiles where the length has a tensor kernel and no scalar tail, over the row-major rows
// otherwise, over the word rows of binary views.  Adds the batch's two counters to the statistics.
// r3dm_set_symmetric_ratio: the same scan keeps the second minimum and repeats the batch's forward ratio test (`forward`) in reverse --
// the mutual rule is part of that rule, so the check runs when either switch is on; the third counter goes to
// r3dm_symmetric_ratio_report.
static int run_mutual_check(r3dm_ctx* c, const std::vector<PairJob>& jobs, uint32_t q_stride, ForwardRatio forward)
{
    const uint32_t P = (uint32_t)jobs.size();
    const HostImage& first = *c->imgs[jobs[0].sI];
    R3DM_HIP(c, c->d_mutual.ensure(24));
    R3DM_HIP(c, hipMemsetAsync(c->d_mutual.p, 0, 24, c->stream));
    MutualParams mp{};
    mp.imgs = c->d_imgs.as<ImgDev>(); mp.pairs = c->d_pairs.as<uint2>(); mp.n_pairs = P; mp.q_stride = q_stride;
    mp.nn_idx = c->d_nn.as<uint32_t>(); mp.counters = c->d_mutual.as<unsigned long long>();
    mp.ratio_R = forward.R; mp.ratio_form = !c->symmetric_ratio ? 0u : (forward.on_roots ? 2u : 1u);
    // (a chunk of the MRPT arm may hold views of several lengths: the rows-based kernel reads each pair's own)
    const bool one_length = std::all_of(jobs.begin(), jobs.end(), [&](const PairJob& j) { return c->imgs[j.sI]->dim == first.dim; });
    if (first.dtype == R3DM_BIN) R3DM_HIP(c, launch_hamming_mutual(c->stream, mp, first.words));
    else if (one_length && has_tensor_kernel(first.G) && (first.dim & 3u) == 0) R3DM_HIP(c, launch_l2_mutual_batch(c->stream, mp, first.G));
    else {
        const uint64_t total_slots = (uint64_t)P * q_stride;
        if (total_slots > 0xFFFFFFFFull) { c->err = "batch too large for the rows-based mutual check"; return R3DM_ERR_UNSUPPORTED; }
        std::vector<uint32_t> slots;
        slots.reserve(2 * (size_t)P);
        for (const PairJob& j : jobs) { slots.push_back(j.sI); slots.push_back(j.sJ); }
        { const int rcl = ensure_layouts(c, slots, kLayRows); if (rcl != R3DM_OK) return rcl; }
        R3DM_HIP(c, launch_l2_mutual_items(c->stream, mp, (uint32_t)total_slots));
    }
    unsigned long long counts[3] = {0, 0, 0};
    R3DM_HIP(c, hipMemcpyAsync(counts, mp.counters, 24, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    c->stats.n_mutual_checked += counts[0];
    c->stats.n_mutual_dropped += counts[1];
    if (c->symmetric_ratio) for (int k = 0; k < 3; ++k) c->symratio_counts[k] += counts[k];
    return R3DM_OK;
}

// compaction + ordering + de-duplication of nn_idx[pair][*] (finalize_pairs_kernel), copy back, append the non-empty
// pairs to `g` in job order.  Shared by the exhaustive and the graph-search drivers.  Calls that collect into a graph run the mutual
// check first while its switch or the symmetric ratio test's is on; the raw-list entries (g == nullptr: r3dm_knn2 and its relatives)
// never do.
int finalize_batch(r3dm_ctx* c, const std::vector<PairJob>& jobs, uint32_t q_stride, uint32_t sort_cap,
                          uint64_t n_queries, uint32_t max_nJ, r3dm_graph* g, int32_t* knn_idx_host, float* knn_dist_host, uint32_t knn_cols,
                          ForwardRatio forward)
{
    const uint32_t P = (uint32_t)jobs.size();
    if ((c->mutual_matching || c->symmetric_ratio) && g && P) { const int rcm = run_mutual_check(c, jobs, q_stride, forward); if (rcm != R3DM_OK) return rcm; }
    // ---- finalisation: compact + order + de-duplicate, per pair
    R3DM_HIP(c, c->d_pair_off.ensure((size_t)P * 8));
    R3DM_HIP(c, c->d_pair_cnt.ensure((size_t)P * 4));
    uint64_t out_cap = std::max<uint64_t>(1u << 20, n_queries / 4);
    std::vector<uint64_t> h_off(P);
    std::vector<uint32_t> h_cnt(P);
    unsigned long long total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        R3DM_HIP(c, c->d_out.ensure(out_cap * sizeof(r3dm_match)));
        R3DM_HIP(c, hipMemsetAsync(c->d_cnt.as<uint32_t>() + 8, 0, 8, c->stream));
        FinalizeParams fp{};
        fp.imgs = c->d_imgs.as<ImgDev>(); fp.pairs = c->d_pairs.as<uint2>(); fp.n_pairs = P; fp.q_stride = q_stride;
        fp.nn_idx = c->d_nn.as<uint32_t>(); fp.sort_cap = sort_cap;
        fp.spill_keys = nullptr; fp.spill_drop = nullptr; fp.spill_stride = 0;
        if (q_stride > sort_cap) {                         // views with more rows than the LDS sort holds
            fp.spill_stride = next_pow2(q_stride);
            R3DM_HIP(c, c->d_spill.ensure((size_t)P * fp.spill_stride * 9));
            fp.spill_keys = c->d_spill.as<unsigned long long>();
            fp.spill_drop = c->d_spill.as<unsigned char>() + (size_t)P * fp.spill_stride * 8;
        }
        fp.out = c->d_out.as<r3dm_match>(); fp.out_cap = out_cap;
        fp.total = reinterpret_cast<unsigned long long*>(c->d_cnt.as<uint32_t>() + 8);
        fp.pair_off = c->d_pair_off.as<uint64_t>(); fp.pair_cnt = c->d_pair_cnt.as<uint32_t>();
        R3DM_HIP(c, launch_finalize(c->stream, fp));
        // (every copy back lands in page-locked memory: pageable destinations go through the runtime's staging path)
        R3DM_HIP(c, c->pin_small.ensure(64 + (size_t)P * 12));
        unsigned char* ps = static_cast<unsigned char*>(c->pin_small.p);
        R3DM_HIP(c, hipMemcpyAsync(ps, fp.total, 8, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(ps + 64, fp.pair_off, (size_t)P * 8, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(ps + 64 + (size_t)P * 8, fp.pair_cnt, (size_t)P * 4, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        memcpy(&total, ps, 8); memcpy(h_off.data(), ps + 64, (size_t)P * 8); memcpy(h_cnt.data(), ps + 64 + (size_t)P * 8, (size_t)P * 4);
        if (total <= out_cap) break;
        out_cap = total;                                   // overflow: nothing was lost, run it again with room
    }
    // r3dm_set_match_budget: matches of sub-views go back into their views' own row numbers here, on the device, before the copy back
    // and before the device mirror is made
    if (g && total) { const int rcb = budget_remap(c, jobs, h_cnt.data(), c->d_pair_off.as<uint64_t>(), c->d_pair_cnt.as<uint32_t>(), c->d_out.as<r3dm_match>()); if (rcb != R3DM_OK) return rcb; }
    // the matches come back through the context's page-locked landing buffer on the context's stream (a synchronous hipMemcpy into a
    // fresh pageable vector runs on the null stream, pins the pages on the way and was seen to take 80 ms for 7.7 MB every few calls)
    const r3dm_match* h_m = nullptr;
    if (total) {
        R3DM_HIP(c, c->pin_out.ensure((size_t)total * sizeof(r3dm_match)));
        R3DM_HIP(c, hipMemcpyAsync(c->pin_out.p, c->d_out.p, (size_t)total * sizeof(r3dm_match), hipMemcpyDeviceToHost, c->stream));
        h_m = static_cast<const r3dm_match*>(c->pin_out.p);
    }
    if (knn_idx_host) {
        // single-pair use (r3dm_knn2; the k-lists of the approximate arms: knn_cols entries per query): copy the raw lists of pair 0
        R3DM_HIP(c, hipMemcpyAsync(knn_idx_host, c->d_knn_idx.p, (size_t)max_nJ * knn_cols * 4, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(knn_dist_host, c->d_knn_dist.p, (size_t)max_nJ * knn_cols * 4, hipMemcpyDeviceToHost, c->stream));
    }
    R3DM_HIP(c, hipStreamSynchronize(c->stream));

    if (g) {
        // r3dm_set_device_graphs: the same pairs, in the same order, into the graph's device mirror straight from d_out (no payload byte
        // of the mirror crosses PCIe: ids and counts are 12 bytes per pair of host-side bookkeeping)
        const bool mirror = c->device_graphs && (g->dev.valid || (g->pairs.empty() && g->dev.P == 0));
        GraphBuilder b(c, g, mirror, h_m, nullptr, c->d_out.as<r3dm_match>(), nullptr);
        g->matches.reserve(g->matches.size() + (size_t)total);     // (one allocation: a graph of millions of matches otherwise re-grows a dozen times)
        g->pairs.reserve(g->pairs.size() + 2 * (size_t)P); g->offsets.reserve(g->offsets.size() + P);
        for (uint32_t p = 0; p < P; ++p) {
            if (h_cnt[p] == 0) continue;                   // empty vectors never enter the map
            b.add(jobs[p].I, jobs[p].J, h_off[p], 0, h_cnt[p]);
        }
        b.done();
    }
    return R3DM_OK;
}

// ---- the path of a batch: which kernels it runs on and which layouts they read, decided from the views' statistics and the switches
// alone.  Every fast path is bit-exact only under its own condition on the views: those conditions are here and nowhere else.
enum class BatchPath { kHammingScan, kHammingMfma, kF32Tiles, kIntegerTiles, kSplitPlanes, kCountTiles, kExactScan };
struct BatchPlan { BatchPath path; uint32_t layouts; };                  // layouts: the kLay* bits the path reads
struct PathSwitches { bool integer_mfma, split_mfma, hamming_mfma, count_tiles; };

// same test as the kernels' exact_pair (kernels_match_common.hpp): key + ||q||^2 IS the reference distance, bit for bit
static bool exact_pair(const HostImage& A, const HostImage& B, bool bf16)
{
    const float dpad = (float)(A.G * 8), mI = A.max_abs, mJ = B.max_abs;
    return !A.not_integer && !B.not_integer &&
           ((A.has_negative || B.has_negative)
                ? dpad * (mI + mJ) * (mI + mJ) < 16777216.0f
                : (2.0f * dpad * mI * mJ < 16777216.0f && dpad * mI * mI < 16777216.0f && dpad * mJ * mJ < 16777216.0f)) &&
           (!bf16 || (mI <= 256.0f && mJ <= 256.0f));
}

static BatchPlan plan_batch(const std::vector<std::unique_ptr<HostImage>>& imgs, const std::vector<PairJob>& jobs, const PathSwitches& sw)
{
    auto all_pairs = [&](auto&& pred) { return std::all_of(jobs.begin(), jobs.end(), [&](const PairJob& j) { return pred(*imgs[j.sI], *imgs[j.sJ]); }); };
    const HostImage& first = *imgs[jobs[0].sI];
    if (first.dtype == R3DM_BIN) return sw.hamming_mfma ? BatchPlan{BatchPath::kHammingMfma, kLayBin8} : BatchPlan{BatchPath::kHammingScan, 0u};
    // descriptor length without a tensor kernel: the exact scan of every query reads the rows
    if (!has_tensor_kernel(first.G)) return {BatchPath::kExactScan, kLayRows};
    // integer fast path (r3dm_set_integer_mfma): every view of the batch must hold bf16-exact integers
    if (sw.integer_mfma && first.G != 18 && all_pairs([](const HostImage& A, const HostImage& B) { return exact_pair(A, B, true); }))
        return {BatchPath::kIntegerTiles, kLayBf16};
    // split-f16 nominator (r3dm_set_split_mfma): batches with at least one real-valued view (integer-valued batches are exact
    // on the f32 tiles already and have their own fast path); every view finite, scales within reach of one another
    const bool split = sw.split_mfma &&
        all_pairs([](const HostImage& A, const HostImage& B) {
            return std::isfinite(A.max_abs) && std::isfinite(B.max_abs) && A.max_abs > 0.0f && B.max_abs > 0.0f &&
                   std::abs(A.split_k - B.split_k) <= 40 && std::abs(A.split_k + B.split_k) <= 100;
        }) &&
        !all_pairs([](const HostImage& A, const HostImage& B) { return !A.not_integer && !B.not_integer; });
    // ... and its cheaper form for views whose rows are small integers x a row scale (LIOP: one f16 MFMA per 16 dimensions on the
    // count tiles instead of three on the split planes): every view of the batch must also pass the staging check (ensure_layouts)
    if (split && sw.count_tiles &&
        all_pairs([](const HostImage& A, const HostImage& B) { return counts_eligible(A.dtype, A.n, A.dim) && counts_eligible(B.dtype, B.n, B.dim); }))
        return {BatchPath::kCountTiles, kLayRows | kLayCounts};
    if (split) return {BatchPath::kSplitPlanes, kLayRows | kLaySplit};
    // the f32 tiles: a pair of integer-valued views never re-reads a row (exact_pair); any other pair re-scores its nominees from
    // the row-major rows
    return {BatchPath::kF32Tiles, all_pairs([](const HostImage& A, const HostImage& B) { return exact_pair(A, B, false); }) ? 0u : kLayRows};
}

// The one way off the chosen path: a batch planned on the count tiles that cannot run there (a view failed the votes-x-scale check,
// or the launcher has no count kernel for it) runs on the split planes, which are valid for every such batch.
static BatchPlan without_count_tiles(BatchPlan p)
{
    return p.path == BatchPath::kCountTiles ? BatchPlan{BatchPath::kSplitPlanes, kLayRows | kLaySplit} : p;
}

// The certification slack factor of a launch: a nominee's key + ||q||^2 differs from its reference distance by at most
// err_scale (max||a||^2 + ||q||^2) (MatchParams::err_scale, KnnParams::err_scale; G = padded descriptor length / 8).
// f32 tiles: |MFMA-path distance - reference distance| <= (3.5 D + 14) u (max||a||^2 + ||q||^2),
// u = 2^-24 (DESIGN.md "Certification"); 4.25 D u covers it for every padded D >= 64
// split-f16 keys: residue of the two-piece split 3 x 2^-22 ||a|| ||b|| <= 1.5 x 2^-22 (||a||^2 + ||b||^2), f32 accumulation of
// 3 Dpad products + one C operand per MFMA with a one-sided 2^-23 per addition on partial sums <= 2 (||a||^2 + ||b||^2), plus the
// reference sum's own (D/2 + 12) 2^-24 -- together below (3 Dpad + 34) 2^-22 (kernels_match_16bit.hip, l2_knn2_split_kernel), + 2 for
// the count kernel's bias: its keys carry ||b||^2 / (2 s_b) and drop it again
static float cert_slack_factor(uint32_t G, bool split_or_count_tiles)
{
    const float dpad = (float)(G * 8);
    return split_or_count_tiles ? (3.0f * dpad + 36.0f) * 2.3841858e-07f : 4.25f * dpad * 5.9604645e-08f;
}

// The pair-norm tiles the pruning kernel's filter reads (with `halves`, their f16 form for the level in front) and the tables of them
// by slot, whose addresses go into `hdr` (device).  The tiles are scratch of the call, not a layout of a view: made here from the f32
// tiles of the batch's views (one small kernel per view: 4 MB read, 2 MB written at 8192 rows) into one buffer of the context, which
// the next batch overwrites.  A view therefore holds what it held (r3dm_view_info), and nothing has to follow the views' lifecycle.
// tr: the host side of the asynchronous copies, the caller keeps it to the end of the call.
// prefix16: with them the rows' 96-dimension prefixes as f16 too, the f16 prefix test's table (r3dm_set_half_prefix): 6 KiB per tile and
// no padding, its reads end with a view's last tile (l2_prefix16_tile_stream).
static int stage_pairnorm_scratch(r3dm_ctx* c, const std::vector<uint32_t>& batch_slots, uint32_t G, bool halves, bool prefix16,
                                  PruneHeader* hdr, std::vector<uint64_t>& tr)
{
    constexpr size_t kPad = 4096;                          // the filter's window runs two groups (2 KiB) past a view's last tile
    constexpr size_t kPadH = 8192;                         // the f16 level's window runs four blocks (4 KiB) past a view's last f16 tile
    // per view: its f32 pair-norm tiles and, with the f16 level, its f16 tiles behind them (a quarter of the f32 tiles' bytes)
    const size_t nslots = c->imgs.size();
    size_t total = 0;
    for (uint32_t s : batch_slots)
        total += (size_t)c->imgs[s]->n_tiles * (G / 2) * 1024 + kPad + (halves ? (size_t)c->imgs[s]->n_tiles * (G / 4) * 1024 + kPadH : 0) +
                 (prefix16 ? (size_t)c->imgs[s]->n_tiles * (kPrefixGroups / 2) * 1024 : 0);
    R3DM_HIP(c, c->d_pairnorm_tiles.ensure(total));
    tr.assign(3 * nslots + 3, 0);                          // [slots: f32 tiles][slots: f16 tiles][slots: f16 prefix rows][the three tables' addresses]
    size_t at = 0;
    for (uint32_t s : batch_slots) {
        const HostImage& h = *c->imgs[s];
        float* dst = reinterpret_cast<float*>(c->d_pairnorm_tiles.as<unsigned char>() + at);
        at += (size_t)h.n_tiles * (G / 2) * 1024 + kPad;
        uint16_t* dsth = halves ? reinterpret_cast<uint16_t*>(c->d_pairnorm_tiles.as<unsigned char>() + at) : nullptr;
        if (halves) at += (size_t)h.n_tiles * (G / 4) * 1024 + kPadH;
        uint16_t* dstp = prefix16 ? reinterpret_cast<uint16_t*>(c->d_pairnorm_tiles.as<unsigned char>() + at) : nullptr;
        if (prefix16) at += (size_t)h.n_tiles * (kPrefixGroups / 2) * 1024;
        R3DM_HIP(c, launch_stage_pairnorm(c->stream, h.tiled.as<float>(), h.G, h.n_tiles, dst, dsth, dstp));
        tr[s] = (uint64_t)(uintptr_t)dst;
        tr[nslots + s] = (uint64_t)(uintptr_t)dsth;
        tr[2 * nslots + s] = (uint64_t)(uintptr_t)dstp;
    }
    // the tables of the tiles by slot, and their addresses in the header
    R3DM_HIP(c, c->d_pairnorm.ensure(8 * 3 * nslots));
    tr[3 * nslots] = (uint64_t)(uintptr_t)c->d_pairnorm.p;
    tr[3 * nslots + 1] = (uint64_t)(uintptr_t)(c->d_pairnorm.as<uint64_t>() + nslots);
    tr[3 * nslots + 2] = (uint64_t)(uintptr_t)(c->d_pairnorm.as<uint64_t>() + 2 * nslots);
    R3DM_HIP(c, hipMemcpyAsync(c->d_pairnorm.p, tr.data(), 8 * 3 * nslots, hipMemcpyHostToDevice, c->stream));
    static_assert(sizeof hdr->pairnorm == 8 && sizeof hdr->halfnorm == 8 && sizeof hdr->prefix16 == 8, "a table's address is one 64-bit word of tr");
    R3DM_HIP(c, hipMemcpyAsync(&hdr->pairnorm, &tr[3 * nslots], sizeof hdr->pairnorm, hipMemcpyHostToDevice, c->stream));
    if (halves) R3DM_HIP(c, hipMemcpyAsync(&hdr->halfnorm, &tr[3 * nslots + 1], sizeof hdr->halfnorm, hipMemcpyHostToDevice, c->stream));
    if (prefix16) R3DM_HIP(c, hipMemcpyAsync(&hdr->prefix16, &tr[3 * nslots + 2], sizeof hdr->prefix16, hipMemcpyHostToDevice, c->stream));
    return R3DM_OK;
}

// The exact scan of the queries the nominator could not certify: per pair and slice of image I, and per query for the whole batch
// where a pair's list overflowed (FbHeader::fb_total[1]) or the descriptor length has a scalar tail.
static int rescan_uncertified(r3dm_ctx* c, MatchParams& mp, const std::vector<uint32_t>& batch_slots, const HostImage& first,
                              uint32_t max_nI, uint64_t total_slots, bool overflowed)
{
    const uint32_t P = mp.n_pairs;
    bool rescan = overflowed;                              // some pair overflowed its list
    if ((first.dim & 3u) == 0) {
        // a pair's uncertified queries are scanned by one workgroup per ~1024 rows of image I (at most 64): few pairs with
        // long views (24 views of 28 k rows: 276 workgroups of 7.7 ms each) otherwise leave the chip idle behind one round,
        // and a workgroup walks its rows tile by tile behind two barriers each (4096 rows per workgroup: 3.9 ms on those views)
        uint32_t S = std::min<uint32_t>(64u, std::max<uint32_t>(1u, (max_nI + 1023u) / 1024u));
        while (S > 1 && (uint64_t)P * S > 65535ull * 4) --S;
        mp.fb_slices = S; mp.fb_part = nullptr; mp.fb_done = nullptr;
        if (S > 1) {
            R3DM_HIP(c, c->d_fb2.ensure((size_t)P * kFbPerPair * S * 16 + (size_t)P * 4 + 64));
            mp.fb_part = c->d_fb2.as<float4>();
            mp.fb_done = reinterpret_cast<uint32_t*>(c->d_fb2.as<unsigned char>() + (size_t)P * kFbPerPair * S * 16);
            R3DM_HIP(c, hipMemsetAsync(mp.fb_done, 0, (size_t)P * 4, c->stream));
        }
        R3DM_HIP(c, launch_l2_exact_batch(c->stream, mp, first.G));
    }
    else rescan = true;                                    // scalar-tail dims: generic exact kernel
    if (rescan) {
        if (total_slots > 0xFFFFFFFFull) { c->err = "batch too large for the exact rescan"; return R3DM_ERR_UNSUPPORTED; }
        { const int rcl = ensure_layouts(c, batch_slots, kLayRows); if (rcl != R3DM_OK) return rcl; }      // the per-query scan reads row-major rows
        R3DM_HIP(c, launch_l2_exact_items(c->stream, mp, (uint32_t)total_slots, 2));
    }
    return R3DM_OK;
}

// runs the 2-NN + ratio kernels over `jobs` (slot pairs, all of one dtype/dim) and appends the
// non-empty results to `g` in job order.  knn_idx/knn_dist (host, optional) receive the raw 2-NN.
// prepare -> plan -> stage -> launch -> rescan -> finalize.
int run_match_batch(r3dm_ctx* c, const std::vector<PairJob>& jobs, float ratio_R, r3dm_graph* g,
                    int32_t* knn_idx_host, float* knn_dist_host)
{
    const uint32_t P = (uint32_t)jobs.size();
    if (P == 0) return R3DM_OK;
    const double t_dbg0 = now_ms();
    { const int rcs = sync_view_stats(c); if (rcs != R3DM_OK) return rcs; }      // which path a batch takes depends on its views' statistics
    const HostImage& first = *c->imgs[jobs[0].sI];
    const r3dm_dtype dtype = first.dtype;
    uint32_t max_nI = 0, max_nJ = 0, max_tiles = 0;
    uint64_t n_queries = 0;
    double flops = 0, bytes = 0;
    for (const PairJob& j : jobs) {
        const HostImage& A = *c->imgs[j.sI];
        const HostImage& B = *c->imgs[j.sJ];
        max_nI = std::max(max_nI, A.n);
        max_nJ = std::max(max_nJ, B.n);
        max_tiles = std::max(max_tiles, B.n_tiles);
        n_queries += B.n;
        if (dtype == R3DM_BIN) {
            flops += 2.0 * A.n * (double)B.n * A.words;
            bytes += ((double)A.n + B.n) * A.words * 4 + (double)B.n * 16;
        } else {
            flops += 2.0 * A.n * (double)B.n * A.dim;
            bytes += ((double)A.n + B.n) * A.dim * 4 + (double)B.n * 16;
        }
    }
    // the views of the batch (layouts are staged per view, on first use)
    std::vector<uint32_t> batch_slots;
    batch_slots.reserve(2 * (size_t)P);
    for (const PairJob& j : jobs) { batch_slots.push_back(j.sI); batch_slots.push_back(j.sJ); }
    std::sort(batch_slots.begin(), batch_slots.end());
    batch_slots.erase(std::unique(batch_slots.begin(), batch_slots.end()), batch_slots.end());
    BatchPlan plan = plan_batch(c->imgs, jobs, PathSwitches{c->integer_mfma, c->split_mfma, c->hamming_mfma,
                                                            !r3dm_dev_knob("R3DM_NO_COUNT_TILES", 0)});    // (developer build: A/B against the split planes)
    // the f32 tiles in match mode may take the pruning kernel, whose filter reads pair-norm tiles of the batch's views (launch_l2_knn2
    // decides by the same rule)
    const bool prunes = plan.path == BatchPath::kF32Tiles && l2_prune_serves(first.G, c->prefix_pruning, knn_idx_host != nullptr, ratio_R);
    // ---- the layouts this batch reads that its views do not hold yet (staged once per view; kernels_match.hip, kernels_match_16bit.hip)
    {
        bool counts_ok = true;
        int rcl = plan.layouts ? ensure_layouts(c, batch_slots, plan.layouts, plan.path == BatchPath::kCountTiles ? &counts_ok : nullptr) : R3DM_OK;
        if (rcl == R3DM_OK && !counts_ok) { plan = without_count_tiles(plan); rcl = ensure_layouts(c, batch_slots, plan.layouts); }
        if (rcl != R3DM_OK) return rcl;
    }
    const uint32_t q_stride = match_q_stride(max_nJ);
    const uint32_t sort_cap = std::min<uint32_t>(16384, std::max<uint32_t>(8, next_pow2(q_stride)));   // LDS budget; larger views may spill

    std::vector<uint2> hp(P);
    for (uint32_t p = 0; p < P; ++p) hp[p] = make_uint2(jobs[p].sI, jobs[p].sJ);
    R3DM_HIP(c, c->d_pairs.ensure(sizeof(uint2) * P));
    R3DM_HIP(c, hipMemcpyAsync(c->d_pairs.p, hp.data(), sizeof(uint2) * P, hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, c->d_nn.ensure((size_t)P * q_stride * 4));
    const uint64_t total_slots = (uint64_t)P * q_stride;
    // per-pair lists of uncertified queries: [FbHeader][fb_cnt: P][fb_q: P x kFbPerPair]; the header and the counts start at zero
    R3DM_HIP(c, c->d_fb.ensure(sizeof(FbHeader) + ((size_t)P + (size_t)P * kFbPerPair) * 4));
    R3DM_HIP(c, hipMemsetAsync(c->d_fb.p, 0, sizeof(FbHeader) + (size_t)P * 4, c->stream));
    R3DM_HIP(c, c->d_cnt.ensure(64));
    R3DM_HIP(c, hipMemsetAsync(c->d_cnt.p, 0, 64, c->stream));
    if (knn_idx_host) {
        R3DM_HIP(c, c->d_knn_idx.ensure((size_t)total_slots * 8));
        R3DM_HIP(c, c->d_knn_dist.ensure((size_t)total_slots * 8));
    }

    MatchParams mp{};
    mp.imgs = c->d_imgs.as<ImgDev>();
    mp.pairs = c->d_pairs.as<uint2>();
    mp.n_pairs = P; mp.qb_per_pair = 0; mp.q_stride = q_stride;
    mp.ratio_R = ratio_R;
    mp.err_scale = cert_slack_factor(first.G, plan.path == BatchPath::kSplitPlanes || plan.path == BatchPath::kCountTiles);
    // (developer build: the slack factor in permille of the derived one -- 0 certifies on the bare inequality.  Only verdicts depend
    //  on it, no address does; tests/test_gpu_certificate.py shows that its cases notice.  The split planes' absolute part is a
    //  constant of their kernel and stays.)
    if (const int permille = r3dm_dev_knob("R3DM_CERT_SLACK_PERMILLE", 1000); permille != 1000) mp.err_scale *= (float)permille * 0.001f;
    mp.nn_idx = c->d_nn.as<uint32_t>();
    mp.knn_idx = knn_idx_host ? c->d_knn_idx.as<int32_t>() : nullptr;
    mp.knn_dist = knn_idx_host ? c->d_knn_dist.as<float>() : nullptr;
    FbHeader* const fbh = c->d_fb.as<FbHeader>();
    mp.fb_total = fbh->fb_total;
    mp.fb_cnt = reinterpret_cast<uint32_t*>(fbh + 1);
    mp.fb_q = mp.fb_cnt + P;
    const bool halves = prunes && c->half_filter;          // the f16 level in front of the filter (r3dm_set_half_filter)
    // the three levels' tile tests take their min form (MatchParams::prune bit 2) where no level-1 key can be a NaN or -inf: every view
    // of the batch has max |row|^2 below kMinTileTestNormBits (kernels_match.hip above the kernel has the derivation).  The
    // statistics are on the host since sync_view_stats above; a view without them keeps the batch on the general form.
    bool min_form = halves && c->min_tile_test;
    for (size_t i = 0; min_form && i < batch_slots.size(); ++i) {
        const HostImage& v = *c->imgs[batch_slots[i]];
        min_form = v.stats_valid && v.stat_bits[0] < kMinTileTestNormBits;
    }
    if (halves) (min_form ? c->prune_totals.min_pairs : c->prune_totals.general_pairs) += P;
    // the f16 prefix test in front of the restart (r3dm_set_half_prefix: MatchParams::prune bit 3) serves where the three levels serve
    const bool prefix16 = halves && c->half_prefix;
    mp.prune = c->prefix_pruning ? (halves ? (min_form ? 7u : 3u) | (prefix16 ? 8u : 0u) : 1u) : 0u;
    mp.prune_cnt = &fbh->prune;
    // ---- stage: the pruning kernel's tables
    std::vector<uint64_t> tr;                              // (lives to the end of the call, like hp: the copies from it are asynchronous)
    if (prunes) { const int rcs = stage_pairnorm_scratch(c, batch_slots, first.G, halves, prefix16, mp.prune_cnt, tr); if (rcs != R3DM_OK) return rcs; }

    const double t_dbg1 = now_ms();
    R3DM_HIP(c, hipEventRecord(c->ev0, c->stream));
    uint64_t n_fallback = 0;
    if (plan.path == BatchPath::kHammingMfma || plan.path == BatchPath::kHammingScan) {
        if (plan.path == BatchPath::kHammingMfma) {
            R3DM_HIP(c, launch_hamming_mfma(c->stream, mp, first.words, max_tiles));
            c->stats.n_hamming_mfma += 1;
        } else R3DM_HIP(c, launch_hamming_knn2(c->stream, mp, first.words, max_nJ));
        R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));      // (the finaliser would wait here anyway; keeps the wall breakdown honest)
    } else if (plan.path != BatchPath::kExactScan) {
        if (plan.path == BatchPath::kCountTiles) {
            // hipErrorInvalidValue = no count kernel for this launch (descriptor length, or a grid beyond the launcher's bound)
            // (the one-list kernel packs a key and its row into 32 bits: views beyond 65,536 rows would leave its keys fewer than seven
            //  mantissa bits and send a growing share of their queries to the exact scan -- they take the two-list kernel, float keys)
            const int two_lists = (max_nI > 65536u || r3dm_dev_knob("R3DM_COUNTS_TWO_LISTS", 0)) ? 1 : 0;
            const hipError_t ec = launch_l2_knn2_counts(c->stream, mp, first.G, max_tiles, two_lists);
            if (ec == hipErrorInvalidValue) {
                (void)hipGetLastError();
                plan = without_count_tiles(plan);
                const int rcl = ensure_layouts(c, batch_slots, plan.layouts);
                if (rcl != R3DM_OK) return rcl;
            } else { R3DM_HIP(c, ec); c->stats.n_split_mfma += 1; c->stats.n_counts_mfma += 1; }
        }
        if (plan.path == BatchPath::kSplitPlanes) {
            R3DM_HIP(c, launch_l2_knn2_split(c->stream, mp, first.G, max_tiles));
            c->stats.n_split_mfma += 1;
        } else if (plan.path != BatchPath::kCountTiles) {
            R3DM_HIP(c, launch_l2_knn2(c->stream, mp, first.G, max_tiles, plan.path == BatchPath::kIntegerTiles));
            if (plan.path == BatchPath::kIntegerTiles) c->stats.n_integer_mfma += 1;
        }
        R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
        // the header comes back up to its last counter: the uncertified queries, and this batch's share of the call's pruning totals
        constexpr size_t kRead = offsetof(FbHeader, prune) + sizeof(PruneHeader);
        R3DM_HIP(c, c->pin_small.ensure(kRead));
        R3DM_HIP(c, hipMemcpyAsync(c->pin_small.p, fbh, kRead, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        FbHeader hd{};
        memcpy(&hd, c->pin_small.p, kRead);
        c->prune_totals.tested += hd.prune.n_tested;
        c->prune_totals.pruned += hd.prune.n_pruned;
        c->prune_totals.filtered += hd.prune.n_filtered;
        c->prune_totals.half += hd.prune.n_half;
        c->prune_totals.skipped += hd.prune.n_skip;
        // (the f16 prefix test sees every tile the filter leaves: the skipped ones and those level 2 lets through)
        if (prefix16) c->prune_totals.prefix16_tested += hd.prune.n_tested - hd.prune.n_filtered;
        c->prune_totals.prefix16_pruned += hd.prune.n_prefix16;
        n_fallback = hd.fb_total[0];
        // ---- rescan
        if (hd.fb_total[0] > 0) {
            const int rcr = rescan_uncertified(c, mp, batch_slots, first, max_nI, total_slots, hd.fb_total[1] > 0);
            if (rcr != R3DM_OK) return rcr;
        }
    } else {
        // descriptor length without a tensor kernel: exact scan of every query (slow, still on the GPU)
        if (total_slots > 0xFFFFFFFFull) { c->err = "batch too large for the exact scan"; return R3DM_ERR_UNSUPPORTED; }
        R3DM_HIP(c, launch_l2_exact_items(c->stream, mp, (uint32_t)total_slots, 1));
        R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
        n_fallback = n_queries;
    }

    const double t_post = now_ms();            // (the stream is idle here only on the tensor path; good enough for a breakdown)
    int rcf = finalize_batch(c, jobs, q_stride, sort_cap, n_queries, max_nJ, g, knn_idx_host, knn_dist_host, 2, ForwardRatio{ratio_R, false});
    if (rcf != R3DM_OK) return rcf;
    c->stats.ms_wall_match_post += now_ms() - t_post;
    if (r3dm_dev_knob("R3DM_MATCH_TIMING", 0))
        fprintf(stderr, "run_match_batch: prepare %.2f ms, launch .. exact scan issued %.2f ms, finalize %.2f ms\n", t_dbg1 - t_dbg0, t_post - t_dbg1, now_ms() - t_post);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.ms_match_kernels += ms;
    c->stats.n_match_launches += 1;
    c->stats.n_pairs += P;
    c->stats.n_queries += n_queries;
    c->stats.n_exact_fallback += n_fallback;
    c->stats.algorithmic_flops += flops;
    c->stats.algorithmic_bytes += bytes;
    return R3DM_OK;
}

static int r3dm_match_pairs_impl(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs,
                                float dist_ratio, int squared_metric, r3dm_graph** out)
{
    if (!c || !out || (n_pairs && !pairs_ij)) return R3DM_ERR_INVALID;
    *out = nullptr;
    R3DM_HIP(c, hipSetDevice(c->device));
    c->stats = r3dm_stats{};
    c->symratio_counts[0] = c->symratio_counts[1] = c->symratio_counts[2] = 0;
    c->prune_totals = {};
    const double t_call = now_ms();
    std::vector<PairJob> jobs, none;
    const int rcp = resolve_pairs(c, pairs_ij, n_pairs, nullptr, none, jobs);
    if (rcp != R3DM_OK) return rcp;
    const float R = squared_metric ? dist_ratio * dist_ratio : dist_ratio;
    { const int rcg = preselect_gate(c, R, none, jobs); if (rcg != R3DM_OK) return rcg; }      // r3dm_set_preemptive_matching
    BudgetCallGuard budget_guard{c};
    { const int rcb = budget_substitute(c, none, jobs); if (rcb != R3DM_OK) return rcb; }      // r3dm_set_match_budget

    auto g = std::unique_ptr<r3dm_graph>(new r3dm_graph());
    g->offsets.push_back(0);

    // batches: same (dtype, dim) and a bounded nn_idx footprint
    size_t start = 0;
    while (start < jobs.size()) {
        const HostImage& F = *c->imgs[jobs[start].sI];
        size_t end = start;
        uint64_t slots = 0;
        uint32_t max_n = 0;
        while (end < jobs.size()) {
            const HostImage& A = *c->imgs[jobs[end].sI];
            if (A.dtype != F.dtype || A.dim != F.dim) break;
            const uint32_t mn = std::max(max_n, c->imgs[jobs[end].sJ]->n);
            const uint64_t s = (uint64_t)(end - start + 1) * ((mn + 31) / 32 * 32);
            // <= 3 GiB of nn_idx per batch; one 256-thread workgroup per >= 128 queries keeps the dispatch below 2^32 work-items,
            // one workgroup per pair in the finaliser / exact scan below kMaxBlocksOf256
            if (end > start && (s * 4 > (3ull << 30) || end - start >= kMaxBlocksOf256 - 8)) break;
            max_n = mn; slots = s; ++end;
        }
        (void)slots;
        std::vector<PairJob> batch(jobs.begin() + start, jobs.begin() + end);
        int rc = run_match_batch(c, batch, R, g.get(), nullptr, nullptr);
        if (rc != R3DM_OK) return rc;
        start = end;
    }
    c->stats.ms_wall_match = now_ms() - t_call;
    *out = g.release();
    return R3DM_OK;
}

extern "C" int r3dm_match_pairs(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs,
                                float dist_ratio, int squared_metric, r3dm_graph** out)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_match_pairs_impl(c, pairs_ij, n_pairs, dist_ratio, squared_metric, out); });
}

static int r3dm_knn2_impl(r3dm_ctx* c, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query,
                         uint32_t dim, r3dm_dtype dtype, int32_t* out_idx, float* out_dist)
{
    if (!c || !dataset || !query || !out_idx || !out_dist || dim == 0) return R3DM_ERR_INVALID;
    if (n_query < 1 || n_dataset < 2) return R3DM_ERR_INVALID;      // ArrayMatcherBruteForce: NN > nbRows / nbQuery < 1
    if (dtype == R3DM_BIN && !(((dim + 3) / 4) == 8 || ((dim + 3) / 4) == 16)) return R3DM_ERR_UNSUPPORTED;
    R3DM_HIP(c, hipSetDevice(c->device));
    c->prune_totals = {};                                  // (a raw 2-NN never prunes: the counters of this call read 0 / 0)
    PrivateSlots s(c, 2);
    int rc = stage_into_slot(c, s[0], 0, 0, 0, dataset, n_dataset, dim, dtype, nullptr);
    if (rc == R3DM_OK) rc = stage_into_slot(c, s[1], 0, 0, 0, query, n_query, dim, dtype, nullptr);
    if (rc != R3DM_OK) return rc;
    // which tiles this call ran on (r3dm_set_*_mfma), and how many of its queries went through the exact scan
    CallCounters counters(c, {&r3dm_stats::n_integer_mfma, &r3dm_stats::n_split_mfma, &r3dm_stats::n_hamming_mfma, &r3dm_stats::n_counts_mfma,
                              &r3dm_stats::n_exact_fallback});
    return run_match_batch(c, {{0, 1, s[0], s[1]}}, 1.0f, nullptr, out_idx, out_dist);
}

extern "C" int r3dm_knn2(r3dm_ctx* c, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query,
                         uint32_t dim, r3dm_dtype dtype, int32_t* out_idx, float* out_dist)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_knn2_impl(c, dataset, n_dataset, query, n_query, dim, dtype, out_idx, out_dist); });
}

// ------------------------------------------------------------------------------------------------
// ArrayMatcher::Build / SearchNeighbours with the dataset staged ONCE (the reference builds per I and searches per J:
// /root/reference/src/R3DComputeMatches.cpp:462-479, plugin contract src/utils/matcher_kgraph.h:120-166,205-251)
// ------------------------------------------------------------------------------------------------
static int r3dm_index_create_impl(r3dm_ctx* c, const void* dataset, uint32_t n_dataset, uint32_t dim, r3dm_dtype dtype, r3dm_index** out)
{
    if (!c || !out || !dataset || dim == 0 || n_dataset < 1) return R3DM_ERR_INVALID;
    *out = nullptr;
    if (dtype != R3DM_F32 && dtype != R3DM_U8 && dtype != R3DM_BIN) return R3DM_ERR_INVALID;
    if (n_dataset >= (1u << 22)) { c->err = "more than 4M rows in one index"; return R3DM_ERR_UNSUPPORTED; }
    if (dtype == R3DM_BIN && !(((dim + 3) / 4) == 8 || ((dim + 3) / 4) == 16)) return R3DM_ERR_UNSUPPORTED;
    R3DM_HIP(c, hipSetDevice(c->device));
    auto ix = std::unique_ptr<r3dm_index>(new (std::nothrow) r3dm_index());
    if (!ix) return R3DM_ERR_NOMEM;
    PrivateSlots s(c, 1);
    int rc = stage_into_slot(c, s[0], 0, 0, 0, dataset, n_dataset, dim, dtype, nullptr);
    // Build stages what searches will read: the row-major rows beside the tiles (an index is one dataset: memory is not the concern,
    // a search from any context must not have to add to it) and the layouts of the paths that are switched on; a path switched on
    // later adds its layout on first use, under the index's lock
    if (rc == R3DM_OK) rc = ensure_layouts(c, {s[0]}, dtype == R3DM_BIN ? (c->hamming_mfma ? kLayBin8 : 0u)
                                                                       : (kLayRows | (c->integer_mfma ? kLayBf16 : 0u) | (c->split_mfma ? (kLayCounts | kLaySplit) : 0u)));
    if (rc != R3DM_OK) return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("r3dm_index_create: ") + hipGetErrorString(e); return R3DM_ERR_HIP; }
    ix->device = c->device;
    ix->img = *c->imgs[s[0]];                 // the index takes the buffers over ...
    *c->imgs[s[0]] = HostImage();             // ... and the private slot forgets them
    *out = ix.release();
    return R3DM_OK;
}

extern "C" int r3dm_index_create(r3dm_ctx* c, const void* dataset, uint32_t n_dataset, uint32_t dim, r3dm_dtype dtype, r3dm_index** out)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_index_create_impl(c, dataset, n_dataset, dim, dtype, out); });
}

extern "C" void r3dm_index_destroy(r3dm_index* ix)
{
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    (void)hipDeviceSynchronize();
    ix->img.release();
    delete ix;
}

// an index search's two private slots: the index mounted into slot_index (aliases of its buffers, for this call only) beside the
// freshly staged query view in slot_query
int mount_index_beside_queries(r3dm_ctx* c, const r3dm_index* ix, const void* query, uint32_t n_query, uint32_t slot_index, uint32_t slot_query)
{
    r3dm_index* mix = const_cast<r3dm_index*>(ix);
    { std::lock_guard<std::mutex> lk(mix->mu); c->imgs[slot_index]->mount(mix); }
    const int rc = publish_entry(c, slot_index);
    return rc != R3DM_OK ? rc : stage_into_slot(c, slot_query, 0, 0, 0, query, n_query, ix->img.dim, ix->img.dtype, nullptr);
}

static int r3dm_index_knn2_impl(r3dm_ctx* c, const r3dm_index* ix, const void* query, uint32_t n_query, int32_t* out_idx, float* out_dist)
{
    if (!c || !ix || !query || !out_idx || !out_dist) return R3DM_ERR_INVALID;
    if (n_query < 1 || ix->img.n < 2) return R3DM_ERR_INVALID;          // ArrayMatcherBruteForce: NN > nbRows / nbQuery < 1
    if (ix->device != c->device) { c->err = "r3dm_index_knn2: the index lives on another device"; return R3DM_ERR_INVALID; }
    R3DM_HIP(c, hipSetDevice(c->device));
    PrivateSlots s(c, 2);
    const int rc = mount_index_beside_queries(c, ix, query, n_query, s[0], s[1]);
    if (rc != R3DM_OK) return rc;
    CallCounters counters(c, {&r3dm_stats::n_integer_mfma, &r3dm_stats::n_split_mfma, &r3dm_stats::n_hamming_mfma, &r3dm_stats::n_counts_mfma});
    return run_match_batch(c, {{0, 1, s[0], s[1]}}, 1.0f, nullptr, out_idx, out_dist);
}

extern "C" int r3dm_index_knn2(r3dm_ctx* c, const r3dm_index* ix, const void* query, uint32_t n_query, int32_t* out_idx, float* out_dist)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_index_knn2_impl(c, ix, query, n_query, out_idx, out_dist); });
}

// ------------------------------------------------------------------------------------------------
// k neighbours, k = 1 .. R3DM_KNN_MAX (kernels_match_knn.hip): ArrayMatcher::SearchNeighbours with any NN
// (/root/reference/src/utils/matcher_kgraph.h:205-251).  One (dataset, query) pair per call; k <= 2 is served by the 2-NN path above.
// ------------------------------------------------------------------------------------------------
// the k-list kernels over the views in slots sI (dataset) and sJ (queries): the f32 tiles / the popcount kernel whatever the
// r3dm_set_*_mfma switches say (their nominators keep 2-lists).  r3dm_set_knn_narrow_tiles is this path's own switch: while it is on,
// the pair is planned like a one-job 2-NN batch with the integer and split switches on (plan_batch: the conditions under which the
// bf16 tiles are exact and the split planes usable are stated there and nowhere else) and runs on the K-list kernel of the tiles the
// plan names (kernels_match_knn16.hip).  A launcher that has no kernel for the launch leaves the pair on the f32 K-list kernel.
// Binary views have a switch of their own, r3dm_set_knn_hamming_tiles: while it is on, both views are staged as byte-per-bit tiles and
// the pair runs on the i8 K-list kernel (kernels_match_knn8.hip); a launcher without a kernel leaves it on the popcount K-list kernel.
static int run_knn_batch(r3dm_ctx* c, uint32_t sI, uint32_t sJ, uint32_t k, int32_t* out_idx_host, float* out_dist_host)
{
    { const int rcs = sync_view_stats(c); if (rcs != R3DM_OK) return rcs; }
    const r3dm_dtype dtype = c->imgs[sI]->dtype;
    const uint32_t nI = c->imgs[sI]->n, nq = c->imgs[sJ]->n, G = c->imgs[sI]->G, dim = c->imgs[sI]->dim, words = c->imgs[sI]->words;
    const bool narrow = c->knn_narrow_tiles;
    const BatchPlan plan = plan_batch(c->imgs, {PairJob{0, 1, sI, sJ}}, PathSwitches{narrow, narrow, false, false});
    // the nominees are re-scored on the row-major rows, and the exact scan reads them (on the integer tiles nothing is re-scored, but
    // the in-kernel re-check of the exact-pair condition still has the scan behind it)
    if (dtype != R3DM_BIN) { const int rcl = ensure_layouts(c, {sI, sJ}, kLayRows | plan.layouts); if (rcl != R3DM_OK) return rcl; }
    else if (c->knn_hamming_tiles) { const int rcl = ensure_layouts(c, {sI, sJ}, kLayBin8); if (rcl != R3DM_OK) return rcl; }
    const size_t out_bytes = (size_t)nq * k * 4;
    R3DM_HIP(c, c->d_knn_idx.ensure(out_bytes));
    R3DM_HIP(c, c->d_knn_dist.ensure(out_bytes));
    // [fb_cnt | pad][fb_q: n_query]: a query is listed at most once, the list cannot overflow
    R3DM_HIP(c, c->d_fb.ensure((16 + (size_t)nq) * 4));
    R3DM_HIP(c, hipMemsetAsync(c->d_fb.p, 0, 64, c->stream));

    KnnParams kp{};
    kp.imgs = c->d_imgs.as<ImgDev>();
    kp.sI = sI; kp.sJ = sJ; kp.k = k;
    kp.err_scale = cert_slack_factor(G, false);
    kp.out_idx = c->d_knn_idx.as<int32_t>();
    kp.out_dist = c->d_knn_dist.as<float>();
    kp.fb_cnt = c->d_fb.as<uint32_t>();
    kp.fb_q = c->d_fb.as<uint32_t>() + 16;

    R3DM_HIP(c, hipEventRecord(c->ev0, c->stream));
    uint64_t n_fallback = 0;
    if (dtype == R3DM_BIN) {
        hipError_t e = hipErrorInvalidValue;
        if (c->knn_hamming_tiles) {
            e = launch_hamming_knnk_mfma(c->stream, kp, words, c->imgs[sJ]->n_tiles);
            if (e == hipSuccess) c->stats.n_knn_hamming_tiles += 1;
        }
        if (e == hipErrorInvalidValue || e == hipErrorNotSupported) {
            // no i8-tile kernel for this launch (or none asked for): the popcount K-list kernel
            (void)hipGetLastError();
            e = launch_hamming_knnk(c->stream, kp, words, nq);
        }
        R3DM_HIP(c, e);
        R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
    } else {
        const uint32_t ntI = c->imgs[sI]->n_tiles, ntJ = c->imgs[sJ]->n_tiles;
        hipError_t e = hipErrorInvalidValue;
        if (plan.path == BatchPath::kIntegerTiles) {
            e = launch_l2_knnk_int(c->stream, kp, G, ntI, ntJ);
            if (e == hipSuccess) c->stats.n_knn_integer_tiles += 1;
        } else if (plan.path == BatchPath::kSplitPlanes) {
            KnnParams ks = kp;
            ks.err_scale = cert_slack_factor(G, true);
            e = launch_l2_knnk_split(c->stream, ks, G, ntI, ntJ);
            if (e == hipSuccess) c->stats.n_knn_split_tiles += 1;
        }
        if (e == hipErrorInvalidValue || e == hipErrorNotSupported) {
            // no narrow-tile kernel for this launch (or none asked for): the f32 K-list kernel
            (void)hipGetLastError();
            e = has_tensor_kernel(G) ? launch_l2_knnk(c->stream, kp, G, ntI, ntJ) : hipErrorInvalidValue;
        }
        if (e == hipErrorInvalidValue) {
            // descriptor length without a tensor kernel (or a dataset beyond the nominator's reach): exact scan of every query
            (void)hipGetLastError();
            R3DM_HIP(c, launch_l2_exact_knn_items(c->stream, kp, nq, 0));
            R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
            n_fallback = nq;
        } else {
            R3DM_HIP(c, e);
            R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));      // (the nominator alone, as run_match_batch times its tile kernel)
            uint32_t cnt = 0;
            R3DM_HIP(c, c->pin_small.ensure(64));
            R3DM_HIP(c, hipMemcpyAsync(c->pin_small.p, kp.fb_cnt, 4, hipMemcpyDeviceToHost, c->stream));
            R3DM_HIP(c, hipStreamSynchronize(c->stream));
            memcpy(&cnt, c->pin_small.p, 4);
            if (cnt > nq) { c->err = "k-NN: fallback list corrupt"; return R3DM_ERR_HIP; }
            if (cnt) R3DM_HIP(c, launch_l2_exact_knn_items(c->stream, kp, cnt, 1));
            n_fallback = cnt;
        }
    }
    R3DM_HIP(c, hipMemcpyAsync(out_idx_host, kp.out_idx, out_bytes, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(out_dist_host, kp.out_dist, out_bytes, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.ms_match_kernels += ms;
    c->stats.n_match_launches += 1;
    c->stats.n_pairs += 1;
    c->stats.n_queries += nq;
    c->stats.n_exact_fallback += n_fallback;
    if (dtype == R3DM_BIN) { c->stats.algorithmic_flops += 2.0 * nI * (double)nq * words; c->stats.algorithmic_bytes += ((double)nI + nq) * words * 4 + (double)nq * k * 8; }
    else { c->stats.algorithmic_flops += 2.0 * nI * (double)nq * dim; c->stats.algorithmic_bytes += ((double)nI + nq) * dim * 4 + (double)nq * k * 8; }
    return R3DM_OK;
}

// the counters a k-NN call reports: its queries, how many the exact scan answered, which narrow tiles its K-list kernel ran on
// (r3dm_set_knn_narrow_tiles, r3dm_set_knn_hamming_tiles) -- and the 2-NN opt-in paths' counters, which hold 0 after a call on the k-list kernels;
// ms_match_kernels holds the HIP-event time of the call's first kernel (tools/knn_perf.py)
static constexpr std::initializer_list<uint64_t r3dm_stats::*> kKnnCounters = {
    &r3dm_stats::n_integer_mfma, &r3dm_stats::n_split_mfma, &r3dm_stats::n_hamming_mfma, &r3dm_stats::n_counts_mfma,
    &r3dm_stats::n_exact_fallback, &r3dm_stats::n_queries, &r3dm_stats::n_knn_integer_tiles, &r3dm_stats::n_knn_split_tiles,
    &r3dm_stats::n_knn_hamming_tiles};

// k <= 2 is the 2-NN path itself, bit-identical to r3dm_knn2 / r3dm_index_knn2 by construction: knn2(idx, dist) runs that call; k = 1
// keeps the first column of its result
template <class Knn2>
static int knn_by_knn2(r3dm_ctx* c, uint32_t k, uint32_t n_query, int32_t* out_idx, float* out_dist, Knn2&& knn2)
{
    int rc;
    if (k == 2) rc = knn2(out_idx, out_dist);
    else {
        std::vector<int32_t> i2(2 * (size_t)n_query); std::vector<float> d2(2 * (size_t)n_query);
        rc = knn2(i2.data(), d2.data());
        if (rc == R3DM_OK)
            for (uint32_t q = 0; q < n_query; ++q) { out_idx[q] = i2[2 * (size_t)q]; out_dist[q] = d2[2 * (size_t)q]; }
    }
    if (rc == R3DM_OK) c->stats.n_queries = n_query;
    return rc;
}

// the exact k nearest rows of the view in slot sI for every row of the view in slot sJ, by the rule of r3dm_knn: k <= 2 on the 2-NN path
// (the small views of the approximate arms' k-NN entries are answered here, as their 2-NN siblings answer them with run_match_batch)
int run_exact_knn_pair(r3dm_ctx* c, uint32_t sI, uint32_t sJ, uint32_t k, int32_t* out_idx, float* out_dist)
{
    const uint32_t n_query = c->imgs[sJ]->n;
    if (k <= 2 && c->imgs[sI]->n >= 2)
        return knn_by_knn2(c, k, n_query, out_idx, out_dist,
                           [&](int32_t* idx, float* dist) { return run_match_batch(c, {{0, 1, sI, sJ}}, 1.0f, nullptr, idx, dist); });
    return run_knn_batch(c, sI, sJ, k, out_idx, out_dist);
}

static int r3dm_knn_impl(r3dm_ctx* c, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query,
                         uint32_t dim, r3dm_dtype dtype, uint32_t k, int32_t* out_idx, float* out_dist)
{
    if (!c || !dataset || !query || !out_idx || !out_dist || dim == 0) return R3DM_ERR_INVALID;
    if (k < 1 || k > R3DM_KNN_MAX || n_query < 1 || n_dataset < k) return R3DM_ERR_INVALID;      // ArrayMatcher plugins: NN > nbRows / nbQuery < 1
    if (dtype != R3DM_F32 && dtype != R3DM_U8 && dtype != R3DM_BIN) return R3DM_ERR_INVALID;
    if (dtype == R3DM_BIN && !(((dim + 3) / 4) == 8 || ((dim + 3) / 4) == 16)) return R3DM_ERR_UNSUPPORTED;
    if (k <= 2 && n_dataset >= 2)
        return knn_by_knn2(c, k, n_query, out_idx, out_dist,
                           [&](int32_t* idx, float* dist) { return r3dm_knn2_impl(c, dataset, n_dataset, query, n_query, dim, dtype, idx, dist); });
    if (n_dataset >= (1u << 22)) { c->err = "more than 4M rows in one dataset"; return R3DM_ERR_UNSUPPORTED; }
    R3DM_HIP(c, hipSetDevice(c->device));
    PrivateSlots s(c, 2);
    int rc = stage_into_slot(c, s[0], 0, 0, 0, dataset, n_dataset, dim, dtype, nullptr);
    if (rc == R3DM_OK) rc = stage_into_slot(c, s[1], 0, 0, 0, query, n_query, dim, dtype, nullptr);
    if (rc != R3DM_OK) return rc;
    CallCounters counters(c, kKnnCounters, {&r3dm_stats::ms_match_kernels});
    return run_knn_batch(c, s[0], s[1], k, out_idx, out_dist);
}

extern "C" int r3dm_knn(r3dm_ctx* c, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query,
                        uint32_t dim, r3dm_dtype dtype, uint32_t k, int32_t* out_idx, float* out_dist)
{
    if (!c) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int { return r3dm_knn_impl(c, dataset, n_dataset, query, n_query, dim, dtype, k, out_idx, out_dist); });
}

static int r3dm_index_knn_impl(r3dm_ctx* c, const r3dm_index* ix, const void* query, uint32_t n_query, uint32_t k, int32_t* out_idx, float* out_dist)
{
    if (!c || !ix || !query || !out_idx || !out_dist) return R3DM_ERR_INVALID;
    if (k < 1 || k > R3DM_KNN_MAX || n_query < 1 || ix->img.n < k) return R3DM_ERR_INVALID;
    if (k <= 2 && ix->img.n >= 2)
        return knn_by_knn2(c, k, n_query, out_idx, out_dist,
                           [&](int32_t* idx, float* dist) { return r3dm_index_knn2_impl(c, ix, query, n_query, idx, dist); });
    if (ix->device != c->device) { c->err = "r3dm_index_knn: the index lives on another device"; return R3DM_ERR_INVALID; }
    R3DM_HIP(c, hipSetDevice(c->device));
    PrivateSlots s(c, 2);
    const int rc = mount_index_beside_queries(c, ix, query, n_query, s[0], s[1]);
    if (rc != R3DM_OK) return rc;
    CallCounters counters(c, kKnnCounters, {&r3dm_stats::ms_match_kernels});
    return run_knn_batch(c, s[0], s[1], k, out_idx, out_dist);
}

extern "C" int r3dm_index_knn(r3dm_ctx* c, const r3dm_index* ix, const void* query, uint32_t n_query, uint32_t k, int32_t* out_idx, float* out_dist)
{
    if (!c) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int { return r3dm_index_knn_impl(c, ix, query, n_query, k, out_idx, out_dist); });
}
