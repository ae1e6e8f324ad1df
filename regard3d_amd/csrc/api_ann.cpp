// api_ann.cpp -- part of the host side of libr3dm.so: what the approximate matchers of the C ABI (include/r3dm.h) share, and the first
// of them.
//
// The three arms -- the graph matcher here (r3dm_match_pairs_kgraph), HNSW (api_hnsw.cpp), MRPT (api_mrpt.cpp) -- differ in their index,
// their search kernel and a handful of rules; a collection call, a search batch and an array entry have one frame each, below, and an
// arm hands its differences in as callables.  The exhaustive matcher (api_match.cpp) resolves its pair list
// with the same function.  There is no CPU fallback in this file: when HIP fails, the call fails.
#include "r3dm_ctx.hpp"
#include <cstddef>

extern "C" int r3dm_graph_merge(const r3dm_graph* const* parts, uint32_t n_parts, r3dm_graph** out);

// ------------------------------------------------------------------------------------------------
// the collection call: pairs_ij -> jobs -> indexed part + scanned part -> one graph
// ------------------------------------------------------------------------------------------------
// Matcher_Regions::Match: a pair that names an unregistered view is refused; pairs whose views are empty or of different region types
// are skipped.  Every other pair goes to `indexed` or `scanned` as the arm's classifier says (none: all scanned), both ordered by (I, J)
// and free of duplicates.
int resolve_pairs(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs, const PairClassifier& classify,
                  std::vector<PairJob>& indexed, std::vector<PairJob>& scanned)
{
    if (!classify) scanned.reserve(n_pairs);
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint32_t I = pairs_ij[2 * p], J = pairs_ij[2 * p + 1];
        auto a = c->slot_of.find(I), b = c->slot_of.find(J);
        if (a == c->slot_of.end() || b == c->slot_of.end()) { c->err = "pair references an unregistered view"; return R3DM_ERR_INVALID; }
        const HostImage& A = *c->imgs[a->second];
        const HostImage& B = *c->imgs[b->second];
        if (A.n == 0 || B.n == 0 || A.dtype != B.dtype || A.dim != B.dim) continue;
        bool index = false;
        if (classify) { const int rc = classify(A, index); if (rc != R3DM_OK) return rc; }
        (index ? indexed : scanned).push_back({I, J, a->second, b->second});
    }
    for (auto* v : {&indexed, &scanned}) {
        std::sort(v->begin(), v->end(), [](const PairJob& x, const PairJob& y) { return x.I != y.I ? x.I < y.I : x.J < y.J; });
        v->erase(std::unique(v->begin(), v->end(), [](const PairJob& x, const PairJob& y) { return x.I == y.I && x.J == y.J; }), v->end());
    }
    return R3DM_OK;
}

// the pairs of an approximate matcher whose dataset view is not indexed: few and tiny, scanned exhaustively, one batch per
// (dtype, dim) run
static int run_scanned_pairs(r3dm_ctx* c, const std::vector<PairJob>& jobs, float ratio_R, float bin_ratio_R, r3dm_graph* g)
{
    for (size_t start = 0, end = 0; start < jobs.size(); start = end) {
        const HostImage& F = *c->imgs[jobs[start].sI];
        for (end = start; end < jobs.size() && c->imgs[jobs[end].sI]->dtype == F.dtype && c->imgs[jobs[end].sI]->dim == F.dim;) ++end;
        const float R = (F.dtype == R3DM_BIN && bin_ratio_R >= 0.0f) ? bin_ratio_R : ratio_R;
        const int rc = run_match_batch(c, std::vector<PairJob>(jobs.begin() + start, jobs.begin() + end), R, g, nullptr, nullptr);
        if (rc != R3DM_OK) return rc;
    }
    return R3DM_OK;
}

// (r3dm_set_device_graphs) the two part graphs are merged on the host: a device mirror survives that only when one part is the whole
// result -- then it is built and handed over; with both kinds of pairs present no mirror is built at all (it would be dropped)
struct PartMirrorGuard {
    r3dm_ctx* c; bool keep;
    PartMirrorGuard(r3dm_ctx* c_, bool suppress) : c(c_), keep(c_->device_graphs) { if (suppress) c->device_graphs = false; }
    ~PartMirrorGuard() { c->device_graphs = keep; }
};

// merged = ga + gs ordered by (I, J).  When one part is empty the other one IS the result (its batches appended pairs in (I, J) order):
// its device mirror moves to the merged graph instead of being dropped with the part.
static int merge_parts_keep_mirror(r3dm_graph& ga, r3dm_graph& gs, r3dm_graph** out)
{
    const r3dm_graph* parts[2] = {&ga, &gs};
    const int rc = r3dm_graph_merge(parts, 2, out);
    if (rc != R3DM_OK || !*out) return rc;
    r3dm_graph* whole = ga.pairs.empty() ? &gs : (gs.pairs.empty() ? &ga : nullptr);
    if (whole && whole->dev.valid && whole->dev.P == (*out)->pairs.size() / 2 && whole->dev.M == (*out)->matches.size() && (*out)->pairs == whole->pairs) {
        (*out)->dev = whole->dev;                 // (plain handles: the part forgets them, the merged graph frees them)
        whole->dev = GraphDev();
    }
    return rc;
}

int match_collection_ann(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs, float scanned_ratio_R, const AnnArm& arm, r3dm_graph** out)
{
    const float gate_ratio_R = scanned_ratio_R;       // the three arms scan with ratio^2 on squared distances: the gate's R as well
    R3DM_HIP(c, hipSetDevice(c->device));
    c->stats = r3dm_stats{};
    c->symratio_counts[0] = c->symratio_counts[1] = c->symratio_counts[2] = 0;
    const double t_call = now_ms();
    std::vector<PairJob> indexed, scanned;
    int rc = resolve_pairs(c, pairs_ij, n_pairs, arm.classify, indexed, scanned);
    if (rc != R3DM_OK) return rc;
    rc = preselect_gate(c, gate_ratio_R, indexed, scanned, arm.bin_ratio_R);      // r3dm_set_preemptive_matching
    if (rc != R3DM_OK) return rc;
    BudgetCallGuard budget_guard{c};
    rc = budget_substitute(c, indexed, scanned, arm.classify);                      // r3dm_set_match_budget
    if (rc != R3DM_OK) return rc;

    r3dm_graph ga, gs;
    ga.offsets.push_back(0); gs.offsets.push_back(0);
    PartMirrorGuard mirror_guard(c, !indexed.empty() && !scanned.empty());
    if (!indexed.empty()) {
        rc = arm.ensure(indexed);
        if (rc != R3DM_OK) return rc;
    }
    for (size_t start = 0, end = 0; start < indexed.size(); start = end) {
        const uint32_t dim = c->imgs[indexed[start].sI]->dim;
        const r3dm_dtype dtype = c->imgs[indexed[start].sI]->dtype;
        uint32_t max_n = 0;
        for (end = start; end < indexed.size() && end - start < arm.max_chunk_pairs; ++end) {
            if (arm.one_dim_per_chunk && (c->imgs[indexed[end].sI]->dim != dim || (c->imgs[indexed[end].sI]->dtype == R3DM_BIN) != (dtype == R3DM_BIN))) break;
            const uint32_t mn = std::max(max_n, c->imgs[indexed[end].sJ]->n);
            const uint64_t s = (uint64_t)(end - start + 1) * ((mn + 31) / 32 * 32);
            // <= 3 GiB of nn_idx, and one workgroup per 4 queries: the dispatch must stay below 2^32 work-items (kMaxBlocksOf256)
            if (end > start && (s * 4 > (3ull << 30) || s / 4 > kMaxBlocksOf256 - 4096)) break;
            max_n = mn;
        }
        rc = arm.run_batch(std::vector<PairJob>(indexed.begin() + start, indexed.begin() + end), &ga);
        if (rc != R3DM_OK) return rc;
    }
    rc = run_scanned_pairs(c, scanned, scanned_ratio_R, arm.bin_ratio_R, &gs);
    if (rc != R3DM_OK) return rc;
    rc = merge_parts_keep_mirror(ga, gs, out);
    c->stats.ms_wall_match = now_ms() - t_call;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// one search batch: sizes, pair table, common buffers, event bracket, comparison count, finalisation, common statistics
// ------------------------------------------------------------------------------------------------
int run_ann_batch(r3dm_ctx* c, const std::vector<PairJob>& jobs, r3dm_graph* g, int32_t* knn_idx_host, float* knn_dist_host,
                  const std::function<int(const AnnBatch&)>& launch, uint32_t knn_cols, ForwardRatio forward)
{
    AnnBatch b{};
    b.P = (uint32_t)jobs.size();
    if (b.P == 0) return R3DM_OK;
    {   // index rows and queries are gathered from the row-major rows (f32, or the compact copies made from them)
        std::vector<uint32_t> slots;
        for (const PairJob& j : jobs) { slots.push_back(j.sI); slots.push_back(j.sJ); }
        const int rcl = ensure_layouts(c, slots, kLayRows);
        if (rcl != R3DM_OK) return rcl;
    }
    uint64_t n_queries = 0;
    for (const PairJob& j : jobs) {
        b.max_nI = std::max(b.max_nI, c->imgs[j.sI]->n);
        b.max_nJ = std::max(b.max_nJ, c->imgs[j.sJ]->n);
        n_queries += c->imgs[j.sJ]->n;
    }
    b.dim = c->imgs[jobs[0].sI]->dim;
    b.q_stride = std::max<uint32_t>(32, (b.max_nJ + 31) / 32 * 32);
    const uint32_t sort_cap = std::min<uint32_t>(16384, std::max<uint32_t>(8, next_pow2(b.q_stride)));   // LDS budget; larger views may spill
    std::vector<uint2> hp(b.P);
    for (uint32_t p = 0; p < b.P; ++p) hp[p] = make_uint2(jobs[p].sI, jobs[p].sJ);
    R3DM_HIP(c, c->d_pairs.ensure(sizeof(uint2) * b.P));
    R3DM_HIP(c, hipMemcpyAsync(c->d_pairs.p, hp.data(), sizeof(uint2) * b.P, hipMemcpyHostToDevice, c->stream));
    const uint64_t total_slots = (uint64_t)b.P * b.q_stride;
    R3DM_HIP(c, c->d_nn.ensure((size_t)total_slots * 4));
    R3DM_HIP(c, c->d_cnt.ensure(64));
    if (knn_idx_host) {
        R3DM_HIP(c, c->d_knn_idx.ensure((size_t)total_slots * knn_cols * 4));
        R3DM_HIP(c, c->d_knn_dist.ensure((size_t)total_slots * knn_cols * 4));
    }
    b.nn_idx = c->d_nn.as<uint32_t>();
    b.knn_idx = knn_idx_host ? c->d_knn_idx.as<int32_t>() : nullptr;
    b.knn_dist = knn_idx_host ? c->d_knn_dist.as<float>() : nullptr;
    b.n_comps = reinterpret_cast<unsigned long long*>(c->d_cnt.as<uint32_t>() + 4);
    R3DM_HIP(c, hipMemsetAsync(c->d_cnt.p, 0, 64, c->stream));
    R3DM_HIP(c, hipEventRecord(c->ev0, c->stream));
    int rc = launch(b);
    if (rc != R3DM_OK) return rc;
    R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
    unsigned long long comps = 0;
    R3DM_HIP(c, hipMemcpyAsync(&comps, b.n_comps, 8, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));              // (the pair table and the arm's job records are host temporaries)
    const double t_post = now_ms();
    rc = finalize_batch(c, jobs, b.q_stride, sort_cap, n_queries, b.max_nJ, g, knn_idx_host, knn_dist_host, knn_cols, forward);
    if (rc != R3DM_OK) return rc;
    c->stats.ms_wall_match_post += now_ms() - t_post;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.ms_ann_search += ms;
    c->stats.n_ann_dist += comps;
    c->stats.n_match_launches += 1;
    c->stats.n_pairs += b.P;
    c->stats.n_queries += n_queries;
    return R3DM_OK;
}

// ------------------------------------------------------------------------------------------------
// an arm's structure on an r3dm_index: built once, searched from any context of the device
// ------------------------------------------------------------------------------------------------
// The build runs on a private slot that holds the index's image (its buffers, not aliases: the arm's ensure_* adds the structure's
// buffers to it) and hands the image back on every exit.  It holds the index's lock for that long: a context that mounts the index
// waits; a search that mounted it before runs on, on buffers the build does not touch.
int with_index_structure(r3dm_ctx* c, const r3dm_index* ix, const void* query, uint32_t n_query,
                         const std::function<int(const r3dm_index&)>& state, const std::function<int(r3dm_index&, uint32_t slot)>& build,
                         const std::function<int(uint32_t sI, uint32_t sJ)>& search)
{
    if (ix->device != c->device) { c->err = "the index lives on another device"; return R3DM_ERR_INVALID; }
    R3DM_HIP(c, hipSetDevice(c->device));
    r3dm_index* mix = const_cast<r3dm_index*>(ix);
    PrivateSlots s(c, 2);
    {
        std::lock_guard<std::mutex> lk(mix->mu);
        const int st = state(*mix);
        if (st < 0) return st;
        if (st == 1) {
            struct Lend {                                     // the slot IS the index for the build, and gives it back whatever happens
                r3dm_ctx* c; r3dm_index* ix; HostImage& slot;
                Lend(r3dm_ctx* c_, r3dm_index* ix_, HostImage& slot_) : c(c_), ix(ix_), slot(slot_) { slot = ix->img; }
                ~Lend() { (void)hipStreamSynchronize(c->stream); ix->img = slot; slot = HostImage(); }
            } lend(c, mix, *c->imgs[s[0]]);
            int rc = publish_entry(c, s[0]);
            if (rc == R3DM_OK) rc = build(*mix, s[0]);
            if (rc != R3DM_OK) return rc;
        }
    }
    const int rc = mount_index_beside_queries(c, ix, query, n_query, s[0], s[1]);
    return rc != R3DM_OK ? rc : search(s[0], s[1]);
}

// ------------------------------------------------------------------------------------------------
// approximate matching: graph index + graph search (kernels_ann.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int r3dm_kgraph_preset(int preset, r3dm_kgraph_params* out)
{
    if (!out) return R3DM_ERR_INVALID;
    // src/R3DComputeMatches.cpp:844-873: (K, L, recall, P) = default (16, 24, .99, 10); 0: (2, 20, .6, 2); 1: (16, 24, .2, 6);
    // 2: (16, 24, .8, 12).  NN-descent keeps between S and L neighbours per row depending on how far it converged (its
    // recall target); the exact index has no such knob, so index_K takes the pool length L of the preset.
    r3dm_kgraph_params k{};
    k.search_S = 10; k.seed = 1998;
    switch (preset) {
        case 0:  k.index_K = 20; k.search_P = 2;  break;
        case 1:  k.index_K = 24; k.search_P = 6;  break;
        case 2:  k.index_K = 24; k.search_P = 12; break;
        default: k.index_K = 24; k.search_P = 10; break;
    }
    *out = k;
    return R3DM_OK;
}

// The approximate arms of the reference's dispatch (src/R3DComputeMatches.cpp:2035-2062) all trade recall for speed with a
// different index each (FLANN kd-trees, KGraph, MRPT random-projection trees, HNSW); none of them is reproducible bit for bit
// (random trees / seeds / thread schedules), so parity with any of them is recall.  The HNSW arms have their own matcher
// (api_hnsw.cpp: hnswlib's search, bit-exact on a reference-built index); this table is how the one deterministic graph matcher
// serves an arm when the host asks for the fastest matcher of at least the arm's recall (the facade's default policy), and the
// arms whose index is not built here at all (FLANN, MRPT):
//   1..3  kgraph_match presets                        -> fast / medium / precise
//   6..8  hnsw_match presets (:533-565)               -> fast / medium / precise  (reference-built HNSW on tests/golden/
//                                                        ann_hnsw_ref.npz: 0.573 / 0.933 / 0.975 recall@1; here 0.851 / 0.947 / 0.980)
//   5     mrpt_match (:453-460, targetRecall_ 0.8)     -> medium (0.947)
//   0     Matcher_Regions(ANN_L2): FLANN kd-trees     -> precise
// 4 and 9 are the exhaustive arms (r3dm_match_pairs) and are not ANN.
extern "C" int r3dm_ann_params_for_algorithm(int matching_algorithm, r3dm_kgraph_params* out)
{
    switch (matching_algorithm) {
        case 1: case 6: return r3dm_kgraph_preset(0, out);
        case 2: case 7: case 5: return r3dm_kgraph_preset(1, out);
        case 3: case 8: case 0: return r3dm_kgraph_preset(2, out);
        default: return R3DM_ERR_INVALID;
    }
}

static int check_kgraph_params(r3dm_ctx* c, const r3dm_kgraph_params* kp)
{
    if (!kp) return R3DM_ERR_INVALID;
    if (kp->index_K < 1 || kp->index_K > kAnnMaxK || kp->search_P < 2 || kp->search_P > 61 || kp->search_S < 1 || kp->search_S > 16) {
        c->err = "kgraph parameters out of range (index_K 1..32, search_P 2..61, search_S 1..16)";
        return R3DM_ERR_INVALID;
    }
    return R3DM_OK;
}

extern "C" int r3dm_exhaustive_is_faster(const r3dm_ctx* c)
{
    if (!c) return 0;
    if (sync_view_stats(const_cast<r3dm_ctx*>(c)) != R3DM_OK) return 0;        // (integer-valued? is a statistic of the staging kernel)
    bool any = false;
    for (const auto& up : c->imgs) {
        if (!up || !up->live) continue;
        const HostImage& h = *up;
        any = true;
        // Binary views: 1 while no view exceeds 32,768 rows, the largest measured size at which the faster exhaustive Hamming path is at
        // least as fast as the Hamming graph matcher's default preset (profiles/ann_hamming_perf.txt, 16 views, pairs/s: line 19, MFMA
        // path 3,084, against line 20, graph 2,476; at 65,536 rows lines 26 / 27: 816 against 829 -- where the graph matcher recovers
        // 0.27 of the exhaustive matches, 0.41 at 32,768 and 0.75 at 8,192: it is the approximate matcher)
        if (h.dtype == R3DM_BIN) { if (h.n > 32768u) return 0; continue; }
        if (!h.not_integer) return 0;                                        // integer-valued rows: the byte-row graph search is the faster one
        if (!has_tensor_kernel(kernel_G_for(h.dim))) return 0;               // other lengths run the one-workgroup-per-query exact scan
        if (h.n > 32768u) return 0;
    }
    return any ? 1 : 0;
}

// compact copy of a view's rows for the search's gathers: bytes for integers 0 .. 255 (ImgDev::ann_rows8), bf16 for other integers
// of magnitude <= 256 (ImgDev::ann_rows16), nothing otherwise.  R3DM_ANN_ROWS16 (developer build): 0 = never, 1 = bf16 only,
// 2 = bytes too, 3 (the product) = and integer dot products when both views of every pair are bytes.
static int stage_compact_rows(r3dm_ctx* c, HostImage& h)
{
    const int compact = r3dm_dev_knob("R3DM_ANN_ROWS16", 3);
    const bool ints = h.dtype != R3DM_BIN && !h.not_integer;
    h.ann_rows16.release(); h.ann_rows8.release();
    if (ints && !h.has_negative && h.max_abs <= 255.0f && (h.dim & 15u) == 0 && compact >= 2) {
        R3DM_HIP(c, h.ann_rows8.ensure((size_t)h.n * h.dim + kSlackBytes));
        R3DM_HIP(c, launch_ann_rows8(c->stream, h.rows.as<float>(), h.ann_rows8.as<uint8_t>(), (size_t)h.n * h.dim));
    } else if (ints && h.max_abs <= 256.0f && (h.dim & 7u) == 0 && compact >= 1) {
        R3DM_HIP(c, h.ann_rows16.ensure((size_t)h.n * h.dim * 2 + kSlackBytes));
        R3DM_HIP(c, launch_ann_rows16(c->stream, h.rows.as<float>(), h.ann_rows16.as<uint16_t>(), (size_t)h.n * h.dim));
    }
    h.compact_ready = true;
    return R3DM_OK;
}

// the query side of the integer-dot-product search: views that are only ever J hold no index, but may hold the byte copy
static int ensure_compact_rows(r3dm_ctx* c, std::vector<uint32_t> slots)
{
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    std::vector<const void*> ptrs;
    ptrs.reserve(2 * slots.size());                          // must outlive the asynchronous copies: no reallocation below
    bool any = false;
    for (uint32_t s : slots) {
        HostImage& h = *c->imgs[s];
        if (h.compact_ready) continue;
        int rc = stage_compact_rows(c, h);
        if (rc != R3DM_OK) return rc;
        ptrs.push_back(h.ann_rows16.p); ptrs.push_back(h.ann_rows8.p);
        R3DM_HIP(c, hipMemcpyAsync((void*)&(c->d_imgs.as<ImgDev>() + s)->ann_rows16, &ptrs[ptrs.size() - 2], 2 * sizeof(void*),
                                   hipMemcpyHostToDevice, c->stream));
        any = true;
    }
    if (any) R3DM_HIP(c, hipStreamSynchronize(c->stream));
    return R3DM_OK;
}

// builds the graph index of every listed slot that does not hold one for this K
int ensure_ann_indices(r3dm_ctx* c, std::vector<uint32_t> slots, uint32_t K)
{
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    std::vector<uint32_t> todo;
    for (uint32_t s : slots) if (c->imgs[s]->ann_K != K) todo.push_back(s);
    if (todo.empty()) return R3DM_OK;
    // The index is the EXACT K-NN graph (+ reverse edges): an all-pairs scan of the view against itself, O(n^2 dim) -- 1.1-4.4 ms per
    // 16 k-row view, the right builder at every size BASELINE names, and the wrong one far beyond: at R3DM_KGRAPH_MAX_ROWS rows it is
    // ~0.3 s per view and grows fourfold per doubling.  The reference's NN-descent (kgraph.cpp:703-999) is not built here; a larger view
    // is refused by name rather than indexed silently in quadratic time (the exhaustive matcher serves it: r3dm_match_pairs).
    for (uint32_t s : todo)
        if (c->imgs[s]->n > R3DM_KGRAPH_MAX_ROWS) {
            c->err = "kgraph index: view of " + std::to_string(c->imgs[s]->n) + " rows exceeds R3DM_KGRAPH_MAX_ROWS (" + std::to_string(R3DM_KGRAPH_MAX_ROWS) +
                     "): the exact K-NN graph build is quadratic in the rows";
            return R3DM_ERR_UNSUPPORTED;
        }
    R3DM_HIP(c, hipEventRecord(c->ev0, c->stream));
    size_t start = 0;
    while (start < todo.size()) {
        // chunk: bounded scratch (fwd + rev keys: 16 B per edge slot)
        size_t end = start, bytes = 0;
        uint32_t max_n = 0;
        const uint32_t dim = c->imgs[todo[start]]->dim;
        const bool binary = c->imgs[todo[start]]->dtype == R3DM_BIN;       // packed rows under Hamming: the build reads ImgDev::bin
        while (end < todo.size() && end - start < 256) {
            const HostImage& h = *c->imgs[todo[end]];
            if (h.dim != dim || (h.dtype == R3DM_BIN) != binary) break;
            const size_t need = (size_t)h.n * K * 16 + (size_t)h.n * 12 + 64;
            if (end > start && bytes + need > (4ull << 30)) break;
            bytes += need; max_n = std::max(max_n, h.n); ++end;
        }
        R3DM_HIP(c, c->a_scratch.ensure(bytes));
        R3DM_HIP(c, hipMemsetAsync(c->a_scratch.p, 0, bytes, c->stream));
        std::vector<AnnBuildJob> jobs;
        bool all_rows8 = r3dm_dev_knob("R3DM_ANN_ROWS16", 3) >= 3;
        unsigned char* cur = c->a_scratch.as<unsigned char>();
        for (size_t k = start; k < end; ++k) {
            HostImage& h = *c->imgs[todo[k]];
            R3DM_HIP(c, h.ann_adj.ensure((size_t)h.n * kAnnDeg * 4));
            R3DM_HIP(c, h.ann_deg.ensure((size_t)h.n * 4));
            AnnBuildJob j{};
            j.slot = todo[k];
            j.fwd = (unsigned long long*)cur; cur += (size_t)h.n * K * 8;
            j.rev = (unsigned long long*)cur; cur += (size_t)h.n * K * 8;
            j.rev_cnt = (uint32_t*)cur; cur += (size_t)h.n * 4;
            j.rev_cur = (uint32_t*)cur; cur += (size_t)h.n * 4;
            j.rev_off = (uint32_t*)cur; cur += (size_t)h.n * 4 + 64;
            j.adj = h.ann_adj.as<uint32_t>(); j.deg = h.ann_deg.as<uint32_t>();
            if (!h.compact_ready) { const int rcc = stage_compact_rows(c, h); if (rcc != R3DM_OK) return rcc; }
            j.rows8 = h.ann_rows8.as<uint8_t>();
            all_rows8 = all_rows8 && j.rows8 != nullptr;
            jobs.push_back(j);
        }
        R3DM_HIP(c, c->a_jobs.ensure(jobs.size() * sizeof(AnnBuildJob)));
        R3DM_HIP(c, hipMemcpyAsync(c->a_jobs.p, jobs.data(), jobs.size() * sizeof(AnnBuildJob), hipMemcpyHostToDevice, c->stream));
        AnnBuildParams bp{};
        bp.imgs = c->d_imgs.as<ImgDev>(); bp.jobs = c->a_jobs.as<AnnBuildJob>(); bp.K = K;
        hipError_t e = launch_ann_build(c->stream, bp, (uint32_t)jobs.size(), max_n, dim, !binary && all_rows8 && dim <= 256 && (dim & 15u) == 0,
                                        binary ? c->imgs[todo[start]]->words : 0u);
        if (binary && e == hipSuccess) c->kgraph_hamming_stats.n_index_builds += jobs.size();
        if (e == hipErrorInvalidValue) { c->err = "no graph-index kernel for this descriptor length (dim % 4 != 0 or too long)"; return R3DM_ERR_UNSUPPORTED; }
        R3DM_HIP(c, e);
        static_assert(offsetof(ImgDev, ann_deg) == offsetof(ImgDev, ann_adj) + sizeof(void*) &&
                      offsetof(ImgDev, ann_rows16) == offsetof(ImgDev, ann_adj) + 2 * sizeof(void*) &&
                      offsetof(ImgDev, ann_rows8) == offsetof(ImgDev, ann_adj) + 3 * sizeof(void*), "index pointers are set with one copy");
        std::vector<const void*> ptrs(4 * (end - start));      // must outlive the asynchronous copies
        for (size_t k = start; k < end; ++k) {
            HostImage& h = *c->imgs[todo[k]];
            const void** q = &ptrs[4 * (k - start)];
            q[0] = h.ann_adj.p; q[1] = h.ann_deg.p; q[2] = h.ann_rows16.p; q[3] = h.ann_rows8.p;
            R3DM_HIP(c, hipMemcpyAsync((void*)&(c->d_imgs.as<ImgDev>() + todo[k])->ann_adj, q, 4 * sizeof(void*),
                                       hipMemcpyHostToDevice, c->stream));
            h.ann_K = K;
        }
        R3DM_HIP(c, hipStreamSynchronize(c->stream));          // jobs / ptrs are host temporaries; scratch is reused
        start = end;
    }
    R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.ms_ann_build += ms;
    c->stats.n_ann_built += todo.size();
    return R3DM_OK;
}

// graph search + ratio test over `jobs` (all of one dim; every sI holds an index), results appended to g in job order
// knn_k = 0: the 2-NN search (pool of 2 + P entries, ratio test, optional 2-lists); 1 .. R3DM_KNN_MAX: the k-list search of one pair
// (pool of knn_k + P entries as KGraphImpl::search sizes it, kgraph.cpp:418; knn_*_host receive knn_k entries per query)
static int run_kgraph_batch(r3dm_ctx* c, const std::vector<PairJob>& jobs, float ratio_R, const r3dm_kgraph_params& kp,
                            r3dm_graph* g, int32_t* knn_idx_host, float* knn_dist_host, uint32_t knn_k = 0)
{
    std::vector<uint2> hid(jobs.size());                     // the search is seeded by (I, J); outlives the frame's synchronisation
    bool rows16 = true, rows8 = true, dot8 = r3dm_dev_knob("R3DM_ANN_ROWS16", 3) >= 3;   // every indexed view of the batch holds that compact row copy
    const int rc = run_ann_batch(c, jobs, g, knn_idx_host, knn_dist_host, [&](const AnnBatch& b) -> int {
        for (uint32_t p = 0; p < b.P; ++p) hid[p] = make_uint2(jobs[p].I, jobs[p].J);
        R3DM_HIP(c, c->a_ids.ensure(sizeof(uint2) * b.P));
        R3DM_HIP(c, hipMemcpyAsync(c->a_ids.p, hid.data(), sizeof(uint2) * b.P, hipMemcpyHostToDevice, c->stream));
        AnnSearchParams sp{};
        sp.imgs = c->d_imgs.as<ImgDev>(); sp.pairs = c->d_pairs.as<uint2>(); sp.pair_ids = c->a_ids.as<uint2>();
        sp.n_pairs = b.P; sp.q_stride = b.q_stride;
        sp.P = kp.search_P; sp.S = kp.search_S; sp.pool_cap = (knn_k ? knn_k : 2u) + kp.search_P; sp.seed = kp.seed; sp.ratio_R = ratio_R;
        sp.nn_idx = b.nn_idx; sp.knn_idx = b.knn_idx; sp.knn_dist = b.knn_dist; sp.n_comps = b.n_comps;
        for (const PairJob& j : jobs) {
            const HostImage& A = *c->imgs[j.sI];
            const HostImage& B = *c->imgs[j.sJ];
            rows16 = rows16 && A.compact_ready && A.ann_rows16.p != nullptr;
            rows8 = rows8 && A.compact_ready && A.ann_rows8.p != nullptr;
            dot8 = dot8 && B.compact_ready && B.ann_rows8.p != nullptr;        // ... and every query view its byte copy
        }
        const bool binary = c->imgs[jobs[0].sI]->dtype == R3DM_BIN;             // (a batch is of one dtype and length)
        if (binary) { dot8 = false; rows8 = false; rows16 = false; }
        dot8 = dot8 && rows8 && b.dim <= 256 && (b.dim & 15u) == 0;
        // descriptor lengths 132 .. 144 (nine float4 per lane: LIOP-144) have no compact-row instantiation of the search kernel
        // (launch_ann_search): integer-valued views of that length gather the f32 rows
        if ((b.dim / 4 + 3) / 4 == 9) { dot8 = false; rows8 = false; rows16 = false; }
        const hipError_t e = launch_ann_search(c->stream, sp, b.max_nJ, b.max_nI, b.dim, binary ? 4 : dot8 ? 3 : rows8 ? 2 : (rows16 ? 1 : 0), knn_k);
        if (binary && e == hipSuccess) c->kgraph_hamming_stats.n_search_launches += 1;
        if (e == hipErrorInvalidValue) { c->err = "graph search: unsupported descriptor length / view size / parameters"; return R3DM_ERR_UNSUPPORTED; }
        R3DM_HIP(c, e);
        return R3DM_OK;
    }, knn_k ? knn_k : 2u, ForwardRatio{ratio_R, false});
    if (rc != R3DM_OK || jobs.empty()) return rc;
    c->stats.n_ann_rows16 += (rows16 && !rows8) ? 1 : 0;
    c->stats.n_ann_rows8 += rows8 ? 1 : 0;
    c->stats.n_ann_dot8 += dot8 ? 1 : 0;
    return R3DM_OK;
}

static int r3dm_match_pairs_kgraph_impl(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs, float dist_ratio,
                                       const r3dm_kgraph_params* kp, r3dm_graph** out)
{
    if (!c || !out || (n_pairs && !pairs_ij)) return R3DM_ERR_INVALID;
    *out = nullptr;
    const int rcp = check_kgraph_params(c, kp);
    if (rcp != R3DM_OK) return rcp;
    const float R = dist_ratio * dist_ratio;
    AnnArm arm;
    // binary views (r3dm_set_kgraph_hamming): the ratio unsquared, in the search, the scanned part and the gate alike
    if (c->kgraph_hamming) arm.bin_ratio_R = dist_ratio;
    arm.classify = [&](const HostImage& A, bool& index) -> int {
        if (A.dtype == R3DM_BIN ? !c->kgraph_hamming : (A.dim & 3u) != 0) { c->err = "kgraph matching needs F32/U8 descriptors with dim % 4 == 0"; return R3DM_ERR_UNSUPPORTED; }
        // KGraphImpl::search scans linearly when P >= n (kgraph.cpp:415-421); here every small index is scanned
        index = !(A.n < kAnnMinRows || kp->search_P >= A.n);
        return R3DM_OK;
    };
    arm.ensure = [&](const std::vector<PairJob>& jobs) -> int {
        std::vector<uint32_t> slots;
        // the graph build and the graph search gather row-major rows (f32, or the compact copies made from them)
        for (const PairJob& j : jobs) { slots.push_back(j.sI); slots.push_back(j.sJ); }
        int rc = ensure_layouts(c, slots, kLayRows);
        if (rc != R3DM_OK) return rc;
        slots.clear();
        for (const PairJob& j : jobs) slots.push_back(j.sI);
        rc = ensure_ann_indices(c, slots, kp->index_K);
        if (rc != R3DM_OK) return rc;
        slots.clear();
        for (const PairJob& j : jobs) slots.push_back(j.sJ);
        return ensure_compact_rows(c, slots);
    };
    arm.run_batch = [&](const std::vector<PairJob>& batch, r3dm_graph* g) {
        return run_kgraph_batch(c, batch, c->imgs[batch[0].sI]->dtype == R3DM_BIN ? dist_ratio : R, *kp, g, nullptr, nullptr);
    };
    arm.one_dim_per_chunk = true;                            // (no cap on a chunk's pairs: the search has no per-pair grid dimension)
    return match_collection_ann(c, pairs_ij, n_pairs, R, arm, out);
}

extern "C" int r3dm_match_pairs_kgraph(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs, float dist_ratio,
                                       const r3dm_kgraph_params* kp, r3dm_graph** out)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_match_pairs_kgraph_impl(c, pairs_ij, n_pairs, dist_ratio, kp, out); });
}

// the length check of an array entry: float rows in fours; packed rows (the _bits entries) of 8 or 16 words, as every binary view
static int check_kgraph_row_length(r3dm_ctx* c, r3dm_dtype dtype, uint32_t dim)
{
    if (dtype == R3DM_BIN) {
        if (((dim + 3) / 4) == 8 || ((dim + 3) / 4) == 16) return R3DM_OK;
        c->err = "binary descriptors must be 29..32 or 61..64 bytes";
        return R3DM_ERR_UNSUPPORTED;
    }
    if (dim & 3u) { c->err = "kgraph matching needs dim % 4 == 0"; return R3DM_ERR_UNSUPPORTED; }
    return R3DM_OK;
}

static int r3dm_kgraph_knn2_impl(r3dm_ctx* c, r3dm_dtype dtype, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query,
                                uint32_t dim, const r3dm_kgraph_params* kp, uint32_t pair_i, uint32_t pair_j,
                                int32_t* out_idx, float* out_dist)
{
    if (!c || !dataset || !query || !out_idx || !out_dist || dim == 0) return R3DM_ERR_INVALID;
    if (n_query < 1 || n_dataset < 2) return R3DM_ERR_INVALID;
    int rc = check_kgraph_params(c, kp);
    if (rc != R3DM_OK) return rc;
    rc = check_kgraph_row_length(c, dtype, dim);
    if (rc != R3DM_OK) return rc;
    // like r3dm_knn2: which rows this call gathered, how many evaluations
    return with_staged_pair_of(c, dtype, dataset, n_dataset, query, n_query, dim, pair_i, pair_j,
                            {&r3dm_stats::n_ann_rows16, &r3dm_stats::n_ann_rows8, &r3dm_stats::n_ann_dot8, &r3dm_stats::n_ann_dist}, {},
                            [&](uint32_t sI, uint32_t sJ) -> int {
        const std::vector<PairJob> jobs{{pair_i, pair_j, sI, sJ}};
        if (n_dataset < kAnnMinRows || kp->search_P >= n_dataset) return run_match_batch(c, jobs, 1.0f, nullptr, out_idx, out_dist);
        int rc = ensure_layouts(c, {sI, sJ}, kLayRows);
        if (rc == R3DM_OK) rc = ensure_ann_indices(c, {sI}, kp->index_K);
        if (rc == R3DM_OK) rc = ensure_compact_rows(c, {sJ});
        if (rc == R3DM_OK) rc = run_kgraph_batch(c, jobs, 1.0f, *kp, nullptr, out_idx, out_dist);
        return rc;
    });
}

extern "C" int r3dm_kgraph_knn2(r3dm_ctx* c, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query,
                                uint32_t dim, const r3dm_kgraph_params* kp, uint32_t pair_i, uint32_t pair_j,
                                int32_t* out_idx, float* out_dist)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_kgraph_knn2_impl(c, R3DM_F32, dataset, n_dataset, query, n_query, dim, kp, pair_i, pair_j, out_idx, out_dist); });
}

extern "C" int r3dm_kgraph_knn2_bits(r3dm_ctx* c, const uint8_t* dataset, uint32_t n_dataset, const uint8_t* query, uint32_t n_query,
                                     uint32_t n_bytes, const r3dm_kgraph_params* kp, uint32_t pair_i, uint32_t pair_j,
                                     int32_t* out_idx, float* out_dist)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_kgraph_knn2_impl(c, R3DM_BIN, dataset, n_dataset, query, n_query, n_bytes, kp, pair_i, pair_j, out_idx, out_dist); });
}

// ---- k neighbours, k = 1 .. R3DM_KNN_MAX: ArrayMatcher_kgraph::SearchNeighbours with any NN (matcher_kgraph.h:205-251, sparams.K = NN)
static int check_kgraph_knn(r3dm_ctx* c, const r3dm_kgraph_params* kp, uint32_t k, uint32_t n_dataset, uint32_t n_query)
{
    if (k < 1 || k > R3DM_KNN_MAX || n_query < 1 || n_dataset < k) return R3DM_ERR_INVALID;     // the plugins' "NN > rows" rule
    const int rc = check_kgraph_params(c, kp);
    if (rc != R3DM_OK) return rc;
    if (k + kp->search_P > 63) { c->err = "kgraph k-NN: the pool holds k + search_P entries, 63 at most"; return R3DM_ERR_INVALID; }
    return R3DM_OK;
}

// the search of one staged pair whose dataset slot holds the index
static int kgraph_knn_search(r3dm_ctx* c, const r3dm_kgraph_params& kp, uint32_t pair_i, uint32_t pair_j, uint32_t sI, uint32_t sJ, uint32_t k,
                             int32_t* out_idx, float* out_dist)
{
    int rc = ensure_layouts(c, {sI, sJ}, kLayRows);
    if (rc == R3DM_OK) rc = ensure_ann_indices(c, {sI}, kp.index_K);
    if (rc == R3DM_OK) rc = ensure_compact_rows(c, {sJ});
    if (rc == R3DM_OK) rc = run_kgraph_batch(c, {{pair_i, pair_j, sI, sJ}}, 1.0f, kp, nullptr, out_idx, out_dist, k);
    return rc;
}

static int r3dm_kgraph_knn_impl(r3dm_ctx* c, r3dm_dtype dtype, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query,
                               uint32_t dim, const r3dm_kgraph_params* kp, uint32_t pair_i, uint32_t pair_j, uint32_t k,
                               int32_t* out_idx, float* out_dist)
{
    return r3dm_guarded(c, [&]() -> int {
        if (!c || !dataset || !query || !out_idx || !out_dist || dim == 0) return R3DM_ERR_INVALID;
        int rc = check_kgraph_knn(c, kp, k, n_dataset, n_query);
        if (rc != R3DM_OK) return rc;
        rc = check_kgraph_row_length(c, dtype, dim);
        if (rc != R3DM_OK) return rc;
        return with_staged_pair_of(c, dtype, dataset, n_dataset, query, n_query, dim, pair_i, pair_j,
                                {&r3dm_stats::n_ann_rows16, &r3dm_stats::n_ann_rows8, &r3dm_stats::n_ann_dot8, &r3dm_stats::n_ann_dist},
                                {&r3dm_stats::ms_ann_build, &r3dm_stats::ms_ann_search}, [&](uint32_t sI, uint32_t sJ) -> int {
            // as r3dm_kgraph_knn2: a small dataset, or one the start rows would cover, is scanned
            if (n_dataset < kAnnMinRows || kp->search_P >= n_dataset) return run_exact_knn_pair(c, sI, sJ, k, out_idx, out_dist);
            return kgraph_knn_search(c, *kp, pair_i, pair_j, sI, sJ, k, out_idx, out_dist);
        });
    });
}

extern "C" int r3dm_kgraph_knn(r3dm_ctx* c, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query,
                               uint32_t dim, const r3dm_kgraph_params* kp, uint32_t pair_i, uint32_t pair_j, uint32_t k,
                               int32_t* out_idx, float* out_dist)
{
    return r3dm_kgraph_knn_impl(c, R3DM_F32, dataset, n_dataset, query, n_query, dim, kp, pair_i, pair_j, k, out_idx, out_dist);
}

extern "C" int r3dm_kgraph_knn_bits(r3dm_ctx* c, const uint8_t* dataset, uint32_t n_dataset, const uint8_t* query, uint32_t n_query,
                                    uint32_t n_bytes, const r3dm_kgraph_params* kp, uint32_t pair_i, uint32_t pair_j, uint32_t k,
                                    int32_t* out_idx, float* out_dist)
{
    return r3dm_kgraph_knn_impl(c, R3DM_BIN, dataset, n_dataset, query, n_query, n_bytes, kp, pair_i, pair_j, k, out_idx, out_dist);
}

extern "C" int r3dm_index_kgraph_knn(r3dm_ctx* c, const r3dm_index* ix, const r3dm_kgraph_params* kp, const void* query, uint32_t n_query,
                                     uint32_t pair_i, uint32_t pair_j, uint32_t k, int32_t* out_idx, float* out_dist)
{
    return r3dm_guarded(c, [&]() -> int {
        if (!c || !ix || !query || !out_idx || !out_dist) return R3DM_ERR_INVALID;
        int rc = check_kgraph_knn(c, kp, k, ix->img.n, n_query);
        if (rc != R3DM_OK) return rc;
        // as r3dm_match_pairs_kgraph scans such views: the exhaustive k-NN of the index, exactly
        if (ix->img.n < kAnnMinRows || kp->search_P >= ix->img.n) return r3dm_index_knn(c, ix, query, n_query, k, out_idx, out_dist);
        if (ix->img.dtype == R3DM_BIN ? !c->kgraph_hamming : (ix->img.dim & 3u) != 0) { c->err = "kgraph matching needs F32/U8 descriptors with dim % 4 == 0"; return R3DM_ERR_UNSUPPORTED; }
        CallCounters counters(c, {&r3dm_stats::n_ann_rows16, &r3dm_stats::n_ann_rows8, &r3dm_stats::n_ann_dot8, &r3dm_stats::n_ann_dist, &r3dm_stats::n_ann_built},
                              {&r3dm_stats::ms_ann_build, &r3dm_stats::ms_ann_search});
        return with_index_structure(c, ix, query, n_query,
            [&](const r3dm_index& x) -> int {
                if (!x.kgraph_built) return 1;
                if (x.kgraph_p.index_K != kp->index_K) { c->err = "r3dm_index_kgraph_knn: the index holds a graph of another index_K"; return R3DM_ERR_INVALID; }
                return R3DM_OK;
            },
            [&](r3dm_index& x, uint32_t slot) -> int {
                const int rcb = ensure_ann_indices(c, {slot}, kp->index_K);
                if (rcb == R3DM_OK) { x.kgraph_built = true; x.kgraph_p = *kp; }
                return rcb;
            },
            [&](uint32_t sI, uint32_t sJ) { return kgraph_knn_search(c, *kp, pair_i, pair_j, sI, sJ, k, out_idx, out_dist); });
    });
}

extern "C" int r3dm_drop_indices(r3dm_ctx* c)
{
    if (!c) return R3DM_ERR_INVALID;
    for (auto& h : c->imgs) if (h) { h->ann_K = 0; h->hnsw_M = 0; h->mrpt_trees = 0; }            // the device pointers stay valid until the rebuild replaces them
    return R3DM_OK;
}

extern "C" int r3dm_kgraph_index(r3dm_ctx* c, uint32_t view_id, uint32_t index_K, uint32_t* adj_out, uint32_t* deg_out)
{
    if (!c || !adj_out || !deg_out) return R3DM_ERR_INVALID;
    auto it = c->slot_of.find(view_id);
    if (it == c->slot_of.end()) { c->err = "unregistered view"; return R3DM_ERR_INVALID; }
    if (index_K < 1 || index_K > kAnnMaxK) return R3DM_ERR_INVALID;
    HostImage& h = *c->imgs[it->second];
    if ((h.dtype == R3DM_BIN ? !c->kgraph_hamming : (h.dim & 3u) != 0) || h.n < 2) { c->err = "kgraph index needs >= 2 F32/U8 rows with dim % 4 == 0"; return R3DM_ERR_UNSUPPORTED; }
    R3DM_HIP(c, hipSetDevice(c->device));
    int rc = ensure_layouts(c, {it->second}, kLayRows);
    if (rc == R3DM_OK) rc = ensure_ann_indices(c, {it->second}, index_K);
    if (rc != R3DM_OK) return rc;
    R3DM_HIP(c, hipMemcpy(adj_out, h.ann_adj.p, (size_t)h.n * kAnnDeg * 4, hipMemcpyDeviceToHost));
    R3DM_HIP(c, hipMemcpy(deg_out, h.ann_deg.p, (size_t)h.n * 4, hipMemcpyDeviceToHost));
    return R3DM_OK;
}


// ---- binary views on the graph matcher (kernels_ann.hip: ann_knn_bits_kernel, the ROWS 4 arm of ann_search_kernel)
extern "C" int r3dm_set_kgraph_hamming(r3dm_ctx* c, int enable)
{
    if (!c) return R3DM_ERR_INVALID;
    c->kgraph_hamming = enable != 0;
    return R3DM_OK;
}

extern "C" int r3dm_kgraph_hamming_report(const r3dm_ctx* c, r3dm_kgraph_hamming_stats* out)
{
    if (!c || !out) return R3DM_ERR_INVALID;
    *out = c->kgraph_hamming_stats;
    return R3DM_OK;
}
