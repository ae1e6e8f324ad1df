// compute_matches.cpp -- implementation of the R3DComputeMatches facade (include/r3d_compute_matches.hpp)
// on top of the C ABI only.  Stage order follows /root/reference/src/R3DComputeMatches.cpp:1994-2240, one member function per phase:
// features of the views without files (runFeaturesStage) -> load regions (loadViews) -> exhaustive pairs, or the proposed ones
// (listPairs) -> match (matchPutative) -> save matches.putative.txt (startPutativeFiles) -> F / E / H filters and matches.f / .e / .h.txt
// (runFilters) -> adjacency SVG, wait for the files (finishFiles).  One device or a device list: `Devices` decides, nothing else does.
// The overlap lives in `Background`: every graph's files and map are written on host threads behind whatever the GPU does next.
#include "../../include/r3d_compute_matches.hpp"
#include "feat_text.hpp"
#include "descriptor_arms.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <memory>
#include <thread>
#include <sys/resource.h>
#include <sys/syscall.h>
#include <unistd.h>

namespace r3d_amd {

namespace {

using r3dm_feat::load_feat;      // feat_text.hpp

// first thing in a background writer thread: its work has a whole phase to hide behind, so under contention for the host's cores it
// stands back (Linux: a per-thread nice value, inherited by the helpers it starts)
// (only when the host asked for it: R3DComputeMatches::setBackgroundThreadsNice)
static inline void stand_back(int nice_value) { if (nice_value > 0) (void)setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), nice_value); }

// Save(PairWiseMatches, file) of the .txt and the .bin of a graph on two host threads while the next filter runs on the GPU; the
// destructor waits for every write and frees the graphs it was given
struct MatchFileWriter {
    struct Job { std::thread th; int rc = R3DM_OK; std::string path; };
    std::vector<std::unique_ptr<Job>> jobs;
    std::vector<r3dm_graph*> owned;
    int nice_value = 0;
    void save(const r3dm_graph* g, const std::string& txt_path, const std::string& bin_path)
    {
        const int nv = nice_value;
        for (const std::string& p : {txt_path, bin_path}) {
            std::unique_ptr<Job> j(new Job());
            j->path = p;
            Job* raw = j.get();
            try { raw->th = std::thread([g, raw, nv]() noexcept { stand_back(nv); raw->rc = r3dm_save_matches(g, raw->path.c_str()); }); }
            catch (...) { raw->rc = r3dm_save_matches(g, raw->path.c_str()); }             // no thread to be had: write here
            jobs.push_back(std::move(j));
        }
    }
    void own(r3dm_graph* g) { owned.push_back(g); }
    // waits for all writes; the path of the first one that failed, or ""
    std::string finish()
    {
        std::string bad;
        for (auto& j : jobs) { if (j->th.joinable()) j->th.join(); if (j->rc != R3DM_OK && bad.empty()) bad = j->path; }
        jobs.clear();
        for (r3dm_graph* g : owned) r3dm_graph_free(g);
        owned.clear();
        return bad;
    }
    ~MatchFileWriter() { (void)finish(); }
};

bool load_desc(const std::string& path, size_t row_bytes, std::vector<unsigned char>& data, uint64_t& n)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    bool ok = fread(&n, 8, 1, f) == 1;
    if (ok) {
        // the count comes from the file: check it against what the file can hold before sizing anything by it
        ok = fseek(f, 0, SEEK_END) == 0;
        const long sz = ok ? ftell(f) : -1;
        ok = ok && sz >= 8 && row_bytes > 0 && n <= (uint64_t)(sz - 8) / row_bytes && fseek(f, 8, SEEK_SET) == 0;
    }
    if (ok) {
        data.resize((size_t)n * row_bytes);
        ok = n == 0 || fread(data.data(), row_bytes, n, f) == n;
    }
    fclose(f);
    return ok;
}

void graph_to_map(const r3dm_graph* g, PairWiseMatches& out)
{
    out.clear();
    const uint64_t np = r3dm_graph_num_pairs(g);
    const uint32_t* p = r3dm_graph_pairs(g);
    const uint64_t* o = r3dm_graph_offsets(g);
    const r3dm_match* m = r3dm_graph_matches(g);
    for (uint64_t k = 0; k < np; ++k)
        out.emplace(std::make_pair(p[2 * k], p[2 * k + 1]), MatchList(m + o[k], m + o[k + 1]));
}

// PairWiseMatchingToAdjacencyMatrixSVG (/root/reference/src/R3DComputeMatches.cpp:2074,2238; OpenMVG, external):
// an N x N grid, 5 px per view, a blue square at (J, I) for every pair that kept matches, axis labels 0 / N.
// Same geometry as upstream; the markup is not byte-identical to OpenMVG's svgDrawer output.
bool write_adjacency_svg(const std::string& path, size_t n_views, const PairWiseMatches& m)
{
    if (m.empty()) return true;                             // upstream writes nothing for an empty map
    FILE* f = fopen(path.c_str(), "w");
    if (!f) return false;
    const double s = 5.0;
    const double wh = (n_views + 3) * s;
    fprintf(f, "<?xml version=\"1.0\" standalone=\"yes\"?>\n<svg width=\"%g\" height=\"%g\" version=\"1.1\" "
               "xmlns=\"http://www.w3.org/2000/svg\">\n", wh, wh);
    for (const auto& kv : m) {
        if (kv.second.empty()) continue;
        fprintf(f, "<rect x=\"%g\" y=\"%g\" width=\"%g\" height=\"%g\" fill=\"blue\" stroke=\"none\">"
                   "<title>(%u,%u %zu)</title></rect>\n",
                kv.first.second * s, kv.first.first * s, s / 2.0, s / 2.0, kv.first.second, kv.first.first, kv.second.size());
    }
    fprintf(f, "<text x=\"%g\" y=\"%g\" font-size=\"%g\" fill=\"black\">0</text>\n", (n_views + 1) * s, s, s);
    fprintf(f, "<text x=\"%g\" y=\"%g\" font-size=\"%g\" fill=\"black\">%zu</text>\n", (n_views + 1) * s, n_views * s - s, s, n_views);
    fprintf(f, "<polyline points=\"%g,0 %g,%g 0,%g\" fill=\"none\" stroke=\"black\" stroke-width=\"1\"/>\n",
            n_views * s, n_views * s, n_views * s, n_views * s);
    fprintf(f, "</svg>\n");
    return fclose(f) == 0;
}

double wall_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

bool file_exists(const std::string& p) { FILE* f = fopen(p.c_str(), "rb"); if (!f) return false; fclose(f); return true; }

std::string with_ext(const std::string& path, const char* ext)
{
    const size_t dot = path.find_last_of('.');
    return (dot == std::string::npos ? path : path.substr(0, dot)) + ext;
}

// what the reference passes to its three Robust_model_estimation calls (:2113-2120 F, :2130-2204 E, :2216-2233 H): AC-RANSAC with a
// 4.0 px upper bound and 2048 iterations; E's overlap rule keeps a pair with >= 50 matches and >= 30 % of its putative ones (:2175-2192)
constexpr double kMaxResidualPx = 4.0;
constexpr uint32_t kMaxIterations = 2048, kEMinCount = 50;
constexpr float kEMinRatio = 0.3f;

// One device (ctx) or the multi-device deal (multi): the same operations either way, and the only place that tells the two apart.
// Where the C ABI has no r3dm_multi_* entry, the operation walks the contexts.  Neither set (no GPU): every operation fails or does nothing.
struct Devices {
    r3dm_ctx* ctx;
    r3dm_multi* multi;
    explicit operator bool() const { return ctx || multi; }
    bool single() const { return ctx != nullptr; }
    int count() const { return ctx ? 1 : (multi ? r3dm_multi_num_devices(multi) : 0); }
    r3dm_ctx* at(int k) const { return ctx ? ctx : r3dm_multi_ctx(multi, k); }
    r3dm_ctx* first_ctx() const { return count() ? at(0) : nullptr; }
    template <class One, class List, class... A> auto call(One one, List list, A... a) const { return ctx ? one(ctx, a...) : list(multi, a...); }
    template <class One, class... A> void on_each(One one, A... a) const { for (int k = 0; k < count(); ++k) (void)one(at(k), a...); }

    std::string last_error() const { return call(r3dm_last_error, r3dm_multi_last_error); }
    int clear_images() const { return call(r3dm_clear_images, r3dm_multi_clear_images); }
    int set_image(uint32_t id, uint32_t w, uint32_t h, const void* desc, uint32_t n, uint32_t dim, r3dm_dtype dtype, const float* xy) const
    { return call(r3dm_set_image, r3dm_multi_set_image, id, w, h, desc, n, dim, dtype, xy); }
    // several views in ONE call (helper threads fill the page-locked ring beside the DMAs): single() only, a list registers view by view
    int set_images(const std::vector<r3dm_view_desc>& v) const { return r3dm_set_images(ctx, v.data(), (uint32_t)v.size()); }
    int set_priority(uint32_t id, const std::vector<float>& s) const { return call(r3dm_set_view_priority, r3dm_multi_set_view_priority, id, s.data(), (uint32_t)s.size()); }
    int set_intrinsics(uint32_t id, const double* K) const { return call(r3dm_set_intrinsics, r3dm_multi_set_intrinsics, id, K); }

    void set_integer_mfma(bool on) const { (void)call(r3dm_set_integer_mfma, r3dm_multi_set_integer_mfma, on ? 1 : 0); }
    void set_split_mfma(bool on) const { on_each(r3dm_set_split_mfma, on ? 1 : 0); }
    void set_hamming_mfma(bool on) const { on_each(r3dm_set_hamming_mfma, on ? 1 : 0); }
    void set_mutual(bool on) const { (void)call(r3dm_set_mutual_matching, r3dm_multi_set_mutual_matching, on ? 1 : 0); }
    void set_symmetric_ratio(bool on) const { (void)call(r3dm_set_symmetric_ratio, r3dm_multi_set_symmetric_ratio, on ? 1 : 0); }
    int set_kgraph_hamming(bool on) const { return call(r3dm_set_kgraph_hamming, r3dm_multi_set_kgraph_hamming, on ? 1 : 0); }
    void set_guided(bool on, double rF, double rE, double rH) const { (void)call(r3dm_set_guided_matching, r3dm_multi_set_guided_matching, on ? 1 : 0, rF, rE, rH); }
    int set_preemptive(bool on, uint32_t head_rows, uint32_t min_matches) const
    { return call(r3dm_set_preemptive_matching, r3dm_multi_set_preemptive_matching, on ? 1 : 0, head_rows, min_matches); }
    int set_budget(bool on, uint32_t max_rows) const { return call(r3dm_set_match_budget, r3dm_multi_set_match_budget, on ? 1 : 0, max_rows); }

    // the four matchers: `how` is the squared flag of the exhaustive one, the parameters of the others
    using Pairs = std::vector<uint32_t>;
    int match(const Pairs& p, float ratio, int how, r3dm_graph** out) const { return call(r3dm_match_pairs, r3dm_multi_match_pairs, p.data(), (uint64_t)(p.size() / 2), ratio, how, out); }
    int match_kgraph(const Pairs& p, float ratio, const r3dm_kgraph_params* how, r3dm_graph** out) const { return call(r3dm_match_pairs_kgraph, r3dm_multi_match_pairs_kgraph, p.data(), (uint64_t)(p.size() / 2), ratio, how, out); }
    int match_hnsw(const Pairs& p, float ratio, const r3dm_hnsw_params* how, r3dm_graph** out) const { return call(r3dm_match_pairs_hnsw, r3dm_multi_match_pairs_hnsw, p.data(), (uint64_t)(p.size() / 2), ratio, how, out); }
    int match_mrpt(const Pairs& p, float ratio, const r3dm_mrpt_params* how, r3dm_graph** out) const { return call(r3dm_match_pairs_mrpt, r3dm_multi_match_pairs_mrpt, p.data(), (uint64_t)(p.size() / 2), ratio, how, out); }

    int filter_F(const r3dm_graph* g, uint64_t seed, r3dm_graph** out) const          // (the list entry has the symmetric epipolar error built in)
    { return ctx ? r3dm_filter_F(ctx, g, kMaxResidualPx, kMaxIterations, seed, R3DM_ERR_SYMMETRIC_EPIPOLAR, out, nullptr) : r3dm_multi_filter_F(multi, g, kMaxResidualPx, kMaxIterations, seed, out, nullptr); }
    int filter_E(const r3dm_graph* g, uint64_t seed, r3dm_graph** out) const
    { return call(r3dm_filter_E, r3dm_multi_filter_E, g, kMaxResidualPx, kMaxIterations, seed, kEMinCount, kEMinRatio, out, (double*)nullptr); }
    int filter_H(const r3dm_graph* g, uint64_t seed, r3dm_graph** out) const
    { return call(r3dm_filter_H, r3dm_multi_filter_H, g, kMaxResidualPx, kMaxIterations, seed, out, (double*)nullptr); }
    // the filters of `which` (bit 0 F, 1 E, 2 H) side by side: one device only (a list deals each filter's pairs to its devices instead)
    int filter_FEH(const r3dm_graph* g, uint64_t seed, int which, r3dm_graph* out[3], double ms_kernels[3], double ms_wall[3]) const
    { return r3dm_filter_FEH(ctx, g, kMaxResidualPx, kMaxIterations, seed, which, kEMinCount, kEMinRatio, &out[0], &out[1], &out[2], ms_kernels, ms_wall); }

    // HIP-event time of the dominant kernel of the last match / filter call (the slowest device of a multi-device deal)
    double kernel_ms(bool filter) const
    {
        double ms = 0;
        for (int k = 0; k < count(); ++k) {
            r3dm_stats st{};
            if (r3dm_get_stats(at(k), &st) == R3DM_OK) ms = std::max(ms, filter ? st.ms_filter_kernels : st.ms_match_kernels + st.ms_ann_search + st.ms_ann_build);
        }
        return ms;
    }
    // the statistics that are reported for one device only (host-side wall times of its last match call)
    bool single_stats(r3dm_stats& st) const { return single() && r3dm_get_stats(ctx, &st) == R3DM_OK; }
};

// one view's files as the load step parsed them
struct Loaded { std::vector<float> xy, scale; std::vector<unsigned char> desc; uint64_t n = 0; bool ok = false; };

// a PairWiseMatches map (what the reference keeps in its statistics, :2040-2069) filled on a host thread beside the filters: a
// million matches into per-pair vectors is host work nothing on the device waits for
struct MapJob {
    std::thread th;
    const r3dm_graph* g = nullptr; PairWiseMatches* out = nullptr;
    std::atomic<bool> failed{false};
    void start(const r3dm_graph* g_, PairWiseMatches* out_, int nv)
    {
        g = g_; out = out_;
        try { th = std::thread([this, nv]() { stand_back(nv); try { graph_to_map(g, *out); } catch (...) { failed.store(true); } }); }
        catch (...) { graph_to_map(g, *out); }                                            // no thread to be had: build it here
    }
    // a map the background thread could not build (out of memory) is built again HERE, where a second failure reaches the caller
    // as the exception it is -- never an empty map behind a `true` from computeMatches
    void join() { if (th.joinable()) th.join(); if (failed.exchange(false)) { out->clear(); graph_to_map(g, *out); } }
    ~MapJob() { if (th.joinable()) th.join(); }                                           // (unwinding only: every return path calls join())
};

// the feature files of a call are complete when it returns, however it returns (r3dm_set_deferred_feature_files)
struct FeatureFilesGuard {
    r3dm_multi* const& feat_multi;
    ~FeatureFilesGuard() { if (feat_multi) (void)r3dm_multi_features_files_wait(feat_multi, nullptr, 0); }
};

// the three geometric filters, in the reference's order: who asks for it, the call, where its graph goes, how it is announced and timed
using Stats = R3DComputeMatches::R3DComputeMatchesStatistics;
using Phases = R3DComputeMatches::PhaseTimes;
struct FilterEntry {
    bool R3DFParams::*asked;
    int (Devices::*call)(const r3dm_graph*, uint64_t, r3dm_graph**) const;
    PairWiseMatches Stats::*map;
    std::string R3DProjectPaths::*named; const char* default_name;
    float fraction; const char* message;                              // updateProgress of the reference (:2107, :2133, :2209)
    double Phases::*wall; double Phases::*kernels;
};
const FilterEntry kFilters[3] = {
    {&R3DFParams::computeFundalmentalMatrix_, &Devices::filter_F, &Stats::fundamentalMatches_, &R3DProjectPaths::matchesFFilename_, "/matches.f.txt",
     0.8f, "Calculate fundamental matrix", &Phases::filter_F, &Phases::F_kernels},
    {&R3DFParams::computeEssentialMatrix_, &Devices::filter_E, &Stats::essentialMatches_, &R3DProjectPaths::matchesEFilename_, "/matches.e.txt",      // feeds the global SfM engine
     0.9f, "Calculate essential matrix", &Phases::filter_E, &Phases::E_kernels},
    {&R3DFParams::computeHomographyMatrix_, &Devices::filter_H, &Stats::homographyMatches_, &R3DProjectPaths::matchesHFilename_, "/matches.h.txt",
     0.95f, "Calculate homography matrix", &Phases::filter_H, &Phases::H_kernels}};

// r3dm_features_totals field by field: a = op(a, b)
template <class Op>
void combine(r3dm_features_totals& a, const r3dm_features_totals& b, Op op)
{
    a.n_images = op(a.n_images, b.n_images); a.n_passes = op(a.n_passes, b.n_passes); a.n_keypoints = op(a.n_keypoints, b.n_keypoints);
    a.n_regrows = op(a.n_regrows, b.n_regrows); a.ms_detect_kernels = op(a.ms_detect_kernels, b.ms_detect_kernels);
    a.detect_algorithmic_bytes = op(a.detect_algorithmic_bytes, b.detect_algorithmic_bytes);
    a.ms_liop_kernels = op(a.ms_liop_kernels, b.ms_liop_kernels); a.ms_wall = op(a.ms_wall, b.ms_wall); a.ms_files = op(a.ms_files, b.ms_files);
}
// ... summed over the contexts of the features stage (each context's totals run since it was created)
r3dm_features_totals features_totals(r3dm_multi* m)
{
    r3dm_features_totals sum{};
    for (int k = 0; k < r3dm_multi_num_devices(m); ++k) {
        r3dm_features_totals t{};
        (void)r3dm_get_features_totals(r3dm_multi_ctx(m, k), &t);
        combine(sum, t, [](auto x, auto y) { return x + y; });
    }
    return sum;
}

}  // namespace

// What a computeMatches call has running on host threads behind the GPU: the writers of the match files and the builders of the
// PairWiseMatches maps.  Every graph goes the same way (emit); the writer frees it when its files are written.
struct R3DComputeMatches::Background {
    MatchFileWriter writer;
    MapJob maps[4];            // putative, F, E, H (declared after `writer`: gone before the graphs they read are freed)
    void emit(int slot, r3dm_graph* g, PairWiseMatches* map, const std::string& txt_path)
    {
        writer.own(g);
        maps[slot].start(g, map, writer.nice_value);
        writer.save(g, txt_path, with_ext(txt_path, ".bin"));
    }
    void join_maps() { for (MapJob& m : maps) m.join(); }
};

R3DComputeMatches::R3DComputeMatches(int device_id) : R3DComputeMatches(std::vector<int>(1, device_id)) {}

// one entry: a plain context; more: the multi-device deal
R3DComputeMatches::R3DComputeMatches(const std::vector<int>& device_ids) : devices_(device_ids)
{
    if (device_ids.size() == 1) {
        const int rc = r3dm_create(device_ids[0], &ctx_);
        if (rc != R3DM_OK) { ctx_ = nullptr; errorMessage_ = "r3dm_create failed (" + std::to_string(rc) + "): no gfx950 GPU"; }
    } else {
        const int rc = r3dm_multi_create(device_ids.data(), (int)device_ids.size(), &multi_);
        if (rc != R3DM_OK) { multi_ = nullptr; errorMessage_ = "r3dm_multi_create failed (" + std::to_string(rc) + ")"; }
    }
    setExactFastPaths(true);
}

R3DComputeMatches::~R3DComputeMatches()
{
    if (feat_multi_) r3dm_multi_destroy(feat_multi_);
    if (ctx_) r3dm_destroy(ctx_);
    if (multi_) r3dm_multi_destroy(multi_);
}

// r3dm_features_sink of the features stage: the view is registered with the matcher from the worker thread that computed it
// (descriptors device to device, positions as written to the .feat file).  A registration that fails is not an error: the view
// is then read back from its files like any other.
int R3DComputeMatches::features_sink(void* self_, uint32_t image_index, uint32_t n_features, const float* desc_device, const float* xy_as_written)
{
    R3DComputeMatches* self = static_cast<R3DComputeMatches*>(self_);
    try {                                                  // nothing leaves a C callback by exception (the caller is a worker thread of the library)
        const size_t vi = self->sink_need_[image_index];
        const View& v = self->views_[vi];
        std::lock_guard<std::mutex> lk(self->sink_mu_);
        const int rc = Devices{self->ctx_, self->multi_}.set_image(v.id_view, v.ui_width, v.ui_height, desc_device, n_features, self->dim_, self->dtype_, xy_as_written);
        if (rc == R3DM_OK) { self->registered_[vi] = 1; self->registered_n_[vi] = n_features; }
    } catch (...) {}
    return 0;
}

// R3DFeaturesThread::extractFeaturesAndDescriptors(vec_fileNames, sOutDir, params) (/root/reference/src/R3DComputeMatches.cpp:1994-1995,
// src/threads/R3DFeaturesThread.cpp:38-210) for the views whose two files are not both there.  The reference's worker threads
// admit one image at a time into the detector; here feat_conc_ batches of feat_batch_ same-size images are in flight per device.
bool R3DComputeMatches::runFeaturesStage(const R3DFParams& params, const std::string& dir)
{
    std::vector<size_t> need;
    for (size_t vi = 0; vi < views_.size(); ++vi)
        if (!(file_exists(dir + "/" + views_[vi].basename + ".feat") && file_exists(dir + "/" + views_[vi].basename + ".desc"))) need.push_back(vi);
    if (need.empty()) return true;
    // the detector list of the GUI: one served arm, "Fast-AKAZE" or "AKAZE" (include/regard3d_features.hpp says so too); a list of
    // more than one entry is refused by name
    const std::vector<std::string>& dl = params.keypointDetectorList_;
    for (const std::string& d : dl)
        if (d != "Fast-AKAZE" && d != "AKAZE") { errorMessage_ = "keypoint detector \"" + d + "\" is not served by the GPU path (Fast-AKAZE and AKAZE are)"; return false; }
    if (dl.size() != 1) {
        std::string names;
        for (const std::string& d : dl) names += (names.empty() ? "\"" : ", \"") + d + "\"";
        errorMessage_ = "keypoint detector list {" + names + "} is not served by the GPU path (one entry, Fast-AKAZE or AKAZE, is)";
        return false;
    }
    // the regions type names the descriptor arm: LIOP (float x 144) or the MLDB-486 rows of the Fast-A-KAZE detector (61 bytes)
    // or its M-SURF-64 rows (float x 64)
    const DescriptorArm* arm = descriptor_arm_by_type(dtype_, dim_);
    if (!arm) { errorMessage_ = "the features stage writes LIOP regions (float x 144); setRegionsType disagrees"; return false; }
    if (!feat_multi_) {
        std::vector<int> ids;
        for (int d : devices_) for (int k = 0; k < std::max(1, feat_conc_); ++k) ids.push_back(d);
        const int rc = r3dm_multi_create(ids.data(), (int)ids.size(), &feat_multi_);
        if (rc != R3DM_OK) { feat_multi_ = nullptr; errorMessage_ = "r3dm_multi_create (features stage) failed (" + std::to_string(rc) + ")"; return false; }
    }
    const int n_ctx = r3dm_multi_num_devices(feat_multi_);
    (void)r3dm_multi_set_keypoint_detector(feat_multi_, dl[0] == "AKAZE" ? R3DM_DETECTOR_AKAZE : R3DM_DETECTOR_FAST_AKAZE);
    (void)r3dm_multi_set_descriptor_arm(feat_multi_, arm->id);      // (MLDB / M-SURF with "AKAZE": refused by name by the features call below)
    // the sink carries no scales: while preemptive matching or the match budget is on, every view is registered from its files
    // (setPreemptiveMatching, setMatchBudget)
    const bool direct = direct_registration_ && !preemptive_on_ && !budget_on_;
    (void)r3dm_multi_set_features_sink(feat_multi_, direct ? &R3DComputeMatches::features_sink : nullptr, this);
    // the .feat / .desc of a batch are written behind the sink calls, beside the match phase (computeMatches waits for them before it
    // returns): only when the views are registered straight from the device, else Regions_Provider::load reads those files next
    (void)r3dm_multi_set_deferred_feature_files(feat_multi_, direct ? 1 : 0);
    (void)r3dm_multi_set_background_nice(feat_multi_, background_nice_);
    const r3dm_features_totals before = features_totals(feat_multi_);
    // with a provider, pixels are requested one chunk at a time (every context gets two batches per chunk), else all at once
    const size_t chunk = provider_ ? (size_t)n_ctx * (size_t)std::max(1, feat_batch_) * 2 : need.size();
    for (size_t c0 = 0; c0 < need.size(); c0 += chunk) {
        const size_t cn = std::min(chunk, need.size() - c0);
        std::vector<const float*> grays(cn, nullptr); std::vector<const unsigned char*> bgrs(cn, nullptr);
        std::vector<uint32_t> ws(cn), hs(cn), nf(cn, 0), sk(cn, 0);
        std::vector<std::string> fps(cn), dps(cn);
        std::vector<const char*> fp(cn), dp(cn);
        std::vector<char> provided(cn, 0);
        bool ok = true;
        for (size_t k = 0; k < cn && ok; ++k) {
            const View& v = views_[need[c0 + k]];
            grays[k] = v.gray; bgrs[k] = v.bgr8;
            if (!grays[k] && !bgrs[k] && provider_) {
                Pixels px;
                if (provider_(v, &px, provider_user_)) { grays[k] = px.gray; bgrs[k] = px.bgr8; provided[k] = 1; }
            }
            if (!grays[k] && !bgrs[k]) {
                // the reference would cv::imread the file here; decoding is the caller's, so a view without files AND pixels is an error
                errorMessage_ = "Invalid features: " + v.basename + " (no .feat/.desc in the matches directory and no pixels for the features stage)";
                ok = false;
            }
            ws[k] = v.ui_width; hs[k] = v.ui_height;
            fps[k] = dir + "/" + v.basename + ".feat"; dps[k] = dir + "/" + v.basename + ".desc";
            fp[k] = fps[k].c_str(); dp[k] = dps[k].c_str();
        }
        int rc = R3DM_OK;
        char err[512] = {0};
        sink_need_ = need.data() + c0;
        if (ok) rc = r3dm_multi_extract_features_ex(feat_multi_, (uint32_t)cn, grays.data(), bgrs.data(), ws.data(), hs.data(), params.threshold_,
                                                    fp.data(), dp.data(), nf.data(), sk.data(), (uint32_t)std::max(1, feat_batch_), err, sizeof(err));
        if (provider_release_) for (size_t k = 0; k < cn; ++k) if (provided[k]) provider_release_(views_[need[c0 + k]], provider_user_);
        if (!ok) return false;
        if (rc != R3DM_OK) { errorMessage_ = std::string("features stage failed: ") + err; return false; }
        phases_.images_extracted += cn;
        if (progress_) progress_(0.7f * (float)(c0 + cn) / (float)need.size(), "Extracting features", progress_user_);   // sendMsgToMainFrame, :212-240
    }
    phases_.features_totals = features_totals(feat_multi_);            // what this call added to them
    combine(phases_.features_totals, before, [](auto x, auto y) { return x - y; });
    return true;
}

void R3DComputeMatches::addViews(const std::vector<View>& views) { views_.insert(views_.end(), views.begin(), views.end()); }

void R3DComputeMatches::setIntegerFastPath(bool on) { Devices{ctx_, multi_}.set_integer_mfma(on); }
void R3DComputeMatches::setSplitFastPath(bool on) { Devices{ctx_, multi_}.set_split_mfma(on); }
void R3DComputeMatches::setHammingFastPath(bool on) { Devices{ctx_, multi_}.set_hamming_mfma(on); }
void R3DComputeMatches::setMutualMatching(bool on) { Devices{ctx_, multi_}.set_mutual(on); }
void R3DComputeMatches::setSymmetricRatio(bool on) { Devices{ctx_, multi_}.set_symmetric_ratio(on); }

// TracksBuilder::Build(map_Matches) + Filter(min_length) + ExportToSTL (and, with `kept`, the filter applied to the map itself): the
// map becomes a graph (r3dm_graph_from_csr: map order is graph order), r3dm_build_tracks runs on the first device
bool R3DComputeMatches::buildTracks(const PairWiseMatches& matches, uint32_t min_length, Tracks* out, PairWiseMatches* kept)
{
    r3dm_ctx* c = Devices{ctx_, multi_}.first_ctx();
    if (!c) { errorMessage_ = "buildTracks: no GPU context"; return false; }
    if (!out) { errorMessage_ = "buildTracks: no output"; return false; }
    std::vector<uint32_t> pairs;
    std::vector<uint64_t> offsets{0};
    std::vector<r3dm_match> flat;
    for (const auto& e : matches) {
        pairs.push_back(e.first.first); pairs.push_back(e.first.second);
        flat.insert(flat.end(), e.second.begin(), e.second.end());
        offsets.push_back(flat.size());
    }
    r3dm_graph* g = nullptr;
    r3dm_tracks* t = nullptr;
    r3dm_graph* kg = nullptr;
    int rc = r3dm_graph_from_csr(pairs.data(), pairs.size() / 2, offsets.data(), flat.data(), &g);
    if (rc != R3DM_OK) { errorMessage_ = "buildTracks: r3dm_graph_from_csr failed (" + std::to_string(rc) + ")"; return false; }
    rc = r3dm_build_tracks(c, g, min_length, &t, kept ? &kg : nullptr);
    r3dm_graph_free(g);
    if (rc != R3DM_OK) { errorMessage_ = std::string("buildTracks: ") + r3dm_last_error(c); return false; }
    const uint64_t n = r3dm_tracks_count(t);
    out->offsets.assign(r3dm_tracks_offsets(t), r3dm_tracks_offsets(t) + n + 1);
    out->observations.assign(r3dm_tracks_observations(t), r3dm_tracks_observations(t) + out->offsets.back());
    (void)r3dm_tracks_report(t, &out->stats);
    r3dm_tracks_free(t);
    if (kept) { graph_to_map(kg, *kept); r3dm_graph_free(kg); }
    return true;
}

void R3DComputeMatches::setPreemptiveMatching(bool on, uint32_t head_rows, uint32_t min_matches)
{
    const int rc = Devices{ctx_, multi_}.set_preemptive(on, head_rows, min_matches);
    preemptive_on_ = on && rc == R3DM_OK;
}

void R3DComputeMatches::setMatchBudget(bool on, uint32_t max_rows)
{
    const int rc = Devices{ctx_, multi_}.set_budget(on, max_rows);
    budget_on_ = on && rc == R3DM_OK;
}

void R3DComputeMatches::setPairProposal(bool on, uint32_t n_words, uint32_t top_k)
{
    proposal_on_ = on && n_words >= 2 && n_words <= R3DM_VOCAB_MAX_WORDS && top_k >= 1;
    proposal_words_ = n_words; proposal_top_k_ = top_k;
}

void R3DComputeMatches::setPairProposalTraining(uint32_t max_iterations, bool idf)
{
    proposal_train_iterations_ = max_iterations; proposal_idf_ = idf;
}

void R3DComputeMatches::setGuidedMatching(bool on, double ratio_F, double ratio_E, double ratio_H) { Devices{ctx_, multi_}.set_guided(on, ratio_F, ratio_E, ratio_H); }

void R3DComputeMatches::setRegionsType(r3dm_dtype dtype, uint32_t dim) { dtype_ = dtype; dim_ = dim; }

// ---- Regions_Provider::load + Features_Provider::load (src/R3DComputeMatches.cpp:2040,2094-2095): the views the features stage
// computed in this call are registered already (features_sink); the files of the others are read here, by all host threads, 64 views
// at a time; registration (device copies) stays in view order
bool R3DComputeMatches::loadViews(const std::string& dir)
{
    const Devices dev{ctx_, multi_};
    const size_t row_bytes = dtype_ == R3DM_F32 ? (size_t)dim_ * 4 : (size_t)dim_;
    std::vector<Loaded> chunk;
    std::vector<char> batch_done;
    for (size_t vi = 0; vi < views_.size(); ++vi) {
        if (vi % 64 == 0) {
            const size_t cn = std::min<size_t>(64, views_.size() - vi);
            chunk.assign(cn, Loaded());
#pragma omp parallel for schedule(dynamic) num_threads(r3dm_host_threads(64))
            for (long k = 0; k < (long)cn; ++k) {
                const View& u = views_[vi + (size_t)k];
                Loaded& L = chunk[(size_t)k];
                if (registered_[vi + (size_t)k]) { L.ok = true; continue; }
                // nothing may leave an OpenMP region by exception (std::terminate): a failed allocation is a failed load
                try { L.ok = load_feat(dir + "/" + u.basename + ".feat", L.xy, (preemptive_on_ || budget_on_) ? &L.scale : nullptr) && load_desc(dir + "/" + u.basename + ".desc", row_bytes, L.desc, L.n); }
                catch (...) { L.ok = false; }
            }
            // one device: the chunk's views go to the matcher in ONE call -- up to the first view the per-view pass below will refuse, so
            // that its error is the one reported
            batch_done.assign(cn, 0);
            if (dev.single()) {
                std::vector<r3dm_view_desc> vd;
                std::vector<size_t> which;
                for (size_t k = 0; k < cn; ++k) {
                    const Loaded& L = chunk[k];
                    if (!L.ok) break;
                    if (registered_[vi + k]) continue;
                    if (L.xy.size() != 2 * L.n) break;
                    const View& u = views_[vi + k];
                    vd.push_back(r3dm_view_desc{u.id_view, u.ui_width, u.ui_height, (uint32_t)L.n, dim_, (int32_t)dtype_, L.desc.data(), L.xy.data()});
                    which.push_back(k);
                }
                if (!vd.empty()) {
                    if (dev.set_images(vd) != R3DM_OK) { errorMessage_ = dev.last_error(); return false; }
                    for (size_t k : which) batch_done[k] = 1;
                }
            }
        }
        const View& v = views_[vi];
        const Loaded& L = chunk[vi % 64];
        if (!L.ok) {
            errorMessage_ = "Invalid features: " + v.basename;       // reference: MLOG "Invalid features." + return false (:2096-2097)
            return false;
        }
        if (registered_[vi]) statistics_.numberOfKeypoints_.push_back((int)registered_n_[vi]);
        else {
            if (L.xy.size() != 2 * L.n) { errorMessage_ = "feature/descriptor count mismatch: " + v.basename; return false; }
            statistics_.numberOfKeypoints_.push_back((int)L.n);
            if (!batch_done[vi % 64] && dev.set_image(v.id_view, v.ui_width, v.ui_height, L.desc.data(), (uint32_t)L.n, dim_, dtype_, L.xy.data()) != R3DM_OK) {
                errorMessage_ = dev.last_error();
                return false;
            }
            // the scale column is the view's priority (r3dm_set_view_priority) while preemptive matching or the match budget is on
            if ((preemptive_on_ || budget_on_) && L.n && dev.set_priority(v.id_view, L.scale) != R3DM_OK) { errorMessage_ = "feature scales of " + v.basename + ": " + dev.last_error(); return false; }
        }
        if (v.focal_px > 0.0) {
            const double K[9] = {v.focal_px, 0.0, v.ppx, 0.0, v.focal_px, v.ppy, 0.0, 0.0, 1.0};      // Pinhole_Intrinsic::K()
            if (dev.set_intrinsics(v.id_view, K) != R3DM_OK) { errorMessage_ = dev.last_error(); return false; }
        }
    }
    return true;
}

// ---- exhaustivePairs(#views) (:2042): all (I, J) with I < J, in view-id order -- or, under setPairProposal, the pairs
// r3dm_propose_pairs proposes instead (no reference counterpart).  The views are replicated on every device of a list, so the first
// context holds them all; the matchers deal whatever list they get
bool R3DComputeMatches::listPairs(std::vector<uint32_t>& pairs)
{
    std::vector<uint32_t> ids;
    for (const View& v : views_) ids.push_back(v.id_view);
    std::sort(ids.begin(), ids.end());
    pairs.clear();
    for (size_t a = 0; a < ids.size(); ++a)
        for (size_t b = a + 1; b < ids.size(); ++b) { pairs.push_back(ids[a]); pairs.push_back(ids[b]); }
    if (proposal_on_ && ids.size() >= 2) {
        uint64_t T = 0;
        for (int n : statistics_.numberOfKeypoints_) T += (uint64_t)n;
        const uint32_t n_words = (uint32_t)std::min<uint64_t>(proposal_words_, T / 2);
        if (n_words >= 2) {
            r3dm_ctx* pc = Devices{ctx_, multi_}.first_ctx();
            r3dm_vocab* vocab = nullptr;
            int rcp = r3dm_vocab_sample(pc, ids.data(), (uint32_t)ids.size(), n_words, &vocab);
            if (rcp == R3DM_OK && proposal_train_iterations_) {
                // trained on the views it was sampled from; the sample is the start and is given back
                r3dm_vocab* trained = nullptr;
                rcp = r3dm_vocab_train(pc, vocab, ids.data(), (uint32_t)ids.size(), proposal_train_iterations_, &trained);
                if (rcp == R3DM_OK) { r3dm_vocab_free(vocab); vocab = trained; }
            }
            if (rcp == R3DM_OK && proposal_idf_) rcp = r3dm_vocab_set_weighting(vocab, R3DM_VOCAB_WEIGHT_IDF);
            std::vector<uint32_t> proposed(2 * ids.size() * (size_t)proposal_top_k_);
            uint64_t n_proposed = 0;
            if (rcp == R3DM_OK) rcp = r3dm_propose_pairs(pc, vocab, ids.data(), (uint32_t)ids.size(), proposal_top_k_, proposed.data(), proposed.size() / 2, &n_proposed, nullptr);
            r3dm_vocab_free(vocab);
            if (rcp != R3DM_OK) { errorMessage_ = std::string("pair proposal: ") + r3dm_last_error(pc); return false; }
            proposed.resize(2 * (size_t)n_proposed);
            pairs.swap(proposed);
        }
    }
    last_pair_count_ = pairs.size() / 2;
    return true;
}

// ---- photometric matching (:2048).  Dispatch of src/R3DComputeMatches.cpp:2035-2062: 4 = brute force and 9 = the new arm run the
// exhaustive matcher; every approximate arm (0 FLANN kd-trees, 1..3 KGraph, 5 MRPT, 6..8 HNSW) runs the graph matcher with a preset of
// at least the arm's recall (r3dm_ann_params_for_algorithm); anything else was refused by computeMatches before its features stage
bool R3DComputeMatches::matchPutative(float dist_ratio, int matchingAlgorithm, const std::vector<uint32_t>& pairs, r3dm_graph** putative)
{
    const Devices dev{ctx_, multi_};
    r3dm_kgraph_params kp;
    bool use_kgraph = r3dm_ann_params_for_algorithm(matchingAlgorithm, &kp) == R3DM_OK;
    // binary regions: the graph matcher serves them behind its switch (r3dm_set_kgraph_hamming), which this stage turns on for its own
    // contexts -- HNSW and MRPT do not serve them, their arm numbers run the graph matcher with the preset r3dm_ann_params_for_algorithm names
    if (dtype_ == R3DM_BIN && use_kgraph && dev.set_kgraph_hamming(true) != R3DM_OK) { errorMessage_ = dev.last_error(); return false; }
    // an approximate arm whose job the exhaustive matcher does at least as fast -- and exactly -- is served by it (setApproximateArmsPolicy)
    if (use_kgraph && arms_policy_ == kArmsFastest && r3dm_exhaustive_is_faster(dev.first_ctx()) == 1) use_kgraph = false;
    last_exhaustive_ = !use_kgraph;
    // arms 6 / 7 / 8 taken literally (kArmsAsRequested) run hnsw_match itself: hnswlib's search on a batch-built HNSW index
    // (r3dm_match_pairs_hnsw), for the descriptor lengths hnswlib's SIMD16 distance serves; other lengths keep the graph matcher
    last_hnsw_ = use_kgraph && arms_policy_ == kArmsAsRequested && matchingAlgorithm >= 6 && matchingAlgorithm <= 8 &&
                 dtype_ != R3DM_BIN && (dim_ == 64 || dim_ == 128 || dim_ == 144 || dim_ == 256);
    // arm 5 taken literally runs mrpt_match itself: random projection trees on the device (r3dm_match_pairs_mrpt), the reference's
    // parameters (src/R3DComputeMatches.cpp:453-456); the index takes float rows of any length that is a multiple of 4
    last_mrpt_ = use_kgraph && arms_policy_ == kArmsAsRequested && matchingAlgorithm == 5 && dtype_ != R3DM_BIN && (dim_ & 3u) == 0 && dim_ <= 512;
    int rc;
    if (last_mrpt_) {
        r3dm_mrpt_params mp;
        (void)r3dm_mrpt_preset(&mp);
        rc = dev.match_mrpt(pairs, dist_ratio, &mp, putative);
    } else if (last_hnsw_) {
        r3dm_hnsw_params hp;
        (void)r3dm_hnsw_preset(matchingAlgorithm - 6, &hp);
        rc = dev.match_hnsw(pairs, dist_ratio, &hp, putative);
    } else if (use_kgraph) {
        rc = dev.match_kgraph(pairs, dist_ratio, &kp, putative);
    } else {
        rc = dev.match(pairs, dist_ratio, dtype_ == R3DM_BIN ? 0 : 1, putative);      // RegionsMatcherT squared flag: true for L2 metrics
    }
    if (rc != R3DM_OK) { errorMessage_ = dev.last_error(); return false; }
    return true;
}

// ---- Save(matches.putative.txt) (:2064) and statistics_.putativeMatches_, both started here and finished behind the filters; the
// adjacency SVG (:2074) needs the map at once.  File failures are reported at the end (finishFiles)
void R3DComputeMatches::startPutativeFiles(r3dm_graph* putative, const R3DProjectPaths& paths, bool svgOutput, Background& bg)
{
    const std::string& named = paths.matchesPutitativeFilename_;
    bg.emit(0, putative, &statistics_.putativeMatches_, named.empty() ? paths.relativeMatchesPath_ + "/matches.putative.txt" : named);
    if (svgOutput) { bg.maps[0].join(); write_adjacency_svg(paths.relativeMatchesPath_ + "/PutativeAdjacencyMatrix.svg", views_.size(), statistics_.putativeMatches_); }
}

// ---- geometric filtering (:2113-2233), the filters of kFilters that `params` asks for.  They only read the putative graph: one
// device runs two or three of them side by side (r3dm_filter_FEH), anything else one call per filter -- a device list deals each
// filter's pairs to its devices.  Either way a graph's files and map are written behind the next filter (Background::emit)
bool R3DComputeMatches::runFilters(const R3DFParams& params, const R3DProjectPaths& paths, const r3dm_graph* putative, Background& bg)
{
    const Devices dev{ctx_, multi_};
    int which = 0, announced = -1;
    for (int k = 0; k < 3; ++k) if (params.*kFilters[k].asked) which |= 1 << k;
    auto announce = [&](int k) {                            // once per filter that runs, before it runs
        if (k > announced && progress_) progress_(kFilters[k].fraction, kFilters[k].message, progress_user_);
        announced = std::max(announced, k);
    };
    const double t_filters = wall_ms();
    r3dm_graph* graphs[3] = {nullptr, nullptr, nullptr};
    const bool side_by_side = dev.single() && (which & (which - 1)) != 0;
    if (side_by_side) {
        announce(__builtin_ctz((unsigned)which));           // the first one asked for; the others before their tails
        double msk[3] = {0, 0, 0}, msw[3] = {0, 0, 0};
        if (dev.filter_FEH(putative, seed_, which, graphs, msk, msw) != R3DM_OK) { errorMessage_ = dev.last_error(); return false; }
        for (int k = 0; k < 3; ++k) { phases_.*kFilters[k].wall = msw[k]; phases_.*kFilters[k].kernels = msk[k]; }
        phases_.filters_wall = wall_ms() - t_filters;
    }
    for (int k = 0; k < 3; ++k) {
        const FilterEntry& f = kFilters[k];
        if (!(params.*f.asked)) continue;
        announce(k);
        if (!side_by_side) {
            const double t0 = wall_ms();
            if ((dev.*f.call)(putative, seed_, &graphs[k]) != R3DM_OK) { errorMessage_ = dev.last_error(); return false; }
            phases_.*f.wall = wall_ms() - t0; phases_.*f.kernels = dev.kernel_ms(true);
        }
        const double t0 = wall_ms();
        const std::string& named = paths.*f.named;
        bg.emit(1 + k, graphs[k], &(statistics_.*f.map), named.empty() ? paths.relativeMatchesPath_ + f.default_name : named);
        phases_.files += wall_ms() - t0;
    }
    if (!side_by_side) phases_.filters_wall = wall_ms() - t_filters;
    return true;
}

// ---- the match files and the deferred feature files are complete, or the call fails: the reference returns EXIT_FAILURE (== true)
// from a bool function there (:2069), a real failure is reported instead
bool R3DComputeMatches::finishFiles(Background& bg)
{
    const std::string bad = bg.writer.finish();
    char ferr[512] = {0};
    const int frc = feat_multi_ ? r3dm_multi_features_files_wait(feat_multi_, ferr, sizeof(ferr)) : R3DM_OK;
    if (!bad.empty()) { errorMessage_ = "Cannot save computed matches in: " + bad; return false; }
    if (frc != R3DM_OK) { errorMessage_ = std::string("features stage failed: ") + ferr; return false; }
    return true;
}

bool R3DComputeMatches::computeMatches(R3DFParams& params, bool svgOutput, const R3DProjectPaths& paths,
                                       int /*cameraModel*/, int matchingAlgorithm)
{
    statistics_ = R3DComputeMatchesStatistics();
    phases_ = PhaseTimes();
    { const DescriptorArm* arm = descriptor_arm_by_type(dtype_, dim_); phases_.descriptor_arm = arm ? arm->id : R3DM_DESCRIPTOR_LIOP; }   // (no arm's type: the features stage refuses it)
    const Devices dev{ctx_, multi_};
    if (!dev) return false;
    const double t_begin = wall_ms();
    FeatureFilesGuard feature_files_guard{feat_multi_};
    r3dm_kgraph_params kp;
    if (matchingAlgorithm != kMatchingAlgorithmGPU && matchingAlgorithm != 4 && r3dm_ann_params_for_algorithm(matchingAlgorithm, &kp) != R3DM_OK) {
        errorMessage_ = "matchingAlgorithm " + std::to_string(matchingAlgorithm) + " is not served by the GPU path (0..9 are)";
        return false;
    }
    const std::string dir = paths.relativeMatchesPath_;

    // 1. R3DFeaturesThread::extractFeaturesAndDescriptors(vec_fileNames, sOutDir, params) (:1994-1995)
    if (dev.clear_images() != R3DM_OK) { errorMessage_ = dev.last_error(); return false; }
    registered_.assign(views_.size(), 0); registered_n_.assign(views_.size(), 0);
    double t0 = wall_ms();
    if (!runFeaturesStage(params, dir)) return false;
    phases_.features = wall_ms() - t0;

    // 2. + 3. the views and the pair list
    t0 = wall_ms();
    std::vector<uint32_t> pairs;
    if (!loadViews(dir) || !listPairs(pairs)) return false;
    phases_.load = wall_ms() - t0;

    // 4. the putative match
    if (progress_) progress_(0.7f, "Find putative matches", progress_user_);
    t0 = wall_ms();
    r3dm_graph* putative = nullptr;
    if (!matchPutative(params.distRatio_, matchingAlgorithm, pairs, &putative)) return false;
    phases_.match = wall_ms() - t0; phases_.match_kernels = dev.kernel_ms(false);
    r3dm_stats st{};
    if (dev.single_stats(st)) {
        phases_.match_post = st.ms_wall_match_post;
#ifdef R3DM_DEVTOOLS
        fprintf(stderr, "facade match phase %.2f ms, r3dm_match_pairs inside %.2f ms\n", phases_.match, st.ms_wall_match);
#endif
    }

    // 5. the putative files and map, behind the filters from here on
    t0 = wall_ms();
    Background bg;
    bg.writer.nice_value = background_nice_;
    startPutativeFiles(putative, paths, svgOutput, bg);
    phases_.files += wall_ms() - t0;

    // 6. the filters; the maps are complete behind them whether they succeeded or not
    const bool filtered = runFilters(params, paths, putative, bg);
    t0 = wall_ms();
    bg.join_maps();
    phases_.files += wall_ms() - t0;
    if (!filtered) return false;

    // 7. GeometricAdjacencyMatrix.svg (:2238): the reference draws whichever filter ran last (H, else E, else F); then the files
    if (svgOutput) {
        const PairWiseMatches& last = params.computeHomographyMatrix_ ? statistics_.homographyMatches_
                                    : (params.computeEssentialMatrix_ ? statistics_.essentialMatches_ : statistics_.fundamentalMatches_);
        write_adjacency_svg(dir + "/GeometricAdjacencyMatrix.svg", views_.size(), last);
    }
    t0 = wall_ms();
    const bool written = finishFiles(bg);
    phases_.files += wall_ms() - t0;
    if (!written) return false;
    phases_.total = wall_ms() - t_begin;
    return true;
}

}  // namespace r3d_amd

struct r3dm_stage { r3d_amd::R3DComputeMatches* stage = nullptr; };

extern "C" int r3dm_stage_create(const int* device_ids, int n_devices, r3dm_stage** out)
{
    if (!out || !device_ids || n_devices < 1) return R3DM_ERR_INVALID;
    *out = nullptr;
    try {
        auto* s = new r3dm_stage();
        s->stage = new r3d_amd::R3DComputeMatches(std::vector<int>(device_ids, device_ids + n_devices));
        if (!s->stage->errorMessage().empty()) { delete s->stage; delete s; return R3DM_ERR_NO_DEVICE; }
        *out = s;
        return R3DM_OK;
    } catch (const std::bad_alloc&) { return R3DM_ERR_NOMEM; }
    catch (...) { return R3DM_ERR_INVALID; }
}

extern "C" void r3dm_stage_destroy(r3dm_stage* s)
{
    if (!s) return;
    delete s->stage;
    delete s;
}

// flags no call can honour together: the two descriptor arms.  Refused by name, before a stage is created or run
static bool stage_flags_ok(uint32_t flags, char* err, size_t err_cap)
{
    if (!(flags & R3DM_STAGE_DESCRIPTOR_MLDB) || !(flags & R3DM_STAGE_DESCRIPTOR_MSURF)) return true;
    if (err && err_cap) snprintf(err, err_cap, "R3DM_STAGE_DESCRIPTOR_MLDB and R3DM_STAGE_DESCRIPTOR_MSURF name two descriptor arms: one call runs one");
    return false;
}

// the flags that are switches of the facade, each set to what `flags` says; a flag outside `mask` leaves its switch as it is
// (the descriptor arm and the detector are parameters of the run, not switches: r3dm_stage_run)
static void apply_stage_flags(r3d_amd::R3DComputeMatches& stage, uint32_t flags, uint32_t mask)
{
    using r3d_amd::R3DComputeMatches;
    const auto has = [&](uint32_t f) { return (flags & f) != 0; };
    if (mask & R3DM_STAGE_ARMS_AS_REQUESTED) stage.setApproximateArmsPolicy(has(R3DM_STAGE_ARMS_AS_REQUESTED) ? R3DComputeMatches::kArmsAsRequested : R3DComputeMatches::kArmsFastest);
    if (mask & R3DM_STAGE_BACKGROUND_NICE) stage.setBackgroundThreadsNice(has(R3DM_STAGE_BACKGROUND_NICE) ? 10 : 0);
    if (mask & R3DM_STAGE_F32_TILES) stage.setExactFastPaths(!has(R3DM_STAGE_F32_TILES));      // (R3DM_STAGE_SPLIT_MFMA / _INTEGER_MFMA: implied since round 3)
    if (mask & R3DM_STAGE_GUIDED_MATCHING) stage.setGuidedMatching(has(R3DM_STAGE_GUIDED_MATCHING));
    if (mask & R3DM_STAGE_MUTUAL_MATCHING) stage.setMutualMatching(has(R3DM_STAGE_MUTUAL_MATCHING));
    if (mask & R3DM_STAGE_SYMMETRIC_RATIO) stage.setSymmetricRatio(has(R3DM_STAGE_SYMMETRIC_RATIO));
    if (mask & R3DM_STAGE_PREEMPTIVE_MATCHING) stage.setPreemptiveMatching(has(R3DM_STAGE_PREEMPTIVE_MATCHING));
    if (mask & R3DM_STAGE_MATCH_BUDGET) stage.setMatchBudget(has(R3DM_STAGE_MATCH_BUDGET));
    if (mask & R3DM_STAGE_PAIR_PROPOSAL) stage.setPairProposal(has(R3DM_STAGE_PAIR_PROPOSAL));
    if (mask & R3DM_STAGE_PROPOSAL_TRAINED) stage.setPairProposalTraining(has(R3DM_STAGE_PROPOSAL_TRAINED) ? 10 : 0, has(R3DM_STAGE_PROPOSAL_TRAINED));
}

extern "C" int r3dm_stage_run(r3dm_stage* sp, const char* matches_dir, const r3dm_view_image* views, uint32_t n_views,
                              float threshold, float dist_ratio, int matching_algorithm, int compute_F, int compute_E, int compute_H,
                              uint64_t seed, int features_batches_in_flight, int features_images_per_batch, uint32_t flags,
                              r3dm_stage_report* report, char* err, size_t err_cap)
{
    if (!sp || !sp->stage || !matches_dir || (n_views && !views)) return R3DM_ERR_INVALID;
    if (err && err_cap) err[0] = 0;
    if (!stage_flags_ok(flags, err, err_cap)) return R3DM_ERR_INVALID;
    try {
        r3d_amd::R3DComputeMatches& stage = *sp->stage;
        stage.clearViews();
        std::vector<r3d_amd::View> vs(n_views);
        for (uint32_t k = 0; k < n_views; ++k) {
            r3d_amd::View& v = vs[k];
            v.id_view = views[k].id; v.ui_width = views[k].width; v.ui_height = views[k].height; v.basename = views[k].basename ? views[k].basename : "";
            v.focal_px = views[k].focal_px; v.ppx = views[k].ppx; v.ppy = views[k].ppy;
            v.bgr8 = views[k].bgr8; v.gray = views[k].gray;
        }
        stage.addViews(vs);
        stage.setSeed(seed);
        if (features_batches_in_flight > 0 && features_images_per_batch > 0) stage.setFeaturesConcurrency(features_batches_in_flight, features_images_per_batch);
        apply_stage_flags(stage, flags, ~0u);
        const DescriptorArm& arm = *descriptor_arm_by_id((flags & R3DM_STAGE_DESCRIPTOR_MLDB) ? R3DM_DESCRIPTOR_MLDB : (flags & R3DM_STAGE_DESCRIPTOR_MSURF) ? R3DM_DESCRIPTOR_MSURF : R3DM_DESCRIPTOR_LIOP);
        stage.setRegionsType(arm.dtype, arm.dim);
        r3d_amd::R3DFParams params;
        params.keypointDetectorList_ = {(flags & R3DM_STAGE_DETECTOR_AKAZE) ? "AKAZE" : "Fast-AKAZE"};
        params.threshold_ = threshold;
        params.distRatio_ = dist_ratio;
        params.computeFundalmentalMatrix_ = compute_F != 0;
        params.computeEssentialMatrix_ = compute_E != 0;
        params.computeHomographyMatrix_ = compute_H != 0;
        r3d_amd::R3DProjectPaths paths;
        paths.relativeMatchesPath_ = matches_dir;
        const bool ok = stage.computeMatches(params, false, paths, 1, matching_algorithm);
        if (err && err_cap) { strncpy(err, stage.errorMessage().c_str(), err_cap - 1); err[err_cap - 1] = 0; }
        if (report) {
            const auto& P = stage.getPhaseTimes();
            const auto& S = stage.getStatistics();
            *report = r3dm_stage_report{};
            report->ms_features = P.features; report->ms_load = P.load; report->ms_match = P.match; report->ms_filter_F = P.filter_F;
            report->ms_filter_E = P.filter_E; report->ms_filter_H = P.filter_H; report->ms_files = P.files; report->ms_total = P.total;
            report->ms_filters_wall = P.filters_wall; report->ms_match_post = P.match_post;
            report->ms_match_kernels = P.match_kernels; report->ms_F_kernels = P.F_kernels; report->ms_E_kernels = P.E_kernels; report->ms_H_kernels = P.H_kernels;
            report->images_extracted = P.images_extracted; report->features = P.features_totals;
            report->match_was_exhaustive = stage.lastMatchWasExhaustive() ? 1 : 0;
            report->descriptor_arm = (uint64_t)P.descriptor_arm;
            for (int n : S.numberOfKeypoints_) report->n_keypoints += (uint64_t)n;
            auto count = [](const r3d_amd::PairWiseMatches& m, uint64_t& pairs, uint64_t& matches) { pairs = m.size(); matches = 0; for (const auto& kv : m) matches += kv.second.size(); };
            count(S.putativeMatches_, report->n_putative_pairs, report->n_putative_matches);
            count(S.fundamentalMatches_, report->n_F_pairs, report->n_F_matches);
            count(S.essentialMatches_, report->n_E_pairs, report->n_E_matches);
            count(S.homographyMatches_, report->n_H_pairs, report->n_H_matches);
        }
        return ok ? R3DM_OK : R3DM_ERR_IO;
    } catch (const std::bad_alloc&) { return R3DM_ERR_NOMEM; }          // nothing crosses the C boundary
    catch (...) { return R3DM_ERR_INVALID; }
}

extern "C" int r3dm_compute_matches_stage(const int* device_ids, int n_devices, const char* matches_dir, const r3dm_view_image* views, uint32_t n_views,
                                          float threshold, float dist_ratio, int matching_algorithm, int compute_F, int compute_E, int compute_H,
                                          uint64_t seed, int features_batches_in_flight, int features_images_per_batch, uint32_t flags,
                                          r3dm_stage_report* report, char* err, size_t err_cap)
{
    if (err && err_cap) err[0] = 0;
    if (!stage_flags_ok(flags, err, err_cap)) return R3DM_ERR_INVALID;
    r3dm_stage* s = nullptr;
    int rc = r3dm_stage_create(device_ids, n_devices, &s);
    if (rc != R3DM_OK) { if (err && err_cap) snprintf(err, err_cap, "r3dm_create failed (%d): no gfx950 GPU", rc); return rc; }
    rc = r3dm_stage_run(s, matches_dir, views, n_views, threshold, dist_ratio, matching_algorithm, compute_F, compute_E, compute_H, seed,
                        features_batches_in_flight, features_images_per_batch, flags, report, err, err_cap);
    r3dm_stage_destroy(s);
    return rc;
}

extern "C" int r3dm_compute_matches_dir(int device_id, const char* matches_dir, const r3dm_view* views, uint32_t n_views,
                                        r3dm_dtype dtype, uint32_t dim, float dist_ratio, int compute_F, uint64_t seed,
                                        uint64_t* n_putative_pairs, uint64_t* n_geometric_pairs, char* err, size_t err_cap)
{
    return r3dm_compute_matches_dir_flags(device_id, matches_dir, views, n_views, dtype, dim, dist_ratio, compute_F, seed, 0u,
                                          n_putative_pairs, n_geometric_pairs, err, err_cap);
}

extern "C" int r3dm_compute_matches_dir_flags(int device_id, const char* matches_dir, const r3dm_view* views, uint32_t n_views,
                                              r3dm_dtype dtype, uint32_t dim, float dist_ratio, int compute_F, uint64_t seed, uint32_t flags,
                                              uint64_t* n_putative_pairs, uint64_t* n_geometric_pairs, char* err, size_t err_cap)
{
    if (!matches_dir || (n_views && !views)) return R3DM_ERR_INVALID;
    try {
    r3d_amd::R3DComputeMatches stage(device_id);
    std::vector<r3d_amd::View> vs;
    for (uint32_t k = 0; k < n_views; ++k) vs.push_back({views[k].id, views[k].width, views[k].height, views[k].basename});
    stage.addViews(vs);
    stage.setRegionsType(dtype, dim);
    stage.setSeed(seed);
    apply_stage_flags(stage, flags, R3DM_STAGE_F32_TILES | R3DM_STAGE_MUTUAL_MATCHING | R3DM_STAGE_SYMMETRIC_RATIO | R3DM_STAGE_PREEMPTIVE_MATCHING | R3DM_STAGE_MATCH_BUDGET | R3DM_STAGE_PAIR_PROPOSAL | R3DM_STAGE_PROPOSAL_TRAINED);
    r3d_amd::R3DFParams params;
    params.distRatio_ = dist_ratio;
    params.computeFundalmentalMatrix_ = compute_F != 0;
    params.computeEssentialMatrix_ = false;
    params.computeHomographyMatrix_ = false;
    r3d_amd::R3DProjectPaths paths;
    paths.relativeMatchesPath_ = matches_dir;
    const bool ok = stage.computeMatches(params, false, paths, 1, r3d_amd::R3DComputeMatches::kMatchingAlgorithmGPU);
    if (n_putative_pairs) *n_putative_pairs = stage.getStatistics().putativeMatches_.size();
    if (n_geometric_pairs) *n_geometric_pairs = stage.getStatistics().fundamentalMatches_.size();
    if (err && err_cap) { strncpy(err, stage.errorMessage().c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    return ok ? R3DM_OK : R3DM_ERR_IO;
    } catch (const std::bad_alloc&) { return R3DM_ERR_NOMEM; }          // nothing crosses the C boundary
    catch (...) { return R3DM_ERR_INVALID; }
}
