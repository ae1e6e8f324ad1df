// api_features.cpp -- part of the host side of libr3dm.so (see r3dm_ctx.hpp for the file map): the features work item of
// src/threads/R3DFeaturesThread.cpp and src/Regard3DFeatures.cpp.  The .feat / .desc files; the features batch in its phases -- detect
// (api_akaze.cpp, whichever arm) -> keypoints and patch maps (host team) -> one descriptor pass chosen by the context's descriptor arm:
// LIOP (api_liop.cpp), MLDB-486 or M-SURF-64 (api_akaze.cpp) -> delivery (files + sink, at once or deferred to the context's writer thread) ->
// outputs and totals; the work list over a multi-context; the setters of all this.
// There is no CPU fallback in this file: when HIP fails, the call fails.
#include "fmt_g6.hpp"
#include "r3dm_ctx.hpp"

#include <charconv>
#include <tuple>

extern "C" {
int r3dm_multi_num_devices(const r3dm_multi* m);
r3dm_ctx* r3dm_multi_ctx(r3dm_multi* m, int k);
}

// ======== the .feat / .desc files
// "%g" of one float, locale-independent (the host application runs under setlocale(LC_ALL, "")): printf("%.6g") in the "C" locale,
// i.e. std::to_chars(general, 6) -- through the exact fast path of fmt_g6.hpp for the magnitudes a .feat file holds
static inline char* put_g(char* p, char* end, float v, float* as_parsed = nullptr) { return r3dm_fmt::put_g6(p, end, v, as_parsed); }

// KeypointSet::saveToBinFile (src/keypointSet.hpp:61-67): .feat = one "x y scale orientation" line per feature
// (SIOPointFeature::operator<<, default float formatting; scale = size / 2, :835-836), .desc = count + raw rows
// xy_as_written (optional, n x 2): the positions as a reader of the file parses them (std::from_chars on the text just written)
static size_t format_feat(std::vector<char>& txt, const float* kps, uint32_t n, float* xy_as_written)
{
    txt.resize((size_t)n * 64 + 64);
    char* p = txt.data(); char* const end = p + txt.size();
    for (uint32_t k = 0; k < n; ++k) {
        float* const back = xy_as_written ? xy_as_written + 2 * (size_t)k : nullptr;
        p = put_g(p, end, kps[4 * (size_t)k], back); *p++ = ' ';
        p = put_g(p, end, kps[4 * (size_t)k + 1], back ? back + 1 : nullptr); *p++ = ' ';
        p = put_g(p, end, kps[4 * (size_t)k + 2] / 2.0f); *p++ = ' ';
        p = put_g(p, end, kps[4 * (size_t)k + 3]); *p++ = '\n';
    }
    return (size_t)(p - txt.data());
}

// one image on its way to its files: the text of its .feat, its rows (in pin_desc, row_bytes each: 144 floats of LIOP, 61 bytes of
// MLDB or 64 floats of M-SURF), its two paths, the positions for the sink
struct FeatJob { std::string feat, desc; std::vector<char> txt; size_t len = 0; const unsigned char* rows = nullptr; size_t row_bytes = 0; uint32_t n = 0; std::vector<float> xy; };

static int write_feat_desc_files(std::string& err, const FeatJob& j)
{
    FILE* f = fopen(j.feat.c_str(), "wb");
    if (!f) { err = "cannot write " + j.feat; return R3DM_ERR_IO; }
    bool ok = j.len == 0 || fwrite(j.txt.data(), 1, j.len, f) == j.len;
    ok = (fclose(f) == 0) && ok;
    if (!ok) { err = "cannot write " + j.feat; return R3DM_ERR_IO; }
    f = fopen(j.desc.c_str(), "wb");
    if (!f) { err = "cannot write " + j.desc; return R3DM_ERR_IO; }
    const uint64_t cnt = j.n;
    ok = fwrite(&cnt, 8, 1, f) == 1 && (j.n == 0 || fwrite(j.rows, j.row_bytes, j.n, f) == j.n);
    ok = (fclose(f) == 0) && ok;
    if (!ok) { err = "cannot write " + j.desc; return R3DM_ERR_IO; }
    return R3DM_OK;
}

// the writer thread of a context with deferred feature files: joined before pin_desc is filled again and by the wait entry
static int features_files_join(r3dm_ctx* c)
{
    if (c->file_writer.joinable()) c->file_writer.join();
    const int rc = c->file_writer_rc;
    if (rc != R3DM_OK) c->err = c->file_writer_err.empty() ? "writing the feature files failed" : c->file_writer_err;
    c->file_writer_rc = R3DM_OK; c->file_writer_err.clear();
    return rc;
}

static bool both_files_exist(const char* feat_path, const char* desc_path, uint32_t* n_rows)
{
    FILE* ff = fopen(feat_path, "rb");
    FILE* fd = ff ? fopen(desc_path, "rb") : nullptr;
    if (ff) fclose(ff);
    if (!fd) return false;
    uint64_t cnt = 0;
    if (fread(&cnt, 8, 1, fd) != 1) cnt = 0;
    fclose(fd);
    if (n_rows) *n_rows = (uint32_t)cnt;
    return true;
}

// ======== the features batch
namespace {

// the keypoints of a batch on the host: image b's are the rows first[b] .. first[b + 1]
struct BatchKeypoints {
    std::vector<size_t> first;
    std::vector<float> kps, M6;               // x, y, size, angle in degrees; the 2 x 3 patch map
    std::vector<uint32_t> img_of;
    size_t total() const { return img_of.size(); }
};

// the descriptor rows of a batch where the descriptor pass left them on the device: image b's are at dev + row_bytes first[b]
struct BatchRows { const unsigned char* dev = nullptr; size_t row_bytes = 0; };

// what the context's two switches cannot do together (r3dm_set_descriptor_arm): refused before anything is computed
int descriptor_arm_check(r3dm_ctx* c)
{
    const DescriptorArm& arm = *descriptor_arm_by_id(c->descriptor_arm);
    if (!arm.level_planes || c->detector_arm != R3DM_DETECTOR_AKAZE) return R3DM_OK;
    c->err = std::string("descriptor arm ") + arm.macro + " is not served with the classic detector R3DM_DETECTOR_AKAZE (" + arm.name + " reads the Fast-A-KAZE level planes)";
    return R3DM_ERR_UNSUPPORTED;
}

// phase 2: angle (the Fast arm's: atan2f of the host libm, as the reference) and, with want_maps (the LIOP arm), LIOP patch map of every
// keypoint; a few host threads share the loop, in chunks of 4,096 keypoints over all images of the batch
void keypoints_and_maps(const DetectedBatch& det, uint32_t B, int host_team, bool want_maps, BatchKeypoints& K)
{
    K.first.assign(B + 1, 0);
    for (uint32_t b = 0; b < B; ++b) K.first[b + 1] = K.first[b] + det.count(b);
    const size_t n_total = K.first[B];
    K.kps.resize(4 * n_total); K.M6.resize(want_maps ? 6 * n_total : 0); K.img_of.resize(n_total);
    struct Chunk { uint32_t b; long k0, k1; };
    std::vector<Chunk> chunks;
    for (uint32_t b = 0; b < B; ++b) {
        const long nk = (long)det.count(b);
        for (long k0 = 0; k0 < nk; k0 += 4096) chunks.push_back({b, k0, std::min(nk, k0 + 4096)});
    }
    r3dm_parallel_for((long)chunks.size(), host_team, [&](long ci) {
        const Chunk& ch = chunks[(size_t)ci];
        for (long k = ch.k0; k < ch.k1; ++k) {
            const size_t g = K.first[ch.b] + (size_t)k;
            float* o = &K.kps[4 * g];
            det.keypoint(ch.b, (size_t)k, o);
            if (want_maps) liop_patch_map(o[0], o[1], o[2], o[3], 8.0f /* getKpSizeFactor("AKAZE" / "Fast-AKAZE"), :703-704 */, &K.M6[6 * g]);
            K.img_of[g] = ch.b;
        }
    });
}

// phase 3: one descriptor pass over the keypoints of ALL images -- LIOP on the gray planes, or MLDB / M-SURF-64 on the level planes, that
// the detector left on the device; the rows stay there for the sink (`rows`) and go to page-locked host memory for the files.  Immediately: waited
// for.  Deferred: they travel behind the kernel, only the writer thread waits (ev_desc)
int describe_batch(r3dm_ctx* c, const DetectedBatch& det, uint32_t width, uint32_t height, const BatchKeypoints& K, bool deferred, int host_team, BatchRows& rows)
{
    const DescriptorArm& arm = *descriptor_arm_by_id(c->descriptor_arm);
    rows.row_bytes = arm.row_bytes;
    const size_t out_bytes = K.total() * rows.row_bytes;
    { const int wrc_prev = features_files_join(c); if (wrc_prev != R3DM_OK) return wrc_prev; }      // the previous batch's writer still reads pin_desc
    R3DM_HIP(c, c->pin_desc.ensure(out_bytes));
    if (arm.level_planes) {
        std::vector<size_t> first;
        const int rc = ak_describe_pass(c, arm, det, 0xFFFFFFFFu, host_team, first, &rows.dev);
        if (rc != R3DM_OK) return rc;
    } else {
        const int rc = liop_pass(c, det.grays_dev, width, height, K.M6.data(), K.img_of.data(), (uint32_t)K.total(), false);
        if (rc != R3DM_OK) return rc;
        rows.dev = c->liop_out.as<unsigned char>();
    }
    R3DM_HIP(c, hipMemcpyAsync(c->pin_desc.p, rows.dev, out_bytes, hipMemcpyDeviceToHost, c->stream));
    if (deferred) {
        if (!c->ev_desc) R3DM_HIP(c, hipEventCreateWithFlags(&c->ev_desc, hipEventDisableTiming));
        R3DM_HIP(c, hipEventRecord(c->ev_desc, c->stream));
    } else {
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        liop_read_time(c);
    }
    return R3DM_OK;
}

// phase 4, per image, three steps, each written once: format the text, write the two files, offer the image to the sink.  The two modes
// differ in when the write runs and on which thread.
// the sink sees the image under the index its caller knows it by, its rows on the device (the batch's are still where the descriptor
// pass left them) and the positions as written; a refusal (a sink that throws included) is the image's error
void offer_to_sink(r3dm_ctx* c, uint32_t b, const FeatJob& j, const BatchRows& rows, size_t first_row, int& rc, std::string& err)
{
    const uint32_t id = c->feat_sink_ids ? c->feat_sink_ids[b] : b;
    int src = 1;
    try { src = c->feat_sink(c->feat_sink_user, id, j.n, j.n ? reinterpret_cast<const float*>(rows.dev + rows.row_bytes * first_row) : nullptr, j.xy.data()); } catch (...) {}
    if (src != 0) { rc = R3DM_ERR_INVALID; err = "the features sink refused image " + std::to_string(id); }
}

// the files of the B images are formatted and written by up to 8 host threads (28 k keypoints = 113 k decimal conversions and
// 16 MB per image).  wrc / werr: what went wrong per image.
// Immediately: each thread hands its image to the sink (if any) as soon as its files are written -- the sink of the facade registers the
// view with the matcher (position classes, device-to-device copy, re-layout kernels) while the other threads still format theirs (this
// context's stream is idle: the copy to pin_desc was waited for).
// Deferred (r3dm_set_deferred_feature_files): the text is formatted while the LIOP kernel runs (it needs the keypoints only); when the
// kernel is done the images go to the sink; the fwrites -- 16 MB of descriptors per 28 k keypoints, still on their way to pin_desc -- are
// left to the context's writer thread, which runs beside whatever the caller does next
int deliver_batch(r3dm_ctx* c, uint32_t B, const char* const* feat_paths, const char* const* desc_paths, const DetectedBatch& det,
                  const BatchKeypoints& K, const BatchRows& rows, bool deferred, int host_team, double t_liop, std::vector<int>& wrc,
                  std::vector<std::string>& werr)
{
    const size_t n_total = K.total();
    const unsigned char* desc_host = n_total ? c->pin_desc.as<unsigned char>() : nullptr;
    auto wanted = [&](long b) { return feat_paths[b] && desc_paths[b]; };
    auto format = [&](FeatJob& j, long b) {
        j.feat = feat_paths[b]; j.desc = desc_paths[b]; j.n = (uint32_t)det.count((uint32_t)b);
        j.rows = desc_host ? desc_host + rows.row_bytes * K.first[b] : nullptr; j.row_bytes = rows.row_bytes;
        if (c->feat_sink) j.xy.resize((size_t)j.n * 2 + 2);
        j.len = format_feat(j.txt, K.kps.data() + 4 * K.first[b], j.n, c->feat_sink ? j.xy.data() : nullptr);
    };
    if (!deferred) {
        r3dm_parallel_for((long)B, host_team, [&](long b) {
            if (!wanted(b)) return;
            try {                                                   // nothing may leave a helper thread by exception
                FeatJob j;
                format(j, b);
                wrc[b] = write_feat_desc_files(werr[b], j);
                if (wrc[b] == R3DM_OK && c->feat_sink) offer_to_sink(c, (uint32_t)b, j, rows, K.first[b], wrc[b], werr[b]);
            } catch (...) { wrc[b] = R3DM_ERR_NOMEM; }
        });
        (void)hipSetDevice(c->device);                         // a sink may have worked on another device from this thread
        return R3DM_OK;
    }
    auto jobs = std::make_shared<std::vector<FeatJob>>(B);
    r3dm_parallel_for((long)B, host_team, [&](long b) {
        if (!wanted(b)) return;
        try { format((*jobs)[(size_t)b], b); } catch (...) { wrc[b] = R3DM_ERR_NOMEM; }
    });
    if (n_total) {
        R3DM_HIP(c, hipEventSynchronize(c->ev1));            // the LIOP kernel (the copy to the host is still running)
        liop_read_time(c);
    }
    c->stats.ms_liop_wall = now_ms() - t_liop;
    if (c->feat_sink) {
        r3dm_parallel_for((long)B, host_team, [&](long b) {
            if (!wanted(b) || wrc[b] != R3DM_OK) return;
            try { offer_to_sink(c, (uint32_t)b, (*jobs)[(size_t)b], rows, K.first[b], wrc[b], werr[b]); } catch (...) { wrc[b] = R3DM_ERR_NOMEM; }
            std::vector<float>().swap((*jobs)[(size_t)b].xy);
        });
        (void)hipSetDevice(c->device);
    }
    { const int wrc_prev = features_files_join(c); if (wrc_prev != R3DM_OK) return wrc_prev; }      // (a batch without keypoints has not joined it in describe_batch)
    // a batch that failed here (text formatting, a sink that refused an image) is reported by the caller and writes NO files: a writer
    // started for it would make the files of a failed call appear later, in the background
    for (uint32_t b = 0; b < B; ++b) if (wanted(b) && wrc[b] != R3DM_OK) return R3DM_OK;
    const int nice_value = c->background_nice;
    try {
        // (two threads per context: the writes have the caller's next phase to hide behind and must not take its cores)
        c->file_writer = std::thread([c, jobs, nice_value, writer_team = std::min(host_team, 2), wait_desc = n_total != 0]() {
            r3dm_background_thread(nice_value);
            const double t0 = now_ms();
            if (wait_desc && (hipSetDevice(c->device) != hipSuccess || hipEventSynchronize(c->ev_desc) != hipSuccess)) {
                c->file_writer_rc = R3DM_ERR_HIP; c->file_writer_err = "the descriptors did not reach the host";
                return;
            }
            std::vector<int> rcs(jobs->size(), R3DM_OK); std::vector<std::string> errs(jobs->size());
            r3dm_parallel_for((long)jobs->size(), writer_team, [&](long b) {
                const FeatJob& j = (*jobs)[(size_t)b];
                if (j.feat.empty()) return;
                try { rcs[(size_t)b] = write_feat_desc_files(errs[(size_t)b], j); }
                catch (...) { rcs[(size_t)b] = R3DM_ERR_NOMEM; }
            });
            // (the report comes late -- at the wait, or at this context's next batch: it names the file so that it can be traced to its batch)
            for (size_t b = 0; b < rcs.size(); ++b)
                if (rcs[b] != R3DM_OK && c->file_writer_rc == R3DM_OK) {
                    c->file_writer_rc = rcs[b];
                    c->file_writer_err = "deferred feature files of " + (*jobs)[b].feat + ": " + (errs[b].empty() ? std::string("write failed") : errs[b]);
                }
            c->file_writer_ms += now_ms() - t0;
        });
    } catch (...) { c->err = "cannot start the feature-file writer"; return R3DM_ERR_NOMEM; }
    return R3DM_OK;
}

// detectAndExtract (src/Regard3DFeatures.cpp:206-222) for keypointDetectorList_ = {"Fast-AKAZE"} or {"AKAZE"} (the context's
// r3dm_set_keypoint_detector) over a batch of B same-size images + KeypointSet::saveToBinFile of each.  Every image of the batch is
// computed (the skip rule is the caller's: it only batches images it wants).  feat_paths / desc_paths: B entries, an image without
// both is computed and delivered nowhere.
int extract_features_batch_impl(r3dm_ctx* c, uint32_t B, const float* const* grays, const unsigned char* const* bgrs,
                                uint32_t width, uint32_t height, float threshold, const char* const* feat_paths,
                                const char* const* desc_paths, uint32_t* n_features)
{
    if (!c || B == 0) return R3DM_ERR_INVALID;
    int rc = descriptor_arm_check(c);
    if (rc != R3DM_OK) return rc;
    DetectedBatch det;
    rc = detect_batch(c, B, grays, bgrs, width, height, threshold, det);
    if (rc != R3DM_OK) return rc;
    const double t_liop = now_ms();
    // helper threads of this batch: the cores the process really owns (its cgroup quota), shared with the other batches in flight
    static std::atomic<int> batches_in_flight{0};
    struct InFlight { std::atomic<int>& n; int mine; InFlight(std::atomic<int>& a) : n(a), mine(a.fetch_add(1) + 1) {} ~InFlight() { n.fetch_sub(1); } } in_flight(batches_in_flight);
    const int host_team = r3dm_host_team(8, std::max(2, in_flight.mine));
    BatchKeypoints K;
    keypoints_and_maps(det, B, host_team, !descriptor_arm_by_id(c->descriptor_arm)->level_planes, K);
    const bool deferred = c->defer_files;
    BatchRows rows;
    if (K.total() && (rc = describe_batch(c, det, width, height, K, deferred, host_team, rows)) != R3DM_OK) return rc;
    if (!deferred) c->stats.ms_liop_wall = now_ms() - t_liop;
    const double t_io = now_ms();
    std::vector<int> wrc(B, R3DM_OK);
    std::vector<std::string> werr(B);
    if ((rc = deliver_batch(c, B, feat_paths, desc_paths, det, K, rows, deferred, host_team, t_liop, wrc, werr)) != R3DM_OK) return rc;
    for (uint32_t b = 0; b < B; ++b) {
        if (feat_paths[b] && desc_paths[b] && wrc[b] != R3DM_OK) { c->err = werr[b].empty() ? "out of host memory" : werr[b]; return wrc[b]; }
        if (n_features) n_features[b] = (uint32_t)det.count(b);
    }
    c->stats.ms_feature_files = now_ms() - t_io;            // (the sink's time included)
    c->feat_totals.ms_liop_kernels += K.total() ? c->stats.ms_liop_kernel : 0.0;
    c->feat_totals.ms_wall += c->stats.ms_liop_wall + c->stats.ms_feature_files;
    c->feat_totals.ms_files += c->stats.ms_feature_files;
    return R3DM_OK;
}

}  // namespace

extern "C" int r3dm_extract_features_to_files(r3dm_ctx* c, const float* gray, uint32_t width, uint32_t height, float threshold,
                                              const char* feat_path, const char* desc_path, uint32_t* n_features)
{
    return r3dm_guarded(c, [&]() -> int {
        if (!c || !gray || !feat_path || !desc_path) return R3DM_ERR_INVALID;
        if (n_features) *n_features = 0;
        { const int arc = descriptor_arm_check(c); if (arc != R3DM_OK) return arc; }
        // "Test if descriptor and feature was already computed" (src/threads/R3DFeaturesThread.cpp:139-142): when BOTH files exist the
        // work item does nothing -- files left by a run with other parameters are reused, the reference wipes the matches directory
        // instead (src/threads/R3DComputeMatchesThread.cpp:84-86).  n_features then reports the row count of the existing .desc.
        if (both_files_exist(feat_path, desc_path, n_features)) return R3DM_OK;
        return extract_features_batch_impl(c, 1, &gray, nullptr, width, height, threshold, &feat_path, &desc_path, n_features);
    });
}

// B same-size images through detector + LIOP + files in one pass (no skip rule: the caller decides what to compute).
// grays: B pointers to height x width floats, or NULL and bgrs: B pointers to height x width x 3 bytes (BGR, as cv::imread decodes).
extern "C" int r3dm_extract_features_batch(r3dm_ctx* c, uint32_t n_images, const float* const* grays, const unsigned char* const* bgrs,
                                           uint32_t width, uint32_t height, float threshold, const char* const* feat_paths,
                                           const char* const* desc_paths, uint32_t* n_features)
{
    return r3dm_guarded(c, [&]() -> int {
        if (!feat_paths || !desc_paths) return R3DM_ERR_INVALID;
        return extract_features_batch_impl(c, n_images, grays, bgrs, width, height, threshold, feat_paths, desc_paths, n_features); });
}

// ------------------------------------------------------------------------------------------------
// the features stage over a whole image list: R3DFeaturesThread::extractFeaturesAndDescriptors
// (src/threads/R3DFeaturesThread.cpp:38-89) -- a pool of CPUs + 1 worker threads pulling images off a work list (:93-121), each
// running processWorkItem (:123-210).  The reference admits ONE image at a time into the A-KAZE scale space
// (initAKAZESemaphore(1), src/R3DComputeMatches.cpp:1847; src/Regard3DFeatures.cpp:71-125) to bound host memory; HBM does not
// need that: every context of an r3dm_multi (r3dm_multi_create with a device id repeated K times = K streams + work buffers on
// that device; or one per GPU) is a worker that pulls BATCHES of same-size images off the list from its own host thread -- B images
// per pass of the detector, K passes in flight, the host part of one pass (angles, files) hidden behind the kernels of the others.
// An image whose .feat AND .desc both exist is skipped, exactly as processWorkItem does (:139-142: stale files of other parameters
// are reused; the reference wipes the matches directory instead, src/threads/R3DComputeMatchesThread.cpp:84-86); n_features then
// reports the row count of the existing .desc.
// ------------------------------------------------------------------------------------------------
namespace {

// batch size for images of w x h on context c: 8 when HBM allows (the Fast arm's work buffers take ~125 bytes per pixel and image,
// the classic arm's ~64: six level-0 planes, three per level over four octaves, the walk's arrays), fewer for very large images or a
// nearly full device
uint32_t ak_batch_for(r3dm_ctx* c, uint32_t w, uint32_t h, uint32_t want)
{
    size_t free_b = 0, total_b = 0;
    (void)hipSetDevice(c->device);
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 1;
    double per_image = 0.0, held = 0.0;                // held: bytes the arm's buffers already occupy that this batch would use again
    if (c->detector_arm == R3DM_DETECTOR_AKAZE) {
        // (the classic arm's buffers grow and are kept: what it already holds counts as free)
        per_image = (double)w * h * 4.0 * 16.0 + 64e6;
        size_t bytes = 0;
        for (const DevBuf& d : c->ac_bufs) bytes += d.cap;
        held = (double)bytes;
    } else {
        per_image = (double)w * h * 4.0 * 32.0 + 64e6;
        held = c->ak_w == (int)w && c->ak_h == (int)h ? (double)c->ak_B * per_image : 0.0;
    }
    const double budget = (double)free_b * 0.5 + held;
    uint32_t b = want;
    while (b > 1 && b * per_image > budget) --b;
    return b;
}

int multi_extract_impl(r3dm_multi* m, uint32_t n_images, const float* const* grays, const unsigned char* const* bgrs,
                       const uint32_t* widths, const uint32_t* heights, float threshold, const char* const* feat_paths,
                       const char* const* desc_paths, uint32_t* n_features, uint32_t* skipped, uint32_t batch, char* err, size_t err_cap)
{
    if (!m || (n_images && ((!grays && !bgrs) || !widths || !heights || !feat_paths || !desc_paths))) return R3DM_ERR_INVALID;
    // per image: gray floats if grays[i] is set, else 8-bit BGR
    auto is_gray = [&](uint32_t i) { return grays && grays[i]; };
    if (err && err_cap) err[0] = 0;
    const uint32_t concurrency = (uint32_t)r3dm_multi_num_devices(m);
    if (concurrency == 0) return R3DM_ERR_INVALID;
    if (batch == 0) batch = 8;
    for (uint32_t k = 0; k < concurrency; ++k) {                     // (before the skip rule and the workers: a refused call does nothing)
        r3dm_ctx* c = r3dm_multi_ctx(m, (int)k);
        const int arc = descriptor_arm_check(c);
        if (arc != R3DM_OK) { if (err && err_cap) { strncpy(err, r3dm_last_error(c), err_cap - 1); err[err_cap - 1] = 0; } return arc; }
    }
    int rc_all = R3DM_OK;
    std::vector<std::thread> th;
    try {
        // work list: the images still to compute (the skip rule applied up front), grouped by size so that a worker's batch is
        // a run of same-size images; the order inside a size class is the caller's
        std::vector<uint32_t> todo;
        for (uint32_t i = 0; i < n_images; ++i) {
            if (skipped) skipped[i] = 0;
            uint32_t rows = 0;
            if (both_files_exist(feat_paths[i], desc_paths[i], &rows)) {            // processWorkItem: already computed
                if (n_features) n_features[i] = rows;
                if (skipped) skipped[i] = 1;
            } else todo.push_back(i);
        }
        for (uint32_t i : todo) if (!is_gray(i) && !(bgrs && bgrs[i])) return R3DM_ERR_INVALID;      // an image to compute without pixels
        std::stable_sort(todo.begin(), todo.end(), [&](uint32_t a, uint32_t b) {
            return std::make_tuple(widths[a], heights[a], is_gray(a)) < std::make_tuple(widths[b], heights[b], is_gray(b)); });
        std::mutex mu;
        size_t next = 0;
        std::vector<int> rcs(concurrency, R3DM_OK);
        std::vector<std::string> errs(concurrency);
        // small lists: shrink the batch so that every worker gets something to do
        const uint32_t fair = (uint32_t)std::max<size_t>(1, (todo.size() + concurrency - 1) / concurrency);
        auto worker = [&](uint32_t k) noexcept {
            try {
                r3dm_ctx* c = r3dm_multi_ctx(m, (int)k);
                for (;;) {
                    std::vector<uint32_t> mine;
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (next >= todo.size() || rcs[k] != R3DM_OK) return;
                        const uint32_t w = widths[todo[next]], h = heights[todo[next]];
                        const bool gk = is_gray(todo[next]);
                        const uint32_t bmax = ak_batch_for(c, w, h, std::min(batch, fair));
                        while (next < todo.size() && mine.size() < bmax && widths[todo[next]] == w && heights[todo[next]] == h && is_gray(todo[next]) == gk) mine.push_back(todo[next++]);
                    }
                    const uint32_t B = (uint32_t)mine.size();
                    std::vector<const float*> g(B); std::vector<const unsigned char*> bg(B);
                    std::vector<const char*> fp(B), dp(B); std::vector<uint32_t> nf(B, 0);
                    const bool gk = is_gray(mine[0]);
                    for (uint32_t j = 0; j < B; ++j) { if (gk) g[j] = grays[mine[j]]; else bg[j] = bgrs[mine[j]]; fp[j] = feat_paths[mine[j]]; dp[j] = desc_paths[mine[j]]; }
                    c->feat_sink_ids = mine.data();                    // the sink (if any) is told the caller's indices
                    const int rc = r3dm_extract_features_batch(c, B, gk ? g.data() : nullptr, gk ? nullptr : bg.data(), widths[mine[0]], heights[mine[0]],
                                                               threshold, fp.data(), dp.data(), nf.data());
                    c->feat_sink_ids = nullptr;
                    if (n_features) for (uint32_t j = 0; j < B; ++j) n_features[mine[j]] = nf[j];
                    if (rc != R3DM_OK) { rcs[k] = rc; errs[k] = std::string("image ") + std::to_string(mine[0]) + " (batch of " + std::to_string(B) + "): " + r3dm_last_error(c); }
                }
            } catch (...) { rcs[k] = R3DM_ERR_NOMEM; }          // nothing leaves a worker thread by exception (std::terminate)
        };
        for (uint32_t k = 1; k < concurrency; ++k) th.emplace_back(worker, k);
        worker(0);
        for (auto& t : th) t.join();
        th.clear();
        for (uint32_t k = 0; k < concurrency; ++k)
            if (rcs[k] != R3DM_OK && rc_all == R3DM_OK) {
                rc_all = rcs[k];
                if (err && err_cap) { strncpy(err, errs[k].c_str(), err_cap - 1); err[err_cap - 1] = 0; }
            }
    } catch (...) {
        for (auto& t : th) if (t.joinable()) t.join();          // thread creation failed half way: the started workers finish first
        rc_all = R3DM_ERR_NOMEM;
    }
    return rc_all;
}

}  // namespace

// fn(context) on every context of m: the first failure's code
template <class F>
static int multi_each(r3dm_multi* m, F&& fn)
{
    if (!m) return R3DM_ERR_INVALID;
    int rc = R3DM_OK;
    for (int k = 0; k < r3dm_multi_num_devices(m); ++k) { const int r = fn(r3dm_multi_ctx(m, k)); if (r != R3DM_OK && rc == R3DM_OK) rc = r; }
    return rc;
}

extern "C" int r3dm_set_features_sink(r3dm_ctx* c, r3dm_features_sink sink, void* user)
{
    if (!c) return R3DM_ERR_INVALID;
    c->feat_sink = sink; c->feat_sink_user = sink ? user : nullptr;
    return R3DM_OK;
}

extern "C" int r3dm_set_deferred_feature_files(r3dm_ctx* c, int on)
{
    if (!c) return R3DM_ERR_INVALID;
    c->defer_files = on != 0;
    return on ? R3DM_OK : features_files_join(c);
}

extern "C" int r3dm_set_background_nice(r3dm_ctx* c, int nice_value)
{
    if (!c || nice_value < 0 || nice_value > 19) return R3DM_ERR_INVALID;
    c->background_nice = nice_value;
    return R3DM_OK;
}

extern "C" int r3dm_features_files_wait(r3dm_ctx* c)
{
    if (!c) return R3DM_ERR_INVALID;
    return features_files_join(c);
}

extern "C" int r3dm_set_keypoint_detector(r3dm_ctx* c, int arm)
{
    if (!c) return R3DM_ERR_INVALID;
    if (arm != R3DM_DETECTOR_FAST_AKAZE && arm != R3DM_DETECTOR_AKAZE) { c->err = "r3dm_set_keypoint_detector: unknown arm " + std::to_string(arm); return R3DM_ERR_INVALID; }
    c->detector_arm = arm;
    return R3DM_OK;
}

extern "C" int r3dm_set_descriptor_arm(r3dm_ctx* c, int arm)
{
    if (!c) return R3DM_ERR_INVALID;
    if (!descriptor_arm_by_id(arm)) { c->err = "r3dm_set_descriptor_arm: unknown arm " + std::to_string(arm); return R3DM_ERR_INVALID; }
    c->descriptor_arm = arm;
    return R3DM_OK;
}

extern "C" int r3dm_multi_set_background_nice(r3dm_multi* m, int nice_value)
{
    return multi_each(m, [&](r3dm_ctx* c) { return r3dm_set_background_nice(c, nice_value); });
}

extern "C" int r3dm_multi_set_deferred_feature_files(r3dm_multi* m, int on)
{
    return multi_each(m, [&](r3dm_ctx* c) { return r3dm_set_deferred_feature_files(c, on); });
}

extern "C" int r3dm_multi_set_features_sink(r3dm_multi* m, r3dm_features_sink sink, void* user)
{
    return multi_each(m, [&](r3dm_ctx* c) { return r3dm_set_features_sink(c, sink, user); });
}

extern "C" int r3dm_multi_set_keypoint_detector(r3dm_multi* m, int arm)
{
    if (arm != R3DM_DETECTOR_FAST_AKAZE && arm != R3DM_DETECTOR_AKAZE) return R3DM_ERR_INVALID;
    return multi_each(m, [&](r3dm_ctx* c) { return r3dm_set_keypoint_detector(c, arm); });
}

extern "C" int r3dm_multi_set_descriptor_arm(r3dm_multi* m, int arm)
{
    if (!descriptor_arm_by_id(arm)) return R3DM_ERR_INVALID;
    return multi_each(m, [&](r3dm_ctx* c) { return r3dm_set_descriptor_arm(c, arm); });
}

extern "C" int r3dm_multi_features_files_wait(r3dm_multi* m, char* err, size_t err_cap)
{
    if (!m) return R3DM_ERR_INVALID;
    if (err && err_cap) err[0] = 0;
    return multi_each(m, [&, first = true](r3dm_ctx* c) mutable {
        const int r = features_files_join(c);
        if (r != R3DM_OK && first) { first = false; if (err && err_cap) { strncpy(err, r3dm_last_error(c), err_cap - 1); err[err_cap - 1] = 0; } }
        return r;
    });
}

extern "C" int r3dm_multi_extract_features(r3dm_multi* m, uint32_t n_images, const float* const* grays, const uint32_t* widths,
                                           const uint32_t* heights, float threshold, const char* const* feat_paths,
                                           const char* const* desc_paths, uint32_t* n_features, uint32_t* skipped,
                                           char* err, size_t err_cap)
{
    return multi_extract_impl(m, n_images, grays, nullptr, widths, heights, threshold, feat_paths, desc_paths, n_features, skipped, 0, err, err_cap);
}

extern "C" int r3dm_multi_extract_features_ex(r3dm_multi* m, uint32_t n_images, const float* const* grays, const unsigned char* const* bgrs,
                                              const uint32_t* widths, const uint32_t* heights, float threshold, const char* const* feat_paths,
                                              const char* const* desc_paths, uint32_t* n_features, uint32_t* skipped, uint32_t batch,
                                              char* err, size_t err_cap)
{
    return multi_extract_impl(m, n_images, grays, bgrs, widths, heights, threshold, feat_paths, desc_paths, n_features, skipped, batch, err, err_cap);
}
