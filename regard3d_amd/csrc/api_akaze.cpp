// api_akaze.cpp -- part of the host side of libr3dm.so (see r3dm_ctx.hpp for the file map): keypoint detection.  The frame both detector
// arms stand in (argument checks, gray-or-BGR upload, INTER_AREA tables, statistics tail, the detect entry over a DetectedBatch, the choice
// of the arm), then the Fast-A-KAZE arm (kernels_akaze.hip): ak_detect_batch in its phases -- buffers, scale space, detection with regrow,
// read-back -- the one pass of the level-plane descriptors (ak_describe_pass: MLDB-486, M-SURF-64) and the entries.  The classic arm's launch
// sequence is api_akaze_classic.cpp; what is shared and what stays per arm, of the detectors and of the descriptors: DESIGN.md section 4.21.  There is no CPU fallback in this file: when HIP fails, the call fails.  At the end, developer build only: the
// arm's tail on a caller's planes and lists (r3dm_dev_akaze_tail), and its head -- scale space, extrema, in-level pruning -- on a caller's images
// or determinant planes, every plane and list read back (r3dm_dev_akaze_head, r3dm_dev_akaze_extrema).
#include "r3dm_ctx.hpp"

// ======== the frame of both arms
// getGaussianKernel(n, sigma, CV_32F) for gaussian_2D_convolutionV2's kernel size rule (nldiffusion_functions.cpp:39-58)
AkTaps ak_taps(float sigma)
{
    AkTaps t{};
    int k = (int)ceil(2.0f * (1.0f + (sigma - 0.8f) / (0.3f)));
    if ((k % 2) == 0) k += 1;
    t.n = k;
    const double s = sigma;
    const double scale2X = -0.5 / (s * s);
    double sum = 0;
    for (int i = 0; i < k; ++i) {
        const double x = i - (k - 1) * 0.5;
        const double v = std::exp(scale2X * x * x);
        t.k[i] = (float)v;
        sum += t.k[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < k; ++i) t.k[i] = (float)(t.k[i] * sum);
    return t;
}

// fed_is_prime_internal (fed.cpp) of both libraries.  (They form the trial-division bound as sqrt(1.0f + n) and as sqrt(n + 1.0): the
// same integer for every n the FED cycle lengths can reach)
bool ak_is_prime(int number)
{
    if (number <= 1) return false;
    if (number == 2 || number == 3 || number == 5 || number == 7) return true;
    if ((number % 2) == 0 || (number % 3) == 0 || (number % 5) == 0 || (number % 7) == 0) return false;
    const int upper = (int)sqrt(number + 1.0);
    for (int divisor = 11; divisor <= upper; divisor += 2) if (number % divisor == 0) return false;
    return true;
}

bool detect_args_ok(const r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height)
{
    if (!c || B == 0 || (!images && !bgrs)) return false;
    for (uint32_t b = 0; b < B; ++b) if (!(images ? (const void*)images[b] : (const void*)bgrs[b])) return false;
    return (uint64_t)width * height <= (1ull << 30) && B <= 4096;
}

int detect_upload(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, size_t n0, float* gray, unsigned char* stage)
{
    hipStream_t st = c->stream;
    if (images) {
        for (uint32_t b = 0; b < B; ++b) R3DM_HIP(c, hipMemcpyAsync(gray + b * n0, images[b], n0 * 4, hipMemcpyDefault, st));
    } else {
        // 8-bit BGR -> float / 255 -> gray
        for (uint32_t b = 0; b < B; ++b) R3DM_HIP(c, hipMemcpyAsync(stage + b * n0 * 4, bgrs[b], n0 * 3, hipMemcpyDefault, st));
        for (uint32_t b = 0; b < B; ++b) R3DM_HIP(c, ak_bgr_to_gray(st, stage + b * n0 * 4, gray + b * n0, n0));
    }
    return R3DM_OK;
}

// (its own two buffers, released before it returns: the conversion must not depend on, or disturb, either arm's work images)
extern "C" int r3dm_gray_from_bgr8(r3dm_ctx* c, const unsigned char* bgr, uint32_t width, uint32_t height, float* gray_out)
{
    if (!c || !bgr || !gray_out || !width || !height) return R3DM_ERR_INVALID;
    R3DM_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)width * height;
    DevBuf in, out;
    R3DM_HIP(c, in.ensure(n * 3));
    R3DM_HIP(c, out.ensure(n * 4));
    const int rc = detect_upload(c, 1, nullptr, &bgr, n, out.as<float>(), in.as<unsigned char>());
    if (rc != R3DM_OK) return rc;
    R3DM_HIP(c, hipMemcpyAsync(gray_out, out.p, n * 4, hipMemcpyDefault, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    in.release(); out.release();
    return R3DM_OK;
}

// computeResizeAreaTab (imgproc/resize.cpp) as a CSR over destination cells
static void ak_area_tab(int ssize, int dsize, std::vector<AkAreaTab>& tab, std::vector<int>& begin)
{
    const double scale = (double)ssize / dsize;
    tab.clear(); begin.assign(dsize + 1, 0);
    for (int dx = 0; dx < dsize; ++dx) {
        begin[dx] = (int)tab.size();
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3) tab.push_back({sx1 - 1, (float)((sx1 - fsx1) / cell)});
        for (int sx = sx1; sx < sx2; ++sx) tab.push_back({sx, (float)(1.0 / cell)});
        if (fsx2 - sx2 > 1e-3) tab.push_back({sx2, (float)(std::min(std::min(fsx2 - sx2, 1.), cell) / cell)});
    }
    begin[dsize] = (int)tab.size();
}

int detect_area_tabs(r3dm_ctx* c, DevBuf& buf, const std::vector<AkLevelHost>& lv, std::vector<HalfTabs>& tabs)
{
    const int nl = (int)lv.size();
    tabs.assign(nl, HalfTabs());
    std::vector<unsigned char> blob;
    std::vector<std::array<size_t, 4>> offs(nl, {(size_t)-1, 0, 0, 0});                 // x table, y table, x begins, y begins
    auto put = [&](const void* p, size_t bytes) { const size_t at = (blob.size() + 15) / 16 * 16; blob.resize(at + bytes); memcpy(blob.data() + at, p, bytes); return at; };
    for (int i = 1; i < nl; ++i) {
        if (lv[i].octave == lv[i - 1].octave) continue;
        const int sw = lv[i - 1].w, sh = lv[i - 1].h, lw = lv[i].w, lh = lv[i].h;
        if (lw * 2 == sw && lh * 2 == sh) continue;
        std::vector<AkAreaTab> tx, ty; std::vector<int> bx, by;
        ak_area_tab(sw, lw, tx, bx); ak_area_tab(sh, lh, ty, by);
        offs[i][0] = put(tx.data(), tx.size() * sizeof(AkAreaTab)); offs[i][1] = put(ty.data(), ty.size() * sizeof(AkAreaTab));
        offs[i][2] = put(bx.data(), bx.size() * 4); offs[i][3] = put(by.data(), by.size() * 4);
    }
    if (blob.empty()) return R3DM_OK;
    R3DM_HIP(c, buf.ensure(blob.size() + 64));
    R3DM_HIP(c, hipMemcpyAsync(buf.p, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));                 // `blob` leaves scope
    const unsigned char* base = buf.as<unsigned char>();
    for (int i = 1; i < nl; ++i)
        if (offs[i][0] != (size_t)-1) {
            tabs[i].xt = (const AkAreaTab*)(base + offs[i][0]); tabs[i].yt = (const AkAreaTab*)(base + offs[i][1]);
            tabs[i].xb = (const int*)(base + offs[i][2]); tabs[i].yb = (const int*)(base + offs[i][3]);
        }
    return R3DM_OK;
}

void detect_finish(r3dm_ctx* c, uint32_t B, double t_call, uint64_t n_keypoints, double algorithmic_bytes)
{
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.n_detect_images = B;
    c->stats.ms_detect_kernels = ms;
    c->stats.ms_detect = now_ms() - t_call;
    r3dm_features_totals& T = c->feat_totals;
    T.n_images += B; T.n_passes += 1; T.ms_detect_kernels += ms; T.detect_algorithmic_bytes += algorithmic_bytes; T.ms_wall += c->stats.ms_detect;
    T.n_keypoints += n_keypoints;
}

static int ak_detect_batch_smax(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height,
                                float threshold, float smax, DetectedBatch& out);

int detect_batch(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height,
                 float threshold, DetectedBatch& out)
{
    if (c && c->detector_arm == R3DM_DETECTOR_AKAZE) return ac_detect_batch(c, B, images, bgrs, width, height, threshold, out);
    // (the Fast arm's level table carries the border of the descriptor that will read its planes; the setter admits the table's ids only)
    const DescriptorArm& arm = *descriptor_arm_by_id(c ? c->descriptor_arm : R3DM_DESCRIPTOR_LIOP);
    return ak_detect_batch_smax(c, B, images, bgrs, width, height, threshold, ak_smax(arm), out);
}

int detect_entry(r3dm_ctx* c, DetectArm* arm, bool single, uint32_t B, const float* const* images, uint32_t width, uint32_t height, float threshold,
                 float* const* keypoints_out, float* const* responses_out, uint32_t cap, uint32_t* n_out, DetectedBatch& d)
{
    if (!c || !images || !n_out || (cap && !keypoints_out) || (single && (!images[0] || (cap && !keypoints_out[0])))) return R3DM_ERR_INVALID;
    if (single) *n_out = 0;
    const int rc = arm(c, B, images, nullptr, width, height, threshold, d);
    if (rc != R3DM_OK) return rc;
    for (uint32_t b = 0; b < B; ++b) {
        const size_t n = d.count(b);
        for (size_t k = 0; k < n && k < cap; ++k) {
            d.keypoint(b, k, keypoints_out[b] + 4 * k);
            if (responses_out && responses_out[b]) responses_out[b][k] = d.response(b, k);
        }
        n_out[b] = (uint32_t)n;
    }
    return R3DM_OK;
}

// ======== keypoint detection: Fast-A-KAZE (kernels_akaze.hip)
namespace {

// AKAZEFeaturesV2::Allocate_Memory_Evolution (src/thirdparty/fast-akaze/AKAZEFeatures.cpp:73-131) with the AKAZE2::create()
// defaults (AKAZEConfig.h:18-43): 4 octaves x 4 sublevels, soffset 1.6, derivative_factor 1.5.  The border is the DESCRIPTOR's
// (:78-84): smax = 10 sqrt(2) for MLDB (what the detector, LIOP and MLDB arms run on), 12 sqrt(2) for the KAZE descriptors (M-SURF-64):
// ak_smax of the arm's row in descriptor_arms.hpp.  The larger border cuts the table earlier, so the M-SURF table is a prefix of the
// other with wider borders, and detection under it differs near the frame and on small images.
const float kAkSmaxDetector = ak_smax(*descriptor_arm_by_id(R3DM_DESCRIPTOR_LIOP)), kAkSmaxMsurf = ak_smax(*descriptor_arm_by_id(R3DM_DESCRIPTOR_MSURF));
std::vector<AkLevelHost> ak_levels(int w, int h, float smax = kAkSmaxDetector)
{
    std::vector<AkLevelHost> lv;
    const int omax = 4, nsub = 4;
    const float soffset = 1.6f, dfac = 1.5f;
    int lh = h, lw = w, power = 1;
    for (int i = 0; i < omax; ++i) {
        for (int j = 0; j < nsub; ++j) {
            AkLevelHost e{};
            e.w = lw; e.h = lh;
            e.esigma = soffset * powf(2.f, (float)j / nsub + i);
            e.sigma_size = (int)(e.esigma * dfac / power + 0.5f);
            e.border = (int)(smax * e.sigma_size + 0.5f) + 1;
            e.etime = 0.5f * (e.esigma * e.esigma);
            e.octave = i; e.sublevel = j; e.ratio = (float)power;
            if (e.border * 2 + 1 >= lw || e.border * 2 + 1 >= lh) return lv;
            lv.push_back(e);
        }
        power <<= 1; lh >>= 1; lw >>= 1;
        if (lw < 80 || lh < 40) break;
    }
    return lv;
}

// fed_tau_by_process_timeV2(T, 1, 0.25, reordering) (fed.cpp): float arithmetic, cosf -- the classic arm's ac_fed_tau works in double
std::vector<float> ak_fed_tau(float T)
{
    const float tau_max = 0.25f;
    const int n = (int)(ceilf(sqrtf(3.0f * T / tau_max + 0.25f) - 0.5f - 1.0e-8f) + 0.5f);
    std::vector<float> tau;
    if (n <= 0) return tau;
    const float scale = 3.0f * T / (tau_max * (float)(n * (n + 1)));
    std::vector<float> tauh(n);
    const float cc = 1.0f / (4.0f * n + 2.0f);
    const float d = scale * tau_max / 2.0f;
    for (int k = 0; k < n; ++k) { const float hh = cosf((float)3.1415926535897932384626433832795 * (2.0f * k + 1.0f) * cc); tauh[k] = d / (hh * hh); }
    if (n == 1) return tauh;
    const int kappa = n / 2;
    int prime = n + 1;
    while (!ak_is_prime(prime)) prime++;
    tau.resize(n);
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index = 0;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
        tau[l] = tauh[index];
    }
    return tau;
}

// ------------------------------------------------------------------------------------------------
// The detector over a BATCH of B same-size images.  One image alone cannot fill the chip below the first octave: its ~550
// dependent launches are a few microseconds each (profiles/r02_e_akaze_kernel_stats.txt), so a single image waits for launch
// latency, not for HBM.  The launch sequence depends on the image SIZE only, so the same ~550 launches serve B images
// (blockIdx.z = image), and nothing in the chain goes to the host: the k-contrast stays on the device, the candidate slots are
// laid out on the device from a capacity (ak_layout_kernel) instead of counts read back, list lengths are read by grid-stride
// kernels, and the survivors of all levels are compacted into one 32-byte record per keypoint (ak_compact_kernel).  The host sees
// the batch twice: the per-image counts, then the records.
// ------------------------------------------------------------------------------------------------

// c->ak_bufs, each B planes: [0] image, [1..10] level-0 sized work images, then 4 per level (Lt, Lx, Ly, Ldet), then the T_* buffers
enum { B_IMG = 0, B_SMOOTH, B_LXX, B_LXY, B_LYY, B_TMP, B_TMP2, B_WX, B_WY, B_FLOW, B_LT2, B_SMALL, B_LEVEL0 };
enum { T_META = 0, T_SLOTS, T_DESC /* items, extra bytes and rows of the level-plane descriptor pass */, T_TABS, T_RECS, T_COUNT = 8 };

// the launches of one level i > 0 (ak_level_plan decides, ak_evolve_level issues): the one-pass level head (with its rows per band) or the
// four launches, and per FED launch its form, its steps and (marching) its rows per band
enum { AK_FED_STEP = 0, AK_FED_MULTI = 1, AK_FED_MARCH = 2 };   // ak_fed_step (one step), ak_fed_multi (steps through LDS), ak_fed_march (marching strips)
struct AkLevelPlan { bool head = false; int head_rows = 0; std::vector<int> form, steps, rows; };

// one pass of the arm: what its phases share
struct AkPass {
    r3dm_ctx* c; hipStream_t st;
    uint32_t B; int iB, w, h, nl; size_t n0;
    const std::vector<AkLevelHost>& lv;
    float *img = nullptr, *smooth = nullptr, *tmp = nullptr, *tmp2 = nullptr, *flow = nullptr, *lt2 = nullptr;
    // per image (4096 words apart, kernels_akaze.hip kAkSmallWords): [0] maximum of the gradient modulus (float bits),
    // [16..) 300-bin histogram, [1024 + o] 1 / k^2 of octave o (ak_kcontrast_kernel)
    uint32_t* small = nullptr;
    uint32_t* hmax_bits() const { return small; }
    uint32_t* hist() const { return small + 16; }
    float* inv_k2() const { return reinterpret_cast<float*>(small + 1024); }
    AkTaps taps_off, taps_one;
    std::vector<HalfTabs> half_tabs;
    // algorithmic HBM bytes of the launch sequence: every pass reads / writes whole image planes once
    // Beside it the COMPULSORY count: the planes a perfectly fused level would still move -- a smoothed plane in and out, the determinant
    // out, the conductivity out, and per FED step the evolving plane in and out (a step needs its neighbours' previous step, so steps do
    // not fuse across a plane without halo recomputation); the k-contrast statistics ride on the Gaussian.  This is round 2's 8 bytes per
    // pixel and pass; a roofline fraction on it falls when launches are fused, the as-structured one does not.
    double planes_px = 0.0, compulsory_px = 0.0;
    void tally(int lw, int lh, int n_planes, int n_compulsory) { planes_px += (double)lw * lh * n_planes; compulsory_px += (double)lw * lh * n_compulsory; }
    DevBuf& buf(int k) const { return c->ak_bufs[k]; }
    DevBuf& tail(int k) const { return c->ak_bufs[B_LEVEL0 + 4 * nl + k]; }
    float* Lt(int i) const { return buf(B_LEVEL0 + 4 * i).as<float>(); }
    float* Lx(int i) const { return buf(B_LEVEL0 + 4 * i + 1).as<float>(); }
    float* Ly(int i) const { return buf(B_LEVEL0 + 4 * i + 2).as<float>(); }
    float* Ldet(int i) const { return buf(B_LEVEL0 + 4 * i + 3).as<float>(); }
};

// ---- phase 1: the buffers, keyed on (w, h, B) and released when the key changes
int ak_buffers(AkPass& p)
{
    r3dm_ctx* c = p.c; const int nl = p.nl;
    if (c->ak_w != p.w || c->ak_h != p.h || c->ak_B < p.iB || c->ak_bufs.size() != (size_t)B_LEVEL0 + 4 * nl + T_COUNT) {
        for (DevBuf& b : c->ak_bufs) b.release();
        c->ak_bufs.assign((size_t)B_LEVEL0 + 4 * nl + T_COUNT, DevBuf());
        c->ak_w = p.w; c->ak_h = p.h; c->ak_B = p.iB;
    }
    const size_t PB = (size_t)c->ak_B;                            // planes per buffer (the largest batch of this size so far)
    for (int k = B_IMG; k <= B_LT2; ++k) if (k != B_LYY && k != B_LXX && k != B_LXY && k != B_WX && k != B_WY) R3DM_HIP(c, p.buf(k).ensure(PB * p.n0 * 4));      // (the second derivatives are folded into the determinant kernel)
    R3DM_HIP(c, p.buf(B_SMALL).ensure(PB * 4096 * 4));
    for (int i = 0; i < nl; ++i)
        for (int q = 0; q < 4; ++q) R3DM_HIP(c, p.buf(B_LEVEL0 + 4 * i + q).ensure(PB * (size_t)p.lv[i].w * p.lv[i].h * 4));
    p.img = p.buf(B_IMG).as<float>(); p.smooth = p.buf(B_SMOOTH).as<float>();
    p.tmp = p.buf(B_TMP).as<float>(); p.tmp2 = p.buf(B_TMP2).as<float>();
    p.flow = p.buf(B_FLOW).as<float>(); p.lt2 = p.buf(B_LT2).as<float>();
    p.small = p.buf(B_SMALL).as<uint32_t>();
    return R3DM_OK;
}

// ---- phase 2: Create_Nonlinear_Scale_Space (:245-369), Compute_Base_Evolution_Level (:199-237): ~550 launches for a 12 Mpx image,
// none of which needs the host -- the k-contrast (compute_k_percentileV2: maximum, 300-bin histogram, percentile scan) stays
// on the device.  (Replaying the sequence as a hipGraph was measured SLOWER than issuing it, 15.8 vs 7.5 ms per image:
// DESIGN.md section 4.8 (c); the capture code is in the history.)
#define AK_TRY(call) do { if ((e = (call)) != hipSuccess) return e; } while (0)

// The launch plan of level i > 0 for a batch of nb images: a function of the level table, nb and (developer build) the knobs alone.
AkLevelPlan ak_level_plan(const std::vector<AkLevelHost>& lv, int i, int nb, int taps_one_n, size_t n_tau)
{
    AkLevelPlan pl;
    const int lw = lv[i].w, lh = lv[i].h;
    const size_t n = (size_t)lw * lh;
    // FED launches of this level.  Product: up to four steps per launch in registers (ak_fed_march_kernel: a wavefront marches a
    // strip of columns down the rows, every step level three rows deep in registers -- 12 bytes of HBM traffic per pixel and
    // LAUNCH instead of per step).  The older forms stay for the developer build's A/B runs: one step per launch
    // (R3DM_AK_FED_MARCH=0 R3DM_AK_FED_MULTI=0), four steps through LDS on the levels of <= 3.2 Mpx (R3DM_AK_FED_MARCH=0).
    static const int march_knob = r3dm_dev_knob("R3DM_AK_FED_MARCH", 1);      // 0 = never, 1 = every level, > 1 = levels of at least that many pixels
    // steps per launch: up to 4 on the large levels (a step there is bound by the arithmetic of its cells, more per pass only
    // widens the halo), up to 6 below 1 Mpx per image, where a launch is mostly its own latency and fewer launches is the gain
    static const int kmax_knob = r3dm_dev_knob("R3DM_AK_FED_KMAX", 0);
    const int march_kmax = kmax_knob > 0 ? std::min(6, kmax_knob) : (n < (size_t)1000000 ? 6 : 4);
    static const int march_waves = std::max(256, r3dm_dev_knob("R3DM_AK_FED_WAVES", 12000));
    const bool march = march_knob && lw >= 3 && lh >= 3 && (march_knob == 1 || n >= (size_t)march_knob);
    static const int multi_knob = r3dm_dev_knob("R3DM_AK_FED_MULTI", 1);      // developer build: 0 = never, 1 = the product, > 1 = that many pixels
    static const int multi_px = multi_knob > 1 ? multi_knob : (multi_knob ? 3200000 : 0);
    if (march) {
        const int q = ((int)n_tau + march_kmax - 1) / march_kmax;             // launches, steps spread evenly over them
        for (int m = 0; m < q; ++m) pl.steps.push_back(((int)n_tau * (m + 1)) / q - ((int)n_tau * m) / q);
    } else {
        const int per = n <= (size_t)multi_px ? 4 : 1;
        for (size_t k0 = 0; k0 < n_tau; k0 += (size_t)per) pl.steps.push_back((int)std::min<size_t>((size_t)per, n_tau - k0));
    }
    for (const int kn : pl.steps) {
        if (march) {
            // rows per band: enough wavefronts to fill the chip (strips x bands x images >= march_waves), at most 128 rows
            const int vw = 64 - 2 * kn, strips = (lw + vw - 1) / vw;
            int rows = (int)(((int64_t)lh * strips * nb + march_waves - 1) / march_waves);
            rows = std::max(16, std::min(128, (rows + 7) / 8 * 8));
            pl.form.push_back(AK_FED_MARCH); pl.rows.push_back(rows);
        } else {
            pl.form.push_back(kn == 1 && n > (size_t)multi_px ? AK_FED_STEP : AK_FED_MULTI); pl.rows.push_back(0);
        }
    }
    // Gaussian -> derivatives -> determinant -> conductivity.  Product: four HBM-bound launches (10 plane moves).  The one-pass form
    // (ak_level_head_kernel: a marching wavefront with the intermediates in LDS rings, 5 plane moves, bit-identical -- level_head.inc,
    // tests/cpp/level_head_emul.cpp) is built and MEASURED SLOWER, twice: 1,369 us (stages chained inside an iteration) and 1,573 us
    // (stages one iteration apart) against 1,083 us for the four launches at 8 x 12 Mpx.  PMC (profiles/r05_pmc_level_head.txt):
    // 271 scalar + 138 vector + 28 LDS instructions per 48 stored pixels -- the per-row bookkeeping of a marching wavefront
    // (ring slots, border rows, stage predicates) is paid once per 64 lanes and row, where a thread-per-pixel kernel pays it
    // once per four rows of loads; at ~620 G wave instructions/s the fused form is instruction-bound above the four launches'
    // HBM time.  It stays behind the developer knob R3DM_AK_HEAD=1 (tests/test_gpu_akaze.py runs it for bit-identity).
    static const int head_knob = r3dm_dev_knob("R3DM_AK_HEAD", 0);
    static const int head_waves = std::max(256, r3dm_dev_knob("R3DM_AK_HEAD_WAVES", 8000));
    const int s_i = lv[i].sigma_size;
    pl.head = head_knob && taps_one_n == 5 && s_i >= 2 && s_i <= 4 && lw >= 16 && lh >= 16;
    if (pl.head) {
        const int vw = 64 - 2 * (2 + 2 * s_i), strips = (lw + vw - 1) / vw;
        int rows = (int)(((int64_t)lh * strips * nb + head_waves - 1) / head_waves);
        pl.head_rows = std::max(32, std::min(256, (rows + 15) / 16 * 16));
    }
    return pl;
}

// level i > 0 from level i - 1: start image, conductivity, the FED cycle
// (Splitting the launches of the 3 Mpx octave into sub-batches whose planes fit the Infinity Cache was measured: 2.31-2.34 ms
// per image against 2.36 -- not worth a second launch order; profiles/r03_f_*.)
hipError_t ak_evolve_level(AkPass& p, int i)
{
    hipError_t e; hipStream_t st = p.st;
    const std::vector<AkLevelHost>& lv = p.lv;
    const int nb = p.iB, lw = lv[i].w, lh = lv[i].h;
    const size_t n = (size_t)lw * lh;
    const std::vector<float> tau = ak_fed_tau(lv[i].etime - lv[i - 1].etime);
    float* Lti = p.Lt(i);
    const AkLevelPlan pl = ak_level_plan(lv, i, nb, p.taps_one.n, tau.size());
    const size_t n_launch = pl.steps.size();                            // plane passes of the FED part (3 planes each): launches, not steps
    const float* start = nullptr;
    if (lv[i].octave > lv[i - 1].octave) {
        // the FED launches ping-pong between Lt(i) and the work image and must END in Lt(i): the half-sampled start image
        // goes to whichever of the two the first launch does not write
        float* half = (n_launch % 2 == 1) ? p.lt2 : Lti;
        const HalfTabs& ht = p.half_tabs[i];
        AK_TRY(ak_halfsample(st, p.Lt(i - 1), half, lv[i - 1].w, lv[i - 1].h, nb, ht.xt, ht.xb, ht.yt, ht.yb));
        start = half;
    } else {
        start = p.Lt(i - 1);                                        // same octave: the previous level IS the start image, no copy
    }
    if (tau.empty()) {                                              // (never for the reference's time steps) plain copy
        if (start != Lti) AK_TRY(hipMemcpyAsync(Lti, start, (size_t)nb * n * 4, hipMemcpyDeviceToDevice, st));
        start = Lti;
    }
    const int s_i = lv[i].sigma_size;
    if (pl.head) {
        AK_TRY(ak_level_head(st, start, p.Lx(i), p.Ly(i), p.Ldet(i), p.flow, lw, lh, nb, p.taps_one, s_i, p.inv_k2() + lv[i].octave, pl.head_rows));
    } else {
        AK_TRY(ak_gaussian(st, start, p.tmp, p.smooth, lw, lh, nb, p.taps_one));
        AK_TRY(ak_scaled_deriv_xy(st, p.smooth, p.Lx(i), p.Ly(i), lw, lh, nb, s_i));
        AK_TRY(ak_scaled_deriv_det(st, p.Lx(i), p.Ly(i), p.Ldet(i), lw, lh, nb, s_i));
        AK_TRY(ak_scharr_g2(st, p.smooth, p.flow, lw, lh, nb, p.inv_k2() + lv[i].octave));     // kcontrast * 0.75^octave
    }
    // Fast Explicit Diffusion: lt += lstep * 0.5 * tau_j; launch m of M writes Lt(i) when M - m is even, else the work image
    const float* cur = start;
    size_t k0 = 0;
    for (size_t m = 1; m <= n_launch; ++m) {
        float* o = ((n_launch - m) % 2 == 0) ? Lti : p.lt2;
        const int kn = pl.steps[m - 1];
        if (pl.form[m - 1] == AK_FED_MARCH) AK_TRY(ak_fed_march(st, cur, p.flow, o, lw, lh, nb, tau.data() + k0, kn, pl.rows[m - 1]));
        else if (pl.form[m - 1] == AK_FED_STEP) AK_TRY(ak_fed_step(st, cur, p.flow, o, lw, lh, nb, tau[k0]));
        else AK_TRY(ak_fed_multi(st, cur, p.flow, o, lw, lh, nb, tau.data() + k0, kn));
        cur = o; k0 += (size_t)kn;
    }
    if (lv[i].octave > lv[i - 1].octave) { p.tally(lv[i - 1].w, lv[i - 1].h, 1, 1); p.tally(lw, lh, 1, 1); }
    p.tally(lw, lh, (pl.head ? 5 : 2 + 6 + 2) + 3 * (int)n_launch, 2 + 1 + 1 + 2 * (int)tau.size());       // Gaussian (fused row + column pass) 2, derivatives + determinant 6, conductivity 2, 3 per FED launch (as structured); compulsory: 2 per FED step, the round-2 count
    return hipSuccess;
}

hipError_t ak_scale_space(AkPass& p)
{
    hipError_t e; hipStream_t st = p.st;
    const int w = p.w, h = p.h, iB = p.iB, nl = p.nl;
    // (the base level's smoothed image IS evolution level 0: written straight into Lt(0), no copy)
    AK_TRY(ak_gaussian(st, p.img, p.tmp, p.Lt(0), w, h, iB, p.taps_off)); p.tally(w, h, 2, 2);
    // Compute_Determinant_Hessian_Response_Single (AKAZEFeatures.cpp:389-410), two launches: smooth -> (Lx, Ly);  (Lx, Ly) -> Lxx, Lxy, Lyy on
    // the spot -> the determinant
    AK_TRY(ak_scaled_deriv_xy(st, p.Lt(0), p.Lx(0), p.Ly(0), w, h, iB, p.lv[0].sigma_size)); p.tally(w, h, 3 + 3, 1);
    AK_TRY(ak_scaled_deriv_det(st, p.Lx(0), p.Ly(0), p.Ldet(0), w, h, iB, p.lv[0].sigma_size));
    AK_TRY(hipMemsetAsync(p.small, 0, (size_t)p.B * 4096 * 4, st));
    const int nbins = 300;
    if (nl > 1) {
        AK_TRY(ak_gaussian(st, p.img, p.tmp, p.flow, w, h, iB, p.taps_one)); p.tally(w, h, 2, 1);
        // (the Scharr derivative images of the reference exist only inside these two kernels: DESIGN.md section 4.8)
        AK_TRY(ak_modg_max(st, p.flow, w, h, iB, p.hmax_bits())); p.tally(w, h, 1, 0);
        AK_TRY(ak_modg_hist(st, p.flow, w, h, iB, p.hmax_bits(), nbins, p.hist())); p.tally(w, h, 1, 0);
    }
    AK_TRY(ak_kcontrast(st, p.hmax_bits(), p.hist(), nbins, (uint32_t)((size_t)(w - 2) * (h - 2)), nl > 1 ? 1 : 0, p.inv_k2(), iB));
    for (int i = 1; i < nl; ++i) AK_TRY(ak_evolve_level(p, i));
    return hipSuccess;
}
#undef AK_TRY

// ---- phase 3: Feature_Detection (:371-382): extrema -> in-level pruning -> cross-level pruning -> refinement + orientation
struct AkDetection {
    size_t rows_total = 0, n_lv = 0;
    std::vector<AkLevelDev> ld;                  // [B][nl], uploaded to d_levels by every attempt
    AkLevelDev* d_levels = nullptr;
    AkBatchMeta* d_bmeta = nullptr;
    AkTileTable tiles;
    uint32_t n_tiles = 0;
    int max_rows = 0;
    uint64_t bound = 0;                          // candidates an image can hold at most
    uint32_t cap = 0;                            // slots per image of the attempt that fitted
    std::vector<AkBatchMeta> bm;
};

// the level table of every image, the extremum masks' places, the tiles of the count pass, the candidate bound
int ak_level_table(AkPass& p, AkDetection& d)
{
    r3dm_ctx* c = p.c; const std::vector<AkLevelHost>& lv = p.lv;
    const int nl = p.nl; const uint32_t B = p.B;
    d.ld.assign((size_t)nl * B, AkLevelDev{});
    size_t rows_img = 0;
    for (int i = 0; i < nl; ++i) rows_img += (size_t)std::max(0, lv[i].h - 2 * lv[i].border);
    d.rows_total = rows_img * B; d.n_lv = (size_t)nl * B;
    // row counts + row offsets, per-level counters (4 words), level table, per-image meta
    DevBuf& meta = p.tail(T_META);
    const size_t off_levels = ((d.rows_total * 8 + d.n_lv * 16 + 15) / 16) * 16;
    const size_t off_bmeta = off_levels + ((d.n_lv * sizeof(AkLevelDev) + 15) / 16) * 16;
    R3DM_HIP(c, meta.ensure(off_bmeta + (size_t)B * sizeof(AkBatchMeta) + 256));
    uint32_t* rc = meta.as<uint32_t>();
    uint32_t* cnt = rc + 2 * d.rows_total;
    d.d_levels = reinterpret_cast<AkLevelDev*>(meta.as<unsigned char>() + off_levels);
    d.d_bmeta = reinterpret_cast<AkBatchMeta*>(meta.as<unsigned char>() + off_bmeta);
    std::vector<size_t> mask_off(nl + 1, 0);                          // in 64-bit words, per level, inside an image's mask area
    for (int i = 0; i < nl; ++i)
        mask_off[i + 1] = mask_off[i] + (size_t)std::max(0, lv[i].h - 2 * lv[i].border) * (size_t)std::max(0, (lv[i].w - 2 * lv[i].border + 63) / 64);
    if (mask_off[nl] * 8 + 8 > p.n0 * 4) { c->err = "detector: extremum masks do not fit the work image"; return R3DM_ERR_HIP; }
    size_t ro = 0;
    for (uint32_t b = 0; b < B; ++b)
        for (int i = 0; i < nl; ++i) {
            AkLevelDev& L = d.ld[(size_t)b * nl + i];
            const size_t plane = (size_t)lv[i].w * lv[i].h;
            L.w = lv[i].w; L.h = lv[i].h; L.border = lv[i].border; L.ratio = lv[i].ratio; L.psize = lv[i].esigma * 1.5f;
            L.Ldet = p.Ldet(i) + b * plane; L.Lx = p.Lx(i) + b * plane; L.Ly = p.Ly(i) + b * plane; L.Lt = p.Lt(i) + b * plane;
            L.row_cnt = rc + ro; L.row_off = rc + d.rows_total + ro; L.counts = cnt + 4 * ((size_t)b * nl + i);
            // extremum bit masks: in the row-pass work image of the Gaussian (idle once the scale space is built), image b's
            // plane, the levels one after another (1 bit per pixel + at most 8 bytes per row: far below the plane's 4 bytes per pixel)
            const int rows_i = std::max(0, lv[i].h - 2 * lv[i].border);
            L.mask_words = (uint32_t)std::max(0, (lv[i].w - 2 * lv[i].border + 63) / 64);
            L.mask = reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(p.tmp) + (((size_t)b * p.n0 * 4 + 7) / 8) * 8) + mask_off[i];   // (8-byte aligned also when w h is odd)
            ro += (size_t)rows_i;
        }
    for (int i = 0; i < nl; ++i) d.max_rows = std::max(d.max_rows, lv[i].h - 2 * lv[i].border);
    // tiles of the extremum count pass: 64 columns x 64 rows of a level's interior (kernels_akaze.hip kAkMaskRows = 16 rows per wave), the levels one after another
    for (int i = 0; i < 17; ++i) d.tiles.begin[i] = 0xFFFFFFFFu;
    if (nl > 16) { c->err = "detector: more than 16 evolution levels"; return R3DM_ERR_UNSUPPORTED; }
    for (int i = 0; i < nl; ++i) {
        d.tiles.begin[i] = d.n_tiles;
        const int rows_i = std::max(0, lv[i].h - 2 * lv[i].border), words_i = std::max(0, (lv[i].w - 2 * lv[i].border + 63) / 64);
        d.n_tiles += (uint32_t)words_i * (uint32_t)((rows_i + 63) / 64);
    }
    // slot capacity per image: a strict 3x3 maximum excludes its eight neighbours, so a level holds at most ceil(w/2) ceil(h/2)
    // candidates; start from min(that bound, 256 k) and grow only if an image reports more (the bound itself never overflows)
    for (int i = 0; i < nl; ++i) d.bound += (uint64_t)((lv[i].w + 1) / 2) * (uint64_t)((lv[i].h + 1) / 2);
    return R3DM_OK;
}

// the tail of the detection on the pruned lists (counts[1] entries per level): the row spans of the list chunks, the lower- and the
// upper-level filter, refinement + orientation, the records.  The detector and the developer build's r3dm_dev_akaze_tail both call it.
hipError_t ak_tail_launches(hipStream_t st, const AkLevelDev* d_levels, int nl, int iB, AkKpRec* recs, uint32_t cap, AkBatchMeta* d_bmeta)
{
    hipError_t e;
    if ((e = ak_list_ranges(st, d_levels, nl, iB)) != hipSuccess) return e;
    if ((e = ak_cross(st, d_levels, nl, iB, 0)) != hipSuccess) return e;
    if ((e = ak_cross(st, d_levels, nl, iB, 1)) != hipSuccess) return e;
    if ((e = ak_refine(st, d_levels, nl, iB)) != hipSuccess) return e;
    return ak_compact(st, d_levels, nl, iB, recs, cap, d_bmeta);
}

// the head of the detection on the determinant planes of the level table: the extremum bit masks and row counts, their scan, the slot
// layout at `cap` slots per image, the raster-ordered candidates, the in-level pruning -- it leaves counts[0] candidates and the kept
// list of counts[1] entries per level.  The caller has zeroed the row counts and counters and uploaded the table.  The detector and the
// developer build's r3dm_dev_akaze_head / r3dm_dev_akaze_extrema both call it.
hipError_t ak_head_launches(hipStream_t st, AkLevelDev* d_levels, int nl, int iB, const AkTileTable& tiles, uint32_t n_tiles, int max_rows,
                            unsigned char* slots, uint32_t cap, AkBatchMeta* d_bmeta, float threshold)
{
    hipError_t e;
    const size_t field = (size_t)iB * cap;
    if ((e = ak_extrema_mask(st, d_levels, nl, iB, tiles, n_tiles, threshold)) != hipSuccess) return e;   // all levels of all images in one launch
    if ((e = ak_scan_rows(st, d_levels, nl, iB)) != hipSuccess) return e;
    if ((e = ak_layout(st, d_levels, nl, iB, slots, cap, d_bmeta)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(slots + field * 76, 0, field * 2, st)) != hipSuccess) return e;               // dead_lower / dead_upper flags
    if ((e = ak_extrema(st, d_levels, nl, iB, max_rows, threshold, 1)) != hipSuccess) return e;
    return ak_prune_levels(st, d_levels, nl, iB);
}

// the level table of a pass on the device, as every caller of the head or tail launches (and the developer M-SURF entry, cap 0) puts it
// there: the slot arrays -- with `with_recs` the record array too -- of `cap` slots per image, the row counts and counters cleared, d.ld
// at d.d_levels, in this order on the stream
int ak_table_upload(AkPass& p, AkDetection& d, uint32_t cap, bool with_recs)
{
    r3dm_ctx* c = p.c;
    const size_t field = (size_t)p.B * cap;
    R3DM_HIP(c, p.tail(T_SLOTS).ensure(field * kAkSlotBytes + 256));
    if (with_recs) R3DM_HIP(c, p.tail(T_RECS).ensure(field * sizeof(AkKpRec) + 256));
    R3DM_HIP(c, hipMemsetAsync(p.tail(T_META).p, 0, d.rows_total * 8 + d.n_lv * 16, p.st));
    R3DM_HIP(c, hipMemcpyAsync(d.d_levels, d.ld.data(), d.n_lv * sizeof(AkLevelDev), hipMemcpyHostToDevice, p.st));
    return R3DM_OK;
}

// the detection launches at a slot capacity; an image that reports more candidates than it makes them run again with larger arrays
int ak_detect_regrow(AkPass& p, AkDetection& d, float threshold)
{
    r3dm_ctx* c = p.c; hipStream_t st = p.st;
    const int nl = p.nl, iB = p.iB; const uint32_t B = p.B;
    // (R3DM_AK_CAP, developer build only: a tiny first capacity so that the tests reach the grow-and-repeat path)
    static const uint32_t cap0 = (uint32_t)std::max(1, r3dm_dev_knob("R3DM_AK_CAP", 1 << 18));
    uint32_t cap = (uint32_t)std::min<uint64_t>(d.bound, std::max<uint64_t>(c->ak_cap, cap0));
    d.bm.assign(B, AkBatchMeta{});
    DevBuf &slots = p.tail(T_SLOTS), &recs = p.tail(T_RECS);
    for (int attempt = 0;; ++attempt) {
        { const int urc = ak_table_upload(p, d, cap, true); if (urc != R3DM_OK) return urc; }
        R3DM_HIP(c, ak_head_launches(st, d.d_levels, nl, iB, d.tiles, d.n_tiles, d.max_rows, slots.as<unsigned char>(), cap, d.d_bmeta, threshold));
        R3DM_HIP(c, ak_tail_launches(st, d.d_levels, nl, iB, recs.as<AkKpRec>(), cap, d.d_bmeta));
        R3DM_HIP(c, hipEventRecord(c->ev1, st));
        R3DM_HIP(c, hipMemcpyAsync(d.bm.data(), d.d_bmeta, (size_t)B * sizeof(AkBatchMeta), hipMemcpyDeviceToHost, st));
        R3DM_HIP(c, hipStreamSynchronize(st));                                            // host visit 1 of 2: the counts
        uint32_t need = 0;
        for (uint32_t b = 0; b < B; ++b) if (d.bm[b].overflow) need = std::max(need, d.bm[b].need);
        if (!need) break;
        if (attempt >= 2 || need > d.bound) { c->err = "detector: candidate count exceeds its own bound"; return R3DM_ERR_HIP; }
        cap = (uint32_t)std::min<uint64_t>(d.bound, (uint64_t)need + need / 4 + 1024);       // grow and redo the detection phase (the scale space stays)
        c->feat_totals.n_regrows += 1;
    }
    d.cap = cap;
    c->ak_cap = cap;
    c->ak_n_levels = nl;
    c->ak_levels_dev = d.d_levels;
    return R3DM_OK;
}

// ---- phase 4: the records of every image
int ak_read_back(AkPass& p, const AkDetection& d, std::vector<std::vector<AkKpRec>>& out)
{
    r3dm_ctx* c = p.c; const AkKpRec* recs = p.tail(T_RECS).as<AkKpRec>();
    for (uint32_t b = 0; b < p.B; ++b) {
        out[b].resize(d.bm[b].n_kp);
        if (d.bm[b].n_kp) R3DM_HIP(c, hipMemcpyAsync(out[b].data(), recs + (size_t)b * d.cap, (size_t)d.bm[b].n_kp * sizeof(AkKpRec), hipMemcpyDeviceToHost, p.st));
    }
    R3DM_HIP(c, hipStreamSynchronize(p.st));                                              // host visit 2 of 2: the records
    return R3DM_OK;
}

}  // namespace

// Leaves the B gray images in ak_bufs[0] (B planes) for the LIOP patch extraction and the level images for MLDB.
static int ak_detect_batch_smax(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height,
                                float threshold, float smax, DetectedBatch& out)
{
    if (!detect_args_ok(c, B, images, bgrs, width, height)) return R3DM_ERR_INVALID;
    out = DetectedBatch();
    out.fast.assign(B, std::vector<AkKpRec>());
    if (width < 3 || height < 3) return R3DM_ERR_INVALID;
    R3DM_HIP(c, hipSetDevice(c->device));
    const double t_call = now_ms();
    out.fast_levels = ak_levels((int)width, (int)height, smax);
    out.fast_smax = smax;
    AkPass p{c, c->stream, B, (int)B, (int)width, (int)height, (int)out.fast_levels.size(), (size_t)width * height, out.fast_levels};
    c->stats.n_detect_images = B; c->stats.ms_detect_kernels = 0.0; c->stats.detect_algorithmic_bytes = 0.0; c->stats.detect_compulsory_bytes = 0.0;
    if (p.nl == 0) { c->stats.ms_detect = now_ms() - t_call; return R3DM_OK; }     // image too small for a single evolution level
    int rc = ak_buffers(p);
    out.grays_dev = p.img;                                  // (BGR: the bytes are staged in the not yet used work image tmp2)
    if (rc == R3DM_OK) rc = detect_upload(c, B, images, bgrs, p.n0, p.img, reinterpret_cast<unsigned char*>(p.tmp2));
    p.taps_off = ak_taps(1.6f); p.taps_one = ak_taps(1.0f);
    if (rc == R3DM_OK) rc = detect_area_tabs(c, p.tail(T_TABS), p.lv, p.half_tabs);
    if (rc != R3DM_OK) return rc;
    R3DM_HIP(c, hipEventRecord(c->ev0, p.st));
    R3DM_HIP(c, ak_scale_space(p));
    AkDetection d;
    rc = ak_level_table(p, d);
    if (rc == R3DM_OK) rc = ak_detect_regrow(p, d, threshold);
    if (rc == R3DM_OK) rc = ak_read_back(p, d, out.fast);
    if (rc != R3DM_OK) return rc;
    c->stats.detect_algorithmic_bytes = p.planes_px * 4.0 * B; c->stats.detect_compulsory_bytes = p.compulsory_px * 4.0 * B;
    uint64_t n_kp = 0;
    for (uint32_t b = 0; b < B; ++b) n_kp += d.bm[b].n_kp;
    detect_finish(c, B, t_call, n_kp, p.planes_px * 4.0 * B);
    return R3DM_OK;
}

// the two level tables as detect arms (detect_entry's shape): the detector's own, which LIOP and MLDB read, and that of the KAZE
// descriptors, which M-SURF-64 must be computed on
int ak_detect_batch(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height,
                    float threshold, DetectedBatch& out) { return ak_detect_batch_smax(c, B, images, bgrs, width, height, threshold, kAkSmaxDetector, out); }
int ak_detect_batch_msurf(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height,
                          float threshold, DetectedBatch& out) { return ak_detect_batch_smax(c, B, images, bgrs, width, height, threshold, kAkSmaxMsurf, out); }

// ======== the level-plane descriptors of the Fast arm: MLDB-486 and M-SURF-64 ("The descriptor arms")
// one keypoint of image b as either kernel takes it: the raw (radian) angle of the host libm, its cos / sin, level coordinates, and the
// level's sigma_size -- a float for MLDB, for M-SURF the reference's int scale (fRound(0.5 size / ratio), which is the level's sigma_size:
// size = 2 esigma derivative_factor and sigma_size = fRound(esigma derivative_factor / ratio)).  The two items stay as the kernels declare them.
template <class Item> static Item ak_item(uint32_t b, uint32_t nl, const std::vector<AkLevelHost>& lv, const AkKpRec& r, float* theta_out = nullptr)
{
    const float theta = ak_theta(r);
    if (theta_out) *theta_out = theta;
    return {b * nl + r.level, r.x / lv[r.level].ratio, r.y / lv[r.level].ratio, cosf(theta), sinf(theta), (decltype(Item::scale))lv[r.level].sigma_size};
}
constexpr size_t kAkItemBytes = 24;
static_assert(sizeof(AkMldbItem) == kAkItemBytes && sizeof(AkMsurfItem) == kAkItemBytes, "the level-plane items are 24 bytes each");

// comparison table of MLDB_Binary_Comparisons: per grid, per channel, all value pairs i < j
static std::vector<unsigned char> ak_mldb_pairs()
{
    std::vector<unsigned char> pairs;
    const int bases[3] = {0, 12, 39}, cnts[3] = {4, 9, 16};
    for (int g = 0; g < 3; ++g)
        for (int pos = 0; pos < 3; ++pos)
            for (int i = 0; i < cnts[g]; ++i)
                for (int j = i + 1; j < cnts[g]; ++j) { pairs.push_back((unsigned char)(bases[g] + 3 * i + pos)); pairs.push_back((unsigned char)(bases[g] + 3 * j + pos)); }
    return pairs;
}

// M-SURF's own refusals.  The kernel reads Lx / Ly up to 12 sqrt(2) sigma_size + 1 from a keypoint: only the level table cut with the
// arm's border keeps that inside the planes, a pass on any other is refused here.
static int ak_msurf_refuse(r3dm_ctx* c, const DescriptorArm& arm, const DetectedBatch& det)
{
    const std::vector<AkLevelHost>& lv = det.fast_levels;
    if (det.fast_smax != ak_smax(arm)) { c->err = "M-SURF: the detector pass ran on the MLDB level table, whose borders do not hold the descriptor's reads"; return R3DM_ERR_INVALID; }
    // (the in-plane argument at r3dm_dev_akaze_msurf_check counts on float positions below 2^16 and on sigma_size 2 .. 4)
    if (lv[0].w > 65536 || lv[0].h > 65536) { c->err = "M-SURF: images of more than 65536 columns or rows are not served"; return R3DM_ERR_UNSUPPORTED; }
    for (const AkLevelHost& e : lv) if (e.sigma_size < 2 || e.sigma_size > 4) { c->err = "M-SURF: unexpected level table"; return R3DM_ERR_UNSUPPORTED; }
    return R3DM_OK;
}

// what a level-plane arm adds to the one pass below: how an item is formed from a record, the bytes uploaded behind the items (null:
// none), its launcher, its own refusals (null: none), and the detect arm that cuts its level table
struct AkDescribeOps {
    int id; DetectArm* detect;
    void (*item)(void* at, uint32_t b, uint32_t nl, const std::vector<AkLevelHost>& lv, const AkKpRec& r);
    std::vector<unsigned char> (*extra)();
    hipError_t (*launch)(hipStream_t st, const AkLevelDev* levels, const void* items, uint32_t n, const unsigned char* extra, unsigned char* rows);
    int (*refuse)(r3dm_ctx* c, const DescriptorArm& arm, const DetectedBatch& det);
};
template <class Item> static void ak_item_at(void* at, uint32_t b, uint32_t nl, const std::vector<AkLevelHost>& lv, const AkKpRec& r)
{ const Item it = ak_item<Item>(b, nl, lv, r); memcpy(at, &it, sizeof it); }
static const AkDescribeOps kAkDescribeOps[] = {
    {R3DM_DESCRIPTOR_MLDB, ak_detect_batch, ak_item_at<AkMldbItem>, ak_mldb_pairs,
     [](hipStream_t st, const AkLevelDev* levels, const void* items, uint32_t n, const unsigned char* extra, unsigned char* rows) {
         return ak_mldb(st, levels, (const AkMldbItem*)items, n, extra, rows); }, nullptr},
    {R3DM_DESCRIPTOR_MSURF, ak_detect_batch_msurf, ak_item_at<AkMsurfItem>, nullptr,
     [](hipStream_t st, const AkLevelDev* levels, const void* items, uint32_t n, const unsigned char*, unsigned char* rows) {
         return ak_msurf(st, levels, (const AkMsurfItem*)items, n, reinterpret_cast<float*>(rows)); }, ak_msurf_refuse},
};
static const AkDescribeOps& ak_describe_ops(const DescriptorArm& arm)
{
    for (const AkDescribeOps& o : kAkDescribeOps) if (o.id == arm.id) return o;
    abort();                                                              // (a level-plane arm of the table without a row here)
}

// the launch of the arm's kernel over ni > 0 items (host memory) on the level table the context's last pass left on the device, which the
// caller vouches was cut for the arm: items and the arm's extra bytes up, one launch between ev0 / ev1, waited for (the caller's items may
// leave scope); *rows_dev: arm.row_bytes a row, 256-byte aligned (M-SURF's float4 stores need 16).  One buffer holds items, extra bytes, rows.
static int ak_describe_launch(r3dm_ctx* c, const DescriptorArm& arm, const void* items, size_t ni, const unsigned char** rows_dev)
{
    const AkDescribeOps& ops = ak_describe_ops(arm);
    const std::vector<unsigned char> extra = ops.extra ? ops.extra() : std::vector<unsigned char>();
    hipStream_t st = c->stream;
    DevBuf& mb = c->ak_bufs[c->ak_bufs.size() - T_COUNT + T_DESC];
    const size_t off_extra = ni * kAkItemBytes, off_rows = (off_extra + extra.size() + 255) / 256 * 256;
    R3DM_HIP(c, mb.ensure(off_rows + ni * arm.row_bytes + 64));
    unsigned char* base = mb.as<unsigned char>();
    R3DM_HIP(c, hipMemcpyAsync(base, items, ni * kAkItemBytes, hipMemcpyHostToDevice, st));
    if (!extra.empty()) R3DM_HIP(c, hipMemcpyAsync(base + off_extra, extra.data(), extra.size(), hipMemcpyHostToDevice, st));
    R3DM_HIP(c, hipEventRecord(c->ev0, st));
    R3DM_HIP(c, ops.launch(st, c->ak_levels_dev, base, (uint32_t)ni, base + off_extra, base + off_rows));
    R3DM_HIP(c, hipEventRecord(c->ev1, st));
    R3DM_HIP(c, hipStreamSynchronize(st));                                // the items and `extra` may leave scope
    *rows_dev = base + off_rows;
    return R3DM_OK;
}

// Get_MLDB_Full_Descriptor / Get_MSURF_Descriptor_64 of the first min(count, cap) keypoints of every image of the pass, in ONE launch:
// level coordinates, cos / sin of the raw (radian) angle (host libm, as the oracle and the LIOP patch map: device trigonometry is not
// bit-equal to it).  An item names its level as image * n_levels + level: the level table the detector left on the device (ak_levels_dev)
// and the Lt / Lx / Ly planes of its work buffers cover the B images of the pass until the next pass.  The rows of image b follow those of
// image b - 1, arm.row_bytes apart -- the layout r3dm_set_image(arm.dim, arm.dtype) reads from a device pointer, so a consumer on the
// device takes image b's rows where the kernel stored them, at rows_dev + arm.row_bytes first[b]; nothing is copied.  first (B + 1
// entries): row offsets per image.  rows_dev stays valid until this context's next detector or descriptor pass.
// host_team: the threads that share the item loop (three libm calls per keypoint: 229 k keypoints of eight 12 Mpx images on one thread
// took longer than the detector's kernels), in chunks of 4,096 keypoints over all images as the features batch forms its angles.
int ak_describe_pass(r3dm_ctx* c, const DescriptorArm& arm, const DetectedBatch& det, uint32_t cap, int host_team, std::vector<size_t>& first,
                     const unsigned char** rows_dev)
{
    const AkDescribeOps& ops = ak_describe_ops(arm);
    const uint32_t B = (uint32_t)det.fast.size();
    const std::vector<AkLevelHost>& lv = det.fast_levels;
    const uint32_t nl = (uint32_t)lv.size();
    first.assign((size_t)B + 1, 0);
    for (uint32_t b = 0; b < B; ++b) first[b + 1] = first[b] + std::min<size_t>(det.fast[b].size(), cap);
    *rows_dev = nullptr;
    const size_t ni = first[B];
    if (ni == 0) return R3DM_OK;
    if (ops.refuse) { const int rrc = ops.refuse(c, arm, det); if (rrc != R3DM_OK) return rrc; }
    if (ni >= (1ull << 31)) { c->err = std::string(arm.tag) + ": more than 2^31 keypoints in one pass"; return R3DM_ERR_UNSUPPORTED; }
    std::vector<unsigned char> items(ni * kAkItemBytes);
    struct Chunk { uint32_t b; size_t k0, k1; };
    std::vector<Chunk> chunks;
    for (uint32_t b = 0; b < B; ++b)
        for (size_t k0 = 0, nk = first[b + 1] - first[b]; k0 < nk; k0 += 4096) chunks.push_back({b, k0, std::min(nk, k0 + 4096)});
    r3dm_parallel_for((long)chunks.size(), host_team, [&](long ci) {
        const Chunk& ch = chunks[(size_t)ci];
        const std::vector<AkKpRec>& recs = det.fast[ch.b];
        for (size_t k = ch.k0; k < ch.k1; ++k) ops.item(items.data() + (first[ch.b] + k) * kAkItemBytes, ch.b, nl, lv, recs[k]);
    });
    return ak_describe_launch(c, arm, items.data(), ni, rows_dev);
}

// the detect entry of the describing forms: the keypoints through detect_entry on the arm's level table, then min(count, cap) rows per
// image from the one pass; on failure every count reads 0
static int ak_describe_entry(r3dm_ctx* c, const DescriptorArm& arm, bool single, uint32_t B, const float* const* images, uint32_t width, uint32_t height,
                             float threshold, float* const* keypoints_out, void* const* descriptors_out, uint32_t cap, uint32_t* n_out)
{
    if (cap && !descriptors_out) return R3DM_ERR_INVALID;
    if (cap && images && B <= 4096) for (uint32_t b = 0; b < B; ++b) if (!descriptors_out[b] || (keypoints_out && !keypoints_out[b])) return R3DM_ERR_INVALID;
    DetectedBatch det;
    int rc = detect_entry(c, ak_describe_ops(arm).detect, single, B, images, width, height, threshold, keypoints_out, nullptr, cap, n_out, det);
    if (rc != R3DM_OK) return rc;
    std::vector<size_t> first;
    const unsigned char* rows = nullptr;
    rc = ak_describe_pass(c, arm, det, cap, r3dm_host_team(8), first, &rows);
    const auto lost = [&]() { c->err = std::string(arm.tag) + ": the descriptors did not reach the host"; rc = R3DM_ERR_HIP; };
    for (uint32_t b = 0; rc == R3DM_OK && b < B; ++b) {
        const size_t nb = first[b + 1] - first[b];
        if (nb && hipMemcpyAsync(descriptors_out[b], rows + arm.row_bytes * first[b], nb * arm.row_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) lost();
    }
    if (rc == R3DM_OK && hipStreamSynchronize(c->stream) != hipSuccess) lost();
    if (rc != R3DM_OK) for (uint32_t b = 0; b < B; ++b) n_out[b] = 0;
    return rc;
}
static const DescriptorArm& kArmMldb = *descriptor_arm_by_id(R3DM_DESCRIPTOR_MLDB);
static const DescriptorArm& kArmMsurf = *descriptor_arm_by_id(R3DM_DESCRIPTOR_MSURF);

extern "C" int r3dm_detect_akaze(r3dm_ctx* c, const float* image, uint32_t width, uint32_t height, float threshold,
                                 float* keypoints_out, float* responses_out, uint32_t cap, uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        DetectedBatch det;
        return detect_entry(c, ak_detect_batch, true, 1, &image, width, height, threshold, &keypoints_out, &responses_out, cap, n_out, det);
    });
}

extern "C" int r3dm_detect_akaze_mldb(r3dm_ctx* c, const float* image, uint32_t width, uint32_t height, float threshold,
                                      float* keypoints_out, unsigned char* descriptors_out, uint32_t cap, uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        return ak_describe_entry(c, kArmMldb, true, 1, &image, width, height, threshold, &keypoints_out, (void* const*)&descriptors_out, cap, n_out);
    });
}

// B same-size images in one pass of the detector, then one MLDB launch over the keypoints of all of them.  descriptors_out[b]: cap x 61
// bytes; min(count, cap) rows are written per image, n_out[b] reports the count.
extern "C" int r3dm_detect_akaze_mldb_batch(r3dm_ctx* c, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                                            float threshold, float* const* keypoints_out, unsigned char* const* descriptors_out, uint32_t cap,
                                            uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        return ak_describe_entry(c, kArmMldb, false, n_images, images, width, height, threshold, keypoints_out, (void* const*)descriptors_out, cap, n_out);
    });
}

// Fast-A-KAZE keypoints with their M-SURF-64 rows: the detector runs on the level table of the KAZE descriptors (ak_levels), so near
// the frame and on small images the keypoints are not those of r3dm_detect_akaze.  descriptors_out: cap x 64 floats.
extern "C" int r3dm_detect_akaze_msurf(r3dm_ctx* c, const float* image, uint32_t width, uint32_t height, float threshold,
                                       float* keypoints_out, float* descriptors_out, uint32_t cap, uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        return ak_describe_entry(c, kArmMsurf, true, 1, &image, width, height, threshold, &keypoints_out, (void* const*)&descriptors_out, cap, n_out);
    });
}

extern "C" int r3dm_detect_akaze_msurf_batch(r3dm_ctx* c, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                                             float threshold, float* const* keypoints_out, float* const* descriptors_out, uint32_t cap,
                                             uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        return ak_describe_entry(c, kArmMsurf, false, n_images, images, width, height, threshold, keypoints_out, (void* const*)descriptors_out, cap, n_out);
    });
}

// B same-size images in one pass of the detector.  keypoints_out[b]: cap x 4 floats (x, y, size, angle in degrees),
// responses_out (optional, entries optional): cap floats, n_out[b] = number detected (may exceed cap).
extern "C" int r3dm_detect_akaze_batch(r3dm_ctx* c, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                                       float threshold, float* const* keypoints_out, float* const* responses_out, uint32_t cap,
                                       uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        DetectedBatch det;
        return detect_entry(c, ak_detect_batch, false, n_images, images, width, height, threshold, keypoints_out, responses_out, cap, n_out, det);
    });
}

#ifdef R3DM_DEVTOOLS
// ---- developer build only (libr3dm_dev.so; declared in no header): the Fast arm's tail on a caller's level planes and pruned lists, so
// that the suite can put to the kernels what images hardly produce (a sample at exactly 360 degrees, windows of equal norm, a singular
// Hessian, a shift of exactly 1, equal responses across levels, unsorted lists, more than 256 killer chunks, tied MLDB cells, a keypoint
// on the border at 45 degrees).  What runs is the product's: ak_levels, ak_buffers, ak_level_table, ak_layout,
// ak_table_upload, ak_tail_launches, ak_item / ak_mldb_pairs / ak_describe_pass above.
struct r3dm_dev_ak_level { int32_t w, h, border, sigma_size; float ratio, esigma, psize; };
constexpr uint32_t kAkDevMaxB = 64, kAkDevMaxList = 1u << 20;

// the level table the product forms for a width x height image under a border factor: n_levels <= 16 entries
static int ak_dev_levels(uint32_t width, uint32_t height, float smax, r3dm_dev_ak_level* out, uint32_t* n_levels)
{
    if (!out || !n_levels || width < 3 || height < 3 || width > 65536u || height > 65536u) return R3DM_ERR_INVALID;
    const std::vector<AkLevelHost> lv = ak_levels((int)width, (int)height, smax);
    if (lv.size() > 16) return R3DM_ERR_UNSUPPORTED;
    for (size_t i = 0; i < lv.size(); ++i) out[i] = {lv[i].w, lv[i].h, lv[i].border, lv[i].sigma_size, lv[i].ratio, lv[i].esigma, lv[i].esigma * 1.5f};
    *n_levels = (uint32_t)lv.size();
    return R3DM_OK;
}
// (the detector's table; r3dm_dev_akaze_msurf_levels below gives that of the KAZE descriptors)
extern "C" int r3dm_dev_akaze_tail_levels(uint32_t width, uint32_t height, r3dm_dev_ak_level* out, uint32_t* n_levels) { return ak_dev_levels(width, height, kAkSmaxDetector, out, n_levels); }

// what the _check entries below share: (width, height) has a level table under `smax` of 1 .. 16 levels (-> lv), n_levels and plane_dims
// [n_levels][2] agree with it, and planes [B][n_levels][per] are non-null with every value finite
static bool ak_dev_planes_ok(uint32_t width, uint32_t height, float smax, uint32_t B, uint32_t n_levels, const uint32_t* plane_dims,
                             const float* const* planes, uint32_t per, std::vector<AkLevelHost>& lv)
{
    if (!plane_dims || !planes || width < 3 || height < 3 || width > 65536u || height > 65536u) return false;
    lv = ak_levels((int)width, (int)height, smax);
    const uint32_t nl = (uint32_t)lv.size();
    if (nl < 1 || nl > 16 || n_levels != nl) return false;
    for (uint32_t i = 0; i < nl; ++i) if (plane_dims[2 * i] != (uint32_t)lv[i].w || plane_dims[2 * i + 1] != (uint32_t)lv[i].h) return false;
    for (uint32_t b = 0; b < B; ++b)
        for (uint32_t i = 0; i < nl; ++i)
            for (uint32_t q = 0; q < per; ++q) {
                const float* P = planes[((size_t)b * nl + i) * per + q];
                if (!P) return false;
                for (size_t k = 0, plane = (size_t)lv[i].w * lv[i].h; k < plane; ++k) if (!std::isfinite(P[k])) return false;
            }
    return true;
}

// What the kernels would mis-read is refused here, before anything touches a device (c may be null): R3DM_OK or R3DM_ERR_INVALID.
//   n_levels and plane_dims [n_levels][2] (w, h of the planes the caller holds) are the table's of (width, height); 1 <= B <= 64
//   planes [B][n_levels][4]: Ldet, Lx, Ly, Lt, every value finite (a NaN gradient gives a NaN angle and a garbage slice key into LDS)
//   n_list [B][n_levels] <= 2^20 each; lists: the (x, y, response) triples of image 0's levels, then image 1's, ...: response finite,
//   x = column ratio and y = row ratio for integers column in [border, w - border), row in [border, h - border) of the entry's level.
//   Positions may repeat, lists need no order, entries need not be extrema of Ldet.
// Why every read of an accepted input stays inside its plane (s = sigma_size, border = fRound(10 sqrt 2 s) + 1 >= 15):
//   the cross-level filter reads the lists only;
//   the refinement reads Ldet at column +- 1, row +- 1, and moves the position by at most 1 in level coordinates (a larger shift drops
//   the entry; ratio is a power of two, so position / ratio is exact and rounds to within column +- 1, row +- 1);
//   the orientation reads Lx, Ly at the rounded position +- 5 s (i, j in -6 .. 6 with i i + j j < 36, step fRound(size / 2 / ratio) = s):
//   5 s + 1 < border;
//   MLDB reads at fRound(position + o) with |o| <= 10 sqrt 2 s (l, k in -10 .. 10, |l cos + k sin| <= 10 (|cos| + |sin|)) and position
//   >= border - 1 = fRound(10 sqrt 2 s): position - 10 sqrt 2 s > -0.5, which rounds half up (and truncates) to 0 or more; on the far
//   side position <= dim - border = dim - 1 - fRound(10 sqrt 2 s), so position + 10 sqrt 2 s < dim - 0.5, which rounds to dim - 1 at most.
extern "C" int r3dm_dev_akaze_tail_check(uint32_t width, uint32_t height, uint32_t B, uint32_t n_levels, const uint32_t* plane_dims,
                                         const float* const* planes, const uint32_t* n_list, const float* lists)
{
    std::vector<AkLevelHost> lv;
    if (!n_list || B < 1 || B > kAkDevMaxB || !ak_dev_planes_ok(width, height, kAkSmaxDetector, B, n_levels, plane_dims, planes, 4, lv)) return R3DM_ERR_INVALID;
    const uint32_t nl = (uint32_t)lv.size();
    size_t at = 0;
    for (uint32_t b = 0; b < B; ++b)
        for (uint32_t i = 0; i < nl; ++i) {
            const AkLevelHost& e = lv[i];
            const uint32_t n = n_list[(size_t)b * nl + i];
            if (n > kAkDevMaxList || (n && !lists)) return R3DM_ERR_INVALID;
            for (uint32_t k = 0; k < n; ++k) {
                const float* t = lists + 3 * (at + k);
                if (!std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2])) return R3DM_ERR_INVALID;
                const float col = t[0] / e.ratio, row = t[1] / e.ratio;
                if (col != floorf(col) || row != floorf(row) || col * e.ratio != t[0] || row * e.ratio != t[1]) return R3DM_ERR_INVALID;
                if (col < (float)e.border || col >= (float)(e.w - e.border) || row < (float)e.border || row >= (float)(e.h - e.border)) return R3DM_ERR_INVALID;
            }
            at += n;
        }
    return R3DM_OK;
}

// Runs the lists through the product's tail.  The list lengths stand in for the candidate counts, so that the product's own layout
// kernel places the slot arrays; the lists are then copied to where it put them and counts[1] says how long they are -- the state the
// in-level pruning leaves.  Outputs: n_kp [B]; per image, at the offset of its lists (the sum of the list lengths of the images
// before it; an image has at most as many keypoints as list entries): recs_out (AkKpRec, 32 bytes), angles_out (theta, cos, sin as
// ak_item forms them), desc_out (61 bytes a row, from ak_describe_pass); dead_out: (dead_lower, dead_upper) of every list entry.
extern "C" int r3dm_dev_akaze_tail(r3dm_ctx* c, uint32_t width, uint32_t height, uint32_t B, uint32_t n_levels, const uint32_t* plane_dims,
                                   const float* const* planes, const uint32_t* n_list, const float* lists,
                                   uint32_t* n_kp, AkKpRec* recs_out, float* angles_out, unsigned char* desc_out, unsigned char* dead_out)
{
    const int vrc = r3dm_dev_akaze_tail_check(width, height, B, n_levels, plane_dims, planes, n_list, lists);
    if (vrc != R3DM_OK) { if (c) c->err = "r3dm_dev_akaze_tail: planes or lists the kernels would mis-read"; return vrc; }
    if (!c || !n_kp) return R3DM_ERR_INVALID;
    std::vector<size_t> first_entry((size_t)B + 1, 0);
    for (uint32_t b = 0; b < B; ++b) {
        size_t t = 0;
        for (uint32_t i = 0; i < n_levels; ++i) t += n_list[(size_t)b * n_levels + i];
        first_entry[b + 1] = first_entry[b] + t;
    }
    if (first_entry[B] && (!recs_out || !angles_out || !desc_out || !dead_out)) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int {
        R3DM_HIP(c, hipSetDevice(c->device));
        DetectedBatch det;
        det.fast.assign(B, std::vector<AkKpRec>());
        det.fast_levels = ak_levels((int)width, (int)height);
        const std::vector<AkLevelHost>& lv = det.fast_levels;
        const int nl = (int)lv.size();
        AkPass p{c, c->stream, B, (int)B, (int)width, (int)height, nl, (size_t)width * height, lv};
        hipStream_t st = p.st;
        int rc = ak_buffers(p);
        if (rc != R3DM_OK) return rc;
        for (uint32_t b = 0; b < B; ++b)
            for (int i = 0; i < nl; ++i) {
                const size_t plane = (size_t)lv[i].w * lv[i].h;
                const float* const* P = planes + ((size_t)b * nl + i) * 4;
                R3DM_HIP(c, hipMemcpyAsync(p.Ldet(i) + b * plane, P[0], plane * 4, hipMemcpyHostToDevice, st));
                R3DM_HIP(c, hipMemcpyAsync(p.Lx(i) + b * plane, P[1], plane * 4, hipMemcpyHostToDevice, st));
                R3DM_HIP(c, hipMemcpyAsync(p.Ly(i) + b * plane, P[2], plane * 4, hipMemcpyHostToDevice, st));
                R3DM_HIP(c, hipMemcpyAsync(p.Lt(i) + b * plane, P[3], plane * 4, hipMemcpyHostToDevice, st));
            }
        AkDetection d;
        if ((rc = ak_level_table(p, d)) != R3DM_OK) return rc;
        uint32_t cap = 1;
        for (uint32_t b = 0; b < B; ++b) cap = std::max<uint32_t>(cap, (uint32_t)(first_entry[b + 1] - first_entry[b]));
        if ((rc = ak_table_upload(p, d, cap, true)) != R3DM_OK) return rc;
        DevBuf &slots = p.tail(T_SLOTS), &recs = p.tail(T_RECS);
        const size_t field = (size_t)B * cap;
        std::vector<uint32_t> cnt(4 * d.n_lv, 0u);                       // counts of level k = image * nl + level: [0] candidates, [1] list entries
        for (size_t k = 0; k < d.n_lv; ++k) cnt[4 * k] = cnt[4 * k + 1] = n_list[k];
        R3DM_HIP(c, hipMemcpyAsync(d.ld[0].counts, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice, st));
        R3DM_HIP(c, ak_layout(st, d.d_levels, nl, (int)B, slots.as<unsigned char>(), cap, d.d_bmeta));
        R3DM_HIP(c, hipMemsetAsync(slots.as<unsigned char>() + field * 76, 0, field * 2, st));   // dead_lower / dead_upper flags, as the detector clears them
        std::vector<AkLevelDev> dl(d.n_lv);
        R3DM_HIP(c, hipMemcpyAsync(dl.data(), d.d_levels, d.n_lv * sizeof(AkLevelDev), hipMemcpyDeviceToHost, st));
        R3DM_HIP(c, hipStreamSynchronize(st));
        std::vector<float> l4(4 * std::max<size_t>(first_entry[B], 1), 0.0f);       // the lists as the kernels read them: (x, y, response, -)
        for (size_t k = 0; k < first_entry[B]; ++k) { l4[4 * k] = lists[3 * k]; l4[4 * k + 1] = lists[3 * k + 1]; l4[4 * k + 2] = lists[3 * k + 2]; }
        size_t at = 0;
        for (size_t k = 0; k < d.n_lv; ++k) {
            if (n_list[k]) R3DM_HIP(c, hipMemcpyAsync(dl[k].list, l4.data() + 4 * at, (size_t)n_list[k] * 16, hipMemcpyHostToDevice, st));
            at += n_list[k];
        }
        R3DM_HIP(c, ak_tail_launches(st, d.d_levels, nl, (int)B, recs.as<AkKpRec>(), cap, d.d_bmeta));
        d.bm.assign(B, AkBatchMeta{});
        R3DM_HIP(c, hipMemcpyAsync(d.bm.data(), d.d_bmeta, (size_t)B * sizeof(AkBatchMeta), hipMemcpyDeviceToHost, st));
        // (the two flag arrays of a level are n_list[k] bytes each; they go out interleaved per entry)
        std::vector<unsigned char> fl(2 * std::max<size_t>(first_entry[B], 1), 0);
        at = 0;
        for (size_t k = 0; k < d.n_lv; ++k) {
            if (n_list[k]) {
                R3DM_HIP(c, hipMemcpyAsync(fl.data() + at, dl[k].dead_lower, n_list[k], hipMemcpyDeviceToHost, st));
                R3DM_HIP(c, hipMemcpyAsync(fl.data() + first_entry[B] + at, dl[k].dead_upper, n_list[k], hipMemcpyDeviceToHost, st));
            }
            at += n_list[k];
        }
        R3DM_HIP(c, hipStreamSynchronize(st));
        for (size_t k = 0; k < first_entry[B]; ++k) { dead_out[2 * k] = fl[k]; dead_out[2 * k + 1] = fl[first_entry[B] + k]; }
        for (uint32_t b = 0; b < B; ++b) {
            if (d.bm[b].overflow || d.bm[b].n_kp > first_entry[b + 1] - first_entry[b]) { c->err = "r3dm_dev_akaze_tail: more keypoints than list entries"; return R3DM_ERR_INVALID; }
            n_kp[b] = d.bm[b].n_kp;
        }
        d.cap = cap;
        if ((rc = ak_read_back(p, d, det.fast)) != R3DM_OK) return rc;
        c->ak_n_levels = nl;
        c->ak_levels_dev = d.d_levels;                                   // what the detector leaves for the MLDB pass
        std::vector<size_t> first;
        const unsigned char* rows = nullptr;
        if ((rc = ak_describe_pass(c, kArmMldb, det, 0xFFFFFFFFu, 1, first, &rows)) != R3DM_OK) return rc;
        for (uint32_t b = 0; b < B; ++b) {
            const size_t n = det.fast[b].size(), o = first_entry[b];
            for (size_t k = 0; k < n; ++k) {
                recs_out[o + k] = det.fast[b][k];
                float theta = 0.0f;
                const AkMldbItem it = ak_item<AkMldbItem>(b, (uint32_t)nl, lv, det.fast[b][k], &theta);
                angles_out[3 * (o + k)] = theta; angles_out[3 * (o + k) + 1] = it.co; angles_out[3 * (o + k) + 2] = it.si;
            }
            if (n) R3DM_HIP(c, hipMemcpyAsync(desc_out + 61 * o, rows + 61 * first[b], n * 61, hipMemcpyDeviceToHost, st));
        }
        R3DM_HIP(c, hipStreamSynchronize(st));
        return R3DM_OK;
    });
}

// ---- developer build only: the M-SURF-64 kernel on a caller's Lx / Ly planes of ONE image size and a caller's items, so that the suite
// can put keypoints on the border at the reach extremes, samples on .5 boundaries, windows without gradient.
// What runs is the product's: ak_levels with the M-SURF border, ak_buffers, ak_level_table, ak_table_upload, ak_describe_launch.
// The level table of the KAZE descriptors for a width x height image, as r3dm_dev_akaze_tail_levels gives the other one.
extern "C" int r3dm_dev_akaze_msurf_levels(uint32_t width, uint32_t height, r3dm_dev_ak_level* out, uint32_t* n_levels) { return ak_dev_levels(width, height, kAkSmaxMsurf, out, n_levels); }

// What the kernel would mis-read is refused here, before anything touches a device: R3DM_OK or R3DM_ERR_INVALID.
//   n_levels and plane_dims [n_levels][2] are the M-SURF table's of (width, height); planes [n_levels][2]: Lx, Ly, every value finite;
//   n <= 2^20 items: level < n_levels, scale == the level's sigma_size, xf in [border - 1, w - border] and yf in [border - 1, h - border]
//   of that level (the range the detector's refinement leaves, r3dm_dev_akaze_tail_check), |co^2 + si^2 - 1| <= 1e-6.
// Why every read of an accepted item stays inside its plane (s = sigma_size, which the table holds as 2, 3 or 4; R = 12 sqrt(2) s;
// border = fRound(R) + 1 with fRound(R) - R = 0.059, 0.088, 0.118 for these s):
//   a sample lies at position + (l s co + k s si) resp. + (-l s si + k s co) with k, l in [-12, 11], so |sample - position| <=
//   12 s (|co| + |si|) <= R (1 + 1e-6), and the float sum position + offset adds half an ulp of the position: <= 0.004 for planes of at
//   most 65536 columns and rows, which the check and ak_msurf_refuse hold to (together: e < 5e-3);
//   the rows read are y1 = (int)(sample - 0.5 + 0.5) and y2 = (int)(sample + 0.5 + 0.5), columns alike.  position >= border - 1 =
//   fRound(R) gives sample >= fRound(R) - R - e > 0.05, so y1 >= 0 (and y1 <= y2); position <= dim - border = dim - 1 - fRound(R)
//   gives sample + 1 <= dim - (fRound(R) - R) + e < dim - 0.05, so y2 <= dim - 1.
//   On the MLDB table (border from 10 sqrt(2) s) the same keypoints reach 2 sqrt(2) s beyond the plane: ak_msurf_refuse (ak_describe_pass) refuses it.
extern "C" int r3dm_dev_akaze_msurf_check(uint32_t width, uint32_t height, uint32_t n_levels, const uint32_t* plane_dims, const float* const* planes,
                                          uint32_t n, const AkMsurfItem* items)
{
    std::vector<AkLevelHost> lv;
    if ((n && !items) || n > kAkDevMaxList || !ak_dev_planes_ok(width, height, kAkSmaxMsurf, 1, n_levels, plane_dims, planes, 2, lv)) return R3DM_ERR_INVALID;
    const uint32_t nl = (uint32_t)lv.size();
    for (const AkLevelHost& e : lv) if (e.sigma_size < 2 || e.sigma_size > 4) return R3DM_ERR_INVALID;     // (the in-plane argument above)
    for (uint32_t k = 0; k < n; ++k) {
        const AkMsurfItem& it = items[k];
        if (it.level >= nl) return R3DM_ERR_INVALID;
        const AkLevelHost& e = lv[it.level];
        if (it.scale != e.sigma_size) return R3DM_ERR_INVALID;
        if (!std::isfinite(it.xf) || !std::isfinite(it.yf) || !std::isfinite(it.co) || !std::isfinite(it.si)) return R3DM_ERR_INVALID;
        if (it.xf < (float)(e.border - 1) || it.xf > (float)(e.w - e.border) || it.yf < (float)(e.border - 1) || it.yf > (float)(e.h - e.border)) return R3DM_ERR_INVALID;
        if (fabs((double)it.co * it.co + (double)it.si * it.si - 1.0) > 1e-6) return R3DM_ERR_INVALID;
    }
    return R3DM_OK;
}

// Runs the items through the product's kernel: rows_out = n x 64 floats.
extern "C" int r3dm_dev_akaze_msurf(r3dm_ctx* c, uint32_t width, uint32_t height, uint32_t n_levels, const uint32_t* plane_dims, const float* const* planes,
                                    uint32_t n, const AkMsurfItem* items, float* rows_out)
{
    const int vrc = r3dm_dev_akaze_msurf_check(width, height, n_levels, plane_dims, planes, n, items);
    if (vrc != R3DM_OK) { if (c) c->err = "r3dm_dev_akaze_msurf: planes or items the kernel would mis-read"; return vrc; }
    if (!c || (n && !rows_out)) return R3DM_ERR_INVALID;
    if (n == 0) return R3DM_OK;
    return r3dm_guarded(c, [&]() -> int {
        R3DM_HIP(c, hipSetDevice(c->device));
        const std::vector<AkLevelHost> lv = ak_levels((int)width, (int)height, kAkSmaxMsurf);
        const int nl = (int)lv.size();
        AkPass p{c, c->stream, 1, 1, (int)width, (int)height, nl, (size_t)width * height, lv};
        int rc = ak_buffers(p);
        if (rc != R3DM_OK) return rc;
        for (int i = 0; i < nl; ++i) {
            const size_t plane = (size_t)lv[i].w * lv[i].h;
            R3DM_HIP(c, hipMemcpyAsync(p.Lx(i), planes[2 * i], plane * 4, hipMemcpyHostToDevice, p.st));
            R3DM_HIP(c, hipMemcpyAsync(p.Ly(i), planes[2 * i + 1], plane * 4, hipMemcpyHostToDevice, p.st));
        }
        AkDetection d;
        if ((rc = ak_level_table(p, d)) != R3DM_OK || (rc = ak_table_upload(p, d, 0, false)) != R3DM_OK) return rc;
        R3DM_HIP(c, hipStreamSynchronize(p.st));
        c->ak_n_levels = nl;
        c->ak_levels_dev = d.d_levels;
        const unsigned char* rows = nullptr;
        if ((rc = ak_describe_launch(c, kArmMsurf, items, n, &rows)) != R3DM_OK) return rc;
        R3DM_HIP(c, hipMemcpy(rows_out, rows, (size_t)n * 256, hipMemcpyDeviceToHost));
        return R3DM_OK;
    });
}

// ---- developer build only: the Fast arm's HEAD, every plane and list read back, so that the suite can hold each pixel of each level
// to the oracle -- the border rings no keypoint can lie in, the last level's Lt, the k-contrast's branches, the seams of the extremum
// pass and of the FED launches, the in-level pruning before the cross-level filters hide it.  What runs is the
// product's: ak_levels, ak_buffers, detect_upload, detect_area_tabs, ak_scale_space (with the launch forms the developer knobs choose),
// ak_level_table, ak_head_launches.  The slot capacity is the level table's own bound, so nothing regrows.
// a level's launch plan as it crosses the ABI (AkLevelPlan): form 0 = one step per launch, 1 = steps through LDS, 2 = marching strips
struct r3dm_dev_ak_plan { int32_t head_form, head_rows, n_launch, n_steps; int32_t form[32], steps[32], rows[32]; };
constexpr uint32_t kAkDevHeadMaxB = 8, kAkDevHeadMaxDim = 4096, kAkDevSmallOut = 1 + 300 + 8;

// the candidate bound of an image of the level table (ak_level_table's d.bound): the slots per image both entries below allocate and the
// triples per image of their lists_out
static uint64_t ak_dev_bound(const std::vector<AkLevelHost>& lv)
{
    uint64_t bound = 0;
    for (const AkLevelHost& e : lv) bound += (uint64_t)((e.w + 1) / 2) * (uint64_t)((e.h + 1) / 2);
    return bound;
}

// The launch plan ak_evolve_level follows for every level of a batch of B width x height images (ak_level_plan, the detector's own
// decision; level 0 has no launches of this kind), with the developer knobs of this process.  Needs no device.  plan_out [n_levels].
extern "C" int r3dm_dev_akaze_head_plan(uint32_t width, uint32_t height, uint32_t B, r3dm_dev_ak_plan* plan_out)
{
    if (!plan_out || B < 1 || B > kAkDevHeadMaxB || width < 3 || height < 3 || width > kAkDevHeadMaxDim || height > kAkDevHeadMaxDim) return R3DM_ERR_INVALID;
    const std::vector<AkLevelHost> lv = ak_levels((int)width, (int)height);
    if (lv.empty() || lv.size() > 16) return R3DM_ERR_INVALID;
    const int taps_one_n = ak_taps(1.0f).n;
    for (size_t i = 0; i < lv.size(); ++i) {
        r3dm_dev_ak_plan o{};
        if (i > 0) {
            const size_t n_tau = ak_fed_tau(lv[i].etime - lv[i - 1].etime).size();
            const AkLevelPlan pl = ak_level_plan(lv, (int)i, (int)B, taps_one_n, n_tau);
            if (pl.steps.size() > 32) return R3DM_ERR_UNSUPPORTED;
            o.head_form = pl.head ? 1 : 0; o.head_rows = pl.head_rows; o.n_launch = (int32_t)pl.steps.size(); o.n_steps = (int32_t)n_tau;
            for (size_t m = 0; m < pl.steps.size(); ++m) { o.form[m] = pl.form[m]; o.steps[m] = pl.steps[m]; o.rows[m] = pl.rows[m]; }
        }
        plan_out[i] = o;
    }
    return R3DM_OK;
}

extern "C" int r3dm_dev_akaze_head_bound(uint32_t width, uint32_t height, uint64_t* bound)
{
    if (!bound || width < 3 || height < 3 || width > 65536u || height > 65536u) return R3DM_ERR_INVALID;
    *bound = ak_dev_bound(ak_levels((int)width, (int)height));
    return R3DM_OK;
}

// Refused before anything touches a device (R3DM_OK or R3DM_ERR_INVALID): B outside 1 .. 8, a dimension above 4096 (or below 3), an
// image size without an evolution level, a null image, a value that is not finite or lies outside [0, 1].
// Every kernel of the scale space addresses by the plane's own (w, h) alone -- clamped or reflected taps, one-sided stencils on the rim,
// strips and bands cut at the plane's edge -- and for a finite image in [0, 1] every plane stays finite: the gradient modulus is at most
// 32 sqrt 2 (Scharr weights sum to 32), so a bin index (int)(m 299 / hmax) lies in 0 .. 299.  The extremum pass reads Ldet at interior
// columns +- 1 and at rows border - 1 .. min(., h - 1) (border >= 1 of a level the table holds); the pruning reads the lists only.
extern "C" int r3dm_dev_akaze_head_check(uint32_t B, const float* const* images, uint32_t width, uint32_t height)
{
    if (!images || B < 1 || B > kAkDevHeadMaxB) return R3DM_ERR_INVALID;
    if (width < 3 || height < 3 || width > kAkDevHeadMaxDim || height > kAkDevHeadMaxDim) return R3DM_ERR_INVALID;
    const std::vector<AkLevelHost> lv = ak_levels((int)width, (int)height);
    if (lv.empty() || lv.size() > 16) return R3DM_ERR_INVALID;
    const size_t n0 = (size_t)width * height;
    for (uint32_t b = 0; b < B; ++b) {
        if (!images[b]) return R3DM_ERR_INVALID;
        for (size_t k = 0; k < n0; ++k) if (!(images[b][k] >= 0.0f && images[b][k] <= 1.0f)) return R3DM_ERR_INVALID;    // (false for a NaN too)
    }
    return R3DM_OK;
}

// what both entries share once the planes stand on the device: the level table, the head launches at the bound, the read-back of
// counts_out [B][nl][2] (candidates, kept) and lists_out [B][bound][3] (image b's kept lists, level after level, from b bound on)
static int ak_dev_head_run(AkPass& p, float threshold, uint32_t* counts_out, float* lists_out)
{
    r3dm_ctx* c = p.c; hipStream_t st = p.st;
    const int nl = p.nl; const uint32_t B = p.B;
    AkDetection d;
    int rc = ak_level_table(p, d);
    if (rc != R3DM_OK) return rc;
    if (d.bound == 0 || d.bound * B >= (1ull << 31)) { c->err = "developer head entry: more slots than the arrays index"; return R3DM_ERR_UNSUPPORTED; }
    const uint32_t cap = (uint32_t)d.bound;
    if ((rc = ak_table_upload(p, d, cap, false)) != R3DM_OK) return rc;
    R3DM_HIP(c, ak_head_launches(st, d.d_levels, nl, (int)B, d.tiles, d.n_tiles, d.max_rows, p.tail(T_SLOTS).as<unsigned char>(), cap, d.d_bmeta, threshold));
    std::vector<AkLevelDev> dl(d.n_lv);
    std::vector<uint32_t> cnt(4 * d.n_lv, 0u);
    d.bm.assign(B, AkBatchMeta{});
    R3DM_HIP(c, hipMemcpyAsync(dl.data(), d.d_levels, d.n_lv * sizeof(AkLevelDev), hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipMemcpyAsync(cnt.data(), d.ld[0].counts, cnt.size() * 4, hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipMemcpyAsync(d.bm.data(), d.d_bmeta, (size_t)B * sizeof(AkBatchMeta), hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipStreamSynchronize(st));
    std::vector<float> l4;
    for (uint32_t b = 0; b < B; ++b) {
        if (d.bm[b].overflow) { c->err = "developer head entry: candidate count exceeds its own bound"; return R3DM_ERR_HIP; }
        size_t at = (size_t)b * cap, kept = 0;
        for (int i = 0; i < nl; ++i) {
            const size_t k = (size_t)b * nl + i;
            const uint32_t nc = cnt[4 * k], nk = cnt[4 * k + 1];
            kept += nk;
            if (nk > nc || kept > cap) { c->err = "developer head entry: a list longer than its candidates"; return R3DM_ERR_HIP; }
            counts_out[2 * k] = nc; counts_out[2 * k + 1] = nk;
            if (!nk) continue;
            l4.resize(4 * (size_t)nk);
            R3DM_HIP(c, hipMemcpyAsync(l4.data(), dl[k].list, (size_t)nk * 16, hipMemcpyDeviceToHost, st));
            R3DM_HIP(c, hipStreamSynchronize(st));
            for (size_t q = 0; q < nk; ++q) { lists_out[3 * (at + q)] = l4[4 * q]; lists_out[3 * (at + q) + 1] = l4[4 * q + 1]; lists_out[3 * (at + q) + 2] = l4[4 * q + 2]; }
            at += nk;
        }
    }
    return R3DM_OK;
}

// planes_out [B][nl][4]: Ldet, Lx, Ly, Lt of every level (the caller's, w_i x h_i floats each); small_out [B][309]: the bits of the
// gradient modulus' maximum, the 300 bins, the bits of 1 / k^2 of octaves 0 .. 7; plan_out [nl]: what ak_evolve_level launched.
extern "C" int r3dm_dev_akaze_head(r3dm_ctx* c, uint32_t B, const float* const* images, uint32_t width, uint32_t height, float threshold,
                                   float* const* planes_out, uint32_t* counts_out, float* lists_out, uint32_t* small_out, r3dm_dev_ak_plan* plan_out)
{
    const int vrc = r3dm_dev_akaze_head_check(B, images, width, height);
    if (vrc != R3DM_OK) { if (c) c->err = "r3dm_dev_akaze_head: images the entry does not take"; return vrc; }
    if (!c || !planes_out || !counts_out || !lists_out || !small_out || !plan_out) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int {
        R3DM_HIP(c, hipSetDevice(c->device));
        const std::vector<AkLevelHost> lv = ak_levels((int)width, (int)height);
        const int nl = (int)lv.size();
        for (size_t k = 0; k < (size_t)B * nl * 4; ++k) if (!planes_out[k]) return R3DM_ERR_INVALID;
        AkPass p{c, c->stream, B, (int)B, (int)width, (int)height, nl, (size_t)width * height, lv};
        hipStream_t st = p.st;
        int rc_plan = R3DM_OK;
        if ((rc_plan = r3dm_dev_akaze_head_plan(width, height, B, plan_out)) != R3DM_OK) return rc_plan;
        int rc = ak_buffers(p);
        if (rc == R3DM_OK) rc = detect_upload(c, B, images, nullptr, p.n0, p.img, reinterpret_cast<unsigned char*>(p.tmp2));
        p.taps_off = ak_taps(1.6f); p.taps_one = ak_taps(1.0f);
        if (rc == R3DM_OK) rc = detect_area_tabs(c, p.tail(T_TABS), p.lv, p.half_tabs);
        if (rc != R3DM_OK) return rc;
        R3DM_HIP(c, ak_scale_space(p));
        if ((rc = ak_dev_head_run(p, threshold, counts_out, lists_out)) != R3DM_OK) return rc;
        for (uint32_t b = 0; b < B; ++b) {
            for (int i = 0; i < nl; ++i) {
                const size_t plane = (size_t)lv[i].w * lv[i].h;
                float* const* P = planes_out + ((size_t)b * nl + i) * 4;
                R3DM_HIP(c, hipMemcpyAsync(P[0], p.Ldet(i) + b * plane, plane * 4, hipMemcpyDeviceToHost, st));
                R3DM_HIP(c, hipMemcpyAsync(P[1], p.Lx(i) + b * plane, plane * 4, hipMemcpyDeviceToHost, st));
                R3DM_HIP(c, hipMemcpyAsync(P[2], p.Ly(i) + b * plane, plane * 4, hipMemcpyDeviceToHost, st));
                R3DM_HIP(c, hipMemcpyAsync(P[3], p.Lt(i) + b * plane, plane * 4, hipMemcpyDeviceToHost, st));
            }
            uint32_t* S = small_out + (size_t)b * kAkDevSmallOut;
            const uint32_t* D = p.small + (size_t)b * 4096;
            R3DM_HIP(c, hipMemcpyAsync(S, D, 4, hipMemcpyDeviceToHost, st));
            R3DM_HIP(c, hipMemcpyAsync(S + 1, D + 16, 300 * 4, hipMemcpyDeviceToHost, st));
            R3DM_HIP(c, hipMemcpyAsync(S + 301, D + 1024, 8 * 4, hipMemcpyDeviceToHost, st));
        }
        R3DM_HIP(c, hipStreamSynchronize(st));
        return R3DM_OK;
    });
}

// The extremum pass and the in-level pruning on a caller's determinant planes.  Refused (R3DM_OK or R3DM_ERR_INVALID; c may be null):
// what the tail's check refuses of planes -- n_levels and plane_dims [n_levels][2] other than the table's of (width, height), B outside
// 1 .. 64, a null plane, a value that is not finite.  ldet [B][n_levels].
// Why every read of an accepted input stays inside its plane: the extremum pass reads Ldet at columns border - 1 .. w - border (a lane
// beyond the interior reads column border) and at rows border - 1 .. min(h - border, h - 1), border >= 1; the emit pass reads Ldet at the
// set bits, interior positions; the pruning reads the candidate and list arrays only, which hold at most the bound's entries.
extern "C" int r3dm_dev_akaze_extrema_check(uint32_t width, uint32_t height, uint32_t B, uint32_t n_levels, const uint32_t* plane_dims,
                                            const float* const* ldet)
{
    std::vector<AkLevelHost> lv;
    return B >= 1 && B <= kAkDevMaxB && ak_dev_planes_ok(width, height, kAkSmaxDetector, B, n_levels, plane_dims, ldet, 1, lv) ? R3DM_OK : R3DM_ERR_INVALID;
}

// Lx, Ly and Lt of every level are zero; counts_out and lists_out as r3dm_dev_akaze_head's.
extern "C" int r3dm_dev_akaze_extrema(r3dm_ctx* c, uint32_t width, uint32_t height, uint32_t B, uint32_t n_levels, const uint32_t* plane_dims,
                                      const float* const* ldet, float threshold, uint32_t* counts_out, float* lists_out)
{
    const int vrc = r3dm_dev_akaze_extrema_check(width, height, B, n_levels, plane_dims, ldet);
    if (vrc != R3DM_OK) { if (c) c->err = "r3dm_dev_akaze_extrema: planes the kernels would mis-read"; return vrc; }
    if (!c || !counts_out || !lists_out) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int {
        R3DM_HIP(c, hipSetDevice(c->device));
        const std::vector<AkLevelHost> lv = ak_levels((int)width, (int)height);
        const int nl = (int)lv.size();
        AkPass p{c, c->stream, B, (int)B, (int)width, (int)height, nl, (size_t)width * height, lv};
        hipStream_t st = p.st;
        int rc = ak_buffers(p);
        if (rc != R3DM_OK) return rc;
        for (int i = 0; i < nl; ++i) {
            const size_t plane = (size_t)lv[i].w * lv[i].h;
            for (uint32_t b = 0; b < B; ++b) R3DM_HIP(c, hipMemcpyAsync(p.Ldet(i) + b * plane, ldet[(size_t)b * nl + i], plane * 4, hipMemcpyHostToDevice, st));
            R3DM_HIP(c, hipMemsetAsync(p.Lx(i), 0, (size_t)B * plane * 4, st));
            R3DM_HIP(c, hipMemsetAsync(p.Ly(i), 0, (size_t)B * plane * 4, st));
            R3DM_HIP(c, hipMemsetAsync(p.Lt(i), 0, (size_t)B * plane * 4, st));
        }
        return ak_dev_head_run(p, threshold, counts_out, lists_out);
    });
}
#endif  // R3DM_DEVTOOLS
