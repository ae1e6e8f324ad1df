// api_akaze_classic.cpp -- part of the host side of libr3dm.so: the classic A-KAZE detector, Regard3D's "AKAZE" arm
// (r3dm_detect_akaze_classic / _batch in include/r3dm.h; kernels in kernels_akaze_classic.hip).
// The arm is libAKAZE with its AKAZEConfig.h defaults (src/thirdparty/akaze/lib/), as Regard3D runs it through
// cv::AKAZE::create(DESCRIPTOR_MLDB, 0, 3, threshold, 4, 4, DIFF_PM_G2) + detect() (src/Regard3DFeatures.cpp:578-589).
#include "r3dm_ctx.hpp"

#include <array>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

struct AcLevelHost {
    int w, h, octave, sigma_size;
    float esigma, etime, ratio;
};

// Allocate_Memory_Evolution (AKAZE.cpp:51-99).  Differs from the Fast arm's table: the level size is (int)(size / 2^i), an octave
// i > 0 below 80 x 40 ends the table, and no descriptor border stops it; sigma_size is the multiscale derivative's
// fRound(esigma * derivative_factor / 2^octave) (:198).
std::vector<AcLevelHost> ac_levels(int w, int h)
{
    std::vector<AcLevelHost> lv;
    for (int i = 0; i < 4; ++i) {
        const double rfactor = 1.0 / pow(2.0f, i);
        const int lh = (int)(h * rfactor), lw = (int)(w * rfactor);
        if ((lw < 80 || lh < 40) && i != 0) break;
        for (int j = 0; j < 4; ++j) {
            AcLevelHost e{};
            e.w = lw; e.h = lh; e.octave = i;
            e.esigma = 1.6f * powf(2.0f, (float)j / 4.0f + (float)i);
            e.etime = (float)(0.5 * (e.esigma * e.esigma));
            e.ratio = (float)pow(2.0f, (float)i);
            e.sigma_size = (int)(e.esigma * 1.5f / e.ratio + 0.5f);
            lv.push_back(e);
        }
    }
    return lv;
}

bool ac_is_prime(int number)
{
    if (number <= 1) return false;
    if (number == 2 || number == 3 || number == 5 || number == 7) return true;
    if ((number % 2) == 0 || (number % 3) == 0 || (number % 5) == 0 || (number % 7) == 0) return false;
    const int upper = (int)sqrt(number + 1.0);
    for (int divisor = 11; divisor <= upper; divisor += 2) if (number % divisor == 0) return false;
    return true;
}

// fed_tau_by_process_time(T, 1, 0.25, reordering = true) (fed.cpp).  Differs from fed_tau_by_process_timeV2: n and the scale are formed
// in double and the cosine is the double cos of the host libm.  (libAKAZE also reorders n == 1, reading tauh[-1]; these defaults never
// give n == 1, where this returns tauh.)
std::vector<float> ac_fed_tau(float T)
{
    const float t = T / 1.0f, tau_max = 0.25f;
    const int n = (int)(ceil(sqrt(3.0 * t / tau_max + 0.25f) - 0.5f - 1.0e-8f) + 0.5f);
    std::vector<float> tau;
    if (n <= 0) return tau;
    const float scale = (float)(3.0 * t / (tau_max * (float)(n * (n + 1))));
    const float c = 1.0f / (4.0f * (float)n + 2.0f);
    const float d = scale * tau_max / 2.0f;
    std::vector<float> tauh(n);
    for (int k = 0; k < n; ++k) {
        const float hh = (float)cos(3.1415926535897932384626433832795 * (2.0f * (float)k + 1.0f) * c);
        tauh[k] = d / (hh * hh);
    }
    if (n == 1) return tauh;
    const int kappa = n / 2;
    int prime = n + 1;
    while (!ac_is_prime(prime)) prime++;
    tau.resize(n);
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index = 0;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
        tau[l] = tauh[index];
    }
    return tau;
}

}  // namespace

// the detector over B same-size images; out[b] = the keypoints of image b in the reference's order.  images: B pointers to height x width
// floats (host or device), or bgrs: B pointers to height x width x 3 bytes, converted on the device by the Fast arm's gray kernel.
// Leaves the B gray images in ac_bufs[0] (B planes) for the LIOP pass of the features entries.
int ac_detect_batch(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height,
                    float threshold, std::vector<std::vector<AcOut>>& out)
{
    if (!c || B == 0 || (!images && !bgrs)) return R3DM_ERR_INVALID;
    for (uint32_t b = 0; b < B; ++b) if (!(images ? (const void*)images[b] : (const void*)bgrs[b])) return R3DM_ERR_INVALID;
    if ((uint64_t)width * height > (1ull << 30) || B > 4096) return R3DM_ERR_INVALID;
    out.assign(B, std::vector<AcOut>());
    if (width < 3 || height < 3) return R3DM_OK;                      // no 3 x 3 maximum exists
    R3DM_HIP(c, hipSetDevice(c->device));
    const double t_call = now_ms();
    const int w = (int)width, h = (int)height, iB = (int)B;
    const std::vector<AcLevelHost> lv = ac_levels(w, h);
    const int nl = (int)lv.size();
    hipStream_t st = c->stream;
    const size_t n0 = (size_t)w * h;

    // work buffers on the context, kept between calls (they grow, never shrink; released with the context): B planes each of the image,
    // two evolving images, the smoothed image, the conductivity and a Gaussian scratch; per level Lx, Ly, Ldet (read again by the
    // refinement and the orientation); then the candidate, slot, grid and output arrays
    enum { C_IMG, C_LTA, C_LTB, C_SMOOTH, C_FLOW, C_TMP, C_SMALL, C_ROWS, C_TABS, C_CAND, C_SLOTS, C_NSL, C_OUTS, C_HEADS, C_ESLOT, C_ECELL,
           C_ENEXT, C_CC, C_UPHEADS, C_UPNEXT, C_PLANES };
    if (c->ac_bufs.size() != (size_t)C_PLANES + 3 * kAcMaxLevels) c->ac_bufs.resize((size_t)C_PLANES + 3 * kAcMaxLevels);
    auto buf = [&](int k) -> DevBuf& { return c->ac_bufs[k]; };
    DevBuf &img = buf(C_IMG), &ltA = buf(C_LTA), &ltB = buf(C_LTB), &smooth = buf(C_SMOOTH), &flow = buf(C_FLOW), &tmp = buf(C_TMP);
    DevBuf &small = buf(C_SMALL), &rows = buf(C_ROWS), &tabs = buf(C_TABS);
    DevBuf* planes = &c->ac_bufs[C_PLANES];
    for (DevBuf* b : {&img, &ltA, &ltB, &smooth, &flow, &tmp}) R3DM_HIP(c, b->ensure((size_t)B * n0 * 4));
    R3DM_HIP(c, small.ensure((size_t)B * 4096 * 4));
    for (int i = 0; i < nl; ++i)
        for (int q = 0; q < 3; ++q) R3DM_HIP(c, planes[3 * i + q].ensure((size_t)B * lv[i].w * lv[i].h * 4));
    auto Lx = [&](int i) { return planes[3 * i].as<float>(); };
    auto Ly = [&](int i) { return planes[3 * i + 1].as<float>(); };
    auto Ldet = [&](int i) { return planes[3 * i + 2].as<float>(); };
    if (images) {
        for (uint32_t b = 0; b < B; ++b) R3DM_HIP(c, hipMemcpyAsync(img.as<float>() + b * n0, images[b], n0 * 4, hipMemcpyDefault, st));
    } else {
        // 8-bit BGR -> gray as the Fast arm converts it (ak_bgr_to_gray): the bytes are staged in the (not yet used) work image tmp
        unsigned char* stage = tmp.as<unsigned char>();
        for (uint32_t b = 0; b < B; ++b) R3DM_HIP(c, hipMemcpyAsync(stage + b * n0 * 4, bgrs[b], n0 * 3, hipMemcpyDefault, st));
        for (uint32_t b = 0; b < B; ++b) R3DM_HIP(c, ak_bgr_to_gray(st, stage + b * n0 * 4, img.as<float>() + b * n0, n0));
    }

    // INTER_AREA tables of the octave transitions that are not exact halvings
    std::vector<std::array<size_t, 4>> toff(nl, {(size_t)-1, 0, 0, 0});
    {
        std::vector<unsigned char> blob;
        auto put = [&](const void* p, size_t bytes) { const size_t at = (blob.size() + 15) / 16 * 16; blob.resize(at + bytes); memcpy(blob.data() + at, p, bytes); return at; };
        for (int i = 1; i < nl; ++i) {
            if (lv[i].octave == lv[i - 1].octave) continue;
            const int sw = lv[i - 1].w, sh = lv[i - 1].h;
            if (lv[i].w * 2 == sw && lv[i].h * 2 == sh) continue;
            std::vector<AkAreaTab> tx, ty; std::vector<int> bx, by;
            ak_area_tab(sw, lv[i].w, tx, bx); ak_area_tab(sh, lv[i].h, ty, by);
            toff[i] = {put(tx.data(), tx.size() * sizeof(AkAreaTab)), put(ty.data(), ty.size() * sizeof(AkAreaTab)), put(bx.data(), bx.size() * 4), put(by.data(), by.size() * 4)};
        }
        if (!blob.empty()) {
            R3DM_HIP(c, tabs.ensure(blob.size() + 64));
            R3DM_HIP(c, hipMemcpyAsync(tabs.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
            R3DM_HIP(c, hipStreamSynchronize(st));
        }
    }
    const AkTaps taps_off = ak_taps(1.6f), taps_one = ak_taps(1.0f);
    uint32_t* sm = small.as<uint32_t>();
    const float* inv_k2 = reinterpret_cast<const float*>(sm + 1024);
    R3DM_HIP(c, hipEventRecord(c->ev0, st));

    // Create_Nonlinear_Scale_Space (AKAZE.cpp:102-170).  Level 0: Lt = Lsmooth = the soffset Gaussian of the image.  The contrast factor is
    // compute_k_percentile of the INPUT image (sigma 1, Scharr, its own histogram: ac_kcontrast).
    float* cur = ltA.as<float>();
    float* other = ltB.as<float>();
    R3DM_HIP(c, ak_gaussian(st, img.as<float>(), tmp.as<float>(), cur, w, h, iB, taps_off));
    R3DM_HIP(c, hipMemsetAsync(sm, 0, (size_t)B * 4096 * 4, st));
    R3DM_HIP(c, ak_gaussian(st, img.as<float>(), tmp.as<float>(), smooth.as<float>(), w, h, iB, taps_one));
    R3DM_HIP(c, ak_modg_max(st, smooth.as<float>(), w, h, iB, sm));
    R3DM_HIP(c, ac_kcontrast(st, smooth.as<float>(), w, h, iB, sm));
    // Compute_Multiscale_Derivatives + Compute_Determinant_Hessian_Response (:188-248) of a level: from its Lsmooth, taps of scale s
    auto hessian = [&](int i, const float* src) -> hipError_t {
        const int s = lv[i].sigma_size;
        const float wq = (float)(10.0 / 3.0);
        const float norm = (float)(1.0 / (2.0 * (double)s * (wq + 2.0)));
        return ac_hessian(st, src, Lx(i), Ly(i), Ldet(i), lv[i].w, lv[i].h, iB, s, norm, wq * norm);
    };
    R3DM_HIP(c, hessian(0, cur));
    for (int i = 1; i < nl; ++i) {
        const int lw = lv[i].w, lh = lv[i].h;
        if (lv[i].octave > lv[i - 1].octave) {
            const unsigned char* base = tabs.as<unsigned char>();
            const bool tab = toff[i][0] != (size_t)-1;
            R3DM_HIP(c, ak_halfsample(st, cur, other, lv[i - 1].w, lv[i - 1].h, iB,
                                      tab ? (const AkAreaTab*)(base + toff[i][0]) : nullptr, tab ? (const int*)(base + toff[i][2]) : nullptr,
                                      tab ? (const AkAreaTab*)(base + toff[i][1]) : nullptr, tab ? (const int*)(base + toff[i][3]) : nullptr));
            std::swap(cur, other);
        }
        // (same octave: the previous level's Lt is this level's start image, copyTo without a copy)
        R3DM_HIP(c, ak_gaussian(st, cur, tmp.as<float>(), smooth.as<float>(), lw, lh, iB, taps_one));
        R3DM_HIP(c, hessian(i, smooth.as<float>()));
        R3DM_HIP(c, ak_scharr_g2(st, smooth.as<float>(), flow.as<float>(), lw, lh, iB, inv_k2 + lv[i].octave));   // pm_g2, 1 / k^2 of the octave
        for (float tau : ac_fed_tau(lv[i].etime - lv[i - 1].etime)) {
            R3DM_HIP(c, ac_fed_step(st, cur, flow.as<float>(), other, lw, lh, iB, 0.5f * tau));
            std::swap(cur, other);
        }
    }

    // Find_Scale_Space_Extrema (:251-386): per-row counts, their scan, the candidates in scan order (levels, rows, columns)
    std::vector<uint32_t> row0(nl);
    uint32_t n_rows = 0;
    for (int i = 0; i < nl; ++i) { row0[i] = n_rows; n_rows += (uint32_t)lv[i].h; }
    const uint32_t rows_stride = n_rows + 1;
    R3DM_HIP(c, rows.ensure(((size_t)B * rows_stride + B) * 4));
    uint32_t* rc = rows.as<uint32_t>();
    uint32_t* totals = rc + (size_t)B * rows_stride;
    R3DM_HIP(c, hipMemsetAsync(rc, 0, ((size_t)B * rows_stride + B) * 4, st));
    for (int i = 0; i < nl; ++i) R3DM_HIP(c, ac_extrema(st, Ldet(i), lv[i].w, lv[i].h, iB, threshold, rc, rows_stride, row0[i], nullptr, 0, i, 0));
    R3DM_HIP(c, ac_scan_rows(st, rc, rows_stride, n_rows, iB, totals));
    std::vector<uint32_t> tot(B);
    R3DM_HIP(c, hipMemcpyAsync(tot.data(), totals, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipStreamSynchronize(st));
    uint32_t stride = 1;
    for (uint32_t b = 0; b < B; ++b) stride = std::max(stride, tot[b]);
    DevBuf &cand = buf(C_CAND), &slots = buf(C_SLOTS), &nsl = buf(C_NSL), &outs = buf(C_OUTS);
    R3DM_HIP(c, cand.ensure((size_t)B * stride * sizeof(AcCand)));
    R3DM_HIP(c, slots.ensure((size_t)B * stride * sizeof(AcSlot)));
    R3DM_HIP(c, nsl.ensure((size_t)B * 4));
    R3DM_HIP(c, outs.ensure((size_t)B * stride * sizeof(AcOut)));
    // the kpts_aux walk's grid: cells of side >= 3 px (level 0: size 2.4) over the image, entries = the slots entered at a level start
    // (<= stride) + one per accepted point of the level (<= stride)
    AcGrid grid{};
    grid.img_w = w; grid.img_h = h;
    grid.cells_stride = (size_t)(w / 3 + 2) * (size_t)(h / 3 + 2);
    grid.ent_stride = 2 * (size_t)stride;
    R3DM_HIP(c, buf(C_HEADS).ensure((size_t)B * grid.cells_stride * 4));
    R3DM_HIP(c, buf(C_ESLOT).ensure((size_t)B * grid.ent_stride * 4));
    R3DM_HIP(c, buf(C_ECELL).ensure((size_t)B * grid.ent_stride * 4));
    R3DM_HIP(c, buf(C_ENEXT).ensure((size_t)B * grid.ent_stride * 4));
    grid.heads = buf(C_HEADS).as<int>(); grid.ent_slot = buf(C_ESLOT).as<uint32_t>(); grid.ent_cell = buf(C_ECELL).as<uint32_t>();
    grid.ent_next = buf(C_ENEXT).as<int>();
    R3DM_HIP(c, hipMemsetAsync(grid.heads, 0xFF, (size_t)B * grid.cells_stride * 4, st));
    for (int i = 0; i < nl; ++i)
        R3DM_HIP(c, ac_extrema(st, Ldet(i), lv[i].w, lv[i].h, iB, threshold, rc, rows_stride, row0[i], cand.as<AcCand>(), stride, i, 1));
    AcLevelTab tab{};
    AcPlanes pl{};
    tab.n_levels = nl;
    tab.smax = (float)(10.0 * sqrtf(2.0f));
    for (int i = 0; i < nl; ++i) {
        tab.w[i] = lv[i].w; tab.h[i] = lv[i].h; tab.octave[i] = lv[i].octave;
        tab.esigma[i] = lv[i].esigma; tab.ratio[i] = lv[i].ratio; tab.off[i] = (float)(.5 * (lv[i].ratio - 1.0));
        pl.ldet[i] = Ldet(i); pl.lx[i] = Lx(i); pl.ly[i] = Ly(i);
    }
    for (int i = 0; i < nl; ++i) tab.row0[i] = row0[i];
    // R3DM_AC_AUX=0 (developer build): the one-wavefront walk over every candidate and the upper-level filter over every later slot.
    // R3DM_AC_AUX_BOUND (test hook): a smaller wavefront bound hands more components back to the one-wavefront walk.
    static const bool parallel = r3dm_dev_knob("R3DM_AC_AUX", 1) != 0;
    static const uint32_t bound = [] { const int v = r3dm_dev_knob("R3DM_AC_AUX_BOUND", 64); return (uint32_t)(v < 1 ? 1 : v > 64 ? 64 : v); }();
    AcUpGrid ug{};
    uint32_t* hist = nullptr;
    if (!parallel) {
        R3DM_HIP(c, ac_aux(st, cand.as<AcCand>(), stride, totals, tab, slots.as<AcSlot>(), grid, nsl.as<uint32_t>(), iB));
    } else {
        // nine per-candidate arrays, then n_big [B], scan totals [B], the histogram [32 B]
        const size_t per = (size_t)B * stride;
        R3DM_HIP(c, buf(C_CC).ensure((9 * per + 34 * (size_t)B) * 4));
        uint32_t* w0 = buf(C_CC).as<uint32_t>();
        AcCc cc{};
        uint32_t** arrs[9] = {&cc.par, &cc.csz, &cc.boff, &cc.cur, &cc.memb, &cc.fin, &cc.opn, &cc.big, &cc.bopen};
        for (int k = 0; k < 9; ++k) *arrs[k] = w0 + (size_t)k * per;
        cc.n_big = w0 + 9 * per; cc.scratch = cc.n_big + B; hist = cc.hist = cc.scratch + B;
        cc.rows = rc; cc.rows_stride = rows_stride;
        R3DM_HIP(c, hipMemsetAsync(hist, 0, (size_t)B * 32 * 4, st));
        R3DM_HIP(c, ac_aux_parallel(st, cand.as<AcCand>(), stride, totals, tab, slots.as<AcSlot>(), grid, nsl.as<uint32_t>(), cc, bound, iB));
        // the upper-level filter's buckets: class k >= 1 in cells of side floor(size_{k-1}) + 1 over the image
        ug.img_w = w; ug.img_h = h;
        size_t cells = 0;
        for (int k = 1; k < nl; ++k) {
            ug.G[k] = (int)(lv[k - 1].esigma * 1.5f) + 1;
            ug.cell_off[k] = (uint32_t)cells;
            cells += (size_t)(w / ug.G[k] + 2) * (size_t)(h / ug.G[k] + 2);
        }
        ug.cells_stride = std::max<size_t>(cells, 1);
        R3DM_HIP(c, buf(C_UPHEADS).ensure((size_t)B * ug.cells_stride * 4));
        R3DM_HIP(c, buf(C_UPNEXT).ensure(per * 4));
        ug.heads = buf(C_UPHEADS).as<int>(); ug.next = buf(C_UPNEXT).as<int>();
        R3DM_HIP(c, hipMemsetAsync(ug.heads, 0xFF, (size_t)B * ug.cells_stride * 4, st));
    }
    R3DM_HIP(c, ac_finish(st, slots.as<AcSlot>(), stride, nsl.as<uint32_t>(), tab, pl, outs.as<AcOut>(), stride, iB, ug));
    R3DM_HIP(c, hipEventRecord(c->ev1, st));
    std::vector<uint32_t> ns(B), hs(hist ? (size_t)B * 32 : 0);
    R3DM_HIP(c, hipMemcpyAsync(ns.data(), nsl.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    if (hist) R3DM_HIP(c, hipMemcpyAsync(hs.data(), hist, hs.size() * 4, hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipStreamSynchronize(st));
    for (size_t k = 0; k < hs.size(); ++k) c->ac_components[k % 32] += hs[k];
    for (uint32_t b = 0; b < B; ++b) {
        std::vector<AcOut> all(ns[b]);
        if (ns[b]) R3DM_HIP(c, hipMemcpyAsync(all.data(), outs.as<AcOut>() + (size_t)b * stride, (size_t)ns[b] * sizeof(AcOut), hipMemcpyDeviceToHost, st));
        R3DM_HIP(c, hipStreamSynchronize(st));
        for (const AcOut& o : all) if (o.ok) out[b].push_back(o);             // the slots that survive, in slot order
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.n_detect_images = B;
    c->stats.ms_detect_kernels = ms;
    c->stats.ms_detect = now_ms() - t_call;
    r3dm_features_totals& T = c->feat_totals;
    T.n_images += B; T.n_passes += 1; T.ms_detect_kernels += ms; T.ms_wall += c->stats.ms_detect;
    for (uint32_t b = 0; b < B; ++b) T.n_keypoints += out[b].size();
    return R3DM_OK;
}

namespace {

void ac_write(const std::vector<AcOut>& kp, float* keypoints_out, float* responses_out, uint32_t cap)
{
    for (size_t k = 0; k < kp.size() && k < cap; ++k) {
        float* o = keypoints_out + 4 * k;
        o[0] = kp[k].x; o[1] = kp[k].y; o[2] = kp[k].size; o[3] = kp[k].angle;
        if (responses_out) responses_out[k] = kp[k].resp;
    }
}

}  // namespace

extern "C" int r3dm_detect_akaze_classic(r3dm_ctx* c, const float* image, uint32_t width, uint32_t height, float threshold,
                                         float* keypoints_out, float* responses_out, uint32_t cap, uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        if (!c || !image || !n_out || (cap && !keypoints_out)) return R3DM_ERR_INVALID;
        *n_out = 0;
        std::vector<std::vector<AcOut>> kp;
        const int rc = ac_detect_batch(c, 1, &image, nullptr, width, height, threshold, kp);
        if (rc != R3DM_OK) return rc;
        ac_write(kp[0], keypoints_out, responses_out, cap);
        *n_out = (uint32_t)kp[0].size();
        return R3DM_OK;
    });
}

extern "C" int r3dm_detect_akaze_classic_batch(r3dm_ctx* c, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                                               float threshold, float* const* keypoints_out, float* const* responses_out, uint32_t cap,
                                               uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        if (!c || !images || !n_out || (cap && !keypoints_out)) return R3DM_ERR_INVALID;
        std::vector<std::vector<AcOut>> kp;
        const int rc = ac_detect_batch(c, n_images, images, nullptr, width, height, threshold, kp);
        if (rc != R3DM_OK) return rc;
        for (uint32_t b = 0; b < n_images; ++b) {
            ac_write(kp[b], cap ? keypoints_out[b] : nullptr, responses_out ? responses_out[b] : nullptr, cap);
            n_out[b] = (uint32_t)kp[b].size();
        }
        return R3DM_OK;
    });
}

extern "C" int r3dm_akaze_classic_components(const r3dm_ctx* c, uint64_t* hist)
{
    if (!c || !hist) return R3DM_ERR_INVALID;
    for (int k = 0; k < 32; ++k) hist[k] = c->ac_components[k];
    return R3DM_OK;
}
