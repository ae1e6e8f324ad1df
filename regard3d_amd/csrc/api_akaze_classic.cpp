// api_akaze_classic.cpp -- part of the host side of libr3dm.so: the classic A-KAZE detector, Regard3D's "AKAZE" arm
// (r3dm_detect_akaze_classic / _batch in include/r3dm.h; kernels in kernels_akaze_classic.hip).
// The arm is libAKAZE with its AKAZEConfig.h defaults (src/thirdparty/akaze/lib/), as Regard3D runs it through
// cv::AKAZE::create(DESCRIPTOR_MLDB, 0, 3, threshold, 4, 4, DIFF_PM_G2) + detect() (src/Regard3DFeatures.cpp:578-589).
// The frame it shares with the Fast arm (checks, upload, INTER_AREA tables, statistics tail, the detect entry) is api_akaze.cpp.
#include "r3dm_ctx.hpp"

namespace {

// Allocate_Memory_Evolution (AKAZE.cpp:51-99).  Differs from the Fast arm's table: the level size is (int)(size / 2^i), an octave
// i > 0 below 80 x 40 ends the table, and no descriptor border stops it; sigma_size is the multiscale derivative's
// fRound(esigma * derivative_factor / 2^octave) (:198).
std::vector<AkLevelHost> ac_levels(int w, int h)
{
    std::vector<AkLevelHost> lv;
    for (int i = 0; i < 4; ++i) {
        const double rfactor = 1.0 / pow(2.0f, i);
        const int lh = (int)(h * rfactor), lw = (int)(w * rfactor);
        if ((lw < 80 || lh < 40) && i != 0) break;
        for (int j = 0; j < 4; ++j) {
            AkLevelHost e{};
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
    while (!ak_is_prime(prime)) prime++;
    tau.resize(n);
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index = 0;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
        tau[l] = tauh[index];
    }
    return tau;
}

}  // namespace

// the detector over B same-size images; out.classic[b] = the keypoints of image b in the reference's order.
// Leaves the B gray images in ac_bufs[0] (B planes) for the LIOP pass of the features entries.
int ac_detect_batch(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height,
                    float threshold, DetectedBatch& out)
{
    if (!detect_args_ok(c, B, images, bgrs, width, height)) return R3DM_ERR_INVALID;
    out = DetectedBatch();
    out.classic.assign(B, std::vector<AcOut>());
    if (width < 3 || height < 3) return R3DM_OK;                      // no 3 x 3 maximum exists
    R3DM_HIP(c, hipSetDevice(c->device));
    const double t_call = now_ms();
    const int w = (int)width, h = (int)height, iB = (int)B;
    const std::vector<AkLevelHost> lv = ac_levels(w, h);
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
    out.grays_dev = img.as<float>();
    // (BGR: the bytes are staged in the not yet used work image tmp)
    int frc = detect_upload(c, B, images, bgrs, n0, img.as<float>(), tmp.as<unsigned char>());
    if (frc != R3DM_OK) return frc;
    std::vector<HalfTabs> half_tabs;
    if ((frc = detect_area_tabs(c, tabs, lv, half_tabs)) != R3DM_OK) return frc;
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
            const HalfTabs& ht = half_tabs[i];
            R3DM_HIP(c, ak_halfsample(st, cur, other, lv[i - 1].w, lv[i - 1].h, iB, ht.xt, ht.xb, ht.yt, ht.yb));
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
        for (const AcOut& o : all) if (o.ok) out.classic[b].push_back(o);             // the slots that survive, in slot order
    }
    uint64_t n_kp = 0;
    for (uint32_t b = 0; b < B; ++b) n_kp += out.classic[b].size();
    detect_finish(c, B, t_call, n_kp, 0.0);                              // (this arm tallies no plane moves: the byte statistics stay as they were)
    return R3DM_OK;
}

extern "C" int r3dm_detect_akaze_classic(r3dm_ctx* c, const float* image, uint32_t width, uint32_t height, float threshold,
                                         float* keypoints_out, float* responses_out, uint32_t cap, uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        DetectedBatch det;
        return detect_entry(c, ac_detect_batch, true, 1, &image, width, height, threshold, &keypoints_out, &responses_out, cap, n_out, det);
    });
}

extern "C" int r3dm_detect_akaze_classic_batch(r3dm_ctx* c, uint32_t n_images, const float* const* images, uint32_t width, uint32_t height,
                                               float threshold, float* const* keypoints_out, float* const* responses_out, uint32_t cap,
                                               uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int {
        DetectedBatch det;
        return detect_entry(c, ac_detect_batch, false, n_images, images, width, height, threshold, keypoints_out, responses_out, cap, n_out, det);
    });
}

extern "C" int r3dm_akaze_classic_components(const r3dm_ctx* c, uint64_t* hist)
{
    if (!c || !hist) return R3DM_ERR_INVALID;
    for (int k = 0; k < 32; ++k) hist[k] = c->ac_components[k];
    return R3DM_OK;
}
