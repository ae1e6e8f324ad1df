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

// the context's work buffers of this arm (c->ac_bufs), by index; from C_PLANES on: per level Lx, Ly, Ldet
enum { C_IMG, C_LTA, C_LTB, C_SMOOTH, C_FLOW, C_TMP, C_SMALL, C_ROWS, C_TABS, C_CAND, C_SLOTS, C_NSL, C_OUTS, C_HEADS, C_ESLOT, C_ECELL,
       C_ENEXT, C_CC, C_UPHEADS, C_UPNEXT, C_PLANES };
void ac_bufs_init(r3dm_ctx* c)
{
    if (c->ac_bufs.size() != (size_t)C_PLANES + 3 * kAcMaxLevels) c->ac_bufs.resize((size_t)C_PLANES + 3 * kAcMaxLevels);
}

// The kpts_aux walk and what follows it, from the point where the candidates of the B images (C_CAND, `stride` per image, scan order),
// their row offsets rc (rows_stride per image, tab.row0) and their totals are on the device: the walk in the asked form (parallel: the
// components form with the wavefront bound `bound`; otherwise one wavefront per image over every candidate, and the upper-level filter
// over every later slot), the upper-level filter's buckets, then ac_finish over the planes pl.  Queues on the context's stream and
// returns without waiting: the slots are in C_SLOTS, their counts in C_NSL, the finished slots in C_OUTS, and *hist_out is the
// per-image component histogram on the device (null in the one-wavefront form).  The detector and the developer build's walk entry
// (r3dm_dev_akaze_classic_walk below) both go through it.
int ac_walk(r3dm_ctx* c, uint32_t B, int w, int h, const AcLevelTab& tab, const AcPlanes& pl, uint32_t stride, const uint32_t* rc,
            uint32_t rows_stride, const uint32_t* totals, bool parallel, uint32_t bound, uint32_t** hist_out)
{
    hipStream_t st = c->stream;
    const int iB = (int)B, nl = tab.n_levels;
    auto buf = [&](int k) -> DevBuf& { return c->ac_bufs[k]; };
    DevBuf &cand = buf(C_CAND), &slots = buf(C_SLOTS), &nsl = buf(C_NSL), &outs = buf(C_OUTS);
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
            ug.G[k] = (int)(tab.esigma[k - 1] * 1.5f) + 1;
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
    *hist_out = hist;
    return R3DM_OK;
}

// The head's work buffers on the context, kept between calls (they grow, never shrink; released with the context): B planes each of the
// image, two evolving images, the smoothed image, the conductivity and a Gaussian scratch; the per-image scalars; per level Lx, Ly, Ldet
// (read again by the refinement and the orientation).
int ac_head_bufs(r3dm_ctx* c, uint32_t B, const std::vector<AkLevelHost>& lv)
{
    ac_bufs_init(c);
    const size_t n0 = (size_t)lv[0].w * lv[0].h;
    for (int k : {C_IMG, C_LTA, C_LTB, C_SMOOTH, C_FLOW, C_TMP}) R3DM_HIP(c, c->ac_bufs[k].ensure((size_t)B * n0 * 4));
    R3DM_HIP(c, c->ac_bufs[C_SMALL].ensure((size_t)B * 4096 * 4));
    for (size_t i = 0; i < lv.size(); ++i)
        for (int q = 0; q < 3; ++q) R3DM_HIP(c, c->ac_bufs[C_PLANES + 3 * i + q].ensure((size_t)B * lv[i].w * lv[i].h * 4));
    return R3DM_OK;
}
float* ac_plane(r3dm_ctx* c, int level, int q) { return c->ac_bufs[C_PLANES + 3 * level + q].as<float>(); }     // q: 0 Lx, 1 Ly, 2 Ldet

// A tap of ac_scale_space: called when a level's FED steps are queued, with the level's Lsmooth (the image its derivatives are taken
// from), its conductivity (null at level 0, which has none) and its Lt, B planes each.  The three are work buffers the next level
// overwrites: a tap copies what it wants on the context's stream.  R3DM_OK, or the code the scale space returns with.
using AcTap = std::function<int(int level, const float* smooth, const float* flow, const float* lt)>;

// Create_Nonlinear_Scale_Space (AKAZE.cpp:102-170) with Compute_Multiscale_Derivatives + Compute_Determinant_Hessian_Response (:188-248)
// of every level, for the B images in C_IMG (ac_head_bufs; half_tabs from detect_area_tabs).  Queues on the context's stream and returns
// without waiting: Lx, Ly and Ldet of every level stand in the level planes, the histogram words in C_SMALL.  The detector passes no tap;
// the developer build's head entry (r3dm_dev_akaze_classic_head below) reads the planes through one.
int ac_scale_space(r3dm_ctx* c, uint32_t B, const std::vector<AkLevelHost>& lv, const std::vector<HalfTabs>& half_tabs, const AcTap* tap)
{
    hipStream_t st = c->stream;
    const int iB = (int)B, nl = (int)lv.size(), w = lv[0].w, h = lv[0].h;
    auto buf = [&](int k) { return c->ac_bufs[k].as<float>(); };
    float *img = buf(C_IMG), *smooth = buf(C_SMOOTH), *flow = buf(C_FLOW), *tmp = buf(C_TMP);
    const AkTaps taps_off = ak_taps(1.6f), taps_one = ak_taps(1.0f);
    uint32_t* sm = c->ac_bufs[C_SMALL].as<uint32_t>();
    const float* inv_k2 = reinterpret_cast<const float*>(sm + 1024);
    int trc = R3DM_OK;
    // Level 0: Lt = Lsmooth = the soffset Gaussian of the image.  The contrast factor is compute_k_percentile of the INPUT image
    // (sigma 1, Scharr, its own histogram: ac_kcontrast).
    float* cur = buf(C_LTA);
    float* other = buf(C_LTB);
    R3DM_HIP(c, ak_gaussian(st, img, tmp, cur, w, h, iB, taps_off));
    R3DM_HIP(c, hipMemsetAsync(sm, 0, (size_t)B * 4096 * 4, st));
    R3DM_HIP(c, ak_gaussian(st, img, tmp, smooth, w, h, iB, taps_one));
    R3DM_HIP(c, ak_modg_max(st, smooth, w, h, iB, sm));
    R3DM_HIP(c, ac_kcontrast(st, smooth, w, h, iB, sm));
    // the derivatives and the determinant of a level: from its Lsmooth, taps of scale s
    auto hessian = [&](int i, const float* src) -> hipError_t {
        const int s = lv[i].sigma_size;
        const float wq = (float)(10.0 / 3.0);
        const float norm = (float)(1.0 / (2.0 * (double)s * (wq + 2.0)));
        return ac_hessian(st, src, ac_plane(c, i, 0), ac_plane(c, i, 1), ac_plane(c, i, 2), lv[i].w, lv[i].h, iB, s, norm, wq * norm);
    };
    R3DM_HIP(c, hessian(0, cur));
    if (tap && (trc = (*tap)(0, cur, nullptr, cur)) != R3DM_OK) return trc;
    for (int i = 1; i < nl; ++i) {
        const int lw = lv[i].w, lh = lv[i].h;
        if (lv[i].octave > lv[i - 1].octave) {
            const HalfTabs& ht = half_tabs[i];
            R3DM_HIP(c, ak_halfsample(st, cur, other, lv[i - 1].w, lv[i - 1].h, iB, ht.xt, ht.xb, ht.yt, ht.yb));
            std::swap(cur, other);
        }
        // (same octave: the previous level's Lt is this level's start image, copyTo without a copy)
        R3DM_HIP(c, ak_gaussian(st, cur, tmp, smooth, lw, lh, iB, taps_one));
        R3DM_HIP(c, hessian(i, smooth));
        R3DM_HIP(c, ak_scharr_g2(st, smooth, flow, lw, lh, iB, inv_k2 + lv[i].octave));   // pm_g2, 1 / k^2 of the octave
        for (float tau : ac_fed_tau(lv[i].etime - lv[i - 1].etime)) {
            R3DM_HIP(c, ac_fed_step(st, cur, flow, other, lw, lh, iB, 0.5f * tau));
            std::swap(cur, other);
        }
        if (tap && (trc = (*tap)(i, smooth, flow, cur)) != R3DM_OK) return trc;
    }
    return R3DM_OK;
}

// Find_Scale_Space_Extrema's candidates (AKAZE.cpp:251-287) of the B images' Ldet planes: per-row counts, their scan, the totals (the
// one wait of the head: the candidate stride is the largest total), then the candidates in scan order (levels, rows, columns) in C_CAND.
// The detector and the developer build's head and extrema entries all go through it.
struct AcExtrema {
    std::vector<uint32_t> row0, tot;                     // first row of each level among the image's n_rows rows; candidates per image
    uint32_t n_rows = 0, rows_stride = 0, stride = 1;    // stride: candidates per image in C_CAND
    uint32_t* rc = nullptr;                              // device: row offsets, rows_stride per image
    uint32_t* totals = nullptr;                          // device: [B]
};
int ac_find_extrema(r3dm_ctx* c, uint32_t B, const std::vector<AkLevelHost>& lv, float threshold, AcExtrema& x)
{
    hipStream_t st = c->stream;
    const int iB = (int)B, nl = (int)lv.size();
    x.row0.assign(nl, 0u);
    x.n_rows = 0;
    for (int i = 0; i < nl; ++i) { x.row0[i] = x.n_rows; x.n_rows += (uint32_t)lv[i].h; }
    x.rows_stride = x.n_rows + 1;
    DevBuf &rows = c->ac_bufs[C_ROWS], &cand = c->ac_bufs[C_CAND];
    R3DM_HIP(c, rows.ensure(((size_t)B * x.rows_stride + B) * 4));
    x.rc = rows.as<uint32_t>();
    x.totals = x.rc + (size_t)B * x.rows_stride;
    R3DM_HIP(c, hipMemsetAsync(x.rc, 0, ((size_t)B * x.rows_stride + B) * 4, st));
    for (int i = 0; i < nl; ++i)
        R3DM_HIP(c, ac_extrema(st, ac_plane(c, i, 2), lv[i].w, lv[i].h, iB, threshold, x.rc, x.rows_stride, x.row0[i], nullptr, 0, i, 0));
    R3DM_HIP(c, ac_scan_rows(st, x.rc, x.rows_stride, x.n_rows, iB, x.totals));
    x.tot.assign(B, 0u);
    R3DM_HIP(c, hipMemcpyAsync(x.tot.data(), x.totals, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipStreamSynchronize(st));
    x.stride = 1;
    for (uint32_t b = 0; b < B; ++b) x.stride = std::max(x.stride, x.tot[b]);
    R3DM_HIP(c, cand.ensure((size_t)B * x.stride * sizeof(AcCand)));
    for (int i = 0; i < nl; ++i)
        R3DM_HIP(c, ac_extrema(st, ac_plane(c, i, 2), lv[i].w, lv[i].h, iB, threshold, x.rc, x.rows_stride, x.row0[i], cand.as<AcCand>(), x.stride, i, 1));
    return R3DM_OK;
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
    const int w = (int)width, h = (int)height;
    const std::vector<AkLevelHost> lv = ac_levels(w, h);
    const int nl = (int)lv.size();
    hipStream_t st = c->stream;
    const size_t n0 = (size_t)w * h;

    int frc = ac_head_bufs(c, B, lv);
    if (frc != R3DM_OK) return frc;
    auto buf = [&](int k) -> DevBuf& { return c->ac_bufs[k]; };
    out.grays_dev = buf(C_IMG).as<float>();
    // (BGR: the bytes are staged in the not yet used work image C_TMP)
    if ((frc = detect_upload(c, B, images, bgrs, n0, buf(C_IMG).as<float>(), buf(C_TMP).as<unsigned char>())) != R3DM_OK) return frc;
    std::vector<HalfTabs> half_tabs;
    if ((frc = detect_area_tabs(c, buf(C_TABS), lv, half_tabs)) != R3DM_OK) return frc;
    R3DM_HIP(c, hipEventRecord(c->ev0, st));
    if ((frc = ac_scale_space(c, B, lv, half_tabs, nullptr)) != R3DM_OK) return frc;
    AcExtrema ex;
    if ((frc = ac_find_extrema(c, B, lv, threshold, ex)) != R3DM_OK) return frc;
    const uint32_t stride = ex.stride;
    DevBuf &nsl = buf(C_NSL), &outs = buf(C_OUTS);
    AcLevelTab tab{};
    AcPlanes pl{};
    tab.n_levels = nl;
    tab.smax = (float)(10.0 * sqrtf(2.0f));
    for (int i = 0; i < nl; ++i) {
        tab.w[i] = lv[i].w; tab.h[i] = lv[i].h; tab.octave[i] = lv[i].octave;
        tab.esigma[i] = lv[i].esigma; tab.ratio[i] = lv[i].ratio; tab.off[i] = (float)(.5 * (lv[i].ratio - 1.0));
        pl.ldet[i] = ac_plane(c, i, 2); pl.lx[i] = ac_plane(c, i, 0); pl.ly[i] = ac_plane(c, i, 1);
    }
    for (int i = 0; i < nl; ++i) tab.row0[i] = ex.row0[i];
    // the candidates, their row offsets and totals are on the device: the walk, the upper-level filter, refinement and orientation.
    // R3DM_AC_AUX=0 (developer build): the one-wavefront walk over every candidate and the upper-level filter over every later slot.
    // R3DM_AC_AUX_BOUND (test hook): a smaller wavefront bound hands more components back to the one-wavefront walk.
    static const bool parallel = r3dm_dev_knob("R3DM_AC_AUX", 1) != 0;
    static const uint32_t bound = [] { const int v = r3dm_dev_knob("R3DM_AC_AUX_BOUND", 64); return (uint32_t)(v < 1 ? 1 : v > 64 ? 64 : v); }();
    uint32_t* hist = nullptr;
    if ((frc = ac_walk(c, B, w, h, tab, pl, stride, ex.rc, ex.rows_stride, ex.totals, parallel, bound, &hist)) != R3DM_OK) return frc;
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

#ifdef R3DM_DEVTOOLS
// ---- developer build only (libr3dm_dev.so; declared in no header): the walk on a caller's candidate lists, so that the suite can put the
// cases to the kernels that images cannot reach (equal responses, distances exactly on the boundary, component sizes at the wavefront
// bound, a slot that moved out of its cell).  The kernels that run are the product's: ac_walk above.
struct r3dm_dev_ac_level { int32_t w, h, octave; float esigma, ratio; };

// What the kernels would mis-read is refused here, before anything touches a device: R3DM_OK or R3DM_ERR_INVALID.
//   levels [n_levels <= kAcMaxLevels]: w, h >= 3; octave in 0 .. 6 and ratio = 2^octave (ac_finish_kernel converts with either); the
//   level fits the image (w ratio <= width, h ratio <= height, so a converted position stays inside the walk's grid); esigma finite;
//   size = 1.5 esigma with a cell side floor(size) + 1 >= 3, the side the grid's allocation assumes; the orientation's sample step and
//   the border test's agree (both are fRound(size / ratio), formed in double and in float: the border test then covers every read)
//   n_cand [B], cand: the B lists one after the other, (x = column, y = row, level, value), each in strict scan order (level, row,
//   column), rows 1 .. h - 2, columns 1 .. w - 2 of the candidate's level, finite values
//   parallel: 0 = one wavefront per image and the every-later-slot filter, 1 = the product's parallel form; bound: 1 .. 64
extern "C" int r3dm_dev_akaze_classic_walk_check(const r3dm_dev_ac_level* levels, uint32_t n_levels, uint32_t width, uint32_t height, uint32_t B,
                                                 const uint32_t* n_cand, const AcCand* cand, int parallel, uint32_t bound)
{
    if (!levels || !n_cand || n_levels < 1 || n_levels > (uint32_t)kAcMaxLevels || B < 1 || B > 1024u) return R3DM_ERR_INVALID;
    if (width < 3 || height < 3 || width > 65536u || height > 65536u) return R3DM_ERR_INVALID;
    if ((parallel != 0 && parallel != 1) || bound < 1 || bound > 64) return R3DM_ERR_INVALID;
    for (uint32_t l = 0; l < n_levels; ++l) {
        const r3dm_dev_ac_level& e = levels[l];
        if (e.w < 3 || e.h < 3 || e.octave < 0 || e.octave > 6) return R3DM_ERR_INVALID;
        if (!std::isfinite(e.esigma) || !(e.ratio == (float)(1 << e.octave))) return R3DM_ERR_INVALID;
        if ((double)e.w * e.ratio > (double)width || (double)e.h * e.ratio > (double)height) return R3DM_ERR_INVALID;
        const float size = e.esigma * 1.5f;
        if (!(size >= 2.0f) || size > 4096.0f) return R3DM_ERR_INVALID;             // cell side floor(size) + 1 >= 3
        if ((int)((float)(0.5 * (double)(size * 2.0f) / (double)e.ratio) + 0.5f) != (int)(size / e.ratio + 0.5f)) return R3DM_ERR_INVALID;
    }
    uint64_t at = 0;
    for (uint32_t b = 0; b < B; ++b) {
        if (n_cand[b] > (1u << 24) || (n_cand[b] && !cand)) return R3DM_ERR_INVALID;
        for (uint32_t k = 0; k < n_cand[b]; ++k) {
            const AcCand& p = cand[at + k];
            if (p.level >= n_levels || !std::isfinite(p.value)) return R3DM_ERR_INVALID;
            if (p.y < 1 || p.y > (uint32_t)levels[p.level].h - 2 || p.x < 1 || p.x > (uint32_t)levels[p.level].w - 2) return R3DM_ERR_INVALID;
            if (k) {
                const AcCand& q = cand[at + k - 1];
                const bool later = p.level != q.level ? p.level > q.level : p.y != q.y ? p.y > q.y : p.x > q.x;
                if (!later) return R3DM_ERR_INVALID;
            }
        }
        at += n_cand[b];
    }
    return R3DM_OK;
}

// Runs the lists through ac_walk.  The row offsets that ac_cc_link_kernel and the hand-back read (rows, rows_stride = n_rows + 1,
// tab.row0) are built from the lists here, on the host.  ac_finish_kernel fuses the upper-level filter with the refinement and the
// orientation, which read the level planes: it is handed ZEROED planes (one zeroed buffer stands for every plane).  The Hessian
// determinant around every slot is then 0, so the refinement shifts nothing and erases nothing, the orientation reads zeros inside the
// plane (a slot passed the border test: reach 10 sqrt 2 steps, the orientation's is 6), and AcOut.ok is the filter's verdict alone.
// Outputs: n_slots [B]; slots_out: six words per slot at the offsets of the candidate lists (image b's slots start at six times the
// sum of n_cand before b; n_slots[b] <= n_cand[b]): x, y, size, response as float, then class and the kept flag as uint32; hist
// [B x 32] (may be null): the parallel form's component-size histogram per image, zeros in the one-wavefront form.
extern "C" int r3dm_dev_akaze_classic_walk(r3dm_ctx* c, const r3dm_dev_ac_level* levels, uint32_t n_levels, uint32_t width, uint32_t height,
                                           uint32_t B, const uint32_t* n_cand, const AcCand* cand, int parallel, uint32_t bound,
                                           uint32_t* n_slots, uint32_t* slots_out, uint32_t* hist_out)
{
    const int vrc = r3dm_dev_akaze_classic_walk_check(levels, n_levels, width, height, B, n_cand, cand, parallel, bound);
    if (vrc != R3DM_OK) { if (c) c->err = "r3dm_dev_akaze_classic_walk: a level table, candidate list, form or bound the kernels would mis-read"; return vrc; }
    if (!c || !n_slots) return R3DM_ERR_INVALID;
    uint64_t total = 0;
    for (uint32_t b = 0; b < B; ++b) total += n_cand[b];
    if (total && !slots_out) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int {
        R3DM_HIP(c, hipSetDevice(c->device));
        hipStream_t st = c->stream;
        ac_bufs_init(c);
        auto buf = [&](int k) -> DevBuf& { return c->ac_bufs[k]; };
        const int w = (int)width, h = (int)height, nl = (int)n_levels;
        AcLevelTab tab{};
        AcPlanes pl{};
        tab.n_levels = nl;
        tab.smax = (float)(10.0 * sqrtf(2.0f));
        uint32_t n_rows = 0;
        size_t plane = 0;
        for (int i = 0; i < nl; ++i) {
            tab.w[i] = levels[i].w; tab.h[i] = levels[i].h; tab.octave[i] = levels[i].octave;
            tab.esigma[i] = levels[i].esigma; tab.ratio[i] = levels[i].ratio; tab.off[i] = (float)(.5 * (levels[i].ratio - 1.0));
            tab.row0[i] = n_rows; n_rows += (uint32_t)levels[i].h;
            plane = std::max(plane, (size_t)levels[i].w * levels[i].h);
        }
        DevBuf& zero = buf(C_TMP);
        plane = (size_t)B * plane + 4 * (size_t)width + 16;                          // (a spare row or two behind the last plane)
        R3DM_HIP(c, zero.ensure(plane * 4));
        R3DM_HIP(c, hipMemsetAsync(zero.p, 0, plane * 4, st));
        for (int i = 0; i < nl; ++i) pl.ldet[i] = pl.lx[i] = pl.ly[i] = zero.as<float>();
        // rows[r] = the candidates of the image before row r (levels one after the other), then the totals: what ac_scan_rows leaves
        const uint32_t rows_stride = n_rows + 1;
        std::vector<uint32_t> hrows((size_t)B * rows_stride + B, 0u);
        uint32_t stride = 1;
        uint64_t at = 0;
        for (uint32_t b = 0; b < B; ++b) {
            uint32_t* r = hrows.data() + (size_t)b * rows_stride;
            for (uint32_t k = 0; k < n_cand[b]; ++k) r[tab.row0[cand[at + k].level] + cand[at + k].y + 1]++;
            for (uint32_t q = 1; q <= n_rows; ++q) r[q] += r[q - 1];
            r[n_rows] = 0;                                                           // (ac_scan_rows writes n_rows offsets; the spare word stays 0)
            hrows[(size_t)B * rows_stride + b] = n_cand[b];
            stride = std::max(stride, n_cand[b]);
            at += n_cand[b];
        }
        DevBuf &rows = buf(C_ROWS), &cd = buf(C_CAND);
        R3DM_HIP(c, rows.ensure(hrows.size() * 4));
        R3DM_HIP(c, cd.ensure((size_t)B * stride * sizeof(AcCand)));
        uint32_t* rc = rows.as<uint32_t>();
        const uint32_t* totals = rc + (size_t)B * rows_stride;
        R3DM_HIP(c, hipMemcpyAsync(rc, hrows.data(), hrows.size() * 4, hipMemcpyHostToDevice, st));
        at = 0;
        for (uint32_t b = 0; b < B; ++b) {
            if (n_cand[b]) R3DM_HIP(c, hipMemcpyAsync(cd.as<AcCand>() + (size_t)b * stride, cand + at, (size_t)n_cand[b] * sizeof(AcCand), hipMemcpyHostToDevice, st));
            at += n_cand[b];
        }
        R3DM_HIP(c, hipStreamSynchronize(st));                                       // (the host arrays have been read)
        uint32_t* hist = nullptr;
        const int frc = ac_walk(c, B, w, h, tab, pl, stride, rc, rows_stride, totals, parallel != 0, bound, &hist);
        if (frc != R3DM_OK) { (void)hipStreamSynchronize(st); return frc; }
        std::vector<uint32_t> hs((size_t)B * 32, 0u);
        R3DM_HIP(c, hipMemcpyAsync(n_slots, buf(C_NSL).p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        if (hist) R3DM_HIP(c, hipMemcpyAsync(hs.data(), hist, hs.size() * 4, hipMemcpyDeviceToHost, st));
        R3DM_HIP(c, hipStreamSynchronize(st));
        if (hist_out) std::copy(hs.begin(), hs.end(), hist_out);
        at = 0;
        for (uint32_t b = 0; b < B; ++b) {
            if (n_slots[b] > n_cand[b]) { c->err = "r3dm_dev_akaze_classic_walk: more slots than candidates"; return R3DM_ERR_INVALID; }
            std::vector<AcSlot> sl(n_slots[b]);
            std::vector<AcOut> ou(n_slots[b]);
            if (n_slots[b]) {
                R3DM_HIP(c, hipMemcpyAsync(sl.data(), buf(C_SLOTS).as<AcSlot>() + (size_t)b * stride, sl.size() * sizeof(AcSlot), hipMemcpyDeviceToHost, st));
                R3DM_HIP(c, hipMemcpyAsync(ou.data(), buf(C_OUTS).as<AcOut>() + (size_t)b * stride, ou.size() * sizeof(AcOut), hipMemcpyDeviceToHost, st));
            }
            R3DM_HIP(c, hipStreamSynchronize(st));
            for (uint32_t q = 0; q < n_slots[b]; ++q) {
                uint32_t* o = slots_out + 6 * (at + q);
                memcpy(o, &sl[q], 16);                                               // x, y, size, response
                o[4] = sl[q].cls; o[5] = ou[q].ok;
            }
            at += n_cand[b];
        }
        return R3DM_OK;
    });
}

// ---- the head, plane by plane ("The head, plane by plane"): the entries below run ac_scale_space and
// ac_find_extrema, the functions the detector calls, and read back what the detector only passes on.
constexpr uint32_t kAcDevSmallOut = 309;             // hmax bits, 300 bins, 1 / k^2 of octaves 0 .. 7

// the level table of an image size (needs no device): levels_out [<= 16], *n_levels_out
extern "C" int r3dm_dev_akaze_classic_levels(uint32_t width, uint32_t height, r3dm_dev_ac_level* levels_out, uint32_t* n_levels_out)
{
    if (!levels_out || !n_levels_out || width < 3 || height < 3 || width > 65536u || height > 65536u) return R3DM_ERR_INVALID;
    const std::vector<AkLevelHost> lv = ac_levels((int)width, (int)height);
    for (size_t i = 0; i < lv.size(); ++i) levels_out[i] = r3dm_dev_ac_level{lv[i].w, lv[i].h, lv[i].octave, lv[i].esigma, lv[i].ratio};
    *n_levels_out = (uint32_t)lv.size();
    return R3DM_OK;
}

// Refused before anything touches a device (R3DM_OK or R3DM_ERR_INVALID): B outside 1 .. 1024, a dimension below 3 (no 3 x 3 maximum
// exists; the FED step's corner forms read a neighbour on either axis) or above 65536, a null image array or image, a value that is
// not finite or lies outside [0, 1].  Every kernel of the head addresses by the plane's own (w, h) alone -- clamped or reflected taps,
// one-sided fluxes on the rim -- and the histogram's bin floor(300 (modg / hmax)) of a finite modulus <= hmax lies in 0 .. 300, folded
// to 299.
extern "C" int r3dm_dev_akaze_classic_head_check(uint32_t B, const float* const* images, uint32_t width, uint32_t height)
{
    if (!images || B < 1 || B > 1024u) return R3DM_ERR_INVALID;
    if (width < 3 || height < 3 || width > 65536u || height > 65536u) return R3DM_ERR_INVALID;
    const size_t n0 = (size_t)width * height;
    for (uint32_t b = 0; b < B; ++b) {
        if (!images[b]) return R3DM_ERR_INVALID;
        for (size_t k = 0; k < n0; ++k) if (!(images[b][k] >= 0.0f && images[b][k] <= 1.0f)) return R3DM_ERR_INVALID;    // (false for a NaN too)
    }
    return R3DM_OK;
}

// Refused (R3DM_OK or R3DM_ERR_INVALID): B outside 1 .. 1024, an image size below 3 or above 65536, n_levels or plane_dims [n_levels][2]
// (w, h) other than the table's of (width, height), a null array or plane.  planes [B][n_levels].  Any VALUE is taken, NaN and the
// infinities included: ac_extrema_kernel only compares them (rows 1 .. h - 2, columns 1 .. w - 2 and their eight neighbours, inside a
// plane of the table's size).
extern "C" int r3dm_dev_akaze_classic_extrema_check(uint32_t width, uint32_t height, uint32_t B, uint32_t n_levels, const uint32_t* plane_dims,
                                                    const float* const* planes)
{
    if (!plane_dims || !planes || B < 1 || B > 1024u) return R3DM_ERR_INVALID;
    if (width < 3 || height < 3 || width > 65536u || height > 65536u) return R3DM_ERR_INVALID;
    const std::vector<AkLevelHost> lv = ac_levels((int)width, (int)height);
    if (n_levels != lv.size()) return R3DM_ERR_INVALID;
    for (size_t i = 0; i < lv.size(); ++i)
        if (plane_dims[2 * i] != (uint32_t)lv[i].w || plane_dims[2 * i + 1] != (uint32_t)lv[i].h) return R3DM_ERR_INVALID;
    for (size_t k = 0; k < (size_t)B * n_levels; ++k) if (!planes[k]) return R3DM_ERR_INVALID;
    return R3DM_OK;
}

// what both entries read back once ac_find_extrema has run: counts_out [B][nl] (from the scanned row offsets: a level's count is the
// offset of the next level's first row less its own; the last level's ends at the image's total), n_out [B] and cand_out [B][cap]
// (x, y, level, value bits; image b's candidates from b cap on, in scan order)
static int ac_dev_read_candidates(r3dm_ctx* c, uint32_t B, int nl, const AcExtrema& ex, uint32_t cap, uint32_t* counts_out, uint32_t* n_out,
                                  uint32_t* cand_out)
{
    hipStream_t st = c->stream;
    std::vector<uint32_t> hrc((size_t)B * ex.rows_stride);
    R3DM_HIP(c, hipMemcpyAsync(hrc.data(), ex.rc, hrc.size() * 4, hipMemcpyDeviceToHost, st));
    for (uint32_t b = 0; b < B; ++b) {
        if (ex.tot[b] > cap) { c->err = "developer classic head entry: more candidates than the caller's bound"; return R3DM_ERR_INVALID; }
        if (ex.tot[b]) R3DM_HIP(c, hipMemcpyAsync(cand_out + 4 * (size_t)b * cap, c->ac_bufs[C_CAND].as<AcCand>() + (size_t)b * ex.stride,
                                                  (size_t)ex.tot[b] * sizeof(AcCand), hipMemcpyDeviceToHost, st));
    }
    R3DM_HIP(c, hipStreamSynchronize(st));
    for (uint32_t b = 0; b < B; ++b) {
        const uint32_t* r = hrc.data() + (size_t)b * ex.rows_stride;
        n_out[b] = ex.tot[b];
        for (int i = 0; i < nl; ++i) counts_out[(size_t)b * nl + i] = (i + 1 < nl ? r[ex.row0[i + 1]] : ex.tot[b]) - r[ex.row0[i]];
    }
    return R3DM_OK;
}

// The classic head on the caller's B same-size images in [0, 1]: the detector's upload, ac_scale_space with a tap, ac_find_extrema.
//   small_out [B][309]: the bits of the largest gradient modulus, the 300 histogram bins, the bits of 1 / k^2 of octaves 0 .. 7
//   planes_out [B][n_levels][6]: Lsmooth, Lflow (level 0 has none: left untouched), Lt as the level's FED steps leave it, Lx, Ly, Ldet
//   (the caller's, w_i x h_i floats each); counts_out, n_out, cand_out: ac_dev_read_candidates, cap candidates per image
extern "C" int r3dm_dev_akaze_classic_head(r3dm_ctx* c, uint32_t B, const float* const* images, uint32_t width, uint32_t height, float threshold,
                                           uint32_t* small_out, float* const* planes_out, uint32_t* counts_out, uint32_t cap, uint32_t* n_out,
                                           uint32_t* cand_out)
{
    const int vrc = r3dm_dev_akaze_classic_head_check(B, images, width, height);
    if (vrc != R3DM_OK) { if (c) c->err = "r3dm_dev_akaze_classic_head: images the entry does not take"; return vrc; }
    if (!c || !small_out || !planes_out || !counts_out || !n_out || !cand_out) return R3DM_ERR_INVALID;
    const std::vector<AkLevelHost> lv = ac_levels((int)width, (int)height);
    const int nl = (int)lv.size();
    for (size_t k = 0; k < (size_t)B * nl * 6; ++k) if (!planes_out[k]) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int {
        R3DM_HIP(c, hipSetDevice(c->device));
        hipStream_t st = c->stream;
        int rc = ac_head_bufs(c, B, lv);
        if (rc != R3DM_OK) return rc;
        auto buf = [&](int k) -> DevBuf& { return c->ac_bufs[k]; };
        const size_t n0 = (size_t)width * height;
        if ((rc = detect_upload(c, B, images, nullptr, n0, buf(C_IMG).as<float>(), buf(C_TMP).as<unsigned char>())) != R3DM_OK) return rc;
        std::vector<HalfTabs> half_tabs;
        if ((rc = detect_area_tabs(c, buf(C_TABS), lv, half_tabs)) != R3DM_OK) return rc;
        const AcTap tap = [&](int i, const float* smooth, const float* flow, const float* lt) -> int {
            const size_t plane = (size_t)lv[i].w * lv[i].h;
            for (uint32_t b = 0; b < B; ++b) {
                float* const* P = planes_out + ((size_t)b * nl + i) * 6;
                R3DM_HIP(c, hipMemcpyAsync(P[0], smooth + b * plane, plane * 4, hipMemcpyDeviceToHost, st));
                if (flow) R3DM_HIP(c, hipMemcpyAsync(P[1], flow + b * plane, plane * 4, hipMemcpyDeviceToHost, st));
                R3DM_HIP(c, hipMemcpyAsync(P[2], lt + b * plane, plane * 4, hipMemcpyDeviceToHost, st));
            }
            R3DM_HIP(c, hipStreamSynchronize(st));                                   // (the work buffers are free for the next level)
            return R3DM_OK;
        };
        if ((rc = ac_scale_space(c, B, lv, half_tabs, &tap)) != R3DM_OK) { (void)hipStreamSynchronize(st); return rc; }
        AcExtrema ex;
        if ((rc = ac_find_extrema(c, B, lv, threshold, ex)) != R3DM_OK) { (void)hipStreamSynchronize(st); return rc; }
        for (uint32_t b = 0; b < B; ++b) {
            for (int i = 0; i < nl; ++i) {
                const size_t plane = (size_t)lv[i].w * lv[i].h;
                float* const* P = planes_out + ((size_t)b * nl + i) * 6;
                for (int q = 0; q < 3; ++q) R3DM_HIP(c, hipMemcpyAsync(P[3 + q], ac_plane(c, i, q) + b * plane, plane * 4, hipMemcpyDeviceToHost, st));
            }
            uint32_t* S = small_out + (size_t)b * kAcDevSmallOut;
            const uint32_t* D = buf(C_SMALL).as<uint32_t>() + (size_t)b * 4096;
            R3DM_HIP(c, hipMemcpyAsync(S, D, 4, hipMemcpyDeviceToHost, st));
            R3DM_HIP(c, hipMemcpyAsync(S + 1, D + 16, 300 * 4, hipMemcpyDeviceToHost, st));
            R3DM_HIP(c, hipMemcpyAsync(S + 301, D + 1024, 8 * 4, hipMemcpyDeviceToHost, st));
        }
        return ac_dev_read_candidates(c, B, nl, ex, cap, counts_out, n_out, cand_out);
    });
}

// ac_find_extrema on the caller's Ldet planes (planes [B][n_levels], the level table of width x height); the outputs are
// ac_dev_read_candidates'.
extern "C" int r3dm_dev_akaze_classic_extrema(r3dm_ctx* c, uint32_t width, uint32_t height, uint32_t B, uint32_t n_levels,
                                              const uint32_t* plane_dims, const float* const* planes, float threshold, uint32_t* counts_out,
                                              uint32_t cap, uint32_t* n_out, uint32_t* cand_out)
{
    const int vrc = r3dm_dev_akaze_classic_extrema_check(width, height, B, n_levels, plane_dims, planes);
    if (vrc != R3DM_OK) { if (c) c->err = "r3dm_dev_akaze_classic_extrema: planes the kernels would mis-read"; return vrc; }
    if (!c || !counts_out || !n_out || !cand_out) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int {
        R3DM_HIP(c, hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const std::vector<AkLevelHost> lv = ac_levels((int)width, (int)height);
        const int nl = (int)lv.size();
        int rc = ac_head_bufs(c, B, lv);
        if (rc != R3DM_OK) return rc;
        for (int i = 0; i < nl; ++i) {
            const size_t plane = (size_t)lv[i].w * lv[i].h;
            for (uint32_t b = 0; b < B; ++b)
                R3DM_HIP(c, hipMemcpyAsync(ac_plane(c, i, 2) + b * plane, planes[(size_t)b * nl + i], plane * 4, hipMemcpyHostToDevice, st));
        }
        R3DM_HIP(c, hipStreamSynchronize(st));                                       // (the host planes have been read)
        AcExtrema ex;
        if ((rc = ac_find_extrema(c, B, lv, threshold, ex)) != R3DM_OK) { (void)hipStreamSynchronize(st); return rc; }
        return ac_dev_read_candidates(c, B, nl, ex, cap, counts_out, n_out, cand_out);
    });
}
#endif  // R3DM_DEVTOOLS
