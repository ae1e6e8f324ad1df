// api_liop.cpp -- part of the host side of libr3dm.so (see r3dm_ctx.hpp for the file map): the LIOP descriptor (kernels_liop.hip).
// The patch geometry tables, the patch map of a keypoint, the ONE pass from keypoints to descriptors (liop_pass: the features batch and
// r3dm_extract_liop run it) and the entries r3dm_liop_describe_patches / r3dm_extract_liop.
#include "r3dm_ctx.hpp"

// geometry of the 41x41 patch exactly as vl_liopdesc_new builds it (vl_liop.c:371-421): circular support
// dx^2+dy^2 <= (long)((center - radius + 0.6)^2), 4 samples per pixel on a circle of radius 6 starting at
// atan2(y, x); computed once on the host with the host libm (like the reference) and kept in HBM
static int liop_prepare(r3dm_ctx* c)
{
    if (c->liop_npix) return R3DM_OK;
    const int side = 41, center = (side - 1) / 2;
    const double radius = 6.0, t = center - radius + 0.6;
    const long t2 = (long)(t * t);
    std::vector<int> pix;
    for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x) {
            const long dx = x - center, dy = y - center;
            if (x == 0 && y == 0) continue;
            if (dx * dx + dy * dy <= t2) pix.push_back(x + y * side);
        }
    if (pix.size() > 1024) { c->err = "liop: support larger than the sort capacity"; return R3DM_ERR_UNSUPPORTED; }
    // per support pixel: the four sample positions as (offset of the top-left tap, fractional parts).  The kernel keeps the patch with
    // a ring of zeros (43 x 43), so vl_liop's guarded taps (:516-535: `if (ix >= 0 && iy >= 0) a = ...`) are plain reads; floor and
    // fraction are the reference's own double operations, done once here instead of once per sample and keypoint
    std::vector<double> sw(8 * pix.size());
    std::vector<int> so(4 * pix.size()), pixr(pix.size());
    const double dangle = 2 * M_PI / 4.0;
    for (size_t i = 0; i < pix.size(); ++i) {
        const double x = (pix[i] % side) - center, y = (pix[i] / side) - center;
        const double angle0 = std::atan2(y, x);
        pixr[i] = (pix[i] % side + 1) + (pix[i] / side + 1) * 43;
        for (int k = 0; k < 4; ++k) {
            const double sx = x + radius * std::cos(angle0 + dangle * k) + center;
            const double sy = y + radius * std::sin(angle0 + dangle * k) + center;
            const long xi = (long)sx, yi = (long)sy;
            const long ix = (sx >= 0 || (double)xi == sx) ? xi : xi - 1;          // vl_floor_d
            const long iy = (sy >= 0 || (double)yi == sy) ? yi : yi - 1;
            if (ix < -1 || ix > side - 1 || iy < -1 || iy > side - 1) { c->err = "liop: a sample leaves the ringed patch"; return R3DM_ERR_UNSUPPORTED; }
            sw[8 * i + 2 * k] = sx - ix; sw[8 * i + 2 * k + 1] = sy - iy;
            so[4 * i + k] = (int)((ix + 1) + (iy + 1) * 43);
        }
    }
    R3DM_HIP(c, c->liop_pix.ensure(pixr.size() * 4));
    R3DM_HIP(c, c->liop_sx.ensure(sw.size() * 8));
    R3DM_HIP(c, c->liop_sy.ensure(so.size() * 4));
    R3DM_HIP(c, hipMemcpyAsync(c->liop_pix.p, pixr.data(), pixr.size() * 4, hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(c->liop_sx.p, sw.data(), sw.size() * 8, hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(c->liop_sy.p, so.data(), so.size() * 4, hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    c->liop_npix = (uint32_t)pix.size();
    return R3DM_OK;
}

// cv::getGaussianKernel(11, 1.2, CV_32F): the blur of every LIOP patch (src/Regard3DFeatures.cpp:807)
static void liop_blur_taps(float (&kern)[11])
{
    const double scale2X = -0.5 / (1.2 * 1.2);
    double sum = 0;
    for (int i = 0; i < 11; ++i) { const double xx = i - 5.0; kern[i] = (float)std::exp(scale2X * xx * xx); sum += kern[i]; }
    sum = 1. / sum;
    for (int i = 0; i < 11; ++i) kern[i] = (float)(kern[i] * sum);
}

// exactly as src/Regard3DFeatures.cpp:786-799 computes it
void liop_patch_map(float x, float y, float size, float angle_deg, float kp_size_factor, float* m)
{
    const int patchResolution = 20, patchSize = 41;
    const float angle = -90.0f - angle_deg;
    const float scale = size / static_cast<float>(patchSize) * kp_size_factor;
    const float alpha = scale * std::cos(angle * M_PI / 180.0f);
    const float beta = scale * std::sin(angle * M_PI / 180.0f);
    const float trans_x = x - static_cast<float>(patchResolution), trans_y = y - static_cast<float>(patchResolution);
    m[0] = alpha; m[1] = beta;  m[2] = beta * trans_y + alpha * trans_x - beta * y + (1.0f - alpha) * x;
    m[3] = -beta; m[4] = alpha; m[5] = alpha * trans_y - beta * trans_x + beta * x + (1.0f - alpha) * y;
}

static inline LiopTables liop_tables(const r3dm_ctx* c)
{
    return LiopTables{c->liop_pix.as<int>(), c->liop_sx.as<double>(), c->liop_sy.as<int>(), c->liop_npix};
}

// the descriptor launch over the n patches in liop_in -> liop_out; liop_cnt = [tie count | ...][tie list: n]
static hipError_t liop_describe(r3dm_ctx* c, uint32_t n)
{
    return launch_liop(c->stream, liop_tables(c), c->liop_in.as<float>(), n, c->liop_out.as<float>(), c->liop_cnt.as<uint32_t>(), c->liop_cnt.as<uint32_t>() + 16);
}

void liop_read_time(r3dm_ctx* c)
{
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.ms_liop_kernel = ms;
}

int liop_pass(r3dm_ctx* c, const float* dev_images, uint32_t width, uint32_t height, const float* M6, const uint32_t* img_of, uint32_t n,
              bool want_patches)
{
    const int rc = liop_prepare(c);
    if (rc != R3DM_OK) return rc;
    float kern[11];
    liop_blur_taps(kern);
    static const int fused_knob = r3dm_dev_knob("R3DM_LIOP_FUSED", 1);     // developer build: 0 = patches through HBM (two kernels)
    const bool via_patches = want_patches || !fused_knob;
    const size_t m_bytes = (size_t)n * 6 * 4;
    R3DM_HIP(c, c->liop_M.ensure(m_bytes + (img_of ? (size_t)n * 4 : 0)));
    R3DM_HIP(c, c->liop_kern.ensure(64));
    if (via_patches) R3DM_HIP(c, c->liop_in.ensure((size_t)n * 41 * 41 * 4));
    R3DM_HIP(c, c->liop_out.ensure((size_t)n * 144 * 4));
    R3DM_HIP(c, c->liop_cnt.ensure(64 + (size_t)n * 4));
    uint32_t* d_img_of = img_of ? reinterpret_cast<uint32_t*>(c->liop_M.as<float>() + (size_t)n * 6) : nullptr;
    R3DM_HIP(c, hipMemcpyAsync(c->liop_M.p, M6, m_bytes, hipMemcpyHostToDevice, c->stream));
    if (img_of) R3DM_HIP(c, hipMemcpyAsync(d_img_of, img_of, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(c->liop_kern.p, kern, sizeof(kern), hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipMemsetAsync(c->liop_cnt.p, 0, 64, c->stream));
    R3DM_HIP(c, hipEventRecord(c->ev0, c->stream));
    // the patches only exist in HBM when the caller asks for them (or the developer build's R3DM_LIOP_FUSED=0): otherwise the warp + blur
    // runs inside the descriptor kernel's wavefront
    if (via_patches) {
        R3DM_HIP(c, launch_liop_extract(c->stream, dev_images, (int)width, (int)height, c->liop_M.as<float>(), c->liop_kern.as<float>(), n,
                                        c->liop_in.as<float>(), d_img_of));
        R3DM_HIP(c, liop_describe(c, n));
    } else {
        R3DM_HIP(c, launch_liop_fused(c->stream, liop_tables(c), dev_images, (int)width, (int)height, c->liop_M.as<float>(), c->liop_kern.as<float>(), d_img_of,
                                      n, c->liop_out.as<float>(), c->liop_cnt.as<uint32_t>(), c->liop_cnt.as<uint32_t>() + 16));
    }
    R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
    return R3DM_OK;
}

extern "C" int r3dm_liop_describe_patches(r3dm_ctx* c, const float* patches, uint32_t n, uint32_t side, float* desc_out,
                                          uint32_t* n_resorted)
{
    return r3dm_guarded(c, [&]() -> int {
        if (!c || (n && (!patches || !desc_out))) return R3DM_ERR_INVALID;
        if (side != 41) { c->err = "liop: only the 41x41 patch of Regard3D (patchResolution 20) is supported"; return R3DM_ERR_UNSUPPORTED; }
        R3DM_HIP(c, hipSetDevice(c->device));
        const int rc = liop_prepare(c);
        if (rc != R3DM_OK) return rc;
        if (n_resorted) *n_resorted = 0;
        if (n == 0) return R3DM_OK;
        const size_t in_bytes = (size_t)n * 41 * 41 * 4, out_bytes = (size_t)n * 144 * 4;
        R3DM_HIP(c, c->liop_in.ensure(in_bytes));
        R3DM_HIP(c, c->liop_out.ensure(out_bytes));
        R3DM_HIP(c, c->liop_cnt.ensure(64 + (size_t)n * 4));
        R3DM_HIP(c, hipMemcpyAsync(c->liop_in.p, patches, in_bytes, hipMemcpyDefault, c->stream));
        R3DM_HIP(c, hipMemsetAsync(c->liop_cnt.p, 0, 64, c->stream));
        R3DM_HIP(c, hipEventRecord(c->ev0, c->stream));
        R3DM_HIP(c, liop_describe(c, n));
        R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(desc_out, c->liop_out.p, out_bytes, hipMemcpyDefault, c->stream));
        uint32_t nt = 0;
        R3DM_HIP(c, hipMemcpyAsync(&nt, c->liop_cnt.p, 4, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        if (n_resorted) *n_resorted = nt;
        liop_read_time(c);
        return R3DM_OK;
    });
}

extern "C" int r3dm_extract_liop(r3dm_ctx* c, const float* image, uint32_t width, uint32_t height,
                                 const float* keypoints, uint32_t n, float kp_size_factor, float* desc_out, float* patches_out)
{
    return r3dm_guarded(c, [&]() -> int {
        if (!c || !image || width == 0 || height == 0 || (n && (!keypoints || !desc_out))) return R3DM_ERR_INVALID;
        R3DM_HIP(c, hipSetDevice(c->device));
        int rc = liop_prepare(c);
        if (rc != R3DM_OK) return rc;
        if (n == 0) return R3DM_OK;
        // keypoints to the host (they may live in device memory), 2x3 inverse maps exactly as :786-799 computes them
        std::vector<float> kp(4 * (size_t)n), M6(6 * (size_t)n);
        R3DM_HIP(c, hipMemcpyAsync(kp.data(), keypoints, kp.size() * 4, hipMemcpyDefault, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < n; ++k) liop_patch_map(kp[4 * k], kp[4 * k + 1], kp[4 * k + 2], kp[4 * k + 3], kp_size_factor, &M6[6 * (size_t)k]);
        const size_t img_bytes = (size_t)width * height * 4;
        R3DM_HIP(c, c->liop_img.ensure(img_bytes));
        R3DM_HIP(c, hipMemcpyAsync(c->liop_img.p, image, img_bytes, hipMemcpyDefault, c->stream));
        rc = liop_pass(c, c->liop_img.as<float>(), width, height, M6.data(), nullptr, n, patches_out != nullptr);
        if (rc != R3DM_OK) return rc;
        R3DM_HIP(c, hipMemcpyAsync(desc_out, c->liop_out.p, (size_t)n * 144 * 4, hipMemcpyDefault, c->stream));
        if (patches_out) R3DM_HIP(c, hipMemcpyAsync(patches_out, c->liop_in.p, (size_t)n * 41 * 41 * 4, hipMemcpyDefault, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        liop_read_time(c);
        return R3DM_OK;
    });
}
