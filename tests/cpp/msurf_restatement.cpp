// msurf_restatement.cpp -- TEST INFRASTRUCTURE: the M-SURF-64 descriptor of the vendored Fast-A-KAZE restated for the CPU, one keypoint at
// a time and strictly serially, after MSURF_Descriptor_64_InvokerV2::Get_MSURF_Descriptor_64
// (src/thirdparty/fast-akaze/AKAZEFeatures.cpp:1431-1544) with gaussianV2 and fRoundV2 of utils.h:28-30,65-67.  Written apart from the
// kernel (regard3d_amd/csrc/kernels_akaze.hip: ak_msurf_kernel); the two share ak_expf.hpp and nothing else.
// Built by the tests with g++ -O2 -ffp-contract=off:
//   as a shared library (the msurf_* functions below, called through ctypes by tests/msurf_cases.py), every plane read checked;
//   with -DMSURF_MAIN as a stand-alone program that runs the border cases on exactly-sized heap planes WITHOUT that check, so that
//   an address sanitizer is the judge of "no read leaves a plane" (tests/test_msurf_cases.py).
// use_libm = 1: the exponential is libm's expf, as in the reference; 0: ak_expf, as in the kernel.
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../regard3d_amd/csrc/ak_expf.hpp"

namespace {

struct Plane { const float* p; int w, h; bool left; };

inline float at(Plane& P, int y, int x)
{
#ifndef MSURF_MAIN
    if (x < 0 || y < 0 || x >= P.w || y >= P.h) { P.left = true; return 0.0f; }
#endif
    return P.p[(size_t)y * P.w + x];
}

inline int f_round(float v) { return (int)(v + 0.5f); }                      // fRoundV2

struct Expo {
    int use_libm; float lo, hi; float* args; int n;
    float operator()(float a)
    {
        assert(a >= -4.1f && a <= 0.0f);            // sigma = 2.5 scale, squared distance <= 50 scale^2; the subregion weights >= -1
        if (a < lo) lo = a;
        if (a > hi) hi = a;
        if (args) args[n] = a;
        ++n;
        return use_libm ? expf(a) : ak_expf(a);
    }
};

inline float gaussian(Expo& E, float x, float y, float sigma) { return E(-(x * x + y * y) / (2.0f * sigma * sigma)); }   // gaussianV2

// one keypoint: level coordinates (xf, yf) = pt / ratio, co / si = cos / sin of its angle, scale = fRound(0.5 size / ratio)
int restate(const float* lx, const float* ly, int w, int h, float xf, float yf, float co, float si, int scale, int use_libm, float* desc,
            float* args_out /* 1312 or null */, float* arg_range /* 2 or null */)
{
    Plane X{lx, w, h, false}, Y{ly, w, h, false};
    Expo E{use_libm, 0.0f, -100.0f, args_out, 0};
    const int sample_step = 5, pattern_size = 12;
    float len = 0.0f;
    int dcount = 0;
    float cx = -0.5f;
    // the 4 x 4 subregions: rows i .. i + 8 for i = -12, -7, -2, 3 (:1459-1465,1535), columns j alike (:1464,1473,1532)
    for (int i = -pattern_size; i + 9 <= pattern_size; i += sample_step) {
        cx += 1.0f;
        float cy = -0.5f;
        for (int j = -pattern_size; j + 9 <= pattern_size; j += sample_step) {
            float dx = 0.0f, dy = 0.0f, mdx = 0.0f, mdy = 0.0f;
            cy += 1.0f;
            const int ky = i + sample_step, kx = j + sample_step;
            const float xs = xf + (-kx * scale * si + ky * scale * co);          // :1478-1479 (int products, then float)
            const float ys = yf + (kx * scale * co + ky * scale * si);
            for (int k = i; k < i + 9; ++k)
                for (int l = j; l < j + 9; ++l) {
                    const float sample_y = yf + (l * scale * co + k * scale * si);  // :1484-1485
                    const float sample_x = xf + (-l * scale * si + k * scale * co);
                    const float gauss_s1 = gaussian(E, xs - sample_x, ys - sample_y, 2.5f * scale);
                    const int y1 = f_round(sample_y - 0.5f), x1 = f_round(sample_x - 0.5f);
                    const int y2 = f_round(sample_y + 0.5f), x2 = f_round(sample_x + 0.5f);
                    const float fx = sample_x - x1, fy = sample_y - y1;
                    float r1 = at(X, y1, x1), r2 = at(X, y1, x2), r3 = at(X, y2, x1), r4 = at(X, y2, x2);
                    const float rx = (1.0f - fx) * (1.0f - fy) * r1 + fx * (1.0f - fy) * r2 + (1.0f - fx) * fy * r3 + fx * fy * r4;
                    r1 = at(Y, y1, x1); r2 = at(Y, y1, x2); r3 = at(Y, y2, x1); r4 = at(Y, y2, x2);
                    const float ry = (1.0f - fx) * (1.0f - fy) * r1 + fx * (1.0f - fy) * r2 + (1.0f - fx) * fy * r3 + fx * fy * r4;
                    const float rry = gauss_s1 * (rx * co + ry * si);               // :1512-1513
                    const float rrx = gauss_s1 * (-rx * si + ry * co);
                    dx += rrx; dy += rry;
                    mdx += fabsf(rrx); mdy += fabsf(rry);
                }
            const float gauss_s2 = gaussian(E, cx - 2.0f, cy - 2.0f, 1.5f);
            desc[dcount++] = dx * gauss_s2;
            desc[dcount++] = dy * gauss_s2;
            desc[dcount++] = mdx * gauss_s2;
            desc[dcount++] = mdy * gauss_s2;
            len += (dx * dx + dy * dy + mdx * mdx + mdy * mdy) * gauss_s2 * gauss_s2;
        }
    }
    len = sqrtf(len);                                                            // :1539 (sqrt of a float: the same value)
    for (int q = 0; q < 64; ++q) desc[q] /= len;                                  // 0 / 0 = NaN for a window without gradient, as there
    if (arg_range) { arg_range[0] = E.lo; arg_range[1] = E.hi; }
    assert(dcount == 64 && E.n == 1312);
    return (X.left || Y.left) ? 1 : 0;
}

}  // namespace

#ifndef MSURF_MAIN
// n keypoints on planes of one level.  items: n x 5 floats (xf, yf, co, si, scale as a float holding the int).  Returns the number of
// keypoints any of whose reads left the plane (their rows then hold what a zero outside gives: the caller asserts 0).
extern "C" int msurf_restate(const float* lx, const float* ly, int w, int h, int n, const float* items, int use_libm, float* desc_out,
                             float* args_out, float* arg_range_out)
{
    int left = 0;
    float lo = 0.0f, hi = -100.0f;
    for (int k = 0; k < n; ++k) {
        const float* it = items + 5 * k;
        float r[2];
        left += restate(lx, ly, w, h, it[0], it[1], it[2], it[3], (int)it[4], use_libm, desc_out + 64 * (size_t)k,
                        args_out ? args_out + 1312 * (size_t)k : nullptr, r);
        if (r[0] < lo) lo = r[0];
        if (r[1] > hi) hi = r[1];
    }
    if (arg_range_out) { arg_range_out[0] = lo; arg_range_out[1] = hi; }
    return left;
}

extern "C" void msurf_expf(const float* x, int n, int use_libm, float* out)
{
    for (int k = 0; k < n; ++k) out[k] = use_libm ? expf(x[k]) : ak_expf(x[k]);
}

#else
// stand-alone: argv = w h n, then stdin holds n lines "xf yf co si scale"; the planes are a fixed pattern on the heap, exactly w x h
// floats each.  Prints one checksum line per keypoint.  Every read is unchecked: run it under -fsanitize=address,undefined.
int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: msurf_restatement w h n < items\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), n = atoi(argv[3]);
    if (w < 1 || h < 1 || n < 0) return 2;
    float* lx = (float*)malloc(sizeof(float) * (size_t)w * h);
    float* ly = (float*)malloc(sizeof(float) * (size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) { lx[(size_t)y * w + x] = 0.01f * (float)((x * 7 + y * 3) % 19 - 9); ly[(size_t)y * w + x] = 0.01f * (float)((x * 5 + y * 11) % 23 - 11); }
    for (int k = 0; k < n; ++k) {
        float xf, yf, co, si; int scale;
        if (scanf("%f %f %f %f %d", &xf, &yf, &co, &si, &scale) != 5) return 2;
        float desc[64];
        for (int use_libm = 0; use_libm < 2; ++use_libm) {
            restate(lx, ly, w, h, xf, yf, co, si, scale, use_libm, desc, nullptr, nullptr);
            double s = 0.0;
            for (int q = 0; q < 64; ++q) s += (double)desc[q] * desc[q];
            printf("%d %d %.9g\n", k, use_libm, s);
        }
    }
    free(lx); free(ly);
    printf("done %d\n", n);
    return 0;
}
#endif
