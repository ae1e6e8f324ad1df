// ak_expf.hpp -- the one exponential of the M-SURF-64 descriptor (gaussianV2, fast-akaze utils.h:28-30), for host and device alike.
// The reference calls libm's expf, which no device function reproduces bit for bit.  ak_expf is evaluated in DOUBLE with nothing but
// +, - and * of IEEE binary64 (and one rint, exact by definition), which give the same bits on a CPU and on a GPU, and is rounded to
// float once at the end; so the kernel (kernels_akaze.hip) and the CPU restatement of the tests (tests/cpp/msurf_restatement.cpp), which
// share this header and nothing else, can agree bit for bit.  Every translation unit that includes it is built with -ffp-contract=off:
// a fused multiply-add on one side only would break that.
//   x = k ln2 + r, k = rint(x log2 e), |r| <= ln2 / 2 (+ a rounding); ln2 = ln2HI + ln2LO as in fdlibm's e_exp.c (k ln2HI is exact:
//   ln2HI has 21 trailing zero bits, |k| <= 6 here);
//   exp(r) by Horner over the Taylor coefficients 1 / n! up to n = 14: the first omitted term is (ln2 / 2)^15 / 15! = 9.6e-20 < 2^-60;
//   2^k from its bits.
// The double result is within about 2^-52 of exp(x), so the float is the correctly rounded one except where exp(x) lies within that
// of a rounding boundary: at most 0.5 + 2^-28 ulp.  Arguments: [-4.1, 0] is what M-SURF produces (sigma = 2.5 scale, squared
// distance <= 50 scale^2; the 16 subregion weights have arguments >= -1); the function itself is good for any |x| < 700.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define AK_EXPF_FN __host__ __device__ inline
#else
#define AK_EXPF_FN inline
#endif

AK_EXPF_FN float ak_expf(float x)
{
    const double xd = (double)x;
    const double k = rint(xd * 1.44269504088896338700e+00);
    const double r = (xd - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double p = 1.0 / 87178291200.0;                       // 1 / 14!
    p = p * r + 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const uint64_t bits = (uint64_t)((int64_t)k + 1023) << 52;
    double two_k;
#if defined(__HIP_DEVICE_COMPILE__)
    two_k = __longlong_as_double((long long)bits);
#else
    memcpy(&two_k, &bits, 8);
#endif
    return (float)(p * two_k);
}
