// filter_device.hpp -- what the two AC-RANSAC kernels share: the device routines, the LDS layout and the workgroup barriers of
//   * the one-workgroup-per-pair kernel (filter_acransac.inc, instantiated by kernels_filter.hip for F / H and by
//     kernels_filter_e.hip for E), and
//   * the cooperative kernel of the long pairs (kernels_filter_coop.hip).
// Sample stream, minimal solvers (7-point, 4-point, cooperative 5-point), residuals, FState and the sizes of the LDS regions,
// the developer build's debug macros, wg_fence / wg_sync_* and the register bitonic sort.  Device code and constants only: no
// kernel and no host function is defined here.
//
// f64 throughout, compiled with -ffp-contract=off so residuals agree with the CPU restatement to rounding of the transcendental
// calls (acos/cos/cbrt/log10) only.
#pragma once

#include "r3dm_internal.hpp"
#include <cstdlib>

namespace r3dm {

#define FLT_EPS_D 1.1920928955078125e-07

// ---- sample stream: identical integer arithmetic to oracle/acransac.c orc_rng_u64 ----
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ULL;
    z ^= z >> 27; z *= 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return z;
}

__device__ __forceinline__ uint64_t rng_u64(uint64_t seed, uint32_t I, uint32_t J, uint32_t iter, uint32_t attempt)
{
    const uint64_t G = 0x9E3779B97F4A7C15ULL;
    const uint64_t a = mix64(seed + G * (1ULL + (((uint64_t)I << 32) | (uint64_t)J)));
    return mix64(a + G * (1ULL + (((uint64_t)iter << 32) | (uint64_t)attempt)));
}

// ---- cubic: roots of c0 + c1 x + c2 x^2 + c3 x^3 (Cardano / trigonometric form) ----
__device__ int solve_cubic(const double* c, double* roots)
{
    if (c[3] == 0.0) return 0;
    const double a = c[2] / c[3], b = c[1] / c[3], cc = c[0] / c[3];
    const double q = a * a - 3.0 * b;
    const double r = 2.0 * a * a * a - 9.0 * a * b + 27.0 * cc;
    const double Q = q / 9.0, R = r / 54.0;
    const double Q3 = Q * Q * Q, R2 = R * R;
    const double CR2 = 729.0 * r * r, CQ3 = 2916.0 * q * q * q;
    const double a3 = a / 3.0;
    if (R == 0.0 && Q == 0.0) {
        roots[0] = roots[1] = roots[2] = -a3;
        return 3;
    }
    if (CR2 == CQ3) {
        const double sqrtQ = sqrt(Q);
        if (R > 0.0) { roots[0] = -2.0 * sqrtQ - a3; roots[1] = sqrtQ - a3; roots[2] = sqrtQ - a3; }
        else         { roots[0] = -sqrtQ - a3; roots[1] = -sqrtQ - a3; roots[2] = 2.0 * sqrtQ - a3; }
        return 3;
    }
    if (CR2 < CQ3) {
        const double sqrtQ = sqrt(Q);
        const double sqrtQ3 = sqrtQ * sqrtQ * sqrtQ;
        const double theta = acos(R / sqrtQ3);
        const double norm = -2.0 * sqrtQ;
        const double TWO_PI = 2.0 * 3.14159265358979323846;
        double x0 = norm * cos(theta / 3.0) - a3;
        double x1 = norm * cos((theta + TWO_PI) / 3.0) - a3;
        double x2 = norm * cos((theta - TWO_PI) / 3.0) - a3;
        double t;
        if (x0 > x1) { t = x0; x0 = x1; x1 = t; }
        if (x1 > x2) { t = x1; x1 = x2; x2 = t; if (x0 > x1) { t = x0; x0 = x1; x1 = t; } }
        roots[0] = x0; roots[1] = x1; roots[2] = x2;
        return 3;
    }
    const double sgnR = (R >= 0.0 ? 1.0 : -1.0);
    const double A = -sgnR * cbrt(fabs(R) + sqrt(R2 - Q3));
    const double B = Q / A;
    roots[0] = A + B - a3;
    return 1;
}

__device__ __forceinline__ double det3(const double* r0, const double* r1, const double* r2)
{
    return r0[0] * (r1[1] * r2[2] - r1[2] * r2[1])
         - r0[1] * (r1[0] * r2[2] - r1[2] * r2[0])
         + r0[2] * (r1[0] * r2[1] - r1[1] * r2[0]);
}

// 7-point solver: x1, x2 = 7 normalised correspondences.  Null space of the 7x9 system = last two
// columns of Q in the Householder QR of A^T (9x7); all indices static -> registers.
__device__ int seven_point(const double (&px1)[7][2], const double (&px2)[7][2], double* Fs /* 27 */)
{
    double M[9][7];
#pragma unroll
    for (int p = 0; p < 7; ++p) {
        const double ax = px1[p][0], ay = px1[p][1], bx = px2[p][0], by = px2[p][1];
        M[0][p] = bx * ax; M[1][p] = bx * ay; M[2][p] = bx;
        M[3][p] = by * ax; M[4][p] = by * ay; M[5][p] = by;
        M[6][p] = ax;      M[7][p] = ay;      M[8][p] = 1.0;
    }
    double beta[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double nrm2 = 0.0;
#pragma unroll
        for (int r = j; r < 9; ++r) nrm2 += M[r][j] * M[r][j];
        const double nrm = sqrt(nrm2);
        double bj = 0.0;
        if (nrm != 0.0) {
            const double alpha = (M[j][j] > 0.0) ? -nrm : nrm;
            M[j][j] -= alpha;                       // column j now holds the reflector v_j (rows j..8)
            double vn2 = 0.0;
#pragma unroll
            for (int r = j; r < 9; ++r) vn2 += M[r][j] * M[r][j];
            if (vn2 != 0.0) bj = 2.0 / vn2;
        } else {
#pragma unroll
            for (int r = j; r < 9; ++r) M[r][j] = 0.0;
        }
        beta[j] = bj;
#pragma unroll
        for (int c = j + 1; c < 7; ++c) {
            double dot = 0.0;
#pragma unroll
            for (int r = j; r < 9; ++r) dot += M[r][j] * M[r][c];
            const double s = bj * dot;
#pragma unroll
            for (int r = j; r < 9; ++r) M[r][c] -= s * M[r][j];
        }
    }
    double f[2][9];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
#pragma unroll
        for (int r = 0; r < 9; ++r) f[e][r] = (r == 7 + e) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 6; j >= 0; --j) {
            double dot = 0.0;
#pragma unroll
            for (int r = j; r < 9; ++r) dot += M[r][j] * f[e][r];
            const double s = beta[j] * dot;
#pragma unroll
            for (int r = j; r < 9; ++r) f[e][r] -= s * M[r][j];
        }
    }
    const double* A = f[0];
    const double* B = f[1];
    double P[4];
    P[0] = det3(A, A + 3, A + 6);
    P[1] = det3(B, A + 3, A + 6) + det3(A, B + 3, A + 6) + det3(A, A + 3, B + 6);
    P[2] = det3(A, B + 3, B + 6) + det3(B, A + 3, B + 6) + det3(B, B + 3, A + 6);
    P[3] = det3(B, B + 3, B + 6);
    double roots[3];
    const int n = solve_cubic(P, roots);
    for (int k = 0; k < n; ++k)
#pragma unroll
        for (int e = 0; e < 9; ++e) Fs[9 * k + e] = A[e] + roots[k] * B[e];
    return n;
}

// SymmetricEpipolarDistanceError (squared, /4)
__device__ __forceinline__ double sym_epipolar_err(const double* F, double x1, double y1, double x2, double y2)
{
    const double Fx0 = F[0] * x1 + F[1] * y1 + F[2];
    const double Fx1 = F[3] * x1 + F[4] * y1 + F[5];
    const double Fx2 = F[6] * x1 + F[7] * y1 + F[8];
    const double Fty0 = F[0] * x2 + F[3] * y2 + F[6];
    const double Fty1 = F[1] * x2 + F[4] * y2 + F[7];
    const double yFx = x2 * Fx0 + y2 * Fx1 + Fx2;
    return (yFx * yFx) * (1.0 / (Fx0 * Fx0 + Fx1 * Fx1) + 1.0 / (Fty0 * Fty0 + Fty1 * Fty1)) / 4.0;
}

// 4-point homography (OpenMVG homography::kernel::FourPointSolver, DLT): rows of L per correspondence
//   [x y 1 0 0 0 -x'x -x'y -x'] and [0 0 0 x y 1 -y'x -y'y -y'];  h = null vector of the 8x9 system,
// taken as the last column of Q in the Householder QR of L^T (9x8), all indices static.
__device__ int four_point_h(const double (&px1)[7][2], const double (&px2)[7][2], double* Hs)
{
    double M[9][8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const double x = px1[p][0], y = px1[p][1], u = px2[p][0], v = px2[p][1];
        M[0][2 * p] = x;  M[1][2 * p] = y;  M[2][2 * p] = 1.0; M[3][2 * p] = 0.0; M[4][2 * p] = 0.0; M[5][2 * p] = 0.0;
        M[6][2 * p] = -u * x; M[7][2 * p] = -u * y; M[8][2 * p] = -u;
        M[0][2 * p + 1] = 0.0; M[1][2 * p + 1] = 0.0; M[2][2 * p + 1] = 0.0; M[3][2 * p + 1] = x; M[4][2 * p + 1] = y; M[5][2 * p + 1] = 1.0;
        M[6][2 * p + 1] = -v * x; M[7][2 * p + 1] = -v * y; M[8][2 * p + 1] = -v;
    }
    double beta[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double nrm2 = 0.0;
#pragma unroll
        for (int r = j; r < 9; ++r) nrm2 += M[r][j] * M[r][j];
        const double nrm = sqrt(nrm2);
        double bj = 0.0;
        if (nrm != 0.0) {
            const double alpha = (M[j][j] > 0.0) ? -nrm : nrm;
            M[j][j] -= alpha;
            double vn2 = 0.0;
#pragma unroll
            for (int r = j; r < 9; ++r) vn2 += M[r][j] * M[r][j];
            if (vn2 != 0.0) bj = 2.0 / vn2;
        } else {
#pragma unroll
            for (int r = j; r < 9; ++r) M[r][j] = 0.0;
        }
        beta[j] = bj;
#pragma unroll
        for (int c = j + 1; c < 8; ++c) {
            double dot = 0.0;
#pragma unroll
            for (int r = j; r < 9; ++r) dot += M[r][j] * M[r][c];
            const double s = bj * dot;
#pragma unroll
            for (int r = j; r < 9; ++r) M[r][c] -= s * M[r][j];
        }
    }
    double f[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) f[r] = (r == 8) ? 1.0 : 0.0;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
        double dot = 0.0;
#pragma unroll
        for (int r = j; r < 9; ++r) dot += M[r][j] * f[r];
        const double s = beta[j] * dot;
#pragma unroll
        for (int r = j; r < 9; ++r) f[r] -= s * M[r][j];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) Hs[e] = f[e];
    return 1;
}

// homography AsymmetricError: || x2 - hnormalized(H x1) ||^2
__device__ __forceinline__ double h_asym_err(const double* H, double x1, double y1, double x2, double y2)
{
    const double w = H[6] * x1 + H[7] * y1 + H[8];
    const double ex = x2 - (H[0] * x1 + H[1] * y1 + H[2]) / w;
    const double ey = y2 - (H[3] * x1 + H[4] * y1 + H[5]) / w;
    return ex * ex + ey * ey;
}

// ------------------------------------------------------------------------------------------------
// 5-point essential matrix (OpenMVG essential::kernel::FivePointKernel behind GeometricFilter_EMatrix_AC,
// /root/reference/src/R3DComputeMatches.cpp:2169).  Same polynomial system as OpenMVG's FivePointsRelativePose,
// solved with Nister's hidden-variable elimination + a Sturm sequence; operation for operation the arithmetic of
// oracle/essential.c (only + - * / after the QR), so both produce the same bits.  Sixteen lanes per minimal sample
// (five_point_coop below), the sample's state in an LDS workspace.
// ------------------------------------------------------------------------------------------------
constexpr unsigned char kT11[4][4] = {{0, 2, 3, 4}, {2, 1, 5, 6}, {3, 5, 7, 8}, {4, 6, 8, 9}};
constexpr unsigned char kT21[10][4] = {{0, 2, 4, 5}, {3, 1, 6, 7}, {2, 3, 8, 9}, {4, 8, 10, 11}, {5, 9, 11, 12},
                                       {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};

// products of small polynomials in (x, y, z); fully unrolled: the monomial tables are compile-time constants, so every
// index is static and the operands stay in registers
__device__ __forceinline__ void e_mul11(const double (&a)[4], const double (&b)[4], double (&out)[10])
{
#pragma unroll
    for (int k = 0; k < 10; ++k) out[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[kT11[i][j]] += a[i] * b[j];
}
__device__ __forceinline__ void e_mul21_acc(const double (&a)[10], const double (&b)[4], double (&out)[20])
{
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[kT21[i][j]] += a[i] * b[j];
}
template <int DA, int DB>
__device__ __forceinline__ void e_pmul(const double (&a)[DA + 1], const double (&b)[DB + 1], double (&out)[DA + DB + 1])
{
#pragma unroll
    for (int k = 0; k <= DA + DB; ++k) out[k] = 0.0;
#pragma unroll
    for (int i = 0; i <= DA; ++i)
#pragma unroll
        for (int j = 0; j <= DB; ++j) out[i + j] += a[i] * b[j];
}
template <int D>
__device__ __forceinline__ double e_peval(const double (&p)[D + 1], double t)
{
    double v = p[D];
#pragma unroll
    for (int k = D - 1; k >= 0; --k) v = v * t + p[k];
    return v;
}

// ------------------------------------------------------------------------------------------------
// The 5-point solver as a COOPERATIVE routine: 16 lanes per minimal sample, 16 samples per workgroup pass.
// (Round 2 ran one sample per lane of wave 0: 512 registers + 256 spilled, two out-of-line calls from divergent flow that were
// only correct with SGPR spills forced to memory, 0.85 ms per chunk on one wave while 192 lanes waited, one workgroup per CU.)
// Here every quantity with an index -- matrix columns, constraint rows, polynomial coefficients, Sturm-chain evaluations, roots,
// models -- belongs to a lane of the sample's group, the sample's state lives in a 367-double LDS workspace, and the lanes of a
// group meet at wave-level fences only (a group never leaves its wavefront, so LDS program order is all the synchronisation there
// is; groups of one wave may diverge freely).  No register arrays with dynamic indices, no calls, nothing data-dependent crosses a
// workgroup barrier.  Every value is produced by exactly the operation sequence of the one-lane form (and of oracle/essential.c):
// the split is over INDEPENDENT outputs, sums keep their order.
// ------------------------------------------------------------------------------------------------
constexpr int kE5Lanes = 16;            // lanes per sample
constexpr int kE5Samples = 16;          // samples per workgroup pass = the essential-matrix kernel's chunk of hypotheses
constexpr int kE5Stride = 367;          // doubles per sample workspace (odd: the groups' accesses spread over the LDS banks)
// workspace map (doubles)
constexpr int kE5A = 0;                 // 10 x 20 elimination matrix A[r][k] at 20 r + k; later the Sturm chain f[k][c] at 11 k + c (k < 12)
constexpr int kE5Deg = 140;             //   ... degree of f[k] (inside the dead matrix)
constexpr int kE5Roots = 160;           //   ... real roots
constexpr int kE5Sgn = 172;             //   ... signs of the chain at a point (12)
constexpr int kE5N = 200;               // null space N[e][r] at 9 e + r (e < 4): E1[r][e] = N[e][r]
constexpr int kE5M = 236;               // 9 x 5 design matrix M[r][j] at 5 r + j, Householder vectors in place      (dead after N)
constexpr int kE5Beta = 281;            // beta[5]                                                                    (dead after N)
constexpr int kE5Eii = 236;             // EE^T diagonal polynomials eii[i][10] at 10 i (i < 3)                         (over M)
constexpr int kE5Tr = 266;              // trace polynomial [10]
constexpr int kE5L = 276;               // L[i][j][10] at 10 (3 i + j)  (90 doubles)                                   (dead after the rows)
constexpr int kE5B = 236;               // B[q][v][5] at 5 (3 q + v)   (45 doubles)                                    (over eii / tr / L)
constexpr int kE5Term = 290;            // the three terms of det B, [3][11]
constexpr int kE5P = 330;               // det B, degree 10 [11]
constexpr int kE5Flag = 345;            // model validity flags [10]
static_assert(kE5L + 90 <= kE5Stride && kE5Flag + 10 <= kE5Stride, "5-point workspace map");

// lanes of one sample meet here: compiler fence + scheduling barrier (LDS operations of one wavefront execute in program order)
#define E5_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

__device__ __forceinline__ void e5_row(const double* __restrict__ W, int r, double (&a)[4])     // E1[r][0..3]
{
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = W[kE5N + 9 * e + r];
}
__device__ __forceinline__ void e5_mul11_rows(const double* __restrict__ W, int ra, int rb, double (&out)[10])
{
    double a[4], b[4];
    e5_row(W, ra, a); e5_row(W, rb, b);
    e_mul11(a, b, out);
}

// l = lane within the sample's group (0..15); W = the sample's workspace; Es = its model slots (9 doubles per model).
// Returns the number of models (the same value in every lane of the group).
__device__ __forceinline__ int five_point_coop(const double (&px1)[7][2], const double (&px2)[7][2], double* __restrict__ Es,
                                               double* __restrict__ W, const int l)
{
    // ---- design matrix: lane p < 5 writes the column of point p
    if (l < 5) {
        double ax = 0, ay = 0, bx = 0, by = 0;
#pragma unroll
        for (int p = 0; p < 5; ++p) if (p == l) { ax = px1[p][0]; ay = px1[p][1]; bx = px2[p][0]; by = px2[p][1]; }
        double* M = W + kE5M + l;
        M[0] = bx * ax; M[5] = bx * ay; M[10] = bx;
        M[15] = by * ax; M[20] = by * ay; M[25] = by;
        M[30] = ax;      M[35] = ay;      M[40] = 1.0;
    }
    E5_SYNC();
    // ---- Householder QR of the 9 x 5 matrix: every lane derives the reflection of column j from the column itself (identical
    // values everywhere), lane 0 stores the vector and beta, lanes c = j + 1 .. 4 apply it to their column
    for (int j = 0; j < 5; ++j) {
        double v[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) v[r] = W[kE5M + 5 * r + j];
        double nrm2 = 0.0;
#pragma unroll
        for (int r = 0; r < 9; ++r) if (r >= j) nrm2 += v[r] * v[r];
        const double nrm = sqrt(nrm2);
        double bj = 0.0;
        if (nrm != 0.0) {
            double vjj = 0.0;
#pragma unroll
            for (int r = 0; r < 9; ++r) if (r == j) vjj = v[r];
            const double alpha = (vjj > 0.0) ? -nrm : nrm;
#pragma unroll
            for (int r = 0; r < 9; ++r) if (r == j) v[r] = vjj - alpha;
            double vn2 = 0.0;
#pragma unroll
            for (int r = 0; r < 9; ++r) if (r >= j) vn2 += v[r] * v[r];
            if (vn2 != 0.0) bj = 2.0 / vn2;
        } else {
#pragma unroll
            for (int r = 0; r < 9; ++r) if (r >= j) v[r] = 0.0;
        }
        E5_SYNC();                                                  // every lane has read column j
        if (l == 0) {
#pragma unroll
            for (int r = 0; r < 9; ++r) if (r >= j) W[kE5M + 5 * r + j] = v[r];
            W[kE5Beta + j] = bj;
        }
        if (l > j && l < 5) {
            double col[9];
#pragma unroll
            for (int r = 0; r < 9; ++r) col[r] = W[kE5M + 5 * r + l];
            double dot = 0.0;
#pragma unroll
            for (int r = 0; r < 9; ++r) if (r >= j) dot += v[r] * col[r];
            const double sc = bj * dot;
#pragma unroll
            for (int r = 0; r < 9; ++r) if (r >= j) W[kE5M + 5 * r + l] = col[r] - sc * v[r];
        }
        E5_SYNC();
    }
    // ---- null space: lane e < 4 reflects the unit vector e_{5 + e} back through the five reflections
    if (l < 4) {
        double n[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) n[r] = (r == 5 + l) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 4; j >= 0; --j) {
            double dot = 0.0;
#pragma unroll
            for (int r = j; r < 9; ++r) dot += W[kE5M + 5 * r + j] * n[r];
            const double sc = W[kE5Beta + j] * dot;
#pragma unroll
            for (int r = j; r < 9; ++r) n[r] -= sc * W[kE5M + 5 * r + j];
        }
#pragma unroll
        for (int r = 0; r < 9; ++r) W[kE5N + 9 * l + r] = n[r];
    }
    E5_SYNC();
    // ---- EE^T diagonal polynomials (lanes 0..2) and the determinant constraint, row 0 of A (lane 9)
    if (l < 3) {
        double a0[10], a1[10], a2[10];
        e5_mul11_rows(W, 3 * l, 3 * l, a0); e5_mul11_rows(W, 3 * l + 1, 3 * l + 1, a1); e5_mul11_rows(W, 3 * l + 2, 3 * l + 2, a2);
#pragma unroll
        for (int k = 0; k < 10; ++k) W[kE5Eii + 10 * l + k] = a0[k] + a1[k] + a2[k];
    }
    if (l == 9) {
        double row[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) row[k] = 0.0;
        double t1[10], t2[10], d2[10], e4[4];
        e5_mul11_rows(W, 1, 5, t1); e5_mul11_rows(W, 2, 4, t2);
#pragma unroll
        for (int k = 0; k < 10; ++k) d2[k] = t1[k] - t2[k];
        e5_row(W, 6, e4); e_mul21_acc(d2, e4, row);
        e5_mul11_rows(W, 2, 3, t1); e5_mul11_rows(W, 0, 5, t2);
#pragma unroll
        for (int k = 0; k < 10; ++k) d2[k] = t1[k] - t2[k];
        e5_row(W, 7, e4); e_mul21_acc(d2, e4, row);
        e5_mul11_rows(W, 0, 4, t1); e5_mul11_rows(W, 1, 3, t2);
#pragma unroll
        for (int k = 0; k < 10; ++k) d2[k] = t1[k] - t2[k];
        e5_row(W, 8, e4); e_mul21_acc(d2, e4, row);
#pragma unroll
        for (int k = 0; k < 20; ++k) W[kE5A + k] = row[k];
    }
    E5_SYNC();
    if (l < 10) W[kE5Tr + l] = 0.5 * ((W[kE5Eii + l] + W[kE5Eii + 10 + l]) + W[kE5Eii + 20 + l]);     // 0.5 * ((EET00 + EET11) + EET22)
    E5_SYNC();
    // ---- L[i][j] = (E E^T)_ij - delta_ij tr: lane 3 i + j
    if (l < 9) {
        const int i = l / 3, j = l % 3;
        double a0[10], a1[10], a2[10];
        e5_mul11_rows(W, 3 * i, 3 * j, a0); e5_mul11_rows(W, 3 * i + 1, 3 * j + 1, a1); e5_mul11_rows(W, 3 * i + 2, 3 * j + 2, a2);
#pragma unroll
        for (int k = 0; k < 10; ++k) { double v = a0[k] + a1[k] + a2[k]; if (i == j) v -= W[kE5Tr + k]; W[kE5L + 10 * l + k] = v; }
    }
    E5_SYNC();
    // ---- the nine trace constraints: row 1 + 3 i + j of A = sum over j' of L[i][j'] * E1[3 j' + j], lane 3 i + j
    if (l < 9) {
        const int i = l / 3, j = l % 3;
        double row[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) row[k] = 0.0;
#pragma unroll
        for (int jp = 0; jp < 3; ++jp) {
            double Lp[10], e4[4];
#pragma unroll
            for (int k = 0; k < 10; ++k) Lp[k] = W[kE5L + 10 * (3 * i + jp) + k];
            e5_row(W, 3 * jp + j, e4);
            e_mul21_acc(Lp, e4, row);
        }
#pragma unroll
        for (int k = 0; k < 20; ++k) W[kE5A + 20 * (1 + l) + k] = row[k];
    }
    E5_SYNC();
    // ---- Gauss-Jordan on the first 10 columns, partial pivoting.  Lane l owns column l (and column 16 + l for l < 4).  Per
    // pivot column c: every lane reads column c (the pivot search and all ten multipliers come from it), then updates its own
    // columns: swap rows c / piv, scale the pivot row, eliminate -- the one-lane order of operations per entry.
    bool alive = true;
    for (int c = 0; c < 10; ++c) {
        double colc[10];
#pragma unroll
        for (int r = 0; r < 10; ++r) colc[r] = W[kE5A + 20 * r + c];
        int piv = c;
        double best = 0.0, pval = 0.0, cval = 0.0;
#pragma unroll
        for (int r = 0; r < 10; ++r) if (r == c) { best = fabs(colc[r]); pval = colc[r]; cval = colc[r]; }
#pragma unroll
        for (int r = 0; r < 10; ++r) if (r > c) { const double v = fabs(colc[r]); if (v > best) { best = v; piv = r; pval = colc[r]; } }
        if (best == 0.0) alive = false;                             // (the same decision in every lane of the group)
        E5_SYNC();                                                  // every lane has read column c
        if (alive) {
            const double inv = 1.0 / pval;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = l + 16 * h;
                if (k < 20 && k >= c) {
                    const double old_c = W[kE5A + 20 * c + k], old_p = W[kE5A + 20 * piv + k];
                    const double prow = ((piv != c) ? old_p : old_c) * inv;       // pivot row after the swap, scaled
                    W[kE5A + 20 * c + k] = prow;
                    if (piv != c) W[kE5A + 20 * piv + k] = old_c;
#pragma unroll
                    for (int r = 0; r < 10; ++r) {
                        if (r == c) continue;
                        // row r after the swap: the old row c sits in row piv; its multiplier is its entry in column c
                        const bool moved = (piv != c) && (r == piv);
                        const double fct = moved ? cval : colc[r];
                        if (fct == 0.0) continue;
                        const double cur = moved ? old_c : W[kE5A + 20 * r + k];
                        W[kE5A + 20 * r + k] = cur - fct * prow;
                    }
                }
            }
        }
        E5_SYNC();
    }
    if (!alive) return 0;
    // ---- B(z): lane 3 q + v
    if (l < 9) {
        const int q = l / 3, v = l % 3;
        const int lo = kE5A + 20 * (4 + 2 * q), hi = kE5A + 20 * (5 + 2 * q);
        double b[5];
        if (v < 2) {
            const int o = 10 + 3 * v;
            b[0] = W[lo + o + 2];
            b[1] = W[lo + o + 1] - W[hi + o + 2];
            b[2] = W[lo + o] - W[hi + o + 1];
            b[3] = -W[hi + o];
            b[4] = 0.0;
        } else {
            b[0] = W[lo + 19];
            b[1] = W[lo + 18] - W[hi + 19];
            b[2] = W[lo + 17] - W[hi + 18];
            b[3] = W[lo + 16] - W[hi + 17];
            b[4] = -W[hi + 16];
        }
        E5_SYNC();                                                  // (B overlays nothing that is still read: eii / tr / L are dead)
#pragma unroll
        for (int e = 0; e < 5; ++e) W[kE5B + 5 * l + e] = b[e];
    } else {
        E5_SYNC();
    }
    E5_SYNC();
    // ---- det B(z) = sum of three products: lane q < 3 one term
    if (l < 3) {
        const int q = l, r1 = (q + 1) % 3, r2 = (q + 2) % 3;
        double a30[4], a31[4], b30[4], b31[4], c4[5];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a30[k] = W[kE5B + 5 * (3 * r1 + 0) + k]; a31[k] = W[kE5B + 5 * (3 * r1 + 1) + k];
            b30[k] = W[kE5B + 5 * (3 * r2 + 0) + k]; b31[k] = W[kE5B + 5 * (3 * r2 + 1) + k];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) c4[k] = W[kE5B + 5 * (3 * q + 2) + k];
        double m1[7], m2[7], mn[7], term[11];
        e_pmul<3, 3>(a30, b31, m1);
        e_pmul<3, 3>(a31, b30, m2);
#pragma unroll
        for (int k = 0; k <= 6; ++k) mn[k] = m1[k] - m2[k];
        e_pmul<6, 4>(mn, c4, term);
#pragma unroll
        for (int k = 0; k <= 10; ++k) W[kE5Term + 11 * q + k] = term[k];
    }
    E5_SYNC();
    if (l < 11) { double pk = 0.0; pk += W[kE5Term + l]; pk += W[kE5Term + 11 + l]; pk += W[kE5Term + 22 + l]; W[kE5P + l] = pk; }
    E5_SYNC();
    // ---- real roots of det B (degree <= 10): Sturm chain in the dead matrix area, built coefficient-parallel
    int d = 10;
    while (d > 0 && W[kE5P + d] == 0.0) --d;
    if (d <= 0) return 0;
    // (the chain's 11 x 11 slots start as zeros: every coefficient above a polynomial's degree then IS zero -- copies, eliminations and
    //  normalisations below only write up to the degree and zero what they eliminate -- so the bisection can run Horner over fixed
    //  lengths: leading zeros change no bit of the value)
    for (int e = l; e < 121; e += kE5Lanes) W[kE5A + e] = 0.0;
    E5_SYNC();
    {
        const double lead = W[kE5P + d];
        if (l <= d) W[kE5A + l] = W[kE5P + l] / lead;
        if (l == 15) W[kE5Deg + 0] = (double)d;
    }
    E5_SYNC();
    if (l >= 1 && l <= d) W[kE5A + 11 + l - 1] = (double)l * W[kE5A + l];
    if (l == 15) W[kE5Deg + 1] = (double)(d - 1);
    E5_SYNC();
    int nf = 2;
    {
        int deg_prev = d, deg_cur = d - 1;
        while (deg_cur > 0) {
            // f[nf] = -rem(f[nf-2], f[nf-1]) / |leading coefficient|, remainder built in place in slot nf
            const int bo = kE5A + 11 * (nf - 1), ro = kE5A + 11 * nf;
            const int db = deg_cur;
            int dr = deg_prev;
            if (l <= dr) W[ro + l] = W[kE5A + 11 * (nf - 2) + l];
            E5_SYNC();
            const double blead = W[bo + db];
            while (dr >= db) {
                const double q = W[ro + dr] / blead;
                E5_SYNC();                                          // every lane has read the leading remainder coefficient
                if (l < db) W[ro + dr - db + l] -= q * W[bo + l];
                if (l == 15) W[ro + dr] = 0.0;
                E5_SYNC();
                --dr;
            }
            while (dr >= 0 && W[ro + dr] == 0.0) --dr;
            if (dr < 0) break;
            const double sc = fabs(W[ro + dr]);
            E5_SYNC();
            if (l <= dr) W[ro + l] = -W[ro + l] / sc;
            if (l == 15) W[kE5Deg + nf] = (double)dr;
            E5_SYNC();
            deg_prev = deg_cur; deg_cur = dr;
            ++nf;
        }
    }
    double bound = 0.0;
    for (int k = 0; k < d; ++k) { const double a = fabs(W[kE5A + k]); if (a > bound) bound = a; }
    bound += 1.0;
    // sign changes of the chain at -bound and +bound: lane k evaluates f[k], the count walks the signs in order
    int va = 0, vb = 0;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const double t = side == 0 ? -bound : bound;
        if (l < nf) {
            const int dk = (int)W[kE5Deg + l];
            double v = W[kE5A + 11 * l + dk];
            for (int c = dk - 1; c >= 0; --c) v = v * t + W[kE5A + 11 * l + c];
            W[kE5Sgn + l] = (double)((v > 0.0) - (v < 0.0));
        }
        E5_SYNC();
        int changes = 0, last = 0;
        for (int k = 0; k < nf; ++k) {
            const int sg = (int)W[kE5Sgn + k];
            if (sg != 0) { if (last != 0 && sg != last) ++changes; last = sg; }
        }
        if (side == 0) va = changes; else vb = changes;
        E5_SYNC();
    }
    int nr = va - vb;
    if (nr > 10) nr = 10;
    if (nr <= 0) return 0;
    // ---- bisection: lane r < nr owns root r (the (r + 1)-th real root from below): its own midpoints and sign counts, 64 steps
    if (l < nr) {
        double lo = -bound, hi = bound;
        for (int it = 0; it < 64; ++it) {
            const double mid = 0.5 * (lo + hi);
            int changes = 0, last = 0;
            // f[k] has degree <= 10 - k (the chain's degrees fall by at least one per step) and zeros above its own: eleven Horner
            // chains of FIXED length, independent of one another, their 66 coefficients read from LDS at constant offsets -- the
            // reads pipeline and the chains interleave.  (With the degrees read from LDS the 66 reads and multiply-adds of a step were
            // one dependent sequence: 64 steps x ~66 LDS round trips per root, most of a chunk's 170 us.)  A polynomial beyond the
            // chain's end is all zeros: its sign 0 is skipped like any vanishing value.
            asm volatile("" ::: "memory");              // (the coefficients stay in LDS: 132 registers of them would spill)
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                double v = W[kE5A + 11 * k + (10 - k)];
#pragma unroll
                for (int c = 9 - k; c >= 0; --c) v = v * mid + W[kE5A + 11 * k + c];
                const int sg = (v > 0.0) - (v < 0.0);
                if (sg != 0) { if (last != 0 && sg != last) ++changes; last = sg; }
            }
            if (va - changes >= l + 1) hi = mid; else lo = mid;
        }
        W[kE5Roots + l] = 0.5 * (lo + hi);
    }
    E5_SYNC();
    // ---- one model per root: lane s < nr; models with a vanishing minor are skipped, the others keep their order
    double model[9];
    bool valid = false;
    if (l < nr) {
        const double z = W[kE5Roots + l];
        double b[3][3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            double p0[4], p1[4], p2[5];
#pragma unroll
            for (int k = 0; k < 4; ++k) { p0[k] = W[kE5B + 5 * (3 * q) + k]; p1[k] = W[kE5B + 5 * (3 * q + 1) + k]; }
#pragma unroll
            for (int k = 0; k < 5; ++k) p2[k] = W[kE5B + 5 * (3 * q + 2) + k];
            b[q][0] = e_peval<3>(p0, z); b[q][1] = e_peval<3>(p1, z); b[q][2] = e_peval<4>(p2, z);
        }
        double bx = 0.0, by = 0.0, bw = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int r1 = q, r2 = (q + 1) % 3;
            const double cx = b[r1][1] * b[r2][2] - b[r1][2] * b[r2][1];
            const double cy = b[r1][2] * b[r2][0] - b[r1][0] * b[r2][2];
            const double cw = b[r1][0] * b[r2][1] - b[r1][1] * b[r2][0];
            if (fabs(cw) > fabs(bw)) { bx = cx; by = cy; bw = cw; }
        }
        if (bw != 0.0) {
            valid = true;
            const double x = bx / bw, y = by / bw;
#pragma unroll
            for (int r = 0; r < 9; ++r) model[r] = x * W[kE5N + r] + y * W[kE5N + 9 + r] + z * W[kE5N + 18 + r] + W[kE5N + 27 + r];
        }
    }
    if (l < 10) W[kE5Flag + l] = (l < nr && valid) ? 1.0 : 0.0;
    E5_SYNC();
    int before = 0, n_out = 0;
    for (int s2 = 0; s2 < nr; ++s2) { const int fl = (int)W[kE5Flag + s2]; if (s2 < l) before += fl; n_out += fl; }
    if (valid) {
#pragma unroll
        for (int r = 0; r < 9; ++r) Es[9 * before + r] = model[r];
    }
    return n_out;
}
#undef E5_SYNC

// fundamental::kernel::EpipolarDistanceError: squared distance of x2 to the epipolar line F x1
__device__ __forceinline__ double epipolar_dist_err(const double* F, double x1, double y1, double x2, double y2)
{
    const double l0 = F[0] * x1 + F[1] * y1 + F[2];
    const double l1 = F[3] * x1 + F[4] * y1 + F[5];
    const double l2 = F[6] * x1 + F[7] * y1 + F[8];
    const double d = l0 * x2 + l1 * y2 + l2;
    return (d * d) / (l0 * l0 + l1 * l1);
}

// FundamentalFromEssential: F = K2^-T E K1^-1
__device__ __forceinline__ void f_from_e(const double* E, const double* K1i, const double* K2i, double* F)
{
    double T[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += K2i[3 * k + r] * E[3 * k + c];
            T[3 * r + c] = v;
        }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += T[3 * r + k] * K1i[3 * k + c];
            F[3 * r + c] = v;
        }
}

// ---- per-workgroup shared state (lives at the front of the dynamic LDS region) ----
struct FState {
    double minNFA, errorMax;
    double bestF[9];
    double cur_nfa;          // scratch: NFA of the model under evaluation
    uint32_t nIter, reserve, iter, pool_size, n_inl, acMode, n_models, iters_done;
    uint32_t cnt, cur_k, flag, chunk_n;
    uint32_t wave_cnt[8];    // (up to 8 waves: the wide variant of the kernel runs 512 threads)
    double   red_v[8];
    double   red_b[8];       // reduction slots of the sort-skipping bound
    uint32_t red_k[8];
    uint32_t nm[64];
    uint32_t dbg_smp[64];    // debug trace: first sample index of each hypothesis of the chunk
    uint32_t dbg_pool;       // debug trace: pool size the chunk was drawn from
    double   kinv[18];       // essential matrix: K1^-1, K2^-1 of the pair (read from here at their two use sites: 36 wave-uniform
                             // doubles held in scalar registers for the whole kernel were most of its SGPR spills)
};
static_assert(sizeof(FState) <= 1024, "FState must fit the first 1024 bytes of the dynamic LDS region");

constexpr int kChunk = 64;                          // hypotheses per chunk, F and H: one lane of wave 0 per minimal sample
template <int KIND> struct ChunkOf { static constexpr int n = (KIND == 2) ? kE5Samples : kChunk; };   // E: 16 lanes per sample, 16 samples
// residual histogram of the model under evaluation (the sort-skipping bound below): 2^kHistSub bins per octave of the residual,
// kHistBins bins down from the bound on the residuals; LDS header = FState (padded to 1024) + the histogram
constexpr int kHistBins = 1024, kHistSub = 5, kHistShift = 52 - kHistSub;
constexpr int kHdr = 1024 + kHistBins * 4;
// the scout pass (round 6, acransac_body): per chunk the flat offsets of the hypotheses' models, and per scouted model the number of
// matches within the bound and the lower bound of its NFA; the per-wave histograms of the pass live in the (then idle) sort buffers
constexpr int kScoutModels = 192;                   // 64 x 3 (F), 64 x 1 (H), 16 x 10 (E)
constexpr int kScoutBytes = kScoutModels * 4 + kScoutModels * 8 + 80 * 4;      // totals, bounds, offsets [65] padded: 2624 bytes (16-byte multiple)
constexpr int kScoutHistBytes = 8 * kHistBins * 4;  // eight waves (the 512-thread variant) x 1024 u32 bins

// debug aids of the developer build (-DR3DM_DEVTOOLS; r3dm_internal.hpp): R3DM_FILTER_CHECK=1 records the first violated
// invariant instead of running into a memory fault, R3DM_TRACE_PAIR dumps the per-model trace of one pair.  In the product
// build both pointers are compile-time null and the code below them disappears.
#ifdef R3DM_DEVTOOLS
#define R3DM_DBG(P) ((P).dbg)
#define R3DM_TRACE(P) ((P).trace)
#else
#define R3DM_DBG(P) ((uint32_t*)nullptr)
#define R3DM_TRACE(P) ((double*)nullptr)
#endif
// the timing build (tools/build_bisect.sh, -DR3DM_E_TIMING; read by tools/filter_phase_split.py): E_TIME(statements) keeps the
// cycle counters of acransac_body and is nothing in every other build
#ifdef R3DM_E_TIMING
#define E_TIME(...) __VA_ARGS__
#else
#define E_TIME(...)
#endif
#define FCHECK(cond, code, a, b)                                                                          \
    do {                                                                                                  \
        if (R3DM_DBG(P) && !(cond)) {                                                                           \
            if (atomicCAS(P.dbg, 0u, (uint32_t)(code)) == 0u) { P.dbg[1] = item; P.dbg[2] = (uint32_t)(a); P.dbg[3] = (uint32_t)(b); } \
        }                                                                                                 \
    } while (0)

// Workgroup barriers.  Waves of the workgroup exchange data through LDS almost everywhere (r3dm_syncthreads: barrier with an
// explicit lgkmcnt(0), see r3dm_internal.hpp -- the missing wait at the top of acransac_body's chunk loop (filter_acransac.inc) is what made the
// homography kernel, the only one light enough for two workgroups per CU, return different results from run to run and
// eventually fault).  Through GLOBAL memory they exchange data in three places: the normalised points / pool / log-combinatorial
// table written at start-up, the pool rebuilt after an improvement, and -- spill variant only -- the sort buffers.  Every such
// slice belongs to ONE workgroup, whose waves share a CU and its vector L1 -- a WORKGROUP-scope fence plus a wait for the wave's
// outstanding stores and loads is what the exchange needs.  __threadfence() is agent scope: on this chip of eight L2s that is an L2
// write-back + invalidate per barrier, ~10 per evaluated model on a spilled pair, and it slows every other workgroup of the device
// with it.  (The explicit wait is not redundant: hipcc was seen to emit no vmcnt wait for a workgroup-scope fence on gfx950.)
// Two conditions the shortcut rests on, both enforced here rather than assumed: the s_waitcnt immediate below is the gfx9 encoding
// (vmcnt(0) lgkmcnt(0) = 0x0070), and the workgroup's waves must share one L1, i.e. the kernel is NOT compiled in threadgroup-split
// mode (-mtgsplit: the compiler defines no macro for it, so build.sh refuses the flag instead).
#if defined(__HIP_DEVICE_COMPILE__)
#if !defined(__gfx950__) && !defined(__gfx942__)
#error "wg_fence: the s_waitcnt encoding and the same-CU L1 argument are written for gfx942 / gfx950"
#endif
#endif
__device__ __forceinline__ void wg_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_s_waitcnt(0x0070);          // vmcnt(0) lgkmcnt(0): this wave's global stores and loads have completed
}
__device__ __forceinline__ void wg_sync_global() { wg_fence(); r3dm_syncthreads(); wg_fence(); }
template <bool GLOBAL_BUFFERS>
__device__ __forceinline__ void wg_sync_t()
{
    if (GLOBAL_BUFFERS) { wg_fence(); r3dm_syncthreads(); wg_fence(); }
    else r3dm_syncthreads();
}

// Sort of the (residual, index) pairs of one model, ascending, for the workgroup's 256 threads: `total` compacted entries in
// keys / sidx (LDS), cap = next power of two >= total, E = max(1, cap / 256) entries per thread in registers.  Entry i lives in
// thread i / E, slot i % E; the bitonic network's exchanges at distance < E are register compare-exchanges, at distance < 64 E
// lane exchanges inside the wave (ds_bpermute), and only the two largest distances (three of the log2(cap)(log2(cap)+1)/2
// stages) cross waves through LDS with a barrier.  The pairs are distinct (index breaks ties), so the result is the same total
// order the plain LDS network produces -- 4.5x fewer cycles per model on C2's pairs.
__device__ __forceinline__ bool pair_gt(unsigned long long a, uint32_t ai, unsigned long long b, uint32_t bi)
{
    return (a > b) || (a == b && ai > bi);
}

// GLOBAL: keys / sidx are the global spill buffers of a pair with more matches than the LDS holds (the register part is the same,
// the few wave-crossing stages go through global memory with a fence at the barrier).
template <int E, bool GLOBAL = false>
__device__ __forceinline__ void wg_sort_regs(unsigned long long* __restrict__ keys, uint32_t* __restrict__ sidx,
                                             uint32_t cap, uint32_t total, uint32_t tid)
{
    unsigned long long k[E];
    uint32_t x[E];
    const uint32_t base = tid * (uint32_t)E;
#pragma unroll
    for (int s = 0; s < E; ++s) {
        const uint32_t i = base + (uint32_t)s;
        const bool live = i < total;
        k[s] = live ? keys[i] : ~0ull;
        x[s] = live ? sidx[i] : 0xFFFFFFFFu;
    }
    for (uint32_t size = 2; size <= cap; size <<= 1) {
        // ---- distances that cross waves: through LDS (every thread parks its entries, reads the partner's)
        for (uint32_t stride = size >> 1; stride >= 64u * E; stride >>= 1) {
            wg_sync_t<GLOBAL>();                                   // earlier readers of keys / sidx are done
            if (base < cap) {
#pragma unroll
                for (int s = 0; s < E; ++s) { keys[base + s] = k[s]; sidx[base + s] = x[s]; }
            }
            wg_sync_t<GLOBAL>();
            if (base < cap) {
#pragma unroll
                for (int s = 0; s < E; ++s) {
                    const uint32_t i = base + (uint32_t)s;
                    const unsigned long long ok = keys[i ^ stride];
                    const uint32_t ox = sidx[i ^ stride];
                    const bool lower = (i & stride) == 0u, up = (i & size) == 0u;
                    const bool mine_gt = pair_gt(k[s], x[s], ok, ox);
                    if (mine_gt == (lower == up)) { k[s] = ok; x[s] = ox; }
                }
            }
        }
        // ---- distances inside the wave
        {
            uint32_t stride = size >> 1;
            if (stride >= 64u * E) stride = 32u * E;
            for (; stride >= (uint32_t)E; stride >>= 1) {
                const int lane_xor = (int)(stride / (uint32_t)E);
#pragma unroll
                for (int s = 0; s < E; ++s) {
                    const uint32_t i = base + (uint32_t)s;
                    const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)k[s], lane_xor);
                    const uint32_t ohi = (uint32_t)__shfl_xor((int)(uint32_t)(k[s] >> 32), lane_xor);
                    const uint32_t ox = (uint32_t)__shfl_xor((int)x[s], lane_xor);
                    const unsigned long long ok = ((unsigned long long)ohi << 32) | olo;
                    const bool lower = (i & stride) == 0u, up = (i & size) == 0u;
                    const bool mine_gt = pair_gt(k[s], x[s], ok, ox);
                    if (mine_gt == (lower == up)) { k[s] = ok; x[s] = ox; }
                }
            }
        }
        // ---- distances inside the thread
#pragma unroll
        for (int ST = E / 2; ST >= 1; ST >>= 1) {
            if ((uint32_t)ST < size) {
#pragma unroll
                for (int s = 0; s < E; ++s) {
                    if ((s & ST) == 0) {
                        const bool up = ((base + (uint32_t)s) & size) == 0u;
                        const bool gt = pair_gt(k[s], x[s], k[s | ST], x[s | ST]);
                        if (gt == up) {
                            const unsigned long long tk = k[s]; k[s] = k[s | ST]; k[s | ST] = tk;
                            const uint32_t tx = x[s]; x[s] = x[s | ST]; x[s | ST] = tx;
                        }
                    }
                }
            }
        }
    }
    wg_sync_t<GLOBAL>();
    if (base < cap) {
#pragma unroll
        for (int s = 0; s < E; ++s) { keys[base + s] = k[s]; sidx[base + s] = x[s]; }
    }
    wg_sync_t<GLOBAL>();
}

}  // namespace r3dm
