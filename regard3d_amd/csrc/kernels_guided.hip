// kernels_guided.hip -- guided matching behind the geometric filters: OpenMVG's geometry_aware::GuidedMatching, which
// ImageCollectionGeometricFilter::Robust_model_estimation(functor, putatives, bGuided_matching = true, dDistanceRatio) runs for every
// pair the filter accepted (the reference's src/R3DComputeMatches.cpp:2113-2114,2169-2170,2215-2218 pass false; DESIGN.md section 2 item 12,
// "Guided matching", restates what true does).  The queries are ALL features of view I, the candidates ALL features of view J.
//
// Three passes over the jobs (one per accepted pair, F, E and H alike) of a call, all launched once:
//   sweep (pass 0)  a workgroup owns 256 queries of one job, a lane one query.  The lane forms its epipolar line (F, E) or its transfer
//                   into J (H) once in f64, then sweeps J's positions -- staged through LDS in tiles of kGuidedTile -- in ascending j with
//                   a conservative f32 gate; what passes the gate is decided by the f64 error in the oracle's operation order (this
//                   unit is compiled with -ffp-contract=off, as oracle/ is), strict err < errTh.  A geometry-only query keeps the first
//                   j of smallest error; a descriptor-mode query counts its candidates and reserves room for them.
//   sweep (pass 1)  descriptor-mode queries only: the same gate again, the candidates written in ascending j.  Pass 0 counts them per
//                   workgroup; the host cuts the workgroups into chunks whose lists fit a candidate budget, and pass 1 + desc run per
//                   chunk on one buffer (a wide caller-chosen threshold costs time, not memory).
//   desc            a lane per descriptor-mode query walks its own candidate list: SquaredDescriptorDistance in the reference
//                   arithmetic (exact_l2sq: OpenMVG L2<float> / L2<unsigned char>; popcount: Hamming), OpenMVG's distanceRatio
//                   update, ratio test in double.  Computing distances inside the sweep would stall the wave on every step in
//                   which one lane of 64 meets a candidate (0.1 - 0.3 % of J per query).
//   compact         a workgroup per job: the matched queries in ascending i, coordinate de-duplication (IndMatchDecorator) for the
//                   homography's geometry-only mode.
//
// The f32 gate.  F / E: d32 = l0f x + l1f y + l2f against T = sqrt(errTh (l0^2 + l1^2)).  Every f32 operation of d32 (the three
// coefficients rounded from f64, two products, two sums) is off by at most 2^-24 of |l0 x| + |l1 y| + |l2| and the f64 error is closer
// still, so |d32| <= T (1 + 2^-20) + (|l0f| Xmax + |l1f| Ymax + |l2f|) 2^-20 + 1e-30 holds for every candidate with err < errTh (Xmax,
// Ymax: largest |x|, |y| of the tile; the absolute term covers flushed denormals).  H: |x - pxf| and |y - pyf| against sqrt(errTh)
// with the same slack.  A query or tile whose magnitudes leave that argument (non-finite, |coefficient| >= 1e30, |position| >= 1e7)
// sends every j of the tile to the f64 test instead: slower, same answer.
#include "kernels_match_common.hpp"

#include <float.h>

namespace r3dm {

constexpr float kGateRel = 9.5367431640625e-07f;     // 2^-20
constexpr float kGateAbs = 1e-30f;

__device__ __forceinline__ uint32_t guided_job_of(const GuidedParams& P, uint32_t b)
{
    uint32_t lo = 0, hi = P.n_jobs - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (P.jobs[mid].b0 <= b) lo = mid; else hi = mid - 1; }
    return lo;
}

// lane exclusive prefix of `v` over the wave, and the wave's total
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t incl = v;
    for (uint32_t off = 1; off < 64; off <<= 1) { const uint32_t u = __shfl_up(incl, off); if (lane >= off) incl += u; }
    total = __shfl(incl, 63);
    return incl - v;
}

template <int PASS>
__global__ __launch_bounds__(256)
void guided_sweep_kernel(const GuidedParams P)
{
    __shared__ __attribute__((aligned(16))) float2 sxy[kGuidedTile];     // (read as float4: two positions)
    __shared__ uint32_t smax[2][2];                                     // largest |x|, |y| of the tile, double-buffered by tile parity
    __shared__ uint32_t wsum[4];
    const uint32_t b = blockIdx.x + P.b_lo;
    const uint32_t k = guided_job_of(P, b);
    const GuidedJob& G = P.jobs[k];
    const uint32_t flags = G.flags, kind = G.kind;
    const bool desc = (flags & kGuidedDesc) != 0;
    if (PASS == 1 && !desc) return;                                     // (the whole workgroup: a job is workgroup-uniform)
    const ImgDev* __restrict__ Iv = P.imgs + G.sI;
    const ImgDev* __restrict__ Jv = P.imgs + G.sJ;
    const uint32_t i = (b - G.b0) * 256u + threadIdx.x;
    const bool active = i < G.nI;
    const uint32_t q = G.q0 + i;
    const uint32_t nJ = Jv->n;
    const float2* __restrict__ xyJ = reinterpret_cast<const float2*>(Jv->xy);
    const double errTh = G.errTh;

    // the query's line l = F x_i (F, E) or its transfer (px, py) = hnormalized(H x_i) (H), as orc_epipolar_dist_err / orc_h_asym_err form them
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, den = 0.0;
    float f0 = 0.f, f1 = 0.f, f2 = 0.f, T32 = 0.f;
    bool gate_ok = false;
    if (active) {
        const double x1 = Iv->xy[2 * (size_t)i], y1 = Iv->xy[2 * (size_t)i + 1];
        const double* M = G.M;
        double T;
        if (kind == 0) {
            a0 = M[0] * x1 + M[1] * y1 + M[2];
            a1 = M[3] * x1 + M[4] * y1 + M[5];
            a2 = M[6] * x1 + M[7] * y1 + M[8];
            den = a0 * a0 + a1 * a1;
            T = sqrt(errTh * den);
            gate_ok = fabs(a0) < 1e30 && fabs(a1) < 1e30 && fabs(a2) < 1e30 && T < 1e30;
        } else {
            const double w = M[6] * x1 + M[7] * y1 + M[8];
            a0 = (M[0] * x1 + M[1] * y1 + M[2]) / w;
            a1 = (M[3] * x1 + M[4] * y1 + M[5]) / w;
            T = sqrt(errTh);
            gate_ok = fabs(a0) < 1e30 && fabs(a1) < 1e30 && T < 1e30;
        }
        if (gate_ok) { f0 = (float)a0; f1 = (float)a1; f2 = (float)a2; T32 = (float)T * (1.0f + kGateRel); }
    }

    double best = DBL_MAX;
    uint32_t bj = kNone, cnt = 0;
    unsigned long long wpos = 0;
    if (PASS == 1) {
        // the workgroup's lists in query order from its base in the chunk: an exclusive scan of pass 0's counts
        uint32_t wt = 0;
        const uint32_t before = wave_exclusive(active ? P.q_cnt[q] : 0u, wt);
        if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = wt;
        r3dm_syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) woff += wsum[w];
        wpos = P.blk_base[b] + woff + before;
        if (active) P.q_off[q] = wpos;
    }
    for (uint32_t t0 = 0, par = 0; t0 < nJ; t0 += kGuidedTile, par ^= 1u) {
        const uint32_t tn = min(kGuidedTile, nJ - t0);
        // (buffer `par` was last read two tiles ago, before the barriers of the previous tile)
        if (threadIdx.x < 2) smax[par][threadIdx.x] = 0u;
        r3dm_syncthreads();                                             // the previous tile has been read by every lane
        float mx = 0.f, my = 0.f;
        for (uint32_t e = threadIdx.x; e < tn; e += 256u) {
            const float2 v = xyJ[t0 + e];
            sxy[e] = v;
            mx = fmaxf(mx, fabsf(v.x)); my = fmaxf(my, fabsf(v.y));      // (fmaxf drops NaN: a NaN position fails every test by itself)
        }
        // the sweep reads the tile four positions at a time: pad it to a multiple of 4 with NaN, which no test accepts (err < errTh is
        // false for a NaN error), outside the magnitudes above
        for (uint32_t e = tn + threadIdx.x; e < ((tn + 3u) & ~3u); e += 256u) sxy[e] = make_float2(__builtin_nanf(""), __builtin_nanf(""));
        for (int off = 32; off > 0; off >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, off)); my = fmaxf(my, __shfl_xor(my, off)); }
        if ((threadIdx.x & 63u) == 0) { atomicMax(&smax[par][0], __float_as_uint(mx)); atomicMax(&smax[par][1], __float_as_uint(my)); }
        r3dm_syncthreads();
        if (!active) continue;
        const float Xm = __uint_as_float(smax[par][0]), Ym = __uint_as_float(smax[par][1]);
        const bool exact_all = !(gate_ok && Xm < 1e7f && Ym < 1e7f);
        // four positions per step: two 16-byte LDS reads, four gate tests, and one branch around the (rare) f64 tests
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(sxy);
        auto take = [&](double err, uint32_t j) {
            if (err < errTh) {
                ++cnt;
                if (PASS == 1) P.cand[wpos++] = j;
                else if (err < best) { best = err; bj = j; }
            }
        };
        if (kind == 0) {
            const float lim = T32 + (fabsf(f0) * Xm + fabsf(f1) * Ym + fabsf(f2)) * kGateRel + kGateAbs;
            for (uint32_t e = 0; e < tn; e += 4u) {
                const float4 ab = s4[e >> 1], cd = s4[(e >> 1) + 1];
                const float xs[4] = {ab.x, ab.z, cd.x, cd.z}, ys[4] = {ab.y, ab.w, cd.y, cd.w};
                bool pass[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) pass[u] = (fabsf(f0 * xs[u] + f1 * ys[u] + f2) <= lim) | exact_all;   // (bitwise: no short-circuit branches)
                if (pass[0] | pass[1] | pass[2] | pass[3]) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (pass[u]) {                                  // ascending j: u in order
                            const double d = a0 * (double)xs[u] + a1 * (double)ys[u] + a2;
                            take((d * d) / den, t0 + e + u);
                        }
                }
            }
        } else {
            const float limx = T32 + (fabsf(f0) + Xm) * kGateRel + kGateAbs, limy = T32 + (fabsf(f1) + Ym) * kGateRel + kGateAbs;
            for (uint32_t e = 0; e < tn; e += 4u) {
                const float4 ab = s4[e >> 1], cd = s4[(e >> 1) + 1];
                const float xs[4] = {ab.x, ab.z, cd.x, cd.z}, ys[4] = {ab.y, ab.w, cd.y, cd.w};
                bool pass[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) pass[u] = ((fabsf(xs[u] - f0) <= limx) & (fabsf(ys[u] - f1) <= limy)) | exact_all;
                if (pass[0] | pass[1] | pass[2] | pass[3]) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (pass[u]) {
                            const double ex = (double)xs[u] - a0, ey = (double)ys[u] - a1;
                            take(ex * ex + ey * ey, t0 + e + u);
                        }
                }
            }
        }
    }
    if (PASS == 1) return;
    // pass 0: geometry-only queries are resolved; descriptor-mode queries leave their counts (per query and per workgroup)
    uint32_t wave_tot = 0;
    (void)wave_exclusive(cnt, wave_tot);
    if ((threadIdx.x & 63u) == 0 && wave_tot) {
        if (desc) atomicAdd(&P.blk_cnt[b], (unsigned long long)wave_tot);
        atomicAdd(&P.ctr[0], (unsigned long long)wave_tot);
    }
    if (!active) return;
    if (desc) P.q_cnt[q] = cnt;
    else P.res[q] = bj;
}

hipError_t launch_guided_sweep(hipStream_t st, const GuidedParams& P, int pass)
{
    if (P.n_blocks == 0 || P.n_jobs == 0) return hipSuccess;
    if ((uint64_t)P.n_blocks > kMaxBlocksOf256) return hipErrorInvalidValue;
    if (pass == 0) hipLaunchKernelGGL(guided_sweep_kernel<0>, dim3(P.n_blocks), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(guided_sweep_kernel<1>, dim3(P.n_blocks), dim3(256), 0, st, P);
    return hipGetLastError();
}

// a lane per descriptor-mode query: its candidates in ascending j, OpenMVG's distanceRatio (bd, sbd start at the distance type's max)
__global__ __launch_bounds__(256)
void guided_desc_kernel(const GuidedParams P)
{
    const uint32_t b = blockIdx.x + P.b_lo;
    const uint32_t k = guided_job_of(P, b);
    const GuidedJob& G = P.jobs[k];
    if (!(G.flags & kGuidedDesc)) return;
    const uint32_t i = (b - G.b0) * 256u + threadIdx.x;
    if (i >= G.nI) return;
    const uint32_t q = G.q0 + i;
    const ImgDev* __restrict__ Iv = P.imgs + G.sI;
    const ImgDev* __restrict__ Jv = P.imgs + G.sJ;
    const uint32_t cnt = P.q_cnt[q];
    const uint32_t* __restrict__ cl = P.cand + P.q_off[q];
    uint32_t idx = kNone;
    bool ok = false;
    if (G.flags & kGuidedBin) {
        const uint32_t W = Iv->words;
        const uint32_t* __restrict__ a = Iv->bin + (size_t)i * W;
        uint32_t bd = 0xFFFFFFFFu, sbd = 0xFFFFFFFFu;
        for (uint32_t c = 0; c < cnt; ++c) {
            const uint32_t j = cl[c];
            const uint32_t* __restrict__ b = Jv->bin + (size_t)j * W;
            uint32_t d = 0;
            for (uint32_t w = 0; w < W; ++w) d += (uint32_t)__popc(a[w] ^ b[w]);
            if (d < bd) { sbd = bd; bd = d; idx = j; }
            else if (d < sbd) sbd = d;
        }
        ok = sbd != 0xFFFFFFFFu && (double)bd < G.R * (double)sbd;
    } else {
        const uint32_t dim = Iv->dim;
        const float* __restrict__ a = Iv->rows + (size_t)i * dim;
        float bd = FLT_MAX, sbd = FLT_MAX;
        for (uint32_t c = 0; c < cnt; ++c) {
            const uint32_t j = cl[c];
            const float d = exact_l2sq(a, Jv->rows + (size_t)j * dim, dim);
            if (d < bd) { sbd = bd; bd = d; idx = j; }
            else if (d < sbd) sbd = d;
        }
        ok = sbd != FLT_MAX && (double)bd < G.R * (double)sbd;
    }
    P.res[q] = ok ? idx : kNone;
}

hipError_t launch_guided_desc(hipStream_t st, const GuidedParams& P)
{
    if (P.n_blocks == 0 || P.n_jobs == 0) return hipSuccess;
    if ((uint64_t)P.n_blocks > kMaxBlocksOf256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guided_desc_kernel, dim3(P.n_blocks), dim3(256), 0, st, P);
    return hipGetLastError();
}

// a workgroup per job: matched queries in ascending i; with kGuidedDedup a match goes when an EARLIER match of the list has the same
// (xI, yI, xJ, yJ) -- the position classes of both views (ImgDev::canon: smallest index at the position; such a match has i >= canon_I(i))
__global__ __launch_bounds__(256)
void guided_compact_kernel(const GuidedParams P)
{
    __shared__ uint32_t wave_cnt[4];
    for (uint32_t k = blockIdx.x; k < P.n_jobs; k += gridDim.x) {
        const GuidedJob& G = P.jobs[k];
        const ImgDev* __restrict__ Iv = P.imgs + G.sI;
        const ImgDev* __restrict__ Jv = P.imgs + G.sJ;
        const uint32_t* __restrict__ res = P.res + G.q0;
        const uint32_t* __restrict__ cI = Iv->canon;
        const uint32_t* __restrict__ cJ = Jv->canon;
        const bool dedup = (G.flags & kGuidedDedup) && cI && cJ;
        uint32_t m = 0;
        for (uint32_t base = 0; base < G.nI; base += 256u) {
            const uint32_t i = base + threadIdx.x;
            const uint32_t j = i < G.nI ? res[i] : kNone;
            bool keep = j != kNone;
            if (keep && dedup) {
                const uint32_t ci = cI[i], cj = cJ[j];
                for (uint32_t e = ci; e < i && keep; ++e) {
                    const uint32_t je = res[e];
                    if (je != kNone && cI[e] == ci && cJ[je] == cj) keep = false;
                }
            }
            uint32_t tot;
            const uint32_t rank = wg_compact_rank(keep, wave_cnt, tot);
            if (keep) { r3dm_match mt; mt.i = i; mt.j = j; P.out[(size_t)G.q0 + m + rank] = mt; }
            m += tot;
            r3dm_syncthreads();
        }
        if (threadIdx.x == 0) P.out_cnt[k] = m;
    }
}

hipError_t launch_guided_compact(hipStream_t st, const GuidedParams& P)
{
    if (P.n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(guided_compact_kernel, dim3(P.n_jobs < 16384u ? P.n_jobs : 16384u), dim3(256), 0, st, P);
    return hipGetLastError();
}

}  // namespace r3dm
