// filter_acransac.inc -- the one-workgroup-per-pair AC-RANSAC kernel as a template: acransac_kernel<KIND, NT> and its launcher
// launch_acransac<KIND, NT>.  Included, after filter_device.hpp, by the translation units that instantiate it: kernels_filter.hip
// (F and H) and kernels_filter_e.hip (E).  The kernel itself is described at acransac_body.

namespace r3dm {

// ------------------------------------------------------------------------------------------------
// The scout pass (round 6).  AC-RANSAC walks its models in order, but all a model needs from the matches to be passed over is how many of
// them lie within the bound and -- once some model has been accepted -- a lower bound of the NFA it could reach (the histogram bound
// of the full evaluation below).  Neither depends on the state of the walk, so the models of a chunk are scouted ahead of it, ONE
// WAVEFRONT PER MODEL (a workgroup scouts 4 or 8 models at a time): one sweep over the pair's matches, count by ballot, histogram in the
// wave's own 4 KiB of LDS, prefix and bound inside the wave -- no workgroup barrier, no compaction, no global atomics.  The walk then
// passes over a model without a barrier when the scout says it cannot be accepted (98 % of them, DESIGN.md 4.4), and runs the full
// evaluation -- unchanged -- on the others.  What was ~6 barriers + one pass per model becomes one barrier per sub-batch of models;
// inlier sets, models, iteration and model counts are those of the sequential rule (and of oracle/acransac.c): a skipped model is
// exactly one the full evaluation would have found hopeless or short of AC mode.
// la_g: per-bin NFA slope logalpha0 + mult log10(edge + eps) of the pair (filled once per pair, same expression as the full evaluation)
// ------------------------------------------------------------------------------------------------
// The scout only needs to know on which side of the bound a residual lies and in which histogram bin -- never the value -- so it
// trades the sweep's IEEE divisions (two per residual for F and H, ~11 dependent f64 instructions each) for v_rcp_f64 + one Newton step
// and carries an interval [lo, hi] that contains the residual the full evaluation would compute: v_rcp_f64 is good to 2^-23 (measured:
// tools/ubench/rcp_f64_accuracy.hip), one step squares that; the margins below are 2^-32 where the quotient enters as a factor and
// 2^-40 of the quotient where a difference follows it (H).  `hi <= bound` is surely within, `lo <= bound` possibly; the histogram takes
// `lo` of the possible ones, which can only lower the NFA bound.  Counts that the interval leaves open on either side of a threshold
// of the walk (SS, 2.5 SS) send the model to the full evaluation.  NaN / inf (a degenerate model) fail every comparison, as they do there.
__device__ __forceinline__ double rcp_newton(double a)
{
    const double r = __builtin_amdgcn_rcp(a);
    return __builtin_fma(__builtin_fma(-a, r, 1.0), r, r);
}
template <int KIND>
__device__ __forceinline__ void scout_residual(const double* F, double x1, double y1, double x2, double y2, double& lo, double& hi)
{
    if (KIND == 1) {
        const double rw = rcp_newton(F[6] * x1 + F[7] * y1 + F[8]);
        const double qx = (F[0] * x1 + F[1] * y1 + F[2]) * rw, qy = (F[3] * x1 + F[4] * y1 + F[5]) * rw;
        const double ex = __builtin_fabs(x2 - qx), ey = __builtin_fabs(y2 - qy);
        const double mx = 0x1p-40 * (__builtin_fabs(qx) + ex), my = 0x1p-40 * (__builtin_fabs(qy) + ey);
        const double lx = __builtin_fmax(ex - mx, 0.0), ly = __builtin_fmax(ey - my, 0.0), hx = ex + mx, hy = ey + my;
        lo = (lx * lx + ly * ly) * (1.0 - 0x1p-40);
        hi = (hx * hx + hy * hy) * (1.0 + 0x1p-40);
    } else {
        const double l0 = F[0] * x1 + F[1] * y1 + F[2];
        const double l1 = F[3] * x1 + F[4] * y1 + F[5];
        const double l2 = F[6] * x1 + F[7] * y1 + F[8];
        const double d = x2 * l0 + y2 * l1 + l2;
        double r;
        if (KIND == 0) {
            const double t0 = F[0] * x2 + F[3] * y2 + F[6];
            const double t1 = F[1] * x2 + F[4] * y2 + F[7];
            r = (d * d) * (rcp_newton(l0 * l0 + l1 * l1) + rcp_newton(t0 * t0 + t1 * t1)) * 0.25;
        } else {
            r = (d * d) * rcp_newton(l0 * l0 + l1 * l1);
        }
        lo = r * (1.0 - 0x1p-32);
        hi = r * (1.0 + 0x1p-32);
    }
}
constexpr uint32_t kScoutOpen = 0x80000000u;        // sc_total: the count is open on one side of a threshold of the walk
// lanes of a wavefront that hand values to each other through LDS: to the compiler they are separate threads, so the store of one and the
// load of another need an order it has to respect (found by the scout's check mode: the cross-lane reads of the running counts below had
// been scheduled ahead of the write-back and saw raw bin counts -- a bound that was not one)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int KIND>
__device__ __noinline__ void scout_model(const float4* __restrict__ pt, uint32_t m, const double* __restrict__ Fm, const double* __restrict__ kinv,
                                         double s1, double t1x, double t1y, double s2, double t2x, double t2y, double maxThreshold,
                                         long long hist_base, bool want_bound, const double* __restrict__ la_g, const float* __restrict__ logc_n,
                                         const float* __restrict__ logc_k, double loge0, uint32_t* __restrict__ whist, uint32_t lane,
                                         uint32_t* __restrict__ out_total, double* __restrict__ out_bound, bool exact, double slack)
{
    constexpr uint32_t SS = (KIND == 0) ? 7u : (KIND == 1 ? 4u : 5u);
    double F[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) F[e] = Fm[e];
    if (KIND == 2) { double FE[9]; f_from_e(F, kinv, kinv + 9, FE);
#pragma unroll
        for (int e = 0; e < 9; ++e) F[e] = FE[e]; }
    if (want_bound) {
        uint4* z = reinterpret_cast<uint4*>(whist + 16u * lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_sync();
    }
    uint32_t total = 0, total_sure = 0;
    for (uint32_t base = 0; base < m; base += 256u) {
        double px[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t p = base + 64u * (uint32_t)u + lane;
            const float4 f4 = pt[p < m ? p : 0u];
            px[u][0] = s1 * (double)f4.x + t1x; px[u][1] = s1 * (double)f4.y + t1y;
            px[u][2] = s2 * (double)f4.z + t2x; px[u][3] = s2 * (double)f4.w + t2y;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t p = base + 64u * (uint32_t)u + lane;
            double r_lo, r_hi;
            if (exact || KIND == 1) {           // (H: the interval costs what the two divisions by one denominator do -- measured 10.1 -> 11.0 ms; it keeps them)
                r_lo = (KIND == 0) ? sym_epipolar_err(F, px[u][0], px[u][1], px[u][2], px[u][3])
                     : (KIND == 1) ? h_asym_err(F, px[u][0], px[u][1], px[u][2], px[u][3])
                                   : epipolar_dist_err(F, px[u][0], px[u][1], px[u][2], px[u][3]);
                r_hi = r_lo;
            } else {
                scout_residual<KIND>(F, px[u][0], px[u][1], px[u][2], px[u][3], r_lo, r_hi);
            }
            const bool in = (p < m) && (r_lo <= maxThreshold);
            total += (uint32_t)__builtin_popcountll(__ballot(in));
            total_sure += (uint32_t)__builtin_popcountll(__ballot((p < m) && (r_hi <= maxThreshold)));
            if (want_bound && in) {
                long long bin = (__double_as_longlong(r_lo) >> kHistShift) - hist_base;
                bin = bin < 0 ? 0 : (bin > kHistBins - 1 ? kHistBins - 1 : bin);
                atomicAdd(&whist[bin], 1u);
            }
        }
    }
    const bool open = ((double)total > 2.5 * SS) != ((double)total_sure > 2.5 * SS) || (total > SS) != (total_sure > SS);
    double bound = -__builtin_huge_val();                  // "no bound": the walk then takes the full evaluation
    if (want_bound && total > SS) {
        // inclusive running counts over the bins: 16 consecutive bins per lane, written back in place
        wave_lds_sync();
        uint32_t cb[16];
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) { run += whist[16u * lane + (uint32_t)j]; cb[j] = run; }
        uint32_t incl = run;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, off); if (lane >= (uint32_t)off) incl += o; }
        const uint32_t excl = incl - run;
#pragma unroll
        for (int j = 0; j < 16; ++j) whist[16u * lane + (uint32_t)j] = excl + cb[j];
        wave_lds_sync();
        // bins lane, lane + 64, ...: neighbouring (equally dense) bins go to different lanes.  Within a bin the NFA term of k is
        // la k + g(k) + const with g = logc_n + logc_k; g is concave in k (log-binomials) up to the rounding drift of its float
        // tables, so over the k of a bin the term is smallest at one END of the range, less `slack` (scout_slack below bounds twice the
        // drift): two table reads per bin, all of a lane's in flight at once, where one read pair per k made this loop -- a chain of
        // dependent global loads, up to the bin's whole count long -- the larger part of a model's cost (the scout's first form).
        double wmin = __builtin_huge_val();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t b = lane + 64u * (uint32_t)j;
            const uint32_t k_hi = whist[b], k_prev = b ? whist[b - 1] : 0u;
            uint32_t k_lo = k_prev + 1u; if (k_lo < SS + 1u) k_lo = SS + 1u;
            const bool some = k_hi >= k_lo;
            const uint32_t ka = some ? k_lo : 0u, kb = some ? k_hi : 0u;
            const double la = la_g[b];
            const double wa = loge0 + la * (double)(ka - SS) + (double)logc_n[ka] + (double)logc_k[ka];
            const double wb = loge0 + la * (double)(kb - SS) + (double)logc_n[kb] + (double)logc_k[kb];
            const double w = wa < wb ? wa : wb;
            wmin = (some && w < wmin) ? w : wmin;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(wmin, off); wmin = o < wmin ? o : wmin; }
        bound = wmin - slack;
    }
    if (lane == 0) { *out_total = total | (open ? kScoutOpen : 0u); *out_bound = bound; }
}

// ------------------------------------------------------------------------------------------------
// The batched a-contrario RANSAC filter on gfx950.
//
// Replaces, behind r3dm_filter_F, the reference's
//   ImageCollectionGeometricFilter::Robust_model_estimation(GeometricFilter_FMatrix_AC(4.0, 2048), ...)
//   (src/R3DComputeMatches.cpp:2099,2113-2115), whose arithmetic is OpenMVG 1.4's
//   ACRANSAC + ACKernelAdaptor<SevenPointSolver, SymmetricEpipolarDistanceError> (SURVEY.md A.5).
//
// One workgroup per image pair.  AC-RANSAC is sequentially adaptive (the sampling pool shrinks to
// the inlier set on every meaningful improvement and the iteration budget is cut once), so the
// kernel keeps the reference's iteration ORDER and only parallelises inside it:
//   * a chunk of 64 minimal samples is drawn from the counter-based sample stream and solved
//     (7-point, f64, one lane per hypothesis, Householder QR null space + cubic);
//   * the <= 3 models of each iteration are then evaluated one after the other by all 256 lanes:
//     residuals of all m matches, wave-ballot compaction of those under the residual bound,
//     LDS bitonic sort of (residual, index), parallel NFA scan + argmin;
//   * when an iteration changes the pool, the rest of the chunk is discarded and re-drawn.
// Residuals beyond the bound never enter bestNFA's scan (its loop stops at the first one), so
// sorting only the sub-threshold set yields the same (NFA, k, inlier prefix) as the full sort.
//
// KIND 0: fundamental matrix (7-point, <= 3 models, symmetric epipolar error, point-to-line NFA scale)
// KIND 1: homography (4-point DLT, 1 model, asymmetric transfer error, point-to-point NFA scale)
// KIND 2: essential matrix (5-point on K^-1 x, <= 10 models, epipolar distance in pixels through F = K2^-T E K1^-1,
//         no normalisation of the points: ACKernelAdaptorEssential)
// KeyT / IdxT: the (residual, index) sort buffers live in LDS, or -- for the rare pair with more putative matches than
// the LDS budget holds (near-duplicate views with > 8192 matches) -- in a slice of global scratch.
// NT = threads of the workgroup: 256 (two workgroups per CU), or 512 for collections with long match lists (one workgroup per CU with
// the same registers per lane; every pass over the matches of a pair -- residuals, bound, sort, NFA scan -- takes half the trips)
template <int KIND, bool SPILL, int NT, class KeyT, class IdxT>
__device__ __forceinline__ void acransac_body(const FilterParams& P, double* __restrict__ pts, uint32_t* __restrict__ pool_g,
                                              float* __restrict__ logc_g, unsigned char* smem, KeyT keys, IdxT sidx, uint32_t item)
{
    FState& S = *reinterpret_cast<FState*>(smem);
    constexpr int MS = (KIND == 2) ? 90 : 27;                  // doubles per hypothesis: 9 x MAX_MODELS (27 also for H)
    double* Fs = reinterpret_cast<double*>(smem + kHdr);                                   // [64][MS]
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem + 1024);                             // [kHistBins]

    constexpr uint32_t SS = (KIND == 0) ? 7u : (KIND == 1 ? 4u : 5u);    // Kernel::MINIMUM_SAMPLES
    constexpr double MAXM = (KIND == 0) ? 3.0 : (KIND == 1 ? 1.0 : 10.0); // Kernel::MAX_MODELS
    constexpr double MULT_ERR = (KIND == 1) ? 1.0 : 0.5;       // multError(): point-to-point vs point-to-line
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    constexpr uint32_t NW = (uint32_t)NT / 64u;
    const uint64_t begin = P.offsets[2 * item], end = P.offsets[2 * item + 1];
    const uint32_t m = (uint32_t)(end - begin);
    const uint2 sl = P.pairs[item];
    const uint2 id = P.pair_ids[item];
    const ImgDev* __restrict__ Ip = P.imgs + sl.x;
    const ImgDev* __restrict__ Jp = P.imgs + sl.y;
    const r3dm_match* __restrict__ mm = P.matches + begin;
    // per-item slices of the global work arrays start at multiples of 32 elements (>= one 128-byte line for the narrowest
    // array): workgroups that share a CU -- and with it the vector L1 -- never share a cache line of data one of them is
    // still writing
    const uint64_t so = P.soff[item];
    // The positions of a pair's matches as the four FLOATS the views hold, 16 bytes per match (the first half of the slot a match has in
    // the points scratch): every reader re-forms the normalised f64 coordinates with the two operations that used to fill a 32-byte
    // record of doubles (bit-identical).  Round 4's PMC had this kernel fetch 7.4 GB per launch for 47 MB of input: two workgroups per
    // CU, 64 per XCD, each re-reading ~59 KB per model = the 4 MiB of an XCD's L2.  Half the footprint stays inside it.
    float4* __restrict__ pt = reinterpret_cast<float4*>(pts + 4 * so);
    uint32_t* __restrict__ pool = pool_g + so;
    uint32_t* __restrict__ inl = P.inl_idx + so;
    float* __restrict__ logc_n = logc_g + so;                 // m + 1 entries

    // ---- ACKernelAdaptor: normalisation N = [[s,0,-s w/2],[0,s,-s h/2],[0,0,1]], s = 1/sqrt(w h)
    const int wI = (int)Ip->width, hI = (int)Ip->height, wJ = (int)Jp->width, hJ = (int)Jp->height;
    const double s1 = (KIND == 2) ? 1.0 : 1.0 / sqrt((double)(wI * hI));
    const double s2 = (KIND == 2) ? 1.0 : 1.0 / sqrt((double)(wJ * hJ));
    const double t1x = (KIND == 2) ? 0.0 : -0.5 * wI * s1, t1y = (KIND == 2) ? 0.0 : -0.5 * hI * s1;
    const double t2x = (KIND == 2) ? 0.0 : -0.5 * wJ * s2, t2y = (KIND == 2) ? 0.0 : -0.5 * hJ * s2;
    const double* K1i = S.kinv;
    const double* K2i = S.kinv + 9;
    if (KIND == 2 && tid < 18) S.kinv[tid] = P.kinv[9 * (size_t)(tid < 9 ? sl.x : sl.y) + (tid < 9 ? tid : tid - 9)];
    for (uint32_t p = tid; p < m; p += NT) {
        const r3dm_match q = mm[p];
        pt[p] = make_float4(Ip->xy[2 * (size_t)q.i], Ip->xy[2 * (size_t)q.i + 1], Jp->xy[2 * (size_t)q.j], Jp->xy[2 * (size_t)q.j + 1]);
        pool[p] = p;
    }
    const double Dd = sqrt((double)wJ * (double)wJ + (double)hJ * (double)hJ);
    const double Aa = (double)wJ * (double)hJ;
    const double logalpha0 = (KIND == 0) ? log10(2.0 * Dd / Aa / s2)                       // 2 D / A / N2(0,0)
                           : (KIND == 1) ? log10(3.14159265358979323846 / Aa / (s2 * s2))   // pi / A / N2(0,0)^2
                                         : log10(2.0 * Dd / Aa * 0.5);                        // ACKernelAdaptorEssential
    const double maxThreshold = P.precision_px * P.precision_px * s2 * s2;
    const double loge0 = log10(MAXM * (double)(m - SS));
    // histogram bins: the top kHistSub + 12 bits of the residual's IEEE pattern (monotone for r >= 0), counted down from the
    // pattern of the largest residual that is kept; everything below the lowest bin shares bin 0 (lower edge 0)
    const long long hist_base = (__double_as_longlong(fmin(maxThreshold, 1.0e6)) >> kHistShift) - (long long)(kHistBins - 1);

    if (tid == 0) {
        // logcombi(k, m) as a running prefix in the reference's float accumulation order
        // (makelogcombi_n; SURVEY.md A.5): pre[i] = pre[i-1] + (l10[m-i+1] - l10[i]); mirrored for k > m/2
        float pre = 0.0f;
        logc_n[0] = 0.0f; logc_n[m] = 0.0f;
        for (uint32_t i = 1; i <= m / 2; ++i) {
            pre = pre + (P.log10_tab[m - i + 1] - P.log10_tab[i]);
            logc_n[i] = pre;
            if (m - i > i) logc_n[m - i] = pre;
        }
        S.minNFA = __builtin_huge_val(); S.errorMax = __builtin_huge_val();
        for (int e = 0; e < 9; ++e) S.bestF[e] = 0.0;
        const uint32_t reserve = P.max_iter / 10;
        S.reserve = reserve; S.nIter = P.max_iter - reserve; S.iter = 0;
        S.pool_size = m; S.n_inl = 0; S.acMode = !(P.precision_px < __builtin_huge_val());
        S.n_models = 0; S.iters_done = 0;
        S.cnt = 0u;
    }
#pragma unroll
    for (int j = 0; j < kHistBins / NT; ++j) hist[tid + NT * j] = 0u;
    // the scout pass (scout_model above): on in the product; the developer build can switch it off (A/B, parity of the two walks) and
    // its traces / invariant checks take the full evaluation for every model
    // (developer build: R3DM_FILTER_SCOUT=2 -- the scout divides like the full evaluation; =3 with R3DM_FILTER_CHECK=1 -- the scout runs,
    // nothing is skipped, and every model's count and NFA are checked against what the scout promised: invariants 9 and 10)
    const uint32_t scout_mode = P.scout & 0xFFu;
    const bool scout_check = scout_mode >= 3u && R3DM_DBG(P) && !R3DM_TRACE(P);
    const bool scout_on = scout_mode != 0u && P.la_tab != nullptr && !R3DM_TRACE(P) && (!R3DM_DBG(P) || scout_check);
    const bool scout_exact = scout_mode == 2u || scout_mode == 5u;
    double* __restrict__ la_g = P.la_tab ? P.la_tab + (size_t)item * kHistBins : nullptr;
    if (scout_on) {
#pragma unroll
        for (int j = 0; j < kHistBins / NT; ++j) {
            const uint32_t b = tid + (uint32_t)NT * (uint32_t)j;
            const double edge = b ? __longlong_as_double(((long long)b + hist_base) << kHistShift) : 0.0;
            la_g[b] = logalpha0 + MULT_ERR * log10(edge + FLT_EPS_D);
        }
    }
    // walk state every thread keeps for itself (all threads take the same decisions on the same shared values): AC mode, models walked,
    // iterations done -- the full evaluation used to keep them in LDS behind a barrier per model
    bool ac_reg = !(P.precision_px < __builtin_huge_val());
    uint32_t nmod_reg = 0, iters_done_reg = 0;
    wg_sync_global();          // points, pool, logcombi and slope tables go through global memory
    // what the float accumulation of the log-binomial tables (orc_logcombi_tables: <= m / 2 additions of float log10 differences, each
    // rounded at the running sum's ulp) can move them away from a concave sequence, twice: drift <= (m / 2) (2^-25 max + 2^-21)
    const double scout_slack = scout_on ? 0x1p-24 * (double)m * ((double)logc_n[m / 2u] + 32.0) + 1.0e-4 : 0.0;

    E_TIME(unsigned long long cyc_solve = 0, cyc_eval = 0, cyc_t0 = 0, cyc_res = 0, cyc_sort = 0;)
    while (true) {
        wg_sync_t<SPILL>();
        E_TIME(cyc_t0 = __builtin_readcyclecounter();)
        const uint32_t iter0 = S.iter, nIter0 = S.nIter;
        uint32_t nIter_reg = nIter0, reserve_reg = S.reserve;
        if (iter0 >= nIter0) break;
        constexpr uint32_t CH = (uint32_t)ChunkOf<KIND>::n;
        const uint32_t chunk_n = (nIter0 - iter0 < CH) ? nIter0 - iter0 : CH;
        // the hypothesis of the chunk this lane works on: lane c of wave 0 for F / H, the 16-lane group tid / 16 for E
        const uint32_t hyp = (KIND == 2) ? (tid >> 4) : tid;             // (threads beyond the first 256 of the wide variant draw nothing: hyp >= 16)
        const uint32_t pool_size = S.pool_size;

        // ---- draw + solve one chunk of minimal samples (hypothesis c <-> iteration iter0 + c)
        if ((KIND == 2 || tid < (uint32_t)kChunk) && hyp < chunk_n) {
            uint32_t pos[7];
            uint32_t cnt = 0, attempt = 0;
            while (cnt < SS) {
                const uint64_t r = rng_u64(P.seed, id.x, id.y, iter0 + hyp, attempt++);
                const uint32_t ps = (uint32_t)(((r >> 32) * (uint64_t)pool_size) >> 32);
                bool dup = false;
#pragma unroll
                for (int k = 0; k < 7; ++k) dup |= (k < (int)cnt) && (pos[k] == ps);
                if (!dup) {
#pragma unroll
                    for (int k = 0; k < 7; ++k) if (k == (int)cnt) pos[k] = ps;
                    ++cnt;
                }
            }
            double px1[7][2], px2[7][2];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                uint32_t sidx_ = pool[pos[k < (int)SS ? k : 0]];
                FCHECK(pos[k < (int)SS ? k : 0] < pool_size, 1, pos[k < (int)SS ? k : 0], pool_size);
                FCHECK(sidx_ < m, 2, sidx_, m);
                if (R3DM_DBG(P) && sidx_ >= m) sidx_ = 0;
                const float4 f4 = pt[sidx_];
                px1[k][0] = s1 * (double)f4.x + t1x; px1[k][1] = s1 * (double)f4.y + t1y;
                px2[k][0] = s2 * (double)f4.z + t2x; px2[k][1] = s2 * (double)f4.w + t2y;
                if (KIND == 2) {                 // camera coordinates: hnormalized(K^-1 (x, y, 1))
                    const double xa = px1[k][0], ya = px1[k][1], xb = px2[k][0], yb = px2[k][1];
                    const double w1 = K1i[6] * xa + K1i[7] * ya + K1i[8];
                    px1[k][0] = (K1i[0] * xa + K1i[1] * ya + K1i[2]) / w1;
                    px1[k][1] = (K1i[3] * xa + K1i[4] * ya + K1i[5]) / w1;
                    const double w2 = K2i[6] * xb + K2i[7] * yb + K2i[8];
                    px2[k][0] = (K2i[0] * xb + K2i[1] * yb + K2i[2]) / w2;
                    px2[k][1] = (K2i[3] * xb + K2i[4] * yb + K2i[5]) / w2;
                }
            }
            if constexpr (KIND == 2) {
                // the 16 lanes of the group solve the sample together; the models go straight into the hypothesis' LDS slots, the
                // workspaces are the region behind the hypothesis buffer (the sort buffers of the evaluation phase, idle during the solves)
                double* W = reinterpret_cast<double*>(smem + kHdr + CH * MS * 8) + (size_t)hyp * kE5Stride;
                const int l = (int)(tid & 15u);
                const int nm = five_point_coop(px1, px2, Fs + hyp * MS, W, l);
                for (int e = 9 * nm + l; e < MS; e += kE5Lanes) Fs[hyp * MS + e] = 0.0;
                if (l == 0) {
                    S.nm[hyp] = (uint32_t)nm;
                    if (R3DM_TRACE(P)) S.dbg_smp[hyp] = pool[pos[0]];
                    if (R3DM_TRACE(P) && item == P.trace_item && iter0 + hyp == P.trace_iter) {
                        double* t = P.trace + 5 * (size_t)(P.trace_cap - 4);
                        for (int k = 0; k < 7; ++k) t[k] = (double)pool[pos[k < (int)SS ? k : 0]];
                        t[7] = nm; t[8] = pool_size; t[9] = iter0 + hyp;
                        for (int k = 0; k < 7; ++k) t[10 + k] = (double)pos[k < (int)SS ? k : 0];
                    }
                    if (R3DM_TRACE(P) && hyp == 0) S.dbg_pool = pool_size;
                }
            } else {
                double F3[MS];
                int nm;
                if constexpr (KIND == 0) nm = seven_point(px1, px2, F3);
                else nm = four_point_h(px1, px2, F3);
                S.nm[tid] = (uint32_t)nm;
                if (R3DM_TRACE(P)) S.dbg_smp[tid] = pool[pos[0]];
                if (R3DM_TRACE(P) && item == P.trace_item && iter0 + tid == P.trace_iter) {
                    double* t = P.trace + 5 * (size_t)(P.trace_cap - 4);
                    for (int k = 0; k < 7; ++k) t[k] = (double)pool[pos[k]];
                    t[7] = nm; t[8] = pool_size; t[9] = iter0 + tid;
                    for (int k = 0; k < 7; ++k) t[10 + k] = (double)pos[k];
                }
                if (R3DM_TRACE(P) && tid == 0) S.dbg_pool = pool_size;
                for (int e = 0; e < MS; ++e) Fs[tid * MS + e] = (e < 9 * nm) ? F3[e] : 0.0;
            }
        }
        wg_sync_t<SPILL>();
        E_TIME({ const unsigned long long now = __builtin_readcyclecounter(); cyc_solve += now - cyc_t0; cyc_t0 = now; })

        // ---- flat offsets of the chunk's models (scout pass): moff[c] = models of the hypotheses before c
        uint32_t* __restrict__ sc_total = reinterpret_cast<uint32_t*>(smem + kHdr + CH * MS * 8);
        double* __restrict__ sc_bound = reinterpret_cast<double*>(sc_total + kScoutModels);
        uint32_t* __restrict__ moff = reinterpret_cast<uint32_t*>(sc_bound + kScoutModels);
        uint32_t* __restrict__ whist = reinterpret_cast<uint32_t*>(smem + kHdr + CH * MS * 8 + kScoutBytes) + wave * (uint32_t)kHistBins;   // (the idle LDS sort buffers)
        if (scout_on) {
            if (tid <= chunk_n) { uint32_t o = 0; for (uint32_t j = 0; j < tid; ++j) o += S.nm[j]; moff[tid] = o; }
            wg_sync_t<SPILL>();
        }
        uint32_t scouted = 0;                          // models [0, scouted) of the chunk hold scout results

        // ---- evaluate the chunk's iterations in order
        bool pool_changed = false;
        uint32_t c = 0;
        for (; c < chunk_n && !pool_changed; ++c) {
            const uint32_t it = iter0 + c;
            const uint32_t nm = S.nm[c];
            bool better = false;
            for (uint32_t k = 0; k < nm; ++k) {
                [[maybe_unused]] uint32_t chk_tot = 0u; [[maybe_unused]] double chk_bound = -__builtin_huge_val();
                if (scout_on) {
                    const uint32_t f = moff[c] + k;
                    if (f >= scouted) {
                        // scout the next sub-batch of models (a pool change discards what lies behind it)
                        const uint32_t n_chunk_models = moff[chunk_n];
                        // (two per wavefront: what lies behind an accepted model is scouted for nothing -- 16 per wavefront cost F 10.2 ms where 2 cost 6.9;
                        //  developer build: R3DM_FILTER_SCOUT_SUB)
                        const uint32_t sub_n = (P.scout >> 8) ? (P.scout >> 8) * NW : 2u * NW;
                        const uint32_t end_f = scouted + sub_n < n_chunk_models ? scouted + sub_n : n_chunk_models;
                        const bool want_bound = S.minNFA < __builtin_huge_val();
                        for (uint32_t fi = scouted + wave; fi < end_f; fi += NW) {
                            const bool hit = lane < chunk_n && moff[lane] <= fi && fi < moff[lane + 1u];
                            const uint32_t cc = (uint32_t)__builtin_ctzll(__ballot(hit));
                            const uint32_t kk = fi - moff[cc];
                            scout_model<KIND>(pt, m, Fs + cc * MS + kk * 9, S.kinv, s1, t1x, t1y, s2, t2x, t2y, maxThreshold, hist_base, want_bound,
                                              la_g, logc_n, P.logc_k, loge0, whist, lane, sc_total + fi, sc_bound + fi, scout_exact, scout_slack);
                        }
                        wg_sync_t<SPILL>();
                        scouted = end_f;
                    }
                    // can the full evaluation accept this model?  Not below AC mode's 2.5 x sample size, not with SS or fewer matches
                    // within the bound, not when the best NFA its residual histogram allows is above the best so far
                    const uint32_t tot_w = sc_total[f], tot_f = tot_w & ~kScoutOpen;
                    const double bound_f = sc_bound[f], minNFA_f = S.minNFA;
                    const bool ac_f = ac_reg || ((double)tot_f > 2.5 * SS);
                    const bool skip = !(tot_w & kScoutOpen) &&
                                      (!(ac_f && tot_f > SS) ||
                                       (bound_f > -__builtin_huge_val() && minNFA_f < __builtin_huge_val() && bound_f - 1.0e-6 >= minNFA_f));
                    if (skip && !scout_check) { ac_reg = ac_f; nmod_reg += 1; continue; }
                    chk_tot = tot_w; chk_bound = bound_f;
                }
                double F[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) F[e] = Fs[c * MS + k * 9 + e];
                double FE[9];
                if (KIND == 2) f_from_e(F, K1i, K2i, FE);
                // residuals + compaction of those within the bound
                E_TIME(const unsigned long long cyc_m0 = __builtin_readcyclecounter();)
                // (order of the compacted entries: whatever the atomics give -- the sort below fixes the order, `total` and the
                // set do not depend on it)
                // (S.cnt and the histogram are zero here: cleared once at kernel start and again at the end of every model, behind the
                // barrier that closes it -- one barrier less per model than clearing them here)
                // four batches of 256 matches per trip: the point loads (global memory, 16 bytes per match) of all four are in
                // flight before the first residual is needed
                for (uint32_t base = 0; base < m; base += 4u * NT) {
                    double r[4]; bool in[4];
                    double px[4][4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t p = base + (uint32_t)NT * (uint32_t)u + tid;
                        const float4 f4 = pt[p < m ? p : 0u];
                        px[u][0] = s1 * (double)f4.x + t1x; px[u][1] = s1 * (double)f4.y + t1y;
                        px[u][2] = s2 * (double)f4.z + t2x; px[u][3] = s2 * (double)f4.w + t2y;
                    }
                    unsigned long long bal[4];
                    uint32_t n_new = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t p = base + (uint32_t)NT * (uint32_t)u + tid;
                        r[u] = (KIND == 0) ? sym_epipolar_err(F, px[u][0], px[u][1], px[u][2], px[u][3])
                             : (KIND == 1) ? h_asym_err(F, px[u][0], px[u][1], px[u][2], px[u][3])
                                           : epipolar_dist_err(FE, px[u][0], px[u][1], px[u][2], px[u][3]);
                        in[u] = (p < m) && (r[u] <= maxThreshold);
                        bal[u] = __ballot(in[u]);
                        n_new += (uint32_t)__builtin_popcountll(bal[u]);
                    }
                    if (n_new != 0u) {
                        uint32_t woff = 0;
                        if (lane == 0) woff = atomicAdd(&S.cnt, n_new);
                        woff = (uint32_t)__builtin_amdgcn_readfirstlane((int)woff);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const uint32_t pos = woff + (uint32_t)__builtin_popcountll(bal[u] & ((1ull << lane) - 1ull));
                            FCHECK(pos < m || !in[u], 3, pos, m);
                            if (in[u]) {
                                keys[pos] = (unsigned long long)__double_as_longlong(r[u]); sidx[pos] = base + (uint32_t)NT * (uint32_t)u + tid;
                                long long bin = (__double_as_longlong(r[u]) >> kHistShift) - hist_base;
                                bin = bin < 0 ? 0 : (bin > kHistBins - 1 ? kHistBins - 1 : bin);
                                atomicAdd(&hist[bin], 1u);
                            }
                            woff += (uint32_t)__builtin_popcountll(bal[u]);
                        }
                    }
                }
                wg_sync_t<SPILL>();
                const uint32_t total = S.cnt;
                E_TIME(const unsigned long long cyc_m1 = __builtin_readcyclecounter(); cyc_res += cyc_m1 - cyc_m0;)
                // AC mode switches on with the first model that has > 2.5*7 points within the bound
                bool ac = ac_reg;
                if (!ac && (double)total > 2.5 * SS) ac = true;
                double nfa = __builtin_huge_val();
                uint32_t kbest = SS;
                [[maybe_unused]] double S_bound = -__builtin_huge_val();
                // ---- can this model beat the best NFA at all?  The k-th smallest residual lies in the histogram bin where the
                // running count reaches k, so it is at least that bin's lower edge; the NFA term of k grows with the residual
                // (k > SS), hence NFA_k >= the same expression on the edge, evaluated with the same operations.  A model whose
                // bound over all k stays above the best NFA so far cannot be committed: no sort, no NFA scan (98 % of the models
                // on C2's pairs, DESIGN.md section 4.4).  The margin covers log10's last-bit non-monotonicity (effect < 1e-10).
                bool hopeless = false;
                if (ac && total > SS && S.minNFA < __builtin_huge_val() && !R3DM_TRACE(P)) {
                    // inclusive running counts, 4 consecutive bins per thread, written back in place
                    uint32_t cb[kHistBins / NT];
                    uint32_t run = 0;
#pragma unroll
                    for (int j = 0; j < kHistBins / NT; ++j) { run += hist[tid * (kHistBins / NT) + j]; cb[j] = run; }
                    uint32_t incl = run;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, off); if (lane >= (uint32_t)off) incl += o; }
                    if (lane == 63) S.wave_cnt[wave] = incl;
                    wg_sync_t<SPILL>();
                    uint32_t excl = incl - run;
#pragma unroll
                    for (uint32_t w = 0; w < NW; ++w) if (w < wave) excl += S.wave_cnt[w];
#pragma unroll
                    for (int j = 0; j < kHistBins / NT; ++j) hist[tid * (kHistBins / NT) + j] = excl + cb[j];
                    wg_sync_t<SPILL>();
                    // bins tid, tid + 256, ...: neighbouring (equally dense) bins go to different threads
                    double wmin = __builtin_huge_val();
#pragma unroll
                    for (int j = 0; j < kHistBins / NT; ++j) {
                        const uint32_t b = tid + (uint32_t)NT * (uint32_t)j;
                        const uint32_t k_hi = hist[b], k_prev = b ? hist[b - 1] : 0u;
                        uint32_t k_lo = k_prev + 1u; if (k_lo < SS + 1u) k_lo = SS + 1u;
                        if (k_hi >= k_lo) {
                            const double edge = b ? __longlong_as_double(((long long)b + hist_base) << kHistShift) : 0.0;
                            const double la = logalpha0 + MULT_ERR * log10(edge + FLT_EPS_D);
                            for (uint32_t kk = k_lo; kk <= k_hi; ++kk) {
                                const double w = loge0 + la * (double)(kk - SS) + (double)logc_n[kk] + (double)P.logc_k[kk];
                                wmin = w < wmin ? w : wmin;
                            }
                        }
                    }
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(wmin, off); wmin = o < wmin ? o : wmin; }
                    if (lane == 0) S.red_b[wave] = wmin;
                    wg_sync_t<SPILL>();
                    wmin = S.red_b[0];
#pragma unroll
                    for (uint32_t w = 1; w < NW; ++w) wmin = fmin(wmin, S.red_b[w]);      // (own slots: the NFA reduction below uses red_v, no barrier in between)
                    hopeless = !R3DM_DBG(P) && (wmin - 1.0e-6 >= S.minNFA);
                    if (R3DM_DBG(P)) S_bound = wmin;              // developer build: nothing is skipped, the bound is checked against the NFA
                }
                if (ac && total > SS && !hopeless) {
                    // sort (residual, index) ascending: residuals are >= 0 so the u64 bit pattern orders them
                    uint32_t cap = 1; while (cap < total) cap <<= 1;
                    // (the 256-thread variant keeps its spilled lists on the plain network, as before: the register sort of a
                    // global list is instantiated for the wide variant only)
                    bool sorted = !SPILL || NT == 512;
                    if constexpr (!SPILL || NT == 512)
                    switch (cap / (uint32_t)NT) {
                        case 0: case 1: wg_sort_regs<1, SPILL>(keys, sidx, cap, total, tid); break;
                        case 2: wg_sort_regs<2, SPILL>(keys, sidx, cap, total, tid); break;
                        case 4: wg_sort_regs<4, SPILL>(keys, sidx, cap, total, tid); break;
                        case 8: wg_sort_regs<8, SPILL>(keys, sidx, cap, total, tid); break;
                        case 16: wg_sort_regs<16, SPILL>(keys, sidx, cap, total, tid); break;
                        case 32: wg_sort_regs<32, SPILL>(keys, sidx, cap, total, tid); break;
                        default: sorted = false; break;               // longer lists: the plain network below
                    }
                    if (!sorted) {
                    for (uint32_t q = total + tid; q < cap; q += NT) { keys[q] = ~0ull; sidx[q] = 0xFFFFFFFFu; }
                    wg_sync_t<SPILL>();
                    for (uint32_t size = 2; size <= cap; size <<= 1) {
                        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                            for (uint32_t tI = tid; tI < (cap >> 1); tI += NT) {
                                const uint32_t lo = 2 * tI - (tI & (stride - 1));
                                const uint32_t hi = lo + stride;
                                const bool up = ((lo & size) == 0);
                                const unsigned long long x = keys[lo], y = keys[hi];
                                const uint32_t xi = sidx[lo], yi = sidx[hi];
                                const bool gt = (x > y) || (x == y && xi > yi);
                                if (gt == up) { keys[lo] = y; keys[hi] = x; sidx[lo] = yi; sidx[hi] = xi; }
                            }
                            wg_sync_t<SPILL>();
                        }
                    }
                    }
                    E_TIME(cyc_sort += __builtin_readcyclecounter() - cyc_m1;)
                    // bestNFA: k = 8 .. total, first minimum wins
                    double bv = __builtin_huge_val(); uint32_t bk = 0xFFFFFFFFu;
                    for (uint32_t kk = SS + 1 + tid; kk <= total; kk += NT) {
                        const double e = __longlong_as_double((long long)keys[kk - 1]);
                        const double logalpha = logalpha0 + MULT_ERR * log10(e + FLT_EPS_D);
                        const double v = loge0 + logalpha * (double)(kk - SS) + (double)logc_n[kk] + (double)P.logc_k[kk];
                        if (v < bv) { bv = v; bk = kk; }
                    }
                    // wave argmin (value, then smaller k), then across the 4 waves
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) {
                        const double ov = __shfl_xor(bv, off);
                        const uint32_t ok = __shfl_xor(bk, off);
                        if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
                    }
                    if (lane == 0) { S.red_v[wave] = bv; S.red_k[wave] = bk; }
                    wg_sync_t<SPILL>();
#pragma unroll
                    for (uint32_t w = 0; w < NW; ++w) {
                        const double ov = S.red_v[w]; const uint32_t ok = S.red_k[w];
                        if (w == 0 || ov < nfa || (ov == nfa && ok < kbest)) { nfa = ov; kbest = ok; }
                    }
                    if (kbest == 0xFFFFFFFFu) { nfa = __builtin_huge_val(); kbest = SS; }
                }
                // commit (every lane evaluates the same condition on the same shared values)
                const double minNFA = S.minNFA;
                const bool improve = ac && (nfa < minNFA);
                FCHECK(!improve || (kbest <= total && kbest > SS), 4, kbest, total);
                FCHECK(S_bound - 1.0e-6 <= nfa, 8, kbest, total);                 // the sort-skipping bound really is one
                if (scout_check) {
                    const uint32_t ct = chk_tot & ~kScoutOpen;
                    FCHECK(ct >= total && ((chk_tot & kScoutOpen) || (((double)ct > 2.5 * SS) == ((double)total > 2.5 * SS) && (ct > SS) == (total > SS))), 9, ct, total);
                    FCHECK(!(ac && total > SS) || !(S_bound > -__builtin_huge_val()) || chk_bound <= S_bound + 1.0e-9, 11, __float_as_uint((float)chk_bound), __float_as_uint((float)S_bound));   // ... the scout's bound is the full evaluation's, or below it
                    FCHECK(!(ac && total > SS) || chk_bound - 1.0e-6 <= nfa, 10, __float_as_uint((float)chk_bound), __float_as_uint((float)nfa));     // ... and so is the scout's
                }
                if (improve) {
                    for (uint32_t q = tid; q < kbest; q += NT) inl[q] = sidx[q];
                    better = true;
                }
                wg_sync_t<SPILL>();
                if (tid == 0) {
                    if (R3DM_TRACE(P) && item == P.trace_item) {
                        const uint32_t row = *P.trace_rows;
                        if (row < P.trace_cap) {
                            double* t = P.trace + 5 * (size_t)row;
                            t[0] = it; t[1] = k + 10.0 * S.dbg_smp[c]; t[2] = total + 10000.0 * S.dbg_pool; t[3] = nfa; t[4] = (improve ? 1.0 : 0.0) + 2.0 * kbest;
                            *P.trace_rows = row + 1;
                        }
                    }
                    S.acMode = ac ? 1u : 0u;
                    if (improve) {
                        S.minNFA = nfa;
                        S.n_inl = kbest;
                        S.errorMax = __longlong_as_double((long long)keys[kbest - 1]);
#pragma unroll
                        for (int e = 0; e < 9; ++e) S.bestF[e] = F[e];
                    }
                    S.cnt = 0u;                                   // for the next model (every reader of this model's count is behind the barrier above)
                }
#pragma unroll
                for (int j = 0; j < kHistBins / NT; ++j) hist[tid + NT * j] = 0u;     // ... and its histogram: last read before the commit barrier
                ac_reg = ac; nmod_reg += 1;
                wg_sync_t<SPILL>();
            }
            // ---- end of iteration `it`, the common case: no model of it was accepted and the iteration budget does not end here --
            // nothing shared changes (ACRANSAC's pool / budget update below cannot trigger)
            if (scout_on && !better && !(it + 1 == nIter_reg && reserve_reg != 0u)) {
                iters_done_reg = it + 1;
                if (it + 1 >= nIter_reg) { ++c; break; }
                continue;
            }
            // ---- end of iteration `it`: ACRANSAC's pool / budget update.  Thread 0 is about to change the loop bounds that
            // the other waves read right after the previous iteration's last barrier; every evaluated model ends with a
            // barrier, a sample without real solutions (nm == 0, common for the 5-point solver) needs its own.
            if (nm == 0) wg_sync_t<SPILL>();
            if (tid == 0) {
                S.iters_done = it + 1;
                S.flag = 0;
                const bool trigger = (better && S.minNFA < 0.0) || (it + 1 == S.nIter && S.reserve != 0);
                if (trigger) {
                    if (S.n_inl == 0) { S.nIter += 1; S.reserve -= 1; }
                    else {
                        S.flag = 1;
                        S.pool_size = S.n_inl;
                        if (S.reserve) { S.nIter = it + 1 + S.reserve; S.reserve = 0; }
                    }
                }
            }
            wg_sync_t<SPILL>();
            if (S.flag) {
                // new sampling pool = the inlier SET in ascending index order.  (The residual order of the
                // inlier list is rounding noise among the 7 points the model was fitted to, so pool
                // positions must not depend on it -- same rule in oracle/acransac.c.)
                const uint32_t ni = S.n_inl;
                IdxT flags = sidx;                                       // sort scratch, free between models
                for (uint32_t q = tid; q < m; q += NT) flags[q] = 0u;
                wg_sync_t<SPILL>();
                FCHECK(ni <= m, 5, ni, m);
                for (uint32_t q = tid; q < ni; q += NT) { const uint32_t iq = inl[q]; FCHECK(iq < m, 6, iq, q); if (!R3DM_DBG(P) || iq < m) flags[iq] = 1u; }
                wg_sync_t<SPILL>();
                uint32_t filled = 0;
                for (uint32_t base = 0; base < m; base += NT) {
                    const uint32_t p = base + tid;
                    const bool in = (p < m) && (flags[p] != 0u);
                    const unsigned long long bal = __ballot(in);
                    const uint32_t before = (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
                    if (lane == 0) S.wave_cnt[wave] = (uint32_t)__builtin_popcountll(bal);
                    wg_sync_t<SPILL>();
                    uint32_t woff = 0, tot = 0;
#pragma unroll
                    for (uint32_t w = 0; w < NW; ++w) { const uint32_t cw = S.wave_cnt[w]; if (w < wave) woff += cw; tot += cw; }
                    if (in) pool[filled + woff + before] = p;
                    filled += tot;
                    wg_sync_t<SPILL>();
                }
                FCHECK(filled == ni, 7, filled, ni);
                pool_changed = true;
                wg_fence();            // the rebuilt pool (global memory) is read by the sampling lanes of the next chunk (same workgroup)
            }
            wg_sync_t<SPILL>();
            iters_done_reg = it + 1;
            nIter_reg = S.nIter; reserve_reg = S.reserve;
            // the chunk was cut from the old budget: stop when the (possibly shrunk) budget is exhausted
            if (it + 1 >= S.nIter) { ++c; break; }
        }
        if (tid == 0) S.iter = iter0 + c;
        E_TIME(cyc_eval += __builtin_readcyclecounter() - cyc_t0;)
    }

    // ---- result
    wg_sync_t<SPILL>();
    if (tid == 0) {
        uint32_t n_inl = S.n_inl;
        if (!(S.minNFA < 0.0)) n_inl = 0;
        P.inl_count[item] = n_inl;
        double Fo[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        double thr = 0.0;
        if (n_inl > 0) {
            // Unnormalize: F = N2^T * F * N1 (UnnormalizerT) ; H = N2^-1 * H * N1 (UnnormalizerI)
            const double N1[9] = {s1, 0, t1x, 0, s1, t1y, 0, 0, 1};
            const double N2[9] = {s2, 0, t2x, 0, s2, t2y, 0, 0, 1};
            const double N2i[9] = {1.0 / s2, 0, -t2x / s2, 0, 1.0 / s2, -t2y / s2, 0, 0, 1};
            double T[9];
            for (int r = 0; r < 3; ++r)
                for (int cc = 0; cc < 3; ++cc) {
                    double v = 0.0;
                    for (int k = 0; k < 3; ++k) v += ((KIND == 0) ? N2[3 * k + r] : N2i[3 * r + k]) * S.bestF[3 * k + cc];
                    T[3 * r + cc] = v;
                }
            for (int r = 0; r < 3; ++r)
                for (int cc = 0; cc < 3; ++cc) {
                    double v = 0.0;
                    for (int k = 0; k < 3; ++k) v += T[3 * r + k] * N1[3 * k + cc];
                    Fo[3 * r + cc] = v;
                }
            thr = sqrt(S.errorMax) / s2;
            if (KIND == 2) { for (int e = 0; e < 9; ++e) Fo[e] = S.bestF[e]; thr = S.errorMax; }   // E itself; unormalizeError(e) = e
        }
        for (int e = 0; e < 9; ++e) P.F_out[9 * (size_t)item + e] = Fo[e];
        P.thr_nfa[2 * (size_t)item] = thr;
        P.thr_nfa[2 * (size_t)item + 1] = S.minNFA;
        // timing build only: cycles of wave 0 in the solve and the evaluation phases instead of (threshold, NFA); integers below 2^40, so
        // both of a pair survive in one double
        E_TIME(P.thr_nfa[2 * (size_t)item] = (double)cyc_solve + 1e-12 * (double)cyc_res; P.thr_nfa[2 * (size_t)item + 1] = (double)cyc_eval + 1e-12 * (double)cyc_sort;)
        P.iters[2 * (size_t)item] = iters_done_reg;
        P.iters[2 * (size_t)item + 1] = nmod_reg;
    }
}

// Two workgroups per CU for F and H (256 registers per lane; the F kernel trades 42 spilled VGPRs of its cold solver path
// for the second workgroup: 40.0 -> 24.8 ms on the 790 pairs of C2, three per CU at 168 registers gains nothing more);
// E likewise since its 5-point solver became a cooperative LDS routine.  The wide variant (NT = 512, one workgroup per CU, the same
// registers per lane) serves collections with long match lists: FilterParams::wide, set by the host (api_filter.cpp).
template <int KIND, int NT>
__device__ __forceinline__ void acransac_item(const FilterParams& P, unsigned char* smem, uint32_t block)
{
    constexpr int MS = (KIND == 2) ? 90 : 27;
    const uint32_t item = P.order ? P.order[block] : block;
    const uint32_t m = (uint32_t)(P.offsets[2 * item + 1] - P.offsets[2 * item]);
    if (m <= P.m_cap) {
        unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + kHdr + ChunkOf<KIND>::n * MS * 8 + kScoutBytes);
        uint32_t* sidx = reinterpret_cast<uint32_t*>(keys + P.m_cap);
        acransac_body<KIND, false, NT>(P, P.pts_scratch, P.pool_scratch, P.scratch_logc, smem, keys, sidx, item);
    } else {
        // slice of the global spill buffer, sized for the next power of two of m (host: spill_off[item])
        unsigned long long* keys = P.spill_keys + P.spill_off[item];
        uint32_t* sidx = P.spill_idx + P.spill_off[item];
        acransac_body<KIND, true, NT>(P, P.pts_scratch, P.pool_scratch, P.scratch_logc, smem, keys, sidx, item);
    }
}

template <int KIND, int NT>
__global__ __launch_bounds__(NT, NT == 256 ? 2 : 1)
void acransac_kernel(const FilterParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    acransac_item<KIND, NT>(P, smem, blockIdx.x);
}

template <int KIND, int NT>
static hipError_t launch_acransac(hipStream_t st, const FilterParams& P, size_t lds)
{
    hipError_t e = hipFuncSetAttribute((const void*)acransac_kernel<KIND, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((acransac_kernel<KIND, NT>), dim3(P.n_short), dim3(NT), lds, st, P);
    return hipGetLastError();
}

}  // namespace r3dm
