// api_guided.cpp -- part of the host side of libr3dm.so: guided matching (include/r3dm.h: r3dm_guided_match, r3dm_set_guided_matching,
// r3dm_guided_report).  The kernels are kernels_guided.hip; the filters (api_filter.cpp) run the same step for their accepted pairs
// when the context's switch is on.  Restated from OpenMVG's ImageCollectionGeometricFilter::Robust_model_estimation(.., bGuided_matching
// = true, dDistanceRatio) and geometry_aware::GuidedMatching ("Guided matching"); the reference binds only false
// (the reference's src/R3DComputeMatches.cpp:2113-2114,2169-2170,2215-2218).
#include "r3dm_ctx.hpp"

#include <memory>

// FundamentalFromEssential: F = K_J^-T E K_I^-1, operation for operation what oracle/essential.c orc_f_from_e does
static void f_from_e(const double* E, const double* K1i, const double* K2i, double* F)
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

int guided_job_make(r3dm_ctx* c, uint32_t sI, uint32_t sJ, int pub_kind, const double* M, double thr_px, double ratio, GuidedJob& out)
{
    const HostImage& A = *c->imgs[sI];
    const HostImage& B = *c->imgs[sJ];
    if (!A.has_xy || !B.has_xy) { c->err = "guided matching: view registered without feature positions"; return R3DM_ERR_INVALID; }
    out = GuidedJob{};
    if (pub_kind == R3DM_GUIDED_E) {
        if (!A.has_K || !B.has_K) { c->err = "guided matching (E): both views need r3dm_set_intrinsics"; return R3DM_ERR_INVALID; }
        f_from_e(M, A.Kinv, B.Kinv, out.M);
    } else {
        memcpy(out.M, M, sizeof(out.M));
    }
    out.kind = pub_kind == R3DM_GUIDED_H ? 1u : 0u;
    out.errTh = thr_px * thr_px;                  // Square(m_dPrecision_robust), for every kind (E: the square of a squared bound)
    out.sI = sI; out.sJ = sJ; out.nI = A.n;
    if (ratio >= 0.0) {
        if (A.dtype != B.dtype && (A.dtype == R3DM_BIN || B.dtype == R3DM_BIN)) { c->err = "guided matching: binary and real-valued views in one pair"; return R3DM_ERR_INVALID; }
        if (A.dim != B.dim) { c->err = "guided matching: descriptor lengths of the pair differ"; return R3DM_ERR_INVALID; }
        out.flags |= kGuidedDesc;
        if (A.dtype == R3DM_BIN) out.flags |= kGuidedBin;
        out.R = ratio * ratio;
    } else if (pub_kind == R3DM_GUIDED_H) {
        out.flags |= kGuidedDedup;
    }
    return R3DM_OK;
}

int guided_run(r3dm_ctx* c, std::vector<GuidedJob>& jobs, GuidedResult& R)
{
    const double t0 = now_ms();
    c->guided_stats = r3dm_guided_stats{};
    R = GuidedResult{};
    R.cnt.assign(jobs.size(), 0u);
    if (jobs.empty()) return R3DM_OK;
    R3DM_HIP(c, hipSetDevice(c->device));
    GuidedBufs& B = c->gb;
    // descriptor mode reads the row-major rows of real-valued views (a layout staged on first use, like every other on-demand one)
    std::vector<uint32_t> need_rows;
    bool any_desc = false;
    for (const GuidedJob& j : jobs) {
        if (!(j.flags & kGuidedDesc)) continue;
        any_desc = true;
        if (!(j.flags & kGuidedBin)) { need_rows.push_back(j.sI); need_rows.push_back(j.sJ); }
    }
    if (!need_rows.empty()) { const int rc = ensure_layouts(c, need_rows, kLayRows); if (rc != R3DM_OK) return rc; }
    uint64_t Q = 0, NB = 0;
    for (GuidedJob& j : jobs) {
        j.q0 = (uint32_t)Q; j.b0 = (uint32_t)NB;
        Q += j.nI; NB += (j.nI + 255u) / 256u;
        if (Q >= 0xFFFFFFFFull) { c->err = "guided matching: more than 4G queries in one call"; return R3DM_ERR_UNSUPPORTED; }
    }
    const size_t NJ = jobs.size();
    R3DM_HIP(c, B.jobs.ensure(NJ * sizeof(GuidedJob)));
    R3DM_HIP(c, B.res.ensure(4 * std::max<uint64_t>(Q, 1)));
    R3DM_HIP(c, B.q_cnt.ensure(4 * std::max<uint64_t>(Q, 1)));
    R3DM_HIP(c, B.q_off.ensure(8 * std::max<uint64_t>(Q, 1)));
    R3DM_HIP(c, B.ctr.ensure(16));
    R3DM_HIP(c, B.blk_cnt.ensure(8 * std::max<uint64_t>(NB, 1)));
    R3DM_HIP(c, B.blk_base.ensure(8 * std::max<uint64_t>(NB, 1)));
    R3DM_HIP(c, B.out.ensure(sizeof(r3dm_match) * std::max<uint64_t>(Q, 1)));
    R3DM_HIP(c, B.out_cnt.ensure(4 * NJ));
    R3DM_HIP(c, B.cand.ensure(64));
    if (B.pin_out.ensure(sizeof(r3dm_match) * std::max<uint64_t>(Q, 1)) != hipSuccess || B.pin_small.ensure(16 + 4 * NJ) != hipSuccess ||
        B.pin_blk.ensure(8 * std::max<uint64_t>(NB, 1)) != hipSuccess) {
        c->err = "guided matching: out of page-locked host memory"; return R3DM_ERR_NOMEM;
    }
    R3DM_HIP(c, hipMemcpyAsync(B.jobs.p, jobs.data(), NJ * sizeof(GuidedJob), hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipMemsetAsync(B.ctr.p, 0, 16, c->stream));
    R3DM_HIP(c, hipMemsetAsync(B.blk_cnt.p, 0, 8 * std::max<uint64_t>(NB, 1), c->stream));
    GuidedParams P{};
    P.imgs = c->d_imgs.as<ImgDev>(); P.jobs = B.jobs.as<GuidedJob>(); P.n_jobs = (uint32_t)NJ; P.n_blocks = (uint32_t)NB;
    P.b_lo = 0;
    P.res = B.res.as<uint32_t>(); P.q_cnt = B.q_cnt.as<uint32_t>(); P.q_off = B.q_off.as<unsigned long long>();
    P.blk_cnt = B.blk_cnt.as<unsigned long long>(); P.blk_base = B.blk_base.as<unsigned long long>();
    P.cand = B.cand.as<uint32_t>(); P.ctr = B.ctr.as<unsigned long long>(); P.out = B.out.as<r3dm_match>(); P.out_cnt = B.out_cnt.as<uint32_t>();
    unsigned long long* hc = B.pin_small.as<unsigned long long>();
    float ms1 = 0.f, ms2 = 0.f;
    R3DM_HIP(c, hipEventRecord(c->ev0, c->stream));
    R3DM_HIP(c, launch_guided_sweep(c->stream, P, 0));
    if (any_desc) {
        // the candidate lists are sized by the first pass (its counts per workgroup come back), then the workgroups are cut into
        // chunks whose lists fit the candidate budget and each chunk runs the second pass and the descriptor pass on one buffer.  A
        // workgroup is never split: one whose 256 queries alone exceed the budget is a chunk of its own (at most 256 x |J| entries).
        R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(B.pin_blk.p, B.blk_cnt.p, 8 * NB, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        R3DM_HIP(c, hipEventElapsedTime(&ms1, c->ev0, c->ev1));
        const uint64_t budget = (uint64_t)std::max(1, r3dm_dev_knob("R3DM_GUIDED_CAND_BUDGET", 1 << 28));     // candidates per chunk (1 GiB)
        unsigned long long* bc = B.pin_blk.as<unsigned long long>();
        std::vector<std::pair<uint32_t, uint32_t>> chunks;
        uint64_t run = 0, largest = 0;
        uint32_t lo = 0;
        for (uint32_t b = 0; b < (uint32_t)NB; ++b) {
            const uint64_t n = bc[b];
            if (run && run + n > budget) { chunks.push_back({lo, b}); largest = std::max(largest, run); lo = b; run = 0; }
            bc[b] = run;                                          // -> the workgroup's base inside its chunk
            run += n;
        }
        chunks.push_back({lo, (uint32_t)NB}); largest = std::max(largest, run);
        R3DM_HIP(c, hipMemcpyAsync(B.blk_base.p, B.pin_blk.p, 8 * NB, hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, B.cand.ensure(4 * (size_t)largest + 64));
        P.cand = B.cand.as<uint32_t>();
        R3DM_HIP(c, hipEventRecord(c->ev0, c->stream));
        for (const auto& ch : chunks) {
            GuidedParams Pc = P;
            Pc.b_lo = ch.first; Pc.n_blocks = ch.second - ch.first;
            R3DM_HIP(c, launch_guided_sweep(c->stream, Pc, 1));
            R3DM_HIP(c, launch_guided_desc(c->stream, Pc));
        }
        c->guided_stats.n_desc_chunks = chunks.size();
    }
    R3DM_HIP(c, launch_guided_compact(c->stream, P));
    R3DM_HIP(c, hipEventRecord(c->ev1, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(hc, B.ctr.p, 16, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(hc + 2, B.out_cnt.p, 4 * NJ, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(B.pin_out.p, B.out.p, sizeof(r3dm_match) * Q, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    R3DM_HIP(c, hipEventElapsedTime(&ms2, c->ev0, c->ev1));
    const uint32_t* oc = reinterpret_cast<const uint32_t*>(hc + 2);
    uint64_t n_matches = 0;
    for (size_t k = 0; k < NJ; ++k) { R.cnt[k] = oc[k]; n_matches += oc[k]; }
    R.host = B.pin_out.as<r3dm_match>();
    R.dev = B.out.as<r3dm_match>();
    r3dm_guided_stats& s = c->guided_stats;
    s.ms_kernels = (double)ms1 + (double)ms2;
    s.n_pairs = NJ; s.n_queries = Q; s.n_candidates = hc[0]; s.n_matches = n_matches;
    s.ms_wall = now_ms() - t0;
    return R3DM_OK;
}

static int r3dm_guided_match_impl(r3dm_ctx* c, const r3dm_graph* pairs, int kind, const double* models, const double* threshold_px, double ratio,
                                  r3dm_graph** out)
{
    const double t0 = now_ms();
    const uint64_t NP = pairs->pairs.size() / 2;
    std::vector<GuidedJob> jobs(NP);
    for (uint64_t p = 0; p < NP; ++p) {
        const uint32_t I = pairs->pairs[2 * p], J = pairs->pairs[2 * p + 1];
        auto a = c->slot_of.find(I), b = c->slot_of.find(J);
        if (a == c->slot_of.end() || b == c->slot_of.end()) { c->err = "r3dm_guided_match: pair references an unregistered view"; return R3DM_ERR_INVALID; }
        const int rc = guided_job_make(c, a->second, b->second, kind, models + 9 * p, threshold_px[p], ratio, jobs[p]);
        if (rc != R3DM_OK) return rc;
    }
    GuidedResult R;
    int rc = guided_run(c, jobs, R);
    if (rc != R3DM_OK) return rc;
    auto g = std::unique_ptr<r3dm_graph>(new r3dm_graph());
    g->offsets.push_back(0);
    GraphBuilder b(c, g.get(), c->device_graphs, R.host, nullptr, R.dev, nullptr);
    for (uint64_t p = 0; p < NP; ++p) {
        const uint32_t n = R.cnt[p];
        if (n == 0) continue;                                  // no empty entries ("Guided matching")
        b.add(pairs->pairs[2 * p], pairs->pairs[2 * p + 1], jobs[p].q0, 0, n);
    }
    b.done();
    c->guided_stats.ms_wall = now_ms() - t0;
    *out = g.release();
    return R3DM_OK;
}

extern "C" int r3dm_guided_match(r3dm_ctx* c, const r3dm_graph* pairs, int kind, const double* models, const double* threshold_px, double ratio,
                                 r3dm_graph** out)
{
    if (!c || !pairs || !out || kind < R3DM_GUIDED_F || kind > R3DM_GUIDED_H) return R3DM_ERR_INVALID;
    *out = nullptr;
    if (pairs->pairs.size() && (!models || !threshold_px)) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int { return r3dm_guided_match_impl(c, pairs, kind, models, threshold_px, ratio, out); });
}

extern "C" int r3dm_set_guided_matching(r3dm_ctx* c, int enable, double ratio_F, double ratio_E, double ratio_H)
{
    if (!c) return R3DM_ERR_INVALID;
    if (std::isnan(ratio_F) || std::isnan(ratio_E) || std::isnan(ratio_H)) { c->err = "r3dm_set_guided_matching: NaN ratio"; return R3DM_ERR_INVALID; }
    c->guided_on = enable != 0;
    c->guided_ratio[R3DM_GUIDED_F] = ratio_F; c->guided_ratio[R3DM_GUIDED_E] = ratio_E; c->guided_ratio[R3DM_GUIDED_H] = ratio_H;
    return R3DM_OK;
}

extern "C" int r3dm_guided_report(const r3dm_ctx* c, r3dm_guided_stats* out)
{
    if (!c || !out) return R3DM_ERR_INVALID;
    *out = c->guided_stats;
    return R3DM_OK;
}
