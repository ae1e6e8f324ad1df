// api_filter.cpp -- part of the host side of libr3dm.so: the C ABI declared in include/r3dm.h (see r3dm_ctx.hpp for the file map).
//
// Mirrors, for the compute-matches hot path only, what the reference does in
// /root/reference/src/R3DComputeMatches.cpp:2035-2129 and src/Regard3DFeatures.cpp -- with every arithmetic stage running as
// HIP kernels on one MI355X.  There is no CPU fallback in this file: when HIP fails, the call fails.
#include "r3dm_ctx.hpp"

#include <memory>

// ------------------------------------------------------------------------------------------------
// geometric filter
// ------------------------------------------------------------------------------------------------
// The filter kinds, in r3dm_filter_FEH's order (`slot`: its `which` bit and its ms_kernels3 / ms_wall3 entry).  model_kind numbers the
// kernels' parameter blocks, the context's buffer sets (c->fb) and the cooperative kernel's start order: 0 F, 1 H, 2 E.
struct FilterKind {
    int model_kind, slot;
    int guided;                  // R3DM_GUIDED_*
    uint32_t SS;                 // Kernel::MINIMUM_SAMPLES
    double coop_work;            // cooperative start order: work per putative ~ models per iteration (E ~4.5, F ~2.6, H ~1) + E's solves
    int prio;                    // stream priority class in a call of several kinds: 2 high, 1 normal, 0 low
    const char* name;
};
static const FilterKind kKinds[3] = {
    {0, 0, R3DM_GUIDED_F, 7, 2.6, 1, "F"},      // fundamental matrix (GeometricFilter_FMatrix_AC)
    {2, 1, R3DM_GUIDED_E, 5, 6.0, 2, "E"},      // essential matrix (GeometricFilter_EMatrix_AC) + Regard3D's overlap rule
    {1, 2, R3DM_GUIDED_H, 4, 1.0, 0, "H"},      // homography (GeometricFilter_HMatrix_AC)
};

// GeometricFilter_{F,H,E}Matrix_AC: a pair is accepted iff #inliers > 2.5 * MINIMUM_SAMPLES
static bool below_acceptance(uint32_t n, uint32_t SS) { return (double)n <= 2.5 * SS; }
// the reference's extra check after the E filter (src/R3DComputeMatches.cpp:2175-2192): n of the pair's m putatives survive
static bool poor_overlap(uint32_t n, uint64_t m, uint32_t min_count, float min_ratio) { return n < min_count || (float)n / (float)m < min_ratio; }

// the developer knobs that shape a call's plan (read by the caller; each is its default in the product build)
struct FilterKnobs {
    uint32_t coop_min;           // R3DM_FILTER_COOP_MIN: pairs with more putatives run on the cooperative kernel; 0 = never
    uint32_t coop_g;             // R3DM_FILTER_COOP_G: > 0: this many slices for every such pair
    int wide;                    // R3DM_FILTER_WIDE: >= 0 forces the 512-thread variant on (1) or off (0)
    int lpt;                     // R3DM_FILTER_LPT: start the long pairs first
};

// What a filter call runs, decided from the putative graph and the views alone (plan_filter makes no HIP call)
struct FilterPlan {
    // work items: pairs with more than SS putatives (ACRANSAC returns nothing for n <= MINIMUM_SAMPLES)
    std::vector<uint32_t> item_pair;           // putative pair of every item
    std::vector<uint2> slots, ids;             // its views' slots and ids
    std::vector<uint64_t> begin_end;           // [begin, end) of its putative list inside the full match array
    std::vector<uint64_t> soff;                // slice offsets of the per-item work arrays: multiples of 32 elements, room for m + 1
    uint32_t max_m = 0, max_m_short = 0;       // longest list of all items / of the items on the one-workgroup kernel
    // long pairs on the cooperative kernel (kernels_filter_coop.hip), by cooperative index: item, slices, slice length, first
    // histogram slot, putative count
    std::vector<unsigned char> is_coop;
    std::vector<uint32_t> coop_items, coop_G, coop_slice, coop_hoff, coop_len;
    uint32_t coop_slots = 0;                   // sum of G
    uint32_t m_cap = 0, wide = 0;              // LDS sort capacity; 512-thread variant of the one-workgroup kernel
    bool spill = false;                        // sort lists in global memory: per-item offsets into a buffer of spill_total entries
    std::vector<uint64_t> spill_off;
    uint64_t spill_total = 0;
    bool ordered = false;                      // launch order of the one-workgroup kernel's items
    std::vector<uint32_t> order;
    uint32_t n_items() const { return (uint32_t)item_pair.size(); }
    uint64_t len(uint32_t k) const { return begin_end[2 * k + 1] - begin_end[2 * k]; }
};

static int plan_filter(const r3dm_graph& putative, const r3dm_ctx& c, const FilterKind& kind, const FilterKnobs& kn, FilterPlan& P,
                       std::string& err)
{
    const uint64_t NP = putative.pairs.size() / 2;
    for (uint64_t p = 0; p < NP; ++p) {
        const uint64_t m = putative.offsets[p + 1] - putative.offsets[p];
        if (m <= kind.SS) continue;
        const uint32_t I = putative.pairs[2 * p], J = putative.pairs[2 * p + 1];
        auto a = c.slot_of.find(I), b = c.slot_of.find(J);
        if (a == c.slot_of.end() || b == c.slot_of.end()) { err = "filter: pair references an unregistered view"; return R3DM_ERR_INVALID; }
        const HostImage& A = *c.imgs[a->second];
        const HostImage& B = *c.imgs[b->second];
        if (!A.has_xy || !B.has_xy) { err = "filter: view registered without feature positions"; return R3DM_ERR_INVALID; }
        // ACKernelAdaptor normalises with 1 / sqrt(w h) and the NFA scale is D / A of image J: a view registered with a zero
        // width or height would turn every residual into NaN and the filter into a silent "no inliers"
        if (A.width == 0 || A.height == 0 || B.width == 0 || B.height == 0) {
            err = "filter: view " + std::to_string(A.width == 0 || A.height == 0 ? I : J) + " was registered without its image size (width / height = 0)";
            return R3DM_ERR_INVALID;
        }
        if (m > (1u << 22)) { err = "filter: more than 4M putative matches in one pair"; return R3DM_ERR_UNSUPPORTED; }
        // E_ACRobust: a pair whose views lack valid pinhole intrinsics is not estimated (and so not kept)
        if (kind.model_kind == 2 && (!A.has_K || !B.has_K)) continue;
        P.item_pair.push_back((uint32_t)p);
        P.slots.push_back(make_uint2(a->second, b->second));
        P.ids.push_back(make_uint2(I, J));
        P.begin_end.push_back(putative.offsets[p]);
        P.begin_end.push_back(putative.offsets[p + 1]);
        P.max_m = std::max<uint32_t>(P.max_m, (uint32_t)m);
    }
    const uint32_t NI = P.n_items();
    if (NI == 0) return R3DM_OK;
    // ---- long pairs run on the cooperative kernel (kernels_filter_coop.hip): G workgroups per batch of models, slices of the match list.
    // G follows the pair-length distribution: slices of 2048 .. 8192 matches, short enough that the long pairs of the call fill the
    // device about one and a half times over; collections of short pairs (C2: every pair below the threshold) keep the one-workgroup
    // kernel and its launch shape untouched.
    P.is_coop.assign(NI, 0);
    uint64_t sum_long = 0;
    for (uint32_t k = 0; k < NI; ++k) {
        const uint64_t mk = P.len(k);
        if (kn.coop_min && mk > kn.coop_min && mk <= (uint64_t)kCoopMaxG * 65472u) { P.is_coop[k] = 1; sum_long += mk; }
        else P.max_m_short = std::max<uint32_t>(P.max_m_short, (uint32_t)mk);
    }
    const uint64_t fill = std::max<uint64_t>(1, (uint64_t)std::max(c.n_cu, 1) * 3 / 2);
    const uint32_t slice_target = (uint32_t)std::min<uint64_t>(8192, std::max<uint64_t>(2048, ((sum_long / fill + 511) / 512) * 512));
    for (uint32_t k = 0; k < NI; ++k) {
        if (!P.is_coop[k]) continue;
        const uint32_t mk = (uint32_t)P.len(k);
        uint32_t G = kn.coop_g ? kn.coop_g : (mk + slice_target - 1) / slice_target;
        G = std::max<uint32_t>(G, (mk + 65471u) / 65472u);                              // a slice counts in 16 bits
        G = std::min<uint32_t>(std::max<uint32_t>(G, 1u), kCoopMaxG);
        const uint32_t len = (((mk + G - 1) / G + 63) / 64) * 64;
        P.coop_items.push_back(k); P.coop_G.push_back(G); P.coop_slice.push_back(len); P.coop_hoff.push_back(P.coop_slots); P.coop_len.push_back(mk);
        P.coop_slots += G;
    }
    P.soff.assign(NI + 1, 0);
    for (uint32_t k = 0; k < NI; ++k) P.soff[k + 1] = P.soff[k] + ((P.len(k) + 1 + 31) / 32) * 32;
    const uint64_t n_slice = P.soff[NI];
    // the cooperative kernel addresses the points and the slice histograms through 32-bit buffer offsets: a call beyond them (about 67 M
    // putatives) runs every pair on the one-workgroup kernel, as every call did before the cooperative kernel existed
    if (!P.coop_items.empty() && (32 * (uint64_t)n_slice >= 0x7FFFFFFFull || 4 * (uint64_t)P.coop_slots * kCoopB * 512 + 256 >= 0x7FFFFFFFull)) {
        for (uint32_t k = 0; k < NI; ++k) {
            P.is_coop[k] = 0;
            P.max_m_short = std::max<uint32_t>(P.max_m_short, (uint32_t)P.len(k));
        }
        P.coop_items.clear(); P.coop_G.clear(); P.coop_slice.clear(); P.coop_hoff.clear(); P.coop_len.clear();
        P.coop_slots = 0;
    }
    const bool coop = !P.coop_items.empty();
    // LDS sort capacity: 8192 (x 12 B) fits beside the hypothesis buffer; pairs with more putatives sort in global scratch
    // (essential matrix: 4096, so that header + 16 hypotheses + sort buffers stay below 80 KB and two workgroups share a CU)
    // collections with long match lists (some pair above 4096 putatives: LDS admits one workgroup per CU anyway) run the 512-thread
    // variant of the kernel -- the same results, every pass over a pair's matches in half the trips
    P.wide = kn.wide >= 0 ? (uint32_t)(kn.wide != 0) : (P.max_m_short > 4096 ? 1u : 0u);
    P.m_cap = std::min<uint32_t>((kind.model_kind == 2 && !P.wide) ? 4096 : 8192, std::max<uint32_t>(64, next_pow2(std::max(P.max_m_short, 1u))));
    P.spill = P.max_m_short > P.m_cap || coop;          // (the cooperative kernel keeps every pair's sort lists in global memory)
    if (P.spill) {
        P.spill_off.assign(NI, 0);
        for (uint32_t k = 0; k < NI; ++k) {
            const uint64_t mk = P.len(k);
            P.spill_off[k] = P.spill_total;
            if (P.is_coop[k]) P.spill_total += 2 * (uint64_t)next_pow2((uint32_t)mk);      // [sort | spare]: the bucket pass of the cooperative kernel's full evaluation
            else if (mk > P.m_cap) P.spill_total += next_pow2((uint32_t)mk);
        }
    }
    // launch order: the workgroup of a pair runs for a time roughly proportional to its putative count, and a C2 call has
    // ~1.5 x as many pairs as resident workgroups -- start the long ones first so the tail of the launch is short ones
    P.ordered = (kn.lpt && NI > 1) || coop;
    if (P.ordered) {
        P.order.reserve(NI);
        for (uint32_t k = 0; k < NI; ++k) if (!P.is_coop[k]) P.order.push_back(k);
        if (kn.lpt) std::stable_sort(P.order.begin(), P.order.end(), [&](uint32_t a, uint32_t b) { return P.len(a) > P.len(b); });
    }
    return R3DM_OK;
}

// the arguments of a filter entry (min_count / min_ratio: E's overlap rule)
struct FilterArgs {
    const r3dm_graph* putative; double max_residual_px; uint32_t max_iter; uint64_t seed; r3dm_ferror err_kind; uint32_t min_count; float min_ratio;
};

#define FHIP(call)                                                                     \
    do {                                                                               \
        hipError_t e__ = (call);                                                       \
        if (e__ != hipSuccess) {                                                       \
            err = std::string(#call) + ": " + hipGetErrorString(e__);                  \
            return R3DM_ERR_HIP;                                                       \
        }                                                                              \
    } while (0)

struct FilterCall;

// The developer build's diagnostics of a filter call (the product build resolves every knob below to "off" at compile time): the
// invariant checks (R3DM_FILTER_CHECK=1), the per-model trace of one pair (R3DM_TRACE_PAIR="I,J" + R3DM_TRACE_FILE=path), the phase
// profile of the cooperative kernel (R3DM_COOP_PROF=1, read by tools/coop_prof_summary.py) and r3dm_filter_FEH's timing line
// (R3DM_FILTER_TIMING=1).  Armed by FilterCall::upload, reported by FilterCall::collect.
struct FilterDiag {
    static constexpr uint32_t kTraceCap = 16384;
    DevBuf check, trace;
    const char* trace_file = nullptr;
    ~FilterDiag() { check.release(); trace.release(); }
    int arm(r3dm_ctx* c, FilterCall& k, std::string& err);
    int report(r3dm_ctx* c, const FilterCall& k, std::string& err);
    static void timing(double t0, double t_prep, double t_launch, float ms_kernels)
    {
        if (r3dm_dev_knob("R3DM_FILTER_TIMING", 0))
            fprintf(stderr, "r3dm_filter_FEH: prepare %.2f ms, launch + wait %.2f ms (kernels %.2f), collect %.2f ms\n", t_prep - t0, t_launch - t_prep,
                    ms_kernels, now_ms() - t_launch);
    }
};

// One filter kind of a call from plan to graph: prepare (plan + upload: tables, uploads on the context's stream, kernel parameters),
// then -- once filter_launch has run and waited for the kernels -- collect (copy back, per-pair report, acceptance rules, the graph) and,
// with guided matching on, finish (the graph from the guided lists).  Written by the call's own thread (the kinds of r3dm_filter_FEH are
// collected side by side); the entries fold what it leaves into the context.
struct FilterCall {
    r3dm_ctx* const c;
    const FilterKind& kind;
    const FilterArgs a;
    r3dm_graph** const out;
    double* const M_out;                       // optional: the models of the kept pairs
    FilterPlan plan;
    FilterParams fp{};
    FilterDiag diag;
    std::unique_ptr<r3dm_graph> g;             // the graph under construction, handed to *out by collect or finish
    std::string err;
    double t_call = 0.0, ms_kernels = 0.0, ms_wall = 0.0;
    bool collected = false;                    // collect succeeded
    std::vector<r3dm_pair_report> report;
    std::vector<double> h_F;                   // the model of every item
    // guided matching on (r3dm_set_guided_matching): the accepted items, whose lists job k of the call replaces (job first + k of
    // the call's one guided launch)
    std::vector<uint32_t> acc;
    std::vector<GuidedJob> gjobs;

    FilterCall(r3dm_ctx* c_, const FilterKind& kind_, const FilterArgs& a_, r3dm_graph** out_, double* M_out_)
        : c(c_), kind(kind_), a(a_), out(out_), M_out(M_out_) { fp.model_kind = kind.model_kind; }
    int prepare(const r3dm_match* dev_matches);
    int upload(const r3dm_match* dev_matches);
    int collect(float ms);
    void finish(const GuidedResult& R, size_t first);
    void deliver() { ms_wall = now_ms() - t_call; *out = g.release(); }
};

// dev_matches: the putative matches another kind of the call has already uploaded
int FilterCall::prepare(const r3dm_match* dev_matches)
{
    if (!a.putative || !out || a.max_iter == 0) return R3DM_ERR_INVALID;
    *out = nullptr;
    FHIP(hipSetDevice(c->device));
    t_call = now_ms();
    static const int lpt = r3dm_dev_knob("R3DM_FILTER_LPT", 1);
    const FilterKnobs kn{(uint32_t)r3dm_dev_knob("R3DM_FILTER_COOP_MIN", 4096), (uint32_t)r3dm_dev_knob("R3DM_FILTER_COOP_G", 0),
                         r3dm_dev_knob("R3DM_FILTER_WIDE", -1), lpt};
    const int rc = plan_filter(*a.putative, *c, kind, kn, plan, err);
    if (rc != R3DM_OK) return rc;
    g.reset(new r3dm_graph());
    g->offsets.push_back(0);
    if (plan.n_items() == 0) return R3DM_OK;         // nothing to launch: collect delivers the empty graph
    if (kind.model_kind == 0 && a.err_kind != R3DM_ERR_SYMMETRIC_EPIPOLAR) { err = "filter: only the symmetric epipolar error is implemented"; return R3DM_ERR_UNSUPPORTED; }
    return upload(dev_matches);
}

int FilterCall::upload(const r3dm_match* dev_matches)
{
    FilterBufs& B = c->fb[kind.model_kind];
    const FilterPlan& P = plan;
    const uint32_t NI = P.n_items(), max_m = P.max_m, n_coop = (uint32_t)P.coop_items.size();
    const uint64_t n_slice = P.soff[NI];
    // host tables in the reference's own float arithmetic (glibc log10f), see acransac_body (filter_acransac.inc)
    std::vector<float> l10(max_m + 2), lck(max_m + 2);
    for (uint32_t k = 0; k <= max_m + 1; ++k) l10[k] = std::log10((float)k);
    for (uint32_t n = 0; n <= max_m + 1; ++n) {
        const uint32_t ks = kind.SS;
        if (ks >= n) { lck[n] = 0.f; continue; }
        const uint32_t kk = (n - ks < ks) ? n - ks : ks;
        float r = 0.f;
        for (uint32_t i = 1; i <= kk; ++i) r += l10[n - i + 1] - l10[i];
        lck[n] = r;
    }
    const uint64_t n_match_total = a.putative->matches.size();
    FHIP(B.f_pairs.ensure(sizeof(uint2) * NI));
    FHIP(B.f_ids.ensure(sizeof(uint2) * NI));
    FHIP(B.f_offs.ensure(sizeof(uint64_t) * 2 * NI));
    if (!dev_matches) FHIP(B.f_matches.ensure(sizeof(r3dm_match) * std::max<uint64_t>(n_match_total, 1)));
    FHIP(B.f_inl_cnt.ensure(4 * (size_t)NI));
    FHIP(B.f_inl_idx.ensure(4 * (size_t)n_slice + 64));
    FHIP(B.f_soff.ensure(8 * (size_t)(NI + 1)));
    FHIP(hipMemcpyAsync(B.f_soff.p, P.soff.data(), 8 * (size_t)(NI + 1), hipMemcpyHostToDevice, c->stream));
    FHIP(B.f_F.ensure(72 * (size_t)NI));
    FHIP(B.f_thr.ensure(16 * (size_t)NI));
    FHIP(B.f_iters.ensure(8 * (size_t)NI));
    FHIP(B.f_log10.ensure(4 * l10.size()));
    FHIP(B.f_logck.ensure(4 * lck.size()));
    FHIP(hipMemcpyAsync(B.f_pairs.p, P.slots.data(), sizeof(uint2) * NI, hipMemcpyHostToDevice, c->stream));
    FHIP(hipMemcpyAsync(B.f_ids.p, P.ids.data(), sizeof(uint2) * NI, hipMemcpyHostToDevice, c->stream));
    FHIP(hipMemcpyAsync(B.f_offs.p, P.begin_end.data(), sizeof(uint64_t) * 2 * NI, hipMemcpyHostToDevice, c->stream));
    if (!dev_matches) FHIP(hipMemcpyAsync(B.f_matches.p, a.putative->matches.data(), sizeof(r3dm_match) * n_match_total, hipMemcpyHostToDevice, c->stream));
    FHIP(hipMemcpyAsync(B.f_log10.p, l10.data(), 4 * l10.size(), hipMemcpyHostToDevice, c->stream));
    FHIP(hipMemcpyAsync(B.f_logck.p, lck.data(), 4 * lck.size(), hipMemcpyHostToDevice, c->stream));
    FHIP(hipMemsetAsync(B.f_inl_cnt.p, 0, 4 * (size_t)NI, c->stream));

    fp.imgs = c->d_imgs.as<ImgDev>();
    fp.pairs = B.f_pairs.as<uint2>(); fp.pair_ids = B.f_ids.as<uint2>();
    fp.offsets = B.f_offs.as<uint64_t>(); fp.matches = dev_matches ? dev_matches : B.f_matches.as<r3dm_match>();
    fp.wide = P.wide;
    fp.n_items = NI; fp.m_cap = P.m_cap;
    fp.spill_keys = nullptr; fp.spill_idx = nullptr; fp.spill_off = nullptr;
    if (P.spill) {
        const uint64_t tot = P.spill_total;
        FHIP(B.f_spill.ensure(tot * 12 + NI * 8 + 64));
        unsigned char* base = B.f_spill.as<unsigned char>();
        FHIP(hipMemcpyAsync(base + tot * 12, P.spill_off.data(), NI * 8, hipMemcpyHostToDevice, c->stream));
        fp.spill_keys = reinterpret_cast<unsigned long long*>(base);
        fp.spill_idx = reinterpret_cast<uint32_t*>(base + tot * 8);
        fp.spill_off = reinterpret_cast<const uint64_t*>(base + tot * 12);
    }
    fp.precision_px = a.max_residual_px; fp.max_iter = a.max_iter; fp.seed = a.seed; fp.err_kind = (int)a.err_kind;
    fp.kinv = nullptr;
    std::vector<double> kinv;
    if (kind.model_kind == 2) {
        kinv.assign(9 * c->imgs.size(), 0.0);
        for (size_t s = 0; s < c->imgs.size(); ++s)
            if (c->imgs[s] && c->imgs[s]->has_K) memcpy(&kinv[9 * s], c->imgs[s]->Kinv, 72);
        FHIP(B.f_kinv.ensure(kinv.size() * 8));
        FHIP(hipMemcpyAsync(B.f_kinv.p, kinv.data(), kinv.size() * 8, hipMemcpyHostToDevice, c->stream));
        fp.kinv = B.f_kinv.as<double>();
    }
    fp.log10_tab = B.f_log10.as<float>(); fp.logc_k = B.f_logck.as<float>();
    fp.inl_count = B.f_inl_cnt.as<uint32_t>(); fp.inl_idx = B.f_inl_idx.as<uint32_t>();
    fp.F_out = B.f_F.as<double>(); fp.thr_nfa = B.f_thr.as<double>(); fp.iters = B.f_iters.as<uint32_t>();
    FHIP(B.f_scratch.ensure(40 * (size_t)n_slice + 256));
    fp.pts_scratch = B.f_scratch.as<double>();
    fp.pool_scratch = reinterpret_cast<uint32_t*>(B.f_scratch.as<unsigned char>() + 32 * (size_t)n_slice);
    fp.scratch_logc = reinterpret_cast<float*>(B.f_scratch.as<unsigned char>() + 36 * (size_t)n_slice);
    fp.soff = B.f_soff.as<uint64_t>();
    FHIP(B.f_la.ensure((size_t)NI * 1024 * 8 + 64));
    fp.la_tab = B.f_la.as<double>();
    { const int sc = r3dm_dev_knob("R3DM_FILTER_SCOUT", 1); fp.scout = (uint32_t)(sc < 0 ? 0 : sc > 5 ? 1 : sc) | ((uint32_t)r3dm_dev_knob("R3DM_FILTER_SCOUT_SUB", 0) << 8); }   // (developer build: 0 = every model through the full evaluation, 2 = the scout divides exactly, 3 = check mode with R3DM_FILTER_CHECK=1; A/B and parity)
    fp.order = nullptr;
    fp.n_short = NI - n_coop;
    if (P.ordered) {
        FHIP(B.f_order.ensure(4 * (size_t)NI));
        if (!P.order.empty()) FHIP(hipMemcpyAsync(B.f_order.p, P.order.data(), 4 * P.order.size(), hipMemcpyHostToDevice, c->stream));
        fp.order = B.f_order.as<uint32_t>();
    }
    fp.n_coop = n_coop;
    fp.coop_workers = 0;
    std::vector<uint32_t> stage;
    if (n_coop) {
        // one allocation: [items | G | slice | hoff] [published records] [models] [batch matrices] [slice counts]
        // [slope tables] [T*] [slice histograms]
        auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        const size_t small_bytes = up(16 * (size_t)n_coop);
        const size_t o_pub = small_bytes, pub_bytes = up(64 * (size_t)n_coop);
        const size_t o_models = o_pub + pub_bytes, models_bytes = up(8 * (size_t)n_coop * filter_coop_model_doubles(kind.model_kind));
        const size_t o_bm = o_models + models_bytes, bm_bytes = up(8 * (size_t)n_coop * kCoopB * 9);
        const size_t o_cnt = o_bm + bm_bytes, cnt_bytes = up(4 * (size_t)P.coop_slots * kCoopB);
        const size_t o_la = o_cnt + cnt_bytes, la_bytes = up(8 * (size_t)n_coop * 1024);
        const size_t o_ts = o_la + la_bytes, ts_bytes = up(8 * (size_t)n_slice + 64);
        const size_t o_hist = o_ts + ts_bytes, hist_bytes = up(4 * (size_t)P.coop_slots * kCoopB * 512);
        // (the kernel addresses the points and the slice histograms through 32-bit buffer offsets: checked by plan_filter, kept as a guard)
        if (32 * (uint64_t)n_slice >= 0x7FFFFFFFull || hist_bytes >= 0x7FFFFFFFull) { err = "filter: putative graph too large for the cooperative kernel's buffer offsets"; return R3DM_ERR_UNSUPPORTED; }
        FHIP(B.f_coop.ensure(o_hist + hist_bytes));
        unsigned char* base = B.f_coop.as<unsigned char>();
        stage.assign(small_bytes / 4, 0u);
        memcpy(&stage[0], P.coop_items.data(), 4 * (size_t)n_coop);
        memcpy(&stage[n_coop], P.coop_G.data(), 4 * (size_t)n_coop);
        memcpy(&stage[2 * (size_t)n_coop], P.coop_slice.data(), 4 * (size_t)n_coop);
        memcpy(&stage[3 * (size_t)n_coop], P.coop_hoff.data(), 4 * (size_t)n_coop);
        FHIP(hipMemcpyAsync(base, stage.data(), 4 * stage.size(), hipMemcpyHostToDevice, c->stream));
        FHIP(hipMemsetAsync(base + o_pub, 0, pub_bytes, c->stream));
        // logcombi(k, m) of every cooperative pair as a running prefix in the reference's float accumulation order (makelogcombi_n,
        // SURVEY.md A.5): pre[i] = pre[i-1] + (l10[m-i+1] - l10[i]), mirrored for k > m/2 -- the same operations, in the same order, as
        // thread 0 of the one-workgroup kernel performs (this translation unit is compiled with -ffp-contract=off like the kernels)
        if (B.pin_idx.ensure(4 * (size_t)n_slice + 64) != hipSuccess) { err = "filter: out of page-locked host memory"; return R3DM_ERR_NOMEM; }
        float* lc = static_cast<float*>(B.pin_idx.p);
        for (uint32_t qi = 0; qi < n_coop; ++qi) {
            const uint32_t m = P.coop_len[qi];
            float* t = lc + P.soff[P.coop_items[qi]];
            float pre = 0.0f;
            t[0] = 0.0f; t[m] = 0.0f;
            for (uint32_t i = 1; i <= m / 2; ++i) {
                pre = pre + (l10[m - i + 1] - l10[i]);
                t[i] = pre;
                if (m - i > i) t[m - i] = pre;
            }
        }
        // (one copy of the whole table array: the slices of the short pairs carry whatever the buffer held -- the one-workgroup
        // kernel fills its own tables before it reads them; the landing buffer is reused for the results)
        FHIP(hipMemcpyAsync(fp.scratch_logc, lc, 4 * (size_t)n_slice, hipMemcpyHostToDevice, c->stream));
        fp.coop_items = reinterpret_cast<const uint32_t*>(base);
        fp.coop_G = fp.coop_items + n_coop; fp.coop_slice = fp.coop_items + 2 * (size_t)n_coop; fp.coop_hoff = fp.coop_items + 3 * (size_t)n_coop;
        fp.coop_q = nullptr;                              // (the scheduling words are shared by the kinds of a call: filter_launch)
        fp.coop_pub = base + o_pub;
        fp.coop_models = reinterpret_cast<double*>(base + o_models);
        fp.coop_bm = reinterpret_cast<double*>(base + o_bm);
        fp.coop_cnt = reinterpret_cast<uint32_t*>(base + o_cnt);
        fp.coop_la = reinterpret_cast<double*>(base + o_la);
        fp.coop_tstar = reinterpret_cast<double*>(base + o_ts);
        fp.coop_hist = reinterpret_cast<uint32_t*>(base + o_hist);
        fp.coop_prof = nullptr;
        if (filter_coop_lds_bytes() > 160 * 1024) { err = "filter: LDS budget exceeded (cooperative kernel)"; return R3DM_ERR_UNSUPPORTED; }
    }
    if (filter_F_lds_bytes(fp.m_cap, kind.model_kind) > 160 * 1024) { err = "filter: LDS budget exceeded"; return R3DM_ERR_UNSUPPORTED; }
    const int rc = diag.arm(c, *this, err);
    if (rc != R3DM_OK) return rc;
    // the host vectors above (the plan's, l10, lck, kinv, stage) were handed to asynchronous copies on the context's stream: they must
    // not leave scope before the copies have read them
    FHIP(hipStreamSynchronize(c->stream));
    return R3DM_OK;
}

int FilterDiag::arm(r3dm_ctx* c, FilterCall& k, std::string& err)
{
    FilterParams& fp = k.fp;
    if (r3dm_dev_knob("R3DM_COOP_PROF", 0) && fp.n_coop) {       // per-pair phase times of the cooperative kernel
        DevBuf& prof = c->fb[k.kind.model_kind].f_coop_prof;
        FHIP(prof.ensure(128 * (size_t)fp.n_coop));
        FHIP(hipMemsetAsync(prof.p, 0, 128 * (size_t)fp.n_coop, c->stream));
        fp.coop_prof = prof.as<unsigned long long>();
    }
    const char* tp = r3dm_dev_str("R3DM_TRACE_PAIR");
    trace_file = r3dm_dev_str("R3DM_TRACE_FILE");
    fp.trace = nullptr; fp.trace_item = 0xFFFFFFFFu; fp.trace_cap = kTraceCap; fp.trace_rows = nullptr;
    fp.trace_iter = (uint32_t)r3dm_dev_knob("R3DM_TRACE_ITER", -1);
    if (tp && trace_file) {
        unsigned tI = 0, tJ = 0;
        if (sscanf(tp, "%u,%u", &tI, &tJ) == 2)
            for (uint32_t q = 0; q < fp.n_items; ++q)
                if (k.plan.ids[q].x == tI && k.plan.ids[q].y == tJ) fp.trace_item = q;
        if (fp.trace_item != 0xFFFFFFFFu) {
            FHIP(trace.ensure(40 * (size_t)kTraceCap + 64));
            FHIP(hipMemsetAsync(trace.p, 0, 40 * (size_t)kTraceCap + 64, c->stream));
            fp.trace = trace.as<double>() + 8;
            fp.trace_rows = trace.as<uint32_t>();
        }
    }
    fp.dbg = nullptr;
    if (r3dm_dev_knob("R3DM_FILTER_CHECK", 0)) {
        FHIP(check.ensure(64));
        FHIP(hipMemsetAsync(check.p, 0, 64, c->stream));
        fp.dbg = check.as<uint32_t>();
    }
    return R3DM_OK;
}

int FilterDiag::report(r3dm_ctx* c, const FilterCall& k, std::string& err)
{
    const FilterParams& fp = k.fp;
    if (fp.dbg) {
        uint32_t d[4] = {0, 0, 0, 0};
        hipError_t e = hipMemcpyAsync(d, fp.dbg, 16, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);       // the kernel runs on c->stream (non-blocking): wait for it
        if (e != hipSuccess || d[0]) {
            err = e != hipSuccess ? std::string("filter check: ") + hipGetErrorString(e)
                : "filter invariant " + std::to_string(d[0]) + " violated at item " + std::to_string(d[1]) + " (" + std::to_string(d[2]) + ", " + std::to_string(d[3]) + ")";
            if (e == hipSuccess && (d[0] == 10u || d[0] == 11u)) {     // (the scout's bound, and the NFA / the full evaluation's bound it exceeds, as float bits)
                float fa, fb; memcpy(&fa, &d[2], 4); memcpy(&fb, &d[3], 4);
                char b[96]; snprintf(b, sizeof b, " = (%.7g, %.7g)", (double)fa, (double)fb); err += b;
            }
            return R3DM_ERR_HIP;
        }
    }
    if (fp.n_coop && fp.coop_prof) {
        std::vector<unsigned long long> pr(16 * (size_t)fp.n_coop);
        FHIP(hipMemcpy(pr.data(), fp.coop_prof, 8 * pr.size(), hipMemcpyDeviceToHost));
        for (uint32_t q = 0; q < fp.n_coop; ++q) {
            const unsigned long long* r = &pr[16 * (size_t)q];
            fprintf(stderr, "coop %s pair %u m %llu G %u: wall %.0f us | init %.0f solve %.0f form+publish %.0f slices %.0f (sum over workgroups) arrive %.0f bounds %.0f "
                    "full %.0f (%llu) walk %.0f | batches %llu models %llu | task delay sum %.0f max %.0f, longest slice %.0f %u\n", k.kind.name, q,
                    (unsigned long long)k.plan.coop_len[q], k.plan.coop_G[q], r[10] / 100.0, r[0] / 100.0, r[1] / 100.0, r[2] / 100.0, r[3] / 100.0,
                    r[4] / 100.0, r[5] / 100.0, r[6] / 100.0, r[7], r[8] / 100.0, r[9], r[11], r[12] / 100.0, r[14] / 100.0, r[13] / 100.0, 0u);
        }
    }
    if (fp.trace) {
        std::vector<double> tr(5 * (size_t)kTraceCap + 8);
        FHIP(hipMemcpy(tr.data(), trace.p, tr.size() * 8, hipMemcpyDeviceToHost));
        const uint32_t rows = std::min<uint32_t>(*reinterpret_cast<uint32_t*>(tr.data()), kTraceCap);
        if (FILE* f = fopen(trace_file, "w")) {
            for (uint32_t r = 0; r < rows; ++r)
                fprintf(f, "%.0f %.0f %.0f %.17g %.0f\n", tr[8 + 5 * r], tr[9 + 5 * r], tr[10 + 5 * r], tr[11 + 5 * r], tr[12 + 5 * r]);
            if (fp.trace_iter != 0xFFFFFFFFu) {
                fprintf(f, "# sample");
                for (int q = 0; q < 20; ++q) fprintf(f, " %.0f", tr[8 + 5 * (size_t)(kTraceCap - 4) + q]);
                fprintf(f, "\n");
            }
            fclose(f);
        }
    }
    return R3DM_OK;
}

// ms: the HIP-event time filter_launch gave the call's kernels
int FilterCall::collect(float ms)
{
    const uint32_t NI = plan.n_items();
    if (NI == 0) { deliver(); return R3DM_OK; }
    const int drc = diag.report(c, *this, err);
    if (drc != R3DM_OK) return drc;
    FilterBufs& B = c->fb[kind.model_kind];
    const uint64_t n_slice = plan.soff[NI];
    std::vector<uint32_t> h_cnt(NI);
    // (inlier indices through the kind's page-locked landing buffer: pageable destinations are pinned on the way by the runtime)
    if (B.pin_idx.ensure(4 * (size_t)n_slice + 64) != hipSuccess) { err = "filter: out of page-locked host memory"; return R3DM_ERR_NOMEM; }
    uint32_t* h_idx = static_cast<uint32_t*>(B.pin_idx.p);
    h_F.resize(9 * (size_t)NI);
    FHIP(hipMemcpyAsync(h_cnt.data(), B.f_inl_cnt.p, 4 * (size_t)NI, hipMemcpyDeviceToHost, c->stream));
    FHIP(hipMemcpyAsync(h_idx, B.f_inl_idx.p, 4 * (size_t)n_slice, hipMemcpyDeviceToHost, c->stream));
    FHIP(hipMemcpyAsync(h_F.data(), B.f_F.p, 72 * (size_t)NI, hipMemcpyDeviceToHost, c->stream));
    FHIP(hipStreamSynchronize(c->stream));
    ms_kernels = ms;
    if (fp.n_coop) {
        uint32_t qh[96];
        FHIP(hipMemcpy(qh, c->coop_sched.p, sizeof(qh), hipMemcpyDeviceToHost));
        qh[2] = qh[64];                                       // pairs finished (of all kinds of the call)
        if (qh[8] != 0u || qh[2] != qh[5]) {
            err = "filter: the cooperative kernel (kind " + std::to_string(kind.model_kind) + ") stalled (code " + std::to_string(qh[8]) + ", info " + std::to_string(qh[9]) + ", " +
                  std::to_string(qh[2]) + " of " + std::to_string(qh[5]) + " pairs finished; at the stall: idle bits " + std::to_string(qh[10]) + " / " +
                  std::to_string(qh[11]) + " finished " + std::to_string(qh[12]) + " potential " + std::to_string(qh[13]) + " workers " + std::to_string(qh[14]) +
                  " started " + std::to_string(qh[15]) + ")";
            return R3DM_ERR_HIP;
        }
    }
    // per-item diagnostics of this call (threshold px, NFA, iterations, models), in putative-pair order
    {
        std::vector<double> h_thr(2 * (size_t)NI);
        std::vector<uint32_t> h_it(2 * (size_t)NI);
        FHIP(hipMemcpyAsync(h_thr.data(), B.f_thr.p, 16 * (size_t)NI, hipMemcpyDeviceToHost, c->stream));
        FHIP(hipMemcpyAsync(h_it.data(), B.f_iters.p, 8 * (size_t)NI, hipMemcpyDeviceToHost, c->stream));
        FHIP(hipStreamSynchronize(c->stream));
        report.assign(a.putative->pairs.size() / 2, r3dm_pair_report{});
        for (uint32_t k = 0; k < NI; ++k) {
            r3dm_pair_report& r = report[plan.item_pair[k]];
            r.threshold_px = h_thr[2 * k]; r.nfa = h_thr[2 * k + 1];
            r.iterations = h_it[2 * k]; r.models = h_it[2 * k + 1]; r.inliers = h_cnt[k];
        }
    }
    const r3dm_graph& pg = *a.putative;
    if (c->guided_on) {
        // the accepted pairs are re-matched by guided matching; their lists replace the inliers once the call's guided launch has run
        // (finish); models and report stay AC-RANSAC's
        for (uint32_t k = 0; k < NI; ++k) {
            if (below_acceptance(h_cnt[k], kind.SS)) continue;
            GuidedJob jb;
            const int grc = guided_job_make(c, plan.slots[k].x, plan.slots[k].y, kind.guided, h_F.data() + 9 * (size_t)k,
                                            report[plan.item_pair[k]].threshold_px, c->guided_ratio[kind.guided], jb);
            if (grc != R3DM_OK) { err = c->err; return grc; }
            gjobs.push_back(jb);
            acc.push_back(k);
        }
        return R3DM_OK;
    }
    {
        uint64_t total_kept = 0;
        for (uint32_t k = 0; k < NI; ++k) total_kept += h_cnt[k];
        g->matches.reserve(total_kept);
    }
    // r3dm_set_device_graphs: the same inliers gathered on the device (putative matches through the inlier indices)
    GraphBuilder b(c, g.get(), c->device_graphs, pg.matches.data(), h_idx, fp.matches, B.f_inl_idx.as<uint32_t>());
    uint64_t kept = 0;
    for (uint32_t k = 0; k < NI; ++k) {
        if (below_acceptance(h_cnt[k], kind.SS)) continue;
        const uint32_t p = plan.item_pair[k];
        const uint64_t base = pg.offsets[p];
        if (kind.model_kind == 2 && poor_overlap(h_cnt[k], pg.offsets[p + 1] - base, a.min_count, a.min_ratio)) continue;
        b.add(pg.pairs[2 * p], pg.pairs[2 * p + 1], base, plan.soff[k], h_cnt[k]);
        if (M_out) memcpy(M_out + 9 * kept, h_F.data() + 9 * (size_t)k, 72);
        ++kept;
    }
    b.done();
    deliver();
    return R3DM_OK;
}

// the graph from the guided lists of the accepted pairs (job k of this call is job first + k of the launch)
void FilterCall::finish(const GuidedResult& R, size_t first)
{
    if (!g) return;                                       // (a kind without work items -- E without intrinsics -- has its graph already)
    const r3dm_graph& pg = *a.putative;
    GraphBuilder b(c, g.get(), c->device_graphs, R.host, nullptr, R.dev, nullptr);
    uint64_t kept = 0;
    for (size_t q = 0; q < acc.size(); ++q) {
        const uint32_t k = acc[q], p = plan.item_pair[k];
        const uint32_t n = R.cnt[first + q];
        // Regard3D's overlap rule behind the E filter applies to the guided list (it runs after Get_geometric_matches())
        if (kind.model_kind == 2 && poor_overlap(n, pg.offsets[p + 1] - pg.offsets[p], a.min_count, a.min_ratio)) continue;
        if (n == 0) continue;                             // no empty entries ("Guided matching")
        b.add(pg.pairs[2 * p], pg.pairs[2 * p + 1], gjobs[q].q0, 0, n);
        if (M_out) memcpy(M_out + 9 * kept, h_F.data() + 9 * (size_t)k, 72);
        ++kept;
    }
    b.done();
    deliver();
}

using FilterCalls = std::vector<std::unique_ptr<FilterCall>>;

// The cooperative kernel of a call: ONE pool of workers for the long pairs of all its filters (kernels_filter_coop.hip).  Builds the
// scheduling words (counters, idle bitmap, a mailbox line per worker), the start order (kind << 30 | pair, most work
// first) and the device copy of the FilterParams, and launches on the context's cooperative stream; c->coop_ev is recorded behind it.
static int coop_launch_shared(r3dm_ctx* c, std::string& err, FilterCalls& calls, bool& launched)
{
    launched = false;
    uint32_t n_pairs = 0, slots = 0;
    for (auto& k : calls) { n_pairs += k->fp.n_coop; slots += k->plan.coop_slots; }
    if (!n_pairs) return R3DM_OK;
    const int workers_knob = r3dm_dev_knob("R3DM_FILTER_COOP_WORKERS", 0);
    const uint32_t workers = std::min<uint32_t>(256u, workers_knob > 0 ? (uint32_t)workers_knob : std::min<uint32_t>(slots, (uint32_t)std::max(c->n_cu, 1)));   // (the idle bitmap has 256 bits)
    const size_t q_words = 96 + 32 * (size_t)workers;          // three lines of counters + one mailbox line per worker (kernels_filter_coop.hip)
    const size_t start_off = (q_words + 63) / 64 * 64, params_off = ((start_off + n_pairs) * 4 + 255) / 256 * 256;
    std::vector<unsigned char> stage(params_off + 3 * sizeof(FilterParams), 0);
    uint32_t* q = reinterpret_cast<uint32_t*>(stage.data());
    const int leaders_knob = r3dm_dev_knob("R3DM_FILTER_COOP_LEADERS", 0);
    q[5] = n_pairs; q[20] = workers; q[65] = slots; q[66] = workers;
    q[21] = leaders_knob > 0 ? (uint32_t)leaders_knob : std::max<uint32_t>(1u, (workers * 55u + 99u) / 100u);     // pairs led at a time
    for (uint32_t w = 0; w < workers; ++w) q[96 + 32 * (size_t)w] = 0xFFFFFFFEu;   // mailboxes: nobody waits yet
    // start order: the pair with the most work first
    struct Ent { double w; uint32_t v; };
    std::vector<Ent> ents;
    for (auto& k : calls)
        for (uint32_t p = 0; p < k->fp.n_coop; ++p) ents.push_back({k->kind.coop_work * k->plan.coop_len[p], ((uint32_t)k->kind.model_kind << 30) | p});
    std::stable_sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.w > b.w; });
    for (uint32_t i = 0; i < n_pairs; ++i) q[start_off + i] = ents[i].v;
    FHIP(c->coop_sched.ensure(stage.size()));
    unsigned char* base = c->coop_sched.as<unsigned char>();
    FilterParams* hp = reinterpret_cast<FilterParams*>(stage.data() + params_off);
    for (auto& k : calls) {
        // a kind without long pairs (none of its pairs is long, or it has no work items at all: E on views without intrinsics) leaves
        // its block zeroed -- the start order never names it -- and must not overwrite another kind's block
        if (!k->fp.n_coop) continue;
        k->fp.coop_q = reinterpret_cast<uint32_t*>(base);
        k->fp.coop_workers = workers;
        hp[k->kind.model_kind] = k->fp;
    }
    if (!c->coop_stream || !c->coop_ev) {
        hipStream_t s2 = nullptr; hipEvent_t e2 = nullptr;
        FHIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        const hipError_t e = hipEventCreate(&e2);
        if (e != hipSuccess) { (void)hipStreamDestroy(s2); FHIP(e); }
        c->coop_stream = s2; c->coop_ev = e2;
    }
    FHIP(hipMemcpyAsync(base, stage.data(), stage.size(), hipMemcpyHostToDevice, c->coop_stream));
    FHIP(launch_filter_coop(c->coop_stream, reinterpret_cast<const FilterParams*>(base + params_off), reinterpret_cast<uint32_t*>(base),
                            reinterpret_cast<const uint32_t*>(base) + start_off, workers));
    FHIP(hipEventRecord(c->coop_ev, c->coop_stream));
    FHIP(hipStreamSynchronize(c->coop_stream));          // `stage` leaves scope (and the kernels below are waited for anyway)
    launched = true;
    return R3DM_OK;
}

// launch + wait + HIP-event time of the kernels of the prepared calls: the one-workgroup-per-pair kernel of every kind's short pairs
// on a stream of its own (one filter: the context's stream; several: the kinds' priority streams), the cooperative kernel of all long
// pairs once for the call.  ms[k] = HIP-event time from the first launch to the end of kind k's short-pair kernel, or to the end of the
// cooperative kernel if that came later.
static int filter_launch(r3dm_ctx* c, std::string& err, FilterCalls& calls, float* ms)
{
    const int n = (int)calls.size();
    for (int k = 0; k < n; ++k) ms[k] = 0.f;
    int live = 0;
    for (int k = 0; k < n; ++k) live += calls[k]->fp.n_items ? 1 : 0;
    if (!live) return R3DM_OK;
    FHIP(hipStreamSynchronize(c->stream));                // every upload of the prepare steps has landed
    int prio_low = 0, prio_high = 0;
    FHIP(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));          // numerically: low >= high
    std::vector<hipStream_t> st(n, nullptr);
    std::vector<hipEvent_t> e0(n, nullptr), e1(n, nullptr);
    for (int k = 0; k < n; ++k) {
        if (!calls[k]->fp.n_items) continue;
        if (n == 1) { st[k] = c->stream; e0[k] = c->ev0; e1[k] = c->ev1; continue; }
        // r3dm_filter_FEH: the kernel of each kind on a stream of its own PRIORITY class (E high, F normal, H low).  Streams of one
        // priority share a handful of hardware queues -- three plain streams ran the three kernels mostly one after the other --,
        // streams of different priorities never do.
        FilterBufs& B = c->fb[calls[k]->kind.model_kind];
        if (!B.stream || !B.ev0 || !B.ev1) {
            // (all three or none: a half-made set would break every later call of the context)
            if (B.ev0) (void)hipEventDestroy(B.ev0);
            if (B.ev1) (void)hipEventDestroy(B.ev1);
            if (B.stream) (void)hipStreamDestroy(B.stream);
            B.stream = nullptr; B.ev0 = B.ev1 = nullptr;
            const int cls = calls[k]->kind.prio;
            const int prio = cls == 2 ? prio_high : (cls == 1 ? (prio_low + prio_high) / 2 : prio_low);
            hipStream_t s = nullptr; hipEvent_t a = nullptr, b = nullptr;
            hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio);
            if (e == hipSuccess) e = hipEventCreate(&a);
            if (e == hipSuccess) e = hipEventCreate(&b);
            if (e != hipSuccess) {
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
                if (s) (void)hipStreamDestroy(s);
                FHIP(e);
            }
            B.stream = s; B.ev0 = a; B.ev1 = b;
        }
        st[k] = B.stream; e0[k] = B.ev0; e1[k] = B.ev1;
    }
    // the short pairs of every kind first (cheap to launch), then the shared cooperative kernel; every bracket closes behind both
    for (int k = 0; k < n; ++k) {
        const FilterParams& fp = calls[k]->fp;
        if (!fp.n_items) continue;
        FHIP(hipEventRecord(e0[k], st[k]));
        if (fp.n_short) FHIP(launch_filter_F(st[k], fp));
    }
    bool coop = false;
    const int rc = coop_launch_shared(c, err, calls, coop);
    {   // occupancy bookkeeping of the call (r3dm_stats): workgroups launched, items on the cooperative kernel
        uint64_t wgs = 0, items = 0;
        for (int k = 0; k < n; ++k) { wgs += calls[k]->fp.n_short; items += calls[k]->fp.n_coop; }
        for (int k = 0; k < n; ++k) if (coop && calls[k]->fp.n_coop) { wgs += calls[k]->fp.coop_workers; break; }
        c->stats.n_filter_workgroups = wgs; c->stats.n_filter_coop_pairs = coop ? items : 0;
    }
    hipError_t first = hipSuccess;
    for (int k = 0; k < n; ++k) {
        if (!calls[k]->fp.n_items) continue;
        if (rc == R3DM_OK) {
            if (coop && calls[k]->fp.n_coop) (void)hipStreamWaitEvent(st[k], c->coop_ev, 0);
            (void)hipEventRecord(e1[k], st[k]);
        }
        const hipError_t e = hipStreamSynchronize(st[k]);                 // wait for ALL of them, whatever one of them says
        if (e != hipSuccess && first == hipSuccess) first = e;
        if (e == hipSuccess && rc == R3DM_OK) (void)hipEventElapsedTime(&ms[k], e0[k], e1[k]);
    }
    if (rc != R3DM_OK) return rc;
    FHIP(first);
    return R3DM_OK;
}

// What run_filters leaves for the entries' own bookkeeping besides the calls themselves
struct FilterRun {
    float ms[3] = {0.f, 0.f, 0.f};             // HIP-event time of each call's kernels (filter_launch)
    size_t collects = 0;                       // calls whose collect ran, in order (only the last of them can have failed)
    double t0 = 0.0, t_prep = 0.0, t_launch = 0.0;
};

// The one sequence of every filter entry: prepare each call (later kinds reuse the putative matches the first one uploaded) ->
// filter_launch -> collect each call -> with guided matching on, ONE guided launch for the accepted pairs of all calls -> finish each.
// Errors are left in c->err.
static int run_filters(r3dm_ctx* c, FilterCalls& calls, FilterRun& run)
{
    const size_t n = calls.size();
    run.t0 = now_ms();
    int rc = R3DM_OK;
    for (size_t i = 0; i < n && rc == R3DM_OK; ++i) {
        rc = calls[i]->prepare(i > 0 && calls[0]->fp.n_items ? calls[0]->fp.matches : nullptr);
        if (rc != R3DM_OK && !calls[i]->err.empty()) c->err = calls[i]->err;
    }
    run.t_prep = now_ms();
    if (rc == R3DM_OK) {
        std::string err;
        rc = filter_launch(c, err, calls, run.ms);
        if (rc != R3DM_OK && !err.empty()) c->err = err;
    }
    run.t_launch = now_ms();
    // the kinds' results come back side by side as well: each collect is a few copies into its own page-locked buffer and the host-side
    // assembly of its graph (inlier indices -> matches), 1.5-2 ms per kind on a stage's graph; a thread per kind.  (Not with device
    // mirrors -- they share the context's gather scratch -- and not in the developer build, whose traces and checks are written
    // for one collect at a time.)
    std::vector<int> rcs(n, R3DM_OK);
    bool threaded = false;
#ifndef R3DM_DEVTOOLS
    if (rc == R3DM_OK && n > 1 && !c->device_graphs) {
        auto collect = [&](size_t i) { try { rcs[i] = calls[i]->collect(run.ms[i]); } catch (...) { rcs[i] = R3DM_ERR_NOMEM; } };
        std::vector<std::thread> th;
        try {
            for (size_t i = 1; i < n; ++i) th.emplace_back([&, i]() { (void)hipSetDevice(c->device); collect(i); });
        } catch (...) {}                                   // fewer threads than kinds: the rest is collected below
        collect(0);
        const size_t started = th.size();
        for (std::thread& t : th) t.join();
        for (size_t i = 1 + started; i < n; ++i) collect(i);
        threaded = true;
    }
#endif
    for (; run.collects < n && rc == R3DM_OK; ++run.collects) {
        FilterCall& k = *calls[run.collects];
        rc = threaded ? rcs[run.collects] : k.collect(run.ms[run.collects]);
        k.collected = rc == R3DM_OK;
        if (rc != R3DM_OK && !k.err.empty()) c->err = k.err;
    }
    if (rc == R3DM_OK && c->guided_on) {                  // (also without accepted pairs: the guided report then says so)
        std::vector<GuidedJob> all;
        std::vector<size_t> first(n, 0);
        for (size_t i = 0; i < n; ++i) { first[i] = all.size(); all.insert(all.end(), calls[i]->gjobs.begin(), calls[i]->gjobs.end()); }
        GuidedResult R;
        rc = guided_run(c, all, R);
        for (size_t i = 0; i < n && rc == R3DM_OK; ++i) {
            FilterCall& k = *calls[i];
            for (size_t q = 0; q < k.gjobs.size(); ++q) k.gjobs[q].q0 = all[first[i] + q].q0;
            k.finish(R, first[i]);
        }
    }
    return rc;
}

// r3dm_filter_F / _E / _H: one call; its kernel time and wall time (guided finish included) in the statistics, its report only on success
static int filter_single(r3dm_ctx* c, const FilterKind& kind, const FilterArgs& a, r3dm_graph** out, double* M_out)
{
    if (!c) return R3DM_ERR_INVALID;
    FilterCalls calls;
    calls.emplace_back(new FilterCall(c, kind, a, out, M_out));
    FilterRun run;
    const int rc = run_filters(c, calls, run);
    const FilterCall& k = *calls[0];
    c->stats.ms_filter_kernels = k.ms_kernels;
    c->stats.ms_wall_filter = k.ms_wall;
    if (rc == R3DM_OK) c->report = std::move(calls[0]->report);
    return rc;
}

extern "C" int r3dm_filter_F(r3dm_ctx* c, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                             uint64_t seed, r3dm_ferror err_kind, r3dm_graph** out, double* F_out)
{
    return r3dm_guarded(c, [&]() -> int { return filter_single(c, kKinds[0], {putative, max_residual_px, max_iter, seed, err_kind, 0u, 0.f}, out, F_out); });
}

extern "C" int r3dm_filter_H(r3dm_ctx* c, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                             uint64_t seed, r3dm_graph** out, double* H_out)
{
    return r3dm_guarded(c, [&]() -> int {
        return filter_single(c, kKinds[2], {putative, max_residual_px, max_iter, seed, R3DM_ERR_SYMMETRIC_EPIPOLAR, 0u, 0.f}, out, H_out);
    });
}

extern "C" int r3dm_set_intrinsics(r3dm_ctx* c, uint32_t view_id, const double* K)
{
    if (!c) return R3DM_ERR_INVALID;
    auto it = c->slot_of.find(view_id);
    if (it == c->slot_of.end()) { c->err = "r3dm_set_intrinsics: unregistered view"; return R3DM_ERR_INVALID; }
    HostImage& h = *c->imgs[it->second];
    if (!K) { h.has_K = false; return R3DM_OK; }
    // inverse by the adjugate, operation for operation what oracle/essential.c orc_inv3 does
    const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
    const double det = K[0] * c00 + K[1] * c01 + K[2] * c02;
    if (!(det != 0.0) || !std::isfinite(det)) { c->err = "r3dm_set_intrinsics: singular K"; return R3DM_ERR_INVALID; }
    const double id = 1.0 / det;
    h.Kinv[0] = c00 * id; h.Kinv[1] = (K[2] * K[7] - K[1] * K[8]) * id; h.Kinv[2] = (K[1] * K[5] - K[2] * K[4]) * id;
    h.Kinv[3] = c01 * id; h.Kinv[4] = (K[0] * K[8] - K[2] * K[6]) * id; h.Kinv[5] = (K[2] * K[3] - K[0] * K[5]) * id;
    h.Kinv[6] = c02 * id; h.Kinv[7] = (K[1] * K[6] - K[0] * K[7]) * id; h.Kinv[8] = (K[0] * K[4] - K[1] * K[3]) * id;
    h.has_K = true;
    return R3DM_OK;
}

extern "C" int r3dm_filter_E(r3dm_ctx* c, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter,
                             uint64_t seed, uint32_t min_count, float min_ratio, r3dm_graph** out, double* E_out)
{
    return r3dm_guarded(c, [&]() -> int {
        return filter_single(c, kKinds[1], {putative, max_residual_px, max_iter, seed, R3DM_ERR_SYMMETRIC_EPIPOLAR, min_count, min_ratio}, out, E_out);
    });
}

// F, E and H of one putative graph side by side.  Long pairs (>= R3DM_FILTER_COOP_MIN putatives, 4096) of ALL requested filters run on
// ONE cooperative kernel -- a pool of <= 256 persistent workgroups in which a pair's residual passes are row slices handed to idle
// workers (kernels_filter_coop.hip) -- so a collection of few, long pairs (24 photographs: 94 putative pairs of
// 10-20 k matches) fills the chip instead of a third of it, and a pair is no longer bound by one CU's f64 rate.  Short pairs keep the
// one-workgroup-per-pair kernels, one launch per kind on streams of three priority classes, beside the cooperative kernel.  What lets
// kernels overlap at all was taking the agent-scope fences out of their barriers (filter_device.hpp: wg_fence).  Measured and
// dropped in round 3: one merged one-workgroup-per-pair kernel with the three model kinds as branches (hipcc's code for the
// fundamental-matrix branch faulted, product build only, spilled lists only); the cooperative kernel keeps its phases out of line
// (noinline) for the same family of reasons.
extern "C" int r3dm_filter_FEH(r3dm_ctx* c, const r3dm_graph* putative, double max_residual_px, uint32_t max_iter, uint64_t seed, int which,
                               uint32_t e_min_count, float e_min_ratio, r3dm_graph** out_F, r3dm_graph** out_E, r3dm_graph** out_H,
                               double* ms_kernels3, double* ms_wall3)
{
    if (!c || !putative || (which & 7) == 0) return R3DM_ERR_INVALID;
    if (((which & 1) && !out_F) || ((which & 2) && !out_E) || ((which & 4) && !out_H)) return R3DM_ERR_INVALID;
    return r3dm_guarded(c, [&]() -> int {
        r3dm_graph** outs[3] = {out_F, out_E, out_H};
        for (r3dm_graph** o : outs) if (o) *o = nullptr;
        if (ms_kernels3) ms_kernels3[0] = ms_kernels3[1] = ms_kernels3[2] = 0.0;
        if (ms_wall3) ms_wall3[0] = ms_wall3[1] = ms_wall3[2] = 0.0;
        const FilterArgs a{putative, max_residual_px, max_iter, seed, R3DM_ERR_SYMMETRIC_EPIPOLAR, e_min_count, e_min_ratio};
        FilterCalls calls;                                 // in the order F, E, H
        for (const FilterKind& kind : kKinds)
            if (which & (1 << kind.slot)) calls.emplace_back(new FilterCall(c, kind, a, outs[kind.slot], nullptr));
        FilterRun run;
        const int rc = run_filters(c, calls, run);
        float ms_max = 0.f;
        for (size_t i = 0; i < run.collects; ++i) {
            const FilterCall& k = *calls[i];
            ms_max = std::max(ms_max, run.ms[i]);
            if (ms_kernels3) ms_kernels3[k.kind.slot] = run.ms[i];
            if (ms_wall3) ms_wall3[k.kind.slot] = k.ms_wall;
        }
        for (auto& k : calls)                              // the E call's diagnostics, else the last requested kind's
            if (k->collected && (k->kind.model_kind == 2 || !(which & 2))) c->report = k->report;
        c->stats.ms_filter_kernels = ms_max;
        FilterDiag::timing(run.t0, run.t_prep, run.t_launch, ms_max);
        if (rc != R3DM_OK)
            for (r3dm_graph** o : outs) if (o && *o) { r3dm_graph_free(*o); *o = nullptr; }
        return rc;
    });
}

extern "C" int r3dm_filter_report(const r3dm_ctx* c, r3dm_pair_report* out, uint64_t cap)
{
    if (!c || (cap && !out)) return R3DM_ERR_INVALID;
    const uint64_t n = std::min<uint64_t>(cap, c->report.size());
    if (n) memcpy(out, c->report.data(), n * sizeof(r3dm_pair_report));
    return (int)std::min<uint64_t>(c->report.size(), 0x7FFFFFFF);
}
