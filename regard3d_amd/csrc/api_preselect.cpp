// api_preselect.cpp -- part of the host side of libr3dm.so: opt-in preemptive matching (include/r3dm.h: r3dm_set_preemptive_matching;
// DESIGN.md section 4.25).  View priorities, the head of a view (host selection + one gather kernel), the gate the four collection
// entries call right after resolve_pairs, and the primitive r3dm_preselect_pairs.  The kernels are in kernels_match_head.hip.  There
// is no CPU fallback in this file: when HIP fails, the call fails.
#include "r3dm_ctx.hpp"

namespace {

constexpr uint32_t kHeadMin = 2, kHeadMax = 256;

// rows of the head of a view of n rows for head size h, ascending: the min(h, n) rows that come first under (priority descending,
// row index ascending); no priority: the first rows
void head_rows_of(const std::vector<float>& priority, uint32_t n, uint32_t h, uint32_t* out)
{
    const uint32_t hn = std::min(h, n);
    if (priority.empty() || hn == n) { for (uint32_t k = 0; k < hn; ++k) out[k] = k; return; }
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    const float* p = priority.data();
    std::nth_element(idx.begin(), idx.begin() + hn, idx.end(), [p](uint32_t a, uint32_t b) { return p[a] != p[b] ? p[a] > p[b] : a < b; });
    std::sort(idx.begin(), idx.begin() + hn);
    std::copy(idx.begin(), idx.begin() + hn, out);
}

// the class of a view's gate kernel: binary | G or words; false -> no kernel serves the length
bool head_class(const HostImage& h, bool& binary, uint32_t& per_row, uint32_t& klass)
{
    binary = h.dtype == R3DM_BIN;
    if (binary) { per_row = klass = h.words; return h.words == 8 || h.words == 16; }
    klass = h.G; per_row = h.G * 2;
    return has_tensor_kernel(h.G);
}

struct GateTimer {
    r3dm_ctx* c;
    int begin()
    {
        if (!c->pre_ev0) R3DM_HIP(c, hipEventCreate(&c->pre_ev0));
        if (!c->pre_ev1) R3DM_HIP(c, hipEventCreate(&c->pre_ev1));
        R3DM_HIP(c, hipEventRecord(c->pre_ev0, c->stream));
        return R3DM_OK;
    }
};

// the heads of the listed slots (sorted, unique) for head size h: those that are missing, or were made for another h, are selected on
// the host into `lists` (page-locked, room for min(h, n) rows of every listed slot), uploaded in one copy, and gathered by one kernel
// per view
int ensure_heads(r3dm_ctx* c, const std::vector<uint32_t>& slots, uint32_t h, uint32_t* lists)
{
    std::vector<uint32_t> todo;
    size_t total = 0;
    for (uint32_t s : slots) {
        HostImage& v = *c->imgs[s];
        if (v.priority.empty()) c->preselect_stats.n_views_without_priority += 1;
        if ((v.have & kLayHead) && v.head_h == h) continue;
        todo.push_back(s); total += std::min(h, v.n);
    }
    if (todo.empty()) return R3DM_OK;
    R3DM_HIP(c, c->pre_rows.ensure(total * 4));
    std::vector<size_t> at(todo.size());
    { size_t o = 0; for (size_t k = 0; k < todo.size(); ++k) { at[k] = o; o += std::min(h, c->imgs[todo[k]]->n); } }
    r3dm_parallel_for((long)todo.size(), r3dm_host_team(8), [&](long k) {
        const HostImage& v = *c->imgs[todo[(size_t)k]];
        try { head_rows_of(v.priority, v.n, h, lists + at[(size_t)k]); }
        catch (...) { for (uint32_t r = 0, hn = std::min(h, v.n); r < hn; ++r) lists[at[(size_t)k] + r] = kNone; }      // (out of memory: reported below)
    });
    for (size_t k = 0; k < todo.size(); ++k) if (lists[at[k]] == kNone) { c->err = "out of host memory"; return R3DM_ERR_NOMEM; }
    R3DM_HIP(c, hipMemcpyAsync(c->pre_rows.p, lists, total * 4, hipMemcpyHostToDevice, c->stream));
    for (size_t k = 0; k < todo.size(); ++k) {
        HostImage& v = *c->imgs[todo[k]];
        bool binary; uint32_t per_row, klass;
        (void)head_class(v, binary, per_row, klass);
        const uint32_t hn = std::min(h, v.n);
        v.have &= ~kLayHead;
        R3DM_HIP(c, v.head.ensure((size_t)hn * per_row * (binary ? 4 : 16)));
        R3DM_HIP(c, launch_head_gather(c->stream, binary ? (const void*)v.bin.p : (const void*)v.tiled.p, c->pre_rows.as<uint32_t>() + at[k], hn, per_row, binary, v.head.p));
        v.have |= kLayHead; v.head_h = h; v.head_n = hn;
        c->preselect_stats.n_heads_built += 1;
    }
    return R3DM_OK;
}

struct GatePair { uint32_t sI, sJ; };

// counts[p] = the head count of pairs[p] (slots of two non-empty views of one type and length) for head size h under ratio R
// (R_bin >= 0: the R of the binary classes instead)
int head_counts(r3dm_ctx* c, const std::vector<GatePair>& pairs, uint32_t h, float R, std::vector<uint32_t>& counts, float R_bin = -1.0f)
{
    counts.assign(pairs.size(), 0u);
    if (pairs.empty()) return R3DM_OK;
    // one launch per length class: pairs grouped by class, each remembering its place in the caller's order
    struct Class { bool binary; uint32_t klass; std::vector<HeadPair> pairs; };
    std::vector<Class> classes;
    std::vector<uint32_t> slots;
    slots.reserve(2 * pairs.size());
    for (size_t p = 0; p < pairs.size(); ++p) {
        const HostImage& A = *c->imgs[pairs[p].sI];
        bool binary; uint32_t per_row, klass;
        if (!head_class(A, binary, per_row, klass)) { c->err = "preemptive matching serves float / byte rows of at most 256 elements"; return R3DM_ERR_UNSUPPORTED; }
        auto it = std::find_if(classes.begin(), classes.end(), [&](const Class& k) { return k.binary == binary && k.klass == klass; });
        if (it == classes.end()) { classes.push_back(Class{binary, klass, {}}); it = classes.end() - 1; }
        it->pairs.push_back(HeadPair{pairs[p].sI, pairs[p].sJ, (uint32_t)p});
        slots.push_back(pairs[p].sI); slots.push_back(pairs[p].sJ);
    }
    if (pairs.size() > 0xFFFFFFFFull) { c->err = "too many pairs for one gate call"; return R3DM_ERR_UNSUPPORTED; }
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    // one page-locked block for the call, sized before anything is queued (every earlier call has ended with a synchronisation):
    // head table by slot | pairs | counts coming back | row lists of the heads to make
    const size_t n_slots = c->imgs.size();
    const size_t tab_bytes = n_slots * sizeof(HeadDev), pair_bytes = pairs.size() * sizeof(HeadPair), cnt_bytes = pairs.size() * 4;
    size_t list_rows = 0;
    for (uint32_t s : slots) list_rows += std::min(h, c->imgs[s]->n);
    R3DM_HIP(c, c->pre_pin.ensure(tab_bytes + pair_bytes + cnt_bytes + list_rows * 4));
    R3DM_HIP(c, c->pre_heads.ensure(tab_bytes));
    R3DM_HIP(c, c->pre_pairs.ensure(pair_bytes));
    R3DM_HIP(c, c->pre_counts.ensure(cnt_bytes));
    GateTimer timer{c};
    { const int rc = timer.begin(); if (rc != R3DM_OK) return rc; }
    { const int rc = ensure_heads(c, slots, h, reinterpret_cast<uint32_t*>(c->pre_pin.as<unsigned char>() + tab_bytes + pair_bytes + cnt_bytes)); if (rc != R3DM_OK) return rc; }
    HeadDev* tab = c->pre_pin.as<HeadDev>();
    for (size_t s = 0; s < n_slots; ++s) {
        const HostImage* v = c->imgs[s].get();
        const bool has = v && (v->have & kLayHead);
        tab[s] = HeadDev{has ? v->head.p : nullptr, has ? v->head_n : 0u, v ? v->dim : 0u};
    }
    HeadPair* hp = reinterpret_cast<HeadPair*>(c->pre_pin.as<unsigned char>() + tab_bytes);
    { size_t o = 0; for (const Class& k : classes) { std::copy(k.pairs.begin(), k.pairs.end(), hp + o); o += k.pairs.size(); } }
    R3DM_HIP(c, hipMemcpyAsync(c->pre_heads.p, tab, tab_bytes, hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(c->pre_pairs.p, hp, pair_bytes, hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipMemsetAsync(c->pre_counts.p, 0, pairs.size() * 4, c->stream));
    HeadMatchParams P{};
    P.heads = c->pre_heads.as<HeadDev>(); P.counts = c->pre_counts.as<uint32_t>(); P.ratio_R = R;
    size_t o = 0;
    for (const Class& k : classes) {
        P.ratio_R = (k.binary && R_bin >= 0.0f) ? R_bin : R;
        // one workgroup per pair: launches stay below kMaxBlocksOf256
        for (size_t s = 0; s < k.pairs.size();) {
            const size_t cnt = std::min<size_t>(k.pairs.size() - s, (size_t)kMaxBlocksOf256 - 8);
            P.pairs = c->pre_pairs.as<HeadPair>() + o + s;
            R3DM_HIP(c, launch_head_match(c->stream, P, (uint32_t)cnt, k.binary, k.klass));
            s += cnt;
        }
        o += k.pairs.size();
    }
    R3DM_HIP(c, hipEventRecord(c->pre_ev1, c->stream));
    uint32_t* back = reinterpret_cast<uint32_t*>(c->pre_pin.as<unsigned char>() + tab_bytes + pair_bytes);
    R3DM_HIP(c, hipMemcpyAsync(back, c->pre_counts.p, pairs.size() * 4, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    std::copy(back, back + pairs.size(), counts.begin());
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->pre_ev0, c->pre_ev1) == hipSuccess) c->preselect_stats.ms_kernels += ms;
    return R3DM_OK;
}

}  // namespace

int preselect_gate(r3dm_ctx* c, float ratio_R, std::vector<PairJob>& indexed, std::vector<PairJob>& scanned, float bin_ratio_R)
{
    c->preselect_stats = r3dm_preselect_stats{};
    if (!c->preemptive_on) return R3DM_OK;
    const double t0 = now_ms();
    std::vector<GatePair> pairs;
    pairs.reserve(indexed.size() + scanned.size());
    for (const auto* v : {&indexed, &scanned}) for (const PairJob& j : *v) pairs.push_back(GatePair{j.sI, j.sJ});
    std::vector<uint32_t> counts;
    const int rc = head_counts(c, pairs, c->preemptive_h, ratio_R, counts, bin_ratio_R);
    if (rc != R3DM_OK) return rc;
    size_t p = 0;
    for (auto* v : {&indexed, &scanned}) {
        size_t w = 0;
        for (size_t k = 0; k < v->size(); ++k, ++p) if (counts[p] >= c->preemptive_t) (*v)[w++] = (*v)[k];
        v->resize(w);
    }
    c->preselect_stats.n_pairs = pairs.size();
    c->preselect_stats.n_kept = indexed.size() + scanned.size();
    c->preselect_stats.ms_wall = now_ms() - t0;
    return R3DM_OK;
}

static int r3dm_set_view_priority_impl(r3dm_ctx* c, uint32_t view_id, const float* priority, uint32_t n)
{
    if (!c) return R3DM_ERR_INVALID;
    auto it = c->slot_of.find(view_id);
    if (it == c->slot_of.end()) { c->err = "unregistered view"; return R3DM_ERR_INVALID; }
    HostImage& v = *c->imgs[it->second];
    if (priority) {
        if (n != v.n) { c->err = "one priority per row of the view"; return R3DM_ERR_INVALID; }
        for (uint32_t k = 0; k < n; ++k) if (!(std::isfinite(priority[k]) && priority[k] >= 0.0f)) { c->err = "priorities must be finite and >= 0"; return R3DM_ERR_INVALID; }
        std::vector<float> p(priority, priority + n);
        for (float& x : p) x += 0.0f;                 // -0.0 -> +0.0
        v.priority.swap(p);
    } else {
        std::vector<float>().swap(v.priority);
    }
    v.have &= ~kLayHead; v.head_h = 0; v.head_n = 0;  // (the buffer stays: the next head of the view reuses it)
    v.have &= ~kLayBudget; v.bud_N = 0;               // (the match budget's sub-view was selected by the old priority: its slot is refilled)
    return R3DM_OK;
}

extern "C" int r3dm_set_view_priority(r3dm_ctx* c, uint32_t view_id, const float* priority, uint32_t n)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_set_view_priority_impl(c, view_id, priority, n); });
}

extern "C" int r3dm_set_preemptive_matching(r3dm_ctx* c, int enable, uint32_t head_rows, uint32_t min_matches)
{
    if (!c) return R3DM_ERR_INVALID;
    if (head_rows < kHeadMin || head_rows > kHeadMax || min_matches < 1) { c->err = "preemptive matching: head_rows in 2..256, min_matches >= 1"; return R3DM_ERR_INVALID; }
    c->preemptive_on = (enable != 0); c->preemptive_h = head_rows; c->preemptive_t = min_matches;
    return R3DM_OK;
}

extern "C" int r3dm_preselect_report(const r3dm_ctx* c, r3dm_preselect_stats* out)
{
    if (!c || !out) return R3DM_ERR_INVALID;
    *out = c->preselect_stats;
    return R3DM_OK;
}

static int r3dm_preselect_pairs_impl(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs, uint32_t head_rows, float dist_ratio,
                                     int squared_metric, uint32_t* counts_out)
{
    if (!c || (n_pairs && (!pairs_ij || !counts_out))) return R3DM_ERR_INVALID;
    if (head_rows < kHeadMin || head_rows > kHeadMax) { c->err = "preemptive matching: head_rows in 2..256"; return R3DM_ERR_INVALID; }
    R3DM_HIP(c, hipSetDevice(c->device));
    c->preselect_stats = r3dm_preselect_stats{};
    const double t0 = now_ms();
    std::vector<GatePair> pairs;
    std::vector<uint64_t> where;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        auto a = c->slot_of.find(pairs_ij[2 * p]), b = c->slot_of.find(pairs_ij[2 * p + 1]);
        if (a == c->slot_of.end() || b == c->slot_of.end()) { c->err = "pair references an unregistered view"; return R3DM_ERR_INVALID; }
        const HostImage& A = *c->imgs[a->second];
        const HostImage& B = *c->imgs[b->second];
        counts_out[p] = 0;
        if (A.n == 0 || B.n == 0 || A.dtype != B.dtype || A.dim != B.dim) continue;       // as resolve_pairs skips them
        pairs.push_back(GatePair{a->second, b->second}); where.push_back(p);
    }
    std::vector<uint32_t> counts;
    const int rc = head_counts(c, pairs, head_rows, squared_metric ? dist_ratio * dist_ratio : dist_ratio, counts);
    if (rc != R3DM_OK) return rc;
    uint64_t kept = 0;
    for (size_t k = 0; k < counts.size(); ++k) { counts_out[where[k]] = counts[k]; kept += counts[k] >= c->preemptive_t; }
    c->preselect_stats.n_pairs = pairs.size();          // (as the gate of a match entry: pairs with an empty view or views of two types are not looked at)
    c->preselect_stats.n_kept = kept;
    c->preselect_stats.ms_wall = now_ms() - t0;
    return R3DM_OK;
}

extern "C" int r3dm_preselect_pairs(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs, uint32_t head_rows, float dist_ratio,
                                    int squared_metric, uint32_t* counts_out)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_preselect_pairs_impl(c, pairs_ij, n_pairs, head_rows, dist_ratio, squared_metric, counts_out); });
}
