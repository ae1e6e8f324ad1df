// api_budget.cpp -- part of the host side of libr3dm.so: the opt-in match budget (include/r3dm.h: r3dm_set_match_budget; DESIGN.md
// section 4.29).  A view of more than N rows is matched through a sub-view of its N highest-priority rows: the rows are selected on the
// device, gathered out of the view's resident layout and staged into a slot of their own exactly as a registered view is staged, so
// every layout, index and arm works on it without knowing about budgets; the substitution step the four collection entries call right
// after the gate swaps the jobs' slots, and finalize_batch sends every batch's matches back through the row lists (budget_remap) before
// anything leaves the device.  The kernels are in kernels_match_budget.hip.  There is no CPU fallback in this file: when HIP fails,
// the call fails.
#include "r3dm_ctx.hpp"

namespace {

constexpr uint32_t kBudgetMin = 2;
constexpr size_t kGatherGroupBytes = (size_t)64 << 20;       // gathered rows on their way into sub-view slots, per group of views

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

int budget_events(r3dm_ctx* c)
{
    for (hipEvent_t& e : c->bud_ev) if (!e) R3DM_HIP(c, hipEventCreate(&e));
    return R3DM_OK;
}

// elapsed time between the context's two budget events, both passed
double budget_elapsed(r3dm_ctx* c)
{
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, c->bud_ev[0], c->bud_ev[1]) == hipSuccess ? (double)ms : 0.0;
}

// the selection of every listed slot (views of more than N rows) in one launch: the priorities travel now -- nothing of them is on the
// device before a view is budgeted -- and outs[k] receives the N rows of slots[k], ascending.  Bracketed by the budget events, not
// waited for.
int select_rows(r3dm_ctx* c, const std::vector<uint32_t>& slots, uint32_t N, const std::vector<uint32_t*>& outs)
{
    const size_t V = slots.size(), job_bytes = align256(V * sizeof(BudgetSelectJob));
    size_t floats = 0;
    for (uint32_t s : slots) if (!c->imgs[s]->priority.empty()) floats += c->imgs[s]->n;
    R3DM_HIP(c, c->bud_pin.ensure(job_bytes + floats * 4));
    R3DM_HIP(c, c->bud_jobs.ensure(job_bytes));
    if (floats) R3DM_HIP(c, c->bud_prio.ensure(floats * 4));
    BudgetSelectJob* jobs = c->bud_pin.as<BudgetSelectJob>();
    float* hp = reinterpret_cast<float*>(c->bud_pin.as<unsigned char>() + job_bytes);
    size_t at = 0;
    for (size_t k = 0; k < V; ++k) {
        const HostImage& v = *c->imgs[slots[k]];
        const float* dev = nullptr;
        if (!v.priority.empty()) {
            std::memcpy(hp + at, v.priority.data(), (size_t)v.n * 4);
            dev = c->bud_prio.as<float>() + at; at += v.n;
        }
        jobs[k] = BudgetSelectJob{dev, v.n, N, outs[k]};
    }
    R3DM_HIP(c, hipMemcpyAsync(c->bud_jobs.p, jobs, V * sizeof(BudgetSelectJob), hipMemcpyHostToDevice, c->stream));
    if (floats) R3DM_HIP(c, hipMemcpyAsync(c->bud_prio.p, hp, floats * 4, hipMemcpyHostToDevice, c->stream));
    R3DM_HIP(c, hipEventRecord(c->bud_ev[0], c->stream));
    R3DM_HIP(c, launch_budget_select(c->stream, c->bud_jobs.as<BudgetSelectJob>(), (uint32_t)V));
    R3DM_HIP(c, hipEventRecord(c->bud_ev[1], c->stream));
    return R3DM_OK;
}

// makes the sub-views of the listed slots (views of more than N rows whose sub-view is missing or was made for another N, priority or
// registration): one selection launch, then group by group the gather kernels and the staging of every gathered view into its slot
int build_subviews(r3dm_ctx* c, const std::vector<uint32_t>& todo, uint32_t N)
{
    std::vector<uint32_t*> outs;
    outs.reserve(todo.size());
    for (uint32_t s : todo) {
        HostImage& v = *c->imgs[s];
        v.have &= ~kLayBudget; v.bud_N = 0;
        if (v.bud_slot == kNone) {
            // a slot of the table like a registered view's, behind the ones that exist, reachable through no view id
            c->imgs.push_back(std::unique_ptr<HostImage>(new HostImage()));
            c->imgs.back()->use_arena(&c->arena);
            v.bud_slot = (uint32_t)c->imgs.size() - 1;
        }
        R3DM_HIP(c, v.bud_rows.ensure((size_t)N * 4));
        R3DM_HIP(c, hipMemsetAsync(v.bud_rows.p, 0, (size_t)N * 4, c->stream));
        outs.push_back(v.bud_rows.as<uint32_t>());
    }
    { const int rc = select_rows(c, todo, N, outs); if (rc != R3DM_OK) return rc; }
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    c->budget_stats.ms_select += budget_elapsed(c);
    for (size_t k0 = 0; k0 < todo.size();) {
        size_t k1 = k0, bytes = 0;
        std::vector<size_t> off;
        while (k1 < todo.size()) {
            const HostImage& v = *c->imgs[todo[k1]];
            const size_t need = align256((size_t)N * v.dim * (v.dtype == R3DM_F32 ? 4 : 1)) + align256((size_t)N * 8);
            if (k1 > k0 && bytes + need > kGatherGroupBytes) break;
            off.push_back(bytes); bytes += need; ++k1;
        }
        R3DM_HIP(c, c->bud_raw.ensure(bytes));
        R3DM_HIP(c, hipEventRecord(c->bud_ev[0], c->stream));
        for (size_t k = k0; k < k1; ++k) {
            const HostImage& v = *c->imgs[todo[k]];
            unsigned char* dst = c->bud_raw.as<unsigned char>() + off[k - k0];
            BudgetGatherArgs A{};
            const bool binary = v.dtype == R3DM_BIN;
            A.src = binary ? (const void*)v.bin.p : (const void*)v.tiled.p; A.rows = v.bud_rows.as<uint32_t>();
            A.n = v.n; A.hn = N; A.dim = v.dim; A.per_row = binary ? v.words : v.G * 2; A.dtype = (int)v.dtype; A.out = dst;
            A.xy = v.has_xy ? v.xy.as<float>() : nullptr;
            A.xy_out = reinterpret_cast<float*>(dst + align256((size_t)N * v.dim * (v.dtype == R3DM_F32 ? 4 : 1)));
            R3DM_HIP(c, launch_budget_gather(c->stream, A));
        }
        R3DM_HIP(c, hipEventRecord(c->bud_ev[1], c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));       // the staging copies run on the ring's stream: the gathered rows must be there
        c->budget_stats.ms_gather += budget_elapsed(c);
        for (size_t k = k0; k < k1; ++k) {
            HostImage& v = *c->imgs[todo[k]];
            const unsigned char* src = c->bud_raw.as<unsigned char>() + off[k - k0];
            const float* xy = v.has_xy ? reinterpret_cast<const float*>(src + align256((size_t)N * v.dim * (v.dtype == R3DM_F32 ? 4 : 1))) : nullptr;
            // (returns when the ring's copy has read the gathered rows: the next group may overwrite them)
            const int rc = stage_into_slot(c, v.bud_slot, v.view_id, v.width, v.height, src, N, v.dim, v.dtype, xy);
            if (rc != R3DM_OK) return rc;
            c->imgs[v.bud_slot]->live = false;              // not a view of the collection (r3dm_exhaustive_is_faster)
            v.have |= kLayBudget; v.bud_N = N;
            c->budget_stats.n_subviews_built += 1;
        }
        k0 = k1;
    }
    return R3DM_OK;
}

}  // namespace

int budget_substitute(r3dm_ctx* c, std::vector<PairJob>& indexed, std::vector<PairJob>& scanned, const PairClassifier& classify)
{
    c->budget_stats = r3dm_budget_stats{};
    c->bud_maps_live = false;
    if (!c->budget_on) return R3DM_OK;
    const double t0 = now_ms();
    const uint32_t N = c->budget_N;
    std::vector<uint32_t> slots;
    slots.reserve(2 * (indexed.size() + scanned.size()));
    for (const auto* v : {&indexed, &scanned}) for (const PairJob& j : *v) { slots.push_back(j.sI); slots.push_back(j.sJ); }
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    std::vector<uint32_t> todo;
    for (uint32_t s : slots) {
        const HostImage& v = *c->imgs[s];
        if (v.n <= N) { c->budget_stats.n_views_whole += 1; continue; }       // whole: matched as registered, no copy and no kernel
        c->budget_stats.n_views_budgeted += 1;
        c->budget_stats.n_rows_selected += N;
        if (!((v.have & kLayBudget) && v.bud_N == N && v.bud_slot != kNone)) todo.push_back(s);
    }
    if (c->budget_stats.n_views_budgeted == 0) { c->budget_stats.ms_wall = now_ms() - t0; return R3DM_OK; }
    { const int rc = budget_events(c); if (rc != R3DM_OK) return rc; }
    if (!todo.empty()) { const int rc = build_subviews(c, todo, N); if (rc != R3DM_OK) return rc; }
    // the jobs' slots; with a classifier the two lists are dealt again: whether a pair goes through the arm's index is a property of the
    // view that is matched, which is now the sub-view
    auto sub_of = [&](uint32_t s) { const HostImage& v = *c->imgs[s]; return v.n > N ? v.bud_slot : s; };
    for (auto* v : {&indexed, &scanned}) for (PairJob& j : *v) { j.sI = sub_of(j.sI); j.sJ = sub_of(j.sJ); }
    if (classify) {
        std::vector<PairJob> all(indexed);
        all.insert(all.end(), scanned.begin(), scanned.end());
        std::sort(all.begin(), all.end(), [](const PairJob& x, const PairJob& y) { return x.I != y.I ? x.I < y.I : x.J < y.J; });
        indexed.clear(); scanned.clear();
        for (const PairJob& j : all) {
            bool index = false;
            const int rc = classify(*c->imgs[j.sI], index);
            if (rc != R3DM_OK) return rc;
            (index ? indexed : scanned).push_back(j);
        }
    }
    // the row lists by slot, for the remap of every batch of this call
    const size_t n_slots = c->imgs.size();
    R3DM_HIP(c, c->bud_pin.ensure(n_slots * sizeof(BudgetMap)));
    R3DM_HIP(c, c->bud_maps.ensure(n_slots * sizeof(BudgetMap)));
    BudgetMap* maps = c->bud_pin.as<BudgetMap>();
    for (size_t s = 0; s < n_slots; ++s) maps[s] = BudgetMap{nullptr, 0u};
    for (uint32_t s : slots) {
        const HostImage& v = *c->imgs[s];
        if (v.n > N) maps[v.bud_slot] = BudgetMap{v.bud_rows.as<uint32_t>(), N};
    }
    R3DM_HIP(c, hipMemcpyAsync(c->bud_maps.p, maps, n_slots * sizeof(BudgetMap), hipMemcpyHostToDevice, c->stream));
    c->bud_maps_live = true;
    c->budget_stats.ms_wall = now_ms() - t0;
    return R3DM_OK;
}

int budget_remap(r3dm_ctx* c, const std::vector<PairJob>& jobs, const uint32_t* pair_cnt_host, const uint64_t* pair_off_dev,
                 const uint32_t* pair_cnt_dev, r3dm_match* matches_dev)
{
    if (!c->bud_maps_live) return R3DM_OK;
    const double t0 = now_ms();
    uint64_t remapped = 0;
    for (size_t p = 0; p < jobs.size(); ++p) {
        const PairJob& j = jobs[p];
        if (c->imgs[j.sI]->live && c->imgs[j.sJ]->live) continue;          // both views whole
        remapped += pair_cnt_host[p];
    }
    if (remapped == 0) return R3DM_OK;
    BudgetRemapParams P{};
    P.maps = c->bud_maps.as<BudgetMap>(); P.pairs = c->d_pairs.as<uint2>();
    P.pair_off = pair_off_dev; P.pair_cnt = pair_cnt_dev; P.matches = matches_dev;
    R3DM_HIP(c, hipEventRecord(c->bud_ev[0], c->stream));
    R3DM_HIP(c, launch_budget_remap(c->stream, P, (uint32_t)jobs.size()));
    R3DM_HIP(c, hipEventRecord(c->bud_ev[1], c->stream));
    R3DM_HIP(c, hipEventSynchronize(c->bud_ev[1]));
    c->budget_stats.ms_remap += budget_elapsed(c);
    c->budget_stats.n_matches_remapped += remapped;
    c->budget_stats.ms_wall += now_ms() - t0;
    return R3DM_OK;
}

extern "C" int r3dm_set_match_budget(r3dm_ctx* c, int enable, uint32_t max_rows)
{
    if (!c) return R3DM_ERR_INVALID;
    if (max_rows < kBudgetMin) { c->err = "match budget: max_rows >= 2"; return R3DM_ERR_INVALID; }
    c->budget_on = (enable != 0); c->budget_N = max_rows;
    return R3DM_OK;
}

extern "C" int r3dm_budget_report(const r3dm_ctx* c, r3dm_budget_stats* out)
{
    if (!c || !out) return R3DM_ERR_INVALID;
    *out = c->budget_stats;
    return R3DM_OK;
}

static int r3dm_budget_rows_impl(r3dm_ctx* c, uint32_t view_id, uint32_t max_rows, uint32_t* rows_out, uint32_t* n_out)
{
    if (!c || !n_out) return R3DM_ERR_INVALID;
    if (max_rows < kBudgetMin) { c->err = "match budget: max_rows >= 2"; return R3DM_ERR_INVALID; }
    auto it = c->slot_of.find(view_id);
    if (it == c->slot_of.end()) { c->err = "unregistered view"; return R3DM_ERR_INVALID; }
    const HostImage& v = *c->imgs[it->second];
    const uint32_t hn = std::min(max_rows, v.n);
    if (hn && !rows_out) return R3DM_ERR_INVALID;
    R3DM_HIP(c, hipSetDevice(c->device));
    c->budget_stats = r3dm_budget_stats{};
    const double t0 = now_ms();
    *n_out = hn;
    if (v.n <= max_rows) {                                // whole: no kernel
        for (uint32_t k = 0; k < hn; ++k) rows_out[k] = k;
        c->budget_stats.n_views_whole = 1;
    } else {
        { const int rc = budget_events(c); if (rc != R3DM_OK) return rc; }
        R3DM_HIP(c, c->bud_sel.ensure((size_t)hn * 4));
        { const int rc = select_rows(c, {it->second}, max_rows, {c->bud_sel.as<uint32_t>()}); if (rc != R3DM_OK) return rc; }
        R3DM_HIP(c, c->pin_small.ensure((size_t)hn * 4));
        R3DM_HIP(c, hipMemcpyAsync(c->pin_small.p, c->bud_sel.p, (size_t)hn * 4, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(rows_out, c->pin_small.p, (size_t)hn * 4);
        c->budget_stats.ms_select = budget_elapsed(c);
        c->budget_stats.n_views_budgeted = 1;
        c->budget_stats.n_rows_selected = hn;
    }
    c->budget_stats.ms_wall = now_ms() - t0;
    return R3DM_OK;
}

extern "C" int r3dm_budget_rows(r3dm_ctx* c, uint32_t view_id, uint32_t max_rows, uint32_t* rows_out, uint32_t* n_out)
{
    return r3dm_guarded(c, [&]() -> int { return r3dm_budget_rows_impl(c, view_id, max_rows, rows_out, n_out); });
}
