// api_tracks.cpp -- part of the host side of libr3dm.so: feature tracks of a match graph (r3dm_build_tracks and the accessors of an
// r3dm_tracks; the contract is the comment of those entries in include/r3dm.h, the kernels are kernels_tracks.hip).
//
// What the host does: rank the distinct view ids of the pair list (P entries, small), turn the per-view extents the device found into
// slot bases, size the buffers, and read three counts back between the phases (extents; nodes; observations and tracks) because they
// size what follows.  Everything that touches a match or a node runs on the device.  There is no CPU fallback: when HIP fails, the
// call fails.
#include "r3dm_ctx.hpp"

struct r3dm_tracks {
    std::vector<uint64_t> offsets;             // n_tracks + 1
    std::vector<r3dm_observation> obs;
    r3dm_tracks_stats stats{};
    double phase_ms[4] = {0, 0, 0, 0};         // r3dm_tracks_phase_ms
};

namespace {

// the scratch words of a selection / a sort over n elements, in the context's (grown) work buffer
int scratch_for(r3dm_ctx* c, uint64_t n, bool sort, uint32_t** out)
{
    R3DM_HIP(c, c->tb.temp.ensure(tracks_scratch_words(n, sort) * 4));
    *out = c->tb.temp.as<uint32_t>();
    return R3DM_OK;
}

// On every exit of a call the work buffers larger than kTracksKeepBytes go back to the device: a graph with sparse feature indices near
// R3DM_TRACKS_MAX_SLOTS needs 11 bytes per slot (3 GB), which a context must not sit on until r3dm_destroy.  Smaller buffers stay
// for the next call.
constexpr size_t kTracksKeepBytes = (size_t)64 << 20;
struct TrimTracksBufs {
    r3dm_ctx* c;
    ~TrimTracksBufs()
    {
        TracksBufs& B = c->tb;
        DevBuf* b[] = {&B.matches, &B.offsets, &B.pair_rank, &B.par, &B.slots, &B.ma, &B.rel, &B.keep, &B.pair_kept, &B.nodes, &B.keys, &B.skey,
                       &B.sval, &B.nodeflag, &B.oslots, &B.obs, &B.hflag, &B.toff, &B.kept_rel, &B.temp};
        bool any = false;
        for (DevBuf* x : b) any = any || x->cap > kTracksKeepBytes;
        if (!any) return;
        (void)hipStreamSynchronize(c->stream);
        for (DevBuf* x : b) if (x->cap > kTracksKeepBytes) x->release();
    }
};

int build_tracks_impl(r3dm_ctx* c, const r3dm_graph* g, uint32_t min_length, r3dm_tracks** out, r3dm_graph** kept_out)
{
    const double t_call = now_ms();
    const uint64_t P64 = g->pairs.size() / 2, M = g->matches.size();
    if (P64 >= 0xFFFFFFFFull || M >= 0xFFFFFFFFull) { c->err = "r3dm_build_tracks: 2^32 - 1 pairs or matches, or more"; return R3DM_ERR_UNSUPPORTED; }
    const uint32_t P = (uint32_t)P64;
    auto t = std::unique_ptr<r3dm_tracks>(new r3dm_tracks());
    t->offsets.push_back(0);
    t->stats.n_matches = M;
    std::unique_ptr<r3dm_graph> kg;
    if (kept_out) { kg.reset(new r3dm_graph()); kg->offsets.push_back(0); }
    auto deliver = [&]() {
        t->stats.ms_wall = now_ms() - t_call;
        *out = t.release();
        if (kept_out) *kept_out = kg.release();
        return R3DM_OK;
    };
    if (M == 0) {                                              // an empty graph: zero tracks, nothing launched
        if (kept_out) { GraphBuilder b(c, kg.get(), c->device_graphs, nullptr, nullptr, nullptr, nullptr); b.done(); }
        return deliver();
    }

    R3DM_HIP(c, hipSetDevice(c->device));
    TrimTracksBufs trim{c};
    TracksBufs& B = c->tb;
    for (hipEvent_t& e : B.ev) if (!e) R3DM_HIP(c, hipEventCreate(&e));
    hipStream_t st = c->stream;

    // the distinct view ids, ascending, and the rank of both views of every pair
    std::vector<uint32_t> ids(g->pairs);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const uint32_t V = (uint32_t)ids.size();
    std::vector<uint32_t> rank(2 * (size_t)P);
    for (size_t k = 0; k < rank.size(); ++k) rank[k] = (uint32_t)(std::lower_bound(ids.begin(), ids.end(), g->pairs[k]) - ids.begin());

    // the graph: read where it is when its mirror lives on this device, uploaded otherwise
    const bool mirrored = g->dev.valid && g->dev.device == c->device && g->dev.P == P64 && g->dev.M == M;
    TrkParams T{};
    T.P = P; T.V = V; T.M = M; T.min_length = min_length;
    if (mirrored) T.matches = g->dev.matches.as<r3dm_match>();
    else {
        R3DM_HIP(c, B.matches.ensure(M * sizeof(r3dm_match)));
        R3DM_HIP(c, hipMemcpyAsync(B.matches.p, g->matches.data(), M * sizeof(r3dm_match), hipMemcpyHostToDevice, st));
        T.matches = B.matches.as<r3dm_match>();
    }
    R3DM_HIP(c, B.offsets.ensure(((size_t)P + 1) * 8));
    R3DM_HIP(c, B.pair_rank.ensure((size_t)P * 8));
    R3DM_HIP(c, B.view_ids.ensure((size_t)V * 4));
    R3DM_HIP(c, B.base.ensure(((size_t)V + 1) * 4));
    R3DM_HIP(c, B.smax.ensure((size_t)V * 4));
    R3DM_HIP(c, B.ctr.ensure(16 * 8));
    R3DM_HIP(c, B.pin.ensure(256 + (size_t)V * 4));
    R3DM_HIP(c, hipMemcpyAsync(B.offsets.p, g->offsets.data(), ((size_t)P + 1) * 8, hipMemcpyHostToDevice, st));
    R3DM_HIP(c, hipMemcpyAsync(B.pair_rank.p, rank.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));
    R3DM_HIP(c, hipMemcpyAsync(B.view_ids.p, ids.data(), (size_t)V * 4, hipMemcpyHostToDevice, st));
    R3DM_HIP(c, hipMemsetAsync(B.smax.p, 0, (size_t)V * 4, st));
    R3DM_HIP(c, hipMemsetAsync(B.ctr.p, 0, 16 * 8, st));
    T.offsets = B.offsets.as<uint64_t>(); T.pair_rank = B.pair_rank.as<uint32_t>(); T.view_ids = B.view_ids.as<uint32_t>();
    T.base = B.base.as<uint32_t>(); T.smax = B.smax.as<uint32_t>();
    T.ctr = B.ctr.as<unsigned long long>();
    unsigned long long* const sel = T.ctr + 8;                 // [0] nodes, [1] observations, [2] tracks, [3] kept matches: the selections' counts
    unsigned char* const pin = static_cast<unsigned char*>(B.pin.p);

    // ---- phase 1: the extent of every view -> slot bases
    R3DM_HIP(c, hipEventRecord(B.ev[0], st));
    R3DM_HIP(c, launch_tracks(st, T, TrkStep::kExtent));
    R3DM_HIP(c, hipEventRecord(B.ev[1], st));
    R3DM_HIP(c, hipMemcpyAsync(pin + 256, B.smax.p, (size_t)V * 4, hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipStreamSynchronize(st));
    std::vector<uint32_t> base((size_t)V + 1);
    {
        const uint32_t* smax = reinterpret_cast<const uint32_t*>(pin + 256);
        uint64_t total = 0;
        for (uint32_t v = 0; v < V; ++v) {
            base[v] = (uint32_t)total;                         // (total <= the limit so far)
            total += (uint64_t)smax[v] + 1;
            if (total > R3DM_TRACKS_MAX_SLOTS) {
                c->err = "r3dm_build_tracks: the views' feature indices span more than R3DM_TRACKS_MAX_SLOTS slots";
                return R3DM_ERR_UNSUPPORTED;
            }
        }
        base[V] = (uint32_t)total;
    }
    const uint32_t N = base[V];
    T.N = N;
    R3DM_HIP(c, hipMemcpyAsync(B.base.p, base.data(), ((size_t)V + 1) * 4, hipMemcpyHostToDevice, st));

    // ---- phase 2: components
    const uint64_t nodes_cap = std::min<uint64_t>(N, 2 * M);
    R3DM_HIP(c, B.par.ensure((size_t)N * 4));
    R3DM_HIP(c, B.slots.ensure((size_t)N * 7));
    R3DM_HIP(c, B.ma.ensure(M * 4));
    R3DM_HIP(c, B.rel.ensure(M * 4));
    R3DM_HIP(c, B.keep.ensure(M));
    R3DM_HIP(c, B.pair_kept.ensure((size_t)P * 4));
    R3DM_HIP(c, B.nodes.ensure(nodes_cap * 4));
    T.par = B.par.as<uint32_t>();
    T.csz = B.slots.as<uint32_t>();
    T.touched = B.slots.as<uint8_t>() + (size_t)N * 4; T.conf = T.touched + N; T.surv = T.conf + N;
    T.ma = B.ma.as<uint32_t>(); T.rel = B.rel.as<uint32_t>(); T.keep = B.keep.as<uint8_t>(); T.pair_kept = B.pair_kept.as<uint32_t>();
    T.nodes = B.nodes.as<uint32_t>();
    R3DM_HIP(c, hipMemsetAsync(B.slots.p, 0, (size_t)N * 7, st));
    R3DM_HIP(c, hipMemsetAsync(B.pair_kept.p, 0, (size_t)P * 4, st));
    R3DM_HIP(c, hipEventRecord(B.ev[2], st));
    R3DM_HIP(c, launch_tracks(st, T, TrkStep::kInit));
    R3DM_HIP(c, launch_tracks(st, T, TrkStep::kLink));
    R3DM_HIP(c, launch_tracks(st, T, TrkStep::kFlatten));
    uint32_t* scratch = nullptr;
    int rc = scratch_for(c, N, false, &scratch);
    if (rc != R3DM_OK) return rc;
    R3DM_HIP(c, tracks_select(st, scratch, T.touched, N, nullptr, T.nodes, sel + 0));
    R3DM_HIP(c, hipEventRecord(B.ev[3], st));
    R3DM_HIP(c, hipMemcpyAsync(pin, sel, 8, hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipStreamSynchronize(st));
    uint64_t n_nodes = 0;
    memcpy(&n_nodes, pin, 8);
    if (n_nodes == 0 || n_nodes > nodes_cap) { c->err = "r3dm_build_tracks: node count out of range"; return R3DM_ERR_HIP; }
    T.n_nodes = n_nodes;

    // ---- phase 3: components in root order, members ascending; conflicts; the filter
    R3DM_HIP(c, B.keys.ensure(n_nodes * 4));
    R3DM_HIP(c, B.skey.ensure(n_nodes * 4));
    R3DM_HIP(c, B.sval.ensure(n_nodes * 4));
    R3DM_HIP(c, B.nodeflag.ensure(n_nodes));
    R3DM_HIP(c, B.oslots.ensure(n_nodes * 4));
    T.keys = B.keys.as<uint32_t>(); T.skey = B.skey.as<uint32_t>(); T.sval = B.sval.as<uint32_t>();
    T.nodeflag = B.nodeflag.as<uint8_t>(); T.oslots = B.oslots.as<uint32_t>();
    uint32_t bits = 1;
    while (bits < 32 && (1ull << bits) < N) ++bits;            // roots are slots < N
    R3DM_HIP(c, hipEventRecord(B.ev[4], st));
    R3DM_HIP(c, launch_tracks(st, T, TrkStep::kKeys));
    if ((rc = scratch_for(c, n_nodes, true, &scratch)) != R3DM_OK) return rc;
    bool in_second = false;
    R3DM_HIP(c, tracks_sort_by_root(st, scratch, T.keys, T.nodes, T.skey, T.sval, n_nodes, bits, &in_second));
    if (!in_second) { std::swap(T.keys, T.skey); std::swap(T.nodes, T.sval); }       // (the unsorted arrays are not read again)
    R3DM_HIP(c, launch_tracks(st, T, TrkStep::kMark));
    R3DM_HIP(c, launch_tracks(st, T, TrkStep::kClassify));
    R3DM_HIP(c, tracks_select(st, scratch, T.nodeflag, n_nodes, T.sval, T.oslots, sel + 1));
    R3DM_HIP(c, hipEventRecord(B.ev[5], st));
    R3DM_HIP(c, hipMemcpyAsync(pin, T.ctr, 16 * 8, hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipStreamSynchronize(st));
    uint64_t h[16];
    memcpy(h, pin, sizeof h);
    const uint64_t n_tracks = h[3], n_obs = h[9];
    if (n_obs > n_nodes || n_tracks > n_obs) { c->err = "r3dm_build_tracks: observation count out of range"; return R3DM_ERR_HIP; }
    T.n_obs = n_obs;

    // ---- phase 4: the observations, the track offsets, the kept matches
    R3DM_HIP(c, B.obs.ensure(n_obs * sizeof(r3dm_observation)));
    R3DM_HIP(c, B.hflag.ensure(n_obs));
    R3DM_HIP(c, B.toff.ensure(n_tracks * 8));
    if (kept_out) R3DM_HIP(c, B.kept_rel.ensure(M * 4));
    T.obs = B.obs.as<r3dm_observation>(); T.hflag = B.hflag.as<uint8_t>();
    R3DM_HIP(c, hipEventRecord(B.ev[6], st));
    if (n_obs) {
        R3DM_HIP(c, launch_tracks(st, T, TrkStep::kEmit));
        R3DM_HIP(c, tracks_select64(st, scratch, T.hflag, n_obs, B.toff.as<uint64_t>(), sel + 2));
    }
    R3DM_HIP(c, launch_tracks(st, T, TrkStep::kKeep));
    if (kept_out) {
        if ((rc = scratch_for(c, M, false, &scratch)) != R3DM_OK) return rc;
        R3DM_HIP(c, tracks_select(st, scratch, T.keep, M, T.rel, B.kept_rel.as<uint32_t>(), sel + 3));
    }
    R3DM_HIP(c, hipEventRecord(B.ev[7], st));
    t->obs.resize(n_obs);
    t->offsets.assign(n_tracks + 1, n_obs);
    if (n_obs) {
        R3DM_HIP(c, hipMemcpyAsync(t->obs.data(), B.obs.p, n_obs * sizeof(r3dm_observation), hipMemcpyDeviceToHost, st));
        R3DM_HIP(c, hipMemcpyAsync(t->offsets.data(), B.toff.p, n_tracks * 8, hipMemcpyDeviceToHost, st));
    }
    R3DM_HIP(c, hipMemcpyAsync(pin, T.ctr, 16 * 8, hipMemcpyDeviceToHost, st));
    R3DM_HIP(c, hipStreamSynchronize(st));
    memcpy(h, pin, sizeof h);
    if ((n_obs && h[10] != n_tracks) || (kept_out && h[11] != h[4])) { c->err = "r3dm_build_tracks: the selections disagree with the counters"; return R3DM_ERR_HIP; }
    r3dm_tracks_stats& S = t->stats;
    S.n_nodes = n_nodes; S.n_components = h[0]; S.n_conflicting = h[1]; S.n_short = h[2]; S.n_tracks = n_tracks; S.n_observations = n_obs;
    S.n_matches_kept = h[4]; S.longest = (uint32_t)h[5]; S.largest_component = (uint32_t)h[6];
    for (int k = 0; k < 4; ++k) {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, B.ev[2 * k], B.ev[2 * k + 1]);
        S.ms_kernels += ms;
        t->phase_ms[k] = ms;
    }

    // ---- the track filter applied to the graph: per-pair index lists into the matches, gathered like the geometric filters' inliers
    if (kept_out) {
        const uint64_t n_kept = h[4];
        std::vector<uint32_t> h_rel(n_kept), h_cnt(P);
        if (n_kept) R3DM_HIP(c, hipMemcpyAsync(h_rel.data(), B.kept_rel.p, n_kept * 4, hipMemcpyDeviceToHost, st));
        R3DM_HIP(c, hipMemcpyAsync(h_cnt.data(), B.pair_kept.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
        R3DM_HIP(c, hipStreamSynchronize(st));
        kg->matches.reserve(n_kept);
        GraphBuilder b(c, kg.get(), c->device_graphs, g->matches.data(), h_rel.data(), T.matches, B.kept_rel.as<uint32_t>());
        uint64_t at = 0;
        for (uint32_t p = 0; p < P; ++p) {
            if (h_cnt[p] == 0) continue;                       // no empty entries
            b.add(g->pairs[2 * (size_t)p], g->pairs[2 * (size_t)p + 1], g->offsets[p], at, h_cnt[p]);
            at += h_cnt[p];
        }
        b.done();
    }
    return deliver();
}

}  // namespace

extern "C" int r3dm_build_tracks(r3dm_ctx* c, const r3dm_graph* g, uint32_t min_length, r3dm_tracks** out, r3dm_graph** kept_out)
{
    if (out) *out = nullptr;
    if (kept_out) *kept_out = nullptr;
    if (!c || !g || !out) return R3DM_ERR_INVALID;
    if (min_length < 2) { c->err = "r3dm_build_tracks: min_length < 2"; return R3DM_ERR_INVALID; }
    return r3dm_guarded(c, [&]() -> int { return build_tracks_impl(c, g, min_length, out, kept_out); });
}

extern "C" uint64_t r3dm_tracks_count(const r3dm_tracks* t) { return t ? t->offsets.size() - 1 : 0; }
extern "C" const uint64_t* r3dm_tracks_offsets(const r3dm_tracks* t) { return t ? t->offsets.data() : nullptr; }
extern "C" const r3dm_observation* r3dm_tracks_observations(const r3dm_tracks* t) { return t ? t->obs.data() : nullptr; }
extern "C" void r3dm_tracks_free(r3dm_tracks* t) { delete t; }

extern "C" int r3dm_tracks_report(const r3dm_tracks* t, r3dm_tracks_stats* out)
{
    if (!t || !out) return R3DM_ERR_INVALID;
    *out = t->stats;
    return R3DM_OK;
}

extern "C" int r3dm_tracks_phase_ms(const r3dm_tracks* t, double* out4)
{
    if (!t || !out4) return R3DM_ERR_INVALID;
    for (int k = 0; k < 4; ++k) out4[k] = t->phase_ms[k];
    return R3DM_OK;
}

extern "C" int r3dm_tracks_in_pair(const r3dm_tracks* t, uint32_t view_a, uint32_t view_b, r3dm_match* out, uint64_t cap, uint64_t* n_out)
{
    if (n_out) *n_out = 0;
    if (!t || !n_out || view_a == view_b || (cap && !out)) return R3DM_ERR_INVALID;
    uint64_t n = 0;
    const r3dm_observation* obs = t->obs.data();
    auto by_view = [](const r3dm_observation& o, uint32_t v) { return o.view < v; };
    for (size_t k = 0; k + 1 < t->offsets.size(); ++k) {       // a track's observations are sorted by view, one per view
        const r3dm_observation* b = obs + t->offsets[k];
        const r3dm_observation* e = obs + t->offsets[k + 1];
        const r3dm_observation* pa = std::lower_bound(b, e, view_a, by_view);
        if (pa == e || pa->view != view_a) continue;
        const r3dm_observation* pb = std::lower_bound(b, e, view_b, by_view);
        if (pb == e || pb->view != view_b) continue;
        if (n < cap) { out[n].i = pa->feature; out[n].j = pb->feature; }
        ++n;
    }
    *n_out = n;
    return R3DM_OK;
}
