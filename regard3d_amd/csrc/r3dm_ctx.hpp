// r3dm_ctx.hpp -- host-side state shared by the translation units of libr3dm.so (not part of the public ABI).
//   api_core.cpp      context, views (staging), match-graph objects, matches.* files
//   api_match.cpp     exhaustive putative matching: 2-NN batches (run_match_batch), k-NN (run_knn_batch), the mutual check in front of
//                     every finalisation into a graph (finalize_batch), one certificate slack
//                     (cert_slack_factor), one index mount (mount_index_beside_queries), one k <= 2 detour (knn_by_knn2)
//   api_preselect.cpp preemptive matching: view priorities, heads, the gate behind resolve_pairs, r3dm_preselect_pairs
//   api_budget.cpp    the match budget: device selection of a view's rows, sub-view slots, the substitution behind the gate, the remap
//   api_vocab.cpp     pair proposal: vocabularies and their training, view signatures through the exhaustive matcher, scores, top-k selection
//   api_ann.cpp       what the approximate matchers share -- pair resolution (resolve_pairs, also the exhaustive matcher's), the collection
//                     call (match_collection_ann), the search batch (run_ann_batch) -- and the graph matcher (KGraph arms 0-4)
//   api_hnsw.cpp, api_mrpt.cpp   the HNSW arms 6-8 and the MRPT arm 5 on those frames: index build, search launch, their rules
//   api_filter.cpp    AC-RANSAC geometric filters (F, E, H); their kernels: filter_device.hpp (shared device routines), filter_acransac.inc
//                     (one workgroup per pair; kernels_filter.hip F / H, kernels_filter_e.hip E), kernels_filter_coop.hip (long pairs)
//   api_tracks.cpp    feature tracks of a match graph (r3dm_build_tracks), the track filter applied to the graph, r3dm_tracks_in_pair
//   api_akaze.cpp     the frame of both detector arms (checks, upload, INTER_AREA tables, statistics tail, DetectedBatch's writer) and the
//                     Fast-A-KAZE arm: its pass in phases, the one pass of the level-plane descriptors (ak_describe_pass: MLDB, M-SURF-64)
//                     and their one entry, r3dm_detect_akaze / _mldb / _mldb_batch / _msurf / _msurf_batch / _batch,
//                     r3dm_gray_from_bgr8
//   api_akaze_classic.cpp   the classic A-KAZE arm's launch sequence on that frame, r3dm_detect_akaze_classic / _batch
//   descriptor_arms.hpp     the one table of the descriptor arms (host only): id, names, regions type, row bytes, level table
//   api_liop.cpp      LIOP: the patch geometry, the one pass from keypoints to descriptors (liop_pass), its two entries
//   api_features.cpp  the features work item: .feat / .desc files, the features batch in phases (detect, keypoints and maps, LIOP pass,
//                     delivery, outputs), the work list of a multi-context, the setters
#pragma once

#include "r3dm_internal.hpp"
#include "descriptor_arms.hpp"

#include <sched.h>
#include <sys/resource.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

using namespace r3dm;

struct r3dm_index;

// ------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------

// How many host threads a helper team of this library may start: the cores this process may actually use -- the affinity mask AND the
// cgroup CPU quota (a container with `cpu.max = 1600000 100000` sees 256 processors and owns 16: a burst of more runnable threads than
// that is throttled until the end of the 100 ms period, which showed as random 60-100 ms stalls of the stage's main thread) -- divided
// among the workers that may run such a team at the same time, at most `want`.
// called first thing by the library's background writer threads (feature files, match files): their work has a whole phase of the
// caller's to hide behind, so under contention for the host's cores they stand back (Linux: a per-thread nice value, inherited
// by the OpenMP helpers they start)
// (only when the host asked for it -- r3dm_set_background_nice, R3DComputeMatches::setBackgroundThreadsNice: a library does not
// change thread priorities on its own)
inline void r3dm_background_thread(int nice_value)
{
    if (nice_value > 0) (void)setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), nice_value);
}

// fn(i) for i in [0, n) on up to `threads` host threads that EXIT when the work is done.  (An OpenMP team keeps spinning for
// work for milliseconds after every region -- libgomp sizes that spin by the CPUs it can see, not by the cgroup quota the process
// lives under -- and several such teams at once ran a 16-core quota dry: CFS then stalls the whole process for the rest of its
// period.  These regions are a few milliseconds long and few; six thread starts per region cost less than that.)
// fn must not throw.
template <class F>
inline void r3dm_parallel_for(long n, int threads, F&& fn)
{
    if (n <= 0) return;
    if (threads > n) threads = (int)n;
    if (threads <= 1) { for (long i = 0; i < n; ++i) fn(i); return; }
    std::atomic<long> next{0};
    auto worker = [&]() { for (;;) { const long i = next.fetch_add(1, std::memory_order_relaxed); if (i >= n) break; fn(i); } };
    std::vector<std::thread> th;
    th.reserve((size_t)threads - 1);
    try { for (int t = 1; t < threads; ++t) th.emplace_back(worker); } catch (...) {}      // fewer helpers: the work is still done
    worker();
    for (std::thread& t : th) t.join();
}

inline int r3dm_host_team(int want, int concurrent_teams = 2)
{
    static const int cores = [] {
        int n = (int)std::thread::hardware_concurrency();
        if (n < 1) n = 1;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int a = CPU_COUNT(&set); if (a >= 1 && a < n) n = a; }
        for (const char* path : {"/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"}) {
            if (FILE* f = fopen(path, "r")) {
                char a[64] = {0}, b[64] = {0};
                const int got = fscanf(f, "%63s %63s", a, b);
                fclose(f);
                if (got >= 1 && a[0] >= '0' && a[0] <= '9') {
                    double quota = atof(a), period = got >= 2 ? atof(b) : 100000.0;
                    if (got < 2) if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%63s", b) == 1) period = atof(b); fclose(g); }
                    if (quota > 0 && period > 0) { const int q = (int)(quota / period); if (q >= 1 && q < n) n = q; }
                }
                break;
            }
        }
        return n;
    }();
    int t = (cores - 4) / (concurrent_teams > 0 ? concurrent_teams : 1);       // four cores stay free for the main thread, writers and the runtime's own threads
    if (t > want) t = want;
    return t < 1 ? 1 : t;
}

// Device memory of the views of a context: blocks cut from large slabs instead of one hipMalloc per buffer.  A view of 8,192 x 128
// floats is a 4 MiB tile image + 32 KiB of slack + three small arrays: hipMalloc rounds each of them up to its page size (the tile
// image alone occupied 6 MiB), which made a registered collection 1.5 x its own bytes; cut from 64 MiB slabs at 256-byte granularity
// it is 1.05 x.  Blocks freed by a view (replaced, trimmed) go to a free list and serve later requests of at most 1.25 x their size; a
// slab whose blocks are all free goes back to the device.  Not thread-safe: a context is used by one thread at a time.
struct DevArena {
    struct Slab { unsigned char* p = nullptr; size_t cap = 0, used = 0; uint32_t live = 0; };
    std::vector<Slab> slabs;
    std::multimap<size_t, std::pair<uint32_t, size_t>> free_blocks;       // size -> (slab, offset)
    int bump[2] = {-1, -1};                                               // the slabs new blocks are cut from: the newest and the one before
    static constexpr size_t kSlab = (size_t)64 << 20, kAlign = 256;
    hipError_t alloc(size_t bytes, void** out, size_t* got)
    {
        bytes = (bytes + kAlign - 1) / kAlign * kAlign;
        auto it = free_blocks.lower_bound(bytes);
        if (it != free_blocks.end() && it->first <= bytes + bytes / 4) {
            const auto blk = it->second;
            *out = slabs[blk.first].p + blk.second; *got = it->first;
            slabs[blk.first].live += 1;
            free_blocks.erase(it);
            return hipSuccess;
        }
        for (int b : bump) {                                                     // the two newest slabs are bumped
            if (b < 0 || (size_t)b >= slabs.size()) continue;
            Slab& sl = slabs[(size_t)b];
            if (sl.p && sl.cap - sl.used >= bytes) { *out = sl.p + sl.used; *got = bytes; sl.used += bytes; sl.live += 1; return hipSuccess; }
        }
        Slab sl;
        sl.cap = std::max(kSlab, bytes);
        hipError_t e = hipMalloc((void**)&sl.p, sl.cap);
        if (e != hipSuccess) return e;
        sl.used = bytes; sl.live = 1;
        *out = sl.p; *got = bytes;
        uint32_t at = (uint32_t)slabs.size();
        for (uint32_t k = 0; k < slabs.size(); ++k) if (!slabs[k].p) { at = k; break; }      // reuse a dead entry: indices in free_blocks stay valid
        bump[1] = bump[0]; bump[0] = (int)at;
        if (at == slabs.size()) slabs.push_back(sl); else slabs[at] = sl;
        return hipSuccess;
    }
    void free(void* p, size_t bytes)
    {
        unsigned char* q = static_cast<unsigned char*>(p);
        for (uint32_t k = 0; k < slabs.size(); ++k) {
            Slab& sl = slabs[k];
            if (!sl.p || q < sl.p || q >= sl.p + sl.cap) continue;
            sl.live -= 1;
            if (sl.live == 0) {
                for (auto it = free_blocks.begin(); it != free_blocks.end();) it = it->second.first == k ? free_blocks.erase(it) : std::next(it);
                (void)hipFree(sl.p);
                sl = Slab();
            } else free_blocks.insert({bytes, {k, (size_t)(q - sl.p)}});
            return;
        }
    }
    size_t bytes_held() const { size_t b = 0; for (const Slab& sl : slabs) b += sl.p ? sl.cap : 0; return b; }
    void release_all() { for (Slab& sl : slabs) if (sl.p) (void)hipFree(sl.p); slabs.clear(); free_blocks.clear(); bump[0] = bump[1] = -1; }
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevArena* arena = nullptr;        // set: the buffer is a block of this arena (per-view layouts of a context), else its own hipMalloc
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        if (arena) {
            hipError_t e = arena->alloc(bytes, &p, &cap);
            if (e != hipSuccess) { p = nullptr; cap = 0; }
            return e;
        }
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) { if (arena) arena->free(p, cap); else (void)hipFree(p); }
        p = nullptr; cap = 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// page-locked host memory (device-to-host copies into it run at link speed and are truly asynchronous)
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Layouts of a view beyond the ones every view holds from registration on (float views: fragment-order f32 tiles + norms + statistics;
// binary views: padded word rows): staged on FIRST USE by the path that reads them (api_core.cpp: ensure_layouts), or at registration
// when the path's flag (r3dm_set_integer_mfma / _split_mfma / _hamming_mfma) is already on.
enum : uint32_t {
    kLayRows   = 1u,     // row-major f32 rows: exact re-scoring of real-valued pairs, the generic exact scan, the approximate matchers
    kLayBf16   = 2u,     // bf16 tiles (r3dm_set_integer_mfma)
    kLaySplit  = 4u,     // split-f16 planes (r3dm_set_split_mfma)
    kLayCounts = 8u,     // count tiles + scale order (r3dm_set_split_mfma, rows = integer votes x a row scale); needs kLayRows
    kLayBin8   = 16u,    // one byte per bit in i8 fragment order (r3dm_set_hamming_mfma)
    kLayHead   = 32u,    // the head rows of preemptive matching, row-major (api_preselect.cpp: ensure_heads, not ensure_layouts)
    kLayBudget = 64u,    // the sub-view of the match budget: row list + a slot of its own (api_budget.cpp: budget_substitute)
};

// the count tiles exist only for f32 views of at most 256 dimensions (anything else is never votes x scale: counts_ok stays false)
inline bool counts_eligible(r3dm_dtype dtype, uint32_t n, uint32_t dim) { return dtype == R3DM_F32 && n && dim <= 256; }
// the split planes and the count tiles are made from the row-major rows, and the nominees of both are re-scored on them
inline uint32_t with_implied_rows(uint32_t want) { return (want & (kLaySplit | kLayCounts)) ? want | kLayRows : want; }

// The tenant of a slot: the view staged into it, its statistics, and which layouts and indices reflect it
struct ViewState {
    uint32_t view_id = 0, n = 0, dim = 0, width = 0, height = 0;
    r3dm_dtype dtype = R3DM_F32;
    uint32_t G = 0, n_tiles = 0, words = 0;
    bool has_xy = false, has_dup = false, live = false;
    uint32_t have = 0;                // kLay* bits: which on-demand layouts reflect the staged view
    // staging statistics: accumulated by the staging kernel in the view's table entry, read back -- for all views staged since the last
    // read -- by sync_view_stats() at the first call that needs them (no per-view synchronisation at registration)
    bool stats_valid = false;
    uint32_t stat_bits[3] = {0, 0, 1};                                      // ImgDev::max_norm_bits, max_abs_bits, not_integer
    float max_abs = 0.0f; bool not_integer = true, has_negative = true;
    int32_t split_k = 0;                                                    // scale exponent of the f16 split tiles (a function of max_abs)
    bool counts_ok = false;                                                 // every row is small integers x a row scale: the count tiles are valid
    bool compact_ready = false;       // ann_rows16 / ann_rows8 reflect the staged rows
    uint32_t ann_K = 0;               // graph index (r3dm_match_pairs_kgraph) in ann_adj / ann_deg
    uint32_t hnsw_M = 0, hnsw_seed = 0, hnsw_up_rows = 0; int32_t hnsw_enter = -1, hnsw_maxlevel = -1;     // HNSW index, valid when hnsw_M != 0
    uint32_t mrpt_trees = 0, mrpt_depth = 0; float mrpt_density = 0.0f; uint64_t mrpt_seed = 0;          // MRPT index, valid when mrpt_trees != 0
    std::vector<float> priority;      // r3dm_set_view_priority: one per row, or empty
    uint32_t head_h = 0, head_n = 0;  // kLayHead: the head size the head buffer was made for, and its rows (min(head_h, n))
    uint32_t bud_N = 0;               // kLayBudget: the budget the sub-view was made for
    uint64_t serial = 0;              // this registration's number, unique in the process (new_tenant); 0: no tenant.  Keys what outlives
                                      // a registration outside the context: the signatures of an r3dm_vocab (api_vocab.cpp)
};
inline std::atomic<uint64_t> g_view_serial{0};

// A slot of a context's view table.  What survives which transition:
//   ViewState        the tenant: replaced as a whole when a view is staged into the slot (new_tenant) and reset when the collection is
//                    cleared (clear)
//   has_K, Kinv      the view's intrinsics (r3dm_set_intrinsics): survive a re-registration of the view, forgotten by clear()
//   index buffers    ann_*, hnsw_*, mrpt_*: survive a new tenant (a rebuild reuses them), given back by clear() (rebuilt per collection:
//                    a context that once held a 1000-view collection must not sit on their gigabytes)
//   bud_slot         the slot of the view's sub-view (match budget): survives a new tenant (the sub-view is remade there), forgotten by
//                    clear() -- the sub-view's slot is a slot of the table like any other and is cleared with it
//   layout buffers   rows .. canon: survive both (a cleared view is a spare whose buffers serve the next collection), freed by release()
//   borrowed, owner  a mounted r3dm_index (mount): the buffers are aliases of the index's, never freed here
struct HostImage : ViewState {
    bool borrowed = false;
    struct r3dm_index* owner = nullptr;   // (layouts staged on first use are added to the index, under its lock)
    DevBuf rows, tiled, tiled16, tiledh, tiledc, tiledp, cscale, cquad, cperm, tiled8, norms, bin, xy, canon, head, bud_rows;
    uint32_t bud_slot = 0xFFFFFFFFu;      // match budget: the slot that holds this view's sub-view (bud_rows: its row list), or none
    DevBuf ann_adj, ann_deg, ann_rows16, ann_rows8;   // graph index; compact row copies only for bf16- / u8-exact views
    DevBuf hnsw_l0, hnsw_up_off, hnsw_up;             // hnswlib's arrays (kernels_hnsw.hip: HnswView)
    DevBuf mrpt_R, mrpt_RT, mrpt_splits, mrpt_leaves, mrpt_lf;      // kernels_mrpt.hip: MrptView
    bool has_K = false;               // pinhole intrinsics, needed by the essential-matrix filter
    double Kinv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // the layout buffers of a view registered with a context are blocks of the context's arena (an r3dm_index owns plain allocations:
    // it outlives contexts)
    std::array<DevBuf*, 16> layout_bufs() { return {&rows, &tiled, &tiled16, &tiledh, &tiledc, &tiledp, &cscale, &cquad, &cperm, &tiled8, &norms, &bin, &xy, &canon, &head, &bud_rows}; }
    void use_arena(DevArena* a) { for (DevBuf* x : layout_bufs()) x->arena = a; }
    void new_tenant(uint32_t id, uint32_t n_, uint32_t dim_, r3dm_dtype dtype_, uint32_t width_, uint32_t height_, bool xy)
    {
        static_cast<ViewState&>(*this) = ViewState();
        view_id = id; n = n_; dim = dim_; dtype = dtype_; width = width_; height = height_; has_xy = xy; live = true;
        serial = g_view_serial.fetch_add(1, std::memory_order_relaxed) + 1;
    }
    void clear()
    {
        DevBuf* b[] = {&ann_adj, &ann_deg, &ann_rows16, &ann_rows8, &hnsw_l0, &hnsw_up_off, &hnsw_up, &mrpt_R, &mrpt_RT, &mrpt_splits, &mrpt_leaves, &mrpt_lf};
        for (DevBuf* x : b) x->release();
        static_cast<ViewState&>(*this) = ViewState();
        has_K = false; bud_slot = 0xFFFFFFFFu;
    }
    void release()
    {
        if (borrowed) { *this = HostImage(); return; }
        clear();
        for (DevBuf* x : layout_bufs()) x->release();
    }
    // this slot becomes (again) an alias of the index as it stands: the caller holds the index's lock
    inline void mount(struct r3dm_index* ix);
};

inline uint32_t kernel_G_for(uint32_t dim)
{
    const uint32_t g = (dim + 7) / 8;
    if (g <= 8) return 8;
    if (g <= 16) return 16;
    if (g <= 18) return 18;
    if (g <= 32) return 32;
    return g;               // no tensor kernel: exact scan only
}

// entries per pair of a match batch's nn_idx / 2-lists, for the longest query view of the batch (run_match_batch; api_vocab.cpp reads
// the 2-lists of its batches where the matcher left them)
inline uint32_t match_q_stride(uint32_t max_nJ) { return std::max<uint32_t>(32, (max_nJ + 31) / 32 * 32); }

inline uint32_t next_pow2(uint32_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; }

inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline bool has_ext(const char* path, const char* ext)
{
    const size_t lp = strlen(path), le = strlen(ext);
    return lp >= le && strcmp(path + lp - le, ext) == 0;
}

// The same CSR in device memory, kept beside the host vectors when the context was asked to (r3dm_set_device_graphs): what
// r3dm_allgather_graphs puts on the wire without a host round trip of the payload (api_comm.cpp).  Filled where the data already is
// on the device: by the gather kernels behind the match finalisation and the filters (kernels_graph.hip).
struct GraphDev {
    DevBuf pairs, counts, matches;    // u32 [2 P], u32 [P], r3dm_match [M]
    uint64_t P = 0, M = 0;
    int device = -1;
    bool valid = false;
    void release() { pairs.release(); counts.release(); matches.release(); P = M = 0; valid = false; device = -1; }
};

struct r3dm_graph {
    std::vector<uint32_t> pairs;      // 2 per pair
    std::vector<uint64_t> offsets;    // n_pairs + 1
    std::vector<r3dm_match> matches;
    GraphDev dev;                     // optional device mirror (never copied with the graph)
    r3dm_graph() = default;
    r3dm_graph(const r3dm_graph&) = delete;
    r3dm_graph& operator=(const r3dm_graph&) = delete;
    ~r3dm_graph() { dev.release(); }
};

struct FilterBufs {
    DevBuf f_pairs, f_ids, f_offs, f_matches, f_inl_cnt, f_inl_idx, f_F, f_thr, f_iters, f_log10, f_logck, f_scratch, f_kinv, f_spill, f_soff, f_order, f_coop, f_coop_prof, f_la;
    // r3dm_filter_FEH: the kernel of this kind on a stream of its own PRIORITY class (E high, F normal, H low).  Streams of one
    // priority share a handful of hardware queues -- three plain streams ran the three kernels mostly one after the other --, streams
    // of different priorities never do.
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    PinBuf pin_idx;           // page-locked landing zone of the inlier indices
    void release()
    {
        pin_idx.release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
        ev0 = ev1 = nullptr; stream = nullptr;
        DevBuf* b[] = {&f_pairs, &f_ids, &f_offs, &f_matches, &f_inl_cnt, &f_inl_idx, &f_F, &f_thr, &f_iters, &f_log10, &f_logck, &f_scratch, &f_kinv, &f_spill, &f_soff, &f_order, &f_coop, &f_coop_prof, &f_la};
        for (DevBuf* x : b) x->release();
    }
};

// Guided matching (kernels_guided.hip, api_guided.cpp): the work buffers of a call's one launch, and what it hands back
struct GuidedBufs {
    DevBuf jobs, res, q_cnt, q_off, blk_cnt, blk_base, cand, ctr, out, out_cnt;
    PinBuf pin_out, pin_small, pin_blk;
    void release()
    {
        DevBuf* b[] = {&jobs, &res, &q_cnt, &q_off, &blk_cnt, &blk_base, &cand, &ctr, &out, &out_cnt};
        for (DevBuf* x : b) x->release();
        pin_out.release(); pin_small.release(); pin_blk.release();
    }
};
// Feature tracks (kernels_tracks.hip, api_tracks.cpp): the work buffers of r3dm_build_tracks, made by the first call, grown on demand
struct TracksBufs {
    DevBuf matches, offsets, pair_rank, view_ids, base, smax, par, slots, ma, rel, keep, pair_kept, nodes, keys, skey, sval, nodeflag,
           oslots, obs, hflag, toff, kept_rel, ctr, temp;
    PinBuf pin;
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // four timed phases
    void release()
    {
        DevBuf* b[] = {&matches, &offsets, &pair_rank, &view_ids, &base, &smax, &par, &slots, &ma, &rel, &keep, &pair_kept, &nodes, &keys, &skey,
                       &sval, &nodeflag, &oslots, &obs, &hflag, &toff, &kept_rel, &ctr, &temp};
        for (DevBuf* x : b) x->release();
        pin.release();
        for (hipEvent_t& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
};
struct GuidedResult {
    std::vector<uint32_t> cnt;             // matches of every job
    const r3dm_match* host = nullptr;      // job k's list at host + jobs[k].q0 (page-locked, valid until the next guided call)
    const r3dm_match* dev = nullptr;       // the same on the device (the source of graph mirrors)
};
// one job of a guided launch: pub_kind R3DM_GUIDED_F / _E / _H, M the model as the filter returns it, thr_px as r3dm_pair_report
// reports it, ratio < 0: geometry only
int guided_job_make(r3dm_ctx* c, uint32_t sI, uint32_t sJ, int pub_kind, const double* M, double thr_px, double ratio, GuidedJob& out);
// runs the jobs (q0 / b0 are assigned here), fills c->guided_stats; jobs may be empty
int guided_run(r3dm_ctx* c, std::vector<GuidedJob>& jobs, GuidedResult& R);
// ---- the detectors (api_akaze.cpp: the Fast arm and what both arms share; api_akaze_classic.cpp)
// one evolution level of either arm's table (the classic arm has no descriptor border and no sublevel: both stay 0)
struct AkLevelHost {
    int w, h, octave, sublevel, sigma_size, border;
    float esigma, etime, ratio;
};

// angle of a Fast-arm keypoint: getAngleV2(maxX, maxY) (fast-akaze utils.h:11-19: atan2f of the host libm, + 2 pi when negative)
inline float ak_theta(const AkKpRec& r)
{
    float theta = atan2f(r.max_y, r.max_x);
    if (!(theta >= 0)) theta = theta + (float)(2.0f * 3.1415926535897932384626433832795);
    return theta;
}
// ... and the conversion of detectKeypoints (src/Regard3DFeatures.cpp:604-613): degrees, + 90, wrapped into [0, 360]
inline float ak_angle_deg(float ang)
{
    ang *= 180.0 / 3.1415926535897932384626433832795;
    ang += 90.0f;
    while (ang < 0) ang += 360.0f;
    while (ang > 360.0f) ang -= 360.0f;
    return ang;
}

// What a detector pass over B same-size images hands its consumers, whichever arm ran.  The Fast arm keeps its raw records (MLDB reads
// them and the level table): their angle is host libm atan2f per keypoint, formed when a consumer asks -- the features batch asks from
// its parallel loop.  (The classic arm's angle comes from the device, in degrees, without the + 90: DESIGN.md section 7.)
struct DetectedBatch {
    std::vector<std::vector<AkKpRec>> fast;            // Fast arm: per image, the survivors in the reference's order (level, list)
    std::vector<AkLevelHost> fast_levels;              //           the evolution levels of this image size
    float fast_smax = 0.0f;                            //           ... and the border factor they were cut with (ak_smax, descriptor_arms.hpp)
    std::vector<std::vector<AcOut>> classic;           // classic arm: per image, the slots that survive, in slot order
    const float* grays_dev = nullptr;                  // the B gray planes the detector left on the device (read-only for it)
    size_t count(uint32_t b) const { return fast.empty() ? classic[b].size() : fast[b].size(); }
    void keypoint(uint32_t b, size_t k, float* o) const     // x, y, size, angle in degrees
    {
        if (fast.empty()) { const AcOut& a = classic[b][k]; o[0] = a.x; o[1] = a.y; o[2] = a.size; o[3] = a.angle; }
        else { const AkKpRec& r = fast[b][k]; o[0] = r.x; o[1] = r.y; o[2] = r.size; o[3] = ak_angle_deg(ak_theta(r)); }
    }
    float response(uint32_t b, size_t k) const { return fast.empty() ? classic[b][k].resp : fast[b][k].response; }
};
// the two arms; gray images (host or device) or 8-bit BGR.  detect_batch: the context's arm (r3dm_set_keypoint_detector)
using DetectArm = int(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height,
                      float threshold, DetectedBatch& out);
DetectArm ak_detect_batch, ak_detect_batch_msurf, ac_detect_batch, detect_batch;
// A detect entry: its argument checks, B gray images through `arm`, then keypoints_out[b] / responses_out[b] (entries optional) / n_out[b]:
// min(count, cap) rows are written, the count itself is reported.  single: one image by value, whose count reads 0 when the arm fails
int detect_entry(r3dm_ctx* c, DetectArm* arm, bool single, uint32_t B, const float* const* images, uint32_t width, uint32_t height, float threshold,
                 float* const* keypoints_out, float* const* responses_out, uint32_t cap, uint32_t* n_out, DetectedBatch& d);

// The frame both arms stand in (api_akaze.cpp)
AkTaps ak_taps(float sigma);
bool ak_is_prime(int number);
// what every detect entry refuses: no context, no images, an image above 2^30 pixels, more than 4096 images
bool detect_args_ok(const r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, uint32_t width, uint32_t height);
// B gray images, or B 8-bit BGR images converted on the device as processWorkItem does (src/threads/R3DFeaturesThread.cpp:163-191), into
// the B planes of n0 floats at `gray`; the BGR bytes are staged at `stage` (4 n0 bytes apart): a work image of the arm's not yet in use
int detect_upload(r3dm_ctx* c, uint32_t B, const float* const* images, const unsigned char* const* bgrs, size_t n0, float* gray, unsigned char* stage);
// INTER_AREA tables of the octave transitions whose size is not an exact halving (they depend on the image size only): built, uploaded
// into `buf` and waited for before the launch sequence, which then never touches the host.  Per level; null where the halving is exact
struct HalfTabs { const AkAreaTab* xt = nullptr; const int* xb = nullptr; const AkAreaTab* yt = nullptr; const int* yb = nullptr; };
int detect_area_tabs(r3dm_ctx* c, DevBuf& buf, const std::vector<AkLevelHost>& lv, std::vector<HalfTabs>& tabs);
// the tail of a pass: kernel time (ev0 .. ev1) and wall time into the statistics, the pass into the totals
void detect_finish(r3dm_ctx* c, uint32_t B, double t_call, uint64_t n_keypoints, double algorithmic_bytes);

// ---- the level-plane descriptors of a Fast-arm pass, MLDB-486 and M-SURF-64 (api_akaze.cpp): one launch of `arm`'s kernel over the first
// min(count, cap) keypoints of every image of `det`, which must be the context's last detector pass and, for M-SURF, cut on the arm's own
// level table (else R3DM_ERR_INVALID: the other table's borders do not hold its reads in).  first: B + 1 row offsets; *rows_dev: the
// rows, arm.row_bytes each, image b's at + arm.row_bytes first[b] (null when there is no keypoint), valid until the context's next
// detector or descriptor pass.  Bracketed by ev0 / ev1 and waited for; host_team threads share the item loop (cos / sin of every
// keypoint's angle, host libm)
int ak_describe_pass(r3dm_ctx* c, const DescriptorArm& arm, const DetectedBatch& det, uint32_t cap, int host_team, std::vector<size_t>& first,
                     const unsigned char** rows_dev);

// ---- LIOP (api_liop.cpp)
// 2x3 inverse map of one keypoint's patch (x, y, size, angle in degrees)
void liop_patch_map(float x, float y, float size, float angle_deg, float kp_size_factor, float* m);
// One LIOP pass over n > 0 keypoints of the image(s) at dev_images (planes of width x height floats; img_of: the plane of every keypoint,
// null = plane 0), M6 = their patch maps on the host.  Descriptors -> c->liop_out; with want_patches (or the developer build's
// R3DM_LIOP_FUSED=0) the patches go through HBM -> c->liop_in.  Bracketed by ev0 / ev1, not waited for: the caller copies and synchronises
int liop_pass(r3dm_ctx* c, const float* dev_images, uint32_t width, uint32_t height, const float* M6, const uint32_t* img_of, uint32_t n,
              bool want_patches);
void liop_read_time(r3dm_ctx* c);

// The way of a view from host memory to HBM (r3dm_set_image / r3dm_set_images): a ring of page-locked slots the caller's pageable rows
// are copied into by the host (several threads for a batch of views), one asynchronous DMA per view from there into the slot's
// device buffer, the staging kernel behind it, an event behind that -- a slot is reused when its event has passed; nothing waits
// per view.  Every view in flight also owns the slot's position-class hash table.
struct UploadRing {
    static constexpr int kSlots = 8;
    PinBuf pin[kSlots];
    DevBuf raw[kSlots];
    DevBuf ctab[kSlots];                 // position-class hash table: u64 keys [2^bits] then u32 values [2^bits]
    hipEvent_t ev[kSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool busy[kSlots] = {false, false, false, false, false, false, false, false};
    uint64_t next = 0;
    // the DMAs run on a stream of their own, each followed by an event the view's staging kernel waits for on the context's stream: the
    // DMA of view k + 1 then runs beside the kernel of view k instead of behind it (one stream: 85 us + 29 us per 8,192 x 128 view)
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copy[kSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    void release()
    {
        for (int k = 0; k < kSlots; ++k) {
            pin[k].release(); raw[k].release(); ctab[k].release();
            if (ev[k]) (void)hipEventDestroy(ev[k]);
            if (ev_copy[k]) (void)hipEventDestroy(ev_copy[k]);
            ev[k] = nullptr; ev_copy[k] = nullptr; busy[k] = false;
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        copy_stream = nullptr;
    }
};

struct r3dm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    std::string arch;
    int n_cu = 0;
    uint64_t hbm = 0;
    std::vector<std::unique_ptr<HostImage>> imgs;           // slot -> image
    std::vector<std::unique_ptr<HostImage>> spare;          // views dropped by r3dm_clear_images: their device buffers serve the next ones
    std::unordered_map<uint32_t, uint32_t> slot_of;         // view id -> slot
    DevBuf d_imgs;                                           // ImgDev[slots]
    PinBuf tab_host;                                         // page-locked mirror of the table's entries as the host last published them
    PinBuf tab_back;                                         // landing zone of the table read back by sync_view_stats()
    std::vector<uint32_t> pending_stats;                     // slots staged since the last sync_view_stats()
    UploadRing ring;
    DevArena arena;                                          // device memory of the registered views' layouts
    DevBuf d_verdict;                                        // verdict words of count-tile checks launched by ensure_layouts
    uint64_t n_ring_uploads = 0, n_direct_uploads = 0;       // views that went through the ring / were read where the caller had them
    // scratch (grown on demand, reused across calls)
    DevBuf d_pairs, d_pairnorm, d_pairnorm_tiles, d_nn, d_knn_idx, d_knn_dist, d_fb, d_cnt, d_out, d_pair_off, d_pair_cnt, d_raw;
    // geometric filters: one set of work buffers per model kind (0 F, 1 H, 2 E), so that r3dm_filter_FEH can run the three
    // AC-RANSAC kernels of a putative graph side by side (a collection with few, long pairs leaves most CUs idle under one)
    FilterBufs fb[3];
    // the cooperative AC-RANSAC kernel of a call (long pairs of all its filters, one pool of workers): scheduling words + start order +
    // device copy of the kinds' parameters; its stream and the event recorded behind it
    DevBuf coop_sched;
    hipStream_t coop_stream = nullptr;
    hipEvent_t coop_ev = nullptr;
    DevBuf liop_pix, liop_sx, liop_sy, liop_in, liop_out, liop_cnt, liop_img, liop_M, liop_kern;
    DevBuf h_aux, h_jobs;            // HNSW: per-batch layer tables / job records
    DevBuf a_jobs, a_scratch, a_ids, d_spill, d_fb2;
    DevBuf m_raw, m_peer;                                   // r3dm_multi_set_image: the one upload of a view / this device's copy of it
    std::vector<DevBuf> ak_bufs;                            // Fast-A-KAZE work buffers of the last image size, ak_B planes each
    std::vector<DevBuf> ac_bufs;                            // classic A-KAZE work buffers (api_akaze_classic.cpp: grow, never shrink)
    uint64_t ac_components[32] = {};                        // component-size histogram of the classic arm's kpts_aux walk (r3dm_akaze_classic_components)
    int detector_arm = R3DM_DETECTOR_FAST_AKAZE;            // r3dm_set_keypoint_detector: the arm of the features entries
    int descriptor_arm = R3DM_DESCRIPTOR_LIOP;              // r3dm_set_descriptor_arm: what the features entries describe the keypoints with
    int ak_w = 0, ak_h = 0, ak_B = 0;
    uint32_t ak_cap = 0;                                    // candidate slots per image the detector last needed (grows, never shrinks)
    int ak_n_levels = 0;
    AkLevelDev* ak_levels_dev = nullptr;                    // level table of the last detector pass (inside ak_bufs; read by the MLDB kernel)
    PinBuf pin_small;                                       // ... of the counters and per-pair tables that come back with them
    PinBuf pin_out;                                         // page-locked landing zone of the match lists of a batch (finalize_batch)
    PinBuf pin_desc;                                        // page-locked landing zone of the LIOP descriptors of a batch
    bool integer_mfma = false;                              // r3dm_set_integer_mfma
    bool prefix_pruning = true;                             // r3dm_set_prefix_pruning: match mode on 128-dimensional rows stops tiles early
    bool half_filter = true;                                // r3dm_set_half_filter: the f16 level in front of the pair-norm filter
    bool half_prefix = true;                                // r3dm_set_half_prefix: the restart's prefix test on f16 rows in front of the restart
    bool min_tile_test = true;                              // r3dm_set_min_tile_test: the three levels' tile tests in their min form where the norms allow it
    // wave tiles of the last match call, summed over its batches from PruneHeader's counters
    struct PruneTotals {
        uint64_t tested = 0, pruned = 0;                    // r3dm_get_prefix_pruning_counts
        uint64_t filtered = 0;                              // r3dm_get_pair_filter_counts: pruned by the filter (part of pruned)
        uint64_t half = 0;                                  // r3dm_get_half_filter_counts: pruned by the f16 level (part of filtered)
        uint64_t skipped = 0;                               // r3dm_get_level2_skip_counts: sent by the f16 level straight to the restart (no f32 filter)
        uint64_t prefix16_tested = 0, prefix16_pruned = 0;  // r3dm_get_half_prefix_counts: tiles the f16 prefix test saw / pruned (part of pruned)
        uint64_t min_pairs = 0, general_pairs = 0;          // r3dm_get_min_tile_test_counts: pairs the three levels matched in the min form / the general form
    } prune_totals;
    bool split_mfma = false;                                // r3dm_set_split_mfma
    bool hamming_mfma = false;                              // r3dm_set_hamming_mfma
    bool knn_narrow_tiles = false;                          // r3dm_set_knn_narrow_tiles
    bool knn_hamming_tiles = false;                         // r3dm_set_knn_hamming_tiles
    bool mutual_matching = false;                           // r3dm_set_mutual_matching: the mutual check runs before every finalisation into a graph
    bool kgraph_hamming = false;                            // r3dm_set_kgraph_hamming: the graph matcher serves binary views (Hamming index + search on the packed rows)
    r3dm_kgraph_hamming_stats kgraph_hamming_stats{};       // r3dm_kgraph_hamming_report: since r3dm_create (never reset)
    bool symmetric_ratio = false;                           // r3dm_set_symmetric_ratio: the check also applies the reverse ratio test (and runs with the mutual switch off)
    uint64_t symratio_counts[3] = {0, 0, 0};                // r3dm_symmetric_ratio_report: checked / not nearest / removed by the reverse ratio in the last collecting call
    DevBuf d_mutual;                                        // its three counters (allocated by the first batch that runs the check)
    // r3dm_set_preemptive_matching (api_preselect.cpp): the switch, its head size and threshold; the buffers of a gate call (row lists,
    // head table, pairs, counts), its events and its report -- all made by the first gate
    bool preemptive_on = false;
    uint32_t preemptive_h = 128, preemptive_t = 4;
    DevBuf pre_rows, pre_heads, pre_pairs, pre_counts;
    PinBuf pre_pin;
    hipEvent_t pre_ev0 = nullptr, pre_ev1 = nullptr;
    r3dm_preselect_stats preselect_stats{};
    // r3dm_set_match_budget (api_budget.cpp): the switch and its N; the buffers of a substitution (priorities and selection jobs, the
    // gathered rows on their way into a sub-view slot, the row-list table the remap reads), its events and its report -- all made by
    // the first call that budgets a view
    bool budget_on = false;
    uint32_t budget_N = 8192;
    DevBuf bud_jobs, bud_prio, bud_raw, bud_maps, bud_sel;
    PinBuf bud_pin;
    hipEvent_t bud_ev[2] = {nullptr, nullptr};
    bool bud_maps_live = false;                              // bud_maps holds the table of the running collection call: its batches are remapped
    r3dm_budget_stats budget_stats{};
    bool device_graphs = false;                             // r3dm_set_device_graphs: match / filter results keep a device mirror (GraphDev)
    DevBuf g_segs;                                          // segment table of the graph gather kernel (kernels_graph.hip)
    uint32_t liop_npix = 0;
    uint64_t n_views_staged = 0;                            // copies + re-layouts since r3dm_create (never reset)
    r3dm_stats stats{};
    r3dm_features_sink feat_sink = nullptr; void* feat_sink_user = nullptr;   // r3dm_set_features_sink
    const uint32_t* feat_sink_ids = nullptr;                 // indices of the running batch in its caller's arrays (r3dm_multi_extract_features*), else 0 .. B-1
    r3dm_features_totals feat_totals{};                      // since r3dm_create (r3dm_get_features_totals)
    // r3dm_set_deferred_feature_files: the fwrite of a batch's .feat / .desc runs on `file_writer` behind the sink calls; the thread
    // reads pin_desc, so it is joined before that buffer is filled again, by r3dm_features_files_wait and by r3dm_destroy
    bool defer_files = false;
    int background_nice = 0;                                  // r3dm_set_background_nice: nice value of this context's background writer threads (0 = unchanged)
    hipEvent_t ev_desc = nullptr;                            // the descriptors of the batch have landed in pin_desc (created on first use)
    std::thread file_writer;
    int file_writer_rc = 0; std::string file_writer_err;
    double file_writer_ms = 0.0;                             // wall time the writer threads spent (sum since the last wait)
    std::vector<r3dm_pair_report> report;                    // last r3dm_filter_F call, one per putative pair
    // r3dm_set_guided_matching: the filters re-match their accepted pairs; ratios by R3DM_GUIDED_F / _E / _H (< 0: geometry only)
    bool guided_on = false;
    double guided_ratio[3] = {0.6, 0.6, -1.0};
    GuidedBufs gb;
    r3dm_guided_stats guided_stats{};                        // last guided step (r3dm_guided_report)
    TracksBufs tb;                                           // r3dm_build_tracks: nothing in it until the first call
};

int graph_dev_append(r3dm_ctx* c, r3dm_graph* g, const std::vector<uint32_t>& pair_ids, const std::vector<uint32_t>& counts, std::vector<GraphSeg>& segs,
                     const r3dm_match* src, const uint32_t* idx);      // api_core.cpp

// Appends pairs to a result graph (match batches, the filters' inliers and guided lists, r3dm_guided_match): a pair's list is src[at ..
// at + n), or src[idx[ix_at .. ix_at + n)] when the builder has an index list.  With `mirror` (r3dm_set_device_graphs) the builder also
// records where every list lies in the device copies of those arrays, and done() gathers them into the graph's device mirror; a failed
// gather only invalidates the mirror (api_core.cpp).
struct GraphBuilder {
    r3dm_ctx* c;
    r3dm_graph* g;
    bool mirror;
    const r3dm_match* src; const uint32_t* idx;               // host arrays the lists are read from
    const r3dm_match* dev_src; const uint32_t* dev_idx;       // the same arrays on the device
    std::vector<uint32_t> ids, cnts;
    std::vector<GraphSeg> segs;
    uint64_t dst = 0;                                         // matches appended so far (the segments count from the first of them)
    GraphBuilder(r3dm_ctx* c_, r3dm_graph* g_, bool mirror_, const r3dm_match* src_, const uint32_t* idx_, const r3dm_match* dev_src_,
                 const uint32_t* dev_idx_)
        : c(c_), g(g_), mirror(mirror_), src(src_), idx(idx_), dev_src(dev_src_), dev_idx(dev_idx_)
    {
        if (mirror && !g->dev.valid) { g->dev.valid = true; g->dev.device = c->device; }
    }
    void add(uint32_t I, uint32_t J, uint64_t at, uint64_t ix_at, uint32_t n)
    {
        g->pairs.push_back(I); g->pairs.push_back(J);
        if (idx) {
            const size_t base = g->matches.size();
            g->matches.resize(base + n);
            r3dm_match* d = g->matches.data() + base;
            const r3dm_match* s = src + at;
            const uint32_t* ix = idx + ix_at;
            for (uint32_t q = 0; q < n; ++q) d[q] = s[ix[q]];
        } else {
            g->matches.insert(g->matches.end(), src + at, src + at + n);
        }
        g->offsets.push_back(g->matches.size());
        if (mirror) { ids.push_back(I); ids.push_back(J); cnts.push_back(n); segs.push_back(GraphSeg{at, ix_at, dst, n, 0}); }
        dst += n;
    }
    void done() { if (mirror) (void)graph_dev_append(c, g, ids, cnts, segs, dev_src, dev_idx); }
};

#define R3DM_HIP(ctx, call)                                                            \
    do {                                                                               \
        hipError_t e__ = (call);                                                       \
        if (e__ != hipSuccess) {                                                       \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);          \
            return R3DM_ERR_HIP;                                                       \
        }                                                                              \
    } while (0)

// The C ABI never throws: entry points whose bodies size host containers from caller- or file-provided counts run behind this
// guard (std::bad_alloc / std::length_error would otherwise cross the extern "C" boundary and terminate the host application).
template <class F>
static inline int r3dm_guarded(r3dm_ctx* c, F&& body) noexcept
{
    try { return body(); }
    catch (const std::bad_alloc&) { if (c) { try { c->err = "out of host memory"; } catch (...) {} } return R3DM_ERR_NOMEM; }
    catch (const std::exception& e) { if (c) { try { c->err = e.what(); } catch (...) {} } return R3DM_ERR_INVALID; }
    catch (...) { return R3DM_ERR_INVALID; }
}

struct PairJob { uint32_t I, J, sI, sJ; };

// Slots of one call (r3dm_knn2 and its relatives), at the end of the table, never visible through view ids: plain HostImages, not arena
// blocks or spares.  On every exit -- error returns and exceptions included -- the stream is synchronised, and the slots are released,
// dropped from pending_stats and popped.
struct PrivateSlots {
    r3dm_ctx* c;
    uint32_t first;
    PrivateSlots(r3dm_ctx* c_, uint32_t n) : c(c_), first((uint32_t)c_->imgs.size())
    {
        try { for (uint32_t k = 0; k < n; ++k) c->imgs.push_back(std::unique_ptr<HostImage>(new HostImage())); }
        catch (...) { drop(); throw; }
    }
    ~PrivateSlots() { drop(); }
    uint32_t operator[](uint32_t k) const { return first + k; }
    PrivateSlots(const PrivateSlots&) = delete;
    void operator=(const PrivateSlots&) = delete;
private:
    void drop() noexcept
    {
        (void)hipStreamSynchronize(c->stream);
        std::vector<uint32_t>& p = c->pending_stats;
        p.erase(std::remove_if(p.begin(), p.end(), [this](uint32_t s) { return s >= first; }), p.end());
        while (c->imgs.size() > first) { if (c->imgs.back()) c->imgs.back()->release(); c->imgs.pop_back(); }
    }
};

// The counters of a call that reports its own work in a few named fields of the context's statistics (r3dm_knn2 and its relatives):
// on every exit c->stats is back to what it was when this was made, except the named counters, which hold the call's delta.
struct CallCounters {
    r3dm_ctx* c;
    const r3dm_stats before;
    const std::vector<uint64_t r3dm_stats::*> counts;
    const std::vector<double r3dm_stats::*> times;
    CallCounters(r3dm_ctx* c_, std::initializer_list<uint64_t r3dm_stats::*> counts_, std::initializer_list<double r3dm_stats::*> times_ = {})
        : c(c_), before(c_->stats), counts(counts_), times(times_) {}
    ~CallCounters()
    {
        const r3dm_stats after = c->stats;
        c->stats = before;
        for (auto m : counts) c->stats.*m = after.*m - before.*m;
        for (auto m : times) c->stats.*m = after.*m - before.*m;
    }
};

// A dataset staged once for many queries (ArrayMatcher::Build): owns its device buffers, belongs to a device, not to a context
struct r3dm_index {
    int device = 0;
    HostImage img;                              // (statistics included: HostImage::stat_bits)
    std::mutex mu;                              // layouts staged after Build (a flag switched on later) are added under this lock
    // the approximate arms' structures (img.ann_* / hnsw_* / mrpt_*) are built on first use under the lock too, from the first call's
    // build parameters, which are kept here: a later call that names others is refused, nothing is ever rebuilt under a search's feet
    bool kgraph_built = false, hnsw_built = false, mrpt_built = false;
    r3dm_kgraph_params kgraph_p{};
    r3dm_hnsw_params hnsw_p{};
    r3dm_mrpt_params mrpt_p{};
};

inline void HostImage::mount(r3dm_index* ix) { *this = ix->img; borrowed = true; owner = ix; }

// shared between the translation units
// (re)writes the table entry of `slot` from its HostImage, statistics included: only for views whose statistics the host holds
int publish_entry(r3dm_ctx* c, uint32_t slot);
// the statistics of every view staged since the last call -> HostImage (one read of the table, one synchronisation)
int sync_view_stats(r3dm_ctx* c);
// stages the layouts `want` (kLay* bits) of every listed slot that does not hold them; kLayCounts: *counts_all_ok = every listed view
// passed the votes-x-scale check.  Slots that mount an r3dm_index are staged under the index's lock.
int ensure_layouts(r3dm_ctx* c, std::vector<uint32_t> slots, uint32_t want, bool* counts_all_ok = nullptr);
int ensure_layouts_image(r3dm_ctx* c, HostImage& h, uint32_t want);        // (no table entry involved; the caller publishes)
int run_match_batch(r3dm_ctx* c, const std::vector<PairJob>& jobs, float ratio_R, r3dm_graph* g,
                    int32_t* knn_idx_host, float* knn_dist_host);
// knn_cols: entries per query in d_knn_idx / d_knn_dist (2: the 2-NN kernels; k: the k-list kernels of the approximate arms)
int finalize_batch(r3dm_ctx* c, const std::vector<PairJob>& jobs, uint32_t q_stride, uint32_t sort_cap,
                   uint64_t n_queries, uint32_t max_nJ, r3dm_graph* g, int32_t* knn_idx_host, float* knn_dist_host, uint32_t knn_cols = 2,
                   ForwardRatio forward = ForwardRatio());   // forward: the batch's ratio test, which r3dm_set_symmetric_ratio repeats in reverse
int run_exact_knn_pair(r3dm_ctx* c, uint32_t sI, uint32_t sJ, uint32_t k, int32_t* out_idx, float* out_dist);
// an index search's two private slots: the index mounted into slot_index beside the freshly staged query view in slot_query
int mount_index_beside_queries(r3dm_ctx* c, const r3dm_index* ix, const void* query, uint32_t n_query, uint32_t slot_index, uint32_t slot_query);
int ensure_ann_indices(r3dm_ctx* c, std::vector<uint32_t> slots, uint32_t K);
int stage_into_slot(r3dm_ctx* c, uint32_t slot, uint32_t view_id, uint32_t width, uint32_t height,
                    const void* desc, uint32_t n, uint32_t dim, r3dm_dtype dtype, const float* xy);

// ---- the frames of the approximate matchers (api_ann.cpp)
// first view of a valid pair -> index = searched through the arm's index / scanned exhaustively, or the arm's refusal (c->err set)
using PairClassifier = std::function<int(const HostImage& A, bool& index)>;
// pairs_ij -> the jobs of its valid pairs, ordered by (I, J), unique; no classifier: every job is scanned
int resolve_pairs(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs, const PairClassifier& classify,
                  std::vector<PairJob>& indexed, std::vector<PairJob>& scanned);
// the gate of preemptive matching (api_preselect.cpp), called by the four collection entries right after resolve_pairs: resets the
// report; while the switch is on, both lists keep only the pairs whose head count reaches the threshold under ratio R
// (bin_ratio_R >= 0: the R of pairs of binary views, where a call's list may mix them with float views under another rule)
int preselect_gate(r3dm_ctx* c, float ratio_R, std::vector<PairJob>& indexed, std::vector<PairJob>& scanned, float bin_ratio_R = -1.0f);
// the match budget (api_budget.cpp), called by the four collection entries right after the gate: resets the report; while the switch is
// on, every job's sI / sJ whose view has more rows than the budget becomes the slot of the view's sub-view (made here when missing or
// stale; I / J stay), and with a classifier the jobs are dealt again between the two lists by their sub-views.  finalize_batch calls
// budget_remap on the device's match array of every batch of such a call, before the copy back and the device mirror.
int budget_substitute(r3dm_ctx* c, std::vector<PairJob>& indexed, std::vector<PairJob>& scanned, const PairClassifier& classify = nullptr);
int budget_remap(r3dm_ctx* c, const std::vector<PairJob>& jobs, const uint32_t* pair_cnt_host, const uint64_t* pair_off_dev,
                 const uint32_t* pair_cnt_dev, r3dm_match* matches_dev);       // (the pair table of the batch is in c->d_pairs)
// ends the call's remapping on every exit of a collection entry
struct BudgetCallGuard { r3dm_ctx* c; ~BudgetCallGuard() { c->bud_maps_live = false; } };
// What a collection call of an arm is made of.  The chunk rules differ on purpose: KGraph and HNSW launch one descriptor length at a
// time, MRPT's job records carry their own; HNSW and MRPT launch a grid row per pair (65,535 at most), KGraph does not.
struct AnnArm {
    PairClassifier classify;
    std::function<int(const std::vector<PairJob>& indexed)> ensure;                    // layouts + indices of the indexed jobs' views
    std::function<int(const std::vector<PairJob>& batch, r3dm_graph* g)> run_batch;    // one chunk of them, appended to g
    bool one_dim_per_chunk = false;                          // a chunk holds one (dtype, dim)
    size_t max_chunk_pairs = SIZE_MAX;
    // >= 0: the arm serves binary views, whose scanned pairs and gate take this R (the ratio unsquared: Hamming is no squared metric)
    float bin_ratio_R = -1.0f;
};
// resets c->stats; indexed chunks + scanned pairs (ratio scanned_ratio_R) -> *out, ordered by (I, J)
int match_collection_ann(r3dm_ctx* c, const uint32_t* pairs_ij, uint64_t n_pairs, float scanned_ratio_R, const AnnArm& arm, r3dm_graph** out);
// What the batch frame hands an arm's launch: the arm uploads its job records, fills its parameter struct and launches on c->stream
// (the pair table is in c->d_pairs; c->d_cnt is zeroed, n_comps counts the distance evaluations)
struct AnnBatch {
    uint32_t P, dim, q_stride, max_nI, max_nJ;
    uint32_t* nn_idx; int32_t* knn_idx; float* knn_dist; unsigned long long* n_comps;
};
int run_ann_batch(r3dm_ctx* c, const std::vector<PairJob>& jobs, r3dm_graph* g, int32_t* knn_idx_host, float* knn_dist_host,
                  const std::function<int(const AnnBatch&)>& launch, uint32_t knn_cols = 2, ForwardRatio forward = ForwardRatio());

// ---- k-NN through an arm's structure on an r3dm_index (r3dm_index_kgraph_knn / _hnsw_knn / _mrpt_knn)
// state(image of the index): R3DM_OK = the arm's structure is there and was built from these build parameters, 1 = not built yet,
// R3DM_ERR_INVALID = built from others (c->err set).  Not built: build(slot) runs ONCE, under the index's lock, on a slot that holds the
// index's image for that long.  Then the index is mounted beside the staged queries and search(slot of the index, slot of the queries)
// runs, outside the lock: any context of the device, several at a time.
int with_index_structure(r3dm_ctx* c, const r3dm_index* ix, const void* query, uint32_t n_query,
                         const std::function<int(const r3dm_index&)>& state, const std::function<int(r3dm_index&, uint32_t slot)>& build,
                         const std::function<int(uint32_t sI, uint32_t sJ)>& search);

// An array entry of an arm (r3dm_kgraph_knn2 and its relatives): two private slots, dataset and query staged as `dtype` (F32; R3DM_BIN for
// the _bits entries, dim = bytes per row) under the view ids (id_i, id_j), the call's counters (CallCounters), then body(slot of the
// dataset, slot of the queries)
template <class Body>
inline int with_staged_pair_of(r3dm_ctx* c, r3dm_dtype dtype, const void* dataset, uint32_t n_dataset, const void* query, uint32_t n_query, uint32_t dim,
                               uint32_t id_i, uint32_t id_j, std::initializer_list<uint64_t r3dm_stats::*> counts,
                               std::initializer_list<double r3dm_stats::*> times, Body&& body)
{
    R3DM_HIP(c, hipSetDevice(c->device));
    PrivateSlots s(c, 2);
    int rc = stage_into_slot(c, s[0], id_i, 0, 0, dataset, n_dataset, dim, dtype, nullptr);
    if (rc == R3DM_OK) rc = stage_into_slot(c, s[1], id_j, 0, 0, query, n_query, dim, dtype, nullptr);
    if (rc != R3DM_OK) return rc;
    CallCounters counters(c, counts, times);
    return body(s[0], s[1]);
}
template <class Body>
inline int with_staged_pair(r3dm_ctx* c, const float* dataset, uint32_t n_dataset, const float* query, uint32_t n_query, uint32_t dim,
                            uint32_t id_i, uint32_t id_j, std::initializer_list<uint64_t r3dm_stats::*> counts,
                            std::initializer_list<double r3dm_stats::*> times, Body&& body)
{
    return with_staged_pair_of(c, R3DM_F32, dataset, n_dataset, query, n_query, dim, id_i, id_j, counts, times, std::forward<Body>(body));
}
