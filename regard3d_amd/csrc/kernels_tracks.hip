// kernels_tracks.hip -- feature tracks of a match graph (r3dm_build_tracks): what OpenMVG's TracksBuilder
// (Build, Filter, ExportToSTL) computes with a std::set of nodes, a std::map node -> index and a serial union-find.
//
// A node (view, feature) is the SLOT base[rank(view)] + feature: views ranked by id, base = the prefix sum of s(v) = 1 + the view's
// largest feature index.  Slot order is then (view id, feature) order, and everything canonical falls out of two facts:
//   * the union hangs the larger root under the smaller one, so the final root of a component is its smallest slot -- the track's first
//     observation.  Root order is track order.
//   * a stable sort of the touched slots (taken in slot order) by root lists every component contiguously, members ascending: a
//     surviving component's run IS its observation list, and a conflict (two nodes of one view) is two NEIGHBOURS of one view.
//   extent    per match: the largest feature index of both views (one integer atomic per wavefront where its lanes share the pair)
//   init      parent = itself
//   link      per match: both slots touched, union (agent-scope relaxed loads, path halving, atomicCAS: the idiom of the classic
//             A-KAZE detector's component walk, kernels_akaze_classic.hip)
//   flatten   per touched slot: root (no path halving: see the kernel) and the component's node count
//   [select]  the touched slots, ascending; keys = their roots; [sort] by root, stable
//   mark      neighbours of one root and one view -> the root conflicts.  A star of thousands of nodes costs its nodes, like any other
//   classify  per sorted node: does its component survive the filter; per component: the counters
//   [select]  the surviving nodes = the observations in output order
//   emit      slot -> (view id, feature); first node of a track flagged; [select] of the flagged positions = the track offsets
//   keep      per match: is its component a track; its pair's kept count
// The selections and the sort are at the end of this file.  (rocPRIM's would do, but every one of its scan-based algorithms reads an
// environment variable on first use, and the product library never reads the environment.)  All counters are integers; every
// hand-over between kernels goes through the stream order, inside a wavefront through ballots or the release / wave_barrier /
// acquire pattern.
#include "r3dm_internal.hpp"

#include <utility>

namespace r3dm {

__device__ __forceinline__ uint32_t trk_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t trk_find(uint32_t* par, uint32_t x)
{
    for (;;) {
        const uint32_t p = trk_ld(par + x);
        if (p == x) return x;
        const uint32_t g = trk_ld(par + p);
        if (g == p) return p;
        __hip_atomic_store(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // path halving: g is an ancestor of x whatever else happens
        x = g;
    }
}
__device__ __forceinline__ void trk_union(uint32_t* par, uint32_t a, uint32_t b)
{
    for (;;) {
        a = trk_find(par, a); b = trk_find(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }                                // the larger root goes under the smaller one: no cycle
        if (atomicCAS(par + a, a, b) == a) return;
    }
}
// pair of match m: the last p with offsets[p] <= m (offsets[0] = 0, offsets[P] = M > m)
__device__ __forceinline__ uint32_t trk_pair_of(const uint64_t* __restrict__ offsets, uint32_t P, uint64_t m)
{
    uint32_t lo = 0, hi = P;
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (offsets[mid] <= m) lo = mid; else hi = mid; }
    return lo;
}
// rank of the view that owns `slot`: the last r with base[r] <= slot (base[V] = N > slot; s(v) >= 1, so base is strictly increasing)
__device__ __forceinline__ uint32_t trk_rank_of(const uint32_t* __restrict__ base, uint32_t V, uint32_t slot)
{
    uint32_t lo = 0, hi = V;
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (base[mid] <= slot) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ uint32_t trk_wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d); v = v > o ? v : o; }
    return v;
}
// counter += number of lanes with pred: one atomic per wavefront
__device__ __forceinline__ void trk_count(unsigned long long* ctr, bool pred)
{
    const uint64_t b = __ballot(pred);
    if (b && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(b)) atomicAdd(ctr, (unsigned long long)__builtin_popcountll(b));
}

// grid-stride over the matches, whole wavefronts at a time: m0 is the wavefront's first match of the trip
#define TRK_MATCH_LOOP(P_)                                                                                                   \
    for (uint64_t m0 = ((uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u)); m0 < (P_).M; m0 += (uint64_t)gridDim.x * 256u)

__global__ __launch_bounds__(256)
void trk_extent_kernel(TrkParams T)
{
    const uint32_t lane = threadIdx.x & 63u;
    TRK_MATCH_LOOP(T) {
        const uint64_t m = m0 + lane;
        const bool act = m < T.M;
        const uint32_t p = trk_pair_of(T.offsets, T.P, act ? m : m0);
        const r3dm_match mt = T.matches[act ? m : m0];
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
        if (__all(p == p0)) {                                  // the usual wavefront: one pair, two destinations
            const uint32_t fi = trk_wave_max(mt.i), fj = trk_wave_max(mt.j);
            if (lane == 0) { atomicMax(T.smax + T.pair_rank[2 * (size_t)p0], fi); atomicMax(T.smax + T.pair_rank[2 * (size_t)p0 + 1], fj); }
        } else if (act) {
            atomicMax(T.smax + T.pair_rank[2 * (size_t)p], mt.i); atomicMax(T.smax + T.pair_rank[2 * (size_t)p + 1], mt.j);
        }
    }
}

__global__ __launch_bounds__(256)
void trk_init_kernel(TrkParams T)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < T.N) T.par[i] = i;
}

__global__ __launch_bounds__(256)
void trk_link_kernel(TrkParams T)
{
    const uint32_t lane = threadIdx.x & 63u;
    TRK_MATCH_LOOP(T) {
        const uint64_t m = m0 + lane;
        if (m >= T.M) continue;
        const uint32_t p = trk_pair_of(T.offsets, T.P, m);
        const r3dm_match mt = T.matches[m];
        const uint32_t a = T.base[T.pair_rank[2 * (size_t)p]] + mt.i, b = T.base[T.pair_rank[2 * (size_t)p + 1]] + mt.j;
        T.ma[m] = a;
        T.rel[m] = (uint32_t)(m - T.offsets[p]);
        T.touched[a] = 1; T.touched[b] = 1;                    // (the same value from every writer)
        if (a != b) trk_union(T.par, a, b);
    }
}

__global__ __launch_bounds__(256)
void trk_flatten_kernel(TrkParams T)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool act = i < T.N && T.touched[i];
    // a walk WITHOUT path halving: a halving find of another lane could otherwise put a mere ancestor back over a root stored here
    // (kernels_akaze_classic.hip, ac_cc_flatten_kernel).  The only stores now are par[i] = root: every chain stays one of ancestors.
    uint32_t r = i;
    if (act) {
        for (uint32_t p = trk_ld(T.par + r); p != r; p = trk_ld(T.par + r)) r = p;
        if (r != i) __hip_atomic_store(T.par + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // node counts: one integer atomic per distinct root of the wavefront (neighbouring slots of a junk component share theirs)
    uint64_t todo = __ballot(act);
    while (todo) {
        const int f = __builtin_ctzll(todo);
        const uint32_t r0 = (uint32_t)__shfl((int)r, f);
        const uint64_t same = __ballot(act && r == r0) & todo;
        if ((int)lane == f) atomicAdd(T.csz + r0, (uint32_t)__builtin_popcountll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256)
void trk_keys_kernel(TrkParams T)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < T.n_nodes) T.keys[k] = T.par[T.nodes[k]];
}

__global__ __launch_bounds__(256)
void trk_mark_kernel(TrkParams T)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k == 0 || k >= T.n_nodes) return;
    const uint32_t root = T.skey[k];
    if (T.skey[k - 1] != root) return;
    if (trk_rank_of(T.base, T.V, T.sval[k]) == trk_rank_of(T.base, T.V, T.sval[k - 1])) T.conf[root] = 1;     // (the same value from every writer)
}

// ctr: [0] components, [1] conflicting, [2] short, [3] tracks, [4] matches kept, [5] longest track, [6] largest component
__global__ __launch_bounds__(256)
void trk_classify_kernel(TrkParams T)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool act = k < T.n_nodes;
    uint32_t root = 0, sz = 0; bool head = false, cf = false, sv = false;
    if (act) {
        root = T.skey[k]; sz = T.csz[root]; cf = T.conf[root] != 0;
        head = k == 0 || T.skey[k - 1] != root;
        sv = !cf && sz >= T.min_length;
        T.nodeflag[k] = sv ? 1 : 0;
        if (head) T.surv[root] = sv ? 1 : 0;
    }
    trk_count(T.ctr + 0, head);
    trk_count(T.ctr + 1, head && cf);
    trk_count(T.ctr + 2, head && !cf && !sv);
    trk_count(T.ctr + 3, head && sv);
    const uint32_t longest = trk_wave_max(head && sv ? sz : 0u), largest = trk_wave_max(head ? sz : 0u);
    if (lane == 0) {
        if (longest) atomicMax(T.ctr + 5, (unsigned long long)longest);
        if (largest) atomicMax(T.ctr + 6, (unsigned long long)largest);
    }
}

__global__ __launch_bounds__(256)
void trk_emit_kernel(TrkParams T)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= T.n_obs) return;
    const uint32_t slot = T.oslots[k], r = trk_rank_of(T.base, T.V, slot);
    r3dm_observation o; o.view = T.view_ids[r]; o.feature = slot - T.base[r];
    T.obs[k] = o;
    T.hflag[k] = (k == 0 || T.par[T.oslots[k - 1]] != T.par[slot]) ? 1 : 0;
}

__global__ __launch_bounds__(256)
void trk_keep_kernel(TrkParams T)
{
    const uint32_t lane = threadIdx.x & 63u;
    TRK_MATCH_LOOP(T) {
        const uint64_t m = m0 + lane;
        const bool act = m < T.M;
        const uint32_t p = trk_pair_of(T.offsets, T.P, act ? m : m0);
        const bool kp = act && T.surv[T.par[T.ma[m]]] != 0;
        if (act) T.keep[m] = kp ? 1 : 0;
        trk_count(T.ctr + 4, kp);
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
        if (__all(p == p0)) {
            const uint64_t b = __ballot(kp);
            if (b && lane == 0) atomicAdd(T.pair_kept + p0, (uint32_t)__builtin_popcountll(b));
        } else if (kp) {
            atomicAdd(T.pair_kept + p, 1u);
        }
    }
}

static inline dim3 trk_grid(uint64_t n) { const uint64_t b = (n + 255u) / 256u; return dim3((uint32_t)(b < (1u << 20) ? (b ? b : 1u) : (1u << 20))); }

hipError_t launch_tracks(hipStream_t st, const TrkParams& T, TrkStep step)
{
    switch (step) {
    case TrkStep::kExtent:   if (T.M) hipLaunchKernelGGL(trk_extent_kernel, trk_grid(T.M), dim3(256), 0, st, T); break;
    case TrkStep::kInit:     if (T.N) hipLaunchKernelGGL(trk_init_kernel, trk_grid(T.N), dim3(256), 0, st, T); break;
    case TrkStep::kLink:     if (T.M) hipLaunchKernelGGL(trk_link_kernel, trk_grid(T.M), dim3(256), 0, st, T); break;
    case TrkStep::kFlatten:  if (T.N) hipLaunchKernelGGL(trk_flatten_kernel, trk_grid(T.N), dim3(256), 0, st, T); break;
    case TrkStep::kKeys:     if (T.n_nodes) hipLaunchKernelGGL(trk_keys_kernel, trk_grid(T.n_nodes), dim3(256), 0, st, T); break;
    case TrkStep::kMark:     if (T.n_nodes) hipLaunchKernelGGL(trk_mark_kernel, trk_grid(T.n_nodes), dim3(256), 0, st, T); break;
    case TrkStep::kClassify: if (T.n_nodes) hipLaunchKernelGGL(trk_classify_kernel, trk_grid(T.n_nodes), dim3(256), 0, st, T); break;
    case TrkStep::kEmit:     if (T.n_obs) hipLaunchKernelGGL(trk_emit_kernel, trk_grid(T.n_obs), dim3(256), 0, st, T); break;
    case TrkStep::kKeep:     if (T.M) hipLaunchKernelGGL(trk_keep_kernel, trk_grid(T.M), dim3(256), 0, st, T); break;
    }
    return hipGetLastError();
}

// ---- order-preserving selection and stable radix sort.  The unit of both is a TILE walked by one wavefront, 64 consecutive elements a
// step, so that ranks inside a step are popcounts of ballots and nothing is handed between wavefronts inside a kernel:
//   select   count the flagged elements of every tile; exclusive scan of the counts (one workgroup); every tile writes its flagged
//            elements from its offset on, in order
//   sort     per 8-bit digit, least significant first: digit histogram of every tile, laid out [digit][tile]; exclusive scan of that
//            array = where every (digit, tile) run starts; every tile writes its elements behind its runs, in order (stable)
#define TRK_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// a[0 .. n) -> its exclusive prefix sums, in place; *total (optional) = the sum.  One workgroup of 1024 threads, 4096 entries a trip
__global__ __launch_bounds__(1024)
void trk_scan_kernel(uint32_t* __restrict__ a, uint64_t n, unsigned long long* __restrict__ total)
{
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n; base += 4096u) {
        const uint64_t i0 = base + 4u * tid;
        uint32_t v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = i0 + k < n ? a[i0 + k] : 0u; s += v[k]; }
        uint32_t incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, d); if ((int)lane >= d) incl += t; }
        if (lane == 63u) wsum[wave] = incl;
        r3dm_syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16u; ++w) { const uint32_t x = wsum[w]; all += x; if (w < wave) before += x; }
        uint32_t ex = (uint32_t)carry + before + incl - s;
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (i0 + k < n) a[i0 + k] = ex; ex += v[k]; }
        carry += all;
        r3dm_syncthreads();
    }
    if (total && tid == 0) *total = carry;
}

__global__ __launch_bounds__(256)
void trk_select_count_kernel(const uint8_t* __restrict__ flags, uint64_t n, uint64_t tile_elems, uint32_t n_tiles, uint32_t* __restrict__ cnt)
{
    const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const uint64_t b0 = (uint64_t)tile * tile_elems, e0 = b0 + tile_elems < n ? b0 + tile_elems : n;
    uint32_t c = 0;
    for (uint64_t i0 = b0; i0 < e0; i0 += 64u) {
        const uint64_t i = i0 + lane;
        c += (uint32_t)__builtin_popcountll(__ballot(i < e0 && flags[i] != 0));
    }
    if (lane == 0) cnt[tile] = c;
}
// out = vals[i] (vals given) or i, for the flagged i, ascending
template <class OutT>
__global__ __launch_bounds__(256)
void trk_select_write_kernel(const uint8_t* __restrict__ flags, uint64_t n, uint64_t tile_elems, uint32_t n_tiles, const uint32_t* __restrict__ off,
                             const uint32_t* __restrict__ vals, OutT* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const uint64_t b0 = (uint64_t)tile * tile_elems, e0 = b0 + tile_elems < n ? b0 + tile_elems : n;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint64_t at = off[tile];
    for (uint64_t i0 = b0; i0 < e0; i0 += 64u) {
        const uint64_t i = i0 + lane;
        const bool f = i < e0 && flags[i] != 0;
        const uint64_t b = __ballot(f);
        if (f) out[at + (uint64_t)__builtin_popcountll(b & lt)] = vals ? (OutT)vals[i] : (OutT)i;
        at += (uint64_t)__builtin_popcountll(b);
    }
}

__global__ __launch_bounds__(256)
void trk_sort_hist_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint64_t tile_elems, uint32_t n_tiles, uint32_t shift, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t lds[4][256];
    const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t* my = lds[threadIdx.x >> 6];
    if (tile >= n_tiles) return;
    for (uint32_t d = lane; d < 256u; d += 64u) my[d] = 0u;
    TRK_WAVE_SYNC();
    const uint64_t b0 = (uint64_t)tile * tile_elems, e0 = b0 + tile_elems < n ? b0 + tile_elems : n;
    for (uint64_t i0 = b0; i0 < e0; i0 += 64u) {
        const uint64_t i = i0 + lane;
        if (i < e0) atomicAdd(my + ((keys[i] >> shift) & 255u), 1u);
    }
    TRK_WAVE_SYNC();
    for (uint32_t d = lane; d < 256u; d += 64u) hist[(size_t)d * n_tiles + tile] = my[d];
}
__global__ __launch_bounds__(256)
void trk_sort_write_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t n, uint64_t tile_elems, uint32_t n_tiles,
                           uint32_t shift, const uint32_t* __restrict__ hist, uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out)
{
    __shared__ uint32_t lds[4][256];
    const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t* my = lds[threadIdx.x >> 6];                      // where the next element of every digit goes
    if (tile >= n_tiles) return;
    for (uint32_t d = lane; d < 256u; d += 64u) my[d] = hist[(size_t)d * n_tiles + tile];
    TRK_WAVE_SYNC();
    const uint64_t b0 = (uint64_t)tile * tile_elems, e0 = b0 + tile_elems < n ? b0 + tile_elems : n;
    const uint64_t lt = (1ull << lane) - 1ull;
    for (uint64_t i0 = b0; i0 < e0; i0 += 64u) {
        const uint64_t i = i0 + lane;
        const bool act = i < e0;
        const uint32_t key = act ? keys[i] : 0u, val = act ? vals[i] : 0u, d = (key >> shift) & 255u;
        uint64_t same = __ballot(act);                         // the active lanes with this lane's digit
#pragma unroll
        for (uint32_t bit = 0; bit < 8u; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t b = __ballot(one);
            same &= one ? b : ~b;
        }
        if (act) {
            const uint32_t pos = my[d] + (uint32_t)__builtin_popcountll(same & lt);
            keys_out[pos] = key; vals_out[pos] = val;
        }
        TRK_WAVE_SYNC();                                       // every lane has read its digit's cursor
        if (act && lane == 63u - (uint32_t)__builtin_clzll(same)) my[d] += (uint32_t)__builtin_popcountll(same);     // the digit's last lane moves it
        TRK_WAVE_SYNC();
    }
}

// elements per tile: a multiple of 1024 that keeps the number of tiles at or below max_tiles
static inline uint64_t trk_tile_elems(uint64_t n, uint64_t max_tiles) { const uint64_t per = 1024u * max_tiles; return 1024u * ((n + per - 1) / per ? (n + per - 1) / per : 1u); }
constexpr uint64_t kTrkSelectTiles = 1ull << 18, kTrkSortTiles = 1ull << 12;

size_t tracks_scratch_words(uint64_t n, bool sort)
{
    const uint64_t te = trk_tile_elems(n, sort ? kTrkSortTiles : kTrkSelectTiles), tiles = (n + te - 1) / te;
    return (size_t)(sort ? 256u * tiles : tiles) + 4u;
}

template <class OutT>
static hipError_t trk_select(hipStream_t st, uint32_t* scratch, const uint8_t* flags, uint64_t n, const uint32_t* vals, OutT* out, unsigned long long* count)
{
    if (n == 0) return hipMemsetAsync(count, 0, 8, st);
    const uint64_t te = trk_tile_elems(n, kTrkSelectTiles);
    const uint32_t tiles = (uint32_t)((n + te - 1) / te), blocks = (tiles + 3u) / 4u;
    hipLaunchKernelGGL(trk_select_count_kernel, dim3(blocks), dim3(256), 0, st, flags, n, te, tiles, scratch);
    hipLaunchKernelGGL(trk_scan_kernel, dim3(1), dim3(1024), 0, st, scratch, (uint64_t)tiles, count);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(trk_select_write_kernel<OutT>), dim3(blocks), dim3(256), 0, st, flags, n, te, tiles, (const uint32_t*)scratch, vals, out);
    return hipGetLastError();
}
// out = the positions i < n with flags[i] != 0, ascending (vals == nullptr), or vals[i] of those positions; *count = how many
hipError_t tracks_select(hipStream_t st, uint32_t* scratch, const uint8_t* flags, uint64_t n, const uint32_t* vals, uint32_t* out, unsigned long long* count)
{
    return trk_select<uint32_t>(st, scratch, flags, n, vals, out, count);
}
hipError_t tracks_select64(hipStream_t st, uint32_t* scratch, const uint8_t* flags, uint64_t n, uint64_t* out, unsigned long long* count)
{
    return trk_select<uint64_t>(st, scratch, flags, n, nullptr, out, count);
}
// (keys, vals) sorted by the low `bits` bits of the keys, stable; both pairs of arrays are work space, *in_second = the result is in
// (keys2, vals2), else in (keys, vals)
hipError_t tracks_sort_by_root(hipStream_t st, uint32_t* scratch, uint32_t* keys, uint32_t* vals, uint32_t* keys2, uint32_t* vals2, uint64_t n,
                               uint32_t bits, bool* in_second)
{
    *in_second = false;
    if (n == 0) return hipSuccess;
    const uint64_t te = trk_tile_elems(n, kTrkSortTiles);
    const uint32_t tiles = (uint32_t)((n + te - 1) / te), blocks = (tiles + 3u) / 4u;
    for (uint32_t shift = 0; shift < bits; shift += 8u) {
        hipLaunchKernelGGL(trk_sort_hist_kernel, dim3(blocks), dim3(256), 0, st, (const uint32_t*)keys, n, te, tiles, shift, scratch);
        hipLaunchKernelGGL(trk_scan_kernel, dim3(1), dim3(1024), 0, st, scratch, (uint64_t)256u * tiles, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(trk_sort_write_kernel, dim3(blocks), dim3(256), 0, st, (const uint32_t*)keys, (const uint32_t*)vals, n, te, tiles, shift,
                           (const uint32_t*)scratch, keys2, vals2);
        std::swap(keys, keys2); std::swap(vals, vals2);
        *in_second = !*in_second;
    }
    return hipGetLastError();
}

}  // namespace r3dm
