// kernels_akaze_classic.hip -- the classic A-KAZE detector on gfx950: Regard3D's "AKAZE" arm, defined as libAKAZE
// (src/thirdparty/akaze/lib/: AKAZE.cpp, nldiffusion_functions.cpp, fed.cpp).  The Gaussian, the fused
// Scharr + PM-G2 conductivity, the gradient maximum and the half-sampling are the Fast arm's kernels (kernels_akaze.hip): libAKAZE runs
// the same OpenCV primitive with the same operations there.  What differs from Fast-AKAZE's V2 functions lives here, and every
// difference is named at its site.  Same determinism rules as the Fast arm: + - * / sqrt in float without contraction
// (-ffp-contract=off), double only where libAKAZE's own expression is double; batched as B same-size images, blockIdx.z = image
// for the image passes.
#include "r3dm_internal.hpp"

namespace r3dm {

namespace {

constexpr uint32_t kAcSmallWords = 4096;             // per-image scalars, as the Fast arm's: [0] max |grad| bits, [16..316) histogram, [1024 + o] 1 / k^2

__device__ __forceinline__ int ac_refl101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) { if (p < 0) p = -p; else p = 2 * len - 2 - p; }
    return p;
}
__device__ __forceinline__ int ac_fround(float f) { return (int)(f + 0.5f); }      // fRound (AKAZE.h:200)

#define AC_PLANE(ptr, w, h) ((ptr) + (size_t)blockIdx.z * ((size_t)(w) * (size_t)(h)))

// ---- compute_k_percentile's histogram (nldiffusion_functions.cpp:166-186).  Differs from compute_k_percentileV2: a zero modulus is
// not counted, the bin is floor(nbins * (modg / hmax)) with the top value folded into the last bin.  The modulus is the Scharr pair of
// the sigma-1 image computed on the spot with the operations of the Scharr row + column pass (ak_scharr_*_kernel), interior only.
__global__ __launch_bounds__(256)
void ac_kc_hist_kernel(const float* __restrict__ src, int w, int h, const uint32_t* __restrict__ small, uint32_t* __restrict__ hist_out)
{
    __shared__ uint32_t lh[304];
    src = AC_PLANE(src, w, h);
    const uint32_t* sm = small + (size_t)blockIdx.z * kAcSmallWords;
    uint32_t* hist = hist_out + (size_t)blockIdx.z * kAcSmallWords;
    const float hmax = __uint_as_float(sm[0]);
    for (int k = threadIdx.x; k < 300; k += 256) lh[k] = 0;
    r3dm_syncthreads();
    const int x = 1 + blockIdx.x * 64 + (threadIdx.x & 63);
    if (hmax != 0.0f && x < w - 1) {
        for (int y = 1 + blockIdx.y * 4 + (threadIdx.x >> 6); y < h - 1; y += gridDim.y * 4) {
            const float* Su = src + (size_t)(y - 1) * w; const float* Sc = Su + w; const float* Sd = Sc + w;
            const float rdu = Su[x + 1] - Su[x - 1], rdc = Sc[x + 1] - Sc[x - 1], rdd = Sd[x + 1] - Sd[x - 1];
            const float rsu = Su[x] * 10.0f + (Su[x - 1] + Su[x + 1]) * 3.0f, rsd = Sd[x] * 10.0f + (Sd[x - 1] + Sd[x + 1]) * 3.0f;
            const float lx = (rdu + rdd) * 3.0f + rdc * 10.0f;
            const float ly = rsd - rsu;
            const float modg = sqrtf(lx * lx + ly * ly);
            if (modg != 0.0f) {
                int nbin = (int)floorf(300.0f * (modg / hmax));
                if (nbin >= 300) nbin = 299;
                atomicAdd(&lh[nbin], 1u);
            }
        }
    }
    r3dm_syncthreads();
    for (int k = threadIdx.x; k < 300; k += 256) if (lh[k]) atomicAdd(hist + k, lh[k]);
}

// ---- the percentile scan of compute_k_percentile (:188-199), one thread per image.  The reference counts in float: a bin or the
// point count stops at 2^24, and nelements (size_t) + hist[k] (float) is a float sum converted back.  kperc = 0.03 when the percentile
// is not reached.  out[1024 + o] = 1 / k_o^2 with k_o = k_{o-1} * 0.75 (Create_Nonlinear_Scale_Space, AKAZE.cpp:131-134).
__global__ void ac_kc_finish_kernel(uint32_t* __restrict__ small)
{
    uint32_t* sm = small + (size_t)blockIdx.x * kAcSmallWords;
    const float hmax = __uint_as_float(sm[0]);
    const uint32_t* hist = sm + 16;
    const float cap = 16777216.0f;
    uint64_t total = 0;
    for (int k = 0; k < 300; ++k) total += hist[k];
    const float npoints = total >= (1u << 24) ? cap : (float)total;
    const uint64_t nthreshold = (uint64_t)(npoints * 0.7f);
    uint64_t nelements = 0;
    int k = 0;
    for (; nelements < nthreshold && k < 300; ++k) {
        const float hk = hist[k] >= (1u << 24) ? cap : (float)hist[k];
        nelements = (uint64_t)((float)nelements + hk);
    }
    float kc = nelements < nthreshold ? 0.03f : hmax * ((float)k / 300.0f);
    float* inv = reinterpret_cast<float*>(sm + 1024);
    for (int o = 0; o < 8; ++o) { inv[o] = 1.0f / (kc * kc); kc = kc * 0.75f; }
}

// ---- one FED step of nld_step_scalar (nldiffusion_functions.cpp:208-331): Lstep = (0.5f * stepsize) * (xpos - xneg + ypos - yneg),
// out = Lt + Lstep.  Differs from nld_step_scalarV2: the flux differences are subtracted in the reference's order, the half step
// multiplies the sum (the V2 form multiplies the sum by 0.5 then by the step), and the four corners are formed (V2 leaves them).
__device__ __forceinline__ float ac_flux(const float* c, const float* L, size_t p, size_t q) { return (c[p] + c[q]) * (L[q] - L[p]); }
__global__ __launch_bounds__(256)
void ac_fed_step_kernel(const float* __restrict__ Lt, const float* __restrict__ Lf, float* __restrict__ out, int w, int h, float half_step)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    Lt = AC_PLANE(Lt, w, h); Lf = AC_PLANE(Lf, w, h); out = AC_PLANE(out, w, h);
    const size_t p = (size_t)y * w + x, W = (size_t)w;
    float v;
    if (y == 0 || y == h - 1) {
        // the first row's ypos looks down, the last row's "ypos" looks up: (c + c_up) * (L_up - L)
        const float ypos = y == 0 ? ac_flux(Lf, Lt, p, p + W) : ac_flux(Lf, Lt, p, p - W);
        if (x == 0) v = ac_flux(Lf, Lt, p, p + 1) + ypos;
        else if (x == w - 1) v = (-ac_flux(Lf, Lt, p - 1, p)) + ypos;
        else v = (ac_flux(Lf, Lt, p, p + 1) - ac_flux(Lf, Lt, p - 1, p)) + ypos;
    } else {
        const float ypos = ac_flux(Lf, Lt, p, p + W), yneg = ac_flux(Lf, Lt, p - W, p);
        if (x == 0) v = (ac_flux(Lf, Lt, p, p + 1) + ypos) - yneg;
        else if (x == w - 1) v = ((-ac_flux(Lf, Lt, p - 1, p)) + ypos) - yneg;
        else v = ((ac_flux(Lf, Lt, p, p + 1) - ac_flux(Lf, Lt, p - 1, p)) + ypos) - yneg;
    }
    out[p] = Lt[p] + half_step * v;
}

// ---- multiscale derivatives (Compute_Multiscale_Derivatives, AKAZE.cpp:188-216): sepFilter2D, BORDER_REFLECT_101, with the kernels
// of compute_derivative_kernels (nldiffusion_functions.cpp:346-383).  Differs from compute_scharr_derivative_kernelsV2: the smoothing
// taps are normalised by the scale, norm = 1 / (2 s (w + 2)) (the host forms norm and the centre tap w * norm as the reference does).
// The tap structure of the row and column passes is the Fast arm's; each output recomputes its row-pass values on the spot.
struct AcTaps { float norm, kc; int s; };
__device__ __forceinline__ float ac_row(const float* __restrict__ S, int x, int w, const AcTaps& t, bool dx)
{
    const float a = S[ac_refl101(x - t.s, w)], b = S[ac_refl101(x + t.s, w)];
    if (dx) return (-a) + b;
    if (t.s == 2) return S[x] * t.kc + (a + b) * t.norm;           // SymmRowSmallFilter, ksize 5
    return (t.norm * a + t.kc * S[x]) + t.norm * b;                 // RowFilter, left to right
}
__device__ __forceinline__ float ac_deriv(const float* __restrict__ src, int x, int y, int w, int h, const AcTaps& t, bool dx)
{
    const float u = ac_row(src + (size_t)ac_refl101(y - t.s, h) * w, x, w, t, dx);
    const float d = ac_row(src + (size_t)ac_refl101(y + t.s, h) * w, x, w, t, dx);
    if (dx) { const float c = ac_row(src + (size_t)y * w, x, w, t, dx); return t.kc * c + t.norm * (d + u); }
    return d - u;
}
__global__ __launch_bounds__(256)
void ac_deriv_xy_kernel(const float* __restrict__ src, float* __restrict__ Lx, float* __restrict__ Ly, int w, int h, AcTaps t)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    src = AC_PLANE(src, w, h); Lx = AC_PLANE(Lx, w, h); Ly = AC_PLANE(Ly, w, h);
    Lx[(size_t)y * w + x] = ac_deriv(src, x, y, w, h, t, true);
    Ly[(size_t)y * w + x] = ac_deriv(src, x, y, w, h, t, false);
}
// Lxx = d/dx Lx, Lyy = d/dy Ly, Lxy = d/dy Lx and Compute_Determinant_Hessian_Response (:219-248): (Lxx Lyy - Lxy^2) * s^4 in float
// (Fast-AKAZE leaves the determinant unscaled)
__global__ __launch_bounds__(256)
void ac_deriv_det_kernel(const float* __restrict__ Lx, const float* __restrict__ Ly, float* __restrict__ Ldet, int w, int h, AcTaps t, float s4)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    Lx = AC_PLANE(Lx, w, h); Ly = AC_PLANE(Ly, w, h); Ldet = AC_PLANE(Ldet, w, h);
    const float lxx = ac_deriv(Lx, x, y, w, h, t, true);
    const float lyy = ac_deriv(Ly, x, y, w, h, t, false);
    const float lxy = ac_deriv(Lx, x, y, w, h, t, false);
    Ldet[(size_t)y * w + x] = (lxx * lyy - lxy * lxy) * s4;
}

// ---- extrema (Find_Scale_Space_Extrema, AKAZE.cpp:279-287): strict 3 x 3 maxima over dthreshold and min_dthreshold, rows 1..h-2 x
// columns 1..w-2.  One wavefront per row: pass 0 counts, pass 1 writes the row's candidates at its offset in raster order.
__device__ __forceinline__ bool ac_is_max(const float* __restrict__ L, int w, int x, int y, float thr)
{
    const float* c = L + (size_t)y * w + x;
    const float v = c[0];
    return v > thr && v >= 0.00001f && v > c[-1] && v > c[1] && v > c[-w - 1] && v > c[-w] && v > c[-w + 1] &&
           v > c[w - 1] && v > c[w] && v > c[w + 1];
}
__global__ __launch_bounds__(64)
void ac_extrema_kernel(const float* __restrict__ ldet, int w, int h, float thr, uint32_t* __restrict__ row_counts, uint32_t rows_stride,
                       uint32_t row0, AcCand* __restrict__ cand, uint32_t cand_stride, int level, int pass)
{
    const int y = 1 + blockIdx.x;
    if (y >= h - 1) return;
    ldet = AC_PLANE(ldet, w, h);
    uint32_t* rc = row_counts + (size_t)blockIdx.z * rows_stride + row0 + y;
    const int lane = threadIdx.x;
    uint32_t at = pass ? *rc : 0u;
    AcCand* out = cand + (size_t)blockIdx.z * cand_stride;
    for (int x0 = 1; x0 < w - 1; x0 += 64) {
        const int x = x0 + lane;
        const bool m = x < w - 1 && ac_is_max(ldet, w, x, y, thr);
        const uint64_t bal = __ballot(m);
        if (pass && m) {
            const uint32_t q = at + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            out[q] = AcCand{(uint32_t)x, (uint32_t)y, (uint32_t)level, ldet[(size_t)y * w + x]};
        }
        at += (uint32_t)__popcll(bal);
    }
    if (!pass && lane == 0) *rc = at;
}
// exclusive scan of the per-row counts of one image (one workgroup per image, sequential chunks of 1024 rows); total in totals[b]
__global__ __launch_bounds__(1024)
void ac_scan_rows_kernel(uint32_t* __restrict__ row_counts, uint32_t rows_stride, uint32_t n_rows, uint32_t* __restrict__ totals)
{
    __shared__ uint32_t s[1024];
    uint32_t* rc = row_counts + (size_t)blockIdx.x * rows_stride;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_rows; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_rows ? rc[i] : 0u;
        s[threadIdx.x] = v;
        r3dm_syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const uint32_t t = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0u;
            r3dm_syncthreads();
            s[threadIdx.x] += t;
            r3dm_syncthreads();
        }
        if (i < n_rows) rc[i] = carry + s[threadIdx.x] - v;
        const uint32_t add = s[1023];
        r3dm_syncthreads();
        carry += add;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// ---- the sequential kpts_aux rule (AKAZE.cpp:288-350), one wavefront per image, candidates in libAKAZE's scan order (levels in
// order, rows, then columns).  A level-l point compares only with the slots of class l - 1 and l, and only a slot within size^2 of it can
// decide; among those the FIRST in slot order decides.  So the wavefront keeps the slots of the current window in a spatial grid of
// cells of side G = floor(size) + 1 > size (integer cell coordinates of the truncated position: a slot within size of the point lies in
// the 3 x 3 cells around it), and a point's decision is the smallest slot index among the hits of those nine cell lists -- nine lanes
// walk one list each and the wavefront takes the minimum.  The result is the linear scan's by construction; the cost of a point is the
// occupancy of its neighbourhood, not the length of the list.  A replaced slot moves: it gets an entry in its new cell and its old entry
// stays (an entry is only a pointer; every test reads the slot's current class and position).  At the start of level l the cells of the
// previous level are cleared through their entries and the slots of class l - 1 are entered.
__device__ __forceinline__ int ac_cell_of(float v, int G) { return (int)v / G; }
// kMembers = false: every candidate of the image, straight into the slots (the developer build's R3DM_AC_AUX=0 form).
// kMembers = true: the hand-back of the parallel walk below -- only the candidates flagged in cc.big (the members of the components
// larger than the wavefront bound), in scan order.  Components do not interact, so walking their union is walking each of them; the
// slots are scratch (slots[q].pad = the candidate last written into slot q, cc.bopen[q] = the one that opened it) and the walk leaves
// cc.fin[opener] = last writer, cc.opn[opener] = 1 for ac_cc_emit_kernel.
template <bool kMembers>
__global__ __launch_bounds__(64)
void ac_aux_kernel(const AcCand* __restrict__ cand, uint32_t cand_stride, const uint32_t* __restrict__ totals, AcLevelTab tab,
                   AcSlot* __restrict__ slots, AcGrid grid, uint32_t* __restrict__ n_slots, AcCc cc)
{
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (kMembers && cc.n_big[b] == 0) return;
    const AcCand* cb = cand + (size_t)b * cand_stride;
    AcSlot* sl = slots + (size_t)b * cand_stride;
    int* heads = grid.heads + (size_t)b * grid.cells_stride;
    uint32_t* ent_slot = grid.ent_slot + (size_t)b * grid.ent_stride;
    uint32_t* ent_cell = grid.ent_cell + (size_t)b * grid.ent_stride;
    int* ent_next = grid.ent_next + (size_t)b * grid.ent_stride;
    const uint32_t* big = kMembers ? cc.big + (size_t)b * cand_stride : nullptr;
    uint32_t* bopen = kMembers ? cc.bopen + (size_t)b * cand_stride : nullptr;
    const uint32_t* rows = kMembers ? cc.rows + (size_t)b * cc.rows_stride : nullptr;
    const uint32_t nc = totals[b];
    uint32_t n = 0, ne = 0, c = 0;
    for (int l = 0; l < tab.n_levels; ++l) {
        const float size = tab.esigma[l] * 1.5f;                     // point.size = esigma * derivative_factor
        const int G = (int)size + 1;
        const int gw = grid.img_w / G + 2, gh = grid.img_h / G + 2;  // positions stay below img + ratio: inside gw x gh cells
        // clear the previous level's cells, then enter the slots of class l - 1
        for (uint32_t e = lane; e < ne; e += 64) heads[ent_cell[e]] = -1;
        __syncthreads();
        ne = 0;
        if (l > 0)
            for (uint32_t q0 = 0; q0 < n; q0 += 64) {
                const uint32_t q = q0 + lane;
                const bool m = q < n && sl[q].cls == (uint32_t)(l - 1);
                const uint64_t bal = __ballot(m);
                if (m) {
                    const uint32_t e = ne + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                    const uint32_t cell = (uint32_t)(ac_cell_of(sl[q].y, G) * gw + ac_cell_of(sl[q].x, G));
                    ent_slot[e] = q; ent_cell[e] = cell;
                    ent_next[e] = atomicExch(&heads[cell], (int)e);
                }
                ne += (uint32_t)__popcll(bal);
            }
        __syncthreads();
        const float ratio = tab.ratio[l];
        const int ss = ac_fround(size / ratio);
        const float s2 = size * size;
        const float r = tab.smax * (float)ss;
        const float off = tab.off[l];
        // one candidate through the rule
        auto step = [&](uint32_t ci) {
            const AcCand k = cb[ci];
            const float px = (float)k.x, py = (float)k.y;
            const float sx = px * ratio, sy = py * ratio;
            uint32_t best = 0xFFFFFFFFu;
            if (lane < 9) {
                const int cx = ac_cell_of(sx, G) + (int)(lane % 3) - 1, cy = ac_cell_of(sy, G) + (int)(lane / 3) - 1;
                if (cx >= 0 && cx < gw && cy >= 0 && cy < gh)
                    for (int e = heads[cy * gw + cx]; e >= 0; e = ent_next[e]) {
                        const uint32_t q = ent_slot[e];
                        if (q >= best) continue;
                        const AcSlot s = sl[q];
                        if (s.cls != (uint32_t)l && s.cls + 1 != (uint32_t)l) continue;
                        const float tx = sx - s.x, ty = sy - s.y;
                        if (tx * tx + ty * ty <= s2) best = q;
                    }
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_xor((int)best, o); best = v < best ? v : best; }
            const int hit = best == 0xFFFFFFFFu ? -1 : (int)best;
            bool rep = false;
            if (hit >= 0) {
                if (k.value > sl[hit].resp) rep = true;
                else return;                                      // the first hit decides: rejected
            }
            const int left = ac_fround(px - r) - 1, right = ac_fround(px + r) + 1;
            const int up = ac_fround(py - r) - 1, down = ac_fround(py + r) + 1;
            if (left < 0 || right >= tab.w[l] || up < 0 || down >= tab.h[l]) return;   // descriptor border: out
            const uint32_t q = rep ? (uint32_t)hit : n;
            if (lane == 0) {
                // pt * ratio + .5 * (ratio - 1.0): the double sum of exact values, stored as float
                const float nx = (float)((double)sx + (double)off), ny = (float)((double)sy + (double)off);
                sl[q] = AcSlot{nx, ny, size, k.value, (uint32_t)l, kMembers ? ci : 0u};
                if (kMembers && !rep) bopen[q] = ci;
                const uint32_t cell = (uint32_t)(ac_cell_of(ny, G) * gw + ac_cell_of(nx, G));
                ent_slot[ne] = q; ent_cell[ne] = cell;
                ent_next[ne] = atomicExch(&heads[cell], (int)ne);
            }
            ++ne;
            if (!rep) ++n;
            __syncthreads();                                      // workgroup-scope fence: the slot and its entry are seen by every lane
        };
        if (!kMembers) {
            for (; c < nc && cb[c].level == (uint32_t)l; ++c) step(c);
        } else {
            // the level's candidates are [rows[row0[l]], rows[row0[l + 1]]): 64 flags at a time, the flagged ones in order
            const uint32_t lo = rows[tab.row0[l]], hi = l + 1 < tab.n_levels ? rows[tab.row0[l + 1]] : nc;
            for (uint32_t c0 = lo; c0 < hi; c0 += 64) {
                uint64_t bal = __ballot(c0 + lane < hi && big[c0 + lane] != 0u);
                while (bal) {
                    const uint32_t k = (uint32_t)__builtin_ctzll(bal);
                    bal &= bal - 1ull;
                    step(c0 + k);
                }
            }
        }
    }
    if (!kMembers) {
        if (lane == 0) n_slots[b] = n;
    } else {
        uint32_t* fin = cc.fin + (size_t)b * cand_stride;
        uint32_t* opn = cc.opn + (size_t)b * cand_stride;
        for (uint32_t q = lane; q < n; q += 64) { fin[bopen[q]] = sl[q].pad; opn[bopen[q]] = 1u; }
    }
}

// ---- The same rule, in parallel: connected components (the argument of the Fast arm's in-level pruning,
// section 4.8, over two levels).  A level-l candidate p reads only slots of class l - 1 or l whose position lies within size_l of p's
// scaled position, and a slot always holds the position and class of the last candidate written into it.  So link p to every EARLIER
// candidate q of level l - 1 or l that passes the rule's own float predicate against q's converted position: every interaction of the
// serial rule is then an edge (extra edges do no harm).  A candidate that fails the descriptor-border test never changes kpts_aux and
// is dropped before linking.  A slot never leaves its component and no component reads another's slots, so "first slot in list order"
// is the first slot of the component in the order its candidates opened them, and a slot's global index is the running count of the
// openers in scan order -- the order the serial rule appends in.
//   init      per candidate: parent = itself, or none when the border test fails
//   link      union-find over the earlier candidates of the rows within reach (the row offsets of ac_scan_rows, both levels)
//   flatten   root (the component's smallest index) and member count (no path halving here: see the kernel)
//   classify  a lone candidate opens its slot on the spot; a component of <= bound members gets a bucket (bucket sizes, scanned);
//             the members of a larger one are flagged for the hand-back (ac_aux_kernel<true>)
//   gather    members into their buckets (any order; the wavefront sorts them)
//   small     one wavefront per bucketed component: members sorted into scan order, slots in registers (lane = slot, in opening order)
//   emit      opener flags scanned (ac_scan_rows) = slot indices; every slot written from its last writer
// All hand-overs between kernels go through the stream order; inside the small kernel they are cross-lane shuffles.
__device__ __forceinline__ uint32_t ac_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ac_uf_find(uint32_t* par, uint32_t x)
{
    for (;;) {
        const uint32_t p = ac_ld(par + x);
        if (p == x) return x;
        const uint32_t g = ac_ld(par + p);
        if (g == p) return p;
        __hip_atomic_store(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // path halving: g is an ancestor of x whatever else happens
        x = g;
    }
}
__device__ __forceinline__ void ac_uf_union(uint32_t* par, uint32_t a, uint32_t b)
{
    for (;;) {
        a = ac_uf_find(par, a); b = ac_uf_find(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }                                // the later root goes under the earlier one: no cycle
        if (atomicCAS(par + a, a, b) == a) return;
    }
}
__device__ __forceinline__ bool ac_is_out(const AcLevelTab& tab, const AcCand& k)
{
    const int l = (int)k.level;
    const float size = tab.esigma[l] * 1.5f, ratio = tab.ratio[l];
    const float r = tab.smax * (float)ac_fround(size / ratio);
    const float px = (float)k.x, py = (float)k.y;
    return ac_fround(px - r) - 1 < 0 || ac_fround(px + r) + 1 >= tab.w[l] || ac_fround(py - r) - 1 < 0 || ac_fround(py + r) + 1 >= tab.h[l];
}
__device__ __forceinline__ float ac_conv(float v, float ratio, float off) { return (float)((double)(v * ratio) + (double)off); }

__global__ __launch_bounds__(256)
void ac_cc_init_kernel(const AcCand* __restrict__ cand, uint32_t stride, const uint32_t* __restrict__ totals, AcLevelTab tab, AcCc cc)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= stride) return;
    const size_t at = (size_t)b * stride + i;
    const bool in = i < totals[b] && !ac_is_out(tab, cand[at]);
    cc.par[at] = in ? i : kNone;
    cc.csz[at] = 0u; cc.boff[at] = 0u; cc.cur[at] = 0u; cc.opn[at] = 0u; cc.big[at] = 0u; cc.fin[at] = kNone;
    if (i == 0) cc.n_big[b] = 0u;
}
__global__ __launch_bounds__(256)
void ac_cc_link_kernel(const AcCand* __restrict__ cand, uint32_t stride, const uint32_t* __restrict__ totals, AcLevelTab tab, AcCc cc)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= totals[b]) return;
    const AcCand* cb = cand + (size_t)b * stride;
    uint32_t* par = cc.par + (size_t)b * stride;
    if (par[i] == kNone) return;                              // (fixed since init: unions only move roots)
    const uint32_t* rows = cc.rows + (size_t)b * cc.rows_stride;
    const AcCand k = cb[i];
    const int l = (int)k.level;
    const float size = tab.esigma[l] * 1.5f, s2 = size * size, ratio = tab.ratio[l];
    const float sx = (float)k.x * ratio, sy = (float)k.y * ratio;
    for (int m = l > 0 ? l - 1 : l; m <= l; ++m) {
        const float rm = tab.ratio[m], om = tab.off[m];
        // level-m rows and columns whose converted position can lie within size (one spare row / column on each side)
        const int ylo = max(1, (int)floorf((sy - size - om) / rm) - 1), yhi = min(tab.h[m] - 2, (int)ceilf((sy + size - om) / rm) + 1);
        const uint32_t xlo = (uint32_t)max(1, (int)floorf((sx - size - om) / rm) - 1);
        const int xhi = (int)ceilf((sx + size - om) / rm) + 1;
        for (int y = ylo; y <= yhi; ++y) {
            uint32_t j = rows[tab.row0[m] + y], je = rows[tab.row0[m] + y + 1];
            if (m == l && je > i) je = i;                         // only earlier candidates
            uint32_t a = j, z = je;                               // first column >= xlo
            while (a < z) { const uint32_t h = (a + z) >> 1; if (cb[h].x < xlo) a = h + 1; else z = h; }
            for (j = a; j < je && (int)cb[j].x <= xhi; ++j) {
                if (par[j] == kNone) continue;
                const float tx = sx - ac_conv((float)cb[j].x, rm, om), ty = sy - ac_conv((float)cb[j].y, rm, om);
                if (tx * tx + ty * ty <= s2) ac_uf_union(par, i, j);
            }
        }
    }
}
__global__ __launch_bounds__(256)
void ac_cc_flatten_kernel(uint32_t stride, const uint32_t* __restrict__ totals, AcCc cc)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= totals[b]) return;
    uint32_t* par = cc.par + (size_t)b * stride;
    if (ac_ld(par + i) == kNone) return;
    // a walk WITHOUT path halving: a halving find of another lane could otherwise put a mere ancestor back over a root stored here,
    // and that member would miss its component's bucket.  The only stores now are par[i] = root, so every chain a lane follows stays
    // one of ancestors.
    uint32_t r = i;
    for (uint32_t p = ac_ld(par + r); p != r; p = ac_ld(par + r)) r = p;
    if (r != i) __hip_atomic_store(par + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(cc.csz + (size_t)b * stride + r, 1u);
}
__global__ __launch_bounds__(256)
void ac_cc_classify_kernel(uint32_t stride, const uint32_t* __restrict__ totals, AcCc cc, uint32_t bound)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= totals[b]) return;
    const size_t o = (size_t)b * stride;
    const uint32_t r = cc.par[o + i];
    if (r == kNone) return;
    const uint32_t s = cc.csz[o + r];
    if (s == 1u) { cc.fin[o + i] = i; cc.opn[o + i] = 1u; }           // a lone candidate opens its slot on the spot
    else if (s <= bound) { if (r == i) cc.boff[o + i] = s; }
    else { cc.big[o + i] = 1u; if (r == i) atomicAdd(cc.n_big + b, s); }
    if (r == i && cc.hist) atomicAdd(cc.hist + 32u * b + (31u - (uint32_t)__builtin_clz(s)), 1u);   // bin k: sizes in [2^k, 2^(k+1))
}
__global__ __launch_bounds__(256)
void ac_cc_gather_kernel(uint32_t stride, const uint32_t* __restrict__ totals, AcCc cc, uint32_t bound)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= totals[b]) return;
    const size_t o = (size_t)b * stride;
    const uint32_t r = cc.par[o + i];
    if (r == kNone) return;
    const uint32_t s = cc.csz[o + r];
    if (s < 2u || s > bound) return;
    cc.memb[o + cc.boff[o + r] + atomicAdd(cc.cur + o + r, 1u)] = i;
}
__global__ __launch_bounds__(256)
void ac_cc_small_kernel(const AcCand* __restrict__ cand, uint32_t stride, const uint32_t* __restrict__ totals, AcLevelTab tab, AcCc cc,
                        uint32_t bound)
{
    const uint32_t b = blockIdx.y, lane = threadIdx.x & 63u, wave = (blockIdx.x * 256u + threadIdx.x) >> 6, n_waves = gridDim.x * 4u;
    const uint32_t nc = totals[b];
    const size_t o = (size_t)b * stride;
    const AcCand* cb = cand + o;
    for (uint32_t c0 = wave * 64u; c0 < nc; c0 += n_waves * 64u) {
        const uint32_t i = c0 + lane;
        const bool root = i < nc && cc.par[o + i] == i;
        const uint32_t sz = root ? cc.csz[o + i] : 0u;
        uint64_t todo = __ballot(sz >= 2u && sz <= bound);
        while (todo) {
            const int bit = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t r = c0 + (uint32_t)bit, n = (uint32_t)__shfl((int)sz, bit);
            // the members, sorted into scan order (bitonic over the wavefront; the empty lanes sort last)
            uint32_t mem = lane < n ? cc.memb[o + cc.boff[o + r] + lane] : kNone;
#pragma unroll
            for (uint32_t k = 2; k <= 64; k <<= 1)
#pragma unroll
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    const uint32_t other = (uint32_t)__shfl_xor((int)mem, (int)j);
                    const bool up = (lane & k) == 0, low = (lane & j) == 0;
                    mem = (low == up) ? (mem < other ? mem : other) : (mem > other ? mem : other);
                }
            // lane q = slot q of the component, in opening order
            float qx = 0.f, qy = 0.f, qr = 0.f; uint32_t qcls = 0u, qwr = 0u, qop = 0u, n_open = 0u;
            for (uint32_t t = 0; t < n; ++t) {
                const uint32_t ci = (uint32_t)__shfl((int)mem, (int)t);
                const AcCand k = cb[ci];
                const uint32_t l = k.level;
                const float size = tab.esigma[l] * 1.5f, s2 = size * size, ratio = tab.ratio[l];
                const float sx = (float)k.x * ratio, sy = (float)k.y * ratio;
                const float tx = sx - qx, ty = sy - qy;
                const uint64_t bal = __ballot(lane < n_open && (qcls == l || qcls + 1u == l) && tx * tx + ty * ty <= s2);
                const float nx = (float)((double)sx + (double)tab.off[l]), ny = (float)((double)sy + (double)tab.off[l]);
                if (bal) {
                    const int f = __builtin_ctzll(bal);
                    if (k.value > __shfl(qr, f) && (int)lane == f) { qx = nx; qy = ny; qr = k.value; qcls = l; qwr = ci; }
                } else {
                    if (lane == n_open) { qx = nx; qy = ny; qr = k.value; qcls = l; qwr = ci; qop = ci; }
                    ++n_open;
                }
            }
            if (lane < n_open) { cc.fin[o + qop] = qwr; cc.opn[o + qop] = 1u; }
        }
    }
}
// opn holds the slot index of every opener now (exclusive scan); its slot takes the last candidate written into it
__global__ __launch_bounds__(256)
void ac_cc_emit_kernel(const AcCand* __restrict__ cand, uint32_t stride, const uint32_t* __restrict__ totals, AcLevelTab tab, AcCc cc,
                       AcSlot* __restrict__ slots)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= totals[b]) return;
    const size_t o = (size_t)b * stride;
    const uint32_t w = cc.fin[o + i];
    if (w == kNone) return;
    const AcCand k = cand[o + w];
    const uint32_t l = k.level;
    const float ratio = tab.ratio[l];
    slots[o + cc.opn[o + i]] = AcSlot{ac_conv((float)k.x, ratio, tab.off[l]), ac_conv((float)k.y, ratio, tab.off[l]), tab.esigma[l] * 1.5f, k.value, l, 0u};
}

// ---- the upper-level filter's buckets: the slots of class k >= 1 in linked cell lists of side G_k = floor(size_{k-1}) + 1 > size_{k-1},
// so a slot of class k - 1 finds every slot of class k within its size in the 3 x 3 cells around it (the walk's own argument)
__global__ __launch_bounds__(256)
void ac_up_insert_kernel(const AcSlot* __restrict__ slots, uint32_t stride, const uint32_t* __restrict__ n_slots, AcUpGrid ug)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_slots[b]) return;
    const AcSlot s = slots[(size_t)b * stride + i];
    if (s.cls == 0u) return;
    const int G = ug.G[s.cls], gw = ug.img_w / G + 2;
    int* heads = ug.heads + (size_t)b * ug.cells_stride + ug.cell_off[s.cls];
    ug.next[(size_t)b * stride + i] = atomicExch(&heads[ac_cell_of(s.y, G) * gw + ac_cell_of(s.x, G)], (int)i);
}

// ---- upper-level filter (AKAZE.cpp:352-381), one lane per slot: slot i goes if a LATER slot of class + 1 lies within slot i's size
// and responds more strongly.  Then Do_Subpixel_Refinement (:389-460) and Compute_Main_Orientation (:563-625) for the kept slots.
__constant__ float c_ac_gauss25[7][7] = {
    { 0.02546481f, 0.02350698f, 0.01849125f, 0.01239505f, 0.00708017f, 0.00344629f, 0.00142946f },
    { 0.02350698f, 0.02169968f, 0.01706957f, 0.01144208f, 0.00653582f, 0.00318132f, 0.00131956f },
    { 0.01849125f, 0.01706957f, 0.01342740f, 0.00900066f, 0.00514126f, 0.00250252f, 0.00103800f },
    { 0.01239505f, 0.01144208f, 0.00900066f, 0.00603332f, 0.00344629f, 0.00167749f, 0.00069579f },
    { 0.00708017f, 0.00653582f, 0.00514126f, 0.00344629f, 0.00196855f, 0.00095820f, 0.00039744f },
    { 0.00344629f, 0.00318132f, 0.00250252f, 0.00167749f, 0.00095820f, 0.00046640f, 0.00019346f },
    { 0.00142946f, 0.00131956f, 0.00103800f, 0.00069579f, 0.00039744f, 0.00019346f, 0.00008024f } };

// cv::fastAtan2 (OpenCV 4 atan_f32), degrees
__device__ __forceinline__ float ac_fast_atan2_deg(float y, float x)
{
    const float p1 = 0.9997878412794807f * (float)(180 / 3.1415926535897932384626433832795);
    const float p3 = -0.3258083974640975f * (float)(180 / 3.1415926535897932384626433832795);
    const float p5 = 0.1555786518463281f * (float)(180 / 3.1415926535897932384626433832795);
    const float p7 = -0.04432655554792128f * (float)(180 / 3.1415926535897932384626433832795);
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) { c = ay / (ax + (float)2.220446049250313e-16); c2 = c * c; a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c; }
    else { c = ax / (ay + (float)2.220446049250313e-16); c2 = c * c; a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c; }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

__global__ __launch_bounds__(256)
void ac_finish_kernel(const AcSlot* __restrict__ slots, uint32_t stride, const uint32_t* __restrict__ n_slots, AcLevelTab tab,
                      AcPlanes pl, AcOut* __restrict__ out, AcUpGrid ug)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = n_slots[b];
    if (i >= n) return;
    const AcSlot* sl = slots + (size_t)b * stride;
    AcOut& o = out[(size_t)b * stride + i];
    o.ok = 0;
    const AcSlot p = sl[i];
    const float p2 = p.size * p.size;
    auto drops = [&](uint32_t j) {
        const AcSlot q = sl[j];
        if (q.cls != p.cls + 1) return false;
        const float tx = p.x - q.x, ty = p.y - q.y;
        return tx * tx + ty * ty <= p2 && p.resp < q.resp;
    };
    if (!ug.heads) {                                                  // (the developer build's R3DM_AC_AUX=0: every later slot)
        for (uint32_t j = i + 1; j < n; ++j) if (drops(j)) return;
    } else if ((int)p.cls + 1 < tab.n_levels) {
        // the later slots of class + 1 in the 3 x 3 cells around the slot (ac_up_insert_kernel)
        const uint32_t k = p.cls + 1;
        const int G = ug.G[k], gw = ug.img_w / G + 2, gh = ug.img_h / G + 2;
        const int* heads = ug.heads + (size_t)b * ug.cells_stride + ug.cell_off[k];
        const int* next = ug.next + (size_t)b * stride;
        const int cx = ac_cell_of(p.x, G), cy = ac_cell_of(p.y, G);
        for (int y = max(cy - 1, 0); y <= min(cy + 1, gh - 1); ++y)
            for (int x = max(cx - 1, 0); x <= min(cx + 1, gw - 1); ++x)
                for (int j = heads[y * gw + x]; j >= 0; j = next[j])
                    if ((uint32_t)j > i && drops((uint32_t)j)) return;
    }
    const int l = (int)p.cls, w = tab.w[l];
    const size_t plane = (size_t)tab.w[l] * tab.h[l] * b;
    const float* L = pl.ldet[l] + plane;
    const float ratio = tab.ratio[l];
    const int x = ac_fround(p.x / ratio), y = ac_fround(p.y / ratio);
    const float* r0 = L + (size_t)y * w + x;
    const float c = r0[0], le = r0[-1], ri = r0[1], up = r0[-w], dn = r0[w];
    // the reference's expressions carry double constants: formed in double as written, stored as float
    const float Dx = (float)(0.5 * (double)(ri - le));
    const float Dy = (float)(0.5 * (double)(dn - up));
    const float Dxx = (float)((double)(ri + le) - 2.0 * (double)c);
    const float Dyy = (float)((double)(dn + up) - 2.0 * (double)c);
    const float Dxy = (float)(0.25 * (double)(r0[w + 1] + r0[-w - 1]) - 0.25 * (double)(r0[-w + 1] + r0[w - 1]));
    // cv::solve, 2 x 2, DECOMP_LU: Cramer's rule in double (core/lapack.cpp), 0 when singular
    float dx = 0.0f, dy = 0.0f;
    {
        const float b0 = -Dx, b1 = -Dy;
        double d = (double)Dxx * Dyy - (double)Dxy * Dxy;
        if (d != 0.) {
            d = 1. / d;
            const double t = (float)(((double)b0 * Dyy - (double)b1 * Dxy) * d);
            dy = (float)(((double)b1 * Dxx - (double)b0 * Dxy) * d);
            dx = (float)t;
        }
    }
    if (fabsf(dx) > 1.0f || fabsf(dy) > 1.0f) return;               // erased: not stable
    const int power = 1 << tab.octave[l];
    const float kx = (float)((double)(((float)x + dx) * (float)power) + 0.5 * (power - 1));
    const float ky = (float)((double)(((float)y + dy) * (float)power) + 0.5 * (power - 1));
    const float size = p.size * 2.0f;
    // Compute_Main_Orientation on the level's multiscale Lx / Ly
    const int s = ac_fround((float)(0.5 * (double)size / (double)ratio));
    const float xf = kx / ratio, yf = ky / ratio;
    const float* Lx = pl.lx[l] + plane;
    const float* Ly = pl.ly[l] + plane;
    float resX[109], resY[109], Ang[109];
    const int id[13] = {6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6};
    int idx = 0;
    for (int ii = -6; ii <= 6; ++ii)
        for (int jj = -6; jj <= 6; ++jj)
            if (ii * ii + jj * jj < 36) {
                const int iy = ac_fround(yf + (float)(jj * s)), ix = ac_fround(xf + (float)(ii * s));
                const float gw = c_ac_gauss25[id[ii + 6]][id[jj + 6]];
                resX[idx] = gw * Lx[(size_t)iy * w + ix];
                resY[idx] = gw * Ly[(size_t)iy * w + ix];
                Ang[idx] = (float)((double)ac_fast_atan2_deg(resY[idx], resX[idx]) * (3.1415926535897932384626433832795 / 180.0));
                ++idx;
            }
    const double PI = 3.1415926535897932384626433832795;
    float best = 0.0f, angle = 0.0f;
    for (float ang1 = 0.0f; (double)ang1 < 2.0 * PI; ang1 += 0.15f) {
        const float ang2 = (float)((double)ang1 + PI / 3.0f > 2.0 * PI ? (double)ang1 - 5.0f * PI / 3.0f : (double)ang1 + PI / 3.0f);
        float sumX = 0.0f, sumY = 0.0f;
        for (int k = 0; k < 109; ++k) {
            const float ang = Ang[k];
            if (ang1 < ang2 && ang1 < ang && ang < ang2) { sumX += resX[k]; sumY += resY[k]; }
            else if (ang2 < ang1 && ((ang > 0 && ang < ang2) || (ang > ang1 && (double)ang < 2.0 * PI))) { sumX += resX[k]; sumY += resY[k]; }
        }
        if (sumX * sumX + sumY * sumY > best) {
            best = sumX * sumX + sumY * sumY;
            angle = (float)((double)ac_fast_atan2_deg(sumY, sumX) * (PI / 180.0));
        }
    }
    // radians -> degrees in double, 360 wrapped to 0 (no + 90 on this arm)
    float deg = (float)((double)angle * (180.0 / PI));
    if (deg >= 360.0f) deg = deg - 360.0f;
    o = AcOut{kx, ky, size, deg, p.resp, 1u, 0u, 0u};
}

}  // namespace

// ------------------------------------------------------------------------------------------------ launchers
static dim3 ac_grid(int w, int h, int B) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)B); }

hipError_t ac_kcontrast(hipStream_t st, const float* smooth1, int w, int h, int B, uint32_t* small)
{
    if (w >= 3 && h >= 3) {
        hipLaunchKernelGGL(ac_kc_hist_kernel, dim3((unsigned)((w - 2 + 63) / 64), (unsigned)std::min((h - 2 + 3) / 4, 64), (unsigned)B), dim3(256), 0, st,
                           smooth1, w, h, small, small + 16);
    }
    hipLaunchKernelGGL(ac_kc_finish_kernel, dim3((unsigned)B), dim3(1), 0, st, small);
    return hipGetLastError();
}
hipError_t ac_fed_step(hipStream_t st, const float* Lt, const float* Lf, float* out, int w, int h, int B, float half_step)
{
    hipLaunchKernelGGL(ac_fed_step_kernel, ac_grid(w, h, B), dim3(256), 0, st, Lt, Lf, out, w, h, half_step);
    return hipGetLastError();
}
hipError_t ac_hessian(hipStream_t st, const float* smooth, float* Lx, float* Ly, float* Ldet, int w, int h, int B, int s, float norm, float kc)
{
    const AcTaps t{norm, kc, s};
    hipLaunchKernelGGL(ac_deriv_xy_kernel, ac_grid(w, h, B), dim3(256), 0, st, smooth, Lx, Ly, w, h, t);
    hipLaunchKernelGGL(ac_deriv_det_kernel, ac_grid(w, h, B), dim3(256), 0, st, Lx, Ly, Ldet, w, h, t, (float)(s * s * s * s));
    return hipGetLastError();
}
hipError_t ac_extrema(hipStream_t st, const float* ldet, int w, int h, int B, float thr, uint32_t* row_counts, uint32_t rows_stride,
                      uint32_t row0, AcCand* cand, uint32_t cand_stride, int level, int pass)
{
    if (h < 3 || w < 3) return hipSuccess;
    hipLaunchKernelGGL(ac_extrema_kernel, dim3((unsigned)(h - 2), 1, (unsigned)B), dim3(64), 0, st, ldet, w, h, thr, row_counts, rows_stride,
                       row0, cand, cand_stride, level, pass);
    return hipGetLastError();
}
hipError_t ac_scan_rows(hipStream_t st, uint32_t* row_counts, uint32_t rows_stride, uint32_t n_rows, int B, uint32_t* totals)
{
    hipLaunchKernelGGL(ac_scan_rows_kernel, dim3((unsigned)B), dim3(1024), 0, st, row_counts, rows_stride, n_rows, totals);
    return hipGetLastError();
}
hipError_t ac_aux(hipStream_t st, const AcCand* cand, uint32_t cand_stride, const uint32_t* totals, const AcLevelTab& tab, AcSlot* slots,
                  const AcGrid& grid, uint32_t* n_slots, int B)
{
    hipLaunchKernelGGL(ac_aux_kernel<false>, dim3((unsigned)B), dim3(64), 0, st, cand, cand_stride, totals, tab, slots, grid, n_slots, AcCc{});
    return hipGetLastError();
}
hipError_t ac_aux_parallel(hipStream_t st, const AcCand* cand, uint32_t stride, const uint32_t* totals, const AcLevelTab& tab, AcSlot* slots,
                           const AcGrid& grid, uint32_t* n_slots, const AcCc& cc, uint32_t bound, int B)
{
    const dim3 g((stride + 255) / 256, (unsigned)B);
    const uint32_t small_blocks = std::min<uint32_t>((stride + 255) / 256, 1024u);
    hipLaunchKernelGGL(ac_cc_init_kernel, g, dim3(256), 0, st, cand, stride, totals, tab, cc);
    hipLaunchKernelGGL(ac_cc_link_kernel, g, dim3(256), 0, st, cand, stride, totals, tab, cc);
    hipLaunchKernelGGL(ac_cc_flatten_kernel, g, dim3(256), 0, st, stride, totals, cc);
    hipLaunchKernelGGL(ac_cc_classify_kernel, g, dim3(256), 0, st, stride, totals, cc, bound);
    hipLaunchKernelGGL(ac_scan_rows_kernel, dim3((unsigned)B), dim3(1024), 0, st, cc.boff, stride, stride, cc.scratch);
    hipLaunchKernelGGL(ac_cc_gather_kernel, g, dim3(256), 0, st, stride, totals, cc, bound);
    hipLaunchKernelGGL(ac_cc_small_kernel, dim3(small_blocks, (unsigned)B), dim3(256), 0, st, cand, stride, totals, tab, cc, bound);
    hipLaunchKernelGGL(ac_aux_kernel<true>, dim3((unsigned)B), dim3(64), 0, st, cand, stride, totals, tab, slots, grid, n_slots, cc);
    hipLaunchKernelGGL(ac_scan_rows_kernel, dim3((unsigned)B), dim3(1024), 0, st, cc.opn, stride, stride, n_slots);
    hipLaunchKernelGGL(ac_cc_emit_kernel, g, dim3(256), 0, st, cand, stride, totals, tab, cc, slots);
    return hipGetLastError();
}
hipError_t ac_finish(hipStream_t st, const AcSlot* slots, uint32_t stride, const uint32_t* n_slots, const AcLevelTab& tab, const AcPlanes& pl,
                     AcOut* out, uint32_t max_slots, int B, const AcUpGrid& ug)
{
    if (max_slots == 0) return hipSuccess;
    if (ug.heads) hipLaunchKernelGGL(ac_up_insert_kernel, dim3((max_slots + 255) / 256, (unsigned)B), dim3(256), 0, st, slots, stride, n_slots, ug);
    hipLaunchKernelGGL(ac_finish_kernel, dim3((max_slots + 255) / 256, (unsigned)B), dim3(256), 0, st, slots, stride, n_slots, tab, pl, out, ug);
    return hipGetLastError();
}

}  // namespace r3dm
