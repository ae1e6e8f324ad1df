// kernels_match.hip -- putative matching on gfx950 (MI355X): staging of a view and the fused squared-L2 2-NN on FP32 MFMA tiles
// (the headline kernel).  Siblings: kernels_match_16bit.hip (bf16 / f16 nominators), kernels_match_hamming.hip (binary descriptors),
// kernels_match_exact.hip (exact scans, per-pair finalisation), kernels_match_knn.hip / kernels_match_knn16.hip (k-NN); shared device
// helpers in kernels_match_common.hpp; the tile steps of every MFMA nominator, their list interface, the buffer descriptor and the
// launchers' grid in kernels_match_tiles.hpp.
//
// What it replaces in the reference (rhiestan/Regard3D, /root/reference):
//   Matcher_Regions(fDistRatio, BRUTE_FORCE_L2).Match()    src/R3DComputeMatches.cpp:2037-2039,2048
//   per-I / OpenMP-over-J loop nest                          src/R3DComputeMatches.cpp:437-489
//   ArrayMatcher::SearchNeighbours(NN=2) + MatchDistanceRatio  src/utils/matcher_kgraph.h:205-251,
//                                                            src/R3DComputeMatches.cpp:479
// Arithmetic contract (OpenMVG L2<float>): distances are the f32
// 4-way-unrolled sum of squared differences, NO fused multiply-add; equal distances -> lowest
// dataset row.  The MFMA pass only nominates candidates (||a||^2 - 2 a.b, any summation order); the
// two best candidates are re-scored with the reference arithmetic, and a query whose runner-up is
// not provably separated from every un-nominated row is redone by an exact scan (kFallback).
//
// This file is compiled with -ffp-contract=off; fused operations are spelled fmaf()/MFMA.


#include "kernels_match_tiles.hpp"

namespace r3dm {

// ------------------------------------------------------------------------------------------------
// staging (registration of a view: what Regions_Provider::load is to the reference, /root/reference/src/R3DComputeMatches.cpp:2040,2094)
// ONE kernel per view on the default path: the raw row-major descriptors (f32, or u8 converted on the way) are read ONCE -- from the
// upload ring's device slot, from the caller's device buffer, or straight from page-locked host memory over the link -- and leave as
// the MFMA fragment-order tiles + norms + the view's statistics; the row-major f32 copy (`rows`) is written only when asked for
// (a view of integer-valued bins never needs it: its MFMA keys ARE the reference distances, and the exact scan reads the tiles).
// Every other layout (bf16 tiles, split-f16 planes, count tiles, byte tiles) is staged on first use by the path that reads it
// (api_core.cpp: ensure_layouts).
// ------------------------------------------------------------------------------------------------

// role blocks behind the n_tiles tile blocks -- one per 256 features, at least 8: they copy the positions, enter them into the
// position-class hash table (IndMatchDecorator's coordinate de-duplication needs to know which features share a position; one
// compare-and-swap + one minimum per feature, a thread each) and zero the slack
__host__ __device__ inline uint32_t stage_aux_blocks(uint32_t n) { const uint32_t b = (n + 255u) / 256u; return b < 8u ? 8u : (b > 1024u ? 1024u : b); }

__device__ __forceinline__ bool canon_key_of(float fx, float fy, unsigned long long& key)
{
    if (fx != fx || fy != fy) return false;                          // NaN: equals nothing, itself included -> a class of its own
    const float zx = fx == 0.0f ? 0.0f : fx, zy = fy == 0.0f ? 0.0f : fy;      // -0 folded into +0: equal floats <-> equal bit patterns
    key = ((unsigned long long)__float_as_uint(zx) << 32) | __float_as_uint(zy);
    return true;
}
__device__ __forceinline__ uint32_t canon_hash(unsigned long long key, uint32_t bits)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}

__device__ __forceinline__ void stage_aux_role(const StageViewArgs& A, uint32_t rb, uint32_t n_role_blocks)
{
    const uint32_t n = A.n, G = A.G;
    const uint32_t nthr = n_role_blocks * 256u, tid = rb * 256u + threadIdx.x;
    if (A.xy_src) {
        const unsigned long long kEmpty = ~0ull;
        const uint32_t mask = (1u << A.canon_bits) - 1u;
        for (uint32_t k = tid; k < n; k += nthr) {
            const float fx = A.xy_src[2 * (size_t)k], fy = A.xy_src[2 * (size_t)k + 1];
            if (A.xy_dst != A.xy_src) { A.xy_dst[2 * (size_t)k] = fx; A.xy_dst[2 * (size_t)k + 1] = fy; }
            unsigned long long key;
            if (A.canon_keys && canon_key_of(fx, fy, key)) {
                uint32_t slot = canon_hash(key, A.canon_bits) & mask;
                for (;;) {
                    const unsigned long long old = atomicCAS(A.canon_keys + slot, kEmpty, key);
                    if (old == kEmpty || old == key) { atomicMin(A.canon_vals + slot, k); break; }
                    slot = (slot + 1u) & mask;
                }
            }
        }
    }
    // zero slack behind the tiles and the norms (prefetches run past the end; a recycled buffer holds an older view there)
    if (A.tiled) {
        float* ts = A.tiled + (size_t)A.n_tiles * G * 256u;
        for (uint32_t e = tid; e < kSlackBytes / 4u; e += nthr) ts[e] = 0.0f;
        float* ns = A.norms + (size_t)A.n_tiles * 32u;
        for (uint32_t e = tid; e < kSlackBytes / 4u; e += nthr) ns[e] = 0.0f;
        float* ps = A.norms + prefix_norm_offset(A.n_tiles) + (size_t)A.n_tiles * 32u;      // ... and behind the prefix norms
        for (uint32_t e = tid; e < kSlackBytes / 4u; e += nthr) ps[e] = 0.0f;
    }
}

// one workgroup per 32-row tile (+ the role blocks)
__global__ __launch_bounds__(256)
void stage_view_kernel(const StageViewArgs A)
{
    __shared__ float sm[32 * 260];                     // the tile's rows, row stride dim + 4 floats (dim <= 256 staged through LDS)
    const uint32_t n = A.n, dim = A.dim, G = A.G;
    // (the role blocks come first: their atomics' round trips run beside the tile blocks' copies)
    const uint32_t n_role = gridDim.x - A.n_tiles;
    if (blockIdx.x < n_role) { stage_aux_role(A, blockIdx.x, n_role); return; }
    const uint32_t t = blockIdx.x - n_role;
    const uint32_t rows_here = (n - t * 32u < 32u) ? n - t * 32u : 32u;
    const uint32_t per_tile = G * 256u;                // floats per tile = G * 2 * 32 * 4
    float* dst = A.tiled + (size_t)t * per_tile;
    const bool lds = dim <= 256u && (dim & 3u) == 0u && (((uintptr_t)A.raw) & (A.raw_is_u8 ? 3u : 15u)) == 0u;
    const uint32_t stride = dim + 4u;
    if (lds) {
        // coalesced read of the tile's rows_here x dim values (contiguous in the raw image), converted, into LDS: thread (ty, tx) walks
        // rows ty, ty + 8, ... and the 4-element chunks tx, tx + 32, ... of a row
        const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5, d4 = dim >> 2;
        if (A.raw_is_u8) {
            const uint32_t* src = (const uint32_t*)((const uint8_t*)A.raw + (size_t)t * 32u * dim);     // dim % 4 == 0: 4-byte aligned
            for (uint32_t r = ty; r < rows_here; r += 8u)
                for (uint32_t k4 = tx; k4 < d4; k4 += 32u) {
                    const uint32_t w = src[r * d4 + k4];
                    *(f32x4*)(sm + r * stride + 4u * k4) = f32x4{(float)(w & 255u), (float)((w >> 8) & 255u), (float)((w >> 16) & 255u), (float)(w >> 24)};
                }
        } else {
            const f32x4* src = (const f32x4*)((const float*)A.raw + (size_t)t * 32u * dim);
            for (uint32_t r = ty; r < rows_here; r += 8u)
                for (uint32_t k4 = tx; k4 < d4; k4 += 32u) *(f32x4*)(sm + r * stride + 4u * k4) = src[r * d4 + k4];
        }
        __syncthreads();
        if (A.rows) {
            f32x4* ro = (f32x4*)(A.rows + (size_t)t * 32u * dim);
            for (uint32_t r = ty; r < rows_here; r += 8u)
                for (uint32_t k4 = tx; k4 < d4; k4 += 32u) ro[r * d4 + k4] = *(const f32x4*)(sm + r * stride + 4u * k4);
        }
        // fragment order: float4 (g, h, r) = row 32 t + r, dims 8 g + 4 h .. + 3
        for (uint32_t e4 = threadIdx.x; e4 < per_tile / 4u; e4 += 256u) {
            const uint32_t r = e4 & 31u, k = (e4 >> 5) * 4u;            // (g, h) = e4 >> 5: dims 8 g + 4 h = 4 (e4 >> 5)
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r < rows_here && k < dim) v = *(const f32x4*)(sm + r * stride + k);
            ((f32x4*)dst)[e4] = v;
        }
    } else {
        // any other descriptor length: element by element from the raw image
        for (uint32_t e = threadIdx.x; e < per_tile; e += 256u) {
            const uint32_t c = e & 3u, r = (e >> 2) & 31u, h = (e >> 7) & 1u, g = e >> 8;
            const uint32_t row = t * 32u + r, k = 8u * g + 4u * h + c;
            float v = 0.0f;
            if (row < n && k < dim) v = A.raw_is_u8 ? (float)((const uint8_t*)A.raw)[(size_t)row * dim + k] : ((const float*)A.raw)[(size_t)row * dim + k];
            dst[e] = v;
            if (A.rows && row < n && k < dim) A.rows[(size_t)row * dim + k] = v;
        }
    }
    if (threadIdx.x < 32u) {
        const uint32_t row = t * 32u + threadIdx.x;
        float s = R3DM_INF, sp = R3DM_INF;             // sp: the chain below after A.prefix_dims elements (the whole of a shorter row)
        if (row < n) {
            s = 0.0f;
            float mx = 0.0f; bool nonint = false, neg = false;
            // ||row||^2 as ONE fma chain in element order (the accumulators' C operand; what rounds 1-5 computed), four elements per LDS read
            auto take = [&](float v) {
                s = fmaf(v, v, s);
                mx = fmaxf(mx, fabsf(v));
                nonint |= !(v == rintf(v));                  // also true for NaN
                neg |= v < 0.0f;
            };
            if (lds) {
                const float* p = sm + threadIdx.x * stride;
                for (uint32_t k = 0; k < dim; k += 4u) {
                    if (k == A.prefix_dims) sp = s;
                    const f32x4 v = *(const f32x4*)(p + k); take(v[0]); take(v[1]); take(v[2]); take(v[3]);
                }
            } else {
                for (uint32_t k = 0; k < dim; ++k) {
                    if (k == A.prefix_dims) sp = s;
                    take(A.raw_is_u8 ? (float)((const uint8_t*)A.raw)[(size_t)row * dim + k] : ((const float*)A.raw)[(size_t)row * dim + k]);
                }
            }
            if (dim <= A.prefix_dims) sp = s;
            // img_stats = &ImgDev::max_norm_bits, max_abs_bits, not_integer (non-negative floats order like uints)
            atomicMax(A.img_stats + 0, __float_as_uint(s));
            atomicMax(A.img_stats + 1, __float_as_uint(mx));
            if (nonint) atomicOr(A.img_stats + 2, 1u);     // ImgDev::not_integer: bit 0 = some non-integer, bit 1 = some negative
            if (neg) atomicOr(A.img_stats + 2, 2u);
        }
        A.norms[(size_t)t * 32u + threadIdx.x] = s;
        A.norms[prefix_norm_offset(A.n_tiles) + (size_t)t * 32u + threadIdx.x] = sp;
    }
}

// position classes, second pass (behind stage_view_kernel's inserts): canon[k] = the smallest feature index at k's position;
// *has_dup is set when some feature is not the first of its class
__global__ __launch_bounds__(256)
void canon_lookup_kernel(const float* __restrict__ xy, uint32_t n, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals,
                         uint32_t bits, uint32_t* __restrict__ canon, uint32_t* __restrict__ has_dup)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    uint32_t cls = k;
    unsigned long long key;
    if (canon_key_of(xy[2 * (size_t)k], xy[2 * (size_t)k + 1], key)) {
        const uint32_t mask = (1u << bits) - 1u;
        uint32_t slot = canon_hash(key, bits) & mask;
        while (keys[slot] != key) slot = (slot + 1u) & mask;          // the key was entered by the pass before
        cls = vals[slot];
    }
    canon[k] = cls;
    if (cls != k) atomicOr(has_dup, 1u);
}

__global__ __launch_bounds__(256)
void stage_positions_kernel(const StageViewArgs A) { stage_aux_role(A, blockIdx.x, gridDim.x); }

hipError_t launch_stage_positions(hipStream_t st, const StageViewArgs& A)
{
    if (!A.xy_src || A.n == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_positions_kernel, dim3(stage_aux_blocks(A.n)), dim3(256), 0, st, A);
    if (A.canon_keys)
        hipLaunchKernelGGL(canon_lookup_kernel, dim3((A.n + 255u) / 256u), dim3(256), 0, st, A.xy_dst, A.n, A.canon_keys, A.canon_vals, A.canon_bits,
                           A.canon_dst, A.has_dup);
    return hipGetLastError();
}

hipError_t launch_stage_view(hipStream_t st, const StageViewArgs& A)
{
    hipLaunchKernelGGL(stage_view_kernel, dim3(A.n_tiles + stage_aux_blocks(A.n)), dim3(256), 0, st, A);
    if (A.xy_src && A.canon_keys && A.n)
        hipLaunchKernelGGL(canon_lookup_kernel, dim3((A.n + 255u) / 256u), dim3(256), 0, st, A.xy_dst, A.n, A.canon_keys, A.canon_vals, A.canon_bits,
                           A.canon_dst, A.has_dup);
    return hipGetLastError();
}

// ---- layouts staged on first use, from the fragment-order tiles (which hold the view's f32 values verbatim)
// row-major f32 rows: float4 chunk k4 of row q is tiled float4 ((q >> 5) 2G + k4) 32 + (q & 31)
__global__ __launch_bounds__(256)
void untile_rows_kernel(const float* __restrict__ tiled, uint32_t n, uint32_t dim, uint32_t G, float* __restrict__ rows)
{
    const uint32_t t = blockIdx.x;
    const float* src = tiled + (size_t)t * G * 256u;
    for (uint32_t e = threadIdx.x; e < G * 256u; e += 256u) {
        const uint32_t c = e & 3u, r = (e >> 2) & 31u, h = (e >> 7) & 1u, g = e >> 8;
        const uint32_t row = t * 32u + r, k = 8u * g + 4u * h + c;
        if (row < n && k < dim) rows[(size_t)row * dim + k] = src[e];
    }
}
hipError_t launch_untile_rows(hipStream_t st, const float* tiled, uint32_t n, uint32_t dim, uint32_t G, uint32_t n_tiles, float* rows)
{
    if (n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(untile_rows_kernel, dim3(n_tiles), dim3(256), 0, st, tiled, n, dim, G, rows);
    return hipGetLastError();
}

// bf16 tiles of the integer fast path: the upper 16 bits of the float ARE the value when it is an integer of magnitude <= 256 (8
// significant bits); for any other view these tiles are never read (kernel-side check).  [tile][16-dim block][lane half][32 rows][8]
__global__ __launch_bounds__(256)
void stage_bf16_kernel(const float* __restrict__ tiled, uint32_t G, uint16_t* __restrict__ tiled16)
{
    const uint32_t t = blockIdx.x, GB = (G + 1u) / 2u;
    const float* src = tiled + (size_t)t * G * 256u;
    uint16_t* dst16 = tiled16 + (size_t)t * GB * 512u;
    for (uint32_t e = threadIdx.x; e < GB * 512u; e += 256u) {
        const uint32_t c8 = e & 7u, r = (e >> 3) & 31u, h = (e >> 8) & 1u, kb = e >> 9;
        const uint32_t k = 16u * kb + 8u * h + c8;                   // dimension; in the f32 tiles: g = k / 8, half (k / 4) & 1, lane k & 3
        const uint32_t g = k >> 3;
        const float v = g < G ? src[g * 256u + ((k >> 2) & 1u) * 128u + r * 4u + (k & 3u)] : 0.0f;
        dst16[e] = (uint16_t)(__float_as_uint(v) >> 16);
    }
}
hipError_t launch_stage_bf16(hipStream_t st, const float* tiled, uint32_t G, uint32_t n_tiles, uint16_t* tiled16)
{
    if (n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_bf16_kernel, dim3(n_tiles), dim3(256), 0, st, tiled, G, tiled16);
    return hipGetLastError();
}

// pair-norm tiles of the cascade's filter (l2_knn2_half_kernel): [tile][G / 2 groups][2][32][4] f32 in the fragment order of
// `tiled`, element k of a row = an upper bound of sqrt(x[2k]^2 + x[2k+1]^2).  Dimensions 2k and 2k+1 share a float4 of `tiled`.
// The bound: x^2 and y^2 are exact in double (24-bit significands), their sum s and its root rd carry one rounding each, so
// rd >= (1 - 2^-52) |(x, y)| (2^-50 if the root were off by a few ulps); f = (float)rd rounded to nearest is kept only if
// f >= rd (1 + 2^-40) >= |(x, y)|, else the next float up is taken, which lies above rd by more than that.  So f >= |(x, y)| always
// and f <= (1 + 2^-22) |(x, y)|.  Zero pairs (padding rows and dimensions) stay 0; a NaN element gives NaN, which objects in the test.
// tiledrh (may be null): the same pair norms once more as f16, rounded UP again, for the f16 level of l2_knn2_half_kernel:
// [tile][G / 4 blocks of 16 pair norms][lane half][32 rows][8 f16] -- the fragment order of v_mfma_f32_32x32x16_f16, a quarter of
// `tiled`'s bytes.  h >= f for every element (pairnorm_to_half), so h >= |(x, y)| as well.
__device__ __forceinline__ uint16_t pairnorm_to_half(float f)
{
    // f is a pair norm: +0, positive, +inf or NaN.  Each case keeps h >= f:
    if (f != f) return 0x7E00u;                                      // NaN stays NaN: its keys object
    if (f == 0.0f) return 0u;                                        // zero stays zero (padding rows and dimensions)
    if (f > 65504.0f) return 0x7C00u;                                // beyond the largest f16: +inf, whose keys are -inf or NaN -- both object
    if (f < 6.103515625e-05f) return 0x0400u;                        // below 2^-14: 2^-14, the smallest normal (no subnormal is emitted)
    // a normal f16: drop 13 significand bits, rounding up (the carry may run into the exponent; f <= 65504 keeps it below +inf)
    return (uint16_t)((__float_as_uint(f) - (112u << 23) + 0x1FFFu) >> 13);
}

// tiledp16 (may be null): the first 8 kPrefixGroups = 96 dimensions of every row themselves as f16, for the f16 prefix test of
// l2_knn2_half_kernel: [tile][kPrefixGroups / 2 blocks of 16 dimensions][lane half][32 rows][8 f16], the fragment order of
// v_mfma_f32_32x32x16_f16, 6 KiB per tile.  The rounding (row_to_half; tests/half_prefix_cases.py restates it in numpy bit for bit):
//   a NaN stays a NaN;  |x| < 2^-14 becomes +0 (no subnormal is emitted);  |x| > 32,752 becomes a NaN;  any other value is rounded to the
//   nearest f16, ties to even (32,752 is an f16, so nothing rounds past it): |h - x| <= 2^-11 |x|, or h = 0 and |x| < 2^-14.
// Why the cut is at 32,752 and gives a NaN, where the pair norms go to +inf above 65,504: the kernel scales the query fragment by -2 IN
// f16, which is finite for every stored finite value only up to 32,752 (65,504 / 2); and rows have signs, so an infinite factor gives
// keys of -inf OR +inf (the factors' signs differ) -- and a key of +inf objects to nothing.  A NaN factor makes every key it enters a
// NaN, which objects whatever the signs are.
__device__ __forceinline__ uint16_t row_to_half(float f)
{
    const uint32_t u = __float_as_uint(f), mag = u & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) return 0x7E00u;                           // NaN stays NaN: its keys object
    if (mag > 0x46FFE000u) return 0x7E00u;                           // |x| > 32,752 (+-inf too): NaN as well
    if (mag < 0x38800000u) return 0u;                                // |x| < 2^-14: +0
    const uint32_t v = mag - (112u << 23);                           // a normal f16: drop 13 significand bits, to nearest, ties to even
    return (uint16_t)(((u >> 16) & 0x8000u) | ((v + 0xFFFu + ((v >> 13) & 1u)) >> 13));
}

__global__ __launch_bounds__(256)
void stage_pairnorm_kernel(const float* __restrict__ tiled, uint32_t G, float* __restrict__ tiledr, uint16_t* __restrict__ tiledrh,
                           uint16_t* __restrict__ tiledp16)
{
    const uint32_t t = blockIdx.x, GR = G / 2u;
    const float* src = tiled + (size_t)t * G * 256u;
    float* dst = tiledr + (size_t)t * GR * 256u;
    uint16_t* dsth = tiledrh ? tiledrh + (size_t)t * GR * 256u : nullptr;
    for (uint32_t e = threadIdx.x; e < GR * 256u; e += 256u) {
        const uint32_t c = e & 3u, r = (e >> 2) & 31u, h = (e >> 7) & 1u, g = e >> 8;
        const uint32_t d = 2u * (8u * g + 4u * h + c);               // the pair's first dimension; in the f32 tiles: g = d / 8, half (d / 4) & 1
        const float* p = src + (d >> 3) * 256u + ((d >> 2) & 1u) * 128u + r * 4u + (d & 3u);
        const double x = (double)p[0], y = (double)p[1];
        const double rd = __builtin_sqrt(x * x + y * y);
        float f = (float)rd;
        if ((double)f < rd * (1.0 + 0x1p-40)) f = __uint_as_float(__float_as_uint(f) + 1u);      // (f >= 0 and finite here: the next float up)
        dst[e] = f;
        if (dsth) {
            const uint32_t k = 8u * g + 4u * h + c;                  // the pair; in the f16 tiles: block k / 16, lane half (k / 8) & 1
            dsth[(k >> 4) * 512u + ((k >> 3) & 1u) * 256u + r * 8u + (k & 7u)] = pairnorm_to_half(f);
        }
    }
    if (tiledp16) {
        constexpr uint32_t GB = kPrefixGroups / 2u;                   // blocks of 16 dimensions
        uint16_t* dstp = tiledp16 + (size_t)t * GB * 512u;
        for (uint32_t e = threadIdx.x; e < GB * 512u; e += 256u) {
            const uint32_t k = e & 7u, r = (e >> 3) & 31u, hh = (e >> 8) & 1u, b = e >> 9;
            const uint32_t d = 16u * b + 8u * hh + k;                // the dimension; in the f32 tiles: g = d / 8, half (d / 4) & 1
            dstp[e] = row_to_half(src[(d >> 3) * 256u + ((d >> 2) & 1u) * 128u + r * 4u + (d & 3u)]);
        }
    }
}
hipError_t launch_stage_pairnorm(hipStream_t st, const float* tiled, uint32_t G, uint32_t n_tiles, float* tiledr, uint16_t* tiledrh,
                                 uint16_t* tiledp16)
{
    if (n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_pairnorm_kernel, dim3(n_tiles), dim3(256), 0, st, tiled, G, tiledr, tiledrh, tiledp16);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// fused squared-L2 2-NN: one workgroup = 4 waves; each wave keeps NJ query tiles (32 queries each,
// pre-scaled by -2) in registers as MFMA B fragments and streams every 32-row dataset tile of
// image I as the A fragment, straight from the fragment-ordered HBM/L2 image (1 KiB coalesced
// line per load, rolling PF-deep register window).  D = C + A*B with C initialised to ||a||^2
// gives key = ||a||^2 - 2 a.b per (row, query) in the accumulator; lane (h, c) then owns query
// column c and the 16 rows {e + 8*qd + 4h} of the tile.
//   v_mfma_f32_32x32x2_f32: A lane l = A[i = l&31][k = l>>5], B lane l = B[k = l>>5][j = l&31],
//   D lane l reg r = D[i = (r&3) + 8*(r>>2) + 4*(l>>5)][j = l&31].
// The k axis is permuted identically on both operands (lane half h supplies dims 8g+4h+cc at
// step 4g+cc), which a dot product does not notice.
// ------------------------------------------------------------------------------------------------
// One dataset tile is l2_tile_step (kernels_match_tiles.hpp), shared with l2_knnk_mfma_kernel.
template <int G, int NJ, int PF, int PIPE, int WPS>
__global__ __launch_bounds__(256, WPS)
void l2_knn2_mfma_kernel(const MatchParams P)
{
    static_assert(G % PF == 0, "prefetch window must divide the group count");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t h = lane >> 5, c = lane & 31u;
    // (the query load and the drain below stay written out in every 2-NN nominator: as shared functions they change the kernels'
    //  machine code)
    uint32_t pair, qb;
    if (!workgroup_pair(P, pair, qb)) return;
    const uint2 pr = P.pairs[pair];
    const ImgDev* __restrict__ Ip = P.imgs + pr.x;
    const ImgDev* __restrict__ Jp = P.imgs + pr.y;
    const uint32_t nI = Ip->n, ntI = Ip->n_tiles, ntJ = Jp->n_tiles;
    const uint32_t qt0 = (qb * 4u + wave) * NJ;
    if (qt0 >= ntJ) return;                           // wave-uniform; no barriers in this kernel

    // ---- query fragments (B operand), scaled by -2
    f32x4 bq[NJ][G];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        uint32_t qt = qt0 + nj; if (qt >= ntJ) qt = ntJ - 1;          // clamp: results discarded below
        const gf4p src = (gf4p)Jp->tiled + (size_t)qt * (G * 64) + lane;
#pragma unroll
        for (int g = 0; g < G; ++g) bq[nj][g] = src[g * 64] * -2.0f;
    }

    Top2 st[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) top2_init(st[nj]);

    if (nI >= 2) {
        // ---- dataset stream (A operand): float4 index = (t*G + g)*64 + lane.  abase/nbase are
        // wave-uniform (SGPR) bases; only `lane` / `h` are per-lane.
        const gf4p abase = (gf4p)Ip->tiled;
        const gf4p nbase = (gf4p)Ip->norms;               // tile t, quad qd -> float4 index t*8 + 2*qd + h
        f32x4 abuf[PF];
#pragma unroll
        for (int s = 0; s < PF; ++s) abuf[s] = abase[s * 64 + lane];
        f32x4 nrm[4];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) nrm[qd] = nbase[2 * qd + h];

        if constexpr (PIPE != 0) {
            f32x16 accA[NJ], accB[NJ];
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                for (int r = 0; r < 16; ++r) accB[nj][r] = R3DM_INF;          // "tile -1": keys that never win
            const __amdgpu_buffer_rsrc_t ra = wave_uniform_rsrc(Ip->tiled), rn = wave_uniform_rsrc(Ip->norms);
            const uint32_t voffA = lane * 16u, voffN = h * 16u;
            const uint32_t tileB = (uint32_t)G * 1024u;                // bytes per tile
            const uint32_t hb = 4u * h;
            uint32_t t = 0;
            for (; t + 1 < ntI; t += 2) {
                l2_tile_step<G, NJ, PF, PIPE>(ra, rn, voffA, voffN, t * tileB + PF * 1024u, (t + 1) * 128u, abuf, nrm, bq, accA, accB, st, (t - 1) * 32u + hb);
                l2_tile_step<G, NJ, PF, PIPE>(ra, rn, voffA, voffN, (t + 1) * tileB + PF * 1024u, (t + 2) * 128u, abuf, nrm, bq, accB, accA, st, t * 32u + hb);
            }
            if (t < ntI) {
                l2_tile_step<G, NJ, PF, PIPE>(ra, rn, voffA, voffN, t * tileB + PF * 1024u, (t + 1) * 128u, abuf, nrm, bq, accA, accB, st, (t - 1) * 32u + hb);
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) top2_push(st[nj], accA[nj][r], t * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
            } else {
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) top2_push(st[nj], accB[nj][r], (ntI - 1) * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
            }
        } else {
        for (uint32_t t = 0; t < ntI; ++t) {
            f32x16 acc[NJ];
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nj][r] = nrm[r >> 2][r & 3];
            const gf4p atile = abase + (size_t)(t * G + PF) * 64;    // PF groups ahead (slack-padded)
            const gf4p ntile = nbase + (size_t)(t + 1) * 8;          // next tile's norms (slack-padded)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const f32x4 a = abuf[g % PF];
                abuf[g % PF] = atile[g * 64 + lane];
                if (g == 2) {   // next tile's norms: early, so the wait at the tile boundary finds them landed
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd) nrm[qd] = ntile[2 * qd + h];
                }
#pragma unroll
                for (int cc = 0; cc < 4; ++cc)
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj)
                        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], bq[nj][g][cc], acc[nj], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);        // keep each prefetch in its own step
            }
            const uint32_t rowbase = t * 32u + 4u * h;
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    top2_push(st[nj], acc[nj][r], rowbase + (uint32_t)((r & 3) + 8 * (r >> 2)));
        }
        }   // !PIPE
    }

    l2_finish_queries<NJ>(P, pair, Ip, Jp, st, qt0, h, c, (float)(G * 8), false);
}

// ------------------------------------------------------------------------------------------------
// The same kernel for match mode (r3dm_match_pairs: P.knn_idx == nullptr), stopping tiles early.  Match mode returns, per query, the
// best row if d1 < R d2 and nothing else, so a row matters to a lane half only below R x (its runner-up's distance): with R = 0.36
// about a quarter of a stranger's distance.  A squared distance over the first 8 GP dimensions is a lower bound of the whole one;
// a tile whose every prefix distance lies above every lane's threshold needs no further dimensions (l2_prune_tile_prefix / _finish,
// kernels_match_tiles.hpp; the verdict rule and its proof: l2_finish_queries<PRUNE>, kernels_match_common.hpp).
// Per (lane, query tile), with e0 <= e1 the distances (key + ||q||^2, + slack) of the list's best and runner-up:
//   T   = fl(R e1) if e0 >= fl(R e1) (no match in sight), else max(fl(R e1), e0 / R) -- above e0 / R a pruned row cannot spoil the
//         match either, so the verdict rule does not have to send the query to the exact scan -- rounded up;
//   thr = T - |b_P|^2 + slack, rounded up: a prefix key kp = |a_P|^2 - 2 a_P.b_P above thr means kp + |b_P|^2 - slack > T, and the
//         reference distance of the row is at least that (slack = 0 for pairs with the exactness proof);
//   pl  = the smallest thr a tile was pruned under; pl + |b_P|^2 - slack, rounded down, is below the distance of every pruned row.
// e1 = +inf gives thr = +inf (nothing is above it: the first tile, lists of NaN rows); a lane whose query does not exist (the
// ragged last query tile) never objects.
// ------------------------------------------------------------------------------------------------
template <int G, int GP, int NJ, int PF, int WPS>
__global__ __launch_bounds__(256, WPS)
void l2_knn2_prune_kernel(const MatchParams P)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t h = lane >> 5, c = lane & 31u;
    uint32_t pair, qb;
    if (!workgroup_pair(P, pair, qb)) return;
    const uint2 pr = P.pairs[pair];
    const ImgDev* __restrict__ Ip = P.imgs + pr.x;
    const ImgDev* __restrict__ Jp = P.imgs + pr.y;
    const uint32_t nI = Ip->n, ntI = Ip->n_tiles, nJ = Jp->n, ntJ = Jp->n_tiles;
    const uint32_t qt0 = (qb * 4u + wave) * NJ;
    if (qt0 >= ntJ) return;                           // wave-uniform; no barriers in this kernel

    // ---- query fragments (B operand), scaled by -2: the prefix groups; a tile that goes on reads the others again (soffQ)
    f32x4 bq[NJ][GP];
    uint32_t soffQ[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        uint32_t qt = qt0 + nj; if (qt >= ntJ) qt = ntJ - 1;          // clamp: results discarded below
        soffQ[nj] = qt * (uint32_t)(G * 1024);
        const gf4p src = (gf4p)Jp->tiled + (size_t)qt * (G * 64) + lane;
#pragma unroll
        for (int g = 0; g < GP; ++g) bq[nj][g] = src[g * 64] * -2.0f;
    }
    const __amdgpu_buffer_rsrc_t rqt = wave_uniform_rsrc(Jp->tiled);

    Top2 st[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) top2_init(st[nj]);

    // ---- the lane's share of the threshold: e = key + nbs, thr = T + off (the header comment).  Both come from the query's two norms
    // and are needed only where a list has changed and once at the end: they are read again there (the index passes through an
    // empty asm so that the loads stay where they are needed) instead of living in registers the tile loop has no room for.
    const bool exact_pair = l2_pair_is_exact(Ip, Jp, (float)(G * 8), false);
    const float R = P.ratio_R, invR = 1.0f / P.ratio_R;
    const __amdgpu_buffer_rsrc_t rq = wave_uniform_rsrc(Jp->norms);
    const float maxnormI = __uint_as_float(Ip->max_norm_bits);
    auto lane_terms = [&](int nj, float& nbs, float& off) __attribute__((always_inline)) -> bool {
        uint32_t q = (qt0 + (uint32_t)nj) * 32u + c;
        asm volatile("" : "+v"(q));
        const bool dead = !(q < nJ);                    // (covers a query tile beyond the last one too: its rows lie beyond nJ)
        const uint32_t qo = dead ? 0u : q * 4u;
        const float nb = __uint_as_float((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rq, (int)qo, 0, 0));
        const float nbp = __uint_as_float((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rq, (int)qo, (int)(prefix_norm_offset(ntJ) * 4u), 0));
        const float slk = exact_pair ? 0.0f : (P.err_scale + kPruneKeySlack) * (maxnormI + nb);
        nbs = nb + slk;
        off = slk - nbp;
        return dead;
    };
    float thr[NJ], pl[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) { thr[nj] = R3DM_INF; pl[nj] = R3DM_INF; }      // (nothing is above +inf: tile 0 is never pruned)
    uint32_t n_tested = 0, n_pruned = 0;              // wave-uniform
    bool pruned_under_thr = false;                    // ... as is this: a tile was pruned since thr was last refreshed (pl does not hold it yet)

    if (nI >= 2) {
        // ---- dataset stream (A operand): float4 index = (t*G + g)*64 + lane
        const gf4p abase = (gf4p)Ip->tiled;
        const gf4p pbase = (gf4p)(Ip->norms + prefix_norm_offset(ntI));      // tile t, quad qd -> float4 index t*8 + 2*qd + h
        f32x4 abuf[PF];
#pragma unroll
        for (int s = 0; s < PF; ++s) abuf[s] = abase[s * 64 + lane];
        f32x4 pnrm[4];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) pnrm[qd] = pbase[2 * qd + h];

        f32x16 accA[NJ], accB[NJ];
        const __amdgpu_buffer_rsrc_t ra = wave_uniform_rsrc(Ip->tiled), rn = wave_uniform_rsrc(Ip->norms);
        const uint32_t voffA = lane * 16u, voffN = h * 16u;
        const uint32_t tileB = (uint32_t)G * 1024u;                // bytes per tile
        const uint32_t poff = prefix_norm_offset(ntI) * 4u;        // bytes from the norms to the prefix norms
        const uint32_t hb = 4u * h;
        // the thresholds follow the lists: refreshed behind every epilogue (the only place a list changes)
        auto refresh = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) {
                if (pruned_under_thr) pl[nj] = __builtin_fminf(pl[nj], thr[nj]);
                float nbs, off;
                const bool dead = lane_terms(nj, nbs, off);
                const float e0 = st[nj].d0 + nbs, e1 = st[nj].d1 + nbs;
                const float re1 = R * e1;
                float T = e0 < re1 ? __builtin_fmaxf(re1, e0 * invR) : re1;
                T += __builtin_fabsf(T) * 4.76837158203125e-07f;        // 2^-21: the roundings of e1, R e1, 1 / R and e0 / R
                const float x = T + off;
                thr[nj] = dead ? -R3DM_INF : x + __builtin_fabsf(x) * 2.384185791015625e-07f;      // 2^-22: the rounding of x
            }
        };
        // one tile: `live` says whether `prev` holds keys to fold, and afterwards whether `cur` does
        auto tile = [&](uint32_t t, f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ], bool live) __attribute__((always_inline)) -> bool {
            l2_prune_tile_prefix<G, GP, NJ, PF>(ra, rn, voffA, voffN, t * tileB, poff + t * 128u, abuf, pnrm, bq, cur, prev, st,
                                                (t - 1) * 32u + hb, live);
            if (live) { refresh(); pruned_under_thr = false; }
            n_tested += 1u;
            const bool on = l2_prune_tile_finish<G, GP, NJ, PF>(ra, rn, voffA, voffN, t * tileB, t * 128u, poff + t * 128u, abuf, rqt, soffQ, cur, thr);
            if (!on) { n_pruned += 1u; pruned_under_thr = true; }
            return on;
        };
        bool live = false;
        uint32_t t = 0;
        for (; t + 1 < ntI; t += 2) {
            live = tile(t, accA, accB, live);
            live = tile(t + 1, accB, accA, live);
        }
        if (t < ntI) {
            if (tile(t, accA, accB, live)) {
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) top2_push(st[nj], accA[nj][r], t * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
            }
        } else if (live) {
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                for (int r = 0; r < 16; ++r) top2_push(st[nj], accB[nj][r], (ntI - 1) * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
        }
    }

#pragma unroll
    for (int nj = 0; nj < NJ; ++nj)
        if (pruned_under_thr) pl[nj] = __builtin_fminf(pl[nj], thr[nj]);
    // pl -> a lower bound of the pruned rows' distances: pl + |b_P|^2 - slack, rounded down
    float pruned_lb[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        float nbs, off;
        const bool dead = lane_terms(nj, nbs, off);
        const float x = pl[nj] - off;
        pruned_lb[nj] = dead ? -R3DM_INF : x - __builtin_fabsf(x) * 2.384185791015625e-07f;
    }
    if (lane == 0 && n_tested) {
        atomicAdd(&P.prune_cnt->n_tested, (unsigned long long)n_tested);
        if (n_pruned) atomicAdd(&P.prune_cnt->n_pruned, (unsigned long long)n_pruned);
    }
    l2_finish_queries<NJ, false, false, true>(P, pair, Ip, Jp, st, qt0, h, c, (float)(G * 8), false, 1.0f, 0.0f, nullptr, pruned_lb);
}

// ------------------------------------------------------------------------------------------------
// The cascade: a cheaper proof in front of the prefix test.  The prefix test above runs GP = 12 of a tile's 16 groups before it may
// stop it; most tiles it stops hold strangers only, and for those HALF the contraction proves as much.  Split the 128 dimensions
// into 64 pairs; with sa_k >= |(a_2k, a_2k+1)| and sb_k likewise (the pair-norm tiles, stage_pairnorm_kernel), Cauchy-Schwarz per pair gives
// a.b <= sum_k sa_k sb_k, hence
//     kf + |b|^2 <= |a - b|^2,   kf = |a|^2 - 2 sum_k sa_k sb_k,
// for any signs and any data: the same MFMA contraction over reduced rows of 64 floats (8 groups), started from the FULL norms.
// Per tile (T, thr as above; thrF = T - |b|^2 + slackF, rounded up):
//   1. l2_pairnorm_tile_filter: 8 groups on the pair-norm tiles.  No lane has a kf that is not above its thrF -> the tile is done.
//   2. else l2_prune_tile_restart: the tile runs the step above from its group 0 -- prefix norms, 12 groups, the prefix test against
//      thr, suffix, epilogue -- with all its fragments read again (the wave keeps only the reduced query fragments in registers).
// A tile is pruned if EITHER bound rules it out, and the keys of every tile that finishes are the floats of the kernel above.
// slackF (carried by EVERY pair: products of roots are no integers, the exactness proof does not reach kf), in units of
// u (max|a|^2 + |q|^2), u = 2^-24, against the reference distance d_ref:
//     128   the stored |a|^2 (the accumulators' start) and the stored |q|^2 (in thrF): fma chains of 128 non-negative terms, each
//           off by at most 128 u of its own norm
//      65   the 64 products sa_k sb_k and their sum (non-negative terms: the error is relative to the sum), the nudges of both
//           factors included: 2 sum_k sa_k sb_k <= (1 + 2^-21) 2 |a| |b| <= (1 + 2^-21) (|a|^2 + |q|^2)
//      64   64 roundings of accumulators whose values stay within [-|q|^2, |a|^2 + |q|^2] (two products per MFMA, 32 MFMAs)
//     256   d_ref itself: the reference's sum of 128 non-negative terms is at least (1 - 128 u) |a - b|^2 <= 2 (|a|^2 + |q|^2)
//   = 513 <= 4.25 x 128 = 544 u = err_scale, the certificate's own factor; kPruneKeySlack (8 u) on top pays the roundings of slackF,
//     of slackF - |q|^2 and of T.  So slackF = (err_scale + kPruneKeySlack) (max|a|^2 + |q|^2): the certificate's form, for EVERY pair.
//   The nudge itself costs no slack: it only raises sa, sb, which lowers kf -- the bound gets looser, never wrong.
// Rows pruned by either test lie strictly above the lane half's T of that moment in reference distance (the filter: kf > thrF >=
// T - |b|^2 + slackF, and d_ref >= kf + |b|^2 - slackF; the prefix test: kernel above), so plT, the smallest T a lane half pruned
// under, is the lower bound l2_finish_queries<PRUNE> asks for, whichever test pruned.
// MODE (developer ablations): 0 the cascade | 1 filter only (step 2 never stops a tile).
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// The f16 level: a cheaper filter in front of the filter (r3dm_set_half_filter, default on).  The pair-norm filter is the one
// contraction of the cascade whose result reaches no caller -- a lower bound, compared against a threshold -- and it stays a lower
// bound when the pair norms are rounded UP to f16: with ha_k >= sa_k, hb_k >= sb_k (stage_pairnorm_kernel's second table)
//     kh = |a|^2 - 2 sum_k ha_k hb_k  <=  kf            in exact arithmetic,
// and v_mfma_f32_32x32x16_f16 contracts 16 pair norms in 32 cycles where v_mfma_f32_32x32x2_f32 takes 64 for two.  Per tile:
//   1. l2_halfnorm_tile_filter: 4 blocks on the f16 tiles.  No lane has a kh that is not above its thrH -> the tile is done.
//   2. else l2_pairnorm_tile_stream: the cascade's filter, its 8 groups read again (the wave keeps only the f16 query fragments in
//      registers); no lane has a kf that is not above its thrF -> the tile is done.
//   3. else l2_prune_tile_restart, as in the cascade.
// THE INVARIANT: level 1 prunes a tile only if level 2 would.  Then the pruned tiles, hence the lists, T, plT, the counters of the
// cascade and every result are the cascade's on any data, and only the work differs.  It holds when thrH >= thrF + margin and the
// margin covers the evaluation errors of both COMPUTED keys against their exact values on the STORED operands (the stored norm N,
// the stored f32 pair norms s, the stored f16 pair norms h; h >= s holds exactly, whatever the rows):
//     kf_c >= kf - eF,  kh_c <= kh + eH,  kh <= kf   =>   kh_c > thrF + eF + eH  implies  kf_c > thrF.
// In units of u M, u = 2^-24, M = max|a|^2 + |q|^2 (the stored norms, as in slackF), assuming the matrix unit may TRUNCATE: one ulp,
// 2 u of the value, per product rounding and per addition (the form of the split planes' bound, kernels_match_16bit.hip):
//   eF   2   the 64 products -2 sa_k sb_k of the f32 MFMAs, one ulp each: 2 u x 2 sum sa_k sb_k <= 2 u (1 + 2^-20) M
//      128   64 additions into accumulators that stay within [-(1 + 2^-20) M, M]
//   eH     0 the products -2 ha_k hb_k: 11-bit x 11-bit significands, exact in f32 (h <= 65504 and h = 0 or h >= 2^-14: no overflow,
//            no underflow); -2 hb is exact in f16 or overflows to -inf, which objects
//      257   64 additions (16 per MFMA, in any order) of partial sums and accumulators whose magnitude stays below
//            sum_k (ha_k^2 + hb_k^2) + M <= 2 (1 + 2^-10)^2 (1 + 2^-21) M + 2^-20 <= 2.005 M + 2^-20:  h <= (1 + 2^-10) s + 2^-14
//            (the round-up and the floor at 2^-14), so h^2 <= 2 (1 + 2^-10)^2 s^2 + 2^-27 over 128 pair norms
//   = 387 u M + 128 u 2^-19; the kernel takes margin = 400 u M + 2^-35 (kHalfMarginFactor, kHalfMarginAbs: the roundings of the
//   margin itself included) and thrH = (thrF + margin) rounded up by 2^-22 of it, which pays that sum's rounding.  That is
//   0.72 of one more slackF (552 u M): tools/prefix_prune_model.py --filter half shows what it costs (0.15 % of c2's tiles).
// Values outside f16's range cost level 1's work and nothing else: a pair norm above 65,504 is +inf, its keys -inf or NaN, both
// object and the tile goes to level 2; non-zero values below 2^-14 are held at 2^-14 (the bound gets looser, never wrong).
// THE SKIP OF LEVEL 2.  Level 2 leaves a tile alone as soon as ONE lane holds one key kf_c <= thrF, and most tiles that object at
// level 1 hold an f16 key far below the threshold: the f32 pair norms cannot lift it above.  With a bound L on what they can lift,
//     kf_c <= kh_c + L   (same row, same query),   so   kh_c <= thrF - L  =>  kf_c <= thrF  =>  level 2 would not prune,
// and the tile goes from level 1 straight to the restart: the decision is the one level 2 would have taken, its 64 f32 MFMAs and 24 KiB
// are saved.  L on the STORED operands, M = max|a|^2 + |q|^2 as above, eps = 2^-10, dlt = 2^-14:
//   the rounding loss   kf - kh = 2 sum_k (ha_k hb_k - sa_k sb_k).  pairnorm_to_half gives h = 0 iff s = 0 and, for every finite h,
//           h <= (1 + eps) s + dlt (the round-up of a normal; the floor at 2^-14).  A pair with sa_k sb_k = 0 has ha_k hb_k = 0; else
//           ha hb - sa sb <= ((1 + eps)^2 - 1) sa sb + dlt (1 + eps) (sa + sb) + dlt^2.  Over the 64 pairs, twice:
//             ((1 + eps)^2 - 1) 2 sum sa sb  <=  (2^-9 + 2^-20) (1 + 2^-16) M:   2 sum sa sb <= sum sa^2 + sum sb^2, s <= (1 + 2^-22) |(x, y)|
//                 (stage_pairnorm_kernel) and a stored norm is at least (1 - 128 u) of its row's, so sum sa^2 + sum sb^2 <= (1 + 2^-16) M
//             2 dlt (1 + eps) sum (sa + sb)  <=  2^-13 (1 + 2^-16) M + 2^-8 (1 + eps)^2:   2 d x <= e x^2 + d^2 / e for each of the 128
//                 values x, with e = 2^-13, d = dlt (1 + eps): 128 d^2 / e = 2^-8 (1 + eps)^2
//             128 dlt^2 = 2^-21
//   the evaluation errors, in the direction opposite to the margin's: kf_c <= kf + eF, kh_c >= kh - eH, the same counts:
//           130 + 257 = 387 u M + 128 u 2^-19
//   = (2^-9 + 2^-13 + 2^-20 + 2^-24 + 387 u) M + 2^-8 + 2^-16.  The kernel takes L = (2^-9 + 2^-13 + 2^-15) M + 2^-8 + 2^-15
//   (kSkipLossFactor, kSkipLossAbs): 2^-15 = 512 u leaves 100 u M for the three roundings of L itself, and thrS = thrF - L rounded DOWN by
//   2^-22 of it, which pays that difference's rounding.  The form is lane-constant, refreshed beside thrH; tools/prefix_prune_model.py
//   --filter half compares it with the key-dependent form from 2 sum ha hb = N - kh (profiles/level2_skip_model_c2.txt).
// A key that is -inf or NaN comes from an f16 pair norm of +inf (or a NaN), whose loss no L bounds: only a key above -inf counts (a NaN
// fails both compares).  thrS is -inf for a dead lane and while thrF = +inf; a NaN thrS (M = +inf) skips nothing.  A tile may still run
// level 2 when it need not; the skip never fires where level 2 would prune.
// MODE: 0 the three levels, level 2 skipped where it cannot prune | 3 the same with the tile tests in their min form (below);
// developer ablations: 1 level 1, then straight to the restart (timing only: other tiles are pruned) | 2 the three levels without the
// skip | 4 level 1 alone: no tile behind tile 0 goes on | 5 level 1 alone without its decision (4 and 5: timing only) | 8, 9: 4 and 5 in
// the min form | 6, 7: MODE 0 and 3 with the f16 prefix test in front of the restart (below).
// THE MIN FORM OF THE TILE TESTS (MODE 3; r3dm_set_min_tile_test, default on).  The tests above ask of a lane's 16 keys of a query tile
// "is ONE key not above thr?" (the objections of level 1, of level 2, of the restart's prefix test) and "is ONE key above -inf at or below
// thrS?" (the skip): 16 v_cmp that alternate with 16 s_or on every tile, twice on a tile that objects.  Both are questions about the
// MINIMUM of the keys -- unless a key is a NaN (the general form lets it object; v_min3_f32 returns the operand that is no NaN and
// loses it) or -inf (the general form keeps it from the skip; a minimum cannot tell it from a finite key beside it).  Where no key is
// either, with m = min k (tile_key_min: 8 v_min3_f32 / v_min_f32 per query tile, no scalar unit),
//     any(!(k > thr))  ==  !(m > thr)          any(k <= thrS and k > -inf)  ==  m <= thrS       for ANY thr, thrS (NaN, +-inf included),
// so every tile is decided as in MODE 0 -- the same tiles pruned, the same skips, lists, T, plT and counters -- and the skip reads
// the minimum the objection made.  A dead lane (thrH = thrS = -inf) neither objects nor skips, the first tile (thrH = +inf) objects.
// THE RULE: both views of every pair of the batch have ImgDev::max_norm_bits < the bits of 2^28, as unsigned integers (run_match_batch
// decides per batch from the host's copy, kMinTileTestNormBits; any other batch runs MODE 0).  A NaN or +inf norm has larger bits
// than every finite one, so the data is finite, and every STORED norm N (the fma chain of staging, >= (1 - 128 u) |row|^2, u = 2^-24)
// is below 2^28: |row|^2 < 2^28 (1 + 2^-16), every member and every pair |(x, y)| <= |row| < 2^14 (1 + 2^-17).  Then
//   the f32 pair norms   s <= (1 + 2^-22) |(x, y)| < 16,384.2 (stage_pairnorm_kernel's root and nudge)
//   the f16 pair norms   h <= (1 + 2^-10) s + 2^-14 < 16,401 (pairnorm_to_half: the round-up, the floor), far below 32,752, so the
//                        query fragment -2 h is a finite f16 (exact: a power of two) and no h is +inf
//   level 1   a product ha (-2 hb) is below 5.4e8 in magnitude and exact in f32; 64 of them, in any order and with any roundings,
//             stay below 3.5e10 beside an accumulator that starts at N < 2^28, or at +inf on a padding row -- whose pair norms are 0,
//             times finite factors: no 0 x inf.  Every key kh_c is finite, or +inf on a padding row: never a NaN, never -inf
//   level 2   the same with s for h: products sa (-2 sb) below 5.4e8, each rounded once, 64 of them: kf_c finite or +inf
//   the restart's prefix test   starts at the prefix norm (at most N, or +inf on a padding row, whose members are 0) and adds 96
//             products a_i (-2 b_i) below 5.4e8 each: finite or +inf.
// c2's rows have |row|^2 = 2^18.  tests/test_min_tile_test_rule.py has the worst cases in numpy (all of a row in one pair at 2^28 - 16).
// WHAT ELSE MODE 3 DOES: the first MFMA of a tile takes the norm registers as its C operand for BOTH query tiles (l2_halfnorm_tile_filter
// <CSTART>: one 16-register tuple the four norm loads fill; MODE 0 copies it for the second query tile, 8 v_mov_b64).  Per tile the
// decision is 17 VALU + 2 v_cmp + 1 s_or (MODE 0: 32 v_cmp + 32 s_or), the skip test 2 v_cmp + 1 s_or (64 v_cmp + 32 s_and + 32 s_or).
// THE F16 PREFIX TEST (MODE 6 | 7 = MODE 0 | 3 with it; r3dm_set_half_prefix, default on).  A tile that gets to the restart first runs
// the restart's prefix test -- 48 v_mfma_f32_32x32x2_f32 per query tile, 36 KiB -- and three times in four that test prunes it: once
// more a threshold test whose result reaches no caller.  In front of it: the same test on the rows ROUNDED to f16 (stage_pairnorm_kernel's
// third table, row_to_half), 6 v_mfma_f32_32x32x16_f16 per query tile and 18 KiB (l2_prefix16_tile_stream), from the same stored prefix
// norm nP.  No lane has a key kq_c that is not above its thrQ -> the tile is pruned (n_prefix16, part of n_pruned); else the restart as
// ever, its own prefix test included.  THE INVARIANT: this test prunes a tile only if the restart's prefix test would; then the pruned
// tiles, the lists, T, plT, the five older counters and every result are those of MODE 0 | 3 on any data.  It holds when
//     thrQ >= thr + D + eP + eQ:    kp_c >= kp - eP,  kq_c <= kq + eQ,  kq <= kp + D   =>   kq_c > thrQ  implies  kp_c > thr,
// kp = nP - 2 sum_i a_i q_i the restart's prefix key and kq = nP - 2 sum_i A_i Q_i this test's, both exact on the STORED operands (the f32
// rows a, q of the tiles; A, Q their f16 values), i over the 96 prefix dimensions.  S = |a_P|^2 + |q_P|^2 <= (1 + 2^-16) M, M = max|a|^2 +
// |q|^2 on the stored norms as above (a stored norm is at least (1 - 128 u) of its row's), eps = 2^-11, dlt = 2^-14, all operands finite:
//   D, the operand rounding, D = 2 sum_i |a_i q_i - A_i Q_i|.  row_to_half gives |A - a| <= eps |a| for a value it keeps and A = 0 for
//           |a| < dlt.  Per dimension: both kept: |a q - A Q| <= ((1 + eps)^2 - 1) |a| |q|;  a flushed: A Q = 0 and |a q| <= dlt |q|;  q
//           flushed: <= dlt |a| -- ONE term dlt x per dimension, x a member of a or q.  Over the 96 dimensions, twice:
//             (2 eps + eps^2) 2 sum |a_i| |q_i|  <=  (2^-10 + 2^-22) S
//             2 dlt sum x  <=  2^-15 S + 96 x 2^-13:   2 d x <= e x^2 + d^2 / e per value (the step of kSkipLoss) with d = dlt, e = 2^-15
//   eP, the f32 prefix key's evaluation, the matrix unit assumed to TRUNCATE (2 u of the value per product rounding and per addition):
//             2   the 96 products -2 a_i q_i (-2 q is exact): 2 u x 2 sum |a_i| |q_i| <= 2 u S
//           384   96 additions into accumulators within nP + 2 sum |a_i| |q_i| <= 2 (1 + 2^-16) M
//   eQ, the f16 contraction's: the products A (-2 Q) are exact in f32 (11-bit x 11-bit significands; |A|, |Q| <= 32,752 and 0 or >= 2^-14:
//           -2 Q is a finite f16, no product overflows or underflows);
//           385   96 additions (16 per MFMA, six MFMAs, in any order) of partial sums and accumulators within nP + (1 + eps)^2 S <= 2.002 M
//   = (2^-10 + 2^-15 + 2^-22 + 771 u) (1 + 2^-16) M + 3 x 2^-8  <  (2^-10 + 1,288 u) M + 2^-6.4.
// The kernel takes marginQ = (2^-10 + 2^-14 + 2^-15) M + 2^-6 (kPrefixMarginFactor = 2^-10 + 1,536 u, kPrefixMarginAbs): 248 u M and
// 0.0039 pay the two roundings of marginQ itself (2 u of it), and thrQ = (thr + marginQ) rounded up by 2^-22 of it, which pays that
// sum's rounding.  thrQ is lane-constant between two refreshes; the kernel makes it where the test runs, from lane_terms -- on 4 % of
// the tiles -- because one more register per query tile through the tile loop does not fit (256 VGPRs with it, and a spill).
// Operands that are not finite, or beyond f16: row_to_half turns a NaN, +-inf and every |x| > 32,752 into a NaN, and a NaN factor makes
// every key it enters a NaN, which objects (the general form's compare; the min form never sees one, below): such a tile only ever
// goes on to the restart.  (+-inf would not do: rows have signs, so A (-2 Q) with one infinite factor is -inf OR +inf, and a key of
// +inf objects to nothing.  The cut is 32,752 = 65,504 / 2 because the kernel scales Q by -2 in f16.)  thr = +inf gives thrQ = +inf, a
// NaN thr or M = +inf gives a NaN or +inf thrQ: the test objects; a dead lane has thr = -inf and, M finite, thrQ = -inf -- or a NaN,
// which only objects.  A padding row has nP = +inf and members 0: its key is +inf (or a NaN beside a NaN factor), as the restart's.
// THE MIN FORM'S RULE reaches the new keys: max |row|^2 < 2^28 (1 + 2^-16) gives |x| < 2^14 (1 + 2^-17), so |A| <= 2^14 (1 + 2^-10)
// < 32,752: no NaN, -2 Q finite; a product is below 5.4e8 and exact, 96 of them stay below 5.2e10 beside nP < 2^28, or +inf on a
// padding row, whose members are 0 times finite factors.  Every key kq_c is finite, or +inf on a padding row: never a NaN, never -inf.
// tools/prefix_prune_model.py --filter half --skip lane --prefix16 restates the test in numpy (profiles/half_prefix_model_c2.txt);
// tests/test_half_prefix_rule.py has the bound's worst cases.
// ------------------------------------------------------------------------------------------------
constexpr float kHalfMarginFactor = 400.0f * 5.9604644775390625e-08f;       // 400 x 2^-24
constexpr float kHalfMarginAbs = 2.9103830456733704e-11f;                   // 2^-35
constexpr float kSkipLossFactor = 0.001953125f + 0.0001220703125f + 3.0517578125e-05f;      // 2^-9 + 2^-13 + 2^-15
constexpr float kSkipLossAbs = 0.00390625f + 3.0517578125e-05f;                               // 2^-8 + 2^-15
constexpr float kPrefixMarginFactor = 0.0009765625f + 6.103515625e-05f + 3.0517578125e-05f;  // 2^-10 + 2^-14 + 2^-15
constexpr float kPrefixMarginAbs = 0.015625f;                                                 // 2^-6

// ------------------------------------------------------------------------------------------------
// Both forms are ONE kernel, and the template argument MODE also says how many levels run: MODE = 0 .. 9 are the three levels with
// the f16 level's MODE above, MODE = 20 | 21 the two levels (the cascade: pair-norm filter, then the restart) with the cascade's
// MODE 0 | 1 above.  (The name and the argument list are the three-level kernel's, so that its symbol -- which
// profiles/pmc_traffic.json and the tracked profiles name -- stays.)
// They share the frame -- the workgroup's pair, lane_terms, the refresh with the T formula every proof above leans on, the tile
// alternation, the drain of the last tile, pruned_lb, the counters, l2_finish_queries -- and differ in the table level 1 contracts,
// in thrH / thrS, the skip and level 2, and in two counters; what only one form uses is declared in both and dies unused in the
// other.  Each instantiation is, instruction for instruction, the kernel it was when the two were written out
// (profiles/levels_frame_isa.txt).
// ------------------------------------------------------------------------------------------------
// a table's address out of the header, loaded as the 64-bit word it was before the header had a type: read through the pointer-typed
// field, the load sits two instructions earlier in the two-level kernel
template <class T>
__device__ __forceinline__ const T* const* prune_table(const PruneHeader* hdr, size_t offset)
{
    return reinterpret_cast<const T* const*>(reinterpret_cast<const unsigned long long*>(hdr)[offset / 8]);
}

template <int G, int GP, int NJ, int PF, int WPS, int MODE>
__global__ __launch_bounds__(256, WPS)
void l2_knn2_half_kernel(const MatchParams P)
{
    static_assert((MODE >= 0 && MODE <= 9) || MODE == 20 || MODE == 21, "three levels: 0 .. 9; two levels: 20 | 21");
    constexpr bool H = MODE < 20;                     // the f16 level in front
    constexpr bool MIN = MODE == 3 || (MODE >= 7 && MODE <= 9);   // the min form of the three levels' tile tests
    constexpr bool Q16 = MODE == 6 || MODE == 7;      // the f16 prefix test in front of the restart
    constexpr bool L1_ALONE = MODE == 4 || MODE == 8, L1_UNDECIDED = MODE == 5 || MODE == 9;      // (timing only)
    constexpr int ABL = (MIN || Q16) ? 0 : MODE % 20; // the form's own MODE (the header comments)
    constexpr int GR = G / 2, GH = G / 4, G1 = H ? GH : GR;      // groups of a reduced tile, blocks of an f16 tile, what level 1 contracts
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t h = lane >> 5, c = lane & 31u;
    uint32_t pair, qb;
    if (!workgroup_pair(P, pair, qb)) return;
    const uint2 pr = P.pairs[pair];
    const ImgDev* __restrict__ Ip = P.imgs + pr.x;
    const ImgDev* __restrict__ Jp = P.imgs + pr.y;
    const float* const* pairnorm = prune_table<float>(P.prune_cnt, offsetof(PruneHeader, pairnorm));
    const uint16_t* const* halfnorm = H ? prune_table<uint16_t>(P.prune_cnt, offsetof(PruneHeader, halfnorm)) : nullptr;
    const float* __restrict__ redI = pairnorm[pr.x];
    const float* __restrict__ redJ = pairnorm[pr.y];
    const uint16_t* __restrict__ hlfI = H ? halfnorm[pr.x] : nullptr;
    const uint16_t* __restrict__ hlfJ = H ? halfnorm[pr.y] : nullptr;
    const uint16_t* const* prefix16 = Q16 ? prune_table<uint16_t>(P.prune_cnt, offsetof(PruneHeader, prefix16)) : nullptr;
    const uint16_t* __restrict__ p16I = Q16 ? prefix16[pr.x] : nullptr;
    const uint16_t* __restrict__ p16J = Q16 ? prefix16[pr.y] : nullptr;
    const uint32_t nI = Ip->n, ntI = Ip->n_tiles, nJ = Jp->n, ntJ = Jp->n_tiles;
    const uint32_t qt0 = (qb * 4u + wave) * NJ;
    if (qt0 >= ntJ) return;                           // wave-uniform; no barriers in this kernel

    // ---- query fragments of level 1 (B operand), scaled by -2: the reduced ones, or the f16 ones (exact, or -inf); a tile that goes
    // on reads the f32 ones again (soffQR: the reduced groups, soffQ: the full ones)
    f32x4 bq1[NJ][G1];
    uint32_t soffQ[NJ], soffQR[NJ], soffQB[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        uint32_t qt = qt0 + nj; if (qt >= ntJ) qt = ntJ - 1;          // clamp: results discarded below
        soffQ[nj] = qt * (uint32_t)(G * 1024);
        soffQR[nj] = qt * (uint32_t)(GR * 1024);
        soffQB[nj] = qt * (uint32_t)(GP / 2 * 1024);
        const gf4p src = (H ? (gf4p)hlfJ : (gf4p)redJ) + (size_t)qt * (G1 * 64) + lane;
#pragma unroll
        for (int g = 0; g < G1; ++g) {
            if constexpr (H) bq1[nj][g] = __builtin_bit_cast(f32x4, __builtin_bit_cast(f16x8, src[g * 64]) * (_Float16)-2.0f);
            else bq1[nj][g] = src[g * 64] * -2.0f;
        }
    }
    const __amdgpu_buffer_rsrc_t rqt = wave_uniform_rsrc(Jp->tiled), rqr = wave_uniform_rsrc(redJ), rqp = wave_uniform_rsrc(p16J);

    Top2 st[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) top2_init(st[nj]);

    // ---- the lane's share of the thresholds (read again where a list has changed, as in the kernel above; mgn and loss: thrH, thrS)
    const bool exact_pair = l2_pair_is_exact(Ip, Jp, (float)(G * 8), false);
    const float R = P.ratio_R, invR = 1.0f / P.ratio_R;
    const __amdgpu_buffer_rsrc_t rq = wave_uniform_rsrc(Jp->norms);
    const float maxnormI = __uint_as_float(Ip->max_norm_bits);
    auto lane_terms = [&](int nj, float& nbs, float& off, float& offF, float& mgn, float& loss, float& mgnQ) __attribute__((always_inline)) -> bool {
        uint32_t q = (qt0 + (uint32_t)nj) * 32u + c;
        asm volatile("" : "+v"(q));
        const bool dead = !(q < nJ);                    // (covers a query tile beyond the last one too: its rows lie beyond nJ)
        const uint32_t qo = dead ? 0u : q * 4u;
        const float nb = __uint_as_float((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rq, (int)qo, 0, 0));
        const float nbp = __uint_as_float((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rq, (int)qo, (int)(prefix_norm_offset(ntJ) * 4u), 0));
        const float slkF = (P.err_scale + kPruneKeySlack) * (maxnormI + nb);
        const float slk = exact_pair ? 0.0f : slkF;
        nbs = nb + slk;
        off = slk - nbp;
        offF = slkF - nb;
        mgn = kHalfMarginFactor * (maxnormI + nb) + kHalfMarginAbs;
        loss = kSkipLossFactor * (maxnormI + nb) + kSkipLossAbs;
        mgnQ = kPrefixMarginFactor * (maxnormI + nb) + kPrefixMarginAbs;
        return dead;
    };
    float thr[NJ], thrF[NJ], thrH[NJ], thrS[NJ], Tl[NJ], plT[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) { thr[nj] = R3DM_INF; thrF[nj] = R3DM_INF; thrH[nj] = R3DM_INF; thrS[nj] = -R3DM_INF; Tl[nj] = R3DM_INF; plT[nj] = R3DM_INF; }      // (nothing is above +inf: tile 0 is never pruned, and never skips level 2)
    uint32_t n_tested = 0, n_pruned = 0, n_filtered = 0, n_half = 0, n_skip = 0, n_prefix16 = 0;      // wave-uniform
    float sink = 0.0f;                                // (MODE 5: what consumes the keys)
    bool pruned_under_thr = false;                    // ... as is this: a tile was pruned since the thresholds were last refreshed (plT does not hold it yet)

    if (nI >= 2) {
        // ---- dataset stream of level 1 (A operand): the pair-norm tiles or the f16 tiles, float4 index = (t*G1 + g)*64 + lane, and
        // the full norms
        const gf4p abase = H ? (gf4p)hlfI : (gf4p)redI;
        const gf4p nbase = (gf4p)Ip->norms;               // tile t, quad qd -> float4 index t*8 + 2*qd + h
        f32x4 abuf[PF];
#pragma unroll
        for (int s = 0; s < PF; ++s) abuf[s] = abase[s * 64 + lane];
        f32x4 nrm[4];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) nrm[qd] = nbase[2 * qd + h];

        f32x16 accA[NJ], accB[NJ];
        const __amdgpu_buffer_rsrc_t ra = wave_uniform_rsrc(Ip->tiled), rn = wave_uniform_rsrc(Ip->norms), rr = wave_uniform_rsrc(redI),
                                     rh = wave_uniform_rsrc(hlfI), rp = wave_uniform_rsrc(p16I);
        const uint32_t voffA = lane * 16u, voffN = h * 16u;
        const uint32_t tileB = (uint32_t)G * 1024u, tileRB = (uint32_t)GR * 1024u, tileHB = (uint32_t)GH * 1024u;      // bytes per tile, reduced tile, f16 tile
        const uint32_t tileQB = (uint32_t)(GP / 2) * 1024u;           // ... and per tile of the f16 prefix rows
        const uint32_t poff = prefix_norm_offset(ntI) * 4u;        // bytes from the norms to the prefix norms
        uint32_t hb = 4u * h;
        // the thresholds follow the lists: refreshed behind every epilogue (the only place a list changes).  T, thr and thrF are the
        // same floats with two levels and with three; thrH >= thrF + margin (the header comment)
        auto refresh = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) {
                if (pruned_under_thr) plT[nj] = __builtin_fminf(plT[nj], Tl[nj]);
                float nbs, off, offF, mgn, loss, mgnQ;
                const bool dead = lane_terms(nj, nbs, off, offF, mgn, loss, mgnQ);
                const float e0 = st[nj].d0 + nbs, e1 = st[nj].d1 + nbs;
                const float re1 = R * e1;
                float T = e0 < re1 ? __builtin_fmaxf(re1, e0 * invR) : re1;
                T += __builtin_fabsf(T) * 4.76837158203125e-07f;        // 2^-21: the roundings of e1, R e1, 1 / R and e0 / R
                Tl[nj] = T;
                const float x = T + off, xF = T + offF;
                thr[nj] = dead ? -R3DM_INF : x + __builtin_fabsf(x) * 2.384185791015625e-07f;      // 2^-22: the rounding of x
                thrF[nj] = dead ? -R3DM_INF : xF + __builtin_fabsf(xF) * 2.384185791015625e-07f;
                const float xH = thrF[nj] + mgn;
                thrH[nj] = dead ? -R3DM_INF : xH + __builtin_fabsf(xH) * 2.384185791015625e-07f;   // 2^-22: the rounding of xH
                const float xS = thrF[nj] - loss;
                thrS[nj] = (dead || !(thrF[nj] < R3DM_INF)) ? -R3DM_INF : xS - __builtin_fabsf(xS) * 2.384185791015625e-07f;      // rounded down
            }
        };
        // one tile: `live` says whether `prev` holds keys to fold, and afterwards whether `cur` does
        auto tile = [&](uint32_t t, f32x16 (&cur)[NJ], const f32x16 (&prev)[NJ], bool live) __attribute__((always_inline)) -> bool {
            if constexpr (H)
                l2_halfnorm_tile_filter<GH, NJ, PF, MIN>(rh, rn, voffA, voffN, t * tileHB, (t + 1) * 128u, abuf, nrm, bq1, cur, prev, st,
                                                    (t - 1) * 32u + hb, live);
            else
                l2_pairnorm_tile_filter<GR, NJ, PF>(rr, rn, voffA, voffN, t * tileRB, (t + 1) * 128u, abuf, nrm, bq1, cur, prev, st,
                                                    (t - 1) * 32u + hb, live);
            if (live) { refresh(); pruned_under_thr = false; }
            n_tested += 1u;
            // a lane objects when one of its level-1 keys is not above its threshold (written so that a NaN key objects)
            // (MODE 4 and 5 leave tile 0 to the three levels, so that the lists hold rows and no query goes to the exact scan)
            if constexpr (L1_UNDECIDED) {               // (timing only: level 1 without its decision -- one add per query tile keeps the MFMAs)
                if (t != 0) {
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj) sink += cur[nj][0];
                    n_pruned += 1u;
                    return false;
                }
            }
            bool obj = false;
            float m[NJ];                                // (the min form: the smallest of the lane's keys, per query tile)
            if constexpr (MIN) {
                tile_key_min<NJ>(cur, m);
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj) obj |= !(m[nj] > thrH[nj]);
            } else {
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) obj |= !(cur[nj][r] > (H ? thrH[nj] : thrF[nj]));
            }
            if (__builtin_amdgcn_ballot_w64(obj) == 0ull) {
                n_pruned += 1u; n_filtered += 1u; pruned_under_thr = true;
                if constexpr (H) n_half += 1u;
                return false;
            }
            if constexpr (L1_ALONE) { if (t != 0) { n_pruned += 1u; return false; } }      // (timing only: level 1 alone -- no tile behind tile 0 goes on)
            // (two levels, MODE 21: the filter alone -- the restart never stops a tile)
            // (with the f16 prefix test: the restart's prefix test on the rows rounded to f16 first -- no lane has a key that is not above
            //  its thrQ -> the restart would prune the tile, so it is pruned here; else the restart as ever, its verdict its own)
            auto restart = [&]() __attribute__((always_inline)) -> bool {
                if constexpr (Q16) {
                    l2_prefix16_tile_stream<GP / 2, NJ>(rp, rn, voffA, voffN, t * tileQB, poff + t * 128u, rqp, soffQB, cur);
                    // thrQ = thr + marginQ, rounded up: made here from the lane's terms, where 4 % of the tiles come by -- a register per
                    // query tile that lived through the loop would not fit (-inf for a dead lane, +inf while thr is +inf)
                    float thrQ[NJ];
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj) {
                        float nbs, off, offF, mgn, loss, mgnQ;
                        const bool dead = lane_terms(nj, nbs, off, offF, mgn, loss, mgnQ);
                        const float xQ = thr[nj] + mgnQ;
                        thrQ[nj] = dead ? -R3DM_INF : xQ + __builtin_fabsf(xQ) * 2.384185791015625e-07f;   // 2^-22: the rounding of xQ
                    }
                    bool objq = false;
                    if constexpr (MIN) {
                        float mq[NJ];
                        tile_key_min<NJ>(cur, mq);
#pragma unroll
                        for (int nj = 0; nj < NJ; ++nj) objq |= !(mq[nj] > thrQ[nj]);
                    } else {
#pragma unroll
                        for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                            for (int r = 0; r < 16; ++r) objq |= !(cur[nj][r] > thrQ[nj]);
                    }
                    if (__builtin_amdgcn_ballot_w64(objq) == 0ull) { n_pruned += 1u; n_prefix16 += 1u; pruned_under_thr = true; return false; }
                }
                const bool on = l2_prune_tile_restart<G, GP, NJ, H || ABL == 0, MIN>(ra, rn, voffA, voffN, t * tileB, t * 128u, poff + t * 128u, rqt, soffQ, cur, thr);
                if (!on) { n_pruned += 1u; pruned_under_thr = true; }
                return on;
            };
            // level 2 cannot prune a tile that holds a finite f16 key at or below thrS (the header comment): such a tile skips it.  Only
            // the tiles that object get here, so the second pass over the keys is off level 1's path.  The skip has a copy of the restart
            // to itself: with one copy entered from both sides the register allocator spills 70 registers, with two it spills none
            if constexpr (H && ABL == 0) {
                bool far = false;
                if constexpr (MIN) {                    // (no key is -inf: the same minimum answers)
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj) far |= m[nj] <= thrS[nj];
                } else {
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                        for (int r = 0; r < 16; ++r) far |= (cur[nj][r] <= thrS[nj]) && (cur[nj][r] > -R3DM_INF);
                }
                if (__builtin_amdgcn_ballot_w64(far) != 0ull) { n_skip += 1u; return restart(); }
            }
            if constexpr (H && ABL != 1) {
                l2_pairnorm_tile_stream<GR, NJ>(rr, rn, voffA, voffN, t * tileRB, t * 128u, rqr, soffQR, cur);
                obj = false;
                if constexpr (MIN) {
                    tile_key_min<NJ>(cur, m);
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj) obj |= !(m[nj] > thrF[nj]);
                } else {
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                        for (int r = 0; r < 16; ++r) obj |= !(cur[nj][r] > thrF[nj]);
                }
                if (__builtin_amdgcn_ballot_w64(obj) == 0ull) { n_pruned += 1u; n_filtered += 1u; pruned_under_thr = true; return false; }
            }
            return restart();
        };
        bool live = false;
        uint32_t t = 0;
        for (; t + 1 < ntI; t += 2) {
            live = tile(t, accA, accB, live);
            live = tile(t + 1, accB, accA, live);
        }
        // (three levels: the lane's half once more, from the lane counter -- nothing of it has to live through the loop, whose registers
        //  are all taken)
        if constexpr (H) hb = 4u * (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) >> 5);
        if (t < ntI) {
            if (tile(t, accA, accB, live)) {
#pragma unroll
                for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) top2_push(st[nj], accA[nj][r], t * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
            }
        } else if (live) {
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
                for (int r = 0; r < 16; ++r) top2_push(st[nj], accB[nj][r], (ntI - 1) * 32u + hb + (uint32_t)((r & 3) + 8 * (r >> 2)));
        }
    }

    // plT -> the lower bound of the pruned rows' distances (a lane whose query does not exist holds none)
    const uint32_t lane_e = H ? __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) : lane, he = lane_e >> 5, ce = lane_e & 31u;      // (= lane, h, c: as above)
    float pruned_lb[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        if (pruned_under_thr) plT[nj] = __builtin_fminf(plT[nj], Tl[nj]);
        const bool dead = !((qt0 + (uint32_t)nj) * 32u + ce < nJ);
        pruned_lb[nj] = dead ? -R3DM_INF : plT[nj];
    }
    if (lane_e == 0 && n_tested) {
        atomicAdd(&P.prune_cnt->n_tested, (unsigned long long)n_tested);
        if (n_pruned) atomicAdd(&P.prune_cnt->n_pruned, (unsigned long long)n_pruned);
        if (n_filtered) atomicAdd(&P.prune_cnt->n_filtered, (unsigned long long)n_filtered);
        if (n_half) atomicAdd(&P.prune_cnt->n_half, (unsigned long long)n_half);         // (both stay 0 with two levels)
        if (n_skip) atomicAdd(&P.prune_cnt->n_skip, (unsigned long long)n_skip);
        if (n_prefix16) atomicAdd(&P.prune_cnt->n_prefix16, (unsigned long long)n_prefix16);
        if constexpr (L1_UNDECIDED) { if (sink == 12345.0f) atomicAdd(&P.prune_cnt->n_skip, 1ull); }
    }
    l2_finish_queries<NJ, false, false, true>(P, pair, Ip, Jp, st, qt0, he, ce, (float)(G * 8), false, 1.0f, 0.0f, nullptr, pruned_lb);
}

// The pruning kernel serves ratio tests that leave it room: near R = 1 a row matters up to the runner-up's distance, no prefix
// rules a tile out and the test only costs.  tools/prefix_prune_model.py on the synthetic SIFT collection (profiles/
// prefix_prune_model_c2.txt): 96 % of the tiles stop at R = 0.36 (ratio 0.6), 72 % at R = 0.49 (ratio 0.7), 6 % at R = 0.64.
// With the pair-norm filter in front the bound stays (tools/prefix_prune_model.py --filter pairnorm, profiles/
// pairnorm_filter_model_c2.txt): at R = 0.49 the cascade still leaves less work than the plain kernel, at R = 0.64 neither test stops tiles.
constexpr float kPruneMaxR = 0.5f;

bool l2_prune_serves(uint32_t G, bool prune, bool raw_knn, float ratio_R)
{
    return G == 16 && prune && !raw_knn && ratio_R > 0.0f && ratio_R <= kPruneMaxR;
}

uint32_t l2_prefix_groups()
{
#ifdef R3DM_DEVTOOLS
    static const int variant = r3dm_dev_knob("R3DM_L2_VARIANT", 3);
    if (variant >= 109 && variant <= 112) return (uint32_t)(variant - 100);
#endif
    return kPrefixGroups;
}

template <int G, int NJ, int PF, int PIPE, int WPS>
static hipError_t launch_l2_t(hipStream_t st, const MatchParams& P, uint32_t max_nj_tiles)
{
    return launch_pair_kernel(l2_knn2_mfma_kernel<G, NJ, PF, PIPE, WPS>, NJ, true, st, P, max_nj_tiles);
}
template <int G, int GP, int NJ, int PF, int WPS>
static hipError_t launch_l2_prune_t(hipStream_t st, const MatchParams& P, uint32_t max_nj_tiles)
{
    return launch_pair_kernel(l2_knn2_prune_kernel<G, GP, NJ, PF, WPS>, NJ, true, st, P, max_nj_tiles);
}
template <int G, int GP, int NJ, int PF, int WPS, int MODE>
static hipError_t launch_l2_half_t(hipStream_t st, const MatchParams& P, uint32_t max_nj_tiles)
{
    return launch_pair_kernel(l2_knn2_half_kernel<G, GP, NJ, PF, WPS, MODE>, NJ, true, st, P, max_nj_tiles);
}

// The A/B variants below (tools/ab_l2.py) -- including two ablations whose results are meaningless (timing only) -- exist
// only in the developer build (-DR3DM_DEVTOOLS -> regard3d_amd/libr3dm_dev.so, build.sh dev); the product library compiles
// one kernel per descriptor length and never reads the environment.
hipError_t launch_l2_knn2(hipStream_t st, const MatchParams& P, uint32_t G, uint32_t max_nj_tiles, bool integer_mfma)
{
    if (integer_mfma) {
        const hipError_t e = launch_l2_knn2_int(st, P, G, max_nj_tiles);      // kernels_match_16bit.hip; hipErrorNotSupported: no bf16 kernel for this G
        if (e != hipErrorNotSupported) return e;                              // (G = 18, LIOP, never integer: f32 tiles)
    }
#ifdef R3DM_DEVTOOLS
    // R3DM_L2_VARIANT selects a build of the kernel for A/B measurements (tools/ab_l2.py):
    //   0 epilogue after the MFMAs | 1 software-pipelined epilogue | 3 pipelined + wave-wide test-and-skip
    //   (default) | 9 ablation without epilogue (timing only) | 13 / 43: NJ = 1 x 3 waves/SIMD, NJ = 4 x 1 wave/SIMD
    static const int variant = r3dm_dev_knob("R3DM_L2_VARIANT", 3);
    if (G == 16) {
        switch (variant) {
            case 0:  return launch_l2_t<16, 2, 4, 0, 2>(st, P, max_nj_tiles);
            case 1:  return launch_l2_t<16, 2, 4, 1, 2>(st, P, max_nj_tiles);
            case 9:  return launch_l2_t<16, 2, 4, 9, 2>(st, P, max_nj_tiles);
            case 13: return launch_l2_t<16, 1, 4, 3, 3>(st, P, max_nj_tiles);
            case 43: return launch_l2_t<16, 4, 4, 3, 1>(st, P, max_nj_tiles);
            default: break;
        }
    }
    if (G == 18 && variant == 0) return launch_l2_t<18, 2, 3, 0, 2>(st, P, max_nj_tiles);
    if (G == 18 && variant == 2) return launch_l2_t<18, 2, 2, 3, 2>(st, P, max_nj_tiles);
    //   109 .. 112: the prefix test alone (the cascade without its filter) with GP = 9 .. 12 prefix groups (registration writes the
    //   prefix norms of the same variant) | 120: the filter alone (no tile stops at the prefix test)
    if (l2_prune_serves(G, P.prune != 0, P.knn_idx != nullptr, P.ratio_R)) {
        switch (variant) {
            case 109: return launch_l2_prune_t<16, 9, 2, 1, 2>(st, P, max_nj_tiles);
            case 110: return launch_l2_prune_t<16, 10, 2, 2, 2>(st, P, max_nj_tiles);
            case 111: return launch_l2_prune_t<16, 11, 2, 1, 2>(st, P, max_nj_tiles);
            case 112: return launch_l2_prune_t<16, 12, 2, 2, 2>(st, P, max_nj_tiles);
            case 120: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 2, 2, 21>(st, P, max_nj_tiles);
            default: break;
        }
        //   130: the f16 level, then straight to the restart (no f32 filter; timing only) | 131 / 132: the three levels with a
        //   window of 1 / 2 blocks instead of 4 | 133: the three levels without the skip of level 2 (results and older counters unchanged)
        if ((P.prune & 2u) != 0) {
            switch (variant) {
                case 130: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 1>(st, P, max_nj_tiles);
                case 131: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 1, 2, 0>(st, P, max_nj_tiles);
                case 132: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 2, 2, 0>(st, P, max_nj_tiles);
                case 133: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 2>(st, P, max_nj_tiles);
                //   134: level 1 alone, no tile ever goes on | 135: level 1 alone without its decision (both timing only) | 136: the
                //   general form of the tile tests where the min form would run (results and counters unchanged)
                case 134: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 4>(st, P, max_nj_tiles);
                case 135: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 5>(st, P, max_nj_tiles);
                case 136: return (P.prune & 8u) ? launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 6>(st, P, max_nj_tiles)
                                                : launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 0>(st, P, max_nj_tiles);
                //   137 / 138: 134 / 135 in the min form | 139: the three levels without the f16 prefix test where it would run
                //   (results and older counters unchanged)
                case 137: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 8>(st, P, max_nj_tiles);
                case 138: return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 9>(st, P, max_nj_tiles);
                case 139: return (P.prune & 4u) ? launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 3>(st, P, max_nj_tiles)
                                                : launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 0>(st, P, max_nj_tiles);
                default: break;
            }
        }
    }
#endif
    // match mode on 128-dimensional rows: the kernels that stop tiles early (r3dm_set_prefix_pruning, default on) -- with the f16
    // level in front (r3dm_set_half_filter, default on: MatchParams::prune bit 1) or the cascade alone.  The f16 level reaches as far
    // as the cascade does (kPruneMaxR): it prunes what the filter prunes, at a sixteenth of the matrix cycles, and where the filter
    // stops few tiles it adds 256 cycles to a tile of 4,096 and more (profiles/half_filter_model_c2.txt has R = 0.49).
    if (l2_prune_serves(G, P.prune != 0, P.knn_idx != nullptr, P.ratio_R)) {
        // ... and with the tile tests in their min form where the batch's norms allow it (run_match_batch: MatchParams::prune bit 2)
        // ... and with the f16 prefix test in front of the restart (r3dm_set_half_prefix: MatchParams::prune bit 3), in either form
        if ((P.prune & 14u) == 14u) return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 7>(st, P, max_nj_tiles);
        if ((P.prune & 10u) == 10u) return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 6>(st, P, max_nj_tiles);
        if ((P.prune & 6u) == 6u) return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 3>(st, P, max_nj_tiles);
        if ((P.prune & 2u) != 0) return launch_l2_half_t<16, (int)kPrefixGroups, 2, 4, 2, 0>(st, P, max_nj_tiles);
        return launch_l2_half_t<16, (int)kPrefixGroups, 2, 2, 2, 20>(st, P, max_nj_tiles);
    }
    switch (G) {
        case 8:  return launch_l2_t<8, 2, 4, 3, 2>(st, P, max_nj_tiles);
        case 16: return launch_l2_t<16, 2, 4, 3, 2>(st, P, max_nj_tiles);
        case 18: return launch_l2_t<18, 2, 3, 3, 2>(st, P, max_nj_tiles);
        case 32: return launch_l2_t<32, 1, 4, 3, 2>(st, P, max_nj_tiles);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace r3dm
