// kernels_filter.hip -- the fundamental-matrix and homography instantiations of the one-workgroup-per-pair AC-RANSAC kernel
// (acransac_kernel<0, *>, acransac_kernel<1, *>), the size of its dynamic LDS region, and the launcher of all three filters.
// The device routines are filter_device.hpp, the kernel is filter_acransac.inc.

#include "filter_device.hpp"
#include "filter_acransac.inc"

namespace r3dm {

size_t filter_F_lds_bytes(uint32_t m_cap, int model_kind)
{
    // [FState, padded to 1024][histogram: 1024 x u32][Fs: chunk x (9 x MAX_MODELS) doubles][scout: totals, bounds, offsets][keys: m_cap x u64][idx: m_cap x u32]
    const size_t ms = model_kind == 2 ? 90 : 27;
    const size_t chunk = model_kind == 2 ? kE5Samples : kChunk;
    size_t sort_bytes = (size_t)m_cap * 12;
    if (model_kind == 2 && sort_bytes < (size_t)kE5Samples * kE5Stride * 8) sort_bytes = (size_t)kE5Samples * kE5Stride * 8;   // 5-point workspaces
    if (sort_bytes < (size_t)kScoutHistBytes) sort_bytes = (size_t)kScoutHistBytes;                                                // the scout pass's per-wave histograms
    return (size_t)kHdr + chunk * ms * 8 + kScoutBytes + sort_bytes;
}

hipError_t launch_filter_F(hipStream_t st, const FilterParams& P)
{
    if (P.n_short == 0) return hipSuccess;
    const size_t lds = filter_F_lds_bytes(P.m_cap, P.model_kind);
    if (P.model_kind == 2) return launch_filter_E(st, P, lds);
    if (P.model_kind == 0) return P.wide ? launch_acransac<0, 512>(st, P, lds) : launch_acransac<0, 256>(st, P, lds);
    return P.wide ? launch_acransac<1, 512>(st, P, lds) : launch_acransac<1, 256>(st, P, lds);
}

}  // namespace r3dm
