// kernels_filter_e.hip -- the essential-matrix instantiations of the one-workgroup-per-pair AC-RANSAC kernel
// (acransac_kernel<2, *>; filter_device.hpp, filter_acransac.inc).  They are their own translation unit only to compile in
// parallel with the F / H instantiations of kernels_filter.hip: the 5-point solver is the slowest thing to compile in the library.
// No special compiler options (build.sh).  (Round 2 needed -mllvm -amdgpu-spill-sgpr-to-vgpr=0 here: the one-lane 5-point solver
// was called out of line from divergent control flow and SGPRs spilled into VGPR lanes across the calls gave run-to-run different
// inlier sets.  The cooperative solver, five_point_coop, has no calls and no spills; the option is gone, and
// tests/test_gpu_fullsize.py::test_filters_are_deterministic_when_workgroups_share_a_cu runs against the default build.)

#include "filter_device.hpp"
#include "filter_acransac.inc"

namespace r3dm {

// lds = filter_F_lds_bytes(P.m_cap, 2): called by launch_filter_F (kernels_filter.hip)
hipError_t launch_filter_E(hipStream_t st, const FilterParams& P, size_t lds)
{
    return P.wide ? launch_acransac<2, 512>(st, P, lds) : launch_acransac<2, 256>(st, P, lds);
}

}  // namespace r3dm
