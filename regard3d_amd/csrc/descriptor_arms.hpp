// descriptor_arms.hpp -- the one table of the descriptor arms of the features stage (host only, nothing but the public header: the library
// and the facade include it, and a host test compiles it alone).  What an arm is -- its id, its names in the error texts, its regions type
// and row size, the level table of the Fast-A-KAZE detector it needs -- stands here and nowhere else ("The descriptor arms");
// regard3d_amd/api.py keeps the same rows for Python, and tests/test_descriptor_arms.py holds the two to each other.
#pragma once

#include "../../include/r3dm.h"

#include <cmath>

struct DescriptorArm {
    int id;                        // R3DM_DESCRIPTOR_*
    const char* name;              // as the refusal of the classic detector names it
    const char* tag;               // as the arm's own error texts begin
    const char* macro;
    r3dm_dtype dtype;              // the regions type: what setRegionsType and r3dm_set_image take ...
    uint32_t dim;
    uint32_t row_bytes;            // ... and the bytes of a row of the .desc file, of the sink and of the detect entries
    float border_mult;             // the Fast detector's level table it needs: border = fRound(border_mult sqrt(2) sigma_size) + 1 (ak_smax)
    bool level_planes;             // reads the Fast-A-KAZE level planes: one launch over items (api_akaze.cpp), refused with the classic detector
};

inline constexpr DescriptorArm kDescriptorArms[] = {
    {R3DM_DESCRIPTOR_LIOP, "LIOP", "LIOP", "R3DM_DESCRIPTOR_LIOP", R3DM_F32, 144, 144 * 4, 10.0f, false},
    {R3DM_DESCRIPTOR_MLDB, "MLDB", "MLDB", "R3DM_DESCRIPTOR_MLDB", R3DM_BIN, 61, 61, 10.0f, true},
    {R3DM_DESCRIPTOR_MSURF, "M-SURF-64", "M-SURF", "R3DM_DESCRIPTOR_MSURF", R3DM_F32, 64, 64 * 4, 12.0f, true},
};

// null for an id no arm has (2 is reserved and unassigned)
inline const DescriptorArm* descriptor_arm_by_id(int id) { for (const DescriptorArm& a : kDescriptorArms) if (a.id == id) return &a; return nullptr; }
// null for a regions type no arm writes
inline const DescriptorArm* descriptor_arm_by_type(int dtype, uint32_t dim)
{
    for (const DescriptorArm& a : kDescriptorArms) if ((int)a.dtype == dtype && a.dim == dim) return &a;
    return nullptr;
}

// border factor of the Fast arm's level table (Allocate_Memory_Evolution, fast-akaze AKAZEFeatures.cpp:78-84,105,112: border =
// fRound(smax sigma_size) + 1): 10 sqrt(2) under MLDB -- the table of the detector, LIOP and MLDB entries -- and 12 sqrt(2) under the
// KAZE descriptors, i.e. M-SURF-64, whose samples reach that far.  In float: the borders are rounded from it, and passes compare it.
inline float ak_smax(float border_mult) { return border_mult * sqrtf(2.0f); }
inline float ak_smax(const DescriptorArm& arm) { return ak_smax(arm.border_mult); }
