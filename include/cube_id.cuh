// The cube id of a point: the one device text of the reference's binary32 expression (solvers.cuh:357-360),
// which the oracle restates (oracle/yalla_host.hpp).  Shared by libyalla_hip.so's grid build
// (yalla_amd/csrc/core.hip, k_bin), the ensemble's batched grid build (ensemble_grid.cuh) and the update kernels
// that bin the entries they store (solvers.cuh, ya::bin_entry).  Compile with -ffp-contract=off: the arithmetic is
// the plain IEEE evaluation, statement by statement.
//
// Where the translation unit contracts -- the fast tier's update kernels, -ffp-contract=fast -- the pragma below is
// DISREGARDED (only fast-honor-pragmas honours it; __fmul_rn / __fadd_rn are plain `*` / `+` in HIP and do not
// prevent contraction either): that build has v_fmac_f32 for `fx + fy` and for `(..) + fz`.  The ids agree all the
// same, because the arithmetic is exact: floorf(..) + half, the products by gs and the sums are integers, and while
// the grid has fewer than 2^24 cubes every one of them is below 2^24 in magnitude, where binary32 holds every
// integer -- fused or not, nothing is rounded.  (x / cs stays a true division in both builds.)
// tests/test_fast_tier_carry_gpu.py holds that build's binning to the bits of libyalla_hip.so's k_bin.
#pragma once

#include <hip/hip_runtime.h>

namespace ya {

// solvers.cuh:357-360 evaluated in float, left to right:
//   (floor(x/cs) + gs/2) + (floor(y/cs) + gs/2)*gs + (floor(z/cs) + gs/2)*gs*gs
__device__ __forceinline__ int cube_id_of(float x, float y, float z, float cs, int gs)
{
#pragma clang fp contract(off)  // (honoured under fast-honor-pragmas and on; see above for -ffp-contract=fast)
    const float half = (float)(gs / 2);
    const float fgs = (float)gs;
    float fx = floorf(x / cs) + half;
    float fy = (floorf(y / cs) + half) * fgs;
    float fz = ((floorf(z / cs) + half) * fgs) * fgs;
    return (int)((fx + fy) + fz);
}

}  // namespace ya
