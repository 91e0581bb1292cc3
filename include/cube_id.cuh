// The cube id of a point: the one device text of the reference's binary32 expression (solvers.cuh:357-360),
// which the oracle restates (oracle/yalla_host.hpp).  Shared by libyalla_hip.so's grid build
// (yalla_amd/csrc/core.hip, k_bin) and the ensemble's batched grid build (ensemble_grid.cuh).  Compile with
// -ffp-contract=off: the arithmetic is the plain IEEE evaluation, statement by statement.
#pragma once

#include <hip/hip_runtime.h>

namespace ya {

// solvers.cuh:357-360 evaluated in float, left to right:
//   (floor(x/cs) + gs/2) + (floor(y/cs) + gs/2)*gs + (floor(z/cs) + gs/2)*gs*gs
__device__ __forceinline__ int cube_id_of(float x, float y, float z, float cs, int gs)
{
#pragma clang fp contract(off)  // (also where the translation unit contracts: the fast tier's update kernels bin)
    const float half = (float)(gs / 2);
    const float fgs = (float)gs;
    float fx = floorf(x / cs) + half;
    float fy = (floorf(y / cs) + half) * fgs;
    float fz = ((floorf(z / cs) + half) * fgs) * fgs;
    return (int)((fx + fy) + fz);
}

}  // namespace ya
