// The fold of the deterministic reductions: the one device text of the order that the
// oracle (oracle/yalla_host.hpp, YA_REDUCE_TREE) and the numpy statement
// (tests/test_reference_statement_numpy.py, fold256) restate.  Shared by libyalla_hip.so's reduction kernels
// (yalla_amd/csrc/core.hip) and the update kernels that fold partial sums themselves (solvers.cuh, ensemble.cuh).
#pragma once

#include <hip/hip_runtime.h>

namespace ya {

// Every thread of a 256-thread workgroup calls it with its NW running sums; afterwards sh[k * 256] is the
// workgroup's sum of component k (sh: NW * 256 floats of LDS).
template<int NW>
__device__ __forceinline__ void fold256(float (&acc)[NW], float* sh /* [NW][256] */)
{
    // lane[t] += lane[t + s] for s = 128 ... 1 (the documented order).  Round 5: from s = 32 down the
    // operands sit in ONE wavefront and travel by shuffle instead of through LDS and a workgroup
    // barrier per step -- the same additions of the same operands, so the same bits: a reduction
    // kernel is 8 barriers shorter (4.9 -> 3.4 us per launch at any size).
#pragma unroll
    for (int k = 0; k < NW; k++) sh[k * 256 + threadIdx.x] = acc[k];
    __syncthreads();
    if ((int)threadIdx.x < 128) {
#pragma unroll
        for (int k = 0; k < NW; k++)
            sh[k * 256 + threadIdx.x] = sh[k * 256 + threadIdx.x] + sh[k * 256 + threadIdx.x + 128];
    }
    __syncthreads();
    if ((int)threadIdx.x < 64) {
        float v[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) v[k] = sh[k * 256 + threadIdx.x] + sh[k * 256 + threadIdx.x + 64];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int k = 0; k < NW; k++) v[k] = v[k] + __shfl_down(v[k], s, 64);
        }
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < NW; k++) sh[k * 256] = v[k];
        }
    }
    __syncthreads();
}

}  // namespace ya
