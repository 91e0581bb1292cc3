// One lane's share of a grid build's binning: the clamp of a raw cube id (ya::cube_id_of) into the grid and into
// the promised cube range, with the two status bits, and the arrival rank from one returning atomic on
// count[cube] per run of equal ids in the wavefront.  The one device text of it, shared by libyalla_hip.so's
// k_bin (yalla_amd/csrc/core.hip) and the update kernels of a carried step (include/solvers.cuh: euler_step and
// heun_step_sorted bin the entry they have just computed, so the rebuild behind them needs no k_bin launch).
#pragma once

#include <hip/hip_runtime.h>

#include "cube_id.cuh"
#include "yalla_hip.h"

namespace ya {

// What a binning lane needs of a grid (ya_grid_bin_target) and of the build: the cube size.
struct Grid_bin {
    ya_grid_bin_target grid{};
    float cube_size = 0.f;
};

// EVERY lane of the wavefront must call it (shuffles and a ballot): a lane without a cell passes cell = -1
// (and any cube), a lane with one its id (>= 0) and the raw cube id.  Leaves in `cube` the id the cell is
// counted under, -1 for no cell, and returns the cell's arrival rank in that cube's counter.  Workgroups are
// one-dimensional and a multiple of 64 wide, so threadIdx.x & 63 is the lane.
__device__ __forceinline__ int bin_lane(const int cell, int& cube, const int n_cubes, const int range_lo,
    const int range_hi, int* __restrict__ count, int* __restrict__ status)
{
    int id = -1;
    if (cell >= 0) {
        id = cube;
        if (id < 0 || id >= n_cubes) {
            atomicOr(status, YA_STATUS_OUT_OF_GRID);
            id = id < 0 ? 0 : n_cubes - 1;
        }
        // ya_grid_set_cube_range: the caller promised cube ids in [range_lo, range_hi) and the
        // prefix sum only covers those; a cell outside is reported and kept inside (memory-safe)
        if (id < range_lo || id >= range_hi) {
            atomicOr(status, YA_STATUS_OUT_OF_RANGE);
            id = id < range_lo ? range_lo : range_hi - 1;
        }
    }
    // Wave-aggregated counting: in visit order equal cube ids sit in adjacent
    // lanes, so each run of equal ids issues ONE atomic (by its first lane, for
    // the run length) instead of one per lane on the same counter.  Any
    // arrival order inside a cube is fine: k_order restores ascending ids.
    const int lane = threadIdx.x & 63;
    const int id_before = __shfl_up(id, 1, 64);
    const bool head = lane == 0 || id != id_before;
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = heads & (~0ULL >> (63 - lane));          // heads in lanes <= lane
    const unsigned long long after = lane == 63 ? 0ULL : heads & (~0ULL << (lane + 1));
    const int head_lane = 63 - __builtin_clzll(upto);
    const int run_end = after ? __builtin_ctzll(after) : 64;
    int base = 0;
    if (head && id >= 0) base = atomicAdd(&count[id], run_end - lane);
    base = __shfl(base, head_lane, 64);
    cube = id;
    return base + (lane - head_lane);
}

// An update kernel's lane bins the entry it has just stored in slot s (has_cell: s < n; every lane of the
// wavefront calls): what k_bin would leave in cube_of[s], rank[s] and count[] from that entry, and the same
// status bits.
__device__ __forceinline__ void bin_entry(const Grid_bin& b, const bool has_cell, const int s, const float x,
    const float y, const float z)
{
    int cube = has_cell ? cube_id_of(x, y, z, b.cube_size, b.grid.grid_size) : -1;
    const int rank = bin_lane(has_cell ? s : -1, cube, b.grid.n_cubes, b.grid.range_lo, b.grid.range_hi,
        b.grid.d_count, b.grid.d_status);
    if (has_cell) {
        b.grid.d_cube_of[s] = cube;
        b.grid.d_rank[s] = rank;
    }
}

}  // namespace ya
