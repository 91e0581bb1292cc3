// Ordered link forces for Ensemble<Pt, Tile_solver> and Ensemble<Pt, Grid_solver> (ensemble_grid.cuh: inside its
// launches that step from LDS too) and, as a generic force, for the Gabriel form.
// Part of ensemble.cuh, which includes it behind the LDS layout and before the whole-step kernels that use it; a
// model includes ensemble.cuh.
//
//     Links protrusions{n_replicas * S, strength};      // the reference's own Links, over the flat id space
//     cells.take_steps<my_force>(dt, K, ya::ens::Replica_links{protrusions, S});
//
// THE CONTRACT  Slot s of `links` belongs to replica s / S (S = slots_per_replica; links.n_max >= n_replicas * S),
// its ends are ensemble-global ids, slots s >= *links.d_n are unused (the count is read on the device at every
// launch, as ya link kernels do), a slot with a == b is inert.  A slot is SKIPPED if either end lies outside the rows
// [r * n_max, r * n_max + n_r) of its own replica: whatever a model leaves in d_link, nothing here indexes outside
// the slot's replica.  THIS DIFFERS from link_forces (links.cuh), whose atomics touch whatever row a link names.
//
// THE ARITHMETIC is linear_force's, statement by statement: r = X[a] - X[b], dist = sqrtf(fmaf(z, z, fmaf(y, y,
// x x))), f = strength r / dist per component, end a gets -f, end b gets +f.  A cell's terms are added in ASCENDING
// SLOT ORDER to a sum that starts at +0 -- the order of the CPU restatement's serial loop, and one of the orders the
// atomics may take -- the stage's right-hand side starts as {L.x, L.y, L.z, 0, ...} and the pairwise forces are added
// to it by store_rhs(..., has_gen = true, ...): the operations of "zero, gen_forces, force kernel".
//
// TWO IMPLEMENTATIONS, ONE SET OF BITS  ya::ens::link_forces_ordered<Pt>(Replica_links, n_rows, n_max, d_n, d_X, d_dX)
// is a batched global kernel, an ordinary generic force (one thread per cell walks its replica's slots): n_rows is
// the flat row count gen_forces is called with, n_replicas * n_max -- the launch's size, which a Links object whose
// n_max is only AT LEAST n_replicas * S cannot tell -- n_max and d_n are the ensemble's.  Inside a whole-step launch
// (whole_steps_linked, ensemble.cuh) the workgroup builds, once per launch, a per-cell incidence list in LDS --
// 4 (n_max + 1) + 8 S bytes -- and every stage starts with one thread per cell walking the cell's entries, from the
// stage's LDS positions.  No atomics, no scratch.
#pragma once

#ifndef YA_ENSEMBLE_LINKS_FROM_ENSEMBLE_CUH
#error "include ensemble.cuh: ensemble_links.cuh is a part of it"
#endif

#include "links.cuh"

namespace ya {
namespace ens {

struct Replica_links {
    Links& links;
    int slots_per_replica;
};

// What the kernels are handed of a Replica_links.
struct Links_view {
    const Link* d_link = nullptr;
    const int* d_n = nullptr;  // slots in use, read on the device
    int n_slots = 0;           // links.n_max
    int slots_per_replica = 0;
    float strength = 0.f;
};
inline Links_view view_of(const Replica_links& rl)
{
    return Links_view{rl.links.d_link, rl.links.d_n, rl.links.n_max, rl.slots_per_replica, rl.links.strength};
}

// The replica's slots that are in use: [first, end).
struct Slots {
    int first, end;
};
__device__ __forceinline__ Slots slots_of(const Links_view& v, const int replica)
{
    const int used = min(*v.d_n, v.n_slots);
    const int first = replica * v.slots_per_replica;
    const int end = min(first + v.slots_per_replica, used);
    return Slots{first, end > first ? end : first};
}
// a == b is inert; an end outside the replica's n rows (which start at id first_row) skips the slot
__device__ __forceinline__ bool link_counts(const Link l, const unsigned first_row, const int n)
{
    return l.a != l.b && (unsigned)l.a - first_row < (unsigned)n && (unsigned)l.b - first_row < (unsigned)n;
}
// linear_force's f for the link (a, b): end a gets -f, end b +f
template<typename Pt>
__device__ __forceinline__ float3 link_pull(const Pt& Xa, const Pt& Xb, const float strength)
{
    const float x = Xa.x - Xb.x;
    const float y = Xa.y - Xb.y;
    const float z = Xa.z - Xb.z;
    const float dist = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
    return float3{strength * x / dist, strength * y / dist, strength * z / dist};
}
__device__ __forceinline__ void add_link_term(float3& L, const float3 f, const bool end_b)
{
    L.x = L.x + (end_b ? f.x : -f.x);
    L.y = L.y + (end_b ? f.y : -f.y);
    L.z = L.z + (end_b ? f.z : -f.z);
}

// One thread per cell of the flat launch: past its replica's count it returns; else it walks its replica's slots
// in order and adds its own terms to a sum from +0, which it then adds to its row of d_dX.
template<typename Pt>
__global__ __launch_bounds__(UPDATE_BLOCK) void link_ordered_batched(const Links_view v, const int n_rows, const int n_max,
    const int* __restrict__ d_n, const Pt* __restrict__ d_X, Pt* __restrict__ d_dX)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (unsigned)n_rows) return;
    const int replica = (int)(i / (unsigned)n_max);
    const int n = count_of(d_n, replica, n_max);
    const unsigned first_row = (unsigned)replica * (unsigned)n_max;
    if (i - first_row >= (unsigned)n) return;
    const Slots s = slots_of(v, replica);
    float3 L{0.f, 0.f, 0.f};
    for (int k = s.first; k < s.end; k++) {
        const Link l = v.d_link[k];
        if ((unsigned)l.a != i && (unsigned)l.b != i) continue;
        if (!link_counts(l, first_row, n)) continue;
        add_link_term(L, link_pull(d_X[l.a], d_X[l.b], v.strength), (unsigned)l.b == i);
    }
    Pt dX = d_dX[i];
    dX.x += L.x;
    dX.y += L.y;
    dX.z += L.z;
    d_dX[i] = dX;
}

// The ordered link forces of every replica as a generic force: n_rows = n_replicas * n_max, what gen_forces is
// called with; n_max and d_n are the ensemble's.  Queued on the null stream; nothing is read by the host.
template<typename Pt>
void link_forces_ordered(const Replica_links rl, const int n_rows, const int n_max, const int* d_n,
    const Pt* __restrict__ d_X, Pt* d_dX)
{
    assert(rl.slots_per_replica >= 0 && n_max > 0 && n_rows % n_max == 0);
    assert((size_t)(n_rows / n_max) * (size_t)rl.slots_per_replica <= (size_t)rl.links.n_max);
    if (n_rows <= 0 || rl.slots_per_replica == 0) return;
    link_ordered_batched<Pt><<<(unsigned)(((size_t)n_rows + UPDATE_BLOCK - 1) / UPDATE_BLOCK), UPDATE_BLOCK>>>(
        view_of(rl), n_rows, n_max, d_n, d_X, d_dX);
}

// ---- inside a whole-step launch --------------------------------------------------------------------------
// Where the incidence list lies in the launch's LDS is ya::ens::lds_layout's (ensemble.cuh): Lds_layout::list.

// The replica's incidence list, built once per launch by the whole workgroup (every thread calls it: barriers).
// sh_off[c] .. sh_off[c + 1] are cell c's entries in sh_ent, in slot order; an entry is the other end's local row,
// doubled, plus 1 if the cell is the link's end b.  Cell-thread t (rows t, t + 256, ...) scans the replica's slots in
// order and counts its ends; an exclusive scan over the counts (a thread sums 4 consecutive rows, the 256 sums are
// scanned in sh_scan, 256 ints) gives the offsets; a second scan of the slots fills each cell's entries.
__device__ __forceinline__ void whole_links_build(const Links_view& v, const int replica, const int n, const int n_max,
    int* sh_off, unsigned* sh_ent, int* sh_scan)
{
    constexpr int ROWS = WHOLE_STEP_MAX_ROWS / UPDATE_BLOCK;  // rows per cell-thread, and per thread of the scan
    const int t = threadIdx.x;
    const unsigned first_row = (unsigned)replica * (unsigned)n_max;
    const Slots s = slots_of(v, replica);
    int count[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; q++) count[q] = 0;
    for (int k = s.first; k < s.end; k++) {
        const Link l = v.d_link[k];
        if (!link_counts(l, first_row, n)) continue;
        const unsigned a = (unsigned)l.a - first_row, b = (unsigned)l.b - first_row;
#pragma unroll
        for (int q = 0; q < ROWS; q++) {
            const unsigned row = t + q * UPDATE_BLOCK;
            count[q] += (int)(a == row) + (int)(b == row);
        }
    }
#pragma unroll
    for (int q = 0; q < ROWS; q++)
        if (t + q * UPDATE_BLOCK < n) sh_off[t + q * UPDATE_BLOCK] = count[q];
    __syncthreads();
    int mine[ROWS], sum = 0;
#pragma unroll
    for (int q = 0; q < ROWS; q++) {
        mine[q] = ROWS * t + q < n ? sh_off[ROWS * t + q] : 0;
        sum += mine[q];
    }
    sh_scan[t] = sum;
    __syncthreads();
    for (int d = 1; d < UPDATE_BLOCK; d <<= 1) {
        const int before = t >= d ? sh_scan[t - d] : 0;
        __syncthreads();
        sh_scan[t] += before;
        __syncthreads();
    }
    int running = sh_scan[t] - sum;
#pragma unroll
    for (int q = 0; q < ROWS; q++) {
        if (ROWS * t + q <= n) sh_off[ROWS * t + q] = running;  // (row n: the end of the last cell's entries)
        running += mine[q];
    }
    if (t == UPDATE_BLOCK - 1 && n == ROWS * UPDATE_BLOCK) sh_off[n] = running;
    __syncthreads();
    int cursor[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; q++) cursor[q] = t + q * UPDATE_BLOCK < n ? sh_off[t + q * UPDATE_BLOCK] : 0;
    for (int k = s.first; k < s.end; k++) {
        const Link l = v.d_link[k];
        if (!link_counts(l, first_row, n)) continue;
        const unsigned a = (unsigned)l.a - first_row, b = (unsigned)l.b - first_row;
#pragma unroll
        for (int q = 0; q < ROWS; q++) {
            const unsigned row = t + q * UPDATE_BLOCK;
            if (a == row) sh_ent[cursor[q]++] = b << 1;
            if (b == row) sh_ent[cursor[q]++] = (a << 1) | 1u;
        }
    }
    __syncthreads();
}

// The start of a stage's right-hand sides, {L.x, L.y, L.z, 0, ...}: one thread per cell (thread t owns rows t,
// t + 256, ..., as in whole_stage_force) walks the cell's entries and evaluates each link from the stage's positions.
template<typename Pt>
__device__ __forceinline__ void whole_stage_links(const int n, const Pt* sh_in, Pt* sh_rhs, const int* sh_off,
    const unsigned* sh_ent, const float strength)
{
    for (int local = threadIdx.x; local < n; local += UPDATE_BLOCK) {
        const Pt Xi = sh_in[local];
        float3 L{0.f, 0.f, 0.f};
        const int end = sh_off[local + 1];
        for (int e = sh_off[local]; e < end; e++) {
            const unsigned entry = sh_ent[e];
            const Pt Xo = sh_in[entry >> 1];
            const bool end_b = entry & 1u;
            add_link_term(L, end_b ? link_pull(Xo, Xi, strength) : link_pull(Xi, Xo, strength), end_b);
        }
        Pt start = ya::zero<Pt>();
        start.x = L.x;
        start.y = L.y;
        start.z = L.z;
        sh_rhs[local] = start;
    }
}

}  // namespace ens
}  // namespace ya
