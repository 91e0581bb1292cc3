// Ensemble<Pt, Tile_solver>: M independent all-pairs systems of one point type and one functor,
// advanced together -- the same six launches per take_step whatever M is, and nothing read by the
// host: every kernel takes its replica's cell count from d_n[r] on the device.
// Ensemble<Pt, Grid_solver> (ensemble_grid.cuh, included at the end of this file) is the same for M
// Grid_solver systems: everything below holds for it too, except that "forces of a stage" are a batched grid
// build and a batched grid force.  The step -- stages, partial sums, the two update kernels -- exists once,
// in ya::ens::Stepper, which both forms derive from.
//
// One Tile_solver step of a few hundred cells is launch and host latency, not work (DESIGN.md
// section 9: 49 us for 800 cells), and a sweep over M such systems as M Solutions pays that M times
// per step, one system after the other.  Here the latency is paid once per step.
//
//     Ensemble<float3> cells{n_replicas, n_max};        // n_max = capacity of EACH replica
//     cells.h_n[r] = ...; *cells.row(r, i) = ...;       // fill replica r's rows 0 .. h_n[r] - 1
//     cells.copy_to_device();
//     cells.take_step<my_force>(dt);                    // all replicas, bit for bit what a lone
//                                                       // Solution<float3, Tile_solver> of each gives
//
// LAYOUT  One flat allocation per array, replica-major: replica r owns rows
// [r * n_max, r * n_max + n[r]) of h_X, d_X, d_old_v (and of the private right-hand sides);
// h_n[r] / d_n[r] are the counts.  Counts may differ and may be 0 (such a replica is left alone, as
// take_step leaves an empty Solution); model kernels may change d_n[r] between steps.
//
// IDS  Pairwise functors are called with ensemble-global ids i = r * n_max + local, j likewise: a
// model's per-cell arrays are sized n_replicas * n_max and indexed by i as always, `i == j` keeps its
// meaning, and a functor finds its replica as i / n_max (a sweep reads its per-replica parameter
// from the model's own device array that way).  Generic forces are called once per stage on the
// flat arrays, gen_forces(n_replicas * n_max, d_in, d_rhs), with the WHOLE right-hand side zeroed
// beforehand, unused rows included: Links and Property objects sized for the flat id space work
// unchanged.
//
// RESULTS  Every per-cell sum is accumulated in tile_force's order (j ascending over the replica's
// own rows), the centre of mass in ya_reduce_partials' order (B_r = clamp(ceil(n_r / 256), 1, 1024)
// blocks of the replica's rows, fold256, then the update kernels' fold of the B_r partials), the
// updates are Heun_solver's statements: each replica holds the bits a Solution<Pt, Tile_solver>
// run of the same rows holds (tests/test_ensemble_gpu.py, tests/native_ensemble).  The force loops, the
// fold and the corrector's row are the single-system kernels' own device functions (solvers.cuh:
// tile_force_rows, tile_force_coop_rows, heun_row; fold256.cuh): the kernels here add only where a
// workgroup finds its replica's rows, its count and its id offset.
//
// WHOLE STEPS  cells.take_steps<my_force>(dt, 100) is 100 calls of take_step, bit for bit; where a replica fits
// one workgroup's LDS (n_max <= ya::ens::whole_step_capacity<Pt>(), 1024 for the usual point types) and there are
// no generic forces, it can run as ONE launch per steps_per_launch steps: a workgroup per replica runs the whole
// steps from LDS (ya::ens::whole_steps, Ensemble::whole_steps) -- with 4, 16 or 64 lanes per cell for functors declared
// stateless (ya::ens::whole_steps_coop, Ensemble::whole_step_lanes), the same bits.
//
// LINKS  cells.take_steps<my_force>(dt, K, ya::ens::Replica_links{links, S}) steps with the ORDERED link forces of a
// Links object over the flat id space (ensemble_links.cuh: S slots per replica, a cell's terms added in slot order,
// no atomics): the one generic force that also runs inside whole-step launches (ya::ens::whole_steps_linked), the
// same bits as the six-launch step with ya::ens::link_forces_ordered as its generic force.
//
// Ensemble<Pt, Gabriel_solver> (ensemble_gabriel.cuh, included after it) is the same for M Gabriel_solver systems,
// on the grid form's build; its take_steps steps from LDS too (ya::ens::gabriel_lds_steps).
//
// PER-REPLICA dt  cells.take_step<my_force>(ya::ens::Replica_dt{d_dt}) and take_steps<my_force>(ya::ens::Replica_dt{d_dt},
// K[, gen_forces | links]) step replica r with d_dt[r]: n_replicas floats ON THE DEVICE, caller-owned, read by the
// kernels when they run (a model kernel queued before the call may have written them; the host reads nothing).  Every
// form, every path and every fixed mode; the path taken does not depend on it; each replica holds the bits of a lone
// Solution stepped with its value (0.0f is a value like any other).  Ensemble<Pt, Gabriel_solver>::d_gabriel_coefficients
// is the same for that form's coefficient.
//
// Not here ("Ensembles"): the fast-arithmetic tier, graph capture, slabs.
#pragma once

#include <tuple>

#include "solvers.cuh"

namespace ya {
namespace ens {

// A workgroup's replica and its block within the replica, from the flat x index (the replica count is
// not bounded by gridDim.y that way).
struct Where {
    int replica, block;
};
__device__ __forceinline__ Where where(const int blocks_per_replica)
{
    return Where{(int)(blockIdx.x / (unsigned)blocks_per_replica), (int)(blockIdx.x % (unsigned)blocks_per_replica)};
}
// A time step per replica: n_replicas floats on the device, caller-owned, read by the step's kernels when they run.
struct Replica_dt {
    const float* d_dt;
};
// What the step's launches are handed as their time step: the scalar of take_step(float) (PER_REPLICA = false, d_dt
// NULL) or the array of take_step(Replica_dt), which takes the scalar's place.  The kind is a type, so that a program
// that never steps with a Replica_dt instantiates no kernel that exists for one (whole_steps<..., true>).
template<bool PER_REPLICA>
struct Step_dt {
    static constexpr bool per_replica = PER_REPLICA;
    float dt;
    const float* d_dt;
};
inline Step_dt<false> step_dt(const float dt) { return {dt, nullptr}; }
inline Step_dt<true> step_dt(const Replica_dt per_replica)
{
    assert(per_replica.d_dt != nullptr);  // (an array that was never allocated would step with dt = 0)
    return {0.f, per_replica.d_dt};
}
// The replica's value of a parameter that is one scalar for the ensemble or, where d_per_replica is set, a float per
// replica (dt, the Gabriel coefficient).  The replica is the same for a whole workgroup: so is the value.
__device__ __forceinline__ float value_of(const float* __restrict__ d_per_replica, const float scalar, const int replica)
{
    return d_per_replica ? d_per_replica[replica] : scalar;
}
// the replica's count as the device holds it now (never beyond the replica's rows)
__device__ __forceinline__ int count_of(const int* __restrict__ d_n, const int replica, const int n_max)
{
    return min(d_n[replica], n_max);
}

// ya::tile_force for every replica at once: a workgroup serves 64 cells of ONE replica, tiles of
// TILE_POINTS partners come from that replica's rows only, j ascending, the functor is called for every
// (i, j) including i == j, ids are ensemble-global.  The loop is tile_force's own (ya::tile_force_rows).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(TILE_BLOCK) void tile_force_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const Pt* __restrict__ d_X_all, const float3* __restrict__ d_old_v_all,
    Pt* __restrict__ d_dX_all, const bool has_gen)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    if (w.block * TILE_BLOCK >= n) return;  // (the whole workgroup: blocks past n[r] return at once)
    const size_t base = (size_t)w.replica * n_max;
    tile_force_rows<Pt, pw_int, pw_friction>(
        n, w.block, (int)base, d_X_all + base, d_old_v_all + base, d_dX_all + base, has_gen);
}

// ya::tile_force_coop for every replica at once: a 256-thread workgroup owns 16 or 4 cells of ONE replica.
// tile_force_coop's own two phases (ya::tile_force_coop_rows): the lanes of a cell leave a tile's pair terms
// in LDS, one lane per component adds them in ascending j -- the sums of tile_force_batched, bit for bit.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int COOP_LANES>
__global__ __launch_bounds__(256) void tile_force_coop_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const Pt* __restrict__ d_X_all, const float3* __restrict__ d_old_v_all,
    Pt* __restrict__ d_dX_all, const bool has_gen)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    if (w.block * (256 / COOP_LANES) >= n) return;  // (the whole workgroup)
    const size_t base = (size_t)w.replica * n_max;
    tile_force_coop_rows<Pt, pw_int, pw_friction, COOP_LANES>(
        n, w.block, (int)base, d_X_all + base, d_old_v_all + base, d_dX_all + base, has_gen);
}

// Partial sums of every replica's right-hand sides in one launch, in exactly the order of
// libyalla_hip.so's k_reduce_partial (that library's ABI is not extended for this; the fold is the one both
// call, ya::fold256): replica r uses B_r = clamp(ceil(n_r / 256), 1, 1024) of its `max_blocks` workgroups, lane
// (b, t) sums the replica's rows 256 b + t, += 256 B_r, the 256 lanes are folded by halving.  The partials of
// replica r are rows [r * max_blocks, r * max_blocks + B_r) of the workspace.
constexpr int REDUCE_MAX_BLOCKS = 1024;
__host__ __device__ __forceinline__ int reduce_blocks(const int n)
{
    const int b = (n + UPDATE_BLOCK - 1) / UPDATE_BLOCK;
    return b < 1 ? 1 : (b > REDUCE_MAX_BLOCKS ? REDUCE_MAX_BLOCKS : b);
}
template<int NW>
__global__ __launch_bounds__(UPDATE_BLOCK) void reduce_partials_batched(const int n_max, const int max_blocks,
    const int* __restrict__ d_n, const float* __restrict__ v_all, float* __restrict__ partials)
{
    __shared__ float sh[NW * UPDATE_BLOCK];
    const Where w = where(max_blocks);
    const int n = count_of(d_n, w.replica, n_max);
    if (n <= 0) return;
    const int B = reduce_blocks(n);
    if (w.block >= B) return;
    const float* __restrict__ v = v_all + (size_t)w.replica * n_max * NW;
    float acc[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) acc[k] = 0.f;
    for (long i = (long)w.block * UPDATE_BLOCK + threadIdx.x; i < n; i += (long)B * UPDATE_BLOCK) {
        const float* p = v + (size_t)i * NW;
#pragma unroll
        for (int k = 0; k < NW; k++) acc[k] = acc[k] + p[k];
    }
    fold256<NW>(acc, sh);
    if (threadIdx.x < NW)
        partials[((size_t)w.replica * max_blocks + w.block) * NW + threadIdx.x] = sh[threadIdx.x * UPDATE_BLOCK];
}

// What a stage subtracts from dX.xyz (Heun_solver::heun_stages / fix_velocity): the mean of the replica's
// right-hand sides, the fixed point's right-hand side, or the point's x and y with the mean's z.
enum Fix_kind { FIX_MEAN = 0, FIX_POINT = 1, FIX_POINT_XY = 2 };

// The replica's fixed velocity of this stage: the mean folded from the replica's partial sums
// (ya::fixed_velocity_from_partials on its slice, with n_r), the point's row read directly (no make_fix
// launch).  Every thread of the workgroup calls it (the fold has barriers).
template<typename Pt>
__device__ __forceinline__ float3 resolve_fix(const int kind, const float* __restrict__ partials, const int max_blocks,
    const int replica, const int n, const Pt* __restrict__ d_rhs, const int fix_point)
{
    constexpr int NF = N_floats<Pt>::value;
    float3 fix{0.f, 0.f, 0.f};
    if (kind != FIX_POINT)
        fix = fixed_velocity_from_partials<NF>(partials + (size_t)replica * max_blocks * NF, reduce_blocks(n), n);
    if (kind != FIX_MEAN) {
        const Pt p = d_rhs[fix_point];
        fix.x = p.x;
        fix.y = p.y;
        if (kind == FIX_POINT) fix.z = p.z;
    }
    return fix;
}

// euler_step for every replica: X1 = X0 + (dX - fix) dt on the replica's n_r rows; the replica's first
// workgroup leaves the stage's velocity in d_fix_first[4 r ..] for the corrector.  d_dt (may be NULL): the replicas'
// own time steps, d_dt[r] instead of dt.  d_zero (may be NULL): the
// next stage's right-hand side, left zeroed for the generic forces -- ALL of the replica's rows, used or not.
template<typename Pt>
__global__ __launch_bounds__(UPDATE_BLOCK) void euler_step_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const float dt, const float* __restrict__ d_dt, const int kind, const int fix_point,
    const float* __restrict__ partials, const int max_blocks, float* __restrict__ d_fix_first,
    const Pt* __restrict__ d_dX_all, const Pt* __restrict__ d_X0_all, Pt* __restrict__ d_X1_all, Pt* __restrict__ d_zero_all)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    const size_t base = (size_t)w.replica * n_max;
    const int local = w.block * UPDATE_BLOCK + threadIdx.x;
    if (d_zero_all && local < n_max) d_zero_all[base + local] = ya::zero<Pt>();
    if (w.block * UPDATE_BLOCK >= n) return;  // (the whole workgroup; an empty replica is left alone)
    const Pt* __restrict__ d_dX = d_dX_all + base;
    const float3 fix = resolve_fix<Pt>(kind, partials, max_blocks, w.replica, n, d_dX, fix_point);
    if (local == 0) {
        d_fix_first[4 * (size_t)w.replica + 0] = fix.x;
        d_fix_first[4 * (size_t)w.replica + 1] = fix.y;
        d_fix_first[4 * (size_t)w.replica + 2] = fix.z;
    }
    const float dt_r = value_of(d_dt, dt, w.replica);
    if (local < n) d_X1_all[base + local] = d_X0_all[base + local] + ya::minus_fix(d_dX[local], fix) * dt_r;
}

// heun_step for every replica: X += ((dX - fix) + (dX1 - fix1)) / 2 dt and old_v, fix as the predictor left
// it, fix1 from this stage, dt or d_dt[r] as in euler_step_batched.  zero_dX: the replica's rows of d_dX, dead after this, are left zeroed -- all of
// them -- for the next step's generic forces; the fixed point's stage-1 row is therefore never read here.
template<typename Pt>
__global__ __launch_bounds__(UPDATE_BLOCK) void heun_step_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const float dt, const float* __restrict__ d_dt, const int kind, const int fix_point,
    const float* __restrict__ partials, const int max_blocks, const float* __restrict__ d_fix_first,
    Pt* __restrict__ d_dX_all, const Pt* __restrict__ d_dX1_all, Pt* __restrict__ d_X_all,
    float3* __restrict__ d_old_v_all, const bool zero_dX)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    const size_t base = (size_t)w.replica * n_max;
    const int local = w.block * UPDATE_BLOCK + threadIdx.x;
    if (w.block * UPDATE_BLOCK >= n) {  // (the whole workgroup)
        if (zero_dX && local < n_max) d_dX_all[base + local] = ya::zero<Pt>();
        return;
    }
    const float3 fix1 = resolve_fix<Pt>(kind, partials, max_blocks, w.replica, n, d_dX1_all + base, fix_point);
    const float dt_r = value_of(d_dt, dt, w.replica);
    if (local < n) {
        ya::heun_row(local, dt_r, d_fix_first + 4 * (size_t)w.replica, fix1, d_dX_all + base, d_dX1_all + base,
            d_X_all + base, d_old_v_all + base, zero_dX);
    } else if (zero_dX && local < n_max) {
        d_dX_all[base + local] = ya::zero<Pt>();
    }
}

// ---- whole steps in one launch ---------------------------------------------------------------------------
// A replica of at most whole_step_capacity<Pt>() rows fits ONE workgroup's LDS with everything a Heun step
// touches.  ya::ens::whole_steps then runs n_steps whole steps there -- no launch boundary, no global traffic in
// between -- in the order and the arithmetic of the six launches above, so that every bit agrees.  The grid form's
// launches that step from LDS (ensemble_grid.cuh) do the same with a grid's stencil walk as a stage's forces.
// The arrays are laid out for n_max rows (dynamic LDS: small replicas share a CU).
constexpr int WHOLE_STEP_MAX_ROWS = 1024;  // B_r = ceil(n_r / 256) <= 4: a lane's share of a partial sum is ONE row
constexpr size_t LDS_PER_WORKGROUP = 160 * 1024;  // gfx950: a workgroup may take the CU's whole LDS
// ya::fixed_velocity_from_partials' own (static) fold scratch, which comes on top of the dynamic arrays
constexpr size_t WHOLE_STEP_STATIC_LDS = 3 * UPDATE_BLOCK * sizeof(float);
// the term buffer's tile length (lds_layout below); the budget is not measured
constexpr int WHOLE_STEP_COOP_MIN_TILE = 16;
constexpr int WHOLE_STEP_COOP_MAX_TILE = 256;
constexpr size_t WHOLE_STEP_COOP_BUDGET = 32 * 1024;

// the grid form's bitonic sort needs a power of two of keys
constexpr int grid_lds_key_rows(const int n_max)
{
    int p = 1;
    while (p < n_max) p <<= 1;
    return p;
}
// one partner's (candidate's) terms in the term buffer: NF + 4 components for each of the 256 / lanes cells of a round
template<typename Pt>
constexpr size_t whole_step_coop_bytes_per_partner(const int lanes)
{
    return (size_t)(UPDATE_BLOCK / lanes) * (N_floats<Pt>::value + 4) * sizeof(float);
}
constexpr size_t lds_rounded_up(const size_t bytes, const size_t to) { return (bytes + to - 1) / to * to; }

// THE LDS LAYOUT of a launch that steps a replica from LDS, all-pairs (whole_steps*, KEYS = false) or grid
// (grid_lds_steps*, KEYS = true): byte offsets from the start of the dynamic LDS, the term buffer's tile length and
// the launch's dynamic LDS.  Host plans and kernels both read it; the kernels compute it once, at their start.
struct Lds_layout {
    size_t X, X1, dX, dX1;  // the step's arrays: n_max rows of sizeof(Pt) each,
    size_t old_v;           // n_max rows of 12 bytes,
    size_t fold;            // fold256's scratch, NF * 256 floats (whole_links_build's scan and the grid kernels' status
                            // flag borrow it while no fold runs),
    size_t partials;        // the <= 4 partial sums, NF floats each
    size_t keys;            // KEYS: one 64-bit (cube, id) key per row of grid_lds_key_rows(n_max)
    size_t list;            // LINKED: the incidence list, n_max + 1 offsets and at most 2 `slots` entries of 4 bytes
    size_t terms;           // lanes > 1: the term buffer, `tile` partners' terms
    int tile;               // the term buffer's tile length in partners (candidates); 0 with one lane or without room
    size_t bytes;           // the launch's dynamic LDS; 0 = no room (for lanes > 1: run with one lane per cell)
};
// THE RULE, region after region in their order.  LINKED (a compile-time fact, not a slot count: a linked launch of
// no slots still lays out the list's n_max + 1 offsets) and `slots` = the links' slots per replica; lanes = lanes per
// cell (1, 4, 16 or 64).
//   the step's arrays   X, X1, dX, dX1, old_v, the fold's scratch, the partial sums: no padding in between.
//   the keys            8-byte aligned; after the sort, slot s holds the cube of the cell in sorted slot s and the
//                       slot -> id map at once, 8 bytes per row and no sorted copy of the entries.
//   the list            THE TWO FORMS DIFFER HERE, and stay as they are: the all-pairs list starts 16-byte aligned and
//                       its end is rounded up to 16, so that a linked all-pairs launch's bytes are a multiple of 16 even
//                       with one lane; the grid list starts right behind the keys (whose end is 8-byte aligned; the
//                       list needs 4) and its end is not rounded.  No room where that end and WHOLE_STEP_STATIC_LDS
//                       exceed the workgroup's LDS (an 8-float point's 1024 rows and keys leave 896 bytes: no list of
//                       1025 offsets, whatever `slots` is).
//   the term buffer     16-byte aligned behind all that: one tile's pair terms for the 256 / lanes cells of a round.
//                       The tile length, in partners: n_max rounded up to a multiple of 4 (phase (b) reads 16 bytes at
//                       a time; no replica has more partners), at most WHOLE_STEP_COOP_MAX_TILE, at most what
//                       WHOLE_STEP_COOP_BUDGET bytes hold (small replicas keep sharing a CU: with 4 lanes a partner
//                       costs 64 cells' terms) but no less than WHOLE_STEP_COOP_MIN_TILE for that reason, and at most
//                       what is left of the workgroup's LDS beside WHOLE_STEP_STATIC_LDS.  No room where
//                       WHOLE_STEP_COOP_MIN_TILE partners do not fit (an 8-float point's 1024 rows and keys leave 896
//                       bytes; a 7-float point's leave 18320: room for 16 and 64 lanes, none for 4).  No bit depends on
//                       the tile length: a cell's terms are added in ascending order into one running sum, tile
//                       after tile.
// The rule may fill the LDS to the byte, and so may the capacities (a 9-float point's 918 rows and keys leave 8 bytes):
// every kernel that steps from LDS keeps its static LDS at WHOLE_STEP_STATIC_LDS.  Whether the step's arrays (and keys) fit at all is whole_step_capacity's question
// (grid_lds_capacity's), not this function's: without a list and with one lane `bytes` is never 0.
template<typename Pt, bool KEYS, bool LINKED>
constexpr Lds_layout lds_layout(const int n_max, const int slots, const int lanes)
{
    constexpr size_t NF = N_floats<Pt>::value;
    const size_t n = (size_t)n_max;
    Lds_layout l{};
    l.X1 = n * sizeof(Pt);
    l.dX = 2 * n * sizeof(Pt);
    l.dX1 = 3 * n * sizeof(Pt);
    l.old_v = 4 * n * sizeof(Pt);
    l.fold = n * (4 * sizeof(Pt) + sizeof(float3));
    l.partials = l.fold + NF * UPDATE_BLOCK * sizeof(float);
    size_t end = l.partials + NF * (WHOLE_STEP_MAX_ROWS / UPDATE_BLOCK) * sizeof(float);
    if (KEYS) {
        l.keys = lds_rounded_up(end, 8);
        end = l.keys + (size_t)grid_lds_key_rows(n_max) * sizeof(unsigned long long);
    }
    if (LINKED) {
        l.list = KEYS ? end : lds_rounded_up(end, 16);
        end = l.list + 4 * (n + 1) + 8 * (size_t)slots;
    }
    l.terms = lds_rounded_up(end, 16);
    if (LINKED && !KEYS) end = l.terms;  // (the all-pairs list's end is rounded)
    if (LINKED && end + WHOLE_STEP_STATIC_LDS > LDS_PER_WORKGROUP) return l;  // no room for the list
    if (lanes <= 1) {
        l.bytes = end;
        return l;
    }
    const size_t per_partner = whole_step_coop_bytes_per_partner<Pt>(lanes);
    if (l.terms + WHOLE_STEP_STATIC_LDS + WHOLE_STEP_COOP_MIN_TILE * per_partner > LDS_PER_WORKGROUP) return l;
    const size_t room = (LDS_PER_WORKGROUP - WHOLE_STEP_STATIC_LDS - l.terms) / per_partner / 4 * 4;
    const size_t budget = WHOLE_STEP_COOP_BUDGET / per_partner / 4 * 4;
    size_t tile = (n + 3) / 4 * 4;
    if (tile > (size_t)WHOLE_STEP_COOP_MAX_TILE) tile = WHOLE_STEP_COOP_MAX_TILE;
    if (tile > budget) tile = budget < (size_t)WHOLE_STEP_COOP_MIN_TILE ? WHOLE_STEP_COOP_MIN_TILE : budget;
    if (tile > room) tile = room;
    l.tile = (int)tile;
    l.bytes = l.terms + tile * per_partner;
    return l;
}
// Lds_layout::fold for those who borrow it while no fold runs (whole_links_build's scan, the grid kernels' status flag)
template<typename Pt>
__device__ __forceinline__ int* lds_fold_scratch(unsigned char* lds, const int n_max)
{
    return reinterpret_cast<int*>(reinterpret_cast<float3*>(reinterpret_cast<Pt*>(lds) + 4 * n_max) + n_max);
}

// The largest n_max whose step arrays fit one workgroup, the static fold scratch included; at most
// WHOLE_STEP_MAX_ROWS (1024 for every point type up to 8 floats).
template<typename Pt>
constexpr int whole_step_capacity()
{
    constexpr size_t fixed = lds_layout<Pt, false, false>(0, 0, 1).bytes + WHOLE_STEP_STATIC_LDS;
    static_assert(fixed < LDS_PER_WORKGROUP, "a point type whose fold scratch alone overflows the LDS");
    constexpr size_t rows = (LDS_PER_WORKGROUP - fixed) / (lds_layout<Pt, false, false>(1, 0, 1).bytes + WHOLE_STEP_STATIC_LDS - fixed);
    return rows < (size_t)WHOLE_STEP_MAX_ROWS ? (int)rows : WHOLE_STEP_MAX_ROWS;
}

}  // namespace ens
}  // namespace ya

// ordered link forces: Replica_links, link_forces_ordered, the LDS rule and the pieces of whole_steps_linked
#define YA_ENSEMBLE_LINKS_FROM_ENSEMBLE_CUH
#include "ensemble_links.cuh"
#undef YA_ENSEMBLE_LINKS_FROM_ENSEMBLE_CUH

namespace ya {
namespace ens {

// tile_force_batched for the replica in LDS: one thread per cell (thread t owns rows t, t + 256, ...: the contract
// of functors that keep per-cell state), partners straight from the LDS copy, j ascending over 0 .. n - 1 with
// i == j included, ensemble-global ids, the pair and the right-hand side by tile_force_rows' own functions.
// HAS_GEN: the right-hand sides hold a start the forces are added to (the ordered link forces, ensemble_links.cuh).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool HAS_GEN = false>
__device__ __forceinline__ void whole_stage_force(const int n, const int id_base, const Pt* sh_in, const float3* sh_v,
    Pt* sh_rhs)
{
    for (int local = threadIdx.x; local < n; local += UPDATE_BLOCK) {
        const int i = id_base + local;
        const Pt Xi = sh_in[local];
        Pt F = ya::zero<Pt>();
        float3 sum_v{0.f, 0.f, 0.f};
        float sum_friction = 0;
#pragma unroll YA_TILE_UNROLL
        for (int k = 0; k < n; k++)
            tile_pair<Pt, pw_int, pw_friction>(Xi, sh_in[k], sh_v[k], i, id_base + k, F, sum_v, sum_friction);
        store_rhs(sh_rhs, local, HAS_GEN, F, sum_v, sum_friction);
    }
}

// tile_force_coop_batched for the replica in LDS, for functors that keep no per-cell state: COOP_LANES lanes per
// cell.  The workgroup serves 256 / COOP_LANES cells per round, ceil(n / cells) rounds; per round and per tile of
// `tile` partners tile_force_coop_rows' two phases, by its own functions: (a) lane l of a cell evaluates partners l,
// l + COOP_LANES, ... of the tile straight from the stage's LDS arrays and leaves their terms in sh_part,
// [cell][component][j]; (b) one lane per component (components lane, lane + COOP_LANES, ...) adds the tile's terms
// in ascending j to a sum that started from +0 and is carried across tiles: whole_stage_force's sums, bit for bit,
// whatever `tile` is.  The sums then meet in column 0 of the cell's rows and the cell's first lane writes the
// right-hand side.  n is the workgroup's, so every thread makes every trip and reaches every barrier, those of
// cells >= n included.  Every thread calls it; the caller's barrier follows.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int COOP_LANES,
    bool HAS_GEN = false>
__device__ __forceinline__ void whole_stage_force_coop(const int n, const int id_base, const Pt* sh_in,
    const float3* sh_v, Pt* sh_rhs, float* sh_part, const int tile)
{
    static_assert(COOP_LANES == 4 || COOP_LANES == 16 || COOP_LANES == 64, "4, 16 or 64 lanes per cell");
    constexpr int COOP_CELLS = UPDATE_BLOCK / COOP_LANES;
    constexpr int NF = N_floats<Pt>::value;
    constexpr int NC = NF + 4;  // components summed per cell: F (NF), friction, friction * old_v (3)
    constexpr int SLOTS = (NC + COOP_LANES - 1) / COOP_LANES;
    const int cell = threadIdx.x / COOP_LANES, lane = threadIdx.x % COOP_LANES;
    float* const my_terms = sh_part + (size_t)cell * NC * tile;  // this cell's [component][j] rows
    for (int first = 0; first < n; first += COOP_CELLS) {
        const int local = first + cell;
        const bool active = local < n;
        const int i = id_base + local;
        Pt Xi = ya::zero<Pt>();
        if (active) Xi = sh_in[local];
        float acc[SLOTS];
#pragma unroll
        for (int a = 0; a < SLOTS; a++) acc[a] = 0.f;
        for (int tile_start = 0; tile_start < n; tile_start += tile) {
            const int n_tile = min(tile, n - tile_start);
            __syncthreads();  // (the term buffer's readers of the tile or the round before are done)
            if (active) {
#pragma unroll 4
                for (int jj = lane; jj < n_tile; jj += COOP_LANES) {
                    const int k = tile_start + jj;
                    coop_pair_terms<Pt, pw_int, pw_friction>(Xi, sh_in, sh_v, k, i, id_base + k,
                        [&](const int c, const float term) { my_terms[(size_t)c * tile + jj] = term; });
                }
            }
            __syncthreads();
#pragma unroll
            for (int a = 0; a < SLOTS; a++) {
                const int c = lane + COOP_LANES * a;
                if (c < NC && active) acc[a] = coop_ordered_sum(acc[a], my_terms + (size_t)c * tile, n_tile);
            }
        }
        // row c of a cell was read by the lane that now writes its column 0, and by no other
#pragma unroll
        for (int a = 0; a < SLOTS; a++) {
            const int c = lane + COOP_LANES * a;
            if (c < NC && active) my_terms[(size_t)c * tile] = acc[a];
        }
        __syncthreads();
        if (active && lane == 0) {
            Pt F;
#pragma unroll
            for (int c = 0; c < NF; c++) field(F, c) = my_terms[(size_t)c * tile];
            store_rhs(sh_rhs, local, HAS_GEN, F,
                float3{my_terms[(size_t)(NF + 1) * tile], my_terms[(size_t)(NF + 2) * tile], my_terms[(size_t)(NF + 3) * tile]},
                my_terms[(size_t)NF * tile]);
        }
    }
}

// The stage's fixed velocity, as reduce_partials_batched and resolve_fix give it: block b's lane t starts from 0,
// adds row 256 b + t (B_r = reduce_blocks(n) <= 4 blocks cover the replica once), fold256, the B_r partials folded
// by ya::fixed_velocity_from_partials; the fixed point's raw right-hand side.  Every thread calls it (barriers).
template<typename Pt>
__device__ __forceinline__ float3 whole_stage_fix(const int kind, const int n, const Pt* sh_rhs, const int fix_point,
    float* sh_fold, float* sh_partials)
{
    constexpr int NF = N_floats<Pt>::value;
    float3 fix{0.f, 0.f, 0.f};
    if (kind != FIX_POINT) {
        const int B = reduce_blocks(n);
        for (int b = 0; b < B; b++) {
            float acc[NF];
#pragma unroll
            for (int k = 0; k < NF; k++) acc[k] = 0.f;
            const int row = b * UPDATE_BLOCK + threadIdx.x;
            if (row < n) {
                const float* p = reinterpret_cast<const float*>(sh_rhs) + (size_t)row * NF;
#pragma unroll
                for (int k = 0; k < NF; k++) acc[k] = acc[k] + p[k];
            }
            fold256<NF>(acc, sh_fold);
            if (threadIdx.x < NF) sh_partials[b * NF + threadIdx.x] = sh_fold[threadIdx.x * UPDATE_BLOCK];
            __syncthreads();  // (the next fold writes sh_fold)
        }
        fix = fixed_velocity_from_partials<NF>(sh_partials, B, n);
    }
    if (kind != FIX_MEAN) {
        const Pt p = sh_rhs[fix_point];
        fix.x = p.x;
        fix.y = p.y;
        if (kind == FIX_POINT) fix.z = p.z;
    }
    return fix;
}

// A stage's forces by LANES: 1 = whole_stage_force, 4, 16 or 64 = whole_stage_force_coop with tiles of `tile` partners.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES, bool HAS_GEN = false>
__device__ __forceinline__ void whole_stage_forces(const int n, const int id_base, const Pt* sh_in, const float3* sh_v,
    Pt* sh_rhs, float* sh_part, const int tile)
{
    if constexpr (LANES == 1)
        whole_stage_force<Pt, pw_int, pw_friction, HAS_GEN>(n, id_base, sh_in, sh_v, sh_rhs);
    else
        whole_stage_force_coop<Pt, pw_int, pw_friction, LANES, HAS_GEN>(n, id_base, sh_in, sh_v, sh_rhs, sh_part, tile);
}

// THE STEP IN LDS, written once: n_steps Heun steps of a replica of n > 0 rows by ONE 256-thread workgroup whose
// dynamic LDS starts with the step's arrays of lds_layout.  Rows [0, n) of the replica's d_X and d_old_v
// are read at the start and written at the end; in between, per stage: stage_forces(sh_in, sh_v, sh_rhs) -- every
// thread calls it; it leaves the right-hand sides of the positions sh_in (X, then X1) in sh_rhs and may have barriers
// of its own, the barrier after it is here -- then the mean or fixed point (whole_stage_fix), the predictor or
// ya::heun_row.  What a stage's forces are is the caller's: the all-pairs loops (whole_steps_of_a_replica below) or a
// grid's stencil walk (ya::ens::grid_lds_steps, ensemble_grid.cuh).  kind1 / kind2: the Fix_kind of stage 1 and 2.
template<typename Pt, typename Stage_forces>
__device__ __forceinline__ void whole_steps_in_lds(const int n_max, const int n, const int replica, const float dt,
    const int n_steps, const int kind1, const int kind2, const int fix_point, Pt* __restrict__ d_X_all,
    float3* __restrict__ d_old_v_all, unsigned char* lds, const Stage_forces& stage_forces)
{
    // Lds_layout's X .. partials as typed pointer steps, one running sum of n_max rows each.  (Byte offsets taken from a
    // layout computed in the kernel give the same addresses through other instructions, in every kernel's prologue;
    // the kernels keep the code they had.)
    constexpr int NF = N_floats<Pt>::value;
    Pt* sh_X = reinterpret_cast<Pt*>(lds);
    Pt* sh_X1 = sh_X + n_max;
    Pt* sh_dX = sh_X1 + n_max;
    Pt* sh_dX1 = sh_dX + n_max;
    float3* sh_v = reinterpret_cast<float3*>(sh_dX1 + n_max);
    float* sh_fold = reinterpret_cast<float*>(sh_v + n_max);
    float* sh_partials = sh_fold + NF * UPDATE_BLOCK;

    const size_t base = (size_t)replica * n_max;
    Pt* __restrict__ d_X = d_X_all + base;
    float3* __restrict__ d_old_v = d_old_v_all + base;
    for (int local = threadIdx.x; local < n; local += UPDATE_BLOCK) {
        sh_X[local] = d_X[local];
        sh_v[local] = d_old_v[local];
    }
    __syncthreads();

    for (int step = 0; step < n_steps; step++) {
        // predictor: X1 = X + (dX - fix) dt (euler_step_batched)
        stage_forces(sh_X, sh_v, sh_dX);
        __syncthreads();
        const float3 fix = whole_stage_fix<Pt>(kind1, n, sh_dX, fix_point, sh_fold, sh_partials);
        for (int local = threadIdx.x; local < n; local += UPDATE_BLOCK)
            sh_X1[local] = sh_X[local] + ya::minus_fix(sh_dX[local], fix) * dt;
        __syncthreads();
        // corrector (heun_step_batched): old_v is written only after this barrier, when stage 2's forces have read it
        stage_forces(sh_X1, sh_v, sh_dX1);
        __syncthreads();
        const float3 fix1 = whole_stage_fix<Pt>(kind2, n, sh_dX1, fix_point, sh_fold, sh_partials);
        const float fix_first[3] = {fix.x, fix.y, fix.z};  // stage 1's, as the predictor leaves it in d_fix_first
        for (int local = threadIdx.x; local < n; local += UPDATE_BLOCK)
            ya::heun_row(local, dt, fix_first, fix1, sh_dX, sh_dX1, sh_X, sh_v, false);
        __syncthreads();
    }

    for (int local = threadIdx.x; local < n; local += UPDATE_BLOCK) {
        d_X[local] = sh_X[local];
        d_old_v[local] = sh_v[local];
    }
}

// n_steps Heun steps of replica blockIdx.x by ONE 256-thread workgroup, from LDS.  Nothing crosses workgroups.
// Global memory: d_n[r] is read once, rows [0, n_r) of d_X and d_old_v are read at the start and written at the
// end; nothing else is written (unused rows, other replicas, d_n and the ensemble's right-hand-side arrays are
// left as they are).  kind1 / kind2: the Fix_kind of stage 1 and of stage 2.  dt: the replica's, which the kernels
// below resolve from their scalar and their array.
// The body of the kernels below: whole_steps_in_lds with the all-pairs forces of a stage.  LANES = 1: they are
// whole_stage_force; 4, 16 or 64: whole_stage_force_coop with tiles of `tile` partners.
// LINKED (whole_steps_linked below): once per launch the workgroup builds the replica's incidence list behind the
// step's arrays (whole_links_build); every stage starts with the ordered link forces of its positions as the
// right-hand sides (whole_stage_links), to which the stage's forces are added.  Links do not change during a launch.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES, bool LINKED = false>
__device__ __forceinline__ void whole_steps_of_a_replica(const int n_max, const int* __restrict__ d_n, const float dt,
    const int n_steps, const int kind1, const int kind2, const int fix_point, Pt* __restrict__ d_X_all,
    float3* __restrict__ d_old_v_all, const int tile, const Links_view links = Links_view{})
{
    extern __shared__ __attribute__((aligned(16))) unsigned char whole_step_lds[];
    const int replica = blockIdx.x;
    const int n = count_of(d_n, replica, n_max);
    if (n <= 0) return;  // (the whole workgroup; an empty replica is left alone)
    const Lds_layout layout = lds_layout<Pt, false, LINKED>(n_max, links.slots_per_replica, LANES);
    float* const sh_part = reinterpret_cast<float*>(whole_step_lds + layout.terms);  // (used with several lanes per cell)
    int* const sh_off = reinterpret_cast<int*>(whole_step_lds + layout.list);  // LINKED: n_max + 1 offsets,
    unsigned* const sh_ent = reinterpret_cast<unsigned*>(sh_off + n_max + 1);  // at most 2 slots_per_replica entries
    if constexpr (LINKED)  // (its scratch is the fold's)
        whole_links_build(links, replica, n, n_max, sh_off, sh_ent, lds_fold_scratch<Pt>(whole_step_lds, n_max));

    const size_t base = (size_t)replica * n_max;
    whole_steps_in_lds<Pt>(n_max, n, replica, dt, n_steps, kind1, kind2, fix_point, d_X_all, d_old_v_all, whole_step_lds,
        [&](const Pt* sh_in, const float3* sh_v, Pt* sh_rhs) __attribute__((always_inline)) {
            if constexpr (LINKED) {
                whole_stage_links<Pt>(n, sh_in, sh_rhs, sh_off, sh_ent, links.strength);
                if constexpr (LANES > 1) __syncthreads();  // (another thread adds the cell's forces to it)
            }
            whole_stage_forces<Pt, pw_int, pw_friction, LANES, LINKED>(n, (int)base, sh_in, sh_v, sh_rhs, sh_part, tile);
        });
}
// The time step of replica blockIdx.x in the two unlinked kernels below.  REPLICA_DT is a template parameter there
// because it was measured (profiles/ensemble_replica_dt_bench.json, "before_the_template_parameter"): with a nullable
// pointer tested at run time whole_steps_coop's scalar calls ran 0.44 % slower than the parent commit's at M = 256,
// n = 64 (945.1 against 949.3 M cell updates / s, spreads 0.03 % and 0.15 %; the loop's instructions were the same,
// their registers and addresses were not); with the parameter the two agree.  The scalar instance reads no array, and
// only a program that steps with a Replica_dt instantiates the other (ya::ens::Step_dt).
template<bool REPLICA_DT>
__device__ __forceinline__ float whole_step_dt(const float* __restrict__ d_dt, const float dt)
{
    if constexpr (REPLICA_DT)
        return d_dt[blockIdx.x];
    else
        return dt;
}
// One thread per cell: dynamic LDS of lds_layout<Pt, false, false>(n_max, 0, 1).bytes.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool REPLICA_DT = false>
__global__ __launch_bounds__(UPDATE_BLOCK) void whole_steps(const int n_max, const int* __restrict__ d_n, const float dt,
    const float* __restrict__ d_dt, const int n_steps, const int kind1, const int kind2, const int fix_point,
    Pt* __restrict__ d_X_all, float3* __restrict__ d_old_v_all)
{
    whole_steps_of_a_replica<Pt, pw_int, pw_friction, 1>(
        n_max, d_n, whole_step_dt<REPLICA_DT>(d_dt, dt), n_steps, kind1, kind2, fix_point, d_X_all, d_old_v_all, 0);
}
// COOP_LANES (4, 16 or 64) lanes per cell, for functors that keep no per-cell state: dynamic LDS and tile of
// lds_layout<Pt, false, false>(n_max, 0, COOP_LANES), which has room (.bytes > 0).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int COOP_LANES,
    bool REPLICA_DT = false>
__global__ __launch_bounds__(UPDATE_BLOCK) void whole_steps_coop(const int n_max, const int* __restrict__ d_n,
    const float dt, const float* __restrict__ d_dt, const int n_steps, const int kind1, const int kind2,
    const int fix_point, Pt* __restrict__ d_X_all, float3* __restrict__ d_old_v_all, const int tile)
{
    whole_steps_of_a_replica<Pt, pw_int, pw_friction, COOP_LANES>(
        n_max, d_n, whole_step_dt<REPLICA_DT>(d_dt, dt), n_steps, kind1, kind2, fix_point, d_X_all, d_old_v_all, tile);
}
// The same steps with the ordered link forces of `links` (ensemble_links.cuh) at the start of every stage; LANES = 1,
// 4, 16 or 64: dynamic LDS and tile of lds_layout<Pt, false, true>(n_max, links.slots_per_replica, LANES), which has
// room.  d_dt (may be NULL): d_dt[r] instead of dt, decided at run time (not measured against the parent; the linked
// kernels keep their instance count).  Besides what whole_steps reads, the replica's
// slots of links.d_link and *links.d_n are read, at the start of the launch.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES>
__global__ __launch_bounds__(UPDATE_BLOCK) void whole_steps_linked(const int n_max, const int* __restrict__ d_n,
    const float dt, const float* __restrict__ d_dt, const int n_steps, const int kind1, const int kind2,
    const int fix_point, Pt* __restrict__ d_X_all, float3* __restrict__ d_old_v_all, const int tile,
    const Links_view links)
{
    whole_steps_of_a_replica<Pt, pw_int, pw_friction, LANES, true>(
        n_max, d_n, value_of(d_dt, dt, blockIdx.x), n_steps, kind1, kind2, fix_point, d_X_all, d_old_v_all, tile, links);
}

// Whether whole-step launches beat the six-launch step when the model leaves the choice to the engine
// (Ensemble::whole_steps == 0).  THIS RULE IS A PLACEHOLDER until measured (profiles/ensemble_whole_step_bench.json):
// one workgroup per CU; below that the six-launch path spreads a replica over more CUs.
inline bool whole_steps_pay(const int n_replicas, const int n_max)
{
    return n_replicas >= 256;
}

// Lanes per cell of the force launch when the model leaves the choice to the engine and its functors are
// stateless.  The coop kernels exist because ONE small system cannot fill the chip with one lane per
// cell; an ensemble can, and the one-lane kernel does less work per pair.  So the rule looks at the whole
// launch: `waves` = the wavefronts a one-lane launch would have, n_replicas * ceil(n_max / 64).
// THE THRESHOLDS BELOW ARE PLACEHOLDERS until measured (profiles/ensemble_bench.json).
inline int lanes_for(const int n_replicas, const int n_max)
{
    const size_t waves = (size_t)n_replicas * (size_t)((n_max + TILE_BLOCK - 1) / TILE_BLOCK);
    if (waves >= 2048) return 1;
    if (waves >= 256) return 16;
    return n_max <= 4096 ? 64 : 16;
}

// Lanes per cell of a whole-step launch when the model leaves the choice to the engine and its functors are
// stateless (Ensemble::whole_step_lanes == 0): the largest L of 64, 16, 4 with n_max * L <= 256, else 1.  Then one
// round serves the whole replica, every lane evaluates ceil(n / L) pairs instead of n, and the ordered adds are what
// they were: the work per lane only falls.  ABOVE 64 CELLS THE ANSWER (1) IS A PLACEHOLDER until measured
// (profiles/ensemble_whole_lanes_bench.json): whether several lanes also pay with several rounds is not known.
constexpr int whole_step_lanes_for(const int n_max)
{
    if (n_max <= UPDATE_BLOCK / 64) return 64;
    if (n_max <= UPDATE_BLOCK / 16) return 16;
    if (n_max <= UPDATE_BLOCK / 4) return 4;
    return 1;
}

}  // namespace ens
}  // namespace ya


namespace ya {
namespace ens {

// What every form of Ensemble is: the flat replica-major arrays, the counts, the fixed modes and THE STEP.
// Form (CRTP) supplies the forces of a stage,
//     template<pw_int, pw_friction> void forces(const Pt* d_in, Pt* d_rhs, bool has_gen)
// which leaves every replica's right-hand sides of the cells d_in[r * n_max + 0 .. n_r) in d_rhs, added to what
// the generic forces left there if has_gen.
template<typename Pt, typename Form>
class Stepper {
protected:
    static constexpr int n_floats = ya::N_floats<Pt>::value;

public:
    Pt* h_X;          // host mirror, n_replicas * n_max rows, replica-major (page-locked if the runtime grants it)
    Pt* d_X;          // the same on the device
    float3* d_old_v;  // velocities of the previous step, the same rows
    int* const h_n;   // [n_replicas] cells of each replica
    int* d_n;         // the same on the device: what the step reads
    const int n_replicas;
    const int n_max;  // capacity of EACH replica

    Stepper(int n_replicas, int n_max) : h_n{(int*)malloc(sizeof(int) * (n_replicas > 0 ? n_replicas : 1))},
        n_replicas{n_replicas}, n_max{n_max}
    {
        assert(n_replicas > 0 && n_max > 0);
        // ids are ints (the functors' signature, gen_forces' n), and so is a launch's x dimension
        const size_t total = rows();
        assert(total <= (size_t)0x7fffffff);
        for (int r = 0; r < n_replicas; r++) h_n[r] = n_max;
        const size_t pts = total * sizeof(Pt);
        h_X_locked = ya_host_alloc((void**)&h_X, pts) == 0;
        if (h_X_locked)
            memset((void*)h_X, 0, pts);
        else
            h_X = (Pt*)calloc(total, sizeof(Pt));
        YA_CHECK(ya_malloc((void**)&d_X, pts));
        YA_CHECK(ya_malloc((void**)&d_dX, pts));
        YA_CHECK(ya_malloc((void**)&d_X1, pts));
        YA_CHECK(ya_malloc((void**)&d_dX1, pts));
        YA_CHECK(ya_malloc((void**)&d_old_v, total * sizeof(float3)));
        YA_CHECK(ya_memset_async(d_old_v, 0, total * sizeof(float3), nullptr));
        YA_CHECK(ya_malloc((void**)&d_n, (size_t)n_replicas * sizeof(int)));
        YA_CHECK(ya_memset_async(d_n, 0, (size_t)n_replicas * sizeof(int), nullptr));
        YA_CHECK(ya_malloc((void**)&d_fix_first, (size_t)n_replicas * 4 * sizeof(float)));
        YA_CHECK(ya_malloc((void**)&d_partials, (size_t)n_replicas * max_blocks() * n_floats * sizeof(float)));
    }
    ~Stepper()
    {
        if (h_X_locked)
            (void)ya_host_free(h_X);
        else
            free(h_X);
        free(h_n);
        ya_free(d_X);
        ya_free(d_dX);
        ya_free(d_X1);
        ya_free(d_dX1);
        ya_free(d_old_v);
        ya_free(d_n);
        ya_free(d_fix_first);
        ya_free(d_partials);
    }
    Stepper(const Stepper&) = delete;

    size_t rows() const { return (size_t)n_replicas * (size_t)n_max; }
    // row i of replica r in the host mirror (the same index serves d_X, d_old_v and a model's own arrays)
    size_t index(int r, int i) const { return (size_t)r * (size_t)n_max + (size_t)i; }
    Pt* row(int r, int i) { return h_X + index(r, i); }

    void copy_to_device()
    {
        for (int r = 0; r < n_replicas; r++) assert(h_n[r] >= 0 && h_n[r] <= n_max);
        YA_CHECK(ya_memcpy_h2d(d_X, h_X, rows() * sizeof(Pt)));
        YA_CHECK(ya_memcpy_h2d(d_n, h_n, (size_t)n_replicas * sizeof(int)));
    }
    void copy_to_host()
    {
        YA_CHECK(ya_memcpy_d2h(h_X, d_X, rows() * sizeof(Pt)));
        YA_CHECK(ya_memcpy_d2h(h_n, d_n, (size_t)n_replicas * sizeof(int)));
        for (int r = 0; r < n_replicas; r++) assert(h_n[r] <= n_max);
    }
    // Blocking read of replica r's device-side count, for the host's own use: the step never calls it.
    int get_d_n(int r)
    {
        assert(r >= 0 && r < n_replicas);
        int n;
        YA_CHECK(ya_get_n(d_n + r, &n));
        assert(n <= n_max);
        return n;
    }

    // Heun_solver's three modes, applied to EVERY replica with a LOCAL point id.  Precondition:
    // point_id < n[r] for every replica that is not empty (a replica whose point does not exist would hold
    // an unused row's right-hand side).  Semantics are Heun_solver's, quirks included: set_fixed_xy holds
    // x and y in the first stage only -- the second stage holds the whole point -- and stays in force
    // for later set_fixed calls (include/solvers.cuh, heun_stages / fix_velocity).
    void set_fixed() { fix_com = true; }
    void set_fixed(int point_id)
    {
        assert(point_id >= 0 && point_id < n_max);
        fix_com = false;
        fix_point = point_id;
    }
    void set_fixed_xy(int point_id)
    {
        assert(point_id >= 0 && point_id < n_max);
        fix_com = false;
        fix_com_z = true;
        fix_point = point_id;
    }

    template<Pairwise_interaction<Pt> pw_int>
    void take_step(float dt, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        take_step<pw_int, friction_w_neighbour<Pt>>(dt, gen_forces);
    }
    // One Heun step of every replica.  Per stage: the form's forces, partial sums, update; stream-ordered on the
    // null stream; no copy to the host, no synchronisation, no allocation.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_step(float dt, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        one_step<pw_int, pw_friction>(step_dt(dt), gen_forces);
    }
    // The same step with replica r's own time step d_dt[r], which the update kernels read on the device.
    template<Pairwise_interaction<Pt> pw_int>
    void take_step(Replica_dt dt, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        take_step<pw_int, friction_w_neighbour<Pt>>(dt, gen_forces);
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_step(Replica_dt dt, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        one_step<pw_int, pw_friction>(step_dt(dt), gen_forces);
    }

protected:
    // take_step with either kind of time step
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool PER_REPLICA>
    void one_step(const Step_dt<PER_REPLICA> dt, Generic_forces<Pt> gen_forces)
    {
        const bool has_gen = !ya::is_no_gen_forces<Pt>(gen_forces);
        const int update_blocks = (n_max + ya::UPDATE_BLOCK - 1) / ya::UPDATE_BLOCK;
        for (int stage = 1; stage <= 2; stage++) {
            const Pt* d_in = stage == 1 ? d_X : d_X1;
            Pt* d_rhs = stage == 1 ? d_dX : d_dX1;
            if (has_gen) {
                // (the update kernel before this stage may have left the rows zeroed already)
                if (!rhs_zeroed[stage - 1]) YA_CHECK(ya_memset_async(d_rhs, 0, rows() * sizeof(Pt), nullptr));
                gen_forces((int)rows(), d_in, d_rhs);
            }
            rhs_zeroed[stage - 1] = false;  // the force kernel writes it next
            static_cast<Form*>(this)->template forces<pw_int, pw_friction>(d_in, d_rhs, has_gen);
            // Heun_solver::heun_stages: set_fixed_xy(i) holds x and y in the first stage only
            const bool xy = stage == 1 && fix_com_z;
            const int kind = (fix_com && !fix_com_z) ? ya::ens::FIX_MEAN
                             : xy                    ? ya::ens::FIX_POINT_XY
                             : fix_com               ? ya::ens::FIX_MEAN
                                                     : ya::ens::FIX_POINT;
            if (kind != ya::ens::FIX_POINT)
                ya::ens::reduce_partials_batched<n_floats><<<grid_of(max_blocks()), ya::UPDATE_BLOCK>>>(
                    n_max, max_blocks(), d_n, reinterpret_cast<const float*>(d_rhs), d_partials);
            if (stage == 1) {
                ya::ens::euler_step_batched<Pt><<<grid_of(update_blocks), ya::UPDATE_BLOCK>>>(n_max, update_blocks, d_n,
                    dt.dt, dt.d_dt, kind, fix_point, d_partials, max_blocks(), d_fix_first, d_dX, d_X, d_X1,
                    has_gen ? d_dX1 : nullptr);
                rhs_zeroed[1] = has_gen;
            } else {
                ya::ens::heun_step_batched<Pt><<<grid_of(update_blocks), ya::UPDATE_BLOCK>>>(n_max, update_blocks, d_n,
                    dt.dt, dt.d_dt, kind, fix_point, d_partials, max_blocks(), d_fix_first, d_dX, d_dX1, d_X, d_old_v,
                    has_gen);
                rhs_zeroed[0] = has_gen;
            }
        }
    }

    Pt *d_dX, *d_X1, *d_dX1;
    float* d_fix_first;  // [n_replicas][4] stage 1's fixed velocity, left by the predictor for the corrector
    float* d_partials;   // [n_replicas][max_blocks()][n_floats] partial sums of a stage's right-hand sides
    bool h_X_locked = false;
    bool fix_com = true;
    bool fix_com_z = false;
    int fix_point = 0;
    // every row of d_dX / d_dX1 was left zeroed by an update kernel (take_step is their only writer)
    bool rhs_zeroed[2] = {false, false};

    // take_step's expression for what a stage holds fixed (1 = predictor, 2 = corrector)
    int fix_kind_of(const int stage) const
    {
        const bool xy = stage == 1 && fix_com_z;
        return (fix_com && !fix_com_z) ? ya::ens::FIX_MEAN
               : xy                    ? ya::ens::FIX_POINT_XY
               : fix_com               ? ya::ens::FIX_MEAN
                                       : ya::ens::FIX_POINT;
    }
    int max_blocks() const { return ya::ens::reduce_blocks(n_max); }
    dim3 grid_of(int blocks_per_replica) const { return dim3((unsigned)((size_t)n_replicas * blocks_per_replica)); }

    // ---- take_steps: from LDS or as the loop of take_step, decided and launched once for every form ---------------
    // A form whose replicas can be stepped from one workgroup's LDS (the all-pairs form's whole steps, the grid
    // form's lds steps) supplies
    //     static constexpr bool lds_keys                      its lds_layout has keys
    //     Lds_knobs lds_knobs()                               its capacity, settings and rules, as below
    //     template<pw_int, pw_friction, int LANES, bool LINKED, bool REPLICA_DT> static auto lds_kernel()
    //                                                         REPLICA_DT: the call has a time step per replica (a form
    //                                                         whose kernels decide that at run time returns the same)
    //     template<int LANES, bool LINKED> auto lds_kernel_args(const Lds_layout&)    a tuple: the kernel's arguments
    //                                                         behind d_old_v (LINKED: the Links_view follows them)
    // and may supply lds_layout_of (below).
    struct Lds_knobs {
        int capacity;          // the largest n_max that fits (whole_step_capacity / grid_lds_capacity)
        int allowed;           // -1 = never, 1 = whenever eligible, 0 = where `pays` (whole_steps / lds_steps)
        bool pays;             // the form's *_pay rule
        int steps_per_launch;  // a launch runs at most this many steps
        int lanes;             // lanes per cell: 0 = the engine's choice, 1, 4, 16 or 64 (whole_step_lanes / lds_step_lanes)
        int lanes_for;         // the form's *_lanes_for rule for stateless functors
        long* launches;        // counted here (whole_step_launches / lds_step_launches)
        int* lanes_used;       // the lanes per cell of the last such launch (whole_step_lanes_used / lds_step_lanes_used)
    };
    // THE PLAN of a take_steps call (LINKED: with the ordered links of `slots` slots per replica; has_gen: with other
    // generic forces).  From LDS where the call is eligible -- the replica fits (capacity), there are no generic
    // forces but the links, whose incidence list fits the workgroup's LDS too -- and `allowed` says so; with `lanes`
    // lanes per cell (0: one unless the functors are stateless, then lanes_for) where the term buffer fits, with one
    // otherwise.  (An unlinked launch and a linked one of no slots differ: the list's n_max + 1 offsets are in the
    // linked one.)
    struct Lds_plan {
        bool from_lds;
        int lanes;
        Lds_layout layout;  // of that many lanes: tile and bytes
    };
    // THE FORM'S LAYOUT, which the plan asks for: lds_layout with the form's keys -- unless the form declares an
    // lds_layout_of of its own, whose .bytes cover what it lays out behind lds_layout's regions (the Gabriel form's
    // lists, ya::ens::gabriel_lds_layout) and are 0 where that has no room.
    template<bool LINKED>
    static constexpr Lds_layout lds_layout_of(const int n_max, const int slots, const int lanes)
    {
        return lds_layout<Pt, Form::lds_keys, LINKED>(n_max, slots, lanes);
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool LINKED>
    Lds_plan plan_lds_steps(const Lds_knobs& k, const int slots, const bool has_gen) const
    {
        const auto layout_of = [&](const int lanes) { return Form::template lds_layout_of<LINKED>(n_max, slots, lanes); };
        const bool eligible = n_max <= k.capacity && !has_gen && layout_of(1).bytes != 0;
        if (!eligible || k.allowed < 0 || (k.allowed == 0 && !k.pays)) return {false, 0, Lds_layout{}};
        assert(k.steps_per_launch >= 1);
        int lanes = k.lanes;
        assert(lanes == 0 || lanes == 1 || lanes == 4 || lanes == 16 || lanes == 64);
        if (lanes == 0) lanes = ya::stateless_pair<Pt, pw_int, pw_friction>() ? k.lanes_for : 1;
        if (lanes > 1 && layout_of(lanes).bytes == 0) lanes = 1;  // no room for the term buffer
        const Lds_plan plan{true, lanes, layout_of(lanes)};
        assert(plan.layout.bytes > 0 && (lanes == 1 || plan.layout.tile >= 4));
        return plan;
    }
    // from a run-time lane count to a template parameter (as ya::coop::with_lanes)
    template<typename F>
    static void with_lds_lanes(const int lanes, F&& f)
    {
        if (lanes == 64) return f(std::integral_constant<int, 64>{});
        if (lanes == 16) return f(std::integral_constant<int, 16>{});
        if (lanes == 4) return f(std::integral_constant<int, 4>{});
        f(std::integral_constant<int, 1>{});
    }
    // n_steps steps as launches of at most steps_per_launch steps each of the form's kernel of the plan's lanes, if
    // the plan is to step from LDS; false: nothing was launched.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool LINKED, bool PER_REPLICA>
    bool steps_from_lds(const Step_dt<PER_REPLICA> dt, const int n_steps, const bool has_gen, const Links_view links = Links_view{})
    {
        Form& form = *static_cast<Form*>(this);
        const Lds_knobs k = form.lds_knobs();
        const Lds_plan plan = plan_lds_steps<pw_int, pw_friction, LINKED>(k, links.slots_per_replica, has_gen);
        if (!plan.from_lds) return false;
        *k.lanes_used = plan.lanes;
        const size_t lds = plan.layout.bytes;
        with_lds_lanes(plan.lanes, [&](auto lanes) {
            constexpr int LANES = decltype(lanes)::value;
            const auto kernel = Form::template lds_kernel<pw_int, pw_friction, LANES, LINKED, PER_REPLICA>();
            // beyond 64 KiB of dynamic LDS a kernel has to be told once (per kernel: the static is this instance's)
            static size_t lds_allowed = 64 * 1024;
            if (lds > lds_allowed) {
                YA_CHECK((int)hipFuncSetAttribute(
                    reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                lds_allowed = lds;
            }
            const auto launch = [&](const int steps, auto... more) {
                kernel<<<dim3((unsigned)n_replicas), ya::UPDATE_BLOCK, lds>>>(n_max, d_n, dt.dt, dt.d_dt, steps,
                    fix_kind_of(1), fix_kind_of(2), fix_point, d_X, d_old_v, more...);
                (*k.launches)++;
            };
            const auto args = form.template lds_kernel_args<LANES, LINKED>(plan.layout);
            for (int done = 0; done < n_steps;) {
                const int steps = n_steps - done < k.steps_per_launch ? n_steps - done : k.steps_per_launch;
                if constexpr (LINKED)
                    std::apply([&](auto... more) { launch(steps, more..., links); }, args);
                else
                    std::apply([&](auto... more) { launch(steps, more...); }, args);
                done += steps;
            }
        });
        // d_dX / d_dX1 were neither written nor zeroed: a later take_step with generic forces zeroes them itself
        rhs_zeroed[0] = rhs_zeroed[1] = false;
        return true;
    }
    // take_steps(dt, n_steps, gen_forces) of such a form: from LDS, or n_steps calls of take_step.  The plan does not
    // look at the kind of time step.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Dt>
    void steps(const Dt float_or_replica_dt, const int n_steps, Generic_forces<Pt> gen_forces)
    {
        const auto dt = step_dt(float_or_replica_dt);
        if (steps_from_lds<pw_int, pw_friction, false>(dt, n_steps, !ya::is_no_gen_forces<Pt>(gen_forces))) return;
        for (int s = 0; s < n_steps; s++) one_step<pw_int, pw_friction>(dt, gen_forces);
    }
    // take_steps(dt, n_steps, links): from LDS, or n_steps calls of take_step with ya::ens::link_forces_ordered as the
    // generic force
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Dt>
    void steps(const Dt float_or_replica_dt, const int n_steps, const Replica_links links)
    {
        const auto dt = step_dt(float_or_replica_dt);
        const int slots = links.slots_per_replica;
        assert(slots >= 0 && (size_t)n_replicas * (size_t)slots <= (size_t)links.links.n_max);
        if (steps_from_lds<pw_int, pw_friction, true>(dt, n_steps, false, view_of(links))) return;
        const int n_max = this->n_max;
        const int* d_n = this->d_n;
        Links* l = &links.links;
        Generic_forces<Pt> gen = [l, slots, n_max, d_n](const int n, const Pt* __restrict__ d_X, Pt* d_dX) {
            link_forces_ordered<Pt>(Replica_links{*l, slots}, n, n_max, d_n, d_X, d_dX);
        };
        for (int s = 0; s < n_steps; s++) one_step<pw_int, pw_friction>(dt, gen);
    }
};

}  // namespace ens
}  // namespace ya


// Ensemble<Pt> / Ensemble<Pt, Tile_solver>{n_replicas, n_max}, Ensemble<Pt, Grid_solver>{n_replicas, n_max,
// grid_size, cube_size} (ensemble_grid.cuh) and Ensemble<Pt, Gabriel_solver>{n_replicas, n_max, grid_size, cube_size,
// gabriel_coefficient} (ensemble_gabriel.cuh); no other solver has an ensemble.
template<typename Pt, template<typename> class Solver = Tile_solver, typename Which = void>
class Ensemble {
    static_assert(!std::is_same<Which, void>::value,
        "Ensemble steps all-pairs, grid or Gabriel systems: Ensemble<Pt, Tile_solver>, Ensemble<Pt, Grid_solver> or "
        "Ensemble<Pt, Gabriel_solver>");
};

template<typename Pt, template<typename> class Solver>
class Ensemble<Pt, Solver, std::enable_if_t<std::is_same<Solver<Pt>, Tile_solver<Pt>>::value>>
    : public ya::ens::Stepper<Pt, Ensemble<Pt, Solver>> {
    using Base = ya::ens::Stepper<Pt, Ensemble<Pt, Solver>>;
    friend Base;

public:
    // As Tile_computer::lanes_per_cell: 0 (default) = the engine's choice -- one lane per cell unless the
    // functors are declared stateless (YA_STATELESS), then by the size of the whole launch
    // (ya::ens::lanes_for); 1, 16 or 64 = that many lanes per cell whatever the functor says.  Any
    // choice gives the same bits.
    int lanes_per_cell = 0;

    // take_steps as whole-step launches (ya::ens::whole_steps: one workgroup per replica runs the steps from LDS):
    // -1 = never, 1 = whenever the call is eligible, 0 (default) = the engine's choice, eligible and
    // ya::ens::whole_steps_pay(n_replicas, n_max).  Eligible: no generic forces and
    // n_max <= ya::ens::whole_step_capacity<Pt>().  Any choice gives the same bits.
    int whole_steps = 0;
    // A whole-step launch runs at most this many steps (no single kernel runs unboundedly long); take_steps
    // splits longer requests.
    int steps_per_launch = 256;
    // whole-step launches made so far (which path ran)
    long whole_step_launches = 0;
    // Lanes per cell inside a whole-step launch: 0 (default) = the engine's choice -- one lane per cell unless the
    // functors are declared stateless (YA_STATELESS), then ya::ens::whole_step_lanes_for(n_max); 1, 4, 16 or 64 = that
    // many whatever the functor says (several lanes call the functor for one i at once, as with lanes_per_cell).  A
    // replica whose LDS has no room for the terms of 16 partners (ya::ens::lds_layout's .bytes == 0) is stepped with
    // one lane per cell, still as whole-step launches.  Any choice gives the same bits.
    int whole_step_lanes = 0;
    // the lanes per cell of the last whole-step launch: 0 before any, 1 after that fallback
    int whole_step_lanes_used = 0;

    // Six launches per take_step (per stage: forces, partial sums, update).
    Ensemble(int n_replicas, int n_max) : Base{n_replicas, n_max}
    {
        assert((size_t)n_replicas * (size_t)((n_max + 3) / 4) <= (size_t)0x7fffffff);  // (a launch's x dimension)
    }

    template<Pairwise_interaction<Pt> pw_int>
    void take_steps(float dt, int n_steps, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        take_steps<pw_int, friction_w_neighbour<Pt>>(dt, n_steps, gen_forces);
    }
    // n_steps Heun steps of every replica, bit for bit n_steps calls of take_step: as whole-step launches of at
    // most steps_per_launch steps each where the call is eligible and whole_steps allows it, as that loop otherwise
    // (ya::ens::Stepper::steps).
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_steps(float dt, int n_steps, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        this->template steps<pw_int, pw_friction>(dt, n_steps, gen_forces);
    }

    template<Pairwise_interaction<Pt> pw_int>
    void take_steps(float dt, int n_steps, ya::ens::Replica_links links)
    {
        take_steps<pw_int, friction_w_neighbour<Pt>>(dt, n_steps, links);
    }
    // n_steps Heun steps of every replica with the ORDERED link forces of `links` as the generic force
    // (ensemble_links.cuh: slot s belongs to replica s / slots_per_replica, a slot with an end outside its replica's
    // rows is skipped, a cell's terms are added in slot order).  Bit for bit n_steps calls of
    // take_step(dt, gen) where gen calls ya::ens::link_forces_ordered, and that loop unless the call runs whole:
    // as whole-step launches (ya::ens::whole_steps_linked) where whole_steps allows it, n_max <=
    // ya::ens::whole_step_capacity<Pt>() and the incidence list fits the workgroup's LDS
    // (ya::ens::lds_layout<Pt, false, true>(n_max, slots_per_replica, 1).bytes > 0); with whole_step_lanes lanes per
    // cell where the term buffer fits beside the list, with one otherwise.  A launch reads the links and their
    // count at its start: what a model's kernel left there before the call is what the call sees.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_steps(float dt, int n_steps, ya::ens::Replica_links links)
    {
        this->template steps<pw_int, pw_friction>(dt, n_steps, links);
    }

    // The same calls with replica r's own time step dt.d_dt[r] (this file's header): the same plan, the same launches.
    template<Pairwise_interaction<Pt> pw_int>
    void take_steps(ya::ens::Replica_dt dt, int n_steps, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        take_steps<pw_int, friction_w_neighbour<Pt>>(dt, n_steps, gen_forces);
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_steps(ya::ens::Replica_dt dt, int n_steps, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        this->template steps<pw_int, pw_friction>(dt, n_steps, gen_forces);
    }
    template<Pairwise_interaction<Pt> pw_int>
    void take_steps(ya::ens::Replica_dt dt, int n_steps, ya::ens::Replica_links links)
    {
        take_steps<pw_int, friction_w_neighbour<Pt>>(dt, n_steps, links);
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_steps(ya::ens::Replica_dt dt, int n_steps, ya::ens::Replica_links links)
    {
        this->template steps<pw_int, pw_friction>(dt, n_steps, links);
    }

protected:
    // What ya::ens::Stepper's launches from LDS ask of a form: the layout has no keys; the settings above; the kernels.
    static constexpr bool lds_keys = false;
    typename Base::Lds_knobs lds_knobs()
    {
        constexpr int capacity = ya::ens::whole_step_capacity<Pt>();
        return {capacity, whole_steps, ya::ens::whole_steps_pay(this->n_replicas, this->n_max), steps_per_launch, whole_step_lanes, ya::ens::whole_step_lanes_for(this->n_max), &whole_step_launches,
            &whole_step_lanes_used};
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES, bool LINKED, bool REPLICA_DT>
    static auto lds_kernel()
    {
        if constexpr (LINKED)
            return &ya::ens::whole_steps_linked<Pt, pw_int, pw_friction, LANES>;
        else if constexpr (LANES > 1)
            return &ya::ens::whole_steps_coop<Pt, pw_int, pw_friction, LANES, REPLICA_DT>;
        else
            return &ya::ens::whole_steps<Pt, pw_int, pw_friction, REPLICA_DT>;
    }
    template<int LANES, bool LINKED>
    auto lds_kernel_args(const ya::ens::Lds_layout& layout) const
    {
        if constexpr (LINKED || LANES > 1)
            return std::tuple<int>{layout.tile};
        else
            return std::tuple<>{};
    }

    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void forces(const Pt* d_in, Pt* d_rhs, const bool has_gen)
    {
        const int n_max = this->n_max, n_replicas = this->n_replicas;
        const int* d_n = this->d_n;
        const float3* d_old_v = this->d_old_v;
        // (as Tile_computer::has_16_lanes: points of more than 10 floats have no 16-lane kernel, 64 partners' terms for
        // 16 cells do not fit LDS; the engine's choice is 64 lanes for them, lanes_per_cell = 16 is refused)
        constexpr bool has_16_lanes = ya::tile_coop_partners<Pt, 16>() >= 64;
        int lanes = lanes_per_cell;
        if (lanes == 0) {
            lanes = ya::stateless_pair<Pt, pw_int, pw_friction>() ? ya::ens::lanes_for(n_replicas, n_max) : 1;
            if (lanes == 16 && !has_16_lanes) lanes = 64;
        }
        if (lanes >= 64) {
            const int blocks = (n_max + 3) / 4;
            ya::ens::tile_force_coop_batched<Pt, pw_int, pw_friction, 64><<<this->grid_of(blocks), 256>>>(
                n_max, blocks, d_n, d_in, d_old_v, d_rhs, has_gen);
        } else if (lanes > 1) {
            if constexpr (has_16_lanes) {
                const int blocks = (n_max + 15) / 16;
                ya::ens::tile_force_coop_batched<Pt, pw_int, pw_friction, 16><<<this->grid_of(blocks), 256>>>(
                    n_max, blocks, d_n, d_in, d_old_v, d_rhs, has_gen);
            } else {
                fprintf(stderr, "yalla-hip: Ensemble::lanes_per_cell %d: points of %d floats have no 16-lane kernel (a "
                                "tile of their pair terms does not fit LDS); 0, 1 or 64\n", lanes, ya::N_floats<Pt>::value);
                abort();
            }
        } else {
            const int blocks = (n_max + ya::TILE_BLOCK - 1) / ya::TILE_BLOCK;
            ya::ens::tile_force_batched<Pt, pw_int, pw_friction><<<this->grid_of(blocks), ya::TILE_BLOCK>>>(
                n_max, blocks, d_n, d_in, d_old_v, d_rhs, has_gen);
        }
    }
};

#include "ensemble_grid.cuh"
#include "ensemble_gabriel.cuh"
