// Ensemble<Pt, Gabriel_solver>: M independent Gabriel_solver systems of one point type and one functor pair,
// advanced together (included by ensemble.cuh, whose header describes what all forms share: the replica-major
// layout, ragged device-side counts, ensemble-global ids, generic forces on the flat arrays, the fixed modes;
// ensemble_grid.cuh describes the per-replica grid arrays, their build and the status bits, ya::ens::Grid_form).
//
//     Ensemble<float3, Gabriel_solver> cells{n_replicas, n_max, grid_size, cube_size, gabriel_coefficient};
//     cells.h_n[r] = ...; *cells.row(r, i) = ...; cells.copy_to_device();
//     cells.take_step<my_force>(dt);      // every replica, bit for bit what a lone Solution<float3, Gabriel_solver>
//                                         // of the same rows, old_v, grid_size, cube_size and coefficient gives
//
// THE STEP  16 launches and 2 eight-byte memsets whatever M is, nothing read by the host.  Per stage: the two
// list counters cleared (a stream-ordered memset), four launches build every replica's grid
// (Grid_form::build), gabriel_force_batched, gabriel_force_dense_batched, then ya::ens::Stepper's partial sums
// and update.  Both stages go through a fresh build, as Gabriel_computer's do.
//
// THE DENSE CELLS  A lone Gabriel_computer copies the number of cells with more than GABRIEL_CAP candidates, and
// their largest count, to the host in every stage and sizes the dense kernel's launch and workspace from them.
// Here nothing comes back: a cell's candidates are cells of its own replica, so lists of n_max entries always
// suffice (there is still no cap on candidates); the workspace of `dense_blocks` such sets of lists is allocated
// once, and the dense kernel is queued in every stage with that fixed grid -- its workgroups walk the list
// grid-stride and return at once while it is empty.  The results do not depend on the lists' stride or on which
// workgroup serves which cell.
//     dense_blocks = the workgroups whose lists fit 256 MiB, GABRIEL_DENSE_ARRAYS * n_max * 4 bytes each,
//                    but at least 1 (one workgroup's lists are allocated whatever they take), at most 2048
//                    (Gabriel_computer's cap) and at most n_replicas * n_max (there are no more cells).
// dense_cells() reads how many cells the last force stage left to the dense kernel (blocking; which path ran).
//
// AN EMPTY REPLICA  is left alone, its grid arrays included (never built: -1 everywhere; emptied later: what its
// last build left), as a lone Gabriel_solver's step returns before its build when n = 0 -- where a lone
// Grid_solver, and hence the grid ensemble, leaves an empty grid.
//
// cube_size and gabriel_coefficient hold for every replica and may be changed between steps.
//
// PER-REPLICA COEFFICIENT AND dt  d_gabriel_coefficients (default NULL) = n_replicas floats ON THE DEVICE, caller-owned:
// where it is set replica r's forces use [r] and the scalar member is ignored, on the 16-launch path (dense kernel
// included) and in launches that step from LDS.  The kernels read it when they run, in stream order: a model kernel
// queued before the call may have written it.  take_step / take_steps with ya::ens::Replica_dt{d_dt} in place of dt
// are ensemble.cuh's.  Each replica holds the bits of a lone Solution<Pt, Gabriel_solver> with its two values.
//
// WHOLE STEPS FROM LDS  cells.take_steps<my_force>(dt, 100) is 100 calls of take_step, bit for bit (positions, old_v,
// d_status, the public grid arrays); where a replica fits one workgroup's LDS (n_max <=
// ya::ens::gabriel_lds_capacity<Pt>()), there are no generic forces and `lds_steps` allows it, it runs as ONE launch
// per lds_steps_max steps of one 256-thread workgroup per replica (ya::ens::gabriel_lds_steps): the step is
// ya::ens::whole_steps_in_lds (ensemble.cuh), a stage's forces are the grid form's order of the (cube, id) keys
// (grid_lds_order) and then gabriel_force's stages over those keys, sixteen lanes per cell and sixteen cells per
// round, by the very functions the 16-launch path's kernels call (ya::gabriel::cell_by_group,
// ya::gabriel_force_dense_cell: solvers.cuh; what differs is where they find the sorted cells, Lds_rows below).
// Cells with more than GABRIEL_CAP candidates are done in the same launch and stage, after the rounds, one wavefront
// per cell on lists in LDS: no second kernel, no global workspace, no atomics.  lds_dense_cells() counts them.
//
// THE LDS RULE of such a launch, region after region (ya::ens::gabriel_lds_layout, read by host and kernel):
//   the step's arrays and the keys   ya::ens::lds_layout<Pt, true, false>(n_max, 0, 1), as the grid form's launch.
//   the 16 groups' lists             16-byte aligned; per group of sixteen lanes GABRIEL_CAP entries of NF + 4 floats
//                                    (x, y, z, d while the list is tested, then the kept pairs' terms), of the 4-byte
//                                    sorted slot, and of three bytes (rank, order, kept): gabriel_force's static lists.
//   the dense lists                  only where n_max > GABRIEL_CAP (a smaller replica has no cell with more candidates
//                                    than that: small replicas keep sharing a CU): one flag byte per sorted slot, then,
//                                    16-byte aligned, 4, 2 or 1 sets -- the most that fit -- of GABRIEL_DENSE_ARRAYS
//                                    lists of n_max 4-byte entries each, one set per wavefront that does dense cells.
// No room (bytes = 0) where not even one set fits beside WHOLE_STEP_STATIC_LDS in the workgroup's 160 KiB.  The
// capacities (ya::ens::gabriel_lds_capacity: the largest n_max with room, at most 1024): 1024 rows for a 3-float
// point (142384 bytes, one set), 995 for 4 floats, 826 for 5, 592 for 7, 512 for 8 (513 rows lay out 1024 keys).
//
// Not here: a per-replica cube_size, the fast-arithmetic tier, graph capture, the wall
// model's wall_forces (one wall node per system); in launches that step from LDS also ordered links.
#pragma once

namespace ya {
namespace ens {

// ya::gabriel_force for every replica at once: a one-wavefront workgroup serves GABRIEL_CELLS sorted slots of ONE
// replica, GABRIEL_LANES lanes per cell, by gabriel_force's own body (ya::gabriel_force_cells).  Cube ids and
// offs are the replica's own and gabriel::collect clamps the stencil to [0, n_cubes], so no row of another
// replica is read.  A cell with more than GABRIEL_CAP candidates appends its FLAT row r * n_max + slot to the
// ensemble's one dense list.  d_coefficients (may be NULL): the replicas' own coefficients, [r] instead of the scalar.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(64) void gabriel_force_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const Entry<Pt>* __restrict__ sorted_all, const float4* __restrict__ sorted_v_all,
    const int* __restrict__ cube_id_all, const int* __restrict__ offs_all, const int gs, const int n_cubes,
    const float cube_size, const float gabriel_coefficient, const float* __restrict__ d_coefficients,
    Pt* __restrict__ d_dX_all, const bool has_gen, int* __restrict__ dense, int* __restrict__ n_dense)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    if (w.block * GABRIEL_CELLS >= n) return;  // (the whole workgroup: blocks past n[r] return at once)
    const size_t base = (size_t)w.replica * n_max;
    gabriel_force_cells<Pt, pw_int, pw_friction>(n, w.block * GABRIEL_CELLS, (int)base, (int)base, sorted_all + base,
        sorted_v_all + base, cube_id_all + base, offs_all + (size_t)w.replica * (n_cubes + 1), gs, n_cubes, cube_size,
        value_of(d_coefficients, gabriel_coefficient, w.replica), d_dX_all + base, has_gen, dense, n_dense);
}

// ya::gabriel_force_dense for the ensemble's one list of flat rows: a grid-stride walk, one wavefront per cell
// (ya::gabriel_force_dense_cell), the replica is row / n_max -- and with it the coefficient, d_coefficients[replica]
// where that is set --, the lists hold n_max entries each.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(64) void gabriel_force_dense_batched(const int n_max, const int* __restrict__ dense,
    const int* __restrict__ n_dense, const Entry<Pt>* __restrict__ sorted_all, const float4* __restrict__ sorted_v_all,
    const int* __restrict__ cube_id_all, const int* __restrict__ offs_all, const int gs, const int n_cubes,
    const float cube_size, const float gabriel_coefficient, const float* __restrict__ d_coefficients,
    Pt* __restrict__ d_dX_all, const bool has_gen, float* __restrict__ workspace)
{
    const int listed = n_dense[0];
    if ((int)blockIdx.x >= listed) return;  // (the usual case: no dense cell at all)
    const long stride = n_max;
    float* x = workspace + GABRIEL_DENSE_ARRAYS * stride * blockIdx.x;
    for (int t = blockIdx.x; t < listed; t += gridDim.x) {
        const int row = dense[t];
        const int replica = row / n_max;
        const size_t base = (size_t)replica * n_max;
        gabriel_force_dense_cell<Pt, pw_int, pw_friction>(threadIdx.x, row - (int)base, (int)base, sorted_all + base,
            sorted_v_all + base, cube_id_all + base, offs_all + (size_t)replica * (n_cubes + 1), gs, n_cubes, cube_size,
            value_of(d_coefficients, gabriel_coefficient, replica), d_dX_all + base, has_gen, x, stride);
    }
}

// Workgroups of the dense launch = sets of lists in its workspace (this file's header states the rule).
inline int gabriel_dense_blocks(const int n_replicas, const int n_max)
{
    const size_t per_block = (size_t)GABRIEL_DENSE_ARRAYS * (size_t)n_max;  // floats
    const size_t fit = ((size_t)64 << 20) / per_block;                       // 256 MiB of floats
    const size_t rows = (size_t)n_replicas * (size_t)n_max;
    size_t blocks = fit < 2048 ? fit : 2048;
    if (blocks > rows) blocks = rows;
    return blocks < 1 ? 1 : (int)blocks;
}

// ---- whole Heun steps of a replica from LDS (Ensemble<Pt, Gabriel_solver>::take_steps, lds_steps) -----------------
constexpr int GABRIEL_LDS_GROUPS = UPDATE_BLOCK / GABRIEL_LANES;  // cells per round
// one group's lists: NF + 4 floats, the slot and three bytes for each of GABRIEL_CAP entries (a multiple of 64 bytes)
template<typename Pt>
constexpr size_t gabriel_lds_group_bytes()
{
    return (size_t)GABRIEL_CAP * ((N_floats<Pt>::value + 4) * sizeof(float) + sizeof(int) + 3);
}
// THE LDS LAYOUT of ya::ens::gabriel_lds_steps (this file's header states the rule): byte offsets from the start of
// the dynamic LDS.
struct Gabriel_lds_layout {
    Lds_layout step;     // lds_layout<Pt, true, false>(n_max, 0, 1): the step's arrays and the keys
    size_t lists;        // the 16 groups' lists, gabriel_lds_group_bytes<Pt>() each
    size_t dense_flags;  // n_max > GABRIEL_CAP: one byte per sorted slot, "this stage's dense path does this cell"
    size_t dense;        // and dense_sets sets of GABRIEL_DENSE_ARRAYS lists of n_max 4-byte entries
    int dense_sets;      // 4, 2 or 1; 0 where n_max <= GABRIEL_CAP
    size_t bytes;        // the launch's dynamic LDS; 0 = no room
};
template<typename Pt>
constexpr Gabriel_lds_layout gabriel_lds_layout(const int n_max)
{
    Gabriel_lds_layout l{};
    l.step = lds_layout<Pt, true, false>(n_max, 0, 1);
    l.lists = lds_rounded_up(l.step.bytes, 16);
    size_t end = l.lists + GABRIEL_LDS_GROUPS * gabriel_lds_group_bytes<Pt>();
    if (n_max > GABRIEL_CAP) {
        l.dense_flags = end;
        l.dense = lds_rounded_up(end + (size_t)n_max, 16);
        const size_t set = (size_t)GABRIEL_DENSE_ARRAYS * (size_t)n_max * sizeof(float);
        for (int sets = 4; sets >= 1 && l.dense_sets == 0; sets >>= 1)
            if (l.dense + sets * set + WHOLE_STEP_STATIC_LDS <= LDS_PER_WORKGROUP) l.dense_sets = sets;
        if (l.dense_sets == 0) return l;  // no room
        end = l.dense + l.dense_sets * set;
    }
    if (end + WHOLE_STEP_STATIC_LDS > LDS_PER_WORKGROUP) return l;  // no room
    l.bytes = end;
    return l;
}
// The largest n_max whose launch fits one workgroup, ya::fixed_velocity_from_partials' static fold scratch
// included; at most WHOLE_STEP_MAX_ROWS.
template<typename Pt>
constexpr int gabriel_lds_capacity()
{
    int rows = 0;
    for (int n = 1; n <= WHOLE_STEP_MAX_ROWS; n++)
        if (gabriel_lds_layout<Pt>(n).bytes != 0) rows = n;  // (room never comes back once it is gone)
    return rows;
}

// gabriel::Sorted_rows (solvers.cuh) for the replica in LDS: after grid_lds_order, key s holds the cube of the cell in
// sorted slot s and its local id; positions and old_v are the stage's LDS arrays, indexed by that id; offs[c] is a
// binary search of the keys.
template<typename Pt>
struct Lds_rows {
    const unsigned long long* key;
    int n;
    const Pt* sh_in;
    const float3* sh_v;
    __device__ __forceinline__ Entry<Pt> entry(const int k) const
    {
        Entry<Pt> e;
        e.id = (int)(unsigned)key[k];
        e.X = sh_in[e.id];
        return e;
    }
    __device__ __forceinline__ Pt X(const int k) const { return sh_in[(int)(unsigned)key[k]]; }
    __device__ __forceinline__ float4 v(const int k) const
    {
        const float3 v = sh_v[(int)(unsigned)key[k]];
        return make_float4(v.x, v.y, v.z, 0.f);
    }
    __device__ __forceinline__ int cube(const int k) const { return (int)(key[k] >> 32); }
    __device__ __forceinline__ int first_slot(const int c) const { return grid_lds_lower_bound(key, n, c); }
};

// n_steps Heun steps of replica blockIdx.x by ONE 256-thread workgroup, from LDS (dynamic LDS of
// gabriel_lds_layout<Pt>(n_max).bytes > 0): ya::ens::whole_steps_in_lds with a stage's forces =
//   order    grid_lds_order of the stage's positions (its barriers);
//   rounds   ceil(n / 16) rounds of 16 sorted slots, a group of GABRIEL_LANES lanes per slot, each by
//            gabriel::cell_by_group on the group's lists; a group past n skips its cell, every lane reaches the
//            wave_sync that ends the round (the group's lists are the next round's).  No workgroup barrier in here:
//            a group lies in one wavefront.  A cell with more than GABRIEL_CAP candidates writes no right-hand side
//            and raises its slot's flag; every other slot's flag is lowered.
//   dense    n_max > GABRIEL_CAP only: a barrier, then wavefront w < dense_sets walks the slots w, w + dense_sets, ...
//            and does the flagged ones by ya::gabriel_force_dense_cell on its set of lists of n_max entries (a cell's
//            candidates are cells of its replica: the lists always suffice).
// Bit for bit n_steps of the 16-launch take_step without generic forces.  Global memory is what grid_lds_steps reads
// and writes -- d_n[r] read once; rows [0, n_r) of d_X and d_old_v read at the start and written at the end; at the
// end the grid arrays of the LAST stage's order and YA_STATUS_OUT_OF_GRID in d_status[r] if a cell of any stage lay
// outside the grid -- and ONE atomic add of the (cell, stage) pairs that took the dense path to *d_lds_dense, where
// there were any.  A replica with n_r <= 0 returns at once and is left alone, grid arrays included (this file's
// header).  Every barrier is reached by all 256 threads; the trip counts around them depend on n_r, n_max and n_steps.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(UPDATE_BLOCK) void gabriel_lds_steps(const int n_max, const int* __restrict__ d_n,
    const float dt, const float* __restrict__ d_dt, const int n_steps, const int kind1, const int kind2,
    const int fix_point, Pt* __restrict__ d_X_all, float3* __restrict__ d_old_v_all, const float cs, const int gs,
    const int n_cubes, const float gabriel_coefficient, const float* __restrict__ d_coefficients,
    int* __restrict__ d_cube_id_all, int* __restrict__ d_point_id_all, int* __restrict__ d_offs_all,
    int* __restrict__ d_status, unsigned long long* __restrict__ d_lds_dense)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char gabriel_step_lds[];
    constexpr int NF = N_floats<Pt>::value;
    const int replica = blockIdx.x;
    const int n = count_of(d_n, replica, n_max);
    if (n <= 0) return;  // (the whole workgroup; an empty replica is left alone)
    const Gabriel_lds_layout layout = gabriel_lds_layout<Pt>(n_max);
    unsigned long long* const sh_key = reinterpret_cast<unsigned long long*>(gabriel_step_lds + layout.step.keys);
    const int group = threadIdx.x / GABRIEL_LANES, lane = threadIdx.x % GABRIEL_LANES;
    const int first_lane = (group % GABRIEL_CELLS) * GABRIEL_LANES;  // the group's first lane in its wavefront
    unsigned char* const mine = gabriel_step_lds + layout.lists + (size_t)group * gabriel_lds_group_bytes<Pt>();
    float(*const list)[GABRIEL_CAP] = reinterpret_cast<float(*)[GABRIEL_CAP]>(mine);
    int* const slot = reinterpret_cast<int*>(list + (NF + 4));
    unsigned char(*const ranks)[GABRIEL_CAP] = reinterpret_cast<unsigned char(*)[GABRIEL_CAP]>(slot + GABRIEL_CAP);
    unsigned char* const sh_dense_flag = gabriel_step_lds + layout.dense_flags;
    const int dense_sets = layout.dense_sets;
    const int wave = threadIdx.x / 64, wave_lane = threadIdx.x % 64;
    // (the set of wavefront `wave`, which exists where wave < dense_sets and is not touched otherwise)
    float* const dense_lists =
        reinterpret_cast<float*>(gabriel_step_lds + layout.dense) + (size_t)wave * GABRIEL_DENSE_ARRAYS * n_max;
    const int id_base = replica * n_max;
    bool outside = false;
    int dense_done = 0;  // (cell, stage) pairs this wavefront did on the dense path
    // (the replica's own time step and coefficient where the call has them, read once)
    const float dt_r = value_of(d_dt, dt, replica), coefficient = value_of(d_coefficients, gabriel_coefficient, replica);
    whole_steps_in_lds<Pt>(n_max, n, replica, dt_r, n_steps, kind1, kind2, fix_point, d_X_all, d_old_v_all,
        gabriel_step_lds, [&](const Pt* sh_in, const float3* sh_v, Pt* sh_rhs) __attribute__((always_inline)) {
            outside |= grid_lds_order<Pt>(n, sh_in, cs, gs, n_cubes, sh_key);
            const Lds_rows<Pt> rows{sh_key, n, sh_in, sh_v};
            for (int first = 0; first < n; first += GABRIEL_LDS_GROUPS) {
                const int s = first + group;
                if (s < n) {
                    if (dense_sets > 0 && lane == 0) sh_dense_flag[s] = 0;
                    gabriel::cell_by_group<Pt, pw_int, pw_friction>(lane, first_lane, s, id_base, rows, gs, n_cubes, cs,
                        coefficient, list, slot, ranks, sh_rhs, false, [&](const int) {
                            if (dense_sets > 0 && lane == 0) sh_dense_flag[s] = 1;  // (without flags no cell has so many)
                        });
                }
                coop::wave_sync();
            }
            if (dense_sets > 0) {  // (n_max > GABRIEL_CAP: the same for every thread)
                __syncthreads();
                if (wave < dense_sets) {
                    for (int s = wave; s < n; s += dense_sets) {
                        if (!sh_dense_flag[s]) continue;
                        gabriel_force_dense_cell<Pt, pw_int, pw_friction>(wave_lane, s, id_base, rows, gs, n_cubes, cs,
                            coefficient, sh_rhs, false, dense_lists, (long)n_max);
                        dense_done++;
                    }
                }
            }
        });
    // (the keys are the last stage's: its forces were followed by barriers, and nothing has written them since)
    const size_t base = (size_t)replica * n_max;
    int* __restrict__ d_offs = d_offs_all + (size_t)replica * (n_cubes + 1);
    for (int s = threadIdx.x; s < n; s += UPDATE_BLOCK) {
        const unsigned long long key = sh_key[s];
        d_cube_id_all[base + s] = (int)(key >> 32);
        d_point_id_all[base + s] = (int)(unsigned)key;
    }
    for (int c = threadIdx.x; c <= n_cubes; c += UPDATE_BLOCK) d_offs[c] = grid_lds_lower_bound(sh_key, n, c);
    // The threads' status flags and the wavefronts' dense counts meet in the fold's scratch, which nothing uses after
    // the last step (as in grid_lds_steps: no static LDS beyond WHOLE_STEP_STATIC_LDS).
    int* sh_meet = lds_fold_scratch<Pt>(gabriel_step_lds, n_max);
    if (threadIdx.x == 0) sh_meet[0] = 0;
    __syncthreads();
    if (outside) sh_meet[0] = 1;  // (every writer writes the same value)
    if (wave_lane == 0) sh_meet[1 + wave] = dense_done;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sh_meet[0]) atomicOr(d_status + replica, YA_STATUS_OUT_OF_GRID);
        const int dense_total = sh_meet[1] + sh_meet[2] + sh_meet[3] + sh_meet[4];
        if (dense_total > 0) atomicAdd(d_lds_dense, (unsigned long long)dense_total);
    }
}

// Whether these launches beat the 16-launch step when the model leaves the choice to the engine
// (Ensemble<Pt, Gabriel_solver>::lds_steps == 0): THE RULE THE TABLES SUPPORT (tools/ensemble_bench.py --solver gabriel
// --lds-steps, MI355X, relu).  The rule does not see how many steps a call takes, so it answers
// true only where launches of ONE step each and of 256 steps each both beat the 16 launches by more than the
// shape's spread: that is ONE round, n <= 16.  Measured (profiles/ensemble_gabriel_lds_steps_small_bench.json):
// n = 4 and n = 16 at M = 1, 16, 64, 128, 256 -- 2.3 - 2.7 x and 1.5 - 1.8 x with one step per launch, 2.6 - 3.1 x and
// 1.6 - 2.0 x with 256, spreads <= 0.14.  NOT MEASURED, AND ANSWERED BY INTERPOLATION: the other n_max up to 16 (the
// same single round of fewer groups) and the M between those five.  Everything else measured is false: two rounds
// (n = 20, M <= 256) win by 6 - 10 % with 256 steps per launch but tie (1.00 - 1.01 x) with one; n = 32 is 0.89 - 1.07 x;
// from 64 cells on, and from 1024 replicas on, every shape loses (profiles/ensemble_gabriel_lds_steps_bench.json:
// 0.82 x down to 0.03 x -- a workgroup serves 16 cells per round, the 16 launches spread a replica over the chip).
inline bool gabriel_lds_steps_pay(const int n_replicas, const int n_max, const int n_cubes)
{
    return n_max <= GABRIEL_LDS_GROUPS && n_replicas <= 256;
}

}  // namespace ens
}  // namespace ya


template<typename Pt, template<typename> class Solver>
class Ensemble<Pt, Solver, std::enable_if_t<std::is_same<Solver<Pt>, Gabriel_solver<Pt>>::value>>
    : public ya::ens::Grid_form<Pt, Ensemble<Pt, Solver>> {
    using Base = ya::ens::Grid_form<Pt, Ensemble<Pt, Solver>>;
    friend ya::ens::Stepper<Pt, Ensemble<Pt, Solver>>;

public:
    // (grid_size, n_cubes, cube_size, d_cube_id, d_point_id, d_offs, d_status, sizes_ok, status, check_status,
    // copy_to_host: ya::ens::Grid_form)
    float gabriel_coefficient;  // of every replica; may be changed between steps
    // n_replicas floats on the device, caller-owned; non-null: replica r uses [r], the scalar member is ignored
    const float* d_gabriel_coefficients = nullptr;
    const int dense_blocks;     // workgroups of the dense launch, ya::ens::gabriel_dense_blocks

    // take_steps as launches that step from LDS (ya::ens::gabriel_lds_steps: one workgroup per replica): -1 = never,
    // 1 = whenever the call is eligible, 0 (default) = the engine's choice, eligible and
    // ya::ens::gabriel_lds_steps_pay(n_replicas, n_max, n_cubes).  Eligible: no generic forces and
    // n_max <= ya::ens::gabriel_lds_capacity<Pt>().  Any choice gives the same bits.
    int lds_steps = 0;
    // Such a launch runs at most this many steps (no single kernel runs unboundedly long); take_steps splits longer
    // requests.
    int lds_steps_max = 256;
    // such launches made so far (which path ran)
    long lds_step_launches = 0;

    Ensemble(int n_replicas, int n_max, int grid_size = 50, float cube_size = 1, float gabriel_coefficient = 0.8)
        : Base{"Gabriel_solver", n_replicas, n_max, grid_size, cube_size}, gabriel_coefficient{gabriel_coefficient},
          dense_blocks{ya::ens::gabriel_dense_blocks(n_replicas, n_max)}
    {
        YA_CHECK(ya_malloc((void**)&d_dense, (this->rows() + 2) * sizeof(int)));
        YA_CHECK(ya_memset_async(d_dense, 0, 2 * sizeof(int), nullptr));
        const size_t floats = (size_t)dense_blocks * ya::GABRIEL_DENSE_ARRAYS * (size_t)n_max;
        YA_CHECK(ya_malloc((void**)&d_workspace, floats * sizeof(float)));
        YA_CHECK(ya_malloc((void**)&d_lds_dense, sizeof(unsigned long long)));
        YA_CHECK(ya_memset_async(d_lds_dense, 0, sizeof(unsigned long long), nullptr));
    }
    ~Ensemble()
    {
        ya_free(d_dense);
        ya_free(d_workspace);
        ya_free(d_lds_dense);
    }

    template<Pairwise_interaction<Pt> pw_int>
    void take_steps(float dt, int n_steps, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        take_steps<pw_int, friction_w_neighbour<Pt>>(dt, n_steps, gen_forces);
    }
    // n_steps Heun steps of every replica, bit for bit n_steps calls of take_step (positions, old_v, the four grid
    // arrays of the last stage's build, the status bits): as launches of at most lds_steps_max steps each that step
    // from LDS where the call is eligible and lds_steps allows it, as that loop otherwise (ya::ens::Stepper::steps).
    // After such launches d_dX / d_X1 / d_dX1, the build's private arrays and dense_cells() are left as they were.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_steps(float dt, int n_steps, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        this->template steps<pw_int, pw_friction>(dt, n_steps, gen_forces);
    }
    // The same calls with replica r's own time step dt.d_dt[r] (ensemble.cuh's header): the same plan, the same launches.
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

    // Blocking read: the (cell, stage) pairs that took the dense path INSIDE launches that stepped from LDS, over all
    // replicas, since construction.  The step never reads it.  (dense_cells() is the 16-launch path's.)
    unsigned long long lds_dense_cells()
    {
        unsigned long long cells = 0;
        YA_CHECK(ya_memcpy_d2h(&cells, d_lds_dense, sizeof(cells)));
        return cells;
    }

    // Blocking read: the cells the last force stage left to gabriel_force_dense_batched (more than GABRIEL_CAP
    // candidates), over all replicas.  The step never reads it.
    int dense_cells()
    {
        int listed = 0;
        YA_CHECK(ya_memcpy_d2h(&listed, d_dense, sizeof(int)));
        return listed;
    }

protected:
    int* d_dense = nullptr;  // [0] cells left to the dense kernel, [1] their largest count, then their flat rows
    float* d_workspace = nullptr;  // [dense_blocks][GABRIEL_DENSE_ARRAYS][n_max]
    unsigned long long* d_lds_dense = nullptr;  // lds_dense_cells()

    // What ya::ens::Stepper's launches from LDS ask of a form: the layout has keys and, behind them, this form's lists
    // (lds_layout_of: the step's regions with the whole launch's bytes, 0 = no room); the settings above -- there is
    // no lanes knob: the Gabriel force has one shape, the plan's lanes are 1 --; the kernel.
    static constexpr bool lds_keys = true;
    template<bool LINKED>
    static constexpr ya::ens::Lds_layout lds_layout_of(const int n_max, const int, const int)
    {
        static_assert(!LINKED, "the Gabriel form steps without ordered links");
        const ya::ens::Gabriel_lds_layout mine = ya::ens::gabriel_lds_layout<Pt>(n_max);
        ya::ens::Lds_layout l = mine.step;
        l.bytes = mine.bytes;
        return l;
    }
    int lds_lanes_used = 0;  // (the plan's 1 after such a launch)
    typename ya::ens::Stepper<Pt, Ensemble<Pt, Solver>>::Lds_knobs lds_knobs()
    {
        constexpr int capacity = ya::ens::gabriel_lds_capacity<Pt>();
        return {capacity, lds_steps, ya::ens::gabriel_lds_steps_pay(this->n_replicas, this->n_max, this->n_cubes),
            lds_steps_max, 1, 1, &lds_step_launches, &lds_lanes_used};
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES, bool LINKED, bool REPLICA_DT>
    static auto lds_kernel()  // (REPLICA_DT: the kernel decides at run time)
    {
        return &ya::ens::gabriel_lds_steps<Pt, pw_int, pw_friction>;
    }
    template<int LANES, bool LINKED>
    auto lds_kernel_args(const ya::ens::Lds_layout&) const
    {
        return std::make_tuple(this->cube_size, this->grid_size, this->n_cubes, gabriel_coefficient,
            d_gabriel_coefficients, this->d_cube_id, this->d_point_id, this->d_offs, this->d_status, d_lds_dense);
    }

    // A memset and six launches: the counters, the grid of every replica from d_in, then the forces.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void forces(const Pt* d_in, Pt* d_rhs, const bool has_gen)
    {
        const int n_max = this->n_max;
        YA_CHECK(ya_memset_async(d_dense, 0, 2 * sizeof(int), nullptr));
        this->template build<false>(d_in);  // (an empty replica is left alone, grid arrays included)
        const int blocks = (n_max + ya::GABRIEL_CELLS - 1) / ya::GABRIEL_CELLS;
        ya::ens::gabriel_force_batched<Pt, pw_int, pw_friction><<<this->grid_of(blocks), 64>>>(n_max, blocks, this->d_n,
            this->d_sorted, this->d_sorted_v, this->d_cube_id, this->d_offs, this->grid_size, this->n_cubes,
            this->cube_size, gabriel_coefficient, d_gabriel_coefficients, d_rhs, has_gen, d_dense + 2, d_dense);
        ya::ens::gabriel_force_dense_batched<Pt, pw_int, pw_friction><<<dense_blocks, 64>>>(n_max, d_dense + 2, d_dense,
            this->d_sorted, this->d_sorted_v, this->d_cube_id, this->d_offs, this->grid_size, this->n_cubes,
            this->cube_size, gabriel_coefficient, d_gabriel_coefficients, d_rhs, has_gen, d_workspace);
    }
};
