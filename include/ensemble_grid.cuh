// Ensemble<Pt, Grid_solver>: M independent Grid_solver systems of one point type and one functor pair, advanced
// together (included by ensemble.cuh, whose header describes what both forms share: the replica-major layout,
// ragged device-side counts, ensemble-global ids, generic forces on the flat arrays, the fixed modes).
//
//     Ensemble<float3, Grid_solver> cells{n_replicas, n_max, grid_size, cube_size};
//     cells.h_n[r] = ...; *cells.row(r, i) = ...; cells.copy_to_device();
//     cells.take_step<my_force>(dt);      // every replica, bit for bit what a lone Solution<float3, Grid_solver>
//                                         // of the same rows, old_v, grid_size, cube_size and settings gives
//
// THE STEP  14 launches whatever M is, nothing read by the host.  Per stage: four launches build every replica's
// grid (count, scan, scatter, order), one computes the forces, then ya::ens::Stepper's partial sums and update.
// Both stages go d_X -> d_X1 through a fresh build (a lone system's sorted_pipeline = 0, bit-identical to its
// default).
//
// THE GRID ARRAYS  are the reference's Grid arrays, per replica, with replica-LOCAL contents:
//     d_cube_id [r * n_max + s]            cube of the replica's sorted slot s, s < n_r
//     d_point_id[r * n_max + s]            local id of the cell in that slot; inside a cube ids ascend
//     d_offs    [r * (n_cubes + 1) + c]    first slot of cube c, relative to the replica's first row;
//                                          d_offs[.. + n_cubes] = n_r.  cube_start[c] / cube_end[c] of the
//                                          reference are offs[c] / offs[c + 1] - 1 where the cube is not empty
// They are valid after a step for the LAST build (stage 2: the predictor's positions), as a lone Solution's are.
// A replica with n_r = 0 gets an empty grid (every cube empty), as an empty Solution's step leaves its Grid.
//
// WHOLE STEPS FROM LDS  cells.take_steps<my_force>(dt, 100) is 100 calls of take_step, bit for bit (positions, old_v,
// d_status, the public grid arrays); where a replica fits one workgroup's LDS (n_max <= ya::ens::grid_lds_capacity<Pt>(),
// 1024 for the usual point types), there are no generic forces and `lds_steps` allows it, it runs as ONE launch per
// lds_steps_max steps: a workgroup per replica sorts the replica's (cube, id) keys in LDS, finds the stencil rows by
// searching that order and steps from LDS (ya::ens::grid_lds_steps) -- no counters, nothing of size grid_size^3 touched
// in between.  The step itself is ya::ens::whole_steps_in_lds (ensemble.cuh), which the all-pairs whole steps call too.
// SEVERAL LANES PER CELL  Inside such a launch `lds_step_lanes` = 4, 16 or 64 lanes share a cell's candidates
// (ya::ens::grid_lds_walk_coop: terms into an LDS buffer behind the keys, one lane per component adds them in the walk's
// order), for replicas of a few dozen cells, which leave most of the workgroup idle otherwise: the same bits.
// Not built for these launches: the fast tier, graph capture.  (The Gabriel form steps from LDS by a kernel of its
// own, ya::ens::gabriel_lds_steps in ensemble_gabriel.cuh, on this file's order and search of the keys.)
//
// LINKS  cells.take_steps<my_force>(dt, K, ya::ens::Replica_links{links, S}) steps with the ORDERED link forces of a
// Links object over the flat id space (ensemble_links.cuh: slot s belongs to replica s / S, a == b is inert, slots
// from *links.d_n on are unused, a slot with an end outside its own replica's rows is skipped, a cell's terms are
// added in ascending slot order from +0, the right-hand side is "zero, links, force kernel").  The result is DEFINED
// as K calls of take_step(dt, gen) with gen calling ya::ens::link_forces_ordered<Pt>; where the replica and its
// incidence list fit one workgroup's LDS (ya::ens::lds_layout<Pt, true, true>(n_max, S, 1).bytes != 0) and `lds_steps` allows
// it, the call runs as launches that step from LDS (ya::ens::grid_lds_steps_linked), bit for bit alike, the public
// grid arrays and d_status included, with lds_step_lanes lanes per cell where the term buffer fits behind the list.
// Out of scope for these linked launches: the Gabriel form, the fast tier, graph capture, links that change inside a
// launch (a launch reads the links and their count at its start).
//
// COST  Every stage scans n_replicas * grid_size^3 counters (one workgroup per replica walks its cubes) whatever
// the replicas hold: a sweep picks grid_size to fit its replicas, not the single system's default of 50.
//
// STATUS  A cell outside its replica's grid is clamped into it (memory-safe, as Grid's build does) and raises the
// replica's sticky YA_STATUS_OUT_OF_GRID bit in d_status[r]; the step never reads it.  status(r) reads it;
// copy_to_host() aborts naming the replica, as Grid::check_status does.  Other replicas are unaffected.
//
// SHARED  The build, its arrays and the status code are ya::ens::Grid_form (below), which Ensemble<Pt, Gabriel_solver>
// (ensemble_gabriel.cuh) derives from too.
//
// PER-REPLICA dt  take_step / take_steps with ya::ens::Replica_dt{d_dt} in place of dt (ensemble.cuh's header): every
// path of this form, the linked ones included.
//
// Not here: the fast-arithmetic tier, graph capture, a per-replica cube_size or grid_size, the sorted-space
// second stage, grid_force_bits' tails, slabs.
#pragma once

#include "cube_id.cuh"

namespace ya {
namespace ens {

// Cube id of every row (ya::cube_id_of, clamped as k_bin clamps it) and its arrival rank in the cube's counter.
template<typename Pt>
__global__ __launch_bounds__(UPDATE_BLOCK) void grid_count_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const Pt* __restrict__ d_X_all, const float cs, const int gs, const int n_cubes,
    int* __restrict__ cube_of, int* __restrict__ rank, int* __restrict__ count, int* __restrict__ status)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    const int local = w.block * UPDATE_BLOCK + threadIdx.x;
    if (local >= n) return;
    const size_t row = (size_t)w.replica * n_max + local;
    const Pt p = d_X_all[row];
    int id = cube_id_of(p.x, p.y, p.z, cs, gs);
    if (id < 0 || id >= n_cubes) {
        atomicOr(status + w.replica, YA_STATUS_OUT_OF_GRID);
        id = id < 0 ? 0 : n_cubes - 1;
    }
    cube_of[row] = id;
    // any arrival order inside a cube is fine: grid_order_batched restores ascending ids
    rank[row] = atomicAdd(count + (size_t)w.replica * n_cubes + id, 1);
}

// Exclusive scan of a replica's n_cubes counters by ONE workgroup that walks them, 2048 at a time, with a
// running carry: offs[c] relative to the replica's first row, offs[n_cubes] = n_r, the counters re-zeroed in
// passing.  No workgroup waits for another.  BUILD_EMPTY = false leaves an empty replica's offs as they are (its
// counters are zero already): what a lone Gabriel_solver's step, which returns before its build, leaves of its Grid.
constexpr int SCAN_ITEMS = 8;
template<bool BUILD_EMPTY>
__global__ __launch_bounds__(UPDATE_BLOCK) void grid_scan_batched(const int n_max, const int* __restrict__ d_n,
    const int n_cubes, int* __restrict__ count_all, int* __restrict__ offs_all)
{
    __shared__ int sh_wave[2][UPDATE_BLOCK / 64];
    const int r = blockIdx.x;
    if (!BUILD_EMPTY && count_of(d_n, r, n_max) <= 0) return;  // (the whole workgroup)
    const int n = max(count_of(d_n, r, n_max), 0);  // (an empty replica's grid is built too, empty: a lone Solution's is)
    int* __restrict__ count = count_all + (size_t)r * n_cubes;
    int* __restrict__ offs = offs_all + (size_t)r * (n_cubes + 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0, turn = 0;
    for (int chunk = 0; chunk < n_cubes; chunk += UPDATE_BLOCK * SCAN_ITEMS, turn ^= 1) {
        const int first = chunk + threadIdx.x * SCAN_ITEMS;
        int c[SCAN_ITEMS], total = 0;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) {
            c[k] = first + k < n_cubes ? count[first + k] : 0;
            total += c[k];
        }
        int incl = total;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) sh_wave[turn][wave] = incl;
        __syncthreads();  // (two copies of sh_wave: one barrier per chunk)
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < UPDATE_BLOCK / 64; k++) {
            before += k < wave ? sh_wave[turn][k] : 0;
            all += sh_wave[turn][k];
        }
        int run = carry + before + incl - total;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) {
            if (first + k < n_cubes) {
                offs[first + k] = run;
                count[first + k] = 0;
            }
            run += c[k];
        }
        carry += all;
    }
    if (threadIdx.x == 0) offs[n_cubes] = n;
}

// slot = offs[cube] + rank, arrival order inside a cube
__global__ __launch_bounds__(UPDATE_BLOCK) void grid_scatter_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const int n_cubes, const int* __restrict__ cube_of, const int* __restrict__ rank,
    const int* __restrict__ offs_all, int* __restrict__ arrival, int* __restrict__ cube_id)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    const int local = w.block * UPDATE_BLOCK + threadIdx.x;
    if (local >= n) return;
    const size_t base = (size_t)w.replica * n_max;
    const int c = cube_of[base + local];
    const int slot = offs_all[(size_t)w.replica * (n_cubes + 1) + c] + rank[base + local];
    arrival[base + slot] = local;
    cube_id[base + slot] = c;
}

// Ascending ids inside each cube (k_order's rank count within the cube's segment: the stable order, the order of
// every sum) and the cells gathered into that order: Entry{X, local id}, old_v as float4, point_id.
template<typename Pt>
__global__ __launch_bounds__(UPDATE_BLOCK) void grid_order_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const int n_cubes, const int* __restrict__ arrival, const int* __restrict__ cube_id,
    const int* __restrict__ offs_all, const Pt* __restrict__ d_X_all, const float3* __restrict__ d_old_v_all,
    int* __restrict__ point_id, Entry<Pt>* __restrict__ sorted, float4* __restrict__ sorted_v)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    const int s = w.block * UPDATE_BLOCK + threadIdx.x;
    if (s >= n) return;
    const size_t base = (size_t)w.replica * n_max;
    const int* __restrict__ offs = offs_all + (size_t)w.replica * (n_cubes + 1);
    const int c = cube_id[base + s];
    const int a = offs[c], b = offs[c + 1];
    const int p = arrival[base + s];
    int smaller = 0;
    for (int t = a; t < b; t++) smaller += arrival[base + t] < p;
    const size_t dst = base + a + smaller;
    point_id[dst] = p;
    Entry<Pt> e;
    e.X = d_X_all[base + p];
    e.id = p;
    sorted[dst] = e;
    const float3 v = d_old_v_all[base + p];
    sorted_v[dst] = make_float4(v.x, v.y, v.z, 0.f);
}

// ya::grid_force_bits for every replica at once: a one-wavefront workgroup serves 64 sorted slots of ONE
// replica.  The tile is grid_force_bits' own (ya::grid_force_bits_tile): whole tiles only (no tail, no parts).
// Cube ids and offs are the replica's own, so no stencil row reaches another replica's rows.
// (OFF32: a replica's old_v through 32-bit byte offsets from the replica's own base, bits::offsets_fit_32_bits(n_max))
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool STAGE_V, bool OFF32>
__global__ __launch_bounds__(bits::BLOCK, bits::Min_waves<Pt>::value) void grid_force_bits_batched(const int n_max,
    const int blocks_per_replica, const int* __restrict__ d_n, const Entry<Pt>* __restrict__ sorted_all,
    const float4* __restrict__ sorted_v_all, const int* __restrict__ cube_id_all, const int* __restrict__ offs_all,
    const int gs, const int n_cubes, const float cut2, Pt* __restrict__ d_dX_all, const bool has_gen,
    const bool by_plane, const int pass_facts)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    if (w.block * bits::BLOCK >= n) return;  // (the whole workgroup: blocks past n[r] return at once)
    const size_t base = (size_t)w.replica * n_max;
    // (tiles in storage order: which workgroup serves which tile changes no result)
    grid_force_bits_tile<Pt, pw_int, pw_friction, STAGE_V, false, OFF32>(n, w.block, (int)base, -1, 0, sorted_all + base,
        sorted_v_all + base, cube_id_all + base, offs_all + (size_t)w.replica * (n_cubes + 1), gs, n_cubes, cut2,
        d_dX_all + base, has_gen, n, nullptr, nullptr, nullptr, nullptr, by_plane, pass_facts);
}

// ya::grid_force_coop for every replica at once: a 256-thread workgroup owns 256 / LANES sorted slots of ONE
// replica (ya::grid_force_coop_cells).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES>
__global__ __launch_bounds__(coop::BLOCK) void grid_force_coop_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const Entry<Pt>* __restrict__ sorted_all, const float4* __restrict__ sorted_v_all,
    const int* __restrict__ cube_id_all, const int* __restrict__ offs_all, const int gs, const int n_cubes,
    const float cut2, Pt* __restrict__ d_dX_all, const bool has_gen, const bool by_plane)
{
    constexpr int CELLS = coop::BLOCK / LANES;
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    if (w.block * CELLS >= n) return;  // (the whole workgroup)
    const size_t base = (size_t)w.replica * n_max;
    grid_force_coop_cells<Pt, pw_int, pw_friction, LANES>(n, w.block, (n + CELLS - 1) / CELLS, (int)base,
        sorted_all + base, sorted_v_all + base, cube_id_all + base, offs_all + (size_t)w.replica * (n_cubes + 1), gs,
        n_cubes, cut2, d_dX_all + base, has_gen, n, nullptr, nullptr, by_plane);
}

// Lanes per cell of the grid force launch when the model leaves the choice to the engine and its functors are
// stateless, from the size of the WHOLE launch: ya::coop::lanes_for's thresholds are where one launch of that
// many cells stops filling the chip with fewer lanes, and an ensemble's launch of n_replicas * n_max cells is
// such a launch.
// THE THRESHOLDS ARE PLACEHOLDERS (the single system's, measured for ONE system of that many cells:
// solvers.cuh, ya::coop::lanes_for) until profiles/ensemble_grid_bench.json exists.
inline int grid_lanes_for(const int n_replicas, const int n_max)
{
    const size_t cells = (size_t)n_replicas * (size_t)n_max;
    return cells > 120000 ? 1 : coop::lanes_for((int)cells);
}

// ---- whole Heun steps of a replica from LDS (Ensemble<Pt, Grid_solver>::take_steps, lds_steps) ---------------------
// A replica that fits one workgroup's LDS needs no counters: the workgroup sorts the replica's (cube, id) keys in
// LDS, which IS the order count + scan + scatter + grid_order_batched produce (cubes ascending, ids ascending inside
// a cube), and offs[k] -- the number of cells in cubes below k -- is a binary search of that order.  Nothing of size
// grid_size^3 is touched between the launch's first load and its last stores.
//
// THE LDS RULE is ya::ens::lds_layout<Pt, true, LINKED> (ensemble.cuh): the step's own arrays, then ONE 64-bit key per
// row: cube id in the high word, local id in the low word; the array is laid out for grid_lds_key_rows(n_max), n_max
// rounded up to a power of two, which the bitonic sort needs.  With ordered links the replica's incidence list lies
// right behind the keys; the term buffer of several lanes per cell (grid_lds_walk_coop below) behind all that.
// The largest n_max whose launch fits one workgroup, ya::fixed_velocity_from_partials' static fold scratch included;
// at most WHOLE_STEP_MAX_ROWS (1024 for every point type up to 8 floats: an 8-float point's 1024 rows leave 896 bytes).
template<typename Pt>
constexpr int grid_lds_capacity()
{
    int rows = 0;
    for (int n = 1; n <= WHOLE_STEP_MAX_ROWS; n++)
        if (lds_layout<Pt, true, false>(n, 0, 1).bytes + WHOLE_STEP_STATIC_LDS <= LDS_PER_WORKGROUP) rows = n;  // (the rule never falls)
    return rows;
}

// The replica's cube ids (ya::cube_id_of, clamped as grid_count_batched clamps it) and THE ORDER: sh_key[0 .. n)
// ascending in (cube, id), by a bitonic sort of P = the power of two from n up keys (the padding sorts last).  Every
// thread calls it; its barriers are log2(P) (log2(P) + 1) / 2 + 1, a function of n.  Returns whether one of THIS
// thread's cells lay outside the grid.
template<typename Pt>
__device__ __forceinline__ bool grid_lds_order(const int n, const Pt* sh_in, const float cs, const int gs,
    const int n_cubes, unsigned long long* sh_key)
{
    int P = 1;
    while (P < n) P <<= 1;
    bool outside = false;
    // (the walk of the stage before has read the keys: the step's barriers lie in between)
    for (int local = threadIdx.x; local < P; local += UPDATE_BLOCK) {
        unsigned long long key = ~0ull;
        if (local < n) {
            const Pt p = sh_in[local];
            int id = cube_id_of(p.x, p.y, p.z, cs, gs);
            if (id < 0 || id >= n_cubes) {
                outside = true;
                id = id < 0 ? 0 : n_cubes - 1;
            }
            key = ((unsigned long long)(unsigned)id << 32) | (unsigned)local;
        }
        sh_key[local] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            // thread t's pair(s): a = the t-th index with bit j clear, its partner a + j; ascending where (a & k) == 0
            for (int t = threadIdx.x; t < (P >> 1); t += UPDATE_BLOCK) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const unsigned long long lo = sh_key[a], hi = sh_key[a + j];
                if ((lo > hi) == ((a & k) == 0)) {
                    sh_key[a] = hi;
                    sh_key[a + j] = lo;
                }
            }
            __syncthreads();
        }
    }
    return outside;
}

// offs[k] of the order: the number of cells whose cube is below k (the first slot of cube k), k in [0, n_cubes].
__device__ __forceinline__ int grid_lds_lower_bound(const unsigned long long* sh_key, const int n, const int k)
{
    const unsigned long long first = (unsigned long long)(unsigned)k << 32;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sh_key[mid] < first)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// build + grid_force_bits_batched for the replica in LDS: ONE thread per cell (the contract of `d_mes_nbs[i] += 1`;
// thread t owns sorted slots t, t + 256, ...: a wavefront's lanes walk similar rows).  A cell in cube c walks the
// stencil rows 0 .. 8 in ya::stencil_row_offset order, per row the slots [offs[clamp(c + off - 1)],
// offs[clamp(c + off + 2)]) ascending, clamp(k) = min(max(k, 0), n_cubes) as in YA_ROW_BOUNDS; a candidate counts iff
// dist2 < cut2, i == j included; a hit runs bits::pass' pair statements (the functors are inlined into kernels of
// different shapes there and here, so the statements are written again rather than shared), the neighbour's old_v
// from sh_v, ids ensemble-global.  by_plane: rows 0 - 2 and rows 3 - 8 each summed from +0, then added
// (grid_force_bits_tile's whole-tile arithmetic).  No barrier in here.
// HAS_GEN: the right-hand sides hold a start the forces are added to (the ordered link forces, ensemble_links.cuh),
// written by the thread that owns the ROW, not the slot: the caller's barrier lies in between (grid_lds_order's).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool HAS_GEN = false>
__device__ __forceinline__ void grid_lds_walk(const int n, const int id_base, const Pt* sh_in, const float3* sh_v,
    Pt* sh_rhs, const unsigned long long* sh_key, const int gs, const int n_cubes, const float cut2, const bool by_plane)
{
    constexpr int NF = N_floats<Pt>::value;
    constexpr int NC = NF + 4;
    for (int s = threadIdx.x; s < n; s += UPDATE_BLOCK) {
        const unsigned long long mine = sh_key[s];
        const int c = (int)(mine >> 32), local = (int)(unsigned)mine;
        const int i = id_base + local;
        const Pt Xi = sh_in[local];
        Pt F = ya::zero<Pt>();
        float3 sum_v{0.f, 0.f, 0.f};
        float sum_friction = 0;
        float own[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) own[k] = 0.f;
#pragma unroll 1
        for (int row = 0; row < 9; row++) {
            if (by_plane && row == 3) {  // the own plane's sums aside, the other two planes from +0
#pragma unroll
                for (int k = 0; k < NF; k++) own[k] = field(F, k);
                own[NF] = sum_v.x, own[NF + 1] = sum_v.y, own[NF + 2] = sum_v.z, own[NF + 3] = sum_friction;
                F = ya::zero<Pt>(), sum_v = float3{0.f, 0.f, 0.f}, sum_friction = 0;
            }
            const int off = stencil_row_offset(row, gs);
            const int begin = grid_lds_lower_bound(sh_key, n, min(max(c + off - 1, 0), n_cubes));
            const int end = grid_lds_lower_bound(sh_key, n, min(max(c + off + 2, 0), n_cubes));
            for (int t = begin; t < end; t++) {
                const int other = (int)(unsigned)sh_key[t];
                const Pt Xj = sh_in[other];
                if (dist2(Xi, Xj) < cut2) {
                    const float3 vj = sh_v[other];
                    const float4 v{vj.x, vj.y, vj.z, 0.f};
                    Pt r = Xi - Xj;
                    float dist = dist3(r.x, r.y, r.z);
                    const int j = id_base + other;
                    YA_CALL_INLINED F += pw_int(Xi, r, dist, i, j);
                    pair_friction<Pt, pw_friction>(Xi, r, dist, i, j, v, sum_v, sum_friction);
                }
            }
        }
        if (by_plane) {  // S[dz = 0] + S[dz = -1, +1]
#pragma unroll
            for (int k = 0; k < NF; k++) field(F, k) = own[k] + field(F, k);
            sum_v.x = own[NF] + sum_v.x, sum_v.y = own[NF + 1] + sum_v.y, sum_v.z = own[NF + 2] + sum_v.z;
            sum_friction = own[NF + 3] + sum_friction;
        }
        store_rhs(sh_rhs, local, HAS_GEN, F, sum_v, sum_friction);
    }
}

// A cell's lanes meet in the term buffer without a workgroup barrier: LANES <= 64 lanes of consecutive threads lie in
// ONE wavefront, whose LDS accesses complete in program order; the fences keep the compiler from moving an access
// across the point where another lane's access is meant to lie.
__device__ __forceinline__ void grid_lds_lanes_meet()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One candidate's NF + 4 terms {F (NF), friction, friction * old_v (3)}, handed to store(c, term): grid_lds_walk's
// pair statements with each `sum += term` left to phase (b).  The default friction's coefficient is 0 or 1, so its
// products are exact and `sum + f * v` is ya::pair_friction's `fmaf(f, v, sum)`, bit for bit, a non-finite old_v
// included; any other friction adds its old_v terms only where it is not zero, as pair_friction does: a +0 term there
// (see grid_lds_walk_coop on +0 terms).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Store>
__device__ __forceinline__ void grid_lds_pair_terms(const Pt Xi, const Pt Xj, const float3 vj, const int i, const int j,
    const Store& store)
{
    constexpr int NF = N_floats<Pt>::value;
    Pt r = Xi - Xj;
    float dist = dist3(r.x, r.y, r.z);
    Pt f = ya::zero<Pt>();
    YA_CALL_INLINED f = pw_int(Xi, r, dist, i, j);
#pragma unroll
    for (int c = 0; c < NF; c++) store(c, field(f, c));
    if constexpr (pw_friction == &friction_w_neighbour<Pt>) {
        const bool nb = (i != j) & (dist < 1.f);
        const float friction = nb ? 1.f : 0.f;
        store(NF, friction);
        store(NF + 1, friction * vj.x);
        store(NF + 2, friction * vj.y);
        store(NF + 3, friction * vj.z);
    } else {
        const float friction = pw_friction(Xi, r, dist, i, j);
        store(NF, friction);
        store(NF + 1, friction != 0 ? friction * vj.x : 0.f);
        store(NF + 2, friction != 0 ? friction * vj.y : 0.f);
        store(NF + 3, friction != 0 ? friction * vj.z : 0.f);
    }
}

// Phase (b) of grid_lds_walk_coop: sum + terms[0] + terms[1] + ... + terms[n_terms - 1], added one after the other in
// that order, for ONE component of a cell's term buffer: `column` is the component's float4 of the first group of four
// candidates, the next group's lies STRIDE float4 further.  Sixteen terms per trip: four 16-byte LDS reads in flight,
// then the adds in order.
template<int STRIDE>
__device__ __forceinline__ float grid_lds_ordered_sum(float sum, const float4* column, const int n_terms)
{
    int g = 0;
    for (; 4 * (g + 4) <= n_terms; g += 4) {
        float4 p[4];
#pragma unroll
        for (int u = 0; u < 4; u++) p[u] = column[(g + u) * STRIDE];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            sum += p[u].x;
            sum += p[u].y;
            sum += p[u].z;
            sum += p[u].w;
        }
    }
    for (; 4 * (g + 1) <= n_terms; g++) {
        const float4 p = column[g * STRIDE];
        sum += p.x;
        sum += p.y;
        sum += p.z;
        sum += p.w;
    }
    const int rest = n_terms - 4 * g;  // (the group is laid out whole: the tile length is a multiple of 4)
    if (rest > 0) {
        const float4 p = column[g * STRIDE];
        sum += p.x;
        if (rest > 1) sum += p.y;
        if (rest > 2) sum += p.z;
    }
    return sum;
}

// grid_lds_walk for functors that keep no per-cell state: LANES (4, 16 or 64) lanes per cell, the same bits.  The
// workgroup serves 256 / LANES sorted slots per round, ceil(n / cells) rounds.  Per round:
//   bounds   the cell's 18 row bounds are dealt to its lanes (search q = row + 9 * (is it the end) goes to lane
//            q % LANES: with 16 or 64 lanes they are one parallel step) and handed round by wavefront shuffles; every
//            lane then holds, per row, its first slot and the number of candidates in the rows before it.  THE WALK'S
//            ORDER is the candidates numbered q = 0 .. T - 1 through rows 0 .. 8 ascending, slots ascending in a row.
//   (a)      per tile of `tile` candidates (the term buffer: sh_part, [cell][group of four candidates][component][4],
//            so that no address depends on the tile length and a component's four terms are one 16-byte read), lane l
//            evaluates candidates l, l + LANES, ... of the tile: key -> position -> test, and for a hit (dist2 < cut2,
//            i == j included, ids ensemble-global, old_v from sh_v) the pair's terms by grid_lds_pair_terms.
//            A MISS IS RECORDED AS +0 IN EVERY COMPONENT, not compacted away: every running sum of (b) starts at +0
//            and receives IEEE round-to-nearest additions only, and x + y is -0 only where x and y both are, so a
//            running sum never is -0 and adding +0 to it changes no bit (tile_force_coop's argument for its masked
//            friction products).
//   (b)      one lane per component (components lane, lane + LANES, ...) adds the tile's terms in ascending q to a
//            sum that started at +0 and is carried across tiles: no bit depends on `tile`.
// by_plane: candidates [0, cum[3]) -- rows 0 - 2 -- and the rest are two such walks, each summed from +0, then added
// as own + rest (grid_lds_walk's arithmetic, empty parts included).
// Then the sums travel to the cell's first lane by shuffles, and it writes the right-hand side (HAS_GEN: adds to what
// the row's owner left there; the caller's barrier -- grid_lds_order's -- lies in between).
// NO WORKGROUP BARRIER IN HERE: a cell's lanes lie in one wavefront (grid_lds_lanes_meet), so the trip counts of a
// cell's tiles concern that cell's lanes alone, a cube of 300 cells beside isolated ones included.  Every thread calls
// it; the caller's barrier follows.  No atomics, no cooperative launch; the bounds and the running sums live in
// registers indexed by unrolled loops (no scratch).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES, bool HAS_GEN = false>
__device__ __forceinline__ void grid_lds_walk_coop(const int n, const int id_base, const Pt* sh_in, const float3* sh_v,
    Pt* sh_rhs, const unsigned long long* sh_key, const int gs, const int n_cubes, const float cut2, const bool by_plane,
    float* sh_part, const int tile)
{
    static_assert(LANES == 4 || LANES == 16 || LANES == 64, "4, 16 or 64 lanes per cell");
    constexpr int CELLS = UPDATE_BLOCK / LANES;
    constexpr int NF = N_floats<Pt>::value;
    constexpr int NC = NF + 4;
    constexpr int SLOTS = (NC + LANES - 1) / LANES;   // components per lane
    constexpr int SEARCHES = (18 + LANES - 1) / LANES;  // bounds per lane
    const int cell = threadIdx.x / LANES, lane = threadIdx.x % LANES;
    float* const my_terms = sh_part + (size_t)cell * NC * tile;  // this cell's [group][component][4] terms
    for (int first = 0; first < n; first += CELLS) {
        const int s = first + cell;
        const bool active = s < n;
        // (the lanes of a cell past n search too, for the replica's last slot: every lane takes part in the shuffles)
        const unsigned long long mine = sh_key[active ? s : n - 1];
        const int c = (int)(mine >> 32), local = (int)(unsigned)mine;
        const int i = id_base + local;
        int bound[SEARCHES];
#pragma unroll
        for (int a = 0; a < SEARCHES; a++) {
            const int q = lane + LANES * a;
            bound[a] = 0;
            if (q < 18) {
                const int off = stencil_row_offset(q < 9 ? q : q - 9, gs);
                bound[a] = grid_lds_lower_bound(sh_key, n, min(max(c + off + (q < 9 ? -1 : 2), 0), n_cubes));
            }
        }
        // candidate q of row `row` is slot q + shift[row], cum[row] <= q < cum[row + 1]
        int shift[9], cum[10];
        cum[0] = 0;
#pragma unroll
        for (int row = 0; row < 9; row++) {
            const int begin = __shfl(bound[row / LANES], row % LANES, LANES);
            const int end = __shfl(bound[(9 + row) / LANES], (9 + row) % LANES, LANES);
            shift[row] = begin - cum[row];
            cum[row + 1] = cum[row] + (end - begin);
        }
        float acc[SLOTS], own[SLOTS];
#pragma unroll
        for (int a = 0; a < SLOTS; a++) acc[a] = own[a] = 0.f;
        if (active) {
            const Pt Xi = sh_in[local];
            const int split = by_plane ? cum[3] : 0;
#pragma unroll 1
            for (int part = 0; part < 2; part++) {
                const int q_begin = part == 0 ? 0 : split, q_end = part == 0 ? split : cum[9];
#pragma unroll 1
                for (int tile_start = q_begin; tile_start < q_end; tile_start += tile) {
                    const int n_tile = min(tile, q_end - tile_start);
                    grid_lds_lanes_meet();  // (the term buffer's readers of the tile before are done)
#pragma unroll 1
                    for (int jj = lane; jj < n_tile; jj += LANES) {
                        const int q = tile_start + jj;
                        int t = q + shift[0];
#pragma unroll
                        for (int row = 1; row < 9; row++) t = q >= cum[row] ? q + shift[row] : t;
                        const int other = (int)(unsigned)sh_key[t];
                        const Pt Xj = sh_in[other];
                        float* const mine_of_the_group = my_terms + (jj >> 2) * (4 * NC) + (jj & 3);
                        if (dist2(Xi, Xj) < cut2) {
                            grid_lds_pair_terms<Pt, pw_int, pw_friction>(Xi, Xj, sh_v[other], i, id_base + other,
                                [&](const int k, const float term) { mine_of_the_group[4 * k] = term; });
                        } else {
#pragma unroll
                            for (int k = 0; k < NC; k++) mine_of_the_group[4 * k] = 0.f;
                        }
                    }
                    grid_lds_lanes_meet();
#pragma unroll
                    for (int a = 0; a < SLOTS; a++) {
                        const int k = lane + LANES * a;
                        if (k < NC)
                            acc[a] = grid_lds_ordered_sum<NC>(
                                acc[a], reinterpret_cast<const float4*>(my_terms) + k, n_tile);
                    }
                }
                if (part == 0 && by_plane) {  // the own plane's sums aside, the other two planes from +0
#pragma unroll
                    for (int a = 0; a < SLOTS; a++) own[a] = acc[a], acc[a] = 0.f;
                }
            }
            if (by_plane) {  // S[dz = 0] + S[dz = -1, +1]
#pragma unroll
                for (int a = 0; a < SLOTS; a++) acc[a] = own[a] + acc[a];
            }
        }
        // component k is with lane k % LANES; every lane of the wavefront takes part
        float sum[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) sum[k] = __shfl(acc[k / LANES], k % LANES, LANES);
        if (active && lane == 0) {
            Pt F;
#pragma unroll
            for (int k = 0; k < NF; k++) field(F, k) = sum[k];
            store_rhs(sh_rhs, local, HAS_GEN, F, float3{sum[NF + 1], sum[NF + 2], sum[NF + 3]}, sum[NF]);
        }
    }
}

// n_steps Heun steps of replica blockIdx.x by ONE 256-thread workgroup, from LDS (dynamic LDS of
// lds_layout<Pt, true, LINKED>(n_max, slots, LANES).bytes): ya::ens::whole_steps_in_lds (ensemble.cuh) with a stage's forces = grid_lds_order +
// grid_lds_walk of the stage's positions.  Bit for bit n_steps of the 14-launch take_step without generic forces.
// Global memory: d_n[r] is read once; rows [0, n_r) of d_X and d_old_v are read at the start and written at the end;
// at the end the grid arrays of the LAST stage's order, as the 14-launch path leaves them -- d_cube_id and d_point_id
// for slots < n_r, all n_cubes + 1 of the replica's d_offs (threads stride over the cubes and search the order) -- and
// YA_STATUS_OUT_OF_GRID in d_status[r] if a cell of any stage lay outside the grid (one atomic).  A replica with
// n_r <= 0 gets the empty grid (offs all 0) and nothing else.  Nothing else is written: not the unused rows, not
// d_n, not the right-hand-side arrays, not the build's private arrays (d_count stays zeroed for the next take_step).
// Every barrier is reached by all 256 threads; the trip counts around them depend on n_r and n_steps only (LINKED:
// and on the replica's slots in use, which every thread reads alike).
// LINKED (grid_lds_steps_linked below): once per launch the workgroup builds the replica's incidence list behind the
// keys (whole_links_build, its scan scratch the fold's, as in whole_steps_of_a_replica); every stage starts with the
// ordered link forces of its positions as the right-hand sides (whole_stage_links), the order's barriers follow, and
// the walk adds the stage's forces to them.  Links do not change during a launch.
// LANES (4, 16 or 64; Ensemble<Pt, Grid_solver>::lds_step_lanes): the walk is grid_lds_walk_coop, its term buffer
// behind all that, the tile length the layout's, read from the same constexpr function as the host's.  LANES == 1 is
// the one-lane code as it was.  (lanes_per_cell, the 14-launch step's knob, plays no part.)
// Not here: the fast tier, graph capture (the Gabriel form's launch is ya::ens::gabriel_lds_steps, ensemble_gabriel.cuh).
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool LINKED, int LANES = 1>
__device__ __forceinline__ void grid_lds_steps_of_a_replica(const int n_max, const int* __restrict__ d_n,
    const float dt, const float* __restrict__ d_dt, const int n_steps, const int kind1, const int kind2, const int fix_point, Pt* __restrict__ d_X_all,
    float3* __restrict__ d_old_v_all, const float cs, const int gs, const int n_cubes, const float cut2,
    const bool by_plane, int* __restrict__ d_cube_id_all, int* __restrict__ d_point_id_all, int* __restrict__ d_offs_all,
    int* __restrict__ d_status, const Links_view links = Links_view{})
{
    extern __shared__ __attribute__((aligned(16))) unsigned char grid_step_lds[];
    const int replica = blockIdx.x;
    const int n = count_of(d_n, replica, n_max);
    int* __restrict__ d_offs = d_offs_all + (size_t)replica * (n_cubes + 1);
    if (n <= 0) {  // (the whole workgroup)
        for (int c = threadIdx.x; c <= n_cubes; c += UPDATE_BLOCK) d_offs[c] = 0;
        return;
    }
    const Lds_layout layout = lds_layout<Pt, true, LINKED>(n_max, links.slots_per_replica, LANES);
    unsigned long long* const sh_key = reinterpret_cast<unsigned long long*>(grid_step_lds + layout.keys);
    int* const sh_off = reinterpret_cast<int*>(grid_step_lds + layout.list);   // LINKED: n_max + 1 offsets,
    unsigned* const sh_ent = reinterpret_cast<unsigned*>(sh_off + n_max + 1);  // at most 2 slots_per_replica entries
    if constexpr (LINKED)  // (its scratch is the fold's)
        whole_links_build(links, replica, n, n_max, sh_off, sh_ent, lds_fold_scratch<Pt>(grid_step_lds, n_max));
    float* const sh_part = reinterpret_cast<float*>(grid_step_lds + layout.terms);  // (used with several lanes per cell)
    const int tile = layout.tile;
    const int id_base = replica * n_max;
    bool outside = false;
    const float dt_r = value_of(d_dt, dt, replica);  // (d_dt[r] where the call has a time step per replica)
    whole_steps_in_lds<Pt>(n_max, n, replica, dt_r, n_steps, kind1, kind2, fix_point, d_X_all, d_old_v_all, grid_step_lds,
        [&](const Pt* sh_in, const float3* sh_v, Pt* sh_rhs) __attribute__((always_inline)) {
            if constexpr (LINKED) whole_stage_links<Pt>(n, sh_in, sh_rhs, sh_off, sh_ent, links.strength);
            outside |= grid_lds_order<Pt>(n, sh_in, cs, gs, n_cubes, sh_key);
            if constexpr (LANES == 1)
                grid_lds_walk<Pt, pw_int, pw_friction, LINKED>(
                    n, id_base, sh_in, sh_v, sh_rhs, sh_key, gs, n_cubes, cut2, by_plane);
            else
                grid_lds_walk_coop<Pt, pw_int, pw_friction, LANES, LINKED>(
                    n, id_base, sh_in, sh_v, sh_rhs, sh_key, gs, n_cubes, cut2, by_plane, sh_part, tile);
        });
    // (the keys are the last stage's: its walk was followed by barriers, and nothing has written them since)
    const size_t base = (size_t)replica * n_max;
    for (int s = threadIdx.x; s < n; s += UPDATE_BLOCK) {
        const unsigned long long key = sh_key[s];
        d_cube_id_all[base + s] = (int)(key >> 32);
        d_point_id_all[base + s] = (int)(unsigned)key;
    }
    for (int c = threadIdx.x; c <= n_cubes; c += UPDATE_BLOCK) d_offs[c] = grid_lds_lower_bound(sh_key, n, c);
    // The threads' flags meet in the fold's scratch, which nothing uses after the last step.  (__syncthreads_or would cost
    // 256 bytes of static LDS beyond WHOLE_STEP_STATIC_LDS, and the rule may leave none: a list or a term buffer that
    // lds_layout admits, or the rows alone -- a 9-float point's 918 rows and keys leave 8 bytes, an 11-float point's
    // 750 leave 136 -- so no kernel here uses it.)
    int* sh_flag = lds_fold_scratch<Pt>(grid_step_lds, n_max);
    if (threadIdx.x == 0) *sh_flag = 0;
    __syncthreads();
    if (outside) *sh_flag = 1;  // (every writer writes the same value)
    __syncthreads();
    if (threadIdx.x == 0 && *sh_flag) atomicOr(d_status + replica, YA_STATUS_OUT_OF_GRID);
}
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES = 1>
__global__ __launch_bounds__(UPDATE_BLOCK) void grid_lds_steps(const int n_max, const int* __restrict__ d_n,
    const float dt, const float* __restrict__ d_dt, const int n_steps, const int kind1, const int kind2,
    const int fix_point, Pt* __restrict__ d_X_all, float3* __restrict__ d_old_v_all, const float cs, const int gs, const int n_cubes, const float cut2,
    const bool by_plane, int* __restrict__ d_cube_id_all, int* __restrict__ d_point_id_all, int* __restrict__ d_offs_all,
    int* __restrict__ d_status)
{
    grid_lds_steps_of_a_replica<Pt, pw_int, pw_friction, false, LANES>(n_max, d_n, dt, d_dt, n_steps, kind1, kind2, fix_point,
        d_X_all, d_old_v_all, cs, gs, n_cubes, cut2, by_plane, d_cube_id_all, d_point_id_all, d_offs_all, d_status);
}
// The same steps with the ordered link forces of `links` (ensemble_links.cuh) at the start of every stage: bit for
// bit n_steps of the 14-launch take_step with ya::ens::link_forces_ordered as its generic force.  Dynamic LDS of
// lds_layout<Pt, true, true>(n_max, links.slots_per_replica, LANES).bytes > 0.  Besides what grid_lds_steps reads, the
// replica's slots of links.d_link and *links.d_n are read, at the start of the launch; what it writes is what grid_lds_steps
// writes.  No atomics but the status bit, no scratch, no cooperative launch.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES = 1>
__global__ __launch_bounds__(UPDATE_BLOCK) void grid_lds_steps_linked(const int n_max, const int* __restrict__ d_n,
    const float dt, const float* __restrict__ d_dt, const int n_steps, const int kind1, const int kind2,
    const int fix_point, Pt* __restrict__ d_X_all, float3* __restrict__ d_old_v_all, const float cs, const int gs, const int n_cubes, const float cut2,
    const bool by_plane, int* __restrict__ d_cube_id_all, int* __restrict__ d_point_id_all, int* __restrict__ d_offs_all,
    int* __restrict__ d_status, const Links_view links)
{
    grid_lds_steps_of_a_replica<Pt, pw_int, pw_friction, true, LANES>(n_max, d_n, dt, d_dt, n_steps, kind1, kind2, fix_point,
        d_X_all, d_old_v_all, cs, gs, n_cubes, cut2, by_plane, d_cube_id_all, d_point_id_all, d_offs_all, d_status,
        links);
}

// Whether these launches beat the 14-launch step when the model leaves the choice to the engine
// (Ensemble<Pt, Grid_solver>::lds_steps == 0).  THIS RULE IS A PLACEHOLDER until measured
// (profiles/ensemble_grid_lds_steps_bench.json, tools/ensemble_bench.py --solver grid --lds-steps): one workgroup per
// CU; below that the 14-launch path spreads a replica over more CUs.  (the two shapes probed so far lose.)
inline bool lds_steps_pay(const int n_replicas, const int n_max, const int n_cubes)
{
    return n_replicas >= 256;
}

// Lanes per cell inside these launches when the model leaves the choice to the engine and its functors are stateless
// (Ensemble<Pt, Grid_solver>::lds_step_lanes == 0).  The derivation is ya::ens::whole_step_lanes_for's -- the largest L
// of 64, 16, 4 with n_max * L <= 256, else 1: one round serves the whole replica, a lane evaluates ceil(T / L) of a
// cell's T candidates and runs at most ceil(18 / L) of its searches, and the ordered adds are what they were -- and
// THE TABLE CORRECTS IT TWICE (profiles/ensemble_grid_lds_lanes_bench.json, MI355X, relu, M = 1 .. 4096; DESIGN.md
// section 4): at n = 32 two rounds of 16 lanes beat one round of 4 (1.09 - 1.23 x at every M), and at n = 4 16 lanes are
// as fast as 64 or up to 6 % faster (beyond 16 lanes the 18 searches gain nothing and 7 components leave 57 lanes idle
// in phase (b)).  So: 16 lanes up to 32 cells, 4 up to 64 (measured at 64: 4 lanes 1.6 - 2.8 x one lane, 16 lanes less),
// else 1.  Every L > 1 it answers was at least 1.6 x one lane at every measured M, spreads <= 0.13.
// ABOVE 64 CELLS THE ANSWER (1) IS A PLACEHOLDER: at n = 100 4 lanes are 1.5 x one lane up to M = 256 and 0.82 x from
// M = 1024 on, at n >= 256 every L > 1 loses; a rule there needs n_replicas, which this one does not take.
constexpr int grid_lds_lanes_for(const int n_max)
{
    if (n_max <= 32) return 16;
    if (n_max <= 64) return 4;
    return 1;
}


// What the ensembles of the grid-based solvers share (CRTP, between Stepper and Ensemble<Pt, Grid_solver> /
// Ensemble<Pt, Gabriel_solver>): the per-replica grid arrays of this file's header, their build in four launches,
// the status bits.  Form is the Ensemble itself; it supplies Stepper's forces of a stage, which start with build().
template<typename Pt, typename Form>
class Grid_form : public Stepper<Pt, Form> {
    using Base = Stepper<Pt, Form>;

public:
    const int grid_size, n_cubes;
    float cube_size;  // of every replica; may be changed between steps
    // The reference's Grid arrays, per replica (this file's header): [rows()], [rows()], [n_replicas * (n_cubes + 1)]
    int *d_cube_id, *d_point_id, *d_offs;
    int* d_status;  // [n_replicas] sticky YA_STATUS_OUT_OF_GRID bits, never read by the step

    Grid_form(const char* solver, int n_replicas, int n_max, int grid_size, float cube_size)
        : Base{checked(solver, n_replicas, n_max, grid_size), n_max}, grid_size{grid_size},
          n_cubes{grid_size * grid_size * grid_size}, cube_size{cube_size}
    {
        const size_t total = this->rows();
        YA_CHECK(ya_malloc((void**)&d_cube_id, total * sizeof(int)));
        YA_CHECK(ya_malloc((void**)&d_point_id, total * sizeof(int)));
        YA_CHECK(ya_malloc((void**)&d_cube_of, total * sizeof(int)));
        YA_CHECK(ya_malloc((void**)&d_rank, total * sizeof(int)));
        YA_CHECK(ya_malloc((void**)&d_arrival, total * sizeof(int)));
        YA_CHECK(ya_malloc((void**)&d_sorted, total * sizeof(ya::Entry<Pt>)));
        YA_CHECK(ya_malloc((void**)&d_sorted_v, total * sizeof(float4)));
        const size_t counters = (size_t)n_replicas * n_cubes * sizeof(int);
        YA_CHECK(ya_malloc((void**)&d_count, counters));
        YA_CHECK(ya_memset_async(d_count, 0, counters, nullptr));
        // (a replica that was never built holds -1 where its count would be: offs_built())
        const size_t offsets = (size_t)n_replicas * (n_cubes + 1) * sizeof(int);
        YA_CHECK(ya_malloc((void**)&d_offs, offsets));
        YA_CHECK(ya_memset_async(d_offs, 0xff, offsets, nullptr));
        YA_CHECK(ya_malloc((void**)&d_status, (size_t)n_replicas * sizeof(int)));
        YA_CHECK(ya_memset_async(d_status, 0, (size_t)n_replicas * sizeof(int), nullptr));
    }
    ~Grid_form()
    {
        ya_free(d_cube_id);
        ya_free(d_point_id);
        ya_free(d_cube_of);
        ya_free(d_rank);
        ya_free(d_arrival);
        ya_free(d_sorted);
        ya_free(d_sorted_v);
        ya_free(d_count);
        ya_free(d_offs);
        ya_free(d_status);
    }

    // What the constructor refuses, before anything touches the device (the harness asks first and returns -3).
    static bool sizes_ok(int n_replicas, int n_max, int grid_size)
    {
        if (n_replicas <= 0 || n_max <= 0 || grid_size < 1 || grid_size > YA_MAX_GRID_SIZE) return false;
        const size_t n_cubes = (size_t)grid_size * grid_size * grid_size;
        return (size_t)n_replicas * (size_t)n_max <= (size_t)0x7fffffff &&
               (size_t)n_replicas * (n_cubes + 1) <= (size_t)0x7fffffff;
    }

    // Replica r's status bits (YA_STATUS_OUT_OF_GRID), read without aborting; clear = forget them.
    int status(int r, bool clear = true)
    {
        assert(r >= 0 && r < this->n_replicas);
        int bits = 0;
        YA_CHECK(ya_memcpy_d2h(&bits, d_status + r, sizeof(int)));
        if (bits && clear) YA_CHECK(ya_memset_async(d_status + r, 0, sizeof(int), nullptr));
        return bits;
    }
    void check_status()
    {
        std::vector<int> bits(this->n_replicas);
        YA_CHECK(ya_memcpy_d2h(bits.data(), d_status, bits.size() * sizeof(int)));
        for (int r = 0; r < this->n_replicas; r++) {
            if (bits[r] & YA_STATUS_OUT_OF_GRID) {
                fprintf(stderr,
                    "yalla-hip: a cell of replica %d left the %d^3 grid (device assertion at "
                    "ya||a solvers.cuh:361-362); enlarge grid_size or cube_size.\n",
                    r, grid_size);
                abort();
            }
        }
    }
    void copy_to_host()
    {
        check_status();
        Base::copy_to_host();
    }

protected:
    int *d_cube_of, *d_rank, *d_arrival, *d_count;
    ya::Entry<Pt>* d_sorted;
    float4* d_sorted_v;

    static int checked(const char* solver, int n_replicas, int n_max, int grid_size)
    {
        if (!sizes_ok(n_replicas, n_max, grid_size)) {
            fprintf(stderr,
                "yalla-hip: Ensemble<Pt, %s>{%d, %d, %d}: sizes must be positive, grid_size <= %d (cube ids "
                "are binary32), and n_replicas * n_max and n_replicas * (grid_size^3 + 1) at most 2^31 - 1 (ids, "
                "launch sizes and counter offsets are ints)\n",
                solver, n_replicas, n_max, grid_size, YA_MAX_GRID_SIZE);
            abort();
        }
        return n_replicas;
    }

    // Four launches: the grid of every replica from d_in, the cells gathered into d_sorted / d_sorted_v.
    // BUILD_EMPTY: a replica with n_r = 0 gets an empty grid (true) or keeps the arrays it has (false).
    template<bool BUILD_EMPTY = true>
    void build(const Pt* d_in)
    {
        const int n_max = this->n_max, n_replicas = this->n_replicas;
        const int* d_n = this->d_n;
        const int row_blocks = (n_max + ya::UPDATE_BLOCK - 1) / ya::UPDATE_BLOCK;
        grid_count_batched<Pt><<<this->grid_of(row_blocks), ya::UPDATE_BLOCK>>>(
            n_max, row_blocks, d_n, d_in, cube_size, grid_size, n_cubes, d_cube_of, d_rank, d_count, d_status);
        grid_scan_batched<BUILD_EMPTY><<<n_replicas, ya::UPDATE_BLOCK>>>(n_max, d_n, n_cubes, d_count, d_offs);
        grid_scatter_batched<<<this->grid_of(row_blocks), ya::UPDATE_BLOCK>>>(
            n_max, row_blocks, d_n, n_cubes, d_cube_of, d_rank, d_offs, d_arrival, d_cube_id);
        grid_order_batched<Pt><<<this->grid_of(row_blocks), ya::UPDATE_BLOCK>>>(n_max, row_blocks, d_n, n_cubes,
            d_arrival, d_cube_id, d_offs, d_in, this->d_old_v, d_point_id, d_sorted, d_sorted_v);
    }
};

}  // namespace ens
}  // namespace ya


template<typename Pt, template<typename> class Solver>
class Ensemble<Pt, Solver, std::enable_if_t<std::is_same<Solver<Pt>, Grid_solver<Pt>>::value>>
    : public ya::ens::Grid_form<Pt, Ensemble<Pt, Solver>> {
    using Base = ya::ens::Grid_form<Pt, Ensemble<Pt, Solver>>;
    friend ya::ens::Stepper<Pt, Ensemble<Pt, Solver>>;

public:
    // (grid_size, n_cubes, cube_size, d_cube_id, d_point_id, d_offs, d_status, sizes_ok, status, check_status,
    // copy_to_host: ya::ens::Grid_form)
    // 0 (default) = the engine's choice: one lane per cell (grid_force_bits_batched) unless the functors are
    // declared stateless (YA_STATELESS: one thread per cell is the contract of `d_mes_nbs[i] += 1`), then by the
    // size of the whole launch (ya::ens::grid_lanes_for); 1 = one lane per cell; 4, 8, 16 = grid_force_coop_batched.
    // Any choice gives the same bits.
    int lanes_per_cell = 0;
    Ya_sum_order sum_order = YA_SUM_REFERENCE;  // as Grid_computer::sum_order
    // the one-lane kernel keeps old_v in LDS too while the launch's n_replicas * n_max cells are at most this many
    // (Grid_computer::stage_v_max: is the launch big enough to hide the L2's latency?)
    int stage_v_max = 130000;
    int pass_facts = 1;  // the one-lane kernel: as Grid_computer::pass_facts

    // take_steps as launches that step from LDS (ya::ens::grid_lds_steps: one workgroup per replica): -1 = never,
    // 1 = whenever the call is eligible, 0 (default) = the engine's choice, eligible and
    // ya::ens::lds_steps_pay(n_replicas, n_max, n_cubes).  Eligible: n_max <= ya::ens::grid_lds_capacity<Pt>() and
    // either no generic forces, or ya::ens::Replica_links whose incidence list fits
    // (ya::ens::lds_layout<Pt, true, true>(n_max, slots_per_replica, 1).bytes != 0).  Any choice gives the same bits.
    int lds_steps = 0;
    // Such a launch runs at most this many steps (no single kernel runs unboundedly long); take_steps splits longer
    // requests.
    int lds_steps_max = 256;
    // such launches made so far (which path ran)
    long lds_step_launches = 0;
    // Lanes per cell inside such a launch: 0 (default) = the engine's choice -- one lane per cell unless the functors
    // are declared stateless (YA_STATELESS), then ya::ens::grid_lds_lanes_for(n_max); 1 = one thread per cell
    // (ya::ens::grid_lds_walk); 4, 16 or 64 = that many whatever the functor says (ya::ens::grid_lds_walk_coop: several
    // lanes call the functor for one i at once).  A replica whose LDS has no room for the terms of 16 candidates
    // (ya::ens::lds_layout's .bytes == 0) is stepped with one lane per cell, still from LDS.  Any choice gives the same bits.  No part in take_step, the 14-launch path or the Gabriel form.
    int lds_step_lanes = 0;
    // the lanes per cell of the last launch that stepped from LDS: 0 before any, 1 after that fallback
    int lds_step_lanes_used = 0;

    Ensemble(int n_replicas, int n_max, int grid_size = 50, float cube_size = 1)
        : Base{"Grid_solver", n_replicas, n_max, grid_size, cube_size}
    {
    }

    template<Pairwise_interaction<Pt> pw_int>
    void take_steps(float dt, int n_steps, Generic_forces<Pt> gen_forces = no_gen_forces<Pt>)
    {
        take_steps<pw_int, friction_w_neighbour<Pt>>(dt, n_steps, gen_forces);
    }
    // n_steps Heun steps of every replica, bit for bit n_steps calls of take_step: as launches of at most lds_steps_max
    // steps each that step from LDS where the call is eligible and lds_steps allows it, as that loop otherwise
    // (ya::ens::Stepper::steps).  After such launches the public grid arrays and d_status hold what the loop would have
    // left; d_dX / d_X1 / d_dX1 and the build's private arrays are left as they were.
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
    // (ensemble_links.cuh's contract; this file's header).  Bit for bit n_steps calls of take_step(dt, gen) where gen
    // calls ya::ens::link_forces_ordered, and that loop unless the call steps from LDS: as launches of
    // ya::ens::grid_lds_steps_linked where lds_steps allows it, n_max <= ya::ens::grid_lds_capacity<Pt>() and the
    // incidence list fits the workgroup's LDS beside the keys (ya::ens::lds_layout<Pt, true, true>(n_max,
    // slots_per_replica, 1).bytes != 0).  A launch reads the links and their count at its start: what a model's kernel
    // left there before the call is what the call sees.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_steps(float dt, int n_steps, ya::ens::Replica_links links)
    {
        this->template steps<pw_int, pw_friction>(dt, n_steps, links);
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
    // What ya::ens::Stepper's launches from LDS ask of a form: the layout has keys; the settings above; the kernels,
    // which read the tile length from the layout themselves.
    static constexpr bool lds_keys = true;
    typename ya::ens::Stepper<Pt, Ensemble<Pt, Solver>>::Lds_knobs lds_knobs()
    {
        constexpr int capacity = ya::ens::grid_lds_capacity<Pt>();
        return {capacity, lds_steps,
            ya::ens::lds_steps_pay(this->n_replicas, this->n_max, this->n_cubes), lds_steps_max, lds_step_lanes,
            ya::ens::grid_lds_lanes_for(this->n_max), &lds_step_launches, &lds_step_lanes_used};
    }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, int LANES, bool LINKED, bool REPLICA_DT>
    static auto lds_kernel()  // (REPLICA_DT: the kernel decides at run time)
    {
        if constexpr (LINKED)
            return &ya::ens::grid_lds_steps_linked<Pt, pw_int, pw_friction, LANES>;
        else
            return &ya::ens::grid_lds_steps<Pt, pw_int, pw_friction, LANES>;
    }
    template<int LANES, bool LINKED>
    auto lds_kernel_args(const ya::ens::Lds_layout&) const
    {
        return std::make_tuple(this->cube_size, this->grid_size, this->n_cubes, ya::cutoff_squared(this->cube_size),
            sum_order == YA_SUM_BY_PLANE, this->d_cube_id, this->d_point_id, this->d_offs, this->d_status);
    }

    // Five launches: the grid of every replica from d_in, then the forces.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void forces(const Pt* d_in, Pt* d_rhs, const bool has_gen)
    {
        const int n_max = this->n_max, n_replicas = this->n_replicas;
        const int* d_n = this->d_n;
        this->build(d_in);
        const int grid_size = this->grid_size, n_cubes = this->n_cubes;
        const float cut2 = ya::cutoff_squared(this->cube_size);
        const bool by_plane = sum_order == YA_SUM_BY_PLANE;
        int lanes = lanes_per_cell;
        if (lanes == 0)
            lanes = ya::stateless_pair<Pt, pw_int, pw_friction>() ? ya::ens::grid_lanes_for(n_replicas, n_max) : 1;
        const bool coop = ya::coop::with_lanes(lanes, [&](auto per_cell) {
            constexpr int CELLS = ya::coop::BLOCK / decltype(per_cell)::value;
            const int blocks = (n_max + CELLS - 1) / CELLS;
            ya::launch(ya::ens::grid_force_coop_batched<Pt, pw_int, pw_friction, decltype(per_cell)::value>,
                this->grid_of(blocks), ya::coop::BLOCK, nullptr, nullptr, nullptr, n_max, blocks, d_n, this->d_sorted,
                this->d_sorted_v, this->d_cube_id, this->d_offs, grid_size, n_cubes, cut2, d_rhs, has_gen, by_plane);
        });
        if (coop) return;
        const int blocks = (n_max + ya::bits::BLOCK - 1) / ya::bits::BLOCK;
        ya::bits::with_gather(this->rows() <= (size_t)stage_v_max, ya::bits::offsets_fit_32_bits(n_max),
            [&](auto stage_v, auto off32) {
                ya::launch(ya::ens::grid_force_bits_batched<Pt, pw_int, pw_friction, decltype(stage_v)::value,
                               decltype(off32)::value>,
                    this->grid_of(blocks), ya::bits::BLOCK, nullptr, nullptr, nullptr, n_max, blocks, d_n, this->d_sorted,
                    this->d_sorted_v, this->d_cube_id, this->d_offs, grid_size, n_cubes, cut2, d_rhs, has_gen, by_plane,
                    ya::bits::launch_facts(pass_facts, cut2));
            });
    }
};
