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
// Not here: the fast-arithmetic tier, graph capture, a per-replica dt, cube_size or grid_size, the sorted-space
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
    const bool by_plane)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    if (w.block * bits::BLOCK >= n) return;  // (the whole workgroup: blocks past n[r] return at once)
    const size_t base = (size_t)w.replica * n_max;
    // (tiles in storage order: which workgroup serves which tile changes no result)
    grid_force_bits_tile<Pt, pw_int, pw_friction, STAGE_V, false, OFF32>(n, w.block, (int)base, -1, 0, sorted_all + base,
        sorted_v_all + base, cube_id_all + base, offs_all + (size_t)w.replica * (n_cubes + 1), gs, n_cubes, cut2,
        d_dX_all + base, has_gen, n, nullptr, nullptr, nullptr, nullptr, by_plane);
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

    Ensemble(int n_replicas, int n_max, int grid_size = 50, float cube_size = 1)
        : Base{"Grid_solver", n_replicas, n_max, grid_size, cube_size}
    {
    }

protected:
    // Five launches: the grid of every replica from d_in, then the forces.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void forces(const Pt* d_in, Pt* d_rhs, const bool has_gen)
    {
        const int n_max = this->n_max, n_replicas = this->n_replicas;
        const int* d_n = this->d_n;
        this->build(d_in);
        const int grid_size = this->grid_size, n_cubes = this->n_cubes;
        const int *d_cube_id = this->d_cube_id, *d_offs = this->d_offs;
        const ya::Entry<Pt>* d_sorted = this->d_sorted;
        const float4* d_sorted_v = this->d_sorted_v;

        const float cut2 = ya::cutoff_squared(this->cube_size);
        const bool by_plane = sum_order == YA_SUM_BY_PLANE;
        int lanes = lanes_per_cell;
        if (lanes == 0)
            lanes = ya::stateless_pair<Pt, pw_int, pw_friction>() ? ya::ens::grid_lanes_for(n_replicas, n_max) : 1;
#define YA_ENS_COOP_LAUNCH(lanes_)                                                                              \
    {                                                                                                           \
        const int blocks = (n_max + ya::coop::BLOCK / lanes_ - 1) / (ya::coop::BLOCK / lanes_);                 \
        ya::ens::grid_force_coop_batched<Pt, pw_int, pw_friction, lanes_><<<this->grid_of(blocks), ya::coop::BLOCK>>>( \
            n_max, blocks, d_n, d_sorted, d_sorted_v, d_cube_id, d_offs, grid_size, n_cubes, cut2, d_rhs, has_gen,  \
            by_plane);                                                                                          \
    }
#define YA_ENS_BITS_LAUNCH(stage_v_, off32_)                                                                    \
    ya::ens::grid_force_bits_batched<Pt, pw_int, pw_friction, stage_v_, off32_><<<this->grid_of(blocks), ya::bits::BLOCK>>>( \
        n_max, blocks, d_n, d_sorted, d_sorted_v, d_cube_id, d_offs, grid_size, n_cubes, cut2, d_rhs, has_gen, by_plane)
        if (lanes == 16) {
            YA_ENS_COOP_LAUNCH(16)
        } else if (lanes == 8) {
            YA_ENS_COOP_LAUNCH(8)
        } else if (lanes == 4) {
            YA_ENS_COOP_LAUNCH(4)
        } else {
            const int blocks = (n_max + ya::bits::BLOCK - 1) / ya::bits::BLOCK;
            if (this->rows() <= (size_t)stage_v_max) {
                YA_ENS_BITS_LAUNCH(true, true);
            } else if (ya::bits::offsets_fit_32_bits(n_max)) {
                YA_ENS_BITS_LAUNCH(false, true);
            } else {
                YA_ENS_BITS_LAUNCH(false, false);
            }
        }
#undef YA_ENS_BITS_LAUNCH
#undef YA_ENS_COOP_LAUNCH
    }
};
