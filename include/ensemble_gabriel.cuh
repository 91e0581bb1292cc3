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
// Not here: a per-replica gabriel_coefficient, cube_size or dt, the fast-arithmetic tier, graph capture, the wall
// model's wall_forces (one wall node per system).
#pragma once

namespace ya {
namespace ens {

// ya::gabriel_force for every replica at once: a one-wavefront workgroup serves GABRIEL_CELLS sorted slots of ONE
// replica, GABRIEL_LANES lanes per cell, by gabriel_force's own body (ya::gabriel_force_cells).  Cube ids and
// offs are the replica's own and gabriel::collect clamps the stencil to [0, n_cubes], so no row of another
// replica is read.  A cell with more than GABRIEL_CAP candidates appends its FLAT row r * n_max + slot to the
// ensemble's one dense list.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(64) void gabriel_force_batched(const int n_max, const int blocks_per_replica,
    const int* __restrict__ d_n, const Entry<Pt>* __restrict__ sorted_all, const float4* __restrict__ sorted_v_all,
    const int* __restrict__ cube_id_all, const int* __restrict__ offs_all, const int gs, const int n_cubes,
    const float cube_size, const float gabriel_coefficient, Pt* __restrict__ d_dX_all, const bool has_gen,
    int* __restrict__ dense, int* __restrict__ n_dense)
{
    const Where w = where(blocks_per_replica);
    const int n = count_of(d_n, w.replica, n_max);
    if (w.block * GABRIEL_CELLS >= n) return;  // (the whole workgroup: blocks past n[r] return at once)
    const size_t base = (size_t)w.replica * n_max;
    gabriel_force_cells<Pt, pw_int, pw_friction>(n, w.block * GABRIEL_CELLS, (int)base, (int)base, sorted_all + base,
        sorted_v_all + base, cube_id_all + base, offs_all + (size_t)w.replica * (n_cubes + 1), gs, n_cubes, cube_size,
        gabriel_coefficient, d_dX_all + base, has_gen, dense, n_dense);
}

// ya::gabriel_force_dense for the ensemble's one list of flat rows: a grid-stride walk, one wavefront per cell
// (ya::gabriel_force_dense_cell), the replica is row / n_max, the lists hold n_max entries each.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
__global__ __launch_bounds__(64) void gabriel_force_dense_batched(const int n_max, const int* __restrict__ dense,
    const int* __restrict__ n_dense, const Entry<Pt>* __restrict__ sorted_all, const float4* __restrict__ sorted_v_all,
    const int* __restrict__ cube_id_all, const int* __restrict__ offs_all, const int gs, const int n_cubes,
    const float cube_size, const float gabriel_coefficient, Pt* __restrict__ d_dX_all, const bool has_gen,
    float* __restrict__ workspace)
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
            gabriel_coefficient, d_dX_all + base, has_gen, x, stride);
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
    const int dense_blocks;     // workgroups of the dense launch, ya::ens::gabriel_dense_blocks

    Ensemble(int n_replicas, int n_max, int grid_size = 50, float cube_size = 1, float gabriel_coefficient = 0.8)
        : Base{"Gabriel_solver", n_replicas, n_max, grid_size, cube_size}, gabriel_coefficient{gabriel_coefficient},
          dense_blocks{ya::ens::gabriel_dense_blocks(n_replicas, n_max)}
    {
        YA_CHECK(ya_malloc((void**)&d_dense, (this->rows() + 2) * sizeof(int)));
        YA_CHECK(ya_memset_async(d_dense, 0, 2 * sizeof(int), nullptr));
        const size_t floats = (size_t)dense_blocks * ya::GABRIEL_DENSE_ARRAYS * (size_t)n_max;
        YA_CHECK(ya_malloc((void**)&d_workspace, floats * sizeof(float)));
    }
    ~Ensemble()
    {
        ya_free(d_dense);
        ya_free(d_workspace);
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
            this->cube_size, gabriel_coefficient, d_rhs, has_gen, d_dense + 2, d_dense);
        ya::ens::gabriel_force_dense_batched<Pt, pw_int, pw_friction><<<dense_blocks, 64>>>(n_max, d_dense + 2, d_dense,
            this->d_sorted, this->d_sorted_v, this->d_cube_id, this->d_offs, this->grid_size, this->n_cubes,
            this->cube_size, gabriel_coefficient, d_rhs, has_gen, d_workspace);
    }
};
