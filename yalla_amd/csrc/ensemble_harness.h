// What the two ensemble harnesses (ensemble.hip, ensemble_grid.hip) share: the generic-force policies of their
// model tables.
#pragma once

namespace ens_harness {

template<typename Pt>
struct No_gen {
    static Generic_forces<Pt> gen(int, int) { return no_gen_forces<Pt>; }
    static void before_steps(int) {}
};

// The generic force of the `push_*` models (models::push: the right-hand side of cell 1 set to (1, 0, 0)) for
// an ensemble: ONE call on the flat arrays pushes cell 1 of every replica, global row r * n_max + 1.
template<typename Pt>
__global__ void push_cell_1_of_every_replica(const int n_replicas, const int n_max, Pt* d_dX)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_replicas) return;
    Pt* row = d_dX + (size_t)r * n_max + 1;
    row->x = 1;
    row->y = 0;
    row->z = 0;
}
template<typename Pt>
struct Push_gen {
    static Generic_forces<Pt> gen(int n_replicas, int n_max)
    {
        return [n_replicas, n_max](const int n, const Pt* __restrict__ d_X, Pt* d_dX) {
            if (n_max < 2 || n != n_replicas * n_max) return;
            push_cell_1_of_every_replica<Pt><<<(n_replicas + 255) / 256, 256>>>(n_replicas, n_max, d_dX);
        };
    }
    static void before_steps(int) {}
};

}  // namespace ens_harness
