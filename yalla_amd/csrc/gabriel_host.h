// Host-serial restatement of Gabriel_solver (compute_cube_gabriel and Gabriel_computer,
// solvers.cuh:505-644) and of wall_forces with xy_wall_relu_force (links.cuh:142-228), for the CPU
// build of the model harness (models_harness.inc includes it there; the HIP build has both in
// include/).  Built on that build's Grid_computer, Heun_solver and Grid, statement by statement as the
// reference writes them, in plain binary32.  (The CPU build's Makefile does not list this header as a
// dependency: a change here must touch models_harness.inc too, or clean that build.)
#pragma once

#include <vector>

// compute_cube_gabriel (solvers.cuh:509-602) for every cell, then Gabriel_computer::pwints (:620-640)
template<typename Pt>
class Gabriel_computer : public Grid_computer<Pt> {
public:
    float gabriel_coefficient;
    Gabriel_computer(
        int n_max, int grid_size = 50, float cube_size = 1, float gabriel_coefficient = 0.8)
        : Grid_computer<Pt>{n_max, grid_size, cube_size}, gabriel_coefficient{gabriel_coefficient}
    {}

protected:
    std::vector<int> neighbour_id;
    std::vector<float> neighbour_dist;
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void pwints(int n, const Pt* d_X, const float3* d_old_v, Pt* d_dX, float3* d_sum_v,
        float* d_sum_friction, int n_active = -1)
    {
        Grid& grid = this->grid;
        grid.build(n, d_X, this->cube_size);  // :637
        for (int i = 0; i < n; i++) {  // thread i owns sorted slot i
            const int id_i = grid.d_point_id[i];
            const Pt Xi = d_X[id_i];
            Pt F;
            memset(&F, 0, sizeof(Pt));
            float3 sum_v{0, 0, 0};
            float sum_friction = 0;
            // (no fixed list size: the reference's 100 entries are undefined behaviour beyond)
            neighbour_id.clear();
            neighbour_dist.clear();
            for (int jn = 0; jn < 27; jn++) {  // :531-546
                const int cube = grid.d_cube_id[i] + this->nhood[jn];
                // out-of-grid cubes are empty here, as in Grid_computer::pwints
                if (cube < 0 || cube >= grid.n_cubes) continue;
                for (int k = grid.d_cube_start[cube]; k <= grid.d_cube_end[cube]; k++) {
                    const int j = grid.d_point_id[k];
                    const Pt Xj = d_X[j];
                    const Pt r = Xi - Xj;
                    const float dist = ya_dist3(r.x, r.y, r.z);
                    if (dist >= this->cube_size) continue;
                    neighbour_id.push_back(j);
                    neighbour_dist.push_back(dist);
                }
            }
            const int n_neighs = (int)neighbour_id.size();
            for (int m = 0; m < n_neighs - 1; m++) {  // :550-566
                float min_val = neighbour_dist[m];
                int min_index = m;
                for (int q = m + 1; q < n_neighs; q++) {
                    const float compare_val = neighbour_dist[q];
                    if (compare_val < min_val) {
                        min_index = q;
                        min_val = compare_val;
                    }
                }
                if (min_index != m) {
                    const int id_temp = neighbour_id[min_index];
                    neighbour_id[min_index] = neighbour_id[m];
                    neighbour_id[m] = id_temp;
                    neighbour_dist[min_index] = neighbour_dist[m];
                    neighbour_dist[m] = min_val;
                }
            }
            for (int m = n_neighs - 1; m >= 0; m--) {  // :572-599
                bool gabriel_condition = true;
                const int j = neighbour_id[m];
                const Pt Xj = d_X[j];
                const float dist = neighbour_dist[m];
                if (j != id_i) {
                    const float gabriel_radius = 0.5f * neighbour_dist[m] * gabriel_coefficient;
                    const Pt mid_point = 0.5f * (Xi + Xj);
                    for (int q = m - 1; q >= 0; q--) {
                        const int k = neighbour_id[q];
                        const Pt r_mk = mid_point - d_X[k];
                        const float dist_mk = ya_dist3(r_mk.x, r_mk.y, r_mk.z);
                        if (dist_mk < gabriel_radius) {
                            gabriel_condition = false;
                            break;
                        }
                    }
                }
                if (gabriel_condition) {
                    const Pt r = Xi - Xj;
                    F += pw_int(Xi, r, dist, id_i, j);
                    const float friction = pw_friction(Xi, r, dist, id_i, j);
                    sum_friction += friction;
                    sum_v += friction * d_old_v[j];
                }
            }
            d_dX[id_i] += F;  // :600-602
            d_sum_v[id_i] = sum_v;
            d_sum_friction[id_i] = sum_friction;
        }
    }
};

template<typename Pt>
using Gabriel_solver = Heun_solver<Pt, Gabriel_computer>;

// links.cuh:142-160, the wall normal to z at the z of node wall_idx
template<typename Pt>
using Wall_force = void(const Pt* d_X, const int i, const int wall_idx, Pt* d_dX, int* d_nints);

template<typename Pt>
void xy_wall_relu_force(const Pt* d_X, const int i, const int wall_idx, Pt* d_dX, int* d_nints)
{
    const float Xwall = d_X[wall_idx].z;
    const float dist_wall = fabsf(d_X[i].z - Xwall);
    if (dist_wall < 1.0f) {
        const float F = fmaxf(0.8 - dist_wall, 0) - fmaxf(dist_wall - 0.8, 0);
        d_dX[i].z += F;
        d_dX[wall_idx].z += -F;  // the reference's atomicAdd, here in index order
        d_nints[wall_idx] += 1;
    }
}

// links.cuh:196-228 (wall kernel, then update_wall_node)
template<typename Pt, Wall_force<Pt> force>
void wall_forces(const int n, const Pt* d_X, Pt* d_dX, const int wall_idx)
{
    std::vector<int> d_nints((size_t)wall_idx + 1, 0);
    for (int i = 0; i < n; i++) {
        if (i == wall_idx) continue;
        force(d_X, i, wall_idx, d_dX, d_nints.data());
    }
    if (d_nints[wall_idx] > 0) {
        const float inv = 1 / float(d_nints[wall_idx]);
        d_dX[wall_idx].x *= inv;
        d_dX[wall_idx].y *= inv;
        d_dX[wall_idx].z *= inv;
    }
}
