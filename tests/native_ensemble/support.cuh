// What the model programs of this directory share: the headers, EXPECT, the seeded rows, the sweep model's own device
// arrays with the functors that read them, the dividing kernels, and the per-replica State of the three programs
// that compare an Ensemble with lone Solutions.  A program keeps its sizes, its runs, what only it has, and its main.
#pragma once

#include "../../include/dtypes.cuh"
#include "../../include/inits.cuh"
#include "../../include/links.cuh"
#include "../../include/property.cuh"
#include "../../include/solvers.cuh"
#include "../../include/ensemble.cuh"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);   \
            failures++;                                               \
        }                                                             \
    } while (0)

static float next_float(unsigned& s)
{
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) / 16777216.f;
}
// the initial rows of a replica: `count` seeded points in a box of `width` that starts at -offset
static void seed_rows(unsigned seed, int count, float width, float offset, float3* rows)
{
    auto next = [&] { return width * next_float(seed) - offset; };
    for (int i = 0; i < count; i++) rows[i] = float3{next(), next(), next()};
}
// (the whole-step programs' rows of replica r: a box at the origin whose side grows with the count)
static void seed_rows(int r, int count, float3* rows)
{
    seed_rows(4321u + 977u * (unsigned)r, count, 1.f + 0.012f * (float)count, 0.f, rows);
}
static int kind_of(int r, int i) { return (i * 7 + r) % 3; }
// links (2k, 2k + 1) of a replica of `count` cells: every cell in at most one link, so the atomic adds of link_forces
// have one term per row and their order cannot matter
static int n_links_of(int count) { return count / 4; }

static float* on_device(const float* values, int n)
{
    float* d_values;
    (void)hipMalloc(&d_values, n * sizeof(float));
    (void)hipMemcpy(d_values, values, n * sizeof(float), hipMemcpyHostToDevice);
    return d_values;
}

// the model's own arrays: one parameter of the sweep per replica (a rest length or a strength), one kind and one
// neighbour counter per cell (flat id space)
__device__ const float* d_sweep;
__device__ const int* d_kind;
__device__ int* d_n_nbs;
__device__ int d_rows_per_replica;

static void point_model_at(const float* sweep, const int* kind, int* nbs, int rows_per_replica)
{
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_sweep), &sweep, sizeof(sweep));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_kind), &kind, sizeof(kind));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_n_nbs), &nbs, sizeof(nbs));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_rows_per_replica), &rows_per_replica, sizeof(int));
}

// The grid forms' sweep, by strength.
namespace by_strength {
__device__ float3 sweep_spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    const float s = d_sweep[i / d_rows_per_replica];   // <- the sweep: this replica's parameter
    const float k = d_kind[i] == d_kind[j] ? 2.f : 1.f;
    return r * (k * s * (0.6f - dist) / dist);
}
// the same force, counting neighbours as examples/passive_growth.cu does: NOT stateless
__device__ float3 counting_spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    d_n_nbs[i] += 1;
    const float s = d_sweep[i / d_rows_per_replica];
    return r * (s * (0.6f - dist) / dist);
}
}  // namespace by_strength
YA_STATELESS(float3, by_strength::sweep_spring)

// The whole-step programs' sweep, by rest length; NOT declared stateless.
namespace by_rest {
__device__ float3 counting_spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    d_n_nbs[i] += 1;                                   // <- per-cell state without atomics: one thread per cell
    const float L = d_sweep[i / d_rows_per_replica];   // <- the sweep: this replica's parameter
    return r * ((L - dist) / dist);
}
}  // namespace by_rest

// Replica r (of the array handed over) divides if its number in the sweep, first + r, is even and it has room:
// cell 3 % n gets a daughter at row n, and d_n[r] grows -- on the device, nothing travels.
__global__ void divide(int n_replicas, int n_max, int first, float3* d_X, float3* d_old_v, int* d_n, int* kind)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_replicas || (first + r) % 2 != 0) return;
    const int n = d_n[r];
    if (n <= 0 || n >= n_max) return;
    const size_t base = (size_t)r * n_max;
    const size_t mother = base + 3 % n, daughter = base + n;
    d_X[daughter] = float3{d_X[mother].x + 0.05f, d_X[mother].y - 0.03f, d_X[mother].z + 0.02f};
    d_old_v[daughter] = d_old_v[mother];
    kind[daughter] = kind[mother];
    d_n[r] = n + 1;
}
// (the same for every even replica of a model without kinds)
__global__ void divide(int n_replicas, int n_max, float3* d_X, float3* d_old_v, int* d_n)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_replicas || r % 2 != 0) return;
    const int n = d_n[r];
    if (n <= 0 || n >= n_max) return;
    const size_t base = (size_t)r * n_max;
    const size_t mother = base + 3 % n, daughter = base + n;
    d_X[daughter] = float3{d_X[mother].x + 0.05f, d_X[mother].y - 0.03f, d_X[mother].z + 0.02f};
    d_old_v[daughter] = d_old_v[mother];
    d_n[r] = n + 1;
}

// One replica at the end of a run against lone Solutions (nbs stays empty in a model without counters).
struct State {
    std::vector<float3> X, v;
    std::vector<int> kind, nbs;
    int n;
};
static void compare(const std::vector<State>& ens, const std::vector<State>& alone)
{
    for (size_t r = 0; r < alone.size(); r++) {
        const int n = alone[r].n;
        EXPECT(ens[r].n == n);
        EXPECT(memcmp(ens[r].X.data(), alone[r].X.data(), n * sizeof(float3)) == 0);
        EXPECT(memcmp(ens[r].v.data(), alone[r].v.data(), n * sizeof(float3)) == 0);
        EXPECT(memcmp(ens[r].kind.data(), alone[r].kind.data(), n * sizeof(int)) == 0);
        EXPECT(memcmp(ens[r].nbs.data(), alone[r].nbs.data(), n * sizeof(int)) == 0);
    }
}

// A whole ensemble at the end of a run against its twin: every row, used or not, the counts, the neighbour counters
// (if the model has them) and which path ran.
struct Run {
    std::vector<float3> X, v;
    std::vector<int> n, nbs;
    long launches;
    int lanes_used;
};
static Run read_back(Ensemble<float3>& cells, Property<int>* nbs = nullptr)
{
    Run out;
    cells.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + cells.rows());
    out.v.resize(cells.rows());
    (void)hipMemcpy(out.v.data(), cells.d_old_v, out.v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    if (nbs) {
        nbs->copy_to_host();
        out.nbs.assign(nbs->h_prop, nbs->h_prop + cells.rows());
    }
    for (int r = 0; r < cells.n_replicas; r++) {
        out.n.push_back(cells.h_n[r]);
        EXPECT(cells.get_d_n(r) == cells.h_n[r]);
    }
    out.launches = cells.whole_step_launches;
    out.lanes_used = cells.whole_step_lanes_used;
    return out;
}
