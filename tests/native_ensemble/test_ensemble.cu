// Ensemble<Pt, Tile_solver> (include/ensemble.cuh) as a model program uses it: a parameter sweep.
//   * the pairwise functor reads ITS REPLICA's rest length from the model's own device array via i / n_max,
//   * and a Property-style per-cell array by ensemble-global id;
//   * Links over the flat id space are the generic forces;
//   * a model kernel appends a daughter to some replicas by bumping d_n[r] on the device between steps;
//   * nothing is read back until the end.
// Every replica is then compared bit for bit -- positions, old_v, count, the per-cell array -- with a
// Solution<float3, Tile_solver> run of the same system, for the engine's choice of lanes and for 1, 16 and 64
// lanes per cell, with the centre of mass fixed and after set_fixed_xy.
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

// the model's own arrays: one rest length per replica, one kind per cell (flat id space)
__device__ const float* d_rest;
__device__ const int* d_kind;
__device__ int d_rows_per_replica;

__device__ float3 sweep_spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    const float L = d_rest[i / d_rows_per_replica];   // <- the sweep: this replica's parameter
    const float k = d_kind[i] == d_kind[j] ? 2.f : 1.f;
    return r * (k * (L - dist) / dist);
}
YA_STATELESS(float3, sweep_spring)

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

constexpr int M = 6, N_MAX = 400, STEPS = 6;
static const int counts[M] = {300, 0, 64, 257, 129, 3};
static const float rests[M] = {0.5f, 0.55f, 0.6f, 0.65f, 0.7f, 0.75f};

struct State {
    std::vector<float3> X, v;
    std::vector<int> kind;
    int n;
};

// the initial rows of replica r: a seeded ball, different for every replica
static void seed_rows(int r, float3* rows)
{
    unsigned s = 12345u + 977u * (unsigned)r;
    auto next = [&s]() {
        s = s * 1664525u + 1013904223u;
        return (float)(s >> 8) / 16777216.f;
    };
    for (int i = 0; i < counts[r]; i++) rows[i] = float3{3.f * next() - 1.5f, 3.f * next() - 1.5f, 3.f * next() - 1.5f};
}
static int kind_of(int r, int i) { return (i * 7 + r) % 3; }
// links (2k, 2k + 1) of a replica: every cell in at most one link, so the atomic adds of link_forces have one
// term per row and their order cannot matter
static int n_links_of(int r) { return counts[r] / 4; }

template<typename Cells>
static void model_steps(Cells& cells, Links& links, Property<int>& kind, int n_replicas, int first, int fixed_xy)
{
    if (fixed_xy >= 0) cells.set_fixed_xy(fixed_xy);
    auto gen = [&links](const int, const float3* __restrict__ d_X, float3* d_dX) { link_forces<float3>(links, d_X, d_dX); };
    for (int step = 0; step < STEPS; step++) {
        cells.template take_step<sweep_spring>(step < 4 ? 0.05f : 0.02f, Generic_forces<float3>{gen});
        if (step == 1 || step == 3)
            divide<<<(n_replicas + 63) / 64, 64>>>(n_replicas, N_MAX, first, cells.d_X, cells.d_old_v, cells.d_n, kind.d_prop);
    }
}

static void point_model_at(const float* rest, const int* kind, int rows_per_replica)
{
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_rest), &rest, sizeof(rest));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_kind), &kind, sizeof(kind));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_rows_per_replica), &rows_per_replica, sizeof(int));
}

static State single(int r, const float* d_rests, int fixed_xy)
{
    Solution<float3, Tile_solver> cells{N_MAX};
    *cells.h_n = counts[r];
    seed_rows(r, cells.h_X);
    cells.copy_to_device();
    Property<int> kind{N_MAX, "kind"};
    for (int i = 0; i < N_MAX; i++) kind.h_prop[i] = kind_of(r, i);
    kind.copy_to_device();
    Links links{N_MAX, 0.3f};
    for (int k = 0; k < n_links_of(r); k++) links.h_link[k] = Link{2 * k, 2 * k + 1};
    *links.h_n = n_links_of(r);
    links.copy_to_device();
    point_model_at(d_rests + r, kind.d_prop, N_MAX);   // i / N_MAX == 0: this system's one parameter
    model_steps(cells, links, kind, 1, r, counts[r] > 0 ? fixed_xy : -1);
    State out;
    cells.copy_to_host();
    out.n = *cells.h_n;
    out.X.assign(cells.h_X, cells.h_X + N_MAX);
    out.v.resize(N_MAX);
    (void)hipMemcpy(out.v.data(), cells.d_old_v, N_MAX * sizeof(float3), hipMemcpyDeviceToHost);
    kind.copy_to_host();
    out.kind.assign(kind.h_prop, kind.h_prop + N_MAX);
    return out;
}

static std::vector<State> together(const float* d_rests, int lanes, int fixed_xy)
{
    Ensemble<float3> cells{M, N_MAX};
    cells.lanes_per_cell = lanes;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        seed_rows(r, cells.row(r, 0));
    }
    cells.copy_to_device();
    Property<int> kind{M * N_MAX, "kind"};   // sized for the flat id space, indexed by global id
    for (int r = 0; r < M; r++)
        for (int i = 0; i < N_MAX; i++) kind.h_prop[cells.index(r, i)] = kind_of(r, i);
    kind.copy_to_device();
    Links links{M * N_MAX, 0.3f};
    int n_links = 0;
    for (int r = 0; r < M; r++)
        for (int k = 0; k < n_links_of(r); k++)
            links.h_link[n_links++] = Link{(int)cells.index(r, 2 * k), (int)cells.index(r, 2 * k + 1)};
    *links.h_n = n_links;
    links.copy_to_device();
    point_model_at(d_rests, kind.d_prop, N_MAX);
    model_steps(cells, links, kind, M, 0, fixed_xy);
    // ... and only now does anything come back
    std::vector<State> out(M);
    cells.copy_to_host();
    std::vector<float3> v(M * N_MAX);
    (void)hipMemcpy(v.data(), cells.d_old_v, v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    kind.copy_to_host();
    for (int r = 0; r < M; r++) {
        out[r].n = cells.h_n[r];
        EXPECT(cells.get_d_n(r) == out[r].n);
        out[r].X.assign(cells.row(r, 0), cells.row(r, 0) + N_MAX);
        out[r].v.assign(v.begin() + cells.index(r, 0), v.begin() + cells.index(r, 0) + N_MAX);
        out[r].kind.assign(kind.h_prop + cells.index(r, 0), kind.h_prop + cells.index(r, 0) + N_MAX);
    }
    return out;
}

int main()
{
    float* d_rests;
    (void)hipMalloc(&d_rests, sizeof(rests));
    (void)hipMemcpy(d_rests, rests, sizeof(rests), hipMemcpyHostToDevice);
    for (int fixed_xy : {-1, 2}) {
        std::vector<State> alone;
        for (int r = 0; r < M; r++) alone.push_back(single(r, d_rests, fixed_xy));
        // the replicas that divide grew twice, the others and the empty one did not
        for (int r = 0; r < M; r++) EXPECT(alone[r].n == counts[r] + (r % 2 == 0 && counts[r] > 0 ? 2 : 0));
        for (int lanes : {0, 1, 16, 64}) {
            const std::vector<State> ens = together(d_rests, lanes, fixed_xy);
            for (int r = 0; r < M; r++) {
                const int n = alone[r].n;
                EXPECT(ens[r].n == n);
                EXPECT(memcmp(ens[r].X.data(), alone[r].X.data(), n * sizeof(float3)) == 0);
                EXPECT(memcmp(ens[r].v.data(), alone[r].v.data(), n * sizeof(float3)) == 0);
                EXPECT(memcmp(ens[r].kind.data(), alone[r].kind.data(), n * sizeof(int)) == 0);
            }
        }
    }
    {
        // the per-replica parameter is really read: replica 0 stepped alone with replica 4's rest length differs
        float swapped[M];
        memcpy(swapped, rests, sizeof(rests));
        swapped[0] = rests[4];
        float* d_swapped;
        (void)hipMalloc(&d_swapped, sizeof(swapped));
        (void)hipMemcpy(d_swapped, swapped, sizeof(swapped), hipMemcpyHostToDevice);
        const std::vector<State> a = together(d_rests, 0, -1), b = together(d_swapped, 0, -1);
        EXPECT(memcmp(a[0].X.data(), b[0].X.data(), counts[0] * sizeof(float3)) != 0);
        EXPECT(memcmp(a[2].X.data(), b[2].X.data(), counts[2] * sizeof(float3)) == 0);
        (void)hipFree(d_swapped);
    }
    (void)hipFree(d_rests);
    printf(failures ? "%d FAILURES\n" : "ALL ENSEMBLE TESTS PASSED\n", failures);
    return failures != 0;
}
