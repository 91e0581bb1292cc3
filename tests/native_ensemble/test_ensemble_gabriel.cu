// Ensemble<Pt, Gabriel_solver> (include/ensemble_gabriel.cuh) as a model program uses it.
// 1. The reference's known answer (its test_gabriel_solver: the 19-cell regular_hexagon(0.5), grid 5, coefficient
//    0.8 -> 6 / 3 / 4 Gabriel neighbours) in EVERY replica of one ensemble: a functor that counts with a plain
//    `d_n_nbs[i] += 1` (not declared stateless: one lane evaluates a cell's pairs, in order) over a Property sized
//    for the flat id space, reset by a generic force in every stage.  The counts must stand at the GLOBAL ids
//    r * n_max + local: a force kernel that handed the functor local ids would pile them all into replica 0's rows.
// 2. A parameter sweep on ONE ensemble:
//   * the pairwise functor reads ITS REPLICA's strength from the model's own device array via i / n_max,
//   * and a Property-style per-cell array by ensemble-global id;
//   * Links over the flat id space are the generic forces;
//   * a model kernel divides cells of some replicas by raising d_n[r] on the device between steps;
//   * a second functor counts neighbours with a plain `d_n_nbs[i] += 1`;
//   * one replica is dense (more than 64 candidates per cell: the dense kernel's list of flat rows);
//   * nothing is read back until the end.
// Every replica is then compared with memcmp -- positions, old_v, count, the per-cell arrays -- with a
// Solution<float3, Gabriel_solver> run of the same system, with the centre of mass fixed and after set_fixed_xy.
#include "support.cuh"

using by_strength::counting_spring;  // the strength sweep with kinds and its counting twin (support.cuh)
using by_strength::sweep_spring;

// the reference's counting functor (its test_solvers.cu) on the model's own counters
__device__ float3 count_gabriel_neighbours(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist > 1.f) return dF;
    d_n_nbs[i] += 1;
    return dF;
}
__global__ void reset_counters(int n, int* nbs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) nbs[i] = 0;
}

constexpr int M = 6, N_MAX = 400, STEPS = 6, GRID_SIZE = 12, DENSE = 3;
constexpr float COEFFICIENT = 0.8f;
static const int counts[M] = {300, 0, 64, 257, 129, 3};
static const float strengths[M] = {0.5f, 0.75f, 1.f, 1.25f, 1.5f, 2.f};

// the initial rows of replica r: a seeded box well inside the 12^3 grid, different for every replica; replica
// DENSE's box is half as wide: 257 cells in 1.5^3, more than 64 candidates for all but the outermost cells
static void seed_replica(int r, float3* rows)
{
    const float w = r == DENSE ? 1.5f : 3.f;
    seed_rows(12345u + 977u * (unsigned)r, counts[r], w, w / 2, rows);
}

template<typename Cells>
static void model_steps(Cells& cells, Links& links, Property<int>& kind, int n_replicas, int first, int fixed_xy,
    bool counting)
{
    if (fixed_xy >= 0) cells.set_fixed_xy(fixed_xy);
    auto gen = [&links](const int, const float3* __restrict__ d_X, float3* d_dX) { link_forces<float3>(links, d_X, d_dX); };
    for (int step = 0; step < STEPS; step++) {
        const float dt = step < 4 ? 0.05f : 0.02f;
        if (counting)
            cells.template take_step<counting_spring>(dt, Generic_forces<float3>{gen});
        else
            cells.template take_step<sweep_spring>(dt, Generic_forces<float3>{gen});
        if (step == 1 || step == 3)
            divide<<<(n_replicas + 63) / 64, 64>>>(n_replicas, N_MAX, first, cells.d_X, cells.d_old_v, cells.d_n, kind.d_prop);
    }
}

static State single(int r, const float* d_strengths, int fixed_xy, bool counting)
{
    Solution<float3, Gabriel_solver> cells{N_MAX, GRID_SIZE, 1.f, COEFFICIENT};
    *cells.h_n = counts[r];
    seed_replica(r, cells.h_X);
    cells.copy_to_device();
    Property<int> kind{N_MAX, "kind"}, nbs{N_MAX, "nbs"};
    for (int i = 0; i < N_MAX; i++) kind.h_prop[i] = kind_of(r, i), nbs.h_prop[i] = 0;
    kind.copy_to_device();
    nbs.copy_to_device();
    Links links{N_MAX, 0.3f};
    for (int k = 0; k < n_links_of(counts[r]); k++) links.h_link[k] = Link{2 * k, 2 * k + 1};
    *links.h_n = n_links_of(counts[r]);
    links.copy_to_device();
    point_model_at(d_strengths + r, kind.d_prop, nbs.d_prop, N_MAX);   // i / N_MAX == 0: this system's one parameter
    model_steps(cells, links, kind, 1, r, counts[r] > 0 ? fixed_xy : -1, counting);
    State out;
    cells.copy_to_host();
    out.n = *cells.h_n;
    out.X.assign(cells.h_X, cells.h_X + N_MAX);
    out.v.resize(N_MAX);
    (void)hipMemcpy(out.v.data(), cells.d_old_v, N_MAX * sizeof(float3), hipMemcpyDeviceToHost);
    kind.copy_to_host();
    nbs.copy_to_host();
    out.kind.assign(kind.h_prop, kind.h_prop + N_MAX);
    out.nbs.assign(nbs.h_prop, nbs.h_prop + N_MAX);
    return out;
}

static std::vector<State> together(const float* d_strengths, int fixed_xy, bool counting)
{
    Ensemble<float3, Gabriel_solver> cells{M, N_MAX, GRID_SIZE, 1.f, COEFFICIENT};
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        seed_replica(r, cells.row(r, 0));
    }
    cells.copy_to_device();
    Property<int> kind{M * N_MAX, "kind"}, nbs{M * N_MAX, "nbs"};   // sized for the flat id space, indexed by global id
    for (int r = 0; r < M; r++)
        for (int i = 0; i < N_MAX; i++) kind.h_prop[cells.index(r, i)] = kind_of(r, i), nbs.h_prop[cells.index(r, i)] = 0;
    kind.copy_to_device();
    nbs.copy_to_device();
    Links links{M * N_MAX, 0.3f};
    int n_links = 0;
    for (int r = 0; r < M; r++)
        for (int k = 0; k < n_links_of(counts[r]); k++)
            links.h_link[n_links++] = Link{(int)cells.index(r, 2 * k), (int)cells.index(r, 2 * k + 1)};
    *links.h_n = n_links;
    links.copy_to_device();
    point_model_at(d_strengths, kind.d_prop, nbs.d_prop, N_MAX);
    model_steps(cells, links, kind, M, 0, fixed_xy, counting);
    // ... and only now does anything come back
    EXPECT(cells.dense_cells() > 0);  // (replica DENSE: the dense kernel ran)
    std::vector<State> out(M);
    cells.copy_to_host();
    std::vector<float3> v(M * N_MAX);
    (void)hipMemcpy(v.data(), cells.d_old_v, v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    kind.copy_to_host();
    nbs.copy_to_host();
    for (int r = 0; r < M; r++) {
        out[r].n = cells.h_n[r];
        EXPECT(cells.get_d_n(r) == out[r].n);
        EXPECT(cells.status(r) == 0);
        out[r].X.assign(cells.row(r, 0), cells.row(r, 0) + N_MAX);
        out[r].v.assign(v.begin() + cells.index(r, 0), v.begin() + cells.index(r, 0) + N_MAX);
        out[r].kind.assign(kind.h_prop + cells.index(r, 0), kind.h_prop + cells.index(r, 0) + N_MAX);
        out[r].nbs.assign(nbs.h_prop + cells.index(r, 0), nbs.h_prop + cells.index(r, 0) + N_MAX);
    }
    return out;
}

// The reference's known answer in every replica, at global ids.
static void known_answer()
{
    constexpr int REPLICAS = 5, CELLS = 19, ROWS = 24;
    Solution<float3, Gabriel_solver> one{CELLS, 5, 1.f, 0.8f};
    regular_hexagon(0.5f, one);
    Ensemble<float3, Gabriel_solver> cells{REPLICAS, ROWS, 5, 1.f, 0.8f};
    for (int r = 0; r < REPLICAS; r++) {
        cells.h_n[r] = CELLS;
        for (int i = 0; i < CELLS; i++) *cells.row(r, i) = one.h_X[i];
    }
    cells.copy_to_device();
    Property<int> nbs{REPLICAS * ROWS, "nbs"};
    for (int i = 0; i < REPLICAS * ROWS; i++) nbs.h_prop[i] = -7;
    nbs.copy_to_device();
    point_model_at(nullptr, nullptr, nbs.d_prop, ROWS);
    int* d_nbs = nbs.d_prop;
    auto reset = [d_nbs](const int n, const float3* __restrict__, float3*) {
        reset_counters<<<(n + 255) / 256, 256>>>(n, d_nbs);
    };
    cells.take_step<count_gabriel_neighbours>(1.f, Generic_forces<float3>{reset});
    nbs.copy_to_host();
    for (int r = 0; r < REPLICAS; r++) {
        const int* c = nbs.h_prop + cells.index(r, 0);
        for (int i = 0; i < 7; i++) EXPECT(c[i] == 6);
        for (int i = 7; i < CELLS; i += 2) EXPECT(c[i] == 3);
        for (int i = 8; i < CELLS; i += 2) EXPECT(c[i] == 4);
        for (int i = CELLS; i < ROWS; i++) EXPECT(c[i] == 0);  // (reset, never counted)
    }
    EXPECT(cells.dense_cells() == 0);
}

int main()
{
    known_answer();
    float* d_strengths = on_device(strengths, M);
    for (int fixed_xy : {-1, 2}) {
        std::vector<State> alone;
        for (int r = 0; r < M; r++) alone.push_back(single(r, d_strengths, fixed_xy, false));
        // the replicas that divide grew twice, the others and the empty one did not
        for (int r = 0; r < M; r++) EXPECT(alone[r].n == counts[r] + (r % 2 == 0 && counts[r] > 0 ? 2 : 0));
        compare(together(d_strengths, fixed_xy, false), alone);
    }
    {
        // the counting functor: one lane evaluates a cell's pairs, and every count is a lone system's
        std::vector<State> alone;
        long counted = 0;
        for (int r = 0; r < M; r++) {
            alone.push_back(single(r, d_strengths, -1, true));
            for (int i = 0; i < alone[r].n; i++) counted += alone[r].nbs[i];
        }
        EXPECT(counted > 0);
        compare(together(d_strengths, -1, true), alone);
    }
    {
        // the per-replica parameter is really read: replica 0 stepped with replica 4's strength differs
        float swapped[M];
        memcpy(swapped, strengths, sizeof(strengths));
        swapped[0] = strengths[4];
        float* d_swapped = on_device(swapped, M);
        const std::vector<State> a = together(d_strengths, -1, false), b = together(d_swapped, -1, false);
        EXPECT(memcmp(a[0].X.data(), b[0].X.data(), counts[0] * sizeof(float3)) != 0);
        EXPECT(memcmp(a[2].X.data(), b[2].X.data(), counts[2] * sizeof(float3)) == 0);
        (void)hipFree(d_swapped);
    }
    (void)hipFree(d_strengths);
    printf(failures ? "%d FAILURES\n" : "ALL GABRIEL ENSEMBLE TESTS PASSED\n", failures);
    return failures != 0;
}
