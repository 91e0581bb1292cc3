// Ensemble<Pt, Grid_solver> (include/ensemble_grid.cuh) as a model program uses it: a parameter sweep.
//   * the pairwise functor reads ITS REPLICA's strength from the model's own device array via i / n_max,
//   * and a Property-style per-cell array by ensemble-global id;
//   * Links over the flat id space are the generic forces;
//   * a model kernel divides cells of some replicas by raising d_n[r] on the device between steps;
//   * a second functor counts neighbours with a plain `d_n_nbs[i] += 1`: it is not declared stateless, so the
//     engine must give it one lane per cell, and the counts must be exactly a lone system's;
//   * nothing is read back until the end.
// Every replica is then compared with memcmp -- positions, old_v, count, the per-cell arrays -- with a
// Solution<float3, Grid_solver> run of the same system, for the engine's choice of lanes and for 1, 4, 8 and 16
// lanes per cell, with the centre of mass fixed and after set_fixed_xy.
#include "support.cuh"

using by_strength::counting_spring;  // the strength sweep with kinds and its counting twin (support.cuh)
using by_strength::sweep_spring;

constexpr int M = 6, N_MAX = 400, STEPS = 6, GRID_SIZE = 12;
static const int counts[M] = {300, 0, 64, 257, 129, 3};
static const float strengths[M] = {0.5f, 0.75f, 1.f, 1.25f, 1.5f, 2.f};

// the initial rows of replica r: a seeded box well inside the 12^3 grid, different for every replica
static void seed_replica(int r, float3* rows) { seed_rows(12345u + 977u * (unsigned)r, counts[r], 3.f, 1.5f, rows); }

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
    Solution<float3, Grid_solver> cells{N_MAX, GRID_SIZE};
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

static std::vector<State> together(const float* d_strengths, int lanes, int fixed_xy, bool counting)
{
    Ensemble<float3, Grid_solver> cells{M, N_MAX, GRID_SIZE};
    cells.lanes_per_cell = lanes;
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

int main()
{
    float* d_strengths = on_device(strengths, M);
    for (int fixed_xy : {-1, 2}) {
        std::vector<State> alone;
        for (int r = 0; r < M; r++) alone.push_back(single(r, d_strengths, fixed_xy, false));
        // the replicas that divide grew twice, the others and the empty one did not
        for (int r = 0; r < M; r++) EXPECT(alone[r].n == counts[r] + (r % 2 == 0 && counts[r] > 0 ? 2 : 0));
        for (int lanes : {0, 1, 4, 8, 16}) compare(together(d_strengths, lanes, fixed_xy, false), alone);
    }
    {
        // the counting functor: the engine's choice must be one lane per cell, and every count a lone system's
        std::vector<State> alone;
        long counted = 0;
        for (int r = 0; r < M; r++) {
            alone.push_back(single(r, d_strengths, -1, true));
            for (int i = 0; i < alone[r].n; i++) counted += alone[r].nbs[i];
        }
        EXPECT(counted > 0);
        compare(together(d_strengths, 0, -1, true), alone);
    }
    {
        // the per-replica parameter is really read: replica 0 stepped with replica 4's strength differs
        float swapped[M];
        memcpy(swapped, strengths, sizeof(strengths));
        swapped[0] = strengths[4];
        float* d_swapped = on_device(swapped, M);
        const std::vector<State> a = together(d_strengths, 0, -1, false), b = together(d_swapped, 0, -1, false);
        EXPECT(memcmp(a[0].X.data(), b[0].X.data(), counts[0] * sizeof(float3)) != 0);
        EXPECT(memcmp(a[2].X.data(), b[2].X.data(), counts[2] * sizeof(float3)) == 0);
        (void)hipFree(d_swapped);
    }
    (void)hipFree(d_strengths);
    printf(failures ? "%d FAILURES\n" : "ALL GRID ENSEMBLE TESTS PASSED\n", failures);
    return failures != 0;
}
