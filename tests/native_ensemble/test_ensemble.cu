// Ensemble<Pt, Tile_solver> (include/ensemble.cuh) as a model program uses it: a parameter sweep.
//   * the pairwise functor reads ITS REPLICA's rest length from the model's own device array via i / n_max,
//   * and a Property-style per-cell array by ensemble-global id;
//   * Links over the flat id space are the generic forces;
//   * a model kernel appends a daughter to some replicas by bumping d_n[r] on the device between steps;
//   * nothing is read back until the end.
// Every replica is then compared bit for bit -- positions, old_v, count, the per-cell array -- with a
// Solution<float3, Tile_solver> run of the same system, for the engine's choice of lanes and for 1, 16 and 64
// lanes per cell, with the centre of mass fixed and after set_fixed_xy.
#include "support.cuh"

// the rest-length sweep with kinds (support.cuh: d_sweep, d_kind, d_rows_per_replica)
__device__ float3 sweep_spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    const float L = d_sweep[i / d_rows_per_replica];   // <- the sweep: this replica's parameter
    const float k = d_kind[i] == d_kind[j] ? 2.f : 1.f;
    return r * (k * (L - dist) / dist);
}
YA_STATELESS(float3, sweep_spring)

constexpr int M = 6, N_MAX = 400, STEPS = 6;
static const int counts[M] = {300, 0, 64, 257, 129, 3};
static const float rests[M] = {0.5f, 0.55f, 0.6f, 0.65f, 0.7f, 0.75f};

// the initial rows of replica r: a seeded ball, different for every replica
static void seed_replica(int r, float3* rows) { seed_rows(12345u + 977u * (unsigned)r, counts[r], 3.f, 1.5f, rows); }

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

static State single(int r, const float* d_rests, int fixed_xy)
{
    Solution<float3, Tile_solver> cells{N_MAX};
    *cells.h_n = counts[r];
    seed_replica(r, cells.h_X);
    cells.copy_to_device();
    Property<int> kind{N_MAX, "kind"};
    for (int i = 0; i < N_MAX; i++) kind.h_prop[i] = kind_of(r, i);
    kind.copy_to_device();
    Links links{N_MAX, 0.3f};
    for (int k = 0; k < n_links_of(counts[r]); k++) links.h_link[k] = Link{2 * k, 2 * k + 1};
    *links.h_n = n_links_of(counts[r]);
    links.copy_to_device();
    point_model_at(d_rests + r, kind.d_prop, nullptr, N_MAX);   // i / N_MAX == 0: this system's one parameter
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
        seed_replica(r, cells.row(r, 0));
    }
    cells.copy_to_device();
    Property<int> kind{M * N_MAX, "kind"};   // sized for the flat id space, indexed by global id
    for (int r = 0; r < M; r++)
        for (int i = 0; i < N_MAX; i++) kind.h_prop[cells.index(r, i)] = kind_of(r, i);
    kind.copy_to_device();
    Links links{M * N_MAX, 0.3f};
    int n_links = 0;
    for (int r = 0; r < M; r++)
        for (int k = 0; k < n_links_of(counts[r]); k++)
            links.h_link[n_links++] = Link{(int)cells.index(r, 2 * k), (int)cells.index(r, 2 * k + 1)};
    *links.h_n = n_links;
    links.copy_to_device();
    point_model_at(d_rests, kind.d_prop, nullptr, N_MAX);
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
    float* d_rests = on_device(rests, M);
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
        float* d_swapped = on_device(swapped, M);
        const std::vector<State> a = together(d_rests, 0, -1), b = together(d_swapped, 0, -1);
        EXPECT(memcmp(a[0].X.data(), b[0].X.data(), counts[0] * sizeof(float3)) != 0);
        EXPECT(memcmp(a[2].X.data(), b[2].X.data(), counts[2] * sizeof(float3)) == 0);
        (void)hipFree(d_swapped);
    }
    (void)hipFree(d_rests);
    printf(failures ? "%d FAILURES\n" : "ALL ENSEMBLE TESTS PASSED\n", failures);
    return failures != 0;
}
