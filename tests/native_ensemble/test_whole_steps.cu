// Ensemble<Pt, Tile_solver>::take_steps (include/ensemble.cuh) as a model program uses it: a parameter sweep whose
// quiet stretches run as whole-step launches (ya::ens::whole_steps) and whose steps with Links do not.
//   * the pairwise functor reads ITS REPLICA's rest length from the model's own device array via i / n_max;
//   * it is NOT declared YA_STATELESS: it counts a cell's neighbours in a per-cell array (d_n_nbs[i] += 1), which
//     one thread per cell must leave exactly as take_step leaves it;
//   * a model kernel appends a daughter to some replicas by bumping d_n[r] on the device between calls;
//   * ONE Ensemble alternates take_steps (whole-step launches) with take_step carrying Links as generic forces,
//     whose right-hand sides must be zeroed again after the launches that never touched them.
// Everything -- positions, old_v, counts, the neighbour counters -- is compared bit for bit with a twin Ensemble
// that only ever calls take_step, with the centre of mass fixed, a point fixed and after set_fixed_xy.
#include "support.cuh"

using by_rest::counting_spring;  // (support.cuh: reads d_sweep, counts in d_n_nbs)

constexpr int M = 7, N_MAX = 520;
static const int counts[M] = {300, 0, 64, 257, 129, 3, 518};   // (518 + 2 daughters: the replica ends full)
static const float rests[M] = {0.5f, 0.55f, 0.6f, 0.65f, 0.7f, 0.75f, 0.8f};

// The model's run.  whole: the quiet stretches are take_steps calls (whole_steps = 1, at most 2 steps per
// launch); otherwise every step is a take_step (whole_steps = -1 for good measure).
static Run run(const float* d_rests, const bool whole, const int fixed_mode)
{
    Ensemble<float3> cells{M, N_MAX};
    cells.whole_steps = whole ? 1 : -1;
    cells.steps_per_launch = 2;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        seed_rows(r, counts[r], cells.row(r, 0));
    }
    cells.copy_to_device();
    Property<int> nbs{M * N_MAX, "n_nbs"};
    for (int i = 0; i < M * N_MAX; i++) nbs.h_prop[i] = 0;
    nbs.copy_to_device();
    Links links{M * N_MAX, 0.3f};
    int n_links = 0;
    for (int r = 0; r < M; r++)
        for (int k = 0; k < n_links_of(counts[r]); k++)
            links.h_link[n_links++] = Link{(int)cells.index(r, 2 * k), (int)cells.index(r, 2 * k + 1)};
    *links.h_n = n_links;
    links.copy_to_device();
    point_model_at(d_rests, nullptr, nbs.d_prop, N_MAX);

    if (fixed_mode == 1) cells.set_fixed(2);
    if (fixed_mode == 2) cells.set_fixed_xy(1);
    auto gen = [&links](const int, const float3* __restrict__ d_X, float3* d_dX) { link_forces<float3>(links, d_X, d_dX); };
    auto quiet = [&](float dt, int n_steps) {
        if (whole)
            cells.take_steps<counting_spring>(dt, n_steps);
        else
            for (int s = 0; s < n_steps; s++) cells.take_step<counting_spring>(dt);
    };
    auto linked = [&](float dt) { cells.take_step<counting_spring>(dt, Generic_forces<float3>{gen}); };
    quiet(0.05f, 3);   // 2 launches
    linked(0.05f);     // leaves both right-hand sides zeroed for its next call ...
    quiet(0.05f, 1);   // 1 launch   ... which these launches never write
    linked(0.05f);
    linked(0.02f);
    divide<<<(M + 63) / 64, 64>>>(M, N_MAX, cells.d_X, cells.d_old_v, cells.d_n);
    quiet(0.02f, 5);   // 3 launches
    divide<<<(M + 63) / 64, 64>>>(M, N_MAX, cells.d_X, cells.d_old_v, cells.d_n);
    linked(0.05f);
    quiet(0.05f, 2);   // 1 launch
    // (take_steps with generic forces is the loop of take_step, whatever whole_steps says)
    if (whole)
        cells.take_steps<counting_spring>(0.05f, 2, Generic_forces<float3>{gen});
    else
        for (int s = 0; s < 2; s++) linked(0.05f);

    return read_back(cells, &nbs);
}

int main()
{
    static_assert(ya::ens::whole_step_capacity<float3>() == 1024, "float3 replicas of up to 1024 cells fit");
    static_assert(ya::ens::whole_step_capacity<float4>() == 1024, "float4 too");
    float* d_rests = on_device(rests, M);
    for (int fixed_mode : {0, 1, 2}) {
        const Run twin = run(d_rests, false, fixed_mode);
        const Run mixed = run(d_rests, true, fixed_mode);
        EXPECT(twin.launches == 0);
        EXPECT(mixed.launches == 2 + 1 + 3 + 1);
        for (int r = 0; r < M; r++) {
            EXPECT(twin.n[r] == counts[r] + (r % 2 == 0 && counts[r] > 0 ? 2 : 0));
            EXPECT(mixed.n[r] == twin.n[r]);
        }
        EXPECT(twin.n[6] == N_MAX);
        // every row, used or not, and every counter
        EXPECT(memcmp(mixed.X.data(), twin.X.data(), twin.X.size() * sizeof(float3)) == 0);
        EXPECT(memcmp(mixed.v.data(), twin.v.data(), twin.v.size() * sizeof(float3)) == 0);
        EXPECT(memcmp(mixed.nbs.data(), twin.nbs.data(), twin.nbs.size() * sizeof(int)) == 0);
        long counted = 0;
        for (int c : twin.nbs) counted += c;
        EXPECT(counted > 0);
    }
    {
        // the per-replica parameter is really read by the whole-step kernel: replica 0 with replica 4's rest length
        float swapped[M];
        memcpy(swapped, rests, sizeof(rests));
        swapped[0] = rests[4];
        float* d_swapped = on_device(swapped, M);
        const Run a = run(d_rests, true, 0), b = run(d_swapped, true, 0);
        EXPECT(memcmp(a.X.data(), b.X.data(), counts[0] * sizeof(float3)) != 0);
        EXPECT(memcmp(a.X.data() + 2 * N_MAX, b.X.data() + 2 * N_MAX, counts[2] * sizeof(float3)) == 0);
        (void)hipFree(d_swapped);
    }
    (void)hipFree(d_rests);
    printf(failures ? "%d FAILURES\n" : "ALL WHOLE-STEP TESTS PASSED\n", failures);
    return failures != 0;
}
