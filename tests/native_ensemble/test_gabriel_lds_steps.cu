// Ensemble<Pt, Gabriel_solver>::take_steps (include/ensemble_gabriel.cuh) as a model program uses it: ONE ensemble
// alternates take_steps -- launches that step from LDS (lds_steps = 1) -- with take_step, its functor counts
// neighbours per cell with a plain `d_n_nbs[i] += 1` (NOT declared stateless: one lane evaluates a cell's pairs, in
// order, at ensemble-global ids) and reads its replica's strength through i / n_max, and a kernel divides cells of
// some replicas by raising d_n[r] on the device in between.  One replica is dense (more than 64 candidates per cell:
// the in-launch dense path), one is empty.  A twin that only ever calls take_step is the check: every row of
// positions and old_v, the counts and every neighbour counter, memcmp-equal.
#include "support.cuh"

using by_strength::counting_spring;

constexpr int M = 6, N_MAX = 400, GRID_SIZE = 12, DENSE = 3;
constexpr float COEFFICIENT = 0.8f;
static const int counts[M] = {300, 0, 64, 257, 129, 3};
static const float strengths[M] = {0.5f, 0.75f, 1.f, 1.25f, 1.5f, 2.f};

// (tests/native_ensemble/test_ensemble_gabriel.cu's rows: replica DENSE's box is half as wide)
static void seed_replica(int r, float3* rows)
{
    const float w = r == DENSE ? 1.5f : 3.f;
    seed_rows(12345u + 977u * (unsigned)r, counts[r], w, w / 2, rows);
}

struct Result {
    std::vector<float3> X, v;
    std::vector<int> n, nbs;
    long launches;
    unsigned long long lds_dense;
};

// The model: 3 steps, a division, 1 step, 4 steps, a division, 2 steps, 1 step.  from_lds: the runs of several steps
// are take_steps calls; else every step is a take_step.
static Result run(const float* d_strengths, bool from_lds, int fixed_xy)
{
    Ensemble<float3, Gabriel_solver> cells{M, N_MAX, GRID_SIZE, 1.f, COEFFICIENT};
    cells.lds_steps = 1;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        seed_replica(r, cells.row(r, 0));
    }
    cells.copy_to_device();
    if (fixed_xy >= 0) cells.set_fixed_xy(fixed_xy);
    Property<int> kind{M * N_MAX, "kind"}, nbs{M * N_MAX, "nbs"};  // sized for the flat id space
    for (int i = 0; i < M * N_MAX; i++) kind.h_prop[i] = 0, nbs.h_prop[i] = 0;
    kind.copy_to_device();
    nbs.copy_to_device();
    point_model_at(d_strengths, kind.d_prop, nbs.d_prop, N_MAX);
    const auto steps = [&](float dt, int k) {
        if (from_lds) {
            cells.take_steps<counting_spring>(dt, k);
        } else {
            for (int s = 0; s < k; s++) cells.take_step<counting_spring>(dt);
        }
    };
    const auto division = [&] {
        divide<<<(M + 63) / 64, 64>>>(M, N_MAX, 0, cells.d_X, cells.d_old_v, cells.d_n, kind.d_prop);
    };
    steps(0.05f, 3);
    division();
    cells.take_step<counting_spring>(0.05f);
    steps(0.02f, 4);
    division();
    steps(0.05f, 2);
    cells.take_step<counting_spring>(0.02f);

    Result out;
    out.launches = cells.lds_step_launches;
    out.lds_dense = cells.lds_dense_cells();
    cells.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + cells.rows());
    out.v.resize(cells.rows());
    (void)hipMemcpy(out.v.data(), cells.d_old_v, out.v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    nbs.copy_to_host();
    out.nbs.assign(nbs.h_prop, nbs.h_prop + cells.rows());
    for (int r = 0; r < M; r++) {
        out.n.push_back(cells.h_n[r]);
        EXPECT(cells.get_d_n(r) == cells.h_n[r]);
        EXPECT(cells.status(r) == 0);
    }
    return out;
}

int main()
{
    float* d_strengths = on_device(strengths, M);
    for (int fixed_xy : {-1, 2}) {
        const Result twin = run(d_strengths, false, fixed_xy), mine = run(d_strengths, true, fixed_xy);
        EXPECT(twin.launches == 0 && twin.lds_dense == 0);
        EXPECT(mine.launches == 3);      // (one launch per take_steps call: 3, 4 and 2 steps)
        EXPECT(mine.lds_dense > 0);      // (replica DENSE: the in-launch dense path ran)
        for (int r = 0; r < M; r++) EXPECT(mine.n[r] == counts[r] + (r % 2 == 0 && counts[r] > 0 ? 2 : 0));
        EXPECT(mine.n == twin.n);
        EXPECT(memcmp(mine.X.data(), twin.X.data(), mine.X.size() * sizeof(float3)) == 0);
        EXPECT(memcmp(mine.v.data(), twin.v.data(), mine.v.size() * sizeof(float3)) == 0);
        EXPECT(mine.nbs == twin.nbs);
        long counted = 0;
        for (int c : mine.nbs) counted += c;
        EXPECT(counted > 0);
        // the steps moved something
        std::vector<float3> start(N_MAX);
        seed_replica(0, start.data());
        EXPECT(memcmp(mine.X.data(), start.data(), counts[0] * sizeof(float3)) != 0);
    }
    (void)hipFree(d_strengths);
    printf(failures ? "%d FAILURES\n" : "ALL GABRIEL LDS STEP TESTS PASSED\n", failures);
    return failures != 0;
}
