// A time step and a Gabriel coefficient per replica (ya::ens::Replica_dt, Ensemble<Pt, Gabriel_solver>::
// d_gabriel_coefficients) as a model program uses the headers: the arrays live on the device, and BETWEEN two
// take_steps calls a kernel of the model halves d_dt[r] of every replica whose count exceeds a bound -- no copy, no
// synchronisation, the host never learns which.  The check is M lone Solutions, each stepped with its replica's values
// (the halved one where the host, which knows the counts, expects it): positions and old_v, memcmp-equal, for
// Ensemble<float3> and Ensemble<float3, Gabriel_solver>, on the launch-sequence path and from LDS.
#include "support.cuh"

__device__ float3 spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    return r * ((0.6f - dist) / dist);
}

constexpr int M = 6, N_MAX = 300, GRID_SIZE = 12, BOUND = 100, STEPS_BEFORE = 3, STEPS_AFTER = 2;
static const int counts[M] = {300, 0, 64, 257, 129, 3};
static const float dts[M] = {0.05f, 0.1f, 0.013f, 0.02f, 0.07f, 0.0f};
static const float coefficients[M] = {0.8f, 0.5f, 1.f, 0.65f, 0.8f, 0.9f};

// the model's adaptive-dt kernel: a crowded replica takes smaller steps from now on
__global__ void halve_dt_of_crowded_replicas(int n_replicas, const int* d_n, int bound, float* d_dt)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_replicas && d_n[r] > bound) d_dt[r] = 0.5f * d_dt[r];
}

static void seed_replica(int r, float3* rows) { seed_rows(12345u + 977u * (unsigned)r, counts[r], 3.f, 1.5f, rows); }

static State state_of(const float3* h_rows, const float3* d_old_v, int n)
{
    State out;
    out.n = n;
    out.X.assign(h_rows, h_rows + N_MAX);
    out.kind.assign(N_MAX, 0);  // (this model has neither kinds nor counters)
    out.nbs.assign(N_MAX, 0);
    out.v.resize(N_MAX);
    (void)hipMemcpy(out.v.data(), d_old_v, N_MAX * sizeof(float3), hipMemcpyDeviceToHost);
    return out;
}

template<typename Solo>
static State alone(Solo& cells, int r)
{
    *cells.h_n = counts[r];
    seed_replica(r, cells.h_X);
    cells.copy_to_device();
    for (int s = 0; s < STEPS_BEFORE; s++) cells.template take_step<spring>(dts[r]);
    const float later = counts[r] > BOUND ? 0.5f * dts[r] : dts[r];
    for (int s = 0; s < STEPS_AFTER; s++) cells.template take_step<spring>(later);
    cells.copy_to_host();
    return state_of(cells.h_X, cells.d_old_v, *cells.h_n);
}

template<typename Cells>
static std::vector<State> together(Cells& cells)
{
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        seed_replica(r, cells.row(r, 0));
    }
    cells.copy_to_device();
    float* d_dt = on_device(dts, M);
    cells.template take_steps<spring>(ya::ens::Replica_dt{d_dt}, STEPS_BEFORE);
    halve_dt_of_crowded_replicas<<<1, 64>>>(M, cells.d_n, BOUND, d_dt);
    cells.template take_steps<spring>(ya::ens::Replica_dt{d_dt}, STEPS_AFTER);
    // ... and only now does anything come back
    cells.copy_to_host();
    std::vector<State> out;
    for (int r = 0; r < M; r++) out.push_back(state_of(cells.row(r, 0), cells.d_old_v + cells.index(r, 0), cells.h_n[r]));
    (void)hipFree(d_dt);
    return out;
}

int main()
{
    std::vector<State> tile_alone, gabriel_alone;
    for (int r = 0; r < M; r++) {
        Solution<float3, Tile_solver> tile{N_MAX};
        tile_alone.push_back(alone(tile, r));
        Solution<float3, Gabriel_solver> gabriel{N_MAX, GRID_SIZE, 1.f, coefficients[r]};
        gabriel_alone.push_back(alone(gabriel, r));
    }
    // the steps moved something, and the two solvers' forces differ
    std::vector<float3> start(N_MAX);
    seed_replica(0, start.data());
    EXPECT(memcmp(tile_alone[0].X.data(), start.data(), counts[0] * sizeof(float3)) != 0);
    EXPECT(memcmp(tile_alone[0].X.data(), gabriel_alone[0].X.data(), counts[0] * sizeof(float3)) != 0);

    float* d_coefficients = on_device(coefficients, M);
    for (int from_lds : {-1, 1}) {
        Ensemble<float3> tile{M, N_MAX};
        tile.whole_steps = from_lds;
        compare(together(tile), tile_alone);
        EXPECT(tile.whole_step_launches == (from_lds > 0 ? 2 : 0));

        Ensemble<float3, Gabriel_solver> gabriel{M, N_MAX, GRID_SIZE, 1.f, 0.123f};  // (the scalar is ignored)
        gabriel.d_gabriel_coefficients = d_coefficients;
        gabriel.lds_steps = from_lds;
        compare(together(gabriel), gabriel_alone);
        EXPECT(gabriel.lds_step_launches == (from_lds > 0 ? 2 : 0));
        for (int r = 0; r < M; r++) EXPECT(gabriel.status(r) == 0);
    }
    (void)hipFree(d_coefficients);
    printf(failures ? "%d FAILURES\n" : "ALL REPLICA DT TESTS PASSED\n", failures);
    return failures != 0;
}
