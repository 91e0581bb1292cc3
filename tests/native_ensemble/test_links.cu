// Ensemble<Pt, Tile_solver>::take_steps(dt, K, ya::ens::Replica_links) (include/ensemble.cuh, ensemble_links.cuh) as
// a model program uses it: a protrusion sweep in the shape of the reference's intercalation model.
//   * every cell owns prots_per_cell link slots; a kernel renews them before every step (deterministically: no
//     random numbers), sets the used-slot count on the device, and now and then leaves a link into ANOTHER replica
//     or to an unused row, which the ordered forces must skip;
//   * the pairwise functor reads its replica's rest length via i / n_max and counts neighbours in a per-cell array
//     without atomics: it is not declared YA_STATELESS, so a whole-step launch keeps one lane per cell;
//   * replicas divide on the device in between;
//   * ONE Ensemble alternates take_steps(dt, 1, Replica_links) -- whole-step launches -- with take_step(dt, gen)
//     where gen calls ya::ens::link_forces_ordered.
// Everything -- positions, old_v, counts, the neighbour counters -- is compared bit for bit with a twin Ensemble
// that only ever takes the six-launch ordered path, in the three fixed modes, with 1 and 3 protrusions per cell.
// Last, replicas of at most 40 cells under the default lanes: the counting functor keeps one lane per cell (and its
// counters), the same force declared YA_STATELESS gets 4, the bits are the twin's either way.
#include "support.cuh"

using by_rest::counting_spring;  // (support.cuh: reads d_sweep, counts in d_n_nbs)

// The same force without the counter, and declared stateless: under the default the engine may give it several lanes.
__device__ float3 plain_spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    const float L = d_sweep[i / d_rows_per_replica];
    return r * ((L - dist) / dist);
}
YA_STATELESS(float3, plain_spring)

// One thread per link slot, as the reference's update_protrusions: slot s of replica r belongs to cell
// (s % S) / prots_per_cell and now links it to a partner that depends on the step -- or to itself (inert), or, for
// two slots of every replica, to a cell of the NEXT replica and to the row just past the replica's count.
__global__ void update_protrusions(int n_replicas, int n_max, int prots_per_cell, int step, const int* d_n,
    Link* d_link, int* d_n_links)
{
    const int S = n_max * prots_per_cell;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0) *d_n_links = n_replicas * S - 2 * (step % 3);  // (the last slots fall out of use now and then)
    if (s >= n_replicas * S) return;
    const int r = s / S, k = s % S;
    const int n = d_n[r];
    const int base = r * n_max;
    const int cell = k / prots_per_cell;
    if (cell >= n) {
        d_link[s] = Link{cell % 5, cell % 5};  // (inert, whatever the id)
        return;
    }
    const int partner = (cell * 7 + step * 13 + (k % prots_per_cell) * 31 + 1) % n;
    Link l{base + cell, base + partner};       // (partner == cell: inert)
    if ((k + step) % 2) l = Link{l.b, l.a};
    if (k == 5) l.b = ((r + 1) % n_replicas) * n_max;   // into another replica: skipped
    if (k == 9) l.a = base + n;                         // an unused row (or the next replica's first): skipped
    d_link[s] = l;
}

constexpr int M = 6, N_MAX = 300;
static const int counts[M] = {120, 0, 64, 257, 298, 3};   // (298 + 2 daughters: the replica ends full)
static const float rests[M] = {0.5f, 0.55f, 0.6f, 0.65f, 0.7f, 0.75f};

static Run run(const float* d_rests, const bool whole, const int fixed_mode, const int prots_per_cell)
{
    const int S = N_MAX * prots_per_cell;
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
    Links protrusions{M * S, 0.1f};
    point_model_at(d_rests, nullptr, nbs.d_prop, N_MAX);

    if (fixed_mode == 1) cells.set_fixed(2);
    if (fixed_mode == 2) cells.set_fixed_xy(1);
    const ya::ens::Replica_links rl{protrusions, S};
    auto gen = [&](const int n, const float3* __restrict__ d_X, float3* d_dX) {
        ya::ens::link_forces_ordered<float3>(rl, n, N_MAX, cells.d_n, d_X, d_dX);
    };
    for (int step = 0; step < 9; step++) {
        update_protrusions<<<(M * S + 255) / 256, 256>>>(
            M, N_MAX, prots_per_cell, step, cells.d_n, protrusions.d_link, protrusions.d_n);
        if (step % 2 == 0)
            cells.take_steps<counting_spring>(0.05f, 1, rl);                          // 5 launches if whole
        else
            cells.take_step<counting_spring>(0.05f, Generic_forces<float3>{gen});   // never
        if (step == 3 || step == 6) divide<<<(M + 63) / 64, 64>>>(M, N_MAX, cells.d_X, cells.d_old_v, cells.d_n);
    }
    cells.take_steps<counting_spring, friction_w_neighbour<float3>>(0.02f, 3, rl);  // 2 launches if whole

    return read_back(cells, &nbs);
}

// Replicas of at most 40 cells, where ya::ens::whole_step_lanes_for gives a stateless functor 4 lanes per cell: the
// sweep above in short, whole_step_lanes left at its default.
constexpr int SMALL_M = 5, SMALL_N_MAX = 40, SMALL_PROTS = 2;
static const int small_counts[SMALL_M] = {40, 0, 17, 33, 1};

template<Pairwise_interaction<float3> force>
static Run small_run(const float* d_rests, const bool whole)
{
    const int S = SMALL_N_MAX * SMALL_PROTS;
    Ensemble<float3> cells{SMALL_M, SMALL_N_MAX};
    cells.whole_steps = whole ? 1 : -1;
    for (int r = 0; r < SMALL_M; r++) {
        cells.h_n[r] = small_counts[r];
        unsigned s = 99u + 31u * (unsigned)r;
        for (int i = 0; i < small_counts[r]; i++) {
            float x[3];
            for (float& c : x) {
                s = s * 1664525u + 1013904223u;
                c = 1.6f * (float)(s >> 8) / 16777216.f;
            }
            *cells.row(r, i) = float3{x[0], x[1], x[2]};
        }
    }
    cells.copy_to_device();
    Property<int> nbs{SMALL_M * SMALL_N_MAX, "n_nbs"};
    for (int i = 0; i < SMALL_M * SMALL_N_MAX; i++) nbs.h_prop[i] = 0;
    nbs.copy_to_device();
    Links protrusions{SMALL_M * S, 0.1f};
    point_model_at(d_rests, nullptr, nbs.d_prop, SMALL_N_MAX);
    const ya::ens::Replica_links rl{protrusions, S};
    for (int step = 0; step < 4; step++) {
        update_protrusions<<<(SMALL_M * S + 255) / 256, 256>>>(
            SMALL_M, SMALL_N_MAX, SMALL_PROTS, step, cells.d_n, protrusions.d_link, protrusions.d_n);
        cells.take_steps<force>(0.05f, 1, rl);   // 4 launches if whole
    }
    cells.take_steps<force>(0.02f, 3, rl);       // 1 launch if whole
    return read_back(cells, &nbs);
}

int main()
{
    static_assert(ya::ens::lds_layout<float3, false, true>(N_MAX, 3 * N_MAX, 1).bytes > 0, "the list of 3 protrusions per cell fits");
    static_assert(ya::ens::lds_layout<float3, false, true>(N_MAX, 3 * N_MAX, 1).bytes % 16 == 0, "16-byte aligned");
    static_assert(ya::ens::lds_layout<float3, false, true>(1024, 20000, 1).bytes == 0, "and a list beyond the LDS does not");
    float* d_rests = on_device(rests, M);
    for (int prots_per_cell : {1, 3}) {
        Run first;
        for (int fixed_mode : {0, 1, 2}) {
            const Run twin = run(d_rests, false, fixed_mode, prots_per_cell);
            const Run mixed = run(d_rests, true, fixed_mode, prots_per_cell);
            EXPECT(twin.launches == 0 && twin.lanes_used == 0);
            EXPECT(mixed.launches == 5 + 2);
            EXPECT(mixed.lanes_used == 1);  // (the functor is not declared stateless)
            for (int r = 0; r < M; r++) {
                EXPECT(twin.n[r] == counts[r] + (r % 2 == 0 && counts[r] > 0 ? 2 : 0));
                EXPECT(mixed.n[r] == twin.n[r]);
            }
            EXPECT(twin.n[4] == N_MAX);
            // every row, used or not, and every counter
            EXPECT(memcmp(mixed.X.data(), twin.X.data(), twin.X.size() * sizeof(float3)) == 0);
            EXPECT(memcmp(mixed.v.data(), twin.v.data(), twin.v.size() * sizeof(float3)) == 0);
            EXPECT(memcmp(mixed.nbs.data(), twin.nbs.data(), twin.nbs.size() * sizeof(int)) == 0);
            long counted = 0;
            for (int c : twin.nbs) counted += c;
            EXPECT(counted > 0);
            for (const float3& x : twin.X) EXPECT(x.x == x.x && x.y == x.y && x.z == x.z);  // (no NaN went unnoticed)
            if (fixed_mode == 0) first = twin;
        }
        // the links matter: with one protrusion per cell the same run ends elsewhere
        if (prots_per_cell == 3) {
            const Run one = run(d_rests, true, 0, 1);
            EXPECT(memcmp(one.X.data(), first.X.data(), counts[0] * sizeof(float3)) != 0);
        }
    }
    {
        // The default lanes at 40 cells.  A functor that is NOT declared stateless keeps one lane per cell -- with
        // several, its plain `d_n_nbs[i] += 1` would lose counts -- and leaves every counter as the six-launch twin
        // does; the same force declared stateless gets 4 lanes, and the same bits.
        static_assert(ya::ens::whole_step_lanes_for(SMALL_N_MAX) == 4, "a stateless functor gets 4 lanes at 40 cells");
        static_assert(!ya::stateless_pair<float3, counting_spring, friction_w_neighbour<float3>>(), "not declared");
        static_assert(ya::stateless_pair<float3, plain_spring, friction_w_neighbour<float3>>(), "declared");
        const Run twin = small_run<counting_spring>(d_rests, false);
        const Run counting = small_run<counting_spring>(d_rests, true);
        const Run plain = small_run<plain_spring>(d_rests, true);
        EXPECT(twin.launches == 0 && counting.launches == 5 && plain.launches == 5);
        EXPECT(counting.lanes_used == 1);
        EXPECT(plain.lanes_used == 4);
        EXPECT(memcmp(counting.X.data(), twin.X.data(), twin.X.size() * sizeof(float3)) == 0);
        EXPECT(memcmp(counting.v.data(), twin.v.data(), twin.v.size() * sizeof(float3)) == 0);
        EXPECT(memcmp(counting.nbs.data(), twin.nbs.data(), twin.nbs.size() * sizeof(int)) == 0);
        EXPECT(memcmp(plain.X.data(), twin.X.data(), twin.X.size() * sizeof(float3)) == 0);
        EXPECT(memcmp(plain.v.data(), twin.v.data(), twin.v.size() * sizeof(float3)) == 0);
        long counted = 0;
        for (int c : twin.nbs) counted += c;
        EXPECT(counted > 0);
        for (int c : plain.nbs) EXPECT(c == 0);
        for (const float3& x : twin.X) EXPECT(x.x == x.x && x.y == x.y && x.z == x.z);
    }
    (void)hipFree(d_rests);
    printf(failures ? "%d FAILURES\n" : "ALL LINKED WHOLE-STEP TESTS PASSED\n", failures);
    return failures != 0;
}
