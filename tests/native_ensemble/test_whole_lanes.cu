// Ensemble<Pt, Tile_solver>::whole_step_lanes (include/ensemble.cuh) as a model program uses it: several lanes per
// cell inside a whole-step launch (ya::ens::whole_steps_coop).
//   * a functor declared YA_STATELESS records WHICH LANES called it for a cell (atomicOr of bit threadIdx.x into a
//     256-bit mask per cell, nothing else): the bits of a step cannot show that the new stage ran, the masks do;
//   * a functor that is NOT declared stateless and counts neighbours without atomics keeps one lane per cell under
//     the default, and its counters are those of a twin that only calls take_step;
//   * a MAKE_PT type of 8 floats leaves no room for the terms of 16 lanes at n_max = 1024: one lane per cell, still
//     whole-step launches; the largest n_max at which 16 lanes fit comes from ya::ens::lds_layout;
//   * ONE Ensemble alternates take_steps with 16 lanes per cell with take_step carrying Links, a kernel bumping
//     d_n[r] in between, against a twin that only calls take_step.
// Every comparison is of bit patterns.
#include "support.cuh"

// ---- 1. which lanes called the functor ---------------------------------------------------------------------------
__device__ unsigned* d_lane_mask;  // [cell][8]: bit t of a cell's 256 = thread t of a workgroup called the functor for it

__device__ float3 lanes_seen(float3 Xi, float3 r, float dist, int i, int j)
{
    atomicOr(&d_lane_mask[8 * (size_t)i + threadIdx.x / 32], 1u << (threadIdx.x % 32));
    return float3{0.f, 0.f, 0.f};
}
YA_STATELESS(float3, lanes_seen)

// Replicas of n_max, n_max - 1, ..., 0 cells (and a lone cell), 2 steps in two launches with `setting` lanes per
// cell.  With L lanes per cell, cell `local` is cell local % (256 / L) of its round and owns threads
// [L * that, L * that + L); of those the first min(L, n) find a partner.
static void lanes_case(const int n_max, const int setting, const int expected)
{
    const int M = n_max + 2;
    Ensemble<float3> cells{M, n_max};
    cells.whole_steps = 1;
    cells.steps_per_launch = 1;
    cells.whole_step_lanes = setting;
    EXPECT(cells.whole_step_lanes_used == 0);
    unsigned s = 99u + (unsigned)n_max;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = r <= n_max ? n_max - r : 1;
        for (int i = 0; i < cells.h_n[r]; i++) *cells.row(r, i) = float3{next_float(s), next_float(s), next_float(s)};
    }
    cells.copy_to_device();
    Property<unsigned> mask{8 * M * n_max, "lane_mask"};
    for (int k = 0; k < 8 * M * n_max; k++) mask.h_prop[k] = 0;
    mask.copy_to_device();
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_lane_mask), &mask.d_prop, sizeof(mask.d_prop));
    cells.take_steps<lanes_seen>(0.05f, 2);
    EXPECT(cells.whole_step_launches == 2);
    EXPECT(cells.whole_step_lanes_used == expected);
    mask.copy_to_host();
    const int L = expected, per_round = 256 / L;
    int wrong = 0;
    for (int r = 0; r < M; r++) {
        const int n = cells.h_n[r];
        for (int local = 0; local < n_max; local++) {
            const unsigned* got = mask.h_prop + 8 * cells.index(r, local);
            unsigned want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (local < n) {
                const int first = L * (local % per_round), busy = L < n ? L : n;
                for (int t = first; t < first + busy; t++) want[t / 32] |= 1u << (t % 32);
            }
            if (memcmp(got, want, sizeof(want)) != 0) wrong++;
        }
    }
    if (wrong) printf("n_max %d, whole_step_lanes %d: %d cells with other lanes than %d per cell\n", n_max, setting, wrong, L);
    EXPECT(wrong == 0);
}

// ---- 2. per-cell state without atomics: one lane per cell under the default -------------------------------------------
__device__ float3 counting_spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    d_n_nbs[i] += 1;  // <- not declared stateless
    return r * ((0.6f - dist) / dist);
}

struct Counted {
    std::vector<float3> X;
    std::vector<int> nbs;
    long launches;
    int lanes_used;
};
static Counted counting_run(const bool whole)
{
    constexpr int M = 6, N_MAX = 40;  // (a stateless functor would get 4 lanes per cell at 40 cells)
    const int counts[M] = {40, 39, 0, 17, 1, 5};
    Ensemble<float3> cells{M, N_MAX};
    cells.whole_steps = whole ? 1 : -1;
    unsigned s = 7u;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        for (int i = 0; i < counts[r]; i++)
            *cells.row(r, i) = float3{2.f * next_float(s), 2.f * next_float(s), 2.f * next_float(s)};
    }
    cells.copy_to_device();
    Property<int> nbs{M * N_MAX, "n_nbs"};
    for (int i = 0; i < M * N_MAX; i++) nbs.h_prop[i] = 0;
    nbs.copy_to_device();
    point_model_at(nullptr, nullptr, nbs.d_prop, N_MAX);
    EXPECT(cells.whole_step_lanes == 0);
    if (whole)
        cells.take_steps<counting_spring>(0.05f, 3);
    else
        for (int k = 0; k < 3; k++) cells.take_step<counting_spring>(0.05f);
    Counted out;
    cells.copy_to_host();
    nbs.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + M * N_MAX);
    out.nbs.assign(nbs.h_prop, nbs.h_prop + M * N_MAX);
    out.launches = cells.whole_step_launches;
    out.lanes_used = cells.whole_step_lanes_used;
    return out;
}

// ---- 3. a point type of 8 floats: the term buffer does not always fit ----------------------------------------------
MAKE_PT(Pt8, a, b, c, d, e);
static_assert(sizeof(Pt8) == 32, "8 floats");

__device__ Pt8 spring8(Pt8 Xi, Pt8 r, float dist, int i, int j)
{
    Pt8 dF = ya::zero<Pt8>();
    if (i == j || dist >= 1.f) return dF;
    const float F = (0.6f - dist) / dist;
    dF.x = r.x * F;
    dF.y = r.y * F;
    dF.z = r.z * F;
    dF.a = -0.1f * r.a;
    dF.c = 0.05f * r.c * dist;
    dF.e = 0.01f * Xi.e;
    return dF;
}
YA_STATELESS(Pt8, spring8)

// the largest n_max at which the terms of 16 lanes per cell still fit beside a Pt8 replica, by the header's own rule
constexpr int largest_pt8_with_16_lanes()
{
    int best = 0;
    for (int n_max = 1; n_max <= ya::ens::whole_step_capacity<Pt8>(); n_max++)
        if (ya::ens::lds_layout<Pt8, false, false>(n_max, 0, 16).bytes != 0) best = n_max;
    return best;
}

struct Rows8 {
    std::vector<Pt8> X;
    std::vector<float3> v;
    long launches;
    int lanes_used;
};
static Rows8 pt8_run(const int n_max, const bool whole)
{
    constexpr int M = 3;
    const int counts[M] = {n_max, 65, n_max - 1};
    Ensemble<Pt8> cells{M, n_max};
    cells.whole_steps = whole ? 1 : -1;
    cells.whole_step_lanes = 16;
    unsigned s = 31u;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        const float side = 1.f + 0.012f * (float)counts[r];
        for (int i = 0; i < counts[r]; i++) {
            Pt8* p = cells.row(r, i);
            for (int k = 0; k < 8; k++) ya::field(*p, k) = (k < 3 ? side : 1.f) * next_float(s);
        }
    }
    cells.copy_to_device();
    if (whole)
        cells.take_steps<spring8>(0.05f, 2);
    else
        for (int k = 0; k < 2; k++) cells.take_step<spring8>(0.05f);
    Rows8 out;
    cells.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + (size_t)M * n_max);
    out.v.resize((size_t)M * n_max);
    (void)hipMemcpy(out.v.data(), cells.d_old_v, out.v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    out.launches = cells.whole_step_launches;
    out.lanes_used = cells.whole_step_lanes_used;
    return out;
}
static void pt8_case(const int n_max, const int lanes_expected)
{
    const Rows8 twin = pt8_run(n_max, false), whole = pt8_run(n_max, true);
    EXPECT(twin.launches == 0 && twin.lanes_used == 0);
    EXPECT(whole.launches == 1);
    if (whole.lanes_used != lanes_expected) printf("Pt8, n_max %d: %d lanes per cell\n", n_max, whole.lanes_used);
    EXPECT(whole.lanes_used == lanes_expected);
    EXPECT(memcmp(whole.X.data(), twin.X.data(), twin.X.size() * sizeof(Pt8)) == 0);
    EXPECT(memcmp(whole.v.data(), twin.v.data(), twin.v.size() * sizeof(float3)) == 0);
}

// ---- 4. whole-step launches with 16 lanes per cell alternate with linked steps ------------------------------------
__device__ float3 sweep_spring(float3 Xi, float3 r, float dist, int i, int j)
{
    float3 dF{0.f, 0.f, 0.f};
    if (i == j || dist >= 1.f) return dF;
    const float L = d_sweep[i / d_rows_per_replica];  // <- the sweep: this replica's parameter
    return r * ((L - dist) / dist);
}
YA_STATELESS(float3, sweep_spring)

constexpr int M = 7, N_MAX = 130;
static const int counts[M] = {100, 0, 64, 17, 97, 3, 128};  // (128 + 2 daughters: the replica ends full)
static const float rests[M] = {0.5f, 0.55f, 0.6f, 0.65f, 0.7f, 0.75f, 0.8f};

static Run alternating_run(const float* d_rests, const bool whole, const int fixed_mode)
{
    Ensemble<float3> cells{M, N_MAX};
    cells.whole_steps = whole ? 1 : -1;
    cells.whole_step_lanes = 16;
    cells.steps_per_launch = 2;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        seed_rows(r, counts[r], cells.row(r, 0));
    }
    cells.copy_to_device();
    Links links{M * N_MAX, 0.3f};
    int n_links = 0;
    for (int r = 0; r < M; r++)
        for (int k = 0; k < n_links_of(counts[r]); k++)
            links.h_link[n_links++] = Link{(int)cells.index(r, 2 * k), (int)cells.index(r, 2 * k + 1)};
    *links.h_n = n_links;
    links.copy_to_device();
    point_model_at(d_rests, nullptr, nullptr, N_MAX);

    if (fixed_mode == 1) cells.set_fixed(2);
    if (fixed_mode == 2) cells.set_fixed_xy(1);
    auto gen = [&links](const int, const float3* __restrict__ d_X, float3* d_dX) { link_forces<float3>(links, d_X, d_dX); };
    auto quiet = [&](float dt, int n_steps) {
        if (whole)
            cells.take_steps<sweep_spring>(dt, n_steps);
        else
            for (int s = 0; s < n_steps; s++) cells.take_step<sweep_spring>(dt);
    };
    auto linked = [&](float dt) { cells.take_step<sweep_spring>(dt, Generic_forces<float3>{gen}); };
    quiet(0.05f, 3);  // 2 launches
    linked(0.05f);
    quiet(0.05f, 1);  // 1 launch
    linked(0.02f);
    divide<<<(M + 63) / 64, 64>>>(M, N_MAX, cells.d_X, cells.d_old_v, cells.d_n);
    quiet(0.02f, 5);  // 3 launches
    divide<<<(M + 63) / 64, 64>>>(M, N_MAX, cells.d_X, cells.d_old_v, cells.d_n);
    linked(0.05f);
    quiet(0.05f, 2);  // 1 launch
    if (whole) EXPECT(cells.whole_step_lanes_used == 16);

    return read_back(cells);
}

int main()
{
    // 1. the lanes that ran: forced ...
    for (int lanes : {1, 4, 16, 64}) {
        lanes_case(3, lanes, lanes);    // n < L
        lanes_case(70, lanes, lanes);   // several rounds (4 and 16 lanes), partial rounds
    }
    lanes_case(300, 64, 64);            // several tiles
    lanes_case(300, 4, 4);
    // ... and by the engine's rule: the largest L of 64, 16, 4 with n_max * L <= 256, else 1
    static_assert(ya::ens::whole_step_lanes_for(4) == 64 && ya::ens::whole_step_lanes_for(5) == 16, "");
    static_assert(ya::ens::whole_step_lanes_for(16) == 16 && ya::ens::whole_step_lanes_for(17) == 4, "");
    static_assert(ya::ens::whole_step_lanes_for(64) == 4 && ya::ens::whole_step_lanes_for(65) == 1, "");
    for (int n_max : {1, 4, 5, 16, 17, 64, 65}) lanes_case(n_max, 0, ya::ens::whole_step_lanes_for(n_max));

    // 2. a functor that is not declared stateless keeps one lane per cell, and its counters
    {
        const Counted twin = counting_run(false), whole = counting_run(true);
        EXPECT(twin.launches == 0 && whole.launches == 1);
        EXPECT(whole.lanes_used == 1);
        EXPECT(memcmp(whole.X.data(), twin.X.data(), twin.X.size() * sizeof(float3)) == 0);
        EXPECT(memcmp(whole.nbs.data(), twin.nbs.data(), twin.nbs.size() * sizeof(int)) == 0);
        long counted = 0;
        for (int c : twin.nbs) counted += c;
        EXPECT(counted > 0);
    }

    // 3. 8 floats per point
    {
        static_assert(ya::ens::whole_step_capacity<Pt8>() == 1024, "Pt8 replicas of up to 1024 cells fit");
        static_assert(ya::ens::lds_layout<Pt8, false, false>(1024, 0, 16).bytes == 0, "but not with the terms of 16 lanes");
        constexpr int fits = largest_pt8_with_16_lanes();
        static_assert(fits > 64 && fits < 1024, "");
        static_assert(ya::ens::lds_layout<Pt8, false, false>(fits, 0, 16).tile >= 16, "");
        static_assert(ya::ens::lds_layout<Pt8, false, false>(fits, 0, 16).bytes + ya::ens::WHOLE_STEP_STATIC_LDS <=
                          ya::ens::LDS_PER_WORKGROUP, "");
        pt8_case(1024, 1);
        pt8_case(fits, 16);
        pt8_case(fits + 1, 1);
    }

    // 4. alternation, in all three fixed modes
    {
        float* d_rests = on_device(rests, M);
        for (int fixed_mode : {0, 1, 2}) {
            const Run twin = alternating_run(d_rests, false, fixed_mode);
            const Run mixed = alternating_run(d_rests, true, fixed_mode);
            EXPECT(twin.launches == 0);
            EXPECT(mixed.launches == 2 + 1 + 3 + 1);
            for (int r = 0; r < M; r++) {
                EXPECT(twin.n[r] == counts[r] + (r % 2 == 0 && counts[r] > 0 ? 2 : 0));
                EXPECT(mixed.n[r] == twin.n[r]);
            }
            EXPECT(twin.n[6] == N_MAX);
            EXPECT(memcmp(mixed.X.data(), twin.X.data(), twin.X.size() * sizeof(float3)) == 0);
            EXPECT(memcmp(mixed.v.data(), twin.v.data(), twin.v.size() * sizeof(float3)) == 0);
        }
        (void)hipFree(d_rests);
    }
    printf(failures ? "%d FAILURES\n" : "ALL WHOLE-STEP LANES TESTS PASSED\n", failures);
    return failures != 0;
}
