// Ensemble<Pt, Grid_solver>::lds_step_lanes (include/ensemble_grid.cuh) as a model program uses it: several lanes per
// cell inside the launches that step from LDS (ya::ens::grid_lds_walk_coop).
//   1. a functor declared YA_STATELESS records WHICH LANES called it for a cell (atomicOr of bit threadIdx.x into a
//      256-bit mask per cell) and counts its calls per (i, j): forced lanes and the rule under 0 show more than one
//      lane per cell, all of them the lanes of the cell's slot, and every candidate inside the cut-off is evaluated
//      exactly once per stage, as with one lane;
//   2. a functor that is NOT declared stateless and counts neighbours with a plain `d_n_nbs[i] += 1` keeps one lane per
//      cell under the default, and its counters are those of a twin that only calls take_step;
//   3. a MAKE_PT type of 8 floats: at n_max = 1024 the term buffer has no room (one lane, still from LDS); at the
//      largest n_max the rule admits for 16 lanes, read from the constexpr, 16 lanes run; one beyond, one lane.
// Every comparison is of bit patterns.
#include "../native_ensemble/support.cuh"

// ---- 1. which lanes called the functor, and how often per pair -------------------------------------------------------
__device__ unsigned* d_lane_mask;  // [cell][8]: bit t of a cell's 256 = thread t of the workgroup called the functor for it
__device__ int* d_pair_calls;      // [cell i][local id of j]
__device__ int d_pair_rows;        // n_max

__device__ float3 lanes_seen(float3 Xi, float3 r, float dist, int i, int j)
{
    atomicOr(&d_lane_mask[8 * (size_t)i + threadIdx.x / 32], 1u << (threadIdx.x % 32));
    atomicAdd(&d_pair_calls[(size_t)i * d_pair_rows + j % d_pair_rows], 1);
    return float3{0.f, 0.f, 0.f};
}
YA_STATELESS(float3, lanes_seen)

struct Seen {
    std::vector<unsigned> mask;
    std::vector<int> calls, point_id;
};
// Replicas of n_max, n_max - 1, ..., 0 cells in a box where a cell has several neighbours inside the cut-off; one step
// (two stages) in one launch.  The force is zero, so nobody moves and both stages see the same candidates.
static Seen lanes_run(const int n_max, const int setting, const int expected)
{
    const int M = n_max + 1, GS = 6;
    Ensemble<float3, Grid_solver> cells{M, n_max, GS};
    cells.lds_steps = 1;
    cells.lds_step_lanes = setting;
    EXPECT(cells.lds_step_lanes_used == 0);
    unsigned s = 99u + (unsigned)n_max;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = n_max - r;
        for (int i = 0; i < cells.h_n[r]; i++)
            *cells.row(r, i) = float3{2.4f * next_float(s) - 1.2f, 2.4f * next_float(s) - 1.2f, 2.4f * next_float(s) - 1.2f};
    }
    cells.copy_to_device();
    Property<unsigned> mask{8 * M * n_max, "lane_mask"};
    Property<int> calls{M * n_max * n_max, "pair_calls"};
    for (int k = 0; k < 8 * M * n_max; k++) mask.h_prop[k] = 0;
    for (int k = 0; k < M * n_max * n_max; k++) calls.h_prop[k] = 0;
    mask.copy_to_device();
    calls.copy_to_device();
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_lane_mask), &mask.d_prop, sizeof(mask.d_prop));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_pair_calls), &calls.d_prop, sizeof(calls.d_prop));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_pair_rows), &n_max, sizeof(int));
    cells.take_steps<lanes_seen>(0.05f, 1);
    EXPECT(cells.lds_step_launches == 1);
    EXPECT(cells.lds_step_lanes_used == expected);
    mask.copy_to_host();
    calls.copy_to_host();
    Seen out;
    out.mask.assign(mask.h_prop, mask.h_prop + 8 * M * n_max);
    out.calls.assign(calls.h_prop, calls.h_prop + M * n_max * n_max);
    out.point_id.resize((size_t)M * n_max);
    (void)hipMemcpy(out.point_id.data(), cells.d_point_id, out.point_id.size() * sizeof(int), hipMemcpyDeviceToHost);
    for (int r = 0; r < M; r++) EXPECT(cells.status(r) == 0);
    return out;
}
static int bits_of(const unsigned* mask)
{
    int count = 0;
    for (int w = 0; w < 8; w++) count += __builtin_popcount(mask[w]);
    return count;
}
static void lanes_case(const int n_max, const int setting, const int expected, const Seen& one_lane)
{
    const Seen seen = lanes_run(n_max, setting, expected);
    const int M = n_max + 1, L = expected, per_round = 256 / L;
    // every candidate inside the cut-off exactly once per stage: the one-lane walk's calls, 0 or 2 each, 2 for i == j
    EXPECT(seen.calls == one_lane.calls);
    int wrong = 0, several = 0, cells_with_pairs = 0;
    for (int r = 0; r < M; r++) {
        const int n = n_max - r;
        for (int slot = 0; slot < n; slot++) {
            const int local = seen.point_id[(size_t)r * n_max + slot];
            if (local != one_lane.point_id[(size_t)r * n_max + slot]) wrong++;
            const size_t i = (size_t)r * n_max + local;
            int pairs = 0;
            for (int j = 0; j < n_max; j++) {
                const int c = seen.calls[i * n_max + j];
                if (c != 0 && c != 2) wrong++;
                if (j == local && c != 2) wrong++;
                pairs += c / 2;
            }
            // the lanes that called the functor for this cell are lanes of ITS slot: [L * (slot % per_round), + L)
            const unsigned* got = seen.mask.data() + 8 * i;
            const int first = L * (slot % per_round);
            for (int t = 0; t < 256; t++)
                if (((got[t / 32] >> (t % 32)) & 1u) && (t < first || t >= first + L)) wrong++;
            if (bits_of(got) < 1 || bits_of(got) > (pairs < L ? pairs : L)) wrong++;
            if (pairs >= 2) cells_with_pairs++;
            if (bits_of(got) >= 2) several++;
        }
    }
    if (wrong) printf("n_max %d, lds_step_lanes %d: %d wrong cells or pairs\n", n_max, setting, wrong);
    EXPECT(wrong == 0);
    EXPECT(cells_with_pairs > 0);
    EXPECT(L == 1 ? several == 0 : several > 0);  // more than one lane per cell
}

// ---- 2. per-cell state without atomics: one lane per cell under the default -------------------------------------------
using by_strength::counting_spring;

struct Counted {
    std::vector<float3> X;
    std::vector<int> nbs;
    long launches;
    int lanes_used;
};
static Counted counting_run(const float* d_strengths, const bool from_lds)
{
    constexpr int M = 6, N_MAX = 40, GS = 8;  // (a stateless functor would get 4 lanes per cell at 40 cells)
    const int counts[M] = {40, 39, 0, 17, 1, 5};
    Ensemble<float3, Grid_solver> cells{M, N_MAX, GS};
    cells.lds_steps = from_lds ? 1 : -1;
    unsigned s = 7u;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        for (int i = 0; i < counts[r]; i++)
            *cells.row(r, i) = float3{2.f * next_float(s) - 1.f, 2.f * next_float(s) - 1.f, 2.f * next_float(s) - 1.f};
    }
    cells.copy_to_device();
    Property<int> nbs{M * N_MAX, "n_nbs"};
    for (int i = 0; i < M * N_MAX; i++) nbs.h_prop[i] = 0;
    nbs.copy_to_device();
    point_model_at(d_strengths, nullptr, nbs.d_prop, N_MAX);
    EXPECT(cells.lds_step_lanes == 0);
    if (from_lds)
        cells.take_steps<counting_spring>(0.05f, 3);
    else
        for (int k = 0; k < 3; k++) cells.take_step<counting_spring>(0.05f);
    Counted out;
    for (int r = 0; r < M; r++) EXPECT(cells.status(r) == 0);
    cells.copy_to_host();
    nbs.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + M * N_MAX);
    out.nbs.assign(nbs.h_prop, nbs.h_prop + M * N_MAX);
    out.launches = cells.lds_step_launches;
    out.lanes_used = cells.lds_step_lanes_used;
    return out;
}

// ---- 3. a point type of 8 floats ------------------------------------------------------------------------------------
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

constexpr int largest_n_max_with_lanes(const int lanes)
{
    int rows = 0;
    for (int n = 1; n <= ya::ens::WHOLE_STEP_MAX_ROWS; n++)
        if (ya::ens::lds_layout<Pt8, true, false>(n, 0, lanes).bytes != 0) rows = n;
    return rows;
}

struct Rows8 {
    std::vector<Pt8> X;
    std::vector<float3> v;
    std::vector<int> cube_id, point_id, offs, status;
    long launches;
    int lanes_used;
};
static Rows8 pt8_run(const int n_max, const int lds_steps, const int lanes)
{
    constexpr int M8 = 3, GS = 14;
    const int n8[M8] = {n_max, 65, n_max - 1};
    Ensemble<Pt8, Grid_solver> cells{M8, n_max, GS};
    cells.lds_steps = lds_steps;
    cells.lds_step_lanes = lanes;
    unsigned s = 31u;
    for (int r = 0; r < M8; r++) {
        cells.h_n[r] = n8[r];
        const float side = 1.f + 0.008f * (float)n8[r];  // (well inside the 14^3 grid)
        for (int i = 0; i < n8[r]; i++) {
            Pt8* p = cells.row(r, i);
            for (int k = 0; k < 8; k++) ya::field(*p, k) = k < 3 ? side * (next_float(s) - 0.5f) : next_float(s);
        }
    }
    cells.copy_to_device();
    cells.take_steps<spring8>(0.05f, 2);
    Rows8 out;
    out.cube_id.resize(cells.rows());
    out.point_id.resize(cells.rows());
    out.offs.resize((size_t)M8 * (cells.n_cubes + 1));
    (void)hipMemcpy(out.cube_id.data(), cells.d_cube_id, out.cube_id.size() * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemcpy(out.point_id.data(), cells.d_point_id, out.point_id.size() * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemcpy(out.offs.data(), cells.d_offs, out.offs.size() * sizeof(int), hipMemcpyDeviceToHost);
    for (int r = 0; r < M8; r++) out.status.push_back(cells.status(r));
    // (slots from a replica's count on are nobody's)
    for (int r = 0; r < M8; r++)
        for (int slot = n8[r]; slot < n_max; slot++) out.cube_id[(size_t)r * n_max + slot] = out.point_id[(size_t)r * n_max + slot] = -1;
    cells.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + (size_t)M8 * n_max);
    out.v.resize((size_t)M8 * n_max);
    (void)hipMemcpy(out.v.data(), cells.d_old_v, out.v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    out.launches = cells.lds_step_launches;
    out.lanes_used = cells.lds_step_lanes_used;
    return out;
}
static void pt8_case(const int n_max, const int lanes, const int used_expected)
{
    const Rows8 twin = pt8_run(n_max, -1, lanes), lds = pt8_run(n_max, 1, lanes);
    EXPECT(twin.launches == 0 && twin.lanes_used == 0);
    EXPECT(lds.launches == 1);
    EXPECT(lds.lanes_used == used_expected);
    EXPECT(memcmp(twin.X.data(), lds.X.data(), twin.X.size() * sizeof(Pt8)) == 0);
    EXPECT(memcmp(twin.v.data(), lds.v.data(), twin.v.size() * sizeof(float3)) == 0);
    for (int s : twin.status) EXPECT(s == 0);
    EXPECT(twin.status == lds.status && twin.offs == lds.offs && twin.cube_id == lds.cube_id && twin.point_id == lds.point_id);
}

int main()
{
    // 1: 40 and 20 cells, where the rule under 0 gives 4 and 16 lanes
    {
        const Seen one = lanes_run(20, 1, 1);
        lanes_case(20, 1, 1, one);
        lanes_case(20, 4, 4, one);
        lanes_case(20, 16, 16, one);
        lanes_case(20, 64, 64, one);
        lanes_case(20, 0, 16, one);
        static_assert(ya::ens::grid_lds_lanes_for(20) == 16 && ya::ens::grid_lds_lanes_for(32) == 16, "");
        static_assert(ya::ens::grid_lds_lanes_for(33) == 4 && ya::ens::grid_lds_lanes_for(64) == 4, "");
        static_assert(ya::ens::grid_lds_lanes_for(4) == 16 && ya::ens::grid_lds_lanes_for(65) == 1, "");
        const Seen forty = lanes_run(40, 1, 1);
        lanes_case(40, 0, 4, forty);
    }
    // 2
    {
        const float strengths[6] = {0.5f, 0.75f, 1.f, 1.25f, 1.5f, 2.f};
        float* d_strengths = on_device(strengths, 6);
        const Counted twin = counting_run(d_strengths, false), lds = counting_run(d_strengths, true);
        EXPECT(twin.launches == 0 && twin.lanes_used == 0);
        EXPECT(lds.launches == 1 && lds.lanes_used == 1);
        EXPECT(memcmp(twin.X.data(), lds.X.data(), twin.X.size() * sizeof(float3)) == 0);
        EXPECT(twin.nbs == lds.nbs);
        long counted = 0;
        for (int c : twin.nbs) counted += c;
        EXPECT(counted > 0);
        (void)hipFree(d_strengths);
    }
    // 3
    {
        static_assert(ya::ens::grid_lds_capacity<Pt8>() == 1024, "");
        static_assert(ya::ens::lds_layout<Pt8, true, false>(1024, 0, 4).bytes == 0 &&
                          ya::ens::lds_layout<Pt8, true, false>(1024, 0, 16).bytes == 0 &&
                          ya::ens::lds_layout<Pt8, true, false>(1024, 0, 64).bytes == 0,
            "896 bytes: no room for 16 candidates' terms");
        constexpr int largest = largest_n_max_with_lanes(16);
        static_assert(largest == 942, "tests/test_ensemble_grid_lds_lanes_abi.py names the same point");
        static_assert(ya::ens::lds_layout<Pt8, true, false>(largest, 0, 16).tile == 16, "the shortest tile");
        static_assert(ya::ens::lds_layout<Pt8, true, false>(largest, 0, 16).bytes + ya::ens::WHOLE_STEP_STATIC_LDS <= ya::ens::LDS_PER_WORKGROUP, "");
        pt8_case(1024, 16, 1);
        pt8_case(largest, 16, 16);
        pt8_case(largest + 1, 16, 1);
    }
    printf(failures ? "%d FAILURES\n" : "ALL GRID LDS LANES TESTS PASSED\n", failures);
    return failures != 0;
}
