// Ensemble<Pt, Grid_solver>::take_steps as launches that step from LDS (include/ensemble_grid.cuh, lds_steps), as a
// model program uses the header.  Every comparison is a memcmp against a TWIN: an Ensemble of the same rows that only
// ever calls take_step (the 14 launches).
//   1. a sweep on ONE ensemble that alternates take_steps(dt, 4) -- from LDS -- with take_step(dt, link forces) -- the
//      14 launches, on the same object -- and division on the device (a kernel raises d_n[r]); every row, old_v, the
//      counts, the kinds, the status and the three grid arrays;
//   2. a functor that counts neighbours with a plain `d_n_nbs[i] += 1` by global id, not declared stateless: its
//      counters equal the twin's, which shows one thread per cell;
//   3. a MAKE_PT type of 8 floats at its grid_lds_capacity (read from the constexpr) and one row beyond it.
#include "../native_ensemble/support.cuh"

using by_strength::counting_spring;
using by_strength::sweep_spring;

constexpr int M = 6, N_MAX = 400, GRID_SIZE = 12, ROUNDS = 3;
static const int counts[M] = {300, 0, 64, 257, 129, 3};
static const float strengths[M] = {0.5f, 0.75f, 1.f, 1.25f, 1.5f, 2.f};

static void seed_replica(int r, float3* rows) { seed_rows(12345u + 977u * (unsigned)r, counts[r], 3.f, 1.5f, rows); }

// What an ensemble holds at the end of a run, grid arrays included.
struct Grid_run {
    std::vector<float3> X, v;
    std::vector<int> n, kind, nbs, cube_id, point_id, offs, status;
    long launches;
};
template<typename Pt>
static void read_grids(Ensemble<Pt, Grid_solver>& cells, Grid_run& out)
{
    out.cube_id.resize(cells.rows());
    out.point_id.resize(cells.rows());
    out.offs.resize((size_t)cells.n_replicas * (cells.n_cubes + 1));
    (void)hipMemcpy(out.cube_id.data(), cells.d_cube_id, out.cube_id.size() * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemcpy(out.point_id.data(), cells.d_point_id, out.point_id.size() * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemcpy(out.offs.data(), cells.d_offs, out.offs.size() * sizeof(int), hipMemcpyDeviceToHost);
    for (int r = 0; r < cells.n_replicas; r++) out.status.push_back(cells.status(r));
    out.launches = cells.lds_step_launches;
}
// (slots from a replica's count on are nobody's)
static void expect_same_grids(const Grid_run& a, const Grid_run& b, int n_max)
{
    EXPECT(a.n == b.n && a.status == b.status && a.offs == b.offs);
    for (size_t r = 0; r < a.n.size(); r++) {
        const size_t used = a.n[r] > 0 ? a.n[r] : 0;
        EXPECT(memcmp(a.cube_id.data() + r * n_max, b.cube_id.data() + r * n_max, used * sizeof(int)) == 0);
        EXPECT(memcmp(a.point_id.data() + r * n_max, b.point_id.data() + r * n_max, used * sizeof(int)) == 0);
    }
}

// ---- 1 and 2 -------------------------------------------------------------------------------------------------------
static Grid_run sweep(const float* d_strengths, const bool from_lds, const bool counting, const int sum_order)
{
    Ensemble<float3, Grid_solver> cells{M, N_MAX, GRID_SIZE};
    cells.lds_steps = from_lds ? 1 : -1;
    cells.sum_order = sum_order ? YA_SUM_BY_PLANE : YA_SUM_REFERENCE;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        for (int i = 0; i < N_MAX; i++) *cells.row(r, i) = float3{-7.25f, -7.25f, -7.25f};  // unused rows: a pattern
        seed_replica(r, cells.row(r, 0));
    }
    cells.copy_to_device();
    Property<int> kind{M * N_MAX, "kind"}, nbs{M * N_MAX, "nbs"};
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
    auto gen = [&links](const int, const float3* __restrict__ d_X, float3* d_dX) { link_forces<float3>(links, d_X, d_dX); };

    for (int round = 0; round < ROUNDS; round++) {
        const float dt = round < 2 ? 0.05f : 0.02f;
        // four steps without generic forces: from LDS, or (the twin) four calls of take_step
        if (from_lds) {
            if (counting)
                cells.take_steps<counting_spring>(dt, 4);
            else
                cells.take_steps<sweep_spring>(dt, 4);
        } else {
            for (int k = 0; k < 4; k++) {
                if (counting)
                    cells.take_step<counting_spring>(dt);
                else
                    cells.take_step<sweep_spring>(dt);
            }
        }
        // one step with the link forces: the 14 launches on both sides, on the same object
        if (counting)
            cells.take_step<counting_spring>(dt, Generic_forces<float3>{gen});
        else
            cells.take_step<sweep_spring>(dt, Generic_forces<float3>{gen});
        if (round == 1) cells.set_fixed_xy(2);
        divide<<<(M + 63) / 64, 64>>>(M, N_MAX, 0, cells.d_X, cells.d_old_v, cells.d_n, kind.d_prop);
    }
    // (the last thing a run does is a step of each kind, so both kinds of grid arrays get compared over the runs)
    if (sum_order == 1) {
        if (from_lds)
            cells.take_steps<sweep_spring>(0.02f, 2);
        else
            for (int k = 0; k < 2; k++) cells.take_step<sweep_spring>(0.02f);
    }

    Grid_run out;
    read_grids(cells, out);  // (the status first: copy_to_host aborts on a replica that left its grid)
    cells.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + cells.rows());
    out.v.resize(cells.rows());
    (void)hipMemcpy(out.v.data(), cells.d_old_v, out.v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    kind.copy_to_host();
    nbs.copy_to_host();
    out.kind.assign(kind.h_prop, kind.h_prop + cells.rows());
    out.nbs.assign(nbs.h_prop, nbs.h_prop + cells.rows());
    for (int r = 0; r < M; r++) {
        out.n.push_back(cells.h_n[r]);
        EXPECT(cells.get_d_n(r) == cells.h_n[r]);
    }
    return out;
}

static void sweep_case(const float* d_strengths, const bool counting, const int sum_order)
{
    const Grid_run twin = sweep(d_strengths, false, counting, sum_order), lds = sweep(d_strengths, true, counting, sum_order);
    EXPECT(twin.launches == 0);
    EXPECT(lds.launches == ROUNDS + (sum_order == 1 ? 1 : 0));
    // the replicas that divide grew every round, the others and the empty one did not
    for (int r = 0; r < M; r++) EXPECT(twin.n[r] == counts[r] + (r % 2 == 0 && counts[r] > 0 ? ROUNDS : 0));
    for (int r = 0; r < M; r++) EXPECT(twin.status[r] == 0);
    EXPECT(memcmp(twin.X.data(), lds.X.data(), twin.X.size() * sizeof(float3)) == 0);  // every row, used or not
    EXPECT(memcmp(twin.v.data(), lds.v.data(), twin.v.size() * sizeof(float3)) == 0);
    EXPECT(twin.kind == lds.kind);
    EXPECT(twin.nbs == lds.nbs);
    expect_same_grids(twin, lds, N_MAX);
    long counted = 0;
    for (int c : twin.nbs) counted += c;
    EXPECT((counted > 0) == counting);
    EXPECT(twin.X[(size_t)N_MAX - 1].x == -7.25f && twin.X[(size_t)N_MAX + 5].y == -7.25f);  // (the pattern is still there)
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

struct Rows8 {
    std::vector<Pt8> X;
    std::vector<float3> v;
    Grid_run grids;
};
static Rows8 pt8_run(const int n_max, const bool from_lds)
{
    constexpr int M8 = 3, GS = 14;
    const int n8[M8] = {n_max, 65, n_max - 1};
    Ensemble<Pt8, Grid_solver> cells{M8, n_max, GS};
    cells.lds_steps = from_lds ? 1 : -1;
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
    read_grids(cells, out.grids);
    cells.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + (size_t)M8 * n_max);
    out.v.resize((size_t)M8 * n_max);
    (void)hipMemcpy(out.v.data(), cells.d_old_v, out.v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    for (int r = 0; r < M8; r++) out.grids.n.push_back(cells.h_n[r]);
    return out;
}
static void pt8_case(const int n_max, const long launches_expected)
{
    const Rows8 twin = pt8_run(n_max, false), lds = pt8_run(n_max, true);
    EXPECT(twin.grids.launches == 0);
    EXPECT(lds.grids.launches == launches_expected);
    EXPECT(memcmp(twin.X.data(), lds.X.data(), twin.X.size() * sizeof(Pt8)) == 0);
    EXPECT(memcmp(twin.v.data(), lds.v.data(), twin.v.size() * sizeof(float3)) == 0);
    for (int s : twin.grids.status) EXPECT(s == 0);
    expect_same_grids(twin.grids, lds.grids, n_max);
}

int main()
{
    float* d_strengths = on_device(strengths, M);
    for (int sum_order : {0, 1}) sweep_case(d_strengths, false, sum_order);
    sweep_case(d_strengths, true, 0);  // the neighbour counter
    (void)hipFree(d_strengths);

    constexpr int capacity = ya::ens::grid_lds_capacity<Pt8>();
    static_assert(capacity >= 256 && capacity <= ya::ens::WHOLE_STEP_MAX_ROWS, "a replica of 8-float points fits");
    static_assert(ya::ens::lds_layout<Pt8, true, false>(capacity, 0, 1).bytes + ya::ens::WHOLE_STEP_STATIC_LDS <= ya::ens::LDS_PER_WORKGROUP, "");
    static_assert(ya::ens::grid_lds_capacity<float3>() == ya::ens::WHOLE_STEP_MAX_ROWS, "");
    pt8_case(capacity, 1);
    pt8_case(capacity + 1, 0);  // one row beyond: the 14 launches, the same bits

    printf(failures ? "%d FAILURES\n" : "ALL GRID LDS STEP TESTS PASSED\n", failures);
    return failures != 0;
}
