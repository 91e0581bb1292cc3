// Ensemble<Pt, Grid_solver>::take_steps(dt, K, ya::ens::Replica_links) (include/ensemble_grid.cuh, ensemble_links.cuh)
// as a model program uses it: a protrusion sweep in the shape of the reference's intercalation model, on a grid.
//   * every cell owns prots_per_cell link slots; a kernel renews them before every call (deterministically: no random
//     numbers), sets the used-slot count on the device, and now and then leaves a link into ANOTHER replica or to an
//     unused row, which the ordered forces must skip;
//   * the pairwise functor reads its replica's strength via i / n_max and counts neighbours in a per-cell array without
//     atomics: it is not declared YA_STATELESS (one thread per cell);
//   * replicas divide on the device in between (d_n[r] changes);
//   * ONE Ensemble alternates take_steps(dt, K, Replica_links) -- from LDS -- with take_step(dt, gen) where gen calls
//     ya::ens::link_forces_ordered, the 14 launches on the same object.
// Everything -- positions and old_v of every row, the counts, the neighbour counters, the status and the three grid
// arrays -- is compared bit for bit with a twin Ensemble that never steps from LDS, in the three fixed modes and both
// summation orders, with 1 and 3 protrusions per cell.
#include "../native_ensemble/support.cuh"

using by_strength::counting_spring;  // (support.cuh: reads d_sweep, counts in d_n_nbs)

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

constexpr int M = 6, N_MAX = 300, GRID_SIZE = 12;
static const int counts[M] = {120, 0, 64, 257, 298, 3};   // (298 + 2 daughters: the replica ends full)
// (the sweep; the two large replicas get the soft springs: 298 cells in a box of 3 at strength 1.5 leave the grid)
static const float strengths[M] = {1.f, 0.75f, 1.5f, 0.75f, 0.5f, 2.f};

// What an ensemble holds at the end of a run, grid arrays included.
struct Grid_run {
    std::vector<float3> X, v;
    std::vector<int> n, nbs, cube_id, point_id, offs, status;
    long launches;
};

static Grid_run run(const float* d_strengths, const bool from_lds, const int fixed_mode, const int prots_per_cell,
    const int sum_order)
{
    const int S = N_MAX * prots_per_cell;
    Ensemble<float3, Grid_solver> cells{M, N_MAX, GRID_SIZE};
    cells.lds_steps = from_lds ? 1 : -1;
    cells.lds_steps_max = 2;
    cells.sum_order = sum_order ? YA_SUM_BY_PLANE : YA_SUM_REFERENCE;
    for (int r = 0; r < M; r++) {
        cells.h_n[r] = counts[r];
        for (int i = 0; i < N_MAX; i++) *cells.row(r, i) = float3{-7.25f, -7.25f, -7.25f};  // unused rows: a pattern
        seed_rows(12345u + 977u * (unsigned)r, counts[r], 3.f, 1.5f, cells.row(r, 0));
    }
    cells.copy_to_device();
    Property<int> nbs{M * N_MAX, "n_nbs"};
    for (int i = 0; i < M * N_MAX; i++) nbs.h_prop[i] = 0;
    nbs.copy_to_device();
    Links protrusions{M * S, 0.1f};
    point_model_at(d_strengths, nullptr, nbs.d_prop, N_MAX);

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
            cells.take_steps<counting_spring>(0.05f, 1, rl);                          // 5 launches if from LDS
        else
            cells.take_step<counting_spring>(0.05f, Generic_forces<float3>{gen});   // never
        if (step == 3 || step == 6) divide<<<(M + 63) / 64, 64>>>(M, N_MAX, cells.d_X, cells.d_old_v, cells.d_n);
    }
    cells.take_steps<counting_spring, friction_w_neighbour<float3>>(0.02f, 3, rl);  // 2 launches if from LDS

    Grid_run out;
    out.cube_id.resize(cells.rows());
    out.point_id.resize(cells.rows());
    out.offs.resize((size_t)M * (cells.n_cubes + 1));
    (void)hipMemcpy(out.cube_id.data(), cells.d_cube_id, out.cube_id.size() * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemcpy(out.point_id.data(), cells.d_point_id, out.point_id.size() * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemcpy(out.offs.data(), cells.d_offs, out.offs.size() * sizeof(int), hipMemcpyDeviceToHost);
    for (int r = 0; r < M; r++) out.status.push_back(cells.status(r));  // (first: copy_to_host aborts on a set bit)
    out.launches = cells.lds_step_launches;
    cells.copy_to_host();
    out.X.assign(cells.h_X, cells.h_X + cells.rows());
    out.v.resize(cells.rows());
    (void)hipMemcpy(out.v.data(), cells.d_old_v, out.v.size() * sizeof(float3), hipMemcpyDeviceToHost);
    nbs.copy_to_host();
    out.nbs.assign(nbs.h_prop, nbs.h_prop + cells.rows());
    for (int r = 0; r < M; r++) {
        out.n.push_back(cells.h_n[r]);
        EXPECT(cells.get_d_n(r) == cells.h_n[r]);
    }
    return out;
}

int main()
{
    static_assert(ya::ens::lds_layout<float3, true, true>(N_MAX, 3 * N_MAX, 1).bytes > 0, "the list of 3 protrusions per cell fits");
    static_assert(ya::ens::lds_layout<float3, true, true>(N_MAX, 3 * N_MAX, 1).bytes ==
                      ya::ens::lds_layout<float3, true, false>(N_MAX, 0, 1).bytes + 4 * (N_MAX + 1) + 8 * (3 * N_MAX),
        "the step's arrays, the keys, the list");
    static_assert(ya::ens::lds_layout<float3, true, true>(1024, 20000, 1).bytes == 0, "and a list beyond the LDS does not");
    static_assert(!ya::stateless_pair<float3, counting_spring, friction_w_neighbour<float3>>(), "not declared");
    float* d_strengths = on_device(strengths, M);
    for (int prots_per_cell : {1, 3}) {
        Grid_run first;
        for (int mode = 0; mode < 4; mode++) {  // the three fixed modes in the reference's order, then by plane
            const int fixed_mode = mode % 3, sum_order = mode / 3;
            const Grid_run twin = run(d_strengths, false, fixed_mode, prots_per_cell, sum_order);
            const Grid_run mixed = run(d_strengths, true, fixed_mode, prots_per_cell, sum_order);
            EXPECT(twin.launches == 0);
            EXPECT(mixed.launches == 5 + 2);
            for (int r = 0; r < M; r++) {
                EXPECT(twin.n[r] == counts[r] + (r % 2 == 0 && counts[r] > 0 ? 2 : 0));
                EXPECT(twin.status[r] == 0);
                if (twin.status[r]) {  // (which replica left its grid, and how far)
                    float far = 0.f;
                    for (int i = 0; i < twin.n[r]; i++) {
                        const float3 x = twin.X[(size_t)r * N_MAX + i];
                        far = fmaxf(far, fmaxf(fabsf(x.x), fmaxf(fabsf(x.y), fabsf(x.z))));
                    }
                    printf("  prots %d mode %d replica %d: status %d, farthest coordinate %g\n", prots_per_cell, mode, r,
                        twin.status[r], far);
                }
            }
            EXPECT(twin.n[4] == N_MAX);
            EXPECT(mixed.n == twin.n && mixed.status == twin.status);
            // every row, used or not, and every counter
            EXPECT(memcmp(mixed.X.data(), twin.X.data(), twin.X.size() * sizeof(float3)) == 0);
            EXPECT(memcmp(mixed.v.data(), twin.v.data(), twin.v.size() * sizeof(float3)) == 0);
            EXPECT(mixed.nbs == twin.nbs);
            // the grid arrays of the last stage's order (slots from a replica's count on are nobody's)
            EXPECT(mixed.offs == twin.offs);
            for (int r = 0; r < M; r++) {
                const size_t used = twin.n[r], at = (size_t)r * N_MAX;
                EXPECT(memcmp(mixed.cube_id.data() + at, twin.cube_id.data() + at, used * sizeof(int)) == 0);
                EXPECT(memcmp(mixed.point_id.data() + at, twin.point_id.data() + at, used * sizeof(int)) == 0);
            }
            long counted = 0;
            for (int c : twin.nbs) counted += c;
            EXPECT(counted > 0);
            for (const float3& x : twin.X) EXPECT(x.x == x.x && x.y == x.y && x.z == x.z);  // (no NaN went unnoticed)
            EXPECT(twin.X[(size_t)N_MAX + 5].y == -7.25f);  // (the empty replica's pattern is still there)
            if (mode == 0) first = twin;
        }
        // the links matter: with one protrusion per cell the same run ends elsewhere
        if (prots_per_cell == 3) {
            const Grid_run one = run(d_strengths, true, 0, 1, 0);
            EXPECT(memcmp(one.X.data(), first.X.data(), counts[0] * sizeof(float3)) != 0);
        }
    }
    (void)hipFree(d_strengths);
    printf(failures ? "%d FAILURES\n" : "ALL LINKED GRID LDS STEP TESTS PASSED\n", failures);
    return failures != 0;
}
