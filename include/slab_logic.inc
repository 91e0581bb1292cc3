// z-slab decomposition of Grid_solver over ranks (SURVEY.md section 8e): the part that is the
// same on every backend.  Included by include/slab.cuh (HIP engine: Slab_grid_solver) and by
// the CPU oracle's model harness (test infrastructure), after the respective solvers header,
// so it only uses names both define: Heun_solver, Grid_computer, Generic_forces and the
// protected stage_* / begin_build members.  `Ops` supplies memory and the few Pt-agnostic
// device operations (ordered selection, row gathers, appending messages): ya::Slab_device_ops
// over the C ABI of include/yalla_hip.h on the device.  This file carries no backend #ifdef:
// what only one backend has -- streams, events and RCCL on the device; the serial COM sum and
// guard update on the oracle -- sits behind Ops calls or `if constexpr (Ops::device)`.
//
// New relative to the reference, which is single-GPU.
#pragma once

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "yalla_models.h"  // ya_slab_exchange_fn, ya_slab_allreduce_fn

#include <algorithm>
#include <vector>

// ---- decomposing a system (host side, backend independent) --------------------------------
// Cut planes, message capacities and array sizes for `world` z-slabs of the cells in h_X.
// What yalla_amd/slab.py used to do in numpy (round 1-2): now every C++ model program and
// the bench share this one statement.
namespace ya {
struct Slab_plan {
    int world = 1;
    float halo = 0;                 // ghost layer: cube_size * (1 + margin)
    std::vector<float> bounds;      // world + 1 planes; rank r owns z in [bounds[r], bounds[r + 1])
    std::vector<int> n_own;         // cells per rank in the state the plan was made from
    std::vector<int> n_ghost;       // ghost cells per rank in that state (both faces)
    int halo_cap = 0, mig_cap = 0;  // message capacities in cells, the same on every rank
    int n_max = 0;                  // local arrays: any rank's own + ghost + arriving cells
    int error = 0;                  // -9: an interior slab is thinner than the ghost layer
};

// Cut planes for `world` z-slabs of the cells whose z coordinates, ascending, are in `z`.
//
// Round 4: the cuts balance what a rank's step costs, own + ghost_weight * mirrored cells, instead
// of the own cells alone (rounds 1-3: the z-quantiles).  A slab in the middle of a ball mirrors two
// full cross-sections (0.30 M cells beside 1.25 M own ones at 10 M cells in 8 slabs), an end slab one
// small cap (0.10 M); the force launches cost by the own cell (0.47 ns), the grid builds, updates and
// reductions by the local one (0.16 ns: profiles/r04_slab_rehearsal_10M_w8_device_time.json), so a
// mirrored cell weighs 0.16 / (0.47 + 0.16) ~ 0.26 of an own one and the end slabs can take 4 % more
// own cells than the middle ones.  The partition is the classic one: the smallest bound T such that
// a greedy walk -- every slab as many cells as fit under T -- gets through (bisection on T).
// A cut lies at a cell's z (the slab above begins with that cell), anywhere between the grid's
// planes: cuts snapped to cube-plane boundaries, so that no plane of cubes holds own AND mirrored
// cells, were built and measured too (commit 9702081) and bought nothing -- a plane is 120 000
// cells at 10 M, far too coarse a step for the balance, and the tiles of a shared plane cost no more
// than those of a full one.  ghost_weight = 0 (or YALLA_SLAB_PLAN=quantile in the environment) gives
// the z-quantiles.  Capacities come from the fullest ghost layer of the state times `slack` (both
// ends of a message must agree on its size, so they are global).
inline Slab_plan slab_plan_sorted(const std::vector<float>& z, const int world, const float cube_size,
    const float margin = 0.25f, const float slack = 1.15f, float ghost_weight = 0.26f)
{
    Slab_plan plan;
    const int n = (int)z.size();
    plan.world = world;
    plan.halo = cube_size * (1.0f + margin);
    plan.bounds.assign(world + 1, 0.f);
    plan.bounds[0] = -INFINITY;
    plan.bounds[world] = INFINITY;
    auto below = [&](float v) { return (int)(std::lower_bound(z.begin(), z.end(), v) - z.begin()); };
    if (const char* mode = getenv("YALLA_SLAB_PLAN"))
        if (mode[0] == 'q') ghost_weight = 0.f;

    // cut[r] = index of the first cell of slab r in z[]; cut[0] = 0, cut[world] = n
    std::vector<int> cut(world + 1, 0), best;
    for (int r = 0; r <= world; r++) cut[r] = (int)((long long)n * r / world);  // the quantiles
    best = cut;
    if (ghost_weight > 0.f && world > 1 && n >= world) {
        // the slab of cells [a, b): its own cells and those within halo beyond its faces z[a], z[b]
        auto cost = [&](int a, int b) {
            double ghosts = 0;
            if (a > 0) ghosts += a - below(z[a] - plan.halo);
            if (b < n) ghosts += below(z[b] + plan.halo) - b;
            return (double)(b - a) + ghost_weight * ghosts;
        };
        auto fits = [&](double T) {
            cut[0] = 0;
            for (int r = 0; r + 1 < world; r++) {
                const int a = cut[r];
                // the largest b with cost(a, b) <= T (the cost grows with b but for the little the
                // ghost layer above changes: bisection), leaving a cell for every slab above
                int lo = a + 1, hi = n - (world - 1 - r);
                if (lo > hi || cost(a, lo) > T) return false;
                while (lo < hi) {
                    const int mid = lo + (hi - lo + 1) / 2;
                    if (cost(a, mid) <= T) lo = mid; else hi = mid - 1;
                }
                cut[r + 1] = lo;
            }
            cut[world] = n;
            return cost(cut[world - 1], n) <= T;
        };
        double lo = 0, hi = (double)n * (1.0 + 2.0 * ghost_weight) + 1.0;
        if (fits(hi)) {
            best = cut;
            for (int it = 0; it < 50; it++) {
                const double mid = 0.5 * (lo + hi);
                if (fits(mid)) {
                    hi = mid;
                    best = cut;
                } else
                    lo = mid;
            }
        }
    }
    for (int r = 1; r < world; r++) plan.bounds[r] = z[(size_t)std::min(best[r], n - 1)];
    for (int r = 1; r + 1 < world; r++)
        if ((double)plan.bounds[r + 1] - (double)plan.bounds[r] < plan.halo) plan.error = -9;
    int fullest = 0;
    plan.n_own.assign(world, 0);
    plan.n_ghost.assign(world, 0);
    for (int r = 0; r < world; r++) {
        const int lo = r == 0 ? 0 : below(plan.bounds[r]), hi = r + 1 == world ? n : below(plan.bounds[r + 1]);
        plan.n_own[r] = hi - lo;
        if (r > 0) {  // the face at bounds[r]: layers [f - halo, f) and [f, f + halo)
            const float f = plan.bounds[r];
            const int under = below(f) - below(f - plan.halo), over = below(f + plan.halo) - below(f);
            fullest = std::max(fullest, std::max(under, over));
            plan.n_ghost[r] += under;
            plan.n_ghost[r - 1] += over;
        }
    }
    plan.halo_cap = (int)(fullest * slack) + 64;
    plan.mig_cap = plan.halo_cap / 4 + 64;
    const int most = *std::max_element(plan.n_own.begin(), plan.n_own.end());
    plan.n_max = (int)(most * slack) + 2 * plan.halo_cap + 2 * plan.mig_cap + 64;
    return plan;
}

template<typename Pt>
Slab_plan slab_plan(const Pt* h_X, const int n, const int world, const float cube_size,
    const float margin = 0.25f, const float slack = 1.15f, const float ghost_weight = 0.26f)
{
    std::vector<float> z((size_t)n);
    for (int i = 0; i < n; i++) z[i] = h_X[i].z;
    std::sort(z.begin(), z.end());
    return slab_plan_sorted(z, world, cube_size, margin, slack, ghost_weight);
}

// Rank `rank`'s own cells of the whole system, in ascending global id: positions into `out`
// (room for plan.n_own[rank]), their global ids into `gid`.  Returns the count.
template<typename Pt>
int slab_own_cells(const Slab_plan& plan, const int rank, const Pt* h_X, const int n, Pt* out, int* gid)
{
    const float z_lo = plan.bounds[rank], z_hi = plan.bounds[rank + 1];
    int k = 0;
    for (int i = 0; i < n; i++)
        if (h_X[i].z >= z_lo && h_X[i].z < z_hi) {
            out[k] = h_X[i];
            gid[k++] = i;
        }
    return k;
}
}  // namespace ya

template<typename Pt, typename Ops>
class Slab_grid_solver_impl : public Heun_solver<Pt, Grid_computer> {
public:
    template<typename... Args>
    Slab_grid_solver_impl(int n_max, Args... args) : Heun_solver<Pt, Grid_computer>{n_max, args...}
    {}
    Slab_grid_solver_impl(const Slab_grid_solver_impl&) = delete;

    // ---- z-slab decomposition (SURVEY.md §8e; new relative to the reference) ----
    // Local arrays hold the own cells in [0, n_own) and the ghost cells received
    // from the slab neighbours in [n_own, n_local).  Messages are fixed-capacity
    // device buffers: 16-byte header {int count}, then `cap` rows of each field.
    static constexpr size_t P = sizeof(Pt);
    static constexpr size_t HEADER = 16;
    struct Slab_state {
        bool on = false;
        float z_lo = 0, z_hi = 0, halo = 0;
        int n_own = 0, n_local = 0;
        // the own cells the neighbour below [0] / above [1] mirrors: selected by rehalo()
        int *d_idx[2] = {nullptr, nullptr}, *d_count = nullptr, *d_ws = nullptr;
        int* d_counts_in = nullptr;  // received and sent cell counts, staged for one host read
        int* d_n_local = nullptr;    // own + ghost cells, as counted on the device
        int ghosts[2] = {0, 0};      // mirrored cells of the neighbour below / above: local [n_own, n_local)
        int sent[2] = {0, 0};        // own cells mirrored by the neighbour below / above (d_idx[0 / 1])
        int msg_in[2] = {0, 0};      // rows the neighbour below / above sends per stage: ghosts[] unless this rank
                                     // could not keep its mirrored cells (-5), see unpack_halo_state
        bool halo_valid = false;     // false: ownership changed, the next step starts with rehalo()
        char* send_dx[2] = {nullptr, nullptr};  // a stage's right-hand sides of those cells, P bytes each
        void *comm_stream = nullptr, *rhs_packed = nullptr, *rhs_landed = nullptr;  // device build: hipStream_t, 2 x hipEvent_t
        int *d_gid = nullptr, *d_gid_tmp = nullptr;
        float* d_fix = nullptr;  // host backend: the stage's fixed velocity (the device's update kernels work it out)
        // drift guard (see guard_between_stages): z of own and mirrored cells when the mirrored cells were
        // chosen, the per-workgroup maxima the update kernels leave, {moved, predicted, request, error}
        float *d_z_selected = nullptr, *d_moved_partial = nullptr, *d_pred_partial = nullptr, *d_guard = nullptr;
        int n_moved_partials = 0, n_pred_partials = 0;
        bool guard = true;             // false: as rounds 1-3, nothing checks the drift
        float guard_lag_steps = 2.5f;  // a vote cast in step k is on the host when step k + 1 begins, which then
                                       // migrates and re-selects first: only step k's second stage runs on the old
                                       // selection after the vote (moved + 2 predicted; + 25 % for a pace that grows)
        void* votes = nullptr;         // Ops::Votes: the all-reduced votes on their way to the host
        bool votes_pending = false, migrate_requested = false;
        int* d_fix_index = nullptr;    // set_fixed(i) / set_fixed_xy(i): local index of cell i, or -1 (not this rank's)
        int failed = 0;                // sticky: this rank's first failure (it keeps stepping until every rank knows)
        long rehalos = 0, guard_requests = 0;  // statistics: selections of the mirrored cells / those the guard asked for
        // Local order.  A rank's LOCAL cell indices are nobody's business but the engine's (functors see
        // the global ids of d_gid), so every this-many-th selection begins by putting the own cells
        // into cube order (Heun_solver::renumber with d_gid in tow): the first stage's gathers by
        // index (k_bin, k_order) and the force kernel's scatter of dX then walk memory nearly in
        // sequence.  0 = never (the order cells were adopted and migrated in: random in space).
        int local_order_every = 1;
        // one-process-per-rank stepping (slab_step): this rank's place, its message buffers
        // and how they travel
        int rank = 0, world = 1, halo_cap = 0, mig_cap = 0;
        char *send_halo[2] = {nullptr, nullptr}, *recv_halo[2] = {nullptr, nullptr};
        char *send_mig[2] = {nullptr, nullptr}, *recv_mig[2] = {nullptr, nullptr};
        float* d_sum = nullptr;
        ya_slab_exchange_fn exchange = nullptr;
        ya_slab_allreduce_fn allreduce = nullptr;
        void* transport_ctx = nullptr;
        void* rccl = nullptr;  // ya_comm* (device build)
    } slab;
    ~Slab_grid_solver_impl()
    {
        if (!slab.on) return;
        Ops::release(slab.d_idx[0]);
        Ops::release(slab.d_idx[1]);
        Ops::release(slab.d_count);
        Ops::release(slab.d_counts_in);
        Ops::release(slab.d_n_local);
        Ops::release(slab.d_ws);
        Ops::release(slab.d_gid);
        Ops::release(slab.d_gid_tmp);
        Ops::release(slab.d_fix);
        Ops::release(slab.d_z_selected);
        Ops::release(slab.d_moved_partial);
        Ops::release(slab.d_pred_partial);
        Ops::release(slab.d_guard);
        Ops::release(slab.d_fix_index);
        Ops::votes_destroy(slab.votes);
        for (int d = 0; d < 2; d++) {
            Ops::release(slab.send_halo[d]);
            Ops::release(slab.recv_halo[d]);
            Ops::release(slab.send_mig[d]);
            Ops::release(slab.recv_mig[d]);
            Ops::release(slab.send_dx[d]);
        }
        Ops::release(slab.d_sum);
        Ops::rows_path_destroy(slab.comm_stream, slab.rhs_packed, slab.rhs_landed);
    }
    // halo message: header, X (or X1), old_v, global id; migration message: X, old_v, global id
    static long halo_bytes(int cap) { return (long)(HEADER + (size_t)cap * (P + 12 + 4)); }
    static long migrate_bytes(int cap) { return (long)(HEADER + (size_t)cap * (P + 12 + 4)); }

    int slab_init(float z_lo, float z_hi, float halo, const int* gid, int n_own)
    {
        if (slab.on || n_own < 0 || n_own > this->n_max) return -3;
        const size_t ints = (size_t)this->n_max * sizeof(int);
        slab.d_idx[0] = (int*)Ops::alloc(ints);
        slab.d_idx[1] = (int*)Ops::alloc(ints);
        slab.d_count = (int*)Ops::alloc(16);  // [0], [1]: per direction; [2]: scratch
        slab.d_counts_in = (int*)Ops::alloc(32);
        slab.d_n_local = (int*)Ops::alloc(16);
        slab.d_ws = (int*)Ops::alloc(Ops::select_workspace_bytes(this->n_max));
        slab.d_gid = (int*)Ops::alloc(ints);
        slab.d_gid_tmp = (int*)Ops::alloc(ints);
        slab.d_fix = (float*)Ops::alloc(16);
        slab.d_z_selected = (float*)Ops::alloc((size_t)this->n_max * sizeof(float));
        const size_t partials = (size_t)std::max(this->n_max / 256 + 2, 1024) * sizeof(float);
        slab.d_moved_partial = (float*)Ops::alloc(partials);
        slab.d_pred_partial = (float*)Ops::alloc(partials);
        Ops::zero(slab.d_moved_partial, partials);
        Ops::zero(slab.d_pred_partial, partials);
        slab.d_guard = (float*)Ops::alloc(16);
        Ops::zero(slab.d_guard, 16);
        slab.d_fix_index = (int*)Ops::alloc(16);
        Ops::write_int(slab.d_fix_index, -1);
        slab.votes = Ops::votes_create();
        slab.z_lo = z_lo;
        slab.z_hi = z_hi;
        slab.halo = halo;
        slab.n_own = slab.n_local = n_own;
        Ops::h2d(slab.d_gid, gid, (size_t)slab.n_own * sizeof(int));
        // pairwise functors are called with global ids from now on (sorting.cu:24 `i < n / 2`,
        // branching.cu:82 `d_type[i]`: per-cell model arrays are indexed by the undivided id)
        this->d_global_id = slab.d_gid;
        slab.on = true;
        return 0;
    }
    Pt* stage_rhs_array(int stage) { return stage == 1 ? this->d_dX : this->d_dX1; }
    // Solution::renumber (new ids in cube order) would have to rename the cells on every rank that
    // mirrors them: not offered inside a decomposition.
    template<typename... Arrays>
    void renumber(Arrays&... arrays)
    {
        if (slab.on) {
            fprintf(stderr, "yalla-hip: Solution::renumber is not available inside a z-slab decomposition\n");
            abort();
        }
        Heun_solver<Pt, Grid_computer>::renumber(arrays...);
    }

    // ---- the ghost layer -----------------------------------------------------------------
    // Ghost cells are MIRRORED: a rank keeps the full state {X, old_v, global id} of its
    // neighbours' cells within `halo` of the shared face and advances them with the same
    // update kernels as its own cells.  What it cannot compute itself is their right-hand side:
    // per Heun stage the owner sends dX of exactly those cells, nothing else (stage_exchange).
    // Positions therefore never wait for a message, a stage's grid build needs no exchange,
    // and the one message of a stage travels while the interior tiles' forces are computed.
    // The set of mirrored cells is chosen anew whenever ownership changes (rehalo(), after every
    // migration): between two such events a cell may drift at most (halo - cube_size) / 2, the
    // margin the decomposition has always asked for (strays of the owner's cells AND of the
    // selection).
    // a cell's record: the point, old_v, the global id (one launch moves all three)
    void cell_arrays(void* arrays[3], size_t row_bytes[3])
    {
        arrays[0] = this->d_X;
        arrays[1] = this->d_old_v;
        arrays[2] = slab.d_gid;
        row_bytes[0] = P;
        row_bytes[1] = 12;
        row_bytes[2] = 4;
    }
    int pack_halo_state(int dir, void* buf, int cap)
    {
        if (!slab.on || !buf || dir < 0 || dir > 1) return -3;
        int* count = slab.d_count + dir;
        const float inf = INFINITY;
        const float z_min = dir == 0 ? -inf : slab.z_hi - slab.halo;
        const float z_max = dir == 0 ? slab.z_lo + slab.halo : inf;
        Ops::select_z(this->d_X, P, slab.n_own, z_min, z_max, slab.d_idx[dir], count, slab.d_ws);
        void* arrays[3];
        size_t row_bytes[3];
        cell_arrays(arrays, row_bytes);
        Ops::pack_cells(arrays, row_bytes, slab.d_idx[dir], count, cap, buf, HEADER);
        return 0;
    }
    // returns the local cell count own + ghosts.  A ghost layer that outgrew its message (-4) or the
    // local arrays (-5) makes this rank FAIL (slab.failed): it keeps going with what fits, so that
    // every rank learns of it through the next all-reduce and all of them stop in the same step.
    // -5 (no room for mirrored cells: none are kept) must not change what travels: the neighbours
    // did mirror THIS rank's cells and will send their own cells' rows each stage as agreed, so
    // slab.sent[] stays what was selected and slab.msg_in[] what the state messages announced --
    // the rows that come in are taken into the idle state buffers instead of the right-hand side
    // array (stage_exchange).  With sizes that differ between the two ends RCCL's send / recv pairs
    // would not match and the ranks would hang before the vote is ever summed.
    int unpack_halo_state(const void* buf_lo, const void* buf_hi, int cap)
    {
        if (!slab.on) return -3;
        const void* bufs[2] = {buf_lo, buf_hi};
        const void* keep[2] = {buf_lo, buf_hi};
        const int n_bound = slab.n_own + (bufs[0] ? cap : 0) + (bufs[1] ? cap : 0);
        if (n_bound > this->n_max) {
            if (!slab.failed) slab.failed = -5;
            keep[0] = keep[1] = nullptr;  // no room for mirrored cells
        }
        void* arrays[3];
        size_t row_bytes[3];
        cell_arrays(arrays, row_bytes);
        // {received from below, received from above} as sent, then {sent down, sent up}: one read
        Ops::append_cells(arrays, row_bytes, slab.n_own, keep[0], keep[1], cap, HEADER, slab.d_n_local, slab.d_counts_in);
        Ops::copy(slab.d_counts_in + 2, slab.d_count, 2 * sizeof(int));
        int counts[4] = {0, 0, 0, 0};
        Ops::read_ints(slab.d_counts_in, 4, counts);
        int n = slab.n_own;
        for (int d = 0; d < 2; d++) {
            int announced = counts[d];
            if (bufs[d] && !keep[d]) Ops::read_ints(static_cast<const int*>(bufs[d]), 1, &announced);  // the message's own count
            slab.msg_in[d] = bufs[d] ? announced : 0;
            slab.sent[d] = bufs[d] ? counts[2 + d] : 0;
            if (slab.msg_in[d] < 0 || slab.msg_in[d] > cap || slab.sent[d] > cap) {  // a ghost layer outgrew its message
                if (!slab.failed) slab.failed = -4;
                slab.msg_in[d] = std::min(std::max(slab.msg_in[d], 0), cap);  // (what the kernels above and
                slab.sent[d] = std::min(slab.sent[d], cap);                    //  the gathers clamp to as well)
            }
            slab.ghosts[d] = keep[d] ? slab.msg_in[d] : 0;
            n += slab.ghosts[d];
        }
        slab.n_local = n;
        return n;
    }
    // The cube ids that bound the tiles launched first in a stage (Grid_computer::force_part):
    // every own cell whose right-hand side a neighbour waits for lies in a z-plane at or below
    // the plane of z_lo + halo + margin, or at or above that of z_hi - halo - margin.
    void set_boundary_planes()
    {
        if constexpr (Ops::device) {  // (the oracle computes every tile in one go)
        const int gs = this->grid.grid_size;
        const float margin = 0.5f * (slab.halo - this->cube_size);
        // the z-plane of a position exactly as the grid computes it (solvers.cuh:357-360:
        // floor(z / cube_size) + grid_size / 2), which is monotonic in z: a cell below z has a
        // plane <= plane(z)
        auto plane = [&](float z) {
            const float p = floorf(z / this->cube_size) + (float)(gs / 2);
            return (int)fminf(fmaxf(p, 0.f), (float)(gs - 1));
        };
        this->force_part_cube_lo = 0;           // "below no cube"
        this->force_part_cube_hi = 0x7fffffff;  // "from no cube up"
        this->force_own_cube_lo = 0;
        this->force_own_cube_hi = 0x7fffffff;
        if (slab.rank > 0) {
            this->force_part_cube_lo = (plane(slab.z_lo + slab.halo + margin) + 1) * gs * gs;
            // own cells stray at most `margin` below the face between two migrations (the drift guard
            // sees to it): the planes below that hold mirrored cells only
            if (slab.guard) this->force_own_cube_lo = plane(slab.z_lo - margin) * gs * gs;
        }
        if (slab.rank + 1 < slab.world) {
            this->force_part_cube_hi = plane(slab.z_hi - slab.halo - margin) * gs * gs;
            if (slab.guard) this->force_own_cube_hi = (plane(slab.z_hi + margin) + 1) * gs * gs;
        }
        }
    }
    // The cubes that can hold this slab's cells until the mirrored cells are chosen anew: own cells
    // stray at most `margin` beyond a face, mirrored ones lie within halo + margin of it (the drift
    // guard stops the step otherwise), one more plane for good measure.  The grid then runs its
    // prefix sum over those planes only (Grid::set_cube_range: 2 x 15 us per step at 10 M cells in 8
    // slabs for a scan of the whole grid, whatever the slab holds).
    void set_cube_range()
    {
        if constexpr (Ops::device) {
        if (slab.world == 1) return;
        const int gs = this->grid.grid_size;
        const float margin = 0.5f * (slab.halo - this->cube_size);
        auto plane = [&](float z) {
            const float p = floorf(z / this->cube_size) + (float)(gs / 2);
            return (int)fminf(fmaxf(p, 0.f), (float)(gs - 1));
        };
        const int lo = slab.rank > 0 ? std::max(plane(slab.z_lo - slab.halo - margin) - 1, 0) : 0;
        const int hi = slab.rank + 1 < slab.world ? std::min(plane(slab.z_hi + slab.halo + margin) + 2, gs) : gs;
        this->grid.set_cube_range(lo * gs * gs, hi * gs * gs);
        }
    }
    // The cells that left the slab are packed for the neighbour they went to, and their rows are
    // filled with the staying cells from the END of the own cells (round 4: rounds 1-3 compacted all
    // staying cells in order -- three gathers and three copies over the whole slab, after which every
    // cell had a new local index and the grid's memory of the last order was worthless: the first
    // build after a migration took 200 us instead of 85 at 1.5 M local cells).  Now only as many
    // rows move as cells left, and every other cell keeps its index.
    int migrate_pack(void* buf_lo, void* buf_hi, int cap)
    {
        if (!slab.on) return -3;
        const float inf = INFINITY;
        void* bufs[2] = {buf_lo, buf_hi};
        const float z_min[2] = {-inf, slab.z_hi}, z_max[2] = {slab.z_lo, inf};
        void* arrays[3];
        size_t row_bytes[3];
        cell_arrays(arrays, row_bytes);
        for (int dir = 0; dir < 2; dir++) {
            Ops::select_z(this->d_X, P, slab.n_own, z_min[dir], z_max[dir], slab.d_idx[dir], slab.d_count + dir, slab.d_ws);
            if (bufs[dir]) Ops::pack_cells(arrays, row_bytes, slab.d_idx[dir], slab.d_count + dir, cap, bufs[dir], HEADER);
        }
        int left[2] = {0, 0};
        Ops::read_ints(slab.d_count, 2, left);
        for (int dir = 0; dir < 2; dir++) {
            // no neighbour on this side: nothing may leave (the outer faces are at infinity); more
            // cells than the message holds: they would be lost
            if (!bufs[dir] && left[dir] != 0 && !slab.failed) slab.failed = -6;
            if (bufs[dir] && left[dir] > cap && !slab.failed) slab.failed = -4;
        }
        const int n_new = slab.n_own - left[0] - left[1];
        if (n_new < slab.n_own) {
            // the staying cells of the tail [n_new, n_own), ascending, fill the holes below n_new
            Ops::select_z(reinterpret_cast<const char*>(this->d_X) + (size_t)n_new * P, P, slab.n_own - n_new, slab.z_lo,
                slab.z_hi, slab.d_gid_tmp, slab.d_count + 2, slab.d_ws);
            Ops::fill_holes(arrays, row_bytes, slab.d_idx[0], slab.d_count, slab.d_idx[1], slab.d_count + 1, slab.d_gid_tmp,
                slab.d_count + 2, n_new, slab.n_own - n_new);
        }
        slab.n_own = slab.n_local = n_new;
        return n_new;
    }
    int migrate_unpack(const void* buf_lo, const void* buf_hi, int cap)
    {
        if (!slab.on) return -3;
        const void* bufs[2] = {buf_lo, buf_hi};
        // (failures are sticky, the rank goes on with what fits: see slab_step)
        if (slab.n_own + (bufs[0] ? cap : 0) + (bufs[1] ? cap : 0) > this->n_max) {
            if (!slab.failed) slab.failed = -5;
            bufs[0] = bufs[1] = nullptr;
        }
        void* arrays[3];
        size_t row_bytes[3];
        cell_arrays(arrays, row_bytes);
        int counts[2] = {0, 0};
        if (bufs[0] || bufs[1]) {
            Ops::append_cells(arrays, row_bytes, slab.n_own, bufs[0], bufs[1], cap, HEADER, nullptr, slab.d_counts_in);
            Ops::read_ints(slab.d_counts_in, 2, counts);
        }
        int n = slab.n_own;
        for (int d = 0; d < 2; d++) {
            if (!bufs[d]) continue;
            if (counts[d] < 0 || counts[d] > cap) {
                if (!slab.failed) slab.failed = -4;
                counts[d] = std::min(std::max(counts[d], 0), cap);
            }
            n += counts[d];
        }
        slab.n_own = slab.n_local = n;
        Ops::write_int(this->d_n, n);  // (a Solution's h_n is refreshed by its next copy_to_host)
        return n;
    }
    int get_own(float* X_host, int* gid_host)
    {
        if (!slab.on) return -3;
        Ops::sync();
        Ops::d2h(X_host, this->d_X, (size_t)slab.n_own * P);
        Ops::d2h(gid_host, slab.d_gid, (size_t)slab.n_own * sizeof(int));
        return slab.n_own;
    }
    // A stage's right-hand sides, first launch: the grid over own + mirrored cells, then the
    // forces of the tiles in the z-planes next to the slab's faces (all tiles on the oracle and
    // for kernels without a split), then the neighbours' share of the result packed for sending.
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    int stage_forces_boundary(int stage, Generic_forces<Pt> gen)
    {
        if (!slab.on) return -3;
        if constexpr (Ops::device) {
            set_boundary_planes();
            this->force_part = slab.world > 1 ? 1 : 0;
        }
        this->template stage_rhs<pw_int, pw_friction>(stage, slab.n_local, slab.n_own, gen);
        if constexpr (Ops::device) this->force_part = 0;
        // both neighbours' rows in one launch
        if (slab.send_dx[0] || slab.send_dx[1])
            Ops::gather_rows_pair(stage_rhs_array(stage), P, slab.send_dx[0] ? slab.d_idx[0] : nullptr, slab.d_count,
                slab.send_dx[0], slab.send_dx[1] ? slab.d_idx[1] : nullptr, slab.d_count + 1, slab.send_dx[1],
                slab.halo_cap);
        return 0;
    }
    // ... second launch: every other tile, on a stream of its own (device build).
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void stage_forces_interior()
    {
        if constexpr (Ops::device) this->template forces_interior<pw_int, pw_friction>();
    }
    // The one message of a stage: dX (stage 2: dX1) of the own cells a neighbour mirrors goes out,
    // that of the mirrored cells comes in -- straight into their rows of the right-hand side
    // array, [n_own, n_own + ghosts[0]) from below and the rest from above.  With RCCL the
    // messages travel on a stream of their own, between two events: they leave once the packed
    // rows are complete and the update waits for their arrival (stage_join) -- the interior
    // launch runs meanwhile.
    int stage_exchange(int stage)
    {
        Pt* rhs = stage_rhs_array(stage);
        char* recv[2] = {(char*)(rhs + slab.n_own), (char*)(rhs + slab.n_own + slab.ghosts[0])};
        // a rank that could not keep its mirrored cells (-5) still takes the rows it is sent, aside
        for (int d = 0; d < 2; d++)
            if (slab.msg_in[d] != slab.ghosts[d]) recv[d] = slab.recv_halo[d];  // idle, >= halo_cap * P bytes
        const long out_bytes[2] = {(long)slab.sent[0] * (long)P, (long)slab.sent[1] * (long)P};
        const long in_bytes[2] = {(long)slab.msg_in[0] * (long)P, (long)slab.msg_in[1] * (long)P};
        if (slab.world == 1) return 0;
        if (slab.rccl)
            return Ops::rows_over_rccl(slab.rccl, slab.comm_stream, slab.rhs_packed, slab.rhs_landed, slab.send_dx[0],
                (size_t)out_bytes[0], recv[0], (size_t)in_bytes[0], slab.send_dx[1], (size_t)out_bytes[1], recv[1],
                (size_t)in_bytes[1]);
        if (!slab.exchange) return -7;
        return slab.exchange(slab.transport_ctx, 2, slab.send_dx[0], out_bytes[0], recv[0], in_bytes[0], slab.send_dx[1],
            out_bytes[1], recv[1], in_bytes[1]);
    }
    // the step's stream waits for the arrival of the messages
    void stage_join()
    {
        if (slab.rccl && slab.comm_stream && slab.world > 1) Ops::rows_wait(slab.rhs_landed);
    }
    // The fixed velocity of the two stages (ya::fix_from_total; reference solvers.cuh:241-253,265-272):
    // 0 = the mean of the whole system's right-hand sides (set_fixed()), 1 = the fixed point's value
    // (set_fixed(i)), 2 = its x and y with the mean's z (set_fixed_xy(i), first stage only: the second
    // falls through to the point's value, as in the reference)
    int fix_mode(int stage) const
    {
        if (stage == 1) return this->fix_com_z ? 2 : (this->fix_com ? 0 : 1);
        return this->fix_com ? 0 : 1;
    }
    // What this rank puts into a stage's all-reduce: {sum of its own cells' right-hand sides, their
    // count in two pieces that stay exact under a float sum, its vote for an early re-selection of the
    // mirrored cells and its error vote (first stage only), the fixed point's right-hand side if it
    // owns that cell (others: zeros)} = NW + 8 floats.
    float guard_limit() const { return 0.5f * (slab.halo - this->cube_size); }
    int slab_sum(int stage, float* d_out)
    {
        if (!slab.on) return -3;
        constexpr int NW = sizeof(Pt) / sizeof(float);
        const int with_votes = stage == 2 && slab.guard && slab.world > 1;
        const int* fix_index = fix_mode(stage) != 0 ? slab.d_fix_index : nullptr;
        if constexpr (!Ops::device) {
        auto sum = this->stage_sum(stage, slab.n_own);
        Ops::pack_sum(reinterpret_cast<const float*>(&sum), NW, slab.n_own, d_out);
        Ops::pack_extra(reinterpret_cast<const float*>(stage_rhs_array(stage)), NW, slab.d_guard, with_votes,
            slab.failed != 0, fix_index, d_out);
        } else {
        // (the drift guard is brought up to date by the reduction's last kernel: no launch of its own)
        typename Heun_solver<Pt, Grid_computer>::Guard_inputs guard;
        guard.moved_partial = slab.d_moved_partial;
        guard.n_moved = slab.n_moved_partials;
        guard.pred_partial = slab.d_pred_partial;
        guard.n_pred = slab.n_pred_partials;
        guard.limit = guard_limit();
        guard.lag_steps = slab.guard_lag_steps;
        guard.state = slab.d_guard;
        this->stage_sum_packed(stage, slab.n_own, d_out, guard, with_votes, with_votes, slab.failed != 0, fix_index);
        }
        return 0;
    }
    // the faces of this slab for the drift guard's weights (ya::Guard_band: halo + limit either side)
    float guard_band_width() const { return slab.halo + guard_limit(); }
    // own AND mirrored cells: the same kernels, the same fixed velocity, so a mirrored cell
    // moves bit for bit as it does on its owner
    int slab_update(int stage, float dt, const float* d_total, bool has_gen)
    {
        if (!slab.on) return -3;
        const int mode = fix_mode(stage);
        const bool guard = slab.guard && slab.world > 1;
        if constexpr (!Ops::device) {
        Ops::mean_from_total(d_total, sizeof(Pt) / sizeof(float), slab.d_fix, mode);
        this->stage_update(stage, slab.n_local, dt, slab.d_fix);
        if (!guard) return 0;
        // the drift guard's maxima (d_X1 exists here)
        if (stage == 1)
            slab.n_pred_partials = Ops::max_abs_diff(reinterpret_cast<const float*>(this->d_X1) + 2, P,
                reinterpret_cast<const float*>(this->d_X) + 2, P, slab.n_local, slab.z_lo, slab.z_hi, guard_band_width(),
                slab.d_pred_partial);
        else
            slab.n_moved_partials = Ops::max_abs_diff(reinterpret_cast<const float*>(this->d_X) + 2, P,
                slab.d_z_selected, sizeof(float), slab.n_local, slab.z_lo, slab.z_hi, guard_band_width(),
                slab.d_moved_partial);
        } else {
        // The update kernels of the undivided step with the totals source: they take the all-reduced totals as
        // they are and work the fixed velocity out themselves, the predictor moves own and mirrored cells in the
        // cube-sorted copy (and in d_X1 for generic forces), and they leave the drift guard's per-workgroup
        // maxima; the corrector hands the all-reduced votes to the host.
        using Solver = Heun_solver<Pt, Grid_computer>;
        typename Solver::Slab_outputs out;
        out.band.lo_face = slab.z_lo;
        out.band.hi_face = slab.z_hi;
        out.band.width = guard_band_width();
        if (guard && stage == 1) out.pred_partial = slab.d_pred_partial;
        if (guard && stage == 2) {
            out.z_selected = slab.d_z_selected;
            out.moved_partial = slab.d_moved_partial;
        }
        if (stage == 2 && slab.world > 1) out.votes_out = Ops::votes_target(slab.votes);
        this->template stage_update<Solver::Fix::totals>(stage, slab.n_local, dt, {d_total, mode}, has_gen, slab.n_own, out);
        (stage == 1 ? slab.n_pred_partials : slab.n_moved_partials) = guard ? Ops::guard_slots : 0;
        }
        return 0;
    }
    // The drift guard.  Between two selections of the mirrored cells (rehalo) a rank computes with the
    // set chosen then: a neighbour's cell that was further than `halo` from the shared face is not
    // here, and an own cell's right-hand side reaches the neighbour only if it was within `halo` of the
    // face.  Both stay correct exactly as long as NO cell has moved further in z than
    // limit = (halo - cube_size) / 2 since the selection (the predictor's positions included: stage 2
    // computes forces there).  Rounds 1-3 relied on the caller's migrate_every for that.  Now, between a
    // step's two stages, {moved = max |z - z at selection| as the previous step left the cells,
    // predicted = this step's max predictor |dz|} over own and mirrored cells (left by the update
    // kernels, folded here) make this rank's votes:
    //   error    moved + predicted > limit: stage 2 of this step computes beyond the bound
    //   request  moved + guard_lag_steps * predicted > limit: at this pace the bound is reached before a
    //            vote can act
    // The votes ride on the step's second all-reduce (no extra message), reach the host without
    // stalling the stream (Ops::votes_*: collected when the next step begins), and every rank acts on
    // the same sums: a request makes the next step begin with a migration and a new selection, an
    // error stops all ranks with -11 / -12.
    // Cells far from the faces count half (ya::Guard_band): one that was further than halo + limit
    // from a face when the mirrored cells were chosen must cover `limit` more before it can matter.
    void guard_between_stages()
    {
        if constexpr (!Ops::device) {  // (the device folds this into the second stage's reduction: slab_sum)
            if (!slab.guard || slab.world == 1) return;
            Ops::guard_update(slab.d_moved_partial, slab.n_moved_partials, slab.d_pred_partial, slab.n_pred_partials,
                guard_limit(), slab.guard_lag_steps, slab.d_guard);
        }
    }

    // Everything between "the whole system's cells on the host" and "ready to step": this rank's
    // cells (ascending global id) into the local arrays, slab_init, slab_setup.  `cells_on_host`
    // = the Solution's h_X (room for plan.n_max points), `h_n` its host count.
    int slab_adopt(const ya::Slab_plan& plan, int rank, const Pt* whole, int n_total, Pt* cells_on_host, int* h_n)
    {
        if (plan.error || rank < 0 || rank >= plan.world || plan.n_own[rank] > this->n_max) return plan.error ? plan.error : -5;
        std::vector<int> gid((size_t)plan.n_own[rank]);
        const int own = ya::slab_own_cells(plan, rank, whole, n_total, cells_on_host, gid.data());
        *h_n = own;
        Ops::h2d(this->d_X, cells_on_host, (size_t)own * P);
        Ops::write_int(this->d_n, own);
        int rc = slab_init(plan.bounds[rank], plan.bounds[rank + 1], plan.halo, gid.data(), own);
        if (rc == 0) rc = slab_setup(rank, plan.world, plan.halo_cap, plan.mig_cap);
        return rc;
    }

    // ---- the whole step of this rank's slab, sequenced here (one process per rank) ----
    int slab_setup(int rank, int world, int halo_cap, int mig_cap)
    {
        if (!slab.on || rank < 0 || rank >= world || halo_cap <= 0 || mig_cap <= 0 || slab.d_sum) return -3;
        slab.rank = rank;
        slab.world = world;
        slab.halo_cap = halo_cap;
        slab.mig_cap = mig_cap;
        const bool has[2] = {rank > 0, rank + 1 < world};
        for (int d = 0; d < 2; d++) {
            if (!has[d]) continue;
            slab.send_halo[d] = (char*)Ops::alloc(halo_bytes(halo_cap));
            slab.recv_halo[d] = (char*)Ops::alloc(halo_bytes(halo_cap));
            slab.send_mig[d] = (char*)Ops::alloc(migrate_bytes(mig_cap));
            slab.recv_mig[d] = (char*)Ops::alloc(migrate_bytes(mig_cap));
            slab.send_dx[d] = (char*)Ops::alloc((size_t)halo_cap * P);
            Ops::zero(slab.send_halo[d], halo_bytes(halo_cap));
            Ops::zero(slab.recv_halo[d], halo_bytes(halo_cap));
            Ops::zero(slab.send_mig[d], migrate_bytes(mig_cap));
            Ops::zero(slab.recv_mig[d], migrate_bytes(mig_cap));
            Ops::zero(slab.send_dx[d], (size_t)halo_cap * P);
        }
        slab.d_sum = (float*)Ops::alloc(4 * (sizeof(Pt) / sizeof(float) + 8));
        slab.halo_valid = false;
        return 0;
    }
    int slab_set_transport(ya_slab_exchange_fn exchange, ya_slab_allreduce_fn allreduce, void* ctx)
    {
        slab.exchange = exchange;
        slab.allreduce = allreduce;
        slab.transport_ctx = ctx;
        slab.rccl = nullptr;
        return 0;
    }
    int slab_use_rccl(void* comm)
    {
        const int rc = Ops::rccl_is(comm, slab.rank, slab.world);  // -2: this backend has no RCCL
        if (rc) return rc;
        slab.rccl = comm;
        slab.exchange = nullptr;
        slab.allreduce = nullptr;
        return 0;
    }
    // The stream of the interior launch, supplied by the program (Grid_computer::use_interior_stream:
    // several slabs of one process may share one); before the first step.
    int slab_use_interior_stream(void* stream)
    {
        if constexpr (Ops::device) {
            this->use_interior_stream(static_cast<typename Ops::Stream>(stream));
            return 0;
        } else {
            return -2;
        }
    }
    // fixed-capacity messages (kind 0: the mirrored cells' state, 1: migrating cells)
    int transport_exchange(int kind, char* const send[2], char* const recv[2], long bytes)
    {
        if (slab.rccl) return Ops::rccl_exchange(slab.rccl, send[0], recv[0], send[1], recv[1], (size_t)bytes);
        if (slab.world == 1) return 0;
        if (!slab.exchange) return -7;
        return slab.exchange(slab.transport_ctx, kind, send[0], send[0] ? bytes : 0, recv[0], recv[0] ? bytes : 0, send[1],
            send[1] ? bytes : 0, recv[1], recv[1] ? bytes : 0);
    }
    int transport_allreduce(float* buf, int count)
    {
        if (slab.rccl) return Ops::rccl_allreduce(slab.rccl, buf, count);
        if (slab.world == 1) return 0;
        if (!slab.allreduce) return -7;
        return slab.allreduce(slab.transport_ctx, buf, count);
    }
    // Chooses the cells each neighbour mirrors and hands their state over: after set-up and
    // after every migration.  The drift guard starts anew from these positions.
    int rehalo()
    {
        if (slab.local_order_every > 0 && slab.world > 1 && slab.rehalos % slab.local_order_every == 0 && slab.n_own > 0)
            Heun_solver<Pt, Grid_computer>::renumber(slab.d_gid);  // own cells only: *d_n = n_own here
        for (int d = 0; d < 2; d++)
            if (slab.send_halo[d]) {
                const int rc = pack_halo_state(d, slab.send_halo[d], slab.halo_cap);
                if (rc) return rc;
            }
        int rc = transport_exchange(0, slab.send_halo, slab.recv_halo, halo_bytes(slab.halo_cap));
        if (rc) return rc < 0 ? rc : -8;
        rc = unpack_halo_state(slab.recv_halo[0], slab.recv_halo[1], slab.halo_cap);
        if (rc < 0) return rc;
        if (slab.guard && slab.world > 1) {
            Ops::copy_z(this->d_X, P, slab.n_local, slab.d_z_selected);
            Ops::zero(slab.d_guard, 16);
            // nothing has moved since (the corrector folds its maxima INTO these slots: stale ones must go)
            Ops::zero(slab.d_moved_partial, 1024 * sizeof(float));
            slab.n_moved_partials = 0;
        }
        if (!this->fix_com || this->fix_com_z) Ops::find_id(slab.d_gid, slab.n_own, this->fix_point, slab.d_fix_index);
        set_cube_range();
        slab.halo_valid = true;
        slab.rehalos++;
        return 0;
    }
    // The all-reduced votes {requests, errors} of an all-reduce, once they are on the host.
    // Returns 0, or the code every rank leaves the step with.
    int act_on_votes(const float* votes)
    {
        if (votes[1] > 0.f) {
            if (!slab.failed) {
                float own[4] = {0, 0, 0, 0};
                Ops::d2h(own, slab.d_guard, sizeof(own));
                slab.failed = own[3] > 0.f ? -11 : -12;
            }
            return slab.failed;
        }
        // (a request cast before a migration that has happened since is stale)
        if (votes[0] > 0.f && slab.halo_valid) slab.migrate_requested = true;
        return 0;
    }
    // The hand-over of the cells that left the slab; the mirrored cells are dropped and chosen anew
    // by the step that follows.
    int migrate_now()
    {
        slab.n_local = slab.n_own;  // the mirrored cells are dropped, ownership is settled, ...
        slab.halo_valid = false;    // ... and the next stage starts by choosing them anew
        int rc = migrate_pack(slab.send_mig[0], slab.send_mig[1], slab.mig_cap);
        if (rc < 0) return rc;
        rc = transport_exchange(1, slab.send_mig, slab.recv_mig, migrate_bytes(slab.mig_cap));
        if (rc) return rc < 0 ? rc : -8;
        rc = migrate_unpack(slab.recv_mig[0], slab.recv_mig[1], slab.mig_cap);
        return rc < 0 ? rc : 0;
    }
    // One take_step of the decomposed system, this rank's part.  Per Heun stage: the grid over
    // own + mirrored cells (no message needed: their positions are advanced here), the forces
    // of the tiles next to the slab's faces, the exchange of those cells' right-hand sides beside
    // the forces of all other tiles, the all-reduce of {sum dX, cell count, votes, fixed point} for
    // the fixed velocity, the update of own and mirrored cells.  Cells that left the slab are handed
    // over (and the mirrored cells chosen anew) after the step if the caller asks for it, and BEFORE
    // it if the drift guard did in the step before.
    // Failures (-4, -5, -6, -11) do not end this rank's step on the spot: a rank that returned
    // early would leave its peers blocked in a collective.  It marks itself failed, keeps stepping
    // memory-safely, and its error vote reaches every rank with the next all-reduce that is read;
    // they all return non-zero from the same step (-12 on ranks that were fine themselves).
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    int slab_step(float dt, int migrate, Generic_forces<Pt> gen)
    {
        if (!slab.on || !slab.d_sum) return -3;
        constexpr int NW = sizeof(Pt) / sizeof(float);
        float votes[2] = {0.f, 0.f};
        if (slab.votes_pending) {  // the previous step's, complete by now: no stall
            Ops::votes_end(slab.votes, votes);
            slab.votes_pending = false;
            int rc = act_on_votes(votes);
            if (rc) return rc;
            if (slab.migrate_requested) {  // the same decision on every rank: the votes are all-reduced
                slab.migrate_requested = false;
                slab.guard_requests++;
                rc = migrate_now();
                if (rc) return rc;
            }
        }
        bool selected_now = false;
        if (!slab.halo_valid) {
            const int rc = rehalo();
            if (rc) return rc;
            selected_now = true;
        }
        for (int stage = 1; stage <= 2; stage++) {
            int rc = stage_forces_boundary<pw_int, pw_friction>(stage, gen);
            if (rc) return rc;
            stage_forces_interior<pw_int, pw_friction>();
            rc = stage_exchange(stage);
            if (rc) return rc < 0 ? rc : -8;
            if constexpr (Ops::device) this->join_interior();
            slab_sum(stage, slab.d_sum);
            rc = transport_allreduce(slab.d_sum, NW + 8);
            if (rc) return rc < 0 ? rc : -8;
            if (slab.world > 1 && stage == 1 && selected_now) {
                // In a step that selected the mirrored cells the host has just waited for the
                // selection's counts anyway: a failed selection (or migration before it) stops every
                // rank here and now.
                Ops::votes_begin(slab.votes, slab.d_sum + NW + 2);
                Ops::votes_end(slab.votes, votes);
                rc = act_on_votes(votes);
                if (rc) return rc;
            }
            stage_join();
            slab_update(stage, dt, slab.d_sum, Ops::has_generic_forces(gen));
            if (stage == 1) guard_between_stages();
            if (slab.world > 1 && stage == 2) {
                // the second all-reduce carried the drift guard's votes: they reach the host behind the
                // stream (stored by the corrector kernel itself on the device, copied on the host backend) and
                // are collected when the next step begins
                if constexpr (Ops::device)
                    Ops::votes_mark(slab.votes);
                else
                    Ops::votes_begin(slab.votes, slab.d_sum + NW + 2);
                slab.votes_pending = true;
            }
        }
        return migrate ? migrate_now() : 0;
    }

    // ---- for model programs: Solution<Pt, Slab_grid_solver>::take_step --------------------
    // Once slab_init and slab_setup have been called (and a transport chosen), take_step IS the
    // decomposed step; every `migrate_every` steps -- or earlier, when the drift guard asks for it --
    // the cells that left the slab are handed over and the mirrored cells chosen anew.  Between two
    // such events no cell may drift further than (halo - cube_size) / 2: with the default halo of
    // 1.25 cube_size, an eighth of a cube; the guard measures it (guard_between_stages).
    int migrate_every = 8;
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    void take_step(float dt, Generic_forces<Pt> gen_forces)
    {
        if (!slab.on || !slab.d_sum) {
            Heun_solver<Pt, Grid_computer>::template take_step<pw_int, pw_friction>(dt, gen_forces);
            return;
        }
        steps_taken++;
        const int rc = slab_step<pw_int, pw_friction>(dt, steps_taken % migrate_every == 0, gen_forces);
        if (rc != 0) {
            // (-12 and the votes' errors arrive on every rank in the same step; -7 / -8 -- a transport
            // that fails -- cannot be shared through it: whatever started the ranks ends the others)
            fprintf(stderr,
                "yalla-hip: slab step failed on rank %d (%d): -4 = a ghost layer or the migrating cells "
                "outgrew their message, -5 = n_max too small, -6 = a cell left through an outer face, -7 = no "
                "transport, -8 = the transport failed, -11 = a cell of this rank drifted further than "
                "(halo - cube_size) / 2 between two selections of the mirrored cells (smaller dt, or a larger "
                "margin in ya::slab_plan), -12 = another rank failed\n",
                slab.rank, rc);
            abort();
        }
    }

private:
    long steps_taken = 0;
};
