// Shared implementation of include/yalla_models.h.  Included by
// yalla_amd/csrc/models.hip (HIP engine) and by oracle/oracle_models.cpp (CPU
// oracle) after the respective engine headers and model_functors.h.  It is
// model-level glue: everything goes through the public header API
// (Solution, take_step, Grid, Links, random_sphere ...), so both builds make
// the identical sequence of API calls.
//
// The including file defines:
//   YA_IS_DEVICE                     1 / 0
//   YA_D2H(h, d, bytes), YA_H2D(d, h, bytes)   copies from/to "device" memory
//   YA_SYNC()                        wait for the device
//   ya_harness_random_sphere(dist, cells, seed)

#include <math.h>

#include <memory>
#include <string>
#include <vector>

#include "yalla_models.h"

#ifdef YA_ORACLE
// Gabriel_solver and wall_forces, restated host-serially for the CPU build (its engine header has neither)
#include "gabriel_host.h"
#endif

namespace harness {

struct Sim_base {
    virtual ~Sim_base() {}
    virtual int n_floats() = 0;
    virtual int n_max() = 0;
    virtual float* h_X() = 0;
    virtual int* h_n() = 0;
    virtual void copy_to_device() = 0;
    virtual void copy_to_host() = 0;
    virtual int get_d_n() = 0;
    virtual void take_steps(float dt, int n_steps) = 0;
    virtual void set_fixed(int mode, int point) = 0;
    virtual int set_cube_size(float) { return -2; }
    virtual void random_sphere(float dist_to_nb, unsigned seed) = 0;
    virtual void get_old_v(float* out) = 0;
    virtual void set_old_v(const float* in) = 0;
    virtual int get_grid(int*, int*, int*, int*) { return -2; }
    virtual int build_grid(int gs, float cs, int*, int*, int*, int*) = 0;
    virtual int set_param(const char*, double) { return -2; }
    virtual int set_prop(const char*, const int*, int) { return -2; }
    virtual int get_prop(const char*, int*, int) { return -2; }
    virtual int set_links(const int*, int, float) { return -2; }
    virtual int set_reduce_order(int) { return -1; }
    virtual int profile(int) { return -1; }
    virtual int profile_read(double*, int*) { return -1; }
    virtual long graph_launches() { return -1; }
#if YA_IS_DEVICE
    virtual long carried_steps() = 0;
    virtual long fused_bin_rebuilds() = 0;
#endif
    // z-slab decomposition (Grid_solver models only)
    virtual int slab_init(float, float, float, const int*) { return -2; }
    virtual int slab_decompose(const float*, int, int, int, float) { return -2; }
    virtual int slab_n_own() { return -2; }
    virtual int slab_n_local() { return -2; }
    virtual int slab_get_own(float*, int*) { return -2; }
    virtual int slab_setup(int, int, int, int) { return -2; }
    virtual int slab_set_transport(ya_slab_exchange_fn, ya_slab_allreduce_fn, void*) { return -2; }
    virtual int slab_use_rccl(void*) { return -2; }
    virtual int slab_step(float, int) { return -2; }
    virtual long slab_info(int) { return -2; }
};

// Solution<Pt, Solver> with the constructor arguments each solver takes, and
// access to the Grid_solver's protected grid for checks.
// Grid_solver with the z-slab decomposition on top (include/slab_logic.inc), on this build's backend
template<typename Pt>
using Harness_slab_solver = Slab_grid_solver_impl<Pt, harness_ops>;

// The solver of a model: Tile_solver (false), Grid_solver (true), Gabriel_solver
enum Solver_kind { TILE = 0, GRID = 1, GABRIEL = 2 };

template<typename Pt, int SOLVER>
struct Cells;

template<typename Pt>
struct Cells<Pt, TILE> : public Solution<Pt, Tile_solver> {
    Cells(int n_max, int, float) : Solution<Pt, Tile_solver>{n_max} {}
    Grid* grid_ptr() { return nullptr; }
    int set_gabriel_coefficient(float) { return -2; }
    int set_tile_lanes(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        if (v == 16 && !this->has_16_lanes) return -1;  // (no such kernel for points of 11 floats and more)
        this->lanes_per_cell = v;
        return 0;
#endif
    }
    int set_cube_size(float) { return -2; }
    int set_force_variant(int) { return -2; }
    int set_coop_lanes(int) { return -2; }
    int set_stage_v_max(int) { return -2; }
    int set_gather_offset_bits(int) { return -2; }
    int set_pass_facts(int) { return -2; }
    int set_tail_tiles(int) { return -2; }
    int set_sum_order(int) { return -2; }
    int set_sorted_pipeline(int) { return -2; }
    int set_graph(int) { return -2; }
    long graph_launches_so_far() { return -2; }
    int set_slab_global_ids(int) { return -2; }
    // Tile_solver stays single-GPU (all pairs): no slab decomposition.
    int slab_init(float, float, float, const int*, int) { return -2; }
    int get_own(float*, int*) { return -2; }
    int slab_adopt(const ya::Slab_plan&, int, const Pt*, int, Pt*, int*) { return -2; }
    int slab_setup(int, int, int, int) { return -2; }
    int slab_set_transport(ya_slab_exchange_fn, ya_slab_allreduce_fn, void*) { return -2; }
    int slab_use_rccl(void*) { return -2; }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    int slab_step(float, int, Generic_forces<Pt>) { return -2; }
    int set_slab_guard(int) { return -2; }
    int set_slab_guard_lag(float) { return -2; }
    int set_slab_local_order(int) { return -2; }
    struct { int n_own = -2, n_local = -2, failed = 0; long rehalos = -2, guard_requests = -2; float* d_guard = nullptr; } slab;
};

template<typename Pt>
struct Cells<Pt, GRID> : public Solution<Pt, Harness_slab_solver> {
    Cells(int n_max, int gs, float cs) : Solution<Pt, Harness_slab_solver>{n_max, gs, cs} {}
    Grid* grid_ptr() { return &this->grid; }
    int set_gabriel_coefficient(float) { return -2; }
    int set_tile_lanes(int) { return -2; }
    int set_cube_size(float cs)
    {
        this->cube_size = cs;
        return 0;
    }
    int set_force_variant(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        if (v < -1 || v > 3) return -1;  // -1 the engine's choice; 0 / 1 the A/B baselines; 2 bits; 3 cooperative
        this->force_variant = v;
        return 0;
#endif
    }
    // force_variant 3: lanes per cell (0 = chosen from n); grid_force_bits: old_v in LDS up to n cells
    int set_coop_lanes(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        if (v != 0 && v != 4 && v != 8 && v != 16) return -1;
        this->coop_lanes = v;
        return 0;
#endif
    }
    int set_stage_v_max(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        this->stage_v_max = v;
        return 0;
#endif
    }
    // grid_force_bits: old_v through 32-bit byte offsets while they fit (0), or 64-bit addresses at any size (64)
    int set_gather_offset_bits(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        if (v != 0 && v != 64) return -1;
        this->gather_offset_bits = v;
        return 0;
#endif
    }
    // grid_force_bits: what a pass may know about its hits (Grid_computer::pass_facts: 1 default, 0 generic bodies
    // only, 2 / 3 one fact alone)
    int set_pass_facts(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        if (v < 0 || v > 3) return -1;
        this->pass_facts = v;
        return 0;
#endif
    }
    // grid_force_bits: the last v tiles of a launch as half tiles (-1 = chosen from the launch's size)
    int set_tail_tiles(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        if (v < -1) return -1;
        this->force_tail_tiles = v;
        return 0;
#endif
    }
    // Grid_computer::sum_order, on BOTH builds (the oracle restates both orders): 0 = YA_SUM_REFERENCE, the
    // reference's one running sum (default); 1 = YA_SUM_BY_PLANE, own z-plane | other planes
    int set_sum_order(int v)
    {
        if (v != 0 && v != 1) return -1;
        this->sum_order = v ? YA_SUM_BY_PLANE : YA_SUM_REFERENCE;
        return 0;
    }
    int set_sorted_pipeline(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        this->sorted_pipeline = v != 0;
        this->fold_in_update = v != 2;  // 2 = the sorted pipeline with ya_reduce_mean's own second launch (A/B)
        return 0;
#endif
    }
    // Slab mode: 1 (default) = pairwise functors are called with GLOBAL ids, one extra 4-byte
    // gather per interacting pair; 0 = with local ones, enough for functors that only
    // compare i with j (springs).
    int set_slab_global_ids(int v)
    {
        if (!this->slab.on) return -3;
        this->d_global_id = v ? this->slab.d_gid : nullptr;
        return 0;
    }
    // the drift guard of the decomposition (include/slab_logic.inc guard_between_stages): on by default
    int set_slab_guard(int v)
    {
        this->slab.guard = v != 0;
        return 0;
    }
    int set_slab_guard_lag(float v)
    {
        this->slab.guard_lag_steps = v;
        return 0;
    }
    int set_slab_local_order(int v)  // own cells put into cube order at every v-th selection (0: never)
    {
        this->slab.local_order_every = v;
        return 0;
    }
    int set_graph(int v)  // Heun_solver::graph_steps: 1 always, 0 never, -1 small systems only
    {
#ifdef YA_ORACLE
        return -2;
#else
        this->graph_steps = v;
        return 0;
#endif
    }
    long graph_launches_so_far() { return this->graph_launches; }  // (device build only: Sim::graph_launches)

};

// Gabriel_solver (examples/growth_w_wall.cu:142): the grid restricted to Gabriel-graph neighbours.  Single
// GPU, d_X pipeline only: the slab, tile-lane and sorted-pipeline knobs are refused as for Tile_solver.
template<typename Pt>
struct Cells<Pt, GABRIEL> : public Solution<Pt, Gabriel_solver> {
    Cells(int n_max, int gs, float cs) : Solution<Pt, Gabriel_solver>{n_max, gs, cs} {}
    Grid* grid_ptr() { return &this->grid; }
    int set_gabriel_coefficient(float c)
    {
        this->gabriel_coefficient = c;
        return 0;
    }
    int set_tile_lanes(int) { return -2; }
    int set_cube_size(float cs)
    {
        this->cube_size = cs;
        return 0;
    }
    // -1 = ya::gabriel_force (default), 0 = the A/B baseline gabriel_force_direct (tools/ab/force_variants.cuh)
    int set_force_variant(int v)
    {
#ifdef YA_ORACLE
        return -2;
#else
        if (v != -1 && v != 0) return -1;
        this->force_variant = v;
        return 0;
#endif
    }
    int set_coop_lanes(int) { return -2; }
    int set_stage_v_max(int) { return -2; }
    int set_gather_offset_bits(int) { return -2; }
    int set_pass_facts(int) { return -2; }
    int set_tail_tiles(int) { return -2; }
    int set_sum_order(int) { return -2; }
    int set_sorted_pipeline(int) { return -2; }
    int set_graph(int) { return -2; }
    long graph_launches_so_far() { return -2; }
    int set_slab_global_ids(int) { return -2; }
    int slab_init(float, float, float, const int*, int) { return -2; }
    int get_own(float*, int*) { return -2; }
    int slab_adopt(const ya::Slab_plan&, int, const Pt*, int, Pt*, int*) { return -2; }
    int slab_setup(int, int, int, int) { return -2; }
    int slab_set_transport(ya_slab_exchange_fn, ya_slab_allreduce_fn, void*) { return -2; }
    int slab_use_rccl(void*) { return -2; }
    template<Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction>
    int slab_step(float, int, Generic_forces<Pt>) { return -2; }
    int set_slab_guard(int) { return -2; }
    int set_slab_guard_lag(float) { return -2; }
    int set_slab_local_order(int) { return -2; }
    struct { int n_own = -2, n_local = -2, failed = 0; long rehalos = -2, guard_requests = -2; float* d_guard = nullptr; } slab;
};

inline int copy_grid_out(Grid& g, int n_max, int* cube_id, int* point_id, int* cube_start,
    int* cube_end)
{
    YA_SYNC();
    if (cube_id) YA_D2H(cube_id, g.d_cube_id, (size_t)n_max * sizeof(int));
    if (point_id) YA_D2H(point_id, g.d_point_id, (size_t)n_max * sizeof(int));
    if (cube_start) YA_D2H(cube_start, g.d_cube_start, (size_t)g.n_cubes * sizeof(int));
    if (cube_end) YA_D2H(cube_end, g.d_cube_end, (size_t)g.n_cubes * sizeof(int));
    return 0;
}

// ---- generic-force policies ---------------------------------------------------
template<typename Pt>
struct No_gen {
    template<typename C>
    Generic_forces<Pt> gen(C&) { return no_gen_forces<Pt>; }
    template<typename C>
    void pre_step(C&) {}
    // what a model adds to its loop to keep its cells in cube order (opt-in: Solution::renumber)
    template<typename C>
    void post_step(C&, float) {}
#if YA_IS_DEVICE
    // pre_step and post_step do nothing: n steps may go to the solver as ONE take_steps call (Sim::take_steps)
    static constexpr bool steps_alone = true;
#endif
    template<typename C>
    int keep_in_cube_order(C& cells, int every)
    {
        cells.keep_in_cube_order(every);
        return 0;
    }
    int set_links(const int*, int, float) { return -2; }
    int set_param(const char*, double) { return -2; }
    // Solution::renumber with every id-indexed array of the model (none here)
    template<typename C>
    int renumber_now(C& cells)
    {
        cells.renumber();
        return 0;
    }
    template<typename C>
    int set_prop(C&, const char*, const int*, int) { return -2; }
    template<typename C>
    int get_prop(C&, const char*, int*, int) { return -2; }
};

template<typename Pt>
struct Push_gen : public No_gen<Pt> {
    template<typename C>
    Generic_forces<Pt> gen(C&) { return models::push<Pt>; }
    int set_param(const char*, double) { return -2; }  // (the generic force pushes cell 1: ids matter, no renumbering)
    template<typename C>
    int renumber_now(C&) { return -2; }  // ... not on request either
    template<typename C>
    int keep_in_cube_order(C&, int) { return -2; }
};

template<typename Pt, Link_force<Pt> force>
struct Links_gen : public No_gen<Pt> {
    std::unique_ptr<Links> links;
    int set_param(const char*, double) { return -2; }
    template<typename C>
    int keep_in_cube_order(C&, int) { return -2; }  // (renumbering on request only: renumber_now hands the links over)
    template<typename C>
    Generic_forces<Pt> gen(C&)
    {
        Links* l = links.get();
        if (!l) return no_gen_forces<Pt>;
        return [l](const int n, const Pt* __restrict__ d_X, Pt* d_dX) {
            return link_forces<Pt, force>(*l, d_X, d_dX);
        };
    }
    template<typename C>
    int renumber_now(C& cells)
    {
        if (links) cells.renumber(*links);
        else cells.renumber();
        return 0;
    }
    int set_links(const int* ab, int n_links, float strength)
    {
        links.reset(new Links{n_links, strength});
        for (int i = 0; i < n_links; i++) {
            links->h_link[i].a = ab[2 * i];
            links->h_link[i].b = ab[2 * i + 1];
        }
        links->copy_to_device();
        return 0;
    }
};

// the default link force through the API's own two-argument-template overload
// (links.cuh:135-140), which is where the engine may pick its atomics-free path
template<typename Pt>
struct Default_links_gen : public Links_gen<Pt, linear_force<Pt>> {
    template<typename C>
    Generic_forces<Pt> gen(C&)
    {
        Links* l = this->links.get();
        if (!l) return no_gen_forces<Pt>;
        return [l](const int n, const Pt* __restrict__ d_X, Pt* d_dX) {
            return link_forces<Pt>(*l, d_X, d_dX);
        };
    }
};

// examples/growth_w_wall.cu:155-157: the wall of node 0 as the generic force.  Node 0's identity is the
// physics: no renumbering.
struct Wall_gen : public No_gen<float3> {
    template<typename C>
    Generic_forces<float3> gen(C&)
    {
        return [](const int n, const float3* __restrict__ d_X, float3* d_dX) {
            return wall_forces<float3, xy_wall_relu_force>(n, d_X, d_dX, 0);
        };
    }
    template<typename C>
    int renumber_now(C&) { return -2; }
    template<typename C>
    int keep_in_cube_order(C&, int) { return -2; }
};

// tests/test_solvers.cu:354-381: the counters of models::count_neighbours as a Property, reset_nbs as the
// generic force (every stage), read with get_prop("n_nbs").  models::d_n_nbs is ONE symbol for every system
// of this model in a process (as the growth models' symbols below): one live system at a time -- a second
// one's step points the symbol at its own array, and the first one's next step points it back.
struct Count_gen : public No_gen<float3> {
    std::unique_ptr<Property<int>> n_nbs;
    static const void*& symbol_of()
    {
        static const void* owner = nullptr;
        return owner;
    }
    ~Count_gen()
    {
        if (symbol_of() == this) symbol_of() = nullptr;
    }
    template<typename C>
    void ensure(C& cells)
    {
        if (n_nbs) return;
        n_nbs.reset(new Property<int>{cells.n_max});
        n_nbs->copy_to_device();  // zeros
    }
    template<typename C>
    Generic_forces<float3> gen(C& cells)
    {
        ensure(cells);
        if (symbol_of() != this) {
            YA_SET_VAR(models::d_n_nbs, n_nbs->d_prop);
            symbol_of() = this;
        }
        int* nbs = n_nbs->d_prop;
        return [nbs](const int n, const float3* __restrict__ d_X, float3* d_dX) {
            YA_ZERO(nbs, (size_t)n * sizeof(int));
        };
    }
    // (the counters are indexed by id: no renumbering)
    template<typename C>
    int renumber_now(C&) { return -2; }
    template<typename C>
    int keep_in_cube_order(C&, int) { return -2; }
    template<typename C>
    int get_prop(C& cells, const char* name, int* values, int n)
    {
        if (std::string(name) != "n_nbs" || n > cells.n_max) return -2;
        ensure(cells);
        YA_SYNC();
        n_nbs->copy_to_host();
        for (int i = 0; i < n; i++) values[i] = n_nbs->h_prop[i];
        return 0;
    }
};

struct Sorting_params {
    static int set(const char* name, double v)
    {
        if (std::string(name) != "n_cells") return -2;
        YA_SET_VAR(models::sorting_n_cells, (unsigned)v);
        return 0;
    }
};

template<typename Pt>
struct Sorting_gen : public No_gen<Pt> {
    int set_param(const char* name, double v) { return Sorting_params::set(name, v); }
    // a cell's type IS its id (`i < n_cells / 2`, examples/sorting.cu:24): new ids would be other physics
    template<typename C>
    int renumber_now(C&) { return -2; }
    template<typename C>
    int keep_in_cube_order(C&, int) { return -2; }
};

// models::d_type / d_mes_nbs / d_epi_nbs are ONE set of device symbols for every system of the growth models
// in a process (passive growth and branching alike): whose arrays they point at right now
inline const void*& growth_symbols_owner()
{
    static const void* owner = nullptr;
    return owner;
}

// examples/passive_growth.cu: cell types and neighbour counters as Properties,
// reset_nbs as the generic force (:108-113), proliferate after every step (:146-149).
template<typename Rule, bool PROLIFERATE_FIRST>
struct Growth_policy : public No_gen<typename Rule::Pt> {
    using Pt = typename Rule::Pt;
    std::unique_ptr<Property<int>> type, mes_nbs, epi_nbs, scratch;
    float rate = 0.f;
    double mean_dist = 0.75;
    unsigned seed = 1, step = 0;
    bool reset_nbs = true;  // false: take_step without the generic force (:117)
#if YA_IS_DEVICE
    static constexpr bool steps_alone = false;  // (cells divide between the steps)
#endif
    template<typename C>
    void ensure(C& cells)
    {
        if (type) return;
        type.reset(new Property<int>{cells.n_max});
        mes_nbs.reset(new Property<int>{cells.n_max});
        epi_nbs.reset(new Property<int>{cells.n_max});
        scratch.reset(new Property<int>{cells.n_max + cells.n_max / 1024 + 2});  // flags, then their block sums
        type->copy_to_device();  // all mesenchyme (0)
        mes_nbs->copy_to_device();
        epi_nbs->copy_to_device();
    }
    template<typename C>
    void bind(C& cells)
    {
        ensure(cells);
        // (as the reference's model does ONCE after making its properties, examples/passive_growth.cu:103-107 --
        // here again only when another system of this process has pointed the model's symbols at ITS arrays
        // in between: three host-to-symbol copies per step were 10 us of a 349 us step of config 3)
        if (symbols_of() == this) return;
        YA_SET_VAR(models::d_type, reinterpret_cast<decltype(models::d_type)>(type->d_prop));
        YA_SET_VAR(models::d_mes_nbs, mes_nbs->d_prop);
        YA_SET_VAR(models::d_epi_nbs, epi_nbs->d_prop);
        symbols_of() = this;
    }
    static const void*& symbols_of() { return growth_symbols_owner(); }
    ~Growth_policy()
    {
        if (symbols_of() == this) symbols_of() = nullptr;
    }
    template<typename C>
    Generic_forces<Pt> gen(C& cells)
    {
        bind(cells);
        if (!reset_nbs) return no_gen_forces<Pt>;
        int* mes = mes_nbs->d_prop;
        int* epi = epi_nbs->d_prop;
        return [mes, epi](const int n, const Pt* __restrict__ d_X, Pt* d_dX) {
            YA_ZERO(mes, (size_t)n * sizeof(int));
            YA_ZERO(epi, (size_t)n * sizeof(int));
        };
    }
    template<typename C>
    void grow(C& cells)
    {
        step++;
        if (rate <= 0) return;
        ensure(cells);
        const int n = cells.get_d_n();
        models::proliferate<Rule>(rate, mean_dist, seed, step, n, cells.d_X, cells.d_old_v,
            cells.d_n, type->d_prop, mes_nbs->d_prop, epi_nbs->d_prop, scratch->d_prop, cells.n_max);
    }
    // passive_growth.cu:146-149 divides after the step, branching.cu:266-269 before
    template<typename C>
    void pre_step(C& cells)
    {
        if (PROLIFERATE_FIRST) grow(cells);
    }
    template<typename C>
    void post_step(C& cells, float)
    {
        if (!PROLIFERATE_FIRST) grow(cells);
    }
    // what a model adds ONCE to keep its id-indexed arrays local, cells in cube order:
    //     cells.keep_in_cube_order(every, type, n_mes_nbs, n_epi_nbs);
    template<typename C>
    int keep_in_cube_order(C& cells, int every)
    {
        ensure(cells);
        cells.keep_in_cube_order(every, *type, *mes_nbs, *epi_nbs);
        return 0;
    }
    template<typename C>
    int renumber_now(C& cells)
    {
        ensure(cells);
        cells.renumber(*type, *mes_nbs, *epi_nbs);
        return 0;
    }
    int set_param(const char* name, double v)
    {
        const std::string k(name);
        if (k == "prolif_rate") rate = (float)v;
        else if (k == "mean_dist") mean_dist = v;
        else if (k == "seed") seed = (unsigned)v;
        else if (k == "reset_nbs") reset_nbs = v != 0;
        else return -2;
        return 0;
    }
    Property<int>* prop(const char* name)
    {
        const std::string k(name);
        if (k == "type") return type.get();
        if (k == "mes_nbs") return mes_nbs.get();
        if (k == "epi_nbs") return epi_nbs.get();
        return nullptr;
    }
    template<typename C>
    int set_prop(C& cells, const char* name, const int* values, int n)
    {
        ensure(cells);
        Property<int>* p = prop(name);
        if (!p || n > cells.n_max) return -2;
        YA_SYNC();
        p->copy_to_host();
        for (int i = 0; i < n; i++) p->h_prop[i] = values[i];
        p->copy_to_device();
        return 0;
    }
    template<typename C>
    int get_prop(C& cells, const char* name, int* values, int n)
    {
        ensure(cells);
        Property<int>* p = prop(name);
        if (!p || n > cells.n_max) return -2;
        YA_SYNC();
        p->copy_to_host();
        for (int i = 0; i < n; i++) values[i] = p->h_prop[i];
        return 0;
    }
};

// ---- one model = point type x solver x functors x policy ------------------------
template<typename Pt, int SOLVER, Pairwise_interaction<Pt> pw_int,
    Pairwise_friction<Pt> pw_friction, typename Policy>
struct Sim : public Sim_base {
    Cells<Pt, SOLVER> cells;
    Policy policy;
    Sim(int n_max, int gs, float cs) : cells{n_max, gs, cs} {}

    int n_floats() override { return sizeof(Pt) / sizeof(float); }
    int n_max() override { return cells.n_max; }
    float* h_X() override { return reinterpret_cast<float*>(cells.h_X); }
    int* h_n() override { return cells.h_n; }
    void copy_to_device() override { cells.copy_to_device(); }
    void copy_to_host() override { cells.copy_to_host(); }
    int get_d_n() override { return cells.get_d_n(); }
    void take_steps(float dt, int n_steps) override
    {
#if YA_IS_DEVICE
        // a model loop without anything between its steps and without a generic force: one call, in which
        // Grid_solver keeps the cells in cube order from step to step (Solution::take_steps; the same bits)
        if (Policy::steps_alone) {
            Generic_forces<Pt> gen = policy.gen(cells);
            if (ya::is_no_gen_forces<Pt>(gen)) {
                cells.template take_steps<pw_int, pw_friction>(dt, n_steps, gen);
                return;
            }
        }
#endif
        for (int s = 0; s < n_steps; s++) {
            policy.pre_step(cells);
            cells.template take_step<pw_int, pw_friction>(dt, policy.gen(cells));
            policy.post_step(cells, dt);
        }
    }
    void set_fixed(int mode, int point) override
    {
        if (mode == 0) cells.set_fixed();
        if (mode == 1) cells.set_fixed(point);
        if (mode == 2) cells.set_fixed_xy(point);
    }
    int set_cube_size(float cs) override { return cells.set_cube_size(cs); }
    void random_sphere(float dist_to_nb, unsigned seed) override
    {
        ya_harness_random_sphere(dist_to_nb, cells, seed);
    }
    void get_old_v(float* out) override
    {
        YA_SYNC();
        YA_D2H(out, cells.d_old_v, (size_t)cells.n_max * 3 * sizeof(float));
    }
    void set_old_v(const float* in) override
    {
        YA_SYNC();
        YA_H2D(cells.d_old_v, in, (size_t)cells.n_max * 3 * sizeof(float));
    }
    int get_grid(int* a, int* b, int* c, int* d) override
    {
        Grid* g = cells.grid_ptr();
        if (!g) return -2;
        return copy_grid_out(*g, cells.n_max, a, b, c, d);
    }
    int build_grid(int gs, float cs, int* a, int* b, int* c, int* d) override
    {
        Grid grid{cells.n_max, gs};
        grid.build(cells, cs);
        return copy_grid_out(grid, cells.n_max, a, b, c, d);
    }
    int set_param(const char* name, double v) override
    {
        if (std::string(name) == "force_variant") return cells.set_force_variant((int)v);
        if (std::string(name) == "coop_lanes") return cells.set_coop_lanes((int)v);
        if (std::string(name) == "stage_v_max") return cells.set_stage_v_max((int)v);
        if (std::string(name) == "tail_tiles") return cells.set_tail_tiles((int)v);
        if (std::string(name) == "gather_offset_bits") return cells.set_gather_offset_bits((int)v);
        if (std::string(name) == "pass_facts") return cells.set_pass_facts((int)v);
        if (std::string(name) == "sum_order") return cells.set_sum_order((int)v);
        if (std::string(name) == "sorted_pipeline") return cells.set_sorted_pipeline((int)v);
        if (std::string(name) == "graph") return cells.set_graph((int)v);
        if (std::string(name) == "tile_lanes") return cells.set_tile_lanes((int)v);
        if (std::string(name) == "slab_global_ids") return cells.set_slab_global_ids((int)v);
        if (std::string(name) == "gabriel_coefficient") return cells.set_gabriel_coefficient((float)v);
        if (std::string(name) == "renumber_now") return policy.renumber_now(cells);
        // Solution::keep_in_cube_order with every id-indexed array of the model (0 = off again)
        if (std::string(name) == "renumber_every") return policy.keep_in_cube_order(cells, (int)v);
        if (std::string(name) == "slab_guard") return cells.set_slab_guard((int)v);
        if (std::string(name) == "slab_guard_lag") return cells.set_slab_guard_lag((float)v);
        if (std::string(name) == "slab_local_order") return cells.set_slab_local_order((int)v);
#if YA_IS_DEVICE
        if (std::string(name) == "carry_sorted") {  // Heun_solver::carry_sorted (A/B, tests; same results)
            cells.carry_sorted = v != 0;
            return 0;
        }
        if (std::string(name) == "bin_in_update") {  // Heun_solver::bin_in_update (A/B, tests; same results)
            cells.bin_in_update = v != 0;
            return 0;
        }
        if (std::string(name) == "four_tile_updates") {  // Heun_solver::four_tile_updates (A/B; same results)
            cells.four_tile_updates = v != 0;
            return 0;
        }
        if (std::string(name) == "trim_carried_stores") {  // Heun_solver::trim_carried_stores (A/B; same results)
            cells.trim_carried_stores = v != 0;
            return 0;
        }
#endif
#ifndef YA_ORACLE
        if (std::string(name) == "links_segmented_min") {  // ya::links_segmented_min(), process-wide
            ya::links_segmented_min() = (int)v;
            return 0;
        }
#endif
        return policy.set_param(name, v);
    }
    int set_links(const int* ab, int n, float s) override { return policy.set_links(ab, n, s); }
    int set_prop(const char* name, const int* v, int n) override { return policy.set_prop(cells, name, v, n); }
    int get_prop(const char* name, int* v, int n) override { return policy.get_prop(cells, name, v, n); }
    int slab_init(float a, float b, float h, const int* gid) override { return cells.slab_init(a, b, h, gid, *cells.h_n); }
    int slab_decompose(const float* X, int n, int rank, int world, float cube_size) override
    {
        const Pt* whole = reinterpret_cast<const Pt*>(X);
        const ya::Slab_plan plan = ya::slab_plan(whole, n, world, cube_size);
        return cells.slab_adopt(plan, rank, whole, n, cells.h_X, cells.h_n);
    }
    int slab_n_own() override { return cells.slab.n_own; }
    int slab_n_local() override { return cells.slab.n_local; }
    int slab_get_own(float* X, int* gid) override { return cells.get_own(X, gid); }
    int slab_setup(int rank, int world, int hc, int mc) override { return cells.slab_setup(rank, world, hc, mc); }
    int slab_set_transport(ya_slab_exchange_fn e, ya_slab_allreduce_fn a, void* ctx) override
    {
        return cells.slab_set_transport(e, a, ctx);
    }
    int slab_use_rccl(void* comm) override { return cells.slab_use_rccl(comm); }
    long slab_info(int what) override
    {
        if (what == 3 || what == 4) {  // the drift guard's {moved, predicted} of the last step, in millionths of a length unit
            float state[4] = {0, 0, 0, 0};
            if (!cells.slab.d_guard) return -3;
            YA_SYNC();
            YA_D2H(state, cells.slab.d_guard, sizeof(state));
            return (long)(1e6 * (double)state[what - 3]);
        }
        return what == 0 ? cells.slab.rehalos : what == 1 ? cells.slab.guard_requests : what == 2 ? cells.slab.failed : -3;
    }
    int slab_step(float dt, int migrate) override
    {
        const int rc = cells.template slab_step<pw_int, pw_friction>(dt, migrate, policy.gen(cells));
        if (rc == 0) *cells.h_n = cells.slab.n_own;  // (the drift guard may have made the step migrate)
        return rc;
    }
    long graph_launches() override
    {
#ifdef YA_ORACLE
        return -1;
#else
        return cells.graph_launches_so_far();
#endif
    }
#if YA_IS_DEVICE
    long carried_steps() override { return cells.carried_steps; }
    long fused_bin_rebuilds() override { return cells.fused_bin_rebuilds; }
#endif
#ifdef YA_ORACLE
    int set_reduce_order(int order) override
    {
        cells.reduce_order = order ? YA_REDUCE_TREE : YA_REDUCE_SERIAL;
        return 0;
    }
#else
    int profile(int enable) override
    {
        cells.profiler.enable(enable != 0, enable);
        return 0;
    }
    int profile_read(double* ms, int* launches) override
    {
        cells.profiler.read(ms, launches);
        return 0;
    }
#endif
};

using Links3 = Default_links_gen<float3>;
using Links4 = Default_links_gen<float4>;
using Links4_custom = Links_gen<float4, models::custom_force<float4>>;

#ifndef YA_MODEL_EXTRA
#define YA_MODEL_EXTRA
#endif

using Passive_growth = Growth_policy<models::Passive_growth_rule, false>;
using Branching = Growth_policy<models::Branching_rule, true>;

using Factory = Sim_base* (*)(int, int, float);
struct Model {
    const char* name;
    Factory make;
};

template<typename S>
Sim_base* make_sim(int n_max, int gs, float cs)
{
    return new S{n_max, gs, cs};
}

// SOLVER: false / true = Tile_solver / Grid_solver (as before the third one), or GABRIEL
#define YA_MODEL(name, Pt, SOLVER, pw_int, pw_friction, Policy) \
    Model { name, &make_sim<Sim<Pt, SOLVER, pw_int, pw_friction, Policy>> }

// -DYA_MODELS_WIDTHS (widths_models.h): another library's table, compiled instead of this one
static const Model model_table[] = {
#ifdef YA_MODEL_TABLE
    YA_MODEL_TABLE
#else
    // BASELINE configs 1 and 5: springs (examples/springs.cu)
    YA_MODEL("springs_tile", float3, false, models::spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_MODEL("springs_grid", float3, true, models::spring, friction_w_neighbour<float3>, No_gen<float3>),
    // tests/test_solvers.cu: clipped_spring with both frictions
    YA_MODEL("clipped_tile", float3, false, models::clipped_spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_MODEL("clipped_grid", float3, true, models::clipped_spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_MODEL("fading_tile", float3, false, models::fading_spring, friction_on_background<float3>, No_gen<float3>),
    YA_MODEL("fading_grid", float3, true, models::fading_spring, friction_on_background<float3>, No_gen<float3>),
    YA_MODEL("clipped_push_grid", float3, true, models::clipped_spring, friction_w_neighbour<float3>, Push_gen<float3>),
    // inits.cuh relu_force (relaxation)
    YA_MODEL("relu_tile", float3, false, relu_force<float3>, friction_w_neighbour<float3>, No_gen<float3>),
    YA_MODEL("relu_grid", float3, true, relu_force<float3>, friction_w_neighbour<float3>, No_gen<float3>),
    // BASELINE config 2: sorting (examples/sorting.cu)
    YA_MODEL("sorting_tile", float3, false, models::differential_adhesion, friction_w_neighbour<float3>, Sorting_gen<float3>),
    YA_MODEL("sorting_grid", float3, true, models::differential_adhesion, friction_w_neighbour<float3>, Sorting_gen<float3>),
    // tests/test_solvers.cu: oscillator (float4), generic force, frictions
    YA_MODEL("oscillator_tile", float4, false, models::oscillator, friction_w_neighbour<float4>, No_gen<float4>),
    YA_MODEL("push_tile", float3, false, models::no_pw_int<float3>, friction_w_neighbour<float3>, Push_gen<float3>),
    YA_MODEL("push_grid", float3, true, models::no_pw_int<float3>, friction_w_neighbour<float3>, Push_gen<float3>),
    YA_MODEL("push_background_tile", float3, false, models::no_pw_int<float3>, friction_on_background<float3>, Push_gen<float3>),
    YA_MODEL("push_background_grid", float3, true, models::no_pw_int<float3>, friction_on_background<float3>, Push_gen<float3>),
    // tests/test_links.cu: link forces (default and custom) without pairwise force
    YA_MODEL("links_tile", float3, false, models::no_pw_int<float3>, friction_w_neighbour<float3>, Links3),
    YA_MODEL("links_grid", float3, true, models::no_pw_int<float3>, friction_w_neighbour<float3>, Links3),
    YA_MODEL("links4_tile", float4, false, models::no_pw_int<float4>, friction_w_neighbour<float4>, Links4),
    YA_MODEL("links4_custom_tile", float4, false, models::no_pw_int<float4>, friction_w_neighbour<float4>, Links4_custom),
    // springs + links on the grid (link_forces on a large system)
    YA_MODEL("springs_links_grid", float3, true, models::spring, friction_w_neighbour<float3>, Links3),
    // Po_cell through the generic (MAKE_PT) operators
    YA_MODEL("relu_po_tile", Po_cell, false, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, No_gen<Po_cell>),
    YA_MODEL("relu_po_grid", Po_cell, true, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, No_gen<Po_cell>),
    // BASELINE config 4: examples/passive_growth.cu (Po_cell, bending_force, growth)
    YA_MODEL("passive_growth_grid", Po_cell, true, models::relu_w_epithelium, friction_w_neighbour<Po_cell>, Passive_growth),
    YA_MODEL("passive_growth_tile", Po_cell, false, models::relu_w_epithelium, friction_w_neighbour<Po_cell>, Passive_growth),
    // BASELINE config 3: examples/branching.cu (7-float Cell, Turing kinetics, atomics)
    YA_MODEL("branching_grid", Cell, true, models::epi_turing_mes_noturing, friction_w_neighbour<Cell>, Branching),
    YA_MODEL("relu_cell_grid", Cell, true, relu_force<Cell>, friction_w_neighbour<Cell>, No_gen<Cell>),
    // Gabriel_solver (solvers.cuh:505-644): relaxation and tests/test_solvers.cu's clipped spring on the
    // Gabriel graph, and the relaxation stage of examples/growth_w_wall.cu (:36-63, :161-174: wall node 0)
    YA_MODEL("relu_gabriel", float3, GABRIEL, relu_force<float3>, friction_w_neighbour<float3>, No_gen<float3>),
    YA_MODEL("clipped_gabriel", float3, GABRIEL, models::clipped_spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_MODEL("wall_gabriel", float3, GABRIEL, models::wall_relu_force, friction_on_background<float3>, Wall_gen),
    // ... a functor that is not declared YA_STATELESS (what a model that does not know the macro gets, as
    // growth_w_wall.cu's own), tests/test_solvers.cu:339-381's neighbour counter, and the wide point types
    YA_MODEL("relu_plain_gabriel", float3, GABRIEL, models::relu_plain, friction_w_neighbour<float3>, No_gen<float3>),
    YA_MODEL("count_gabriel", float3, GABRIEL, models::count_neighbours, friction_w_neighbour<float3>, Count_gen),
    YA_MODEL("relu_po_gabriel", Po_cell, GABRIEL, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, No_gen<Po_cell>),
    YA_MODEL("relu_cell_gabriel", Cell, GABRIEL, relu_force<Cell>, friction_w_neighbour<Cell>, No_gen<Cell>),
    // user-written frictions (model_functors.h: graded, ids, field) beside the declared relu_force, so that the
    // friction's YA_STATELESS_FRICTION line alone decides the kernel body: the declared name gets the several-lane
    // bodies, its `_plain` twin the one-lane ones (tests/test_friction_functors*.py).  The fewest rows that reach
    // every body; graded sits beside fading_spring, whose force does not jump at the cut-off (the fast tier's row).
    YA_MODEL("friction_graded_tile", float3, false, relu_force<float3>, models::graded_friction<float3>, No_gen<float3>),
    YA_MODEL("friction_ids_tile", float3, false, relu_force<float3>, models::ids_friction, No_gen<float3>),
    YA_MODEL("friction_ids_plain_tile", float3, false, relu_force<float3>, models::ids_friction_plain, No_gen<float3>),
    YA_MODEL("friction_field_tile", Po_cell, false, relu_force<Po_cell>, models::field_friction, No_gen<Po_cell>),
    YA_MODEL("friction_field_plain_tile", Po_cell, false, relu_force<Po_cell>, models::field_friction_plain, No_gen<Po_cell>),
    YA_MODEL("friction_graded_fading_grid", float3, true, models::fading_spring, models::graded_friction<float3>, No_gen<float3>),
    YA_MODEL("friction_ids_grid", float3, true, relu_force<float3>, models::ids_friction, No_gen<float3>),
    YA_MODEL("friction_ids_plain_grid", float3, true, relu_force<float3>, models::ids_friction_plain, No_gen<float3>),
    YA_MODEL("friction_field_grid", Po_cell, true, relu_force<Po_cell>, models::field_friction, No_gen<Po_cell>),
    YA_MODEL("friction_graded_gabriel", float3, GABRIEL, relu_force<float3>, models::graded_friction<float3>, No_gen<float3>),
    YA_MODEL("friction_ids_gabriel", float3, GABRIEL, relu_force<float3>, models::ids_friction, No_gen<float3>),
    YA_MODEL("friction_ids_plain_gabriel", float3, GABRIEL, relu_force<float3>, models::ids_friction_plain, No_gen<float3>),
    YA_MODEL("friction_field_gabriel", Po_cell, GABRIEL, relu_force<Po_cell>, models::field_friction, No_gen<Po_cell>),
    YA_MODEL_EXTRA
#endif
};
static const int n_models = sizeof(model_table) / sizeof(model_table[0]);

}  // namespace harness

struct ya_sim {
    std::unique_ptr<harness::Sim_base> p;
};

extern "C" {

int ya_models_is_device(void) { return YA_IS_DEVICE; }
int ya_models_arith(void)
{
#ifdef YA_ARITH_FAST
    return 1;
#else
    return 0;
#endif
}
int ya_models_count(void) { return harness::n_models; }
const char* ya_models_name(int i)
{
    return (i >= 0 && i < harness::n_models) ? harness::model_table[i].name : nullptr;
}

int ya_sim_create(const char* model, int n_max, int grid_size, float cube_size, ya_sim** out)
{
    if (!model || !out || n_max <= 0) return -3;
    for (int i = 0; i < harness::n_models; i++) {
        if (std::string(model) == harness::model_table[i].name) {
            ya_sim* s = new ya_sim;
            s->p.reset(harness::model_table[i].make(n_max, grid_size, cube_size));
            *out = s;
            return 0;
        }
    }
    return -1;
}
void ya_sim_destroy(ya_sim* sim) { delete sim; }

int ya_sim_n_floats(ya_sim* s) { return s->p->n_floats(); }
int ya_sim_n_max(ya_sim* s) { return s->p->n_max(); }
float* ya_sim_h_X(ya_sim* s) { return s->p->h_X(); }
int ya_sim_set_h_n(ya_sim* s, int n)
{
    if (n < 0 || n > s->p->n_max()) return -3;
    *s->p->h_n() = n;
    return 0;
}
int ya_sim_get_h_n(ya_sim* s) { return *s->p->h_n(); }
int ya_sim_copy_to_device(ya_sim* s)
{
    s->p->copy_to_device();
    return 0;
}
int ya_sim_copy_to_host(ya_sim* s)
{
    s->p->copy_to_host();
    return 0;
}
int ya_sim_get_d_n(ya_sim* s) { return s->p->get_d_n(); }
int ya_sim_take_steps(ya_sim* s, float dt, int n_steps)
{
    s->p->take_steps(dt, n_steps);
    return 0;
}
int ya_sim_synchronize(ya_sim*)
{
    YA_SYNC();
    return 0;
}
int ya_sim_set_fixed(ya_sim* s, int mode, int point)
{
    if (mode < 0 || mode > 2) return -3;
    s->p->set_fixed(mode, point);
    return 0;
}
int ya_sim_set_cube_size(ya_sim* s, float cs) { return s->p->set_cube_size(cs); }
int ya_sim_random_sphere(ya_sim* s, float dist_to_nb, unsigned seed)
{
    s->p->random_sphere(dist_to_nb, seed);
    return 0;
}
int ya_sim_get_old_v(ya_sim* s, float* out)
{
    s->p->get_old_v(out);
    return 0;
}
int ya_sim_set_old_v(ya_sim* s, const float* in)
{
    s->p->set_old_v(in);
    return 0;
}
int ya_sim_get_grid(ya_sim* s, int* a, int* b, int* c, int* d) { return s->p->get_grid(a, b, c, d); }
int ya_sim_build_grid(ya_sim* s, int gs, float cs, int* a, int* b, int* c, int* d)
{
    return s->p->build_grid(gs, cs, a, b, c, d);
}
int ya_sim_set_param(ya_sim* s, const char* name, double v) { return s->p->set_param(name, v); }
int ya_sim_set_prop(ya_sim* s, const char* name, const int* v, int n) { return s->p->set_prop(name, v, n); }
int ya_sim_get_prop(ya_sim* s, const char* name, int* v, int n) { return s->p->get_prop(name, v, n); }
int ya_sim_set_links(ya_sim* s, const int* ab, int n, float strength) { return s->p->set_links(ab, n, strength); }
int ya_sim_set_reduce_order(ya_sim* s, int order) { return s->p->set_reduce_order(order); }
int ya_slab_init(ya_sim* s, float z_lo, float z_hi, float halo, const int* gid) { return s->p->slab_init(z_lo, z_hi, halo, gid); }
int ya_slab_decompose(ya_sim* s, const float* X, int n, int rank, int world, float cube_size)
{
    return s->p->slab_decompose(X, n, rank, world, cube_size);
}
long ya_slab_info(ya_sim* s, int what) { return s->p->slab_info(what); }
int ya_slab_n_own(ya_sim* s) { return s->p->slab_n_own(); }
int ya_slab_n_local(ya_sim* s) { return s->p->slab_n_local(); }
int ya_slab_plan(const float* X, int n_floats, int n, int world, float cube_size, float* bounds, int* capacities)
{
    if (!X || n_floats < 3 || n <= 0 || world < 1 || !bounds || !capacities) return -3;
    struct Z_only {  // ya::slab_plan only reads .z
        float z;
    };
    std::vector<Z_only> z((size_t)n);
    for (int i = 0; i < n; i++) z[i].z = X[(size_t)i * n_floats + 2];
    const ya::Slab_plan plan = ya::slab_plan(z.data(), n, world, cube_size);
    for (int r = 0; r <= world; r++) bounds[r] = plan.bounds[r];
    capacities[0] = plan.halo_cap;
    capacities[1] = plan.mig_cap;
    capacities[2] = plan.n_max;
    capacities[3] = (int)((plan.halo_cap - 64) / 1.15f);
    return plan.error;
}
int ya_slab_setup(ya_sim* s, int rank, int world, int halo_cap, int mig_cap) { return s->p->slab_setup(rank, world, halo_cap, mig_cap); }
int ya_slab_set_transport(ya_sim* s, ya_slab_exchange_fn e, ya_slab_allreduce_fn a, void* ctx) { return s->p->slab_set_transport(e, a, ctx); }
int ya_slab_use_rccl(ya_sim* s, void* comm) { return s->p->slab_use_rccl(comm); }
int ya_slab_step(ya_sim* s, float dt, int migrate) { return s->p->slab_step(dt, migrate); }
int ya_slab_get_own(ya_sim* s, float* X, int* gid) { return s->p->slab_get_own(X, gid); }
long ya_check_sqrt(unsigned first_bits, unsigned last_bits)
{
#ifdef YA_ORACLE
    return -1;
#else
    unsigned long long* d_bad = (unsigned long long*)harness_ops::alloc(8);
    YA_ZERO(d_bad, 8);
    ya::check_sqrt_all<<<4096, 256>>>(first_bits, last_bits, d_bad);
    unsigned long long bad = 0;
    YA_D2H(&bad, d_bad, 8);
    harness_ops::release(d_bad);
    return (long)bad;
#endif
}
long ya_check_reciprocal(unsigned first_bits, unsigned last_bits)
{
#ifdef YA_ORACLE
    return -1;
#else
    unsigned long long* d_bad = (unsigned long long*)harness_ops::alloc(8);
    YA_ZERO(d_bad, 8);
    ya::check_reciprocal_all<<<4096, 256>>>(first_bits, last_bits, d_bad);
    unsigned long long bad = 0;
    YA_D2H(&bad, d_bad, 8);
    harness_ops::release(d_bad);
    return (long)bad;
#endif
}
int ya_sim_profile(ya_sim* s, int enable) { return s->p->profile(enable); }
int ya_sim_profile_read(ya_sim* s, double* ms, int* launches) { return s->p->profile_read(ms, launches); }
long ya_sim_graph_launches(ya_sim* s) { return s->p->graph_launches(); }
#if YA_IS_DEVICE
// Device build only, read-only (test hook, beside ya_sim_graph_launches): the steps of this system so far whose
// first grid build started from the step before's cube-sorted cells (Heun_solver::carried_steps): k - 1 per
// qualifying ya_sim_take_steps call of k steps, 0 for everything that ran as the loop of take_step.
__attribute__((visibility("default"))) long ya_sim_carried_steps(ya_sim* s) { return s->p->carried_steps(); }
// The same kind of hook: the grid rebuilds of this system so far that ran without a k_bin launch because the update
// kernel in front of them had binned their entries (Heun_solver::fused_bin_rebuilds): 2 k - 1 per carried call of
// k steps while bin_in_update is on, 0 otherwise.
__attribute__((visibility("default"))) long ya_sim_fused_bin_rebuilds(ya_sim* s) { return s->p->fused_bin_rebuilds(); }
#endif

}  // extern "C"
