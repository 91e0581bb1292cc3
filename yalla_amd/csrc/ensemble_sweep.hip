// libyalla_ensemble_sweep.so -- the sweep harness (include/yalla_ensemble_sweep.h): the three forms of Ensemble
// (include/ensemble.cuh, ensemble_grid.cuh, ensemble_gabriel.cuh) behind ONE handle type, stepped with a time step per
// replica (ya::ens::Replica_dt) and, the Gabriel form, a coefficient per replica (d_gabriel_coefficients) where the
// handle holds such arrays, with the scalar otherwise.  A small model table per form, taken from the other harnesses
// (model_functors.h is included read-only for the functors and their YA_STATELESS declarations).  Links against
// libyalla_hip.so.
#include <cmath>

#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "dtypes.cuh"
#include "inits.cuh"
#include "links.cuh"
#include "property.cuh"
#include "solvers.cuh"
#include "ensemble.cuh"

#include "model_functors.h"

#include "yalla_ensemble_sweep.h"
#include "ensemble_harness.h"  // Replicas(_of), Grid_replicas(_of), Model, the entry points' bodies

namespace swp_harness {
using ens_harness::Grid_replicas;
using ens_harness::Grid_replicas_of;
using ens_harness::Model;
using ens_harness::Replicas;
using ens_harness::Replicas_of;

// A model's own adaptive-dt kernel, in one line: the array is changed on the device, in stream order.
__global__ void scale_floats(const int n, float* __restrict__ d_values, const float factor)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d_values[i] = d_values[i] * factor;
}

// n_replicas floats on the device that a handle owns: absent until the first upload, absent again after clear().
struct Device_floats {
    float* d = nullptr;
    bool set = false;
    Device_floats() = default;
    Device_floats(const Device_floats&) = delete;
    ~Device_floats()
    {
        if (d) ya_free(d);
    }
    void upload(const float* h, int n)
    {
        if (!d) YA_CHECK(ya_malloc((void**)&d, (size_t)n * sizeof(float)));
        YA_CHECK(ya_memcpy_h2d(d, h, (size_t)n * sizeof(float)));
        set = true;
    }
    void clear() { set = false; }
    const float* get() const { return set ? d : nullptr; }
};

// What a handle holds, whatever its form: the shared interfaces of ensemble_harness.h (grid(): null for the all-pairs
// form) and what the forms answer each in its own way.
struct Sweep {
    using Interface = Sweep;  // (what ens_harness::make_sim returns)
    Device_floats dt, coefficients;
    virtual ~Sweep() {}
    virtual Replicas& replicas() = 0;
    virtual Grid_replicas* grid() = 0;
    virtual long take_steps(float dt, int n_steps) = 0;  // returns the launches that stepped from LDS
    virtual int set_param(const std::string& name, double v) = 0;  // (the value is checked already) -3: not this form's
    virtual int lanes_used() = 0;
    virtual int dense_cells() { return -3; }
    virtual long long lds_dense_cells() { return -3; }
    virtual bool has_coefficients() { return false; }
    virtual int* h_link() { return nullptr; }
    virtual int* h_n_links() { return nullptr; }
    virtual int n_slots() { return 0; }
};

// The links of a linked model (at least one slot: an object of no slots has nothing to allocate or launch).
template<bool LINKED>
struct Links_of {
    Links_of(int, int) {}
};
template<>
struct Links_of<true> {
    const int slots_per_replica;
    Links links;
    Links_of(int n_replicas, int slots_per_replica)
        : slots_per_replica{slots_per_replica},
          links{n_replicas * slots_per_replica > 0 ? n_replicas * slots_per_replica : 1, 0.2f}
    {
        static_assert(sizeof(Link) == 2 * sizeof(int), "h_link is handed out as pairs of ints");
        *links.h_n = n_replicas * slots_per_replica;
        links.set_d_n(n_replicas * slots_per_replica);
    }
};

// cells.take_steps with the handle's array or the scalar, with the links of a linked model
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool LINKED, typename Cells>
void step(Cells& cells, Sweep& s, Links_of<LINKED>& l, float dt, int n_steps)
{
    const float* d_dt = s.dt.get();
    if constexpr (LINKED) {
        const ya::ens::Replica_links links{l.links, l.slots_per_replica};
        if (d_dt)
            cells.template take_steps<pw_int, pw_friction>(ya::ens::Replica_dt{d_dt}, n_steps, links);
        else
            cells.template take_steps<pw_int, pw_friction>(dt, n_steps, links);
    } else {
        if (d_dt)
            cells.template take_steps<pw_int, pw_friction>(ya::ens::Replica_dt{d_dt}, n_steps);
        else
            cells.template take_steps<pw_int, pw_friction>(dt, n_steps);
    }
}

#define YA_SWP_LINKS_OVERRIDES                                                                               \
    void copy_to_device() override                                                                           \
    {                                                                                                        \
        cells.copy_to_device();                                                                              \
        if constexpr (LINKED) l.links.copy_to_device();                                                      \
    }                                                                                                        \
    int* h_link() override                                                                                   \
    {                                                                                                        \
        if constexpr (LINKED) return reinterpret_cast<int*>(l.links.h_link);                                 \
        return nullptr;                                                                                      \
    }                                                                                                        \
    int* h_n_links() override                                                                                \
    {                                                                                                        \
        if constexpr (LINKED) return l.links.h_n;                                                            \
        return nullptr;                                                                                      \
    }                                                                                                        \
    int n_slots() override                                                                                   \
    {                                                                                                        \
        if constexpr (LINKED) return cells.n_replicas * l.slots_per_replica;                                 \
        return 0;                                                                                            \
    }

// The all-pairs form.  The harness's own defaults, as the other all-pairs harnesses': the six-launch step, one lane
// per cell inside a whole-step launch.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool LINKED>
struct Tile_sim : public Replicas_of<Ensemble<Pt>, Replicas>, public Sweep {
    using Interface = Sweep;
    using Replicas_of<Ensemble<Pt>, Replicas>::cells;
    Links_of<LINKED> l;
    Tile_sim(int n_replicas, int n_max, int slots_per_replica, int, float, float)
        : Replicas_of<Ensemble<Pt>, Replicas>{n_replicas, n_max}, l{n_replicas, slots_per_replica}
    {
        cells.whole_steps = -1;
        cells.whole_step_lanes = 1;
    }
    Replicas& replicas() override { return *this; }
    Grid_replicas* grid() override { return nullptr; }
    long take_steps(float dt, int n_steps) override
    {
        const long before = cells.whole_step_launches;
        step<Pt, pw_int, pw_friction, LINKED>(cells, *this, l, dt, n_steps);
        return cells.whole_step_launches - before;
    }
    int set_param(const std::string& name, double v) override
    {
        if (name == "whole_steps")
            cells.whole_steps = (int)v;
        else if (name == "whole_step_lanes")
            cells.whole_step_lanes = (int)v;
        else if (name == "steps_per_launch")
            cells.steps_per_launch = (int)v;
        else
            return -3;
        return 0;
    }
    int lanes_used() override { return cells.whole_step_lanes_used; }
    YA_SWP_LINKS_OVERRIDES
};

// The grid form.  Defaults as the grid harnesses': the 14-launch step, one lane per cell in launches from LDS.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool LINKED>
struct Grid_sim : public Grid_replicas_of<Ensemble<Pt, Grid_solver>, Grid_replicas>, public Sweep {
    using Interface = Sweep;
    using Grid_replicas_of<Ensemble<Pt, Grid_solver>, Grid_replicas>::cells;
    Links_of<LINKED> l;
    Grid_sim(int n_replicas, int n_max, int slots_per_replica, int grid_size, float cube_size, float)
        : Grid_replicas_of<Ensemble<Pt, Grid_solver>, Grid_replicas>{n_replicas, n_max, grid_size, cube_size},
          l{n_replicas, slots_per_replica}
    {
        cells.lds_steps = -1;
        cells.lds_step_lanes = 1;
    }
    Replicas& replicas() override { return *this; }
    Grid_replicas* grid() override { return this; }
    long take_steps(float dt, int n_steps) override
    {
        const long before = cells.lds_step_launches;
        step<Pt, pw_int, pw_friction, LINKED>(cells, *this, l, dt, n_steps);
        return cells.lds_step_launches - before;
    }
    int set_param(const std::string& name, double v) override
    {
        if (name == "lds_steps")
            cells.lds_steps = (int)v;
        else if (name == "lds_step_lanes")
            cells.lds_step_lanes = (int)v;
        else if (name == "steps_per_launch")
            cells.lds_steps_max = (int)v;
        else if (name == "cube_size")
            cells.cube_size = (float)v;
        else
            return -3;
        return 0;
    }
    int lanes_used() override { return cells.lds_step_lanes_used; }
    YA_SWP_LINKS_OVERRIDES
};

// The Gabriel form (no links, no lanes knob).  Default as the Gabriel harnesses': the 16-launch step.
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, bool LINKED>
struct Gabriel_sim : public Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Grid_replicas>, public Sweep {
    static_assert(!LINKED, "the Gabriel form steps without ordered links");
    using Interface = Sweep;
    using Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Grid_replicas>::cells;
    Links_of<false> l{0, 0};
    Gabriel_sim(int n_replicas, int n_max, int, int grid_size, float cube_size, float gabriel_coefficient)
        : Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Grid_replicas>{
              n_replicas, n_max, grid_size, cube_size, gabriel_coefficient}
    {
        cells.lds_steps = -1;
    }
    Replicas& replicas() override { return *this; }
    Grid_replicas* grid() override { return this; }
    long take_steps(float dt, int n_steps) override
    {
        const long before = cells.lds_step_launches;
        cells.d_gabriel_coefficients = coefficients.get();
        step<Pt, pw_int, pw_friction, false>(cells, *this, l, dt, n_steps);
        lds_ran = cells.lds_step_launches != before;
        return cells.lds_step_launches - before;
    }
    int set_param(const std::string& name, double v) override
    {
        if (name == "lds_steps")
            cells.lds_steps = (int)v;
        else if (name == "steps_per_launch")
            cells.lds_steps_max = (int)v;
        else if (name == "cube_size")
            cells.cube_size = (float)v;
        else if (name == "gabriel_coefficient")
            cells.gabriel_coefficient = (float)v;
        else
            return -3;
        return 0;
    }
    bool lds_ran = false;
    int lanes_used() override { return lds_ran ? 1 : 0; }  // (the Gabriel force has one shape)
    int dense_cells() override { return cells.dense_cells(); }
    long long lds_dense_cells() override { return (long long)cells.lds_dense_cells(); }
    bool has_coefficients() override { return true; }
};

using Factory = Sweep* (*)(int, int, int, int, float, float);
struct Form {
    const char* name;
    const Model<Factory>* models;
    const bool* linked;
    int n_models;
};

// (name, point type, pairwise force, friction, linked): per form a stateless 3-float model, one that is not declared
// stateless, a wide point type and, where the form has links, a model with links that a lone Solution steps too.
#define YA_SWP_TILE_MODELS(X, Sim)                                                        \
    X(Sim, "relu", float3, relu_force<float3>, friction_w_neighbour<float3>, false)       \
    X(Sim, "springs", float3, models::spring, friction_w_neighbour<float3>, false)        \
    X(Sim, "relu_po", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, false) \
    X(Sim, "links", float3, models::no_pw_int<float3>, friction_w_neighbour<float3>, true)
#define YA_SWP_GRID_MODELS(X, Sim)                                                        \
    X(Sim, "relu", float3, relu_force<float3>, friction_w_neighbour<float3>, false)       \
    X(Sim, "springs", float3, models::spring, friction_w_neighbour<float3>, false)        \
    X(Sim, "relu_po", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, false) \
    X(Sim, "springs_links", float3, models::spring, friction_w_neighbour<float3>, true)
#define YA_SWP_GABRIEL_MODELS(X, Sim)                                                      \
    X(Sim, "relu", float3, relu_force<float3>, friction_w_neighbour<float3>, false)        \
    X(Sim, "relu_plain", float3, models::relu_plain, friction_w_neighbour<float3>, false)  \
    X(Sim, "relu_po", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, false)

#define YA_SWP_ROW(Sim, name, Pt, pw_int, pw_friction, linked) \
    {name, &ens_harness::make_sim<Sim<Pt, pw_int, pw_friction, linked>>},
#define YA_SWP_LINKED(Sim, name, Pt, pw_int, pw_friction, linked) linked,
static const Model<Factory> tile_models[] = {YA_SWP_TILE_MODELS(YA_SWP_ROW, Tile_sim)};
static const bool tile_linked[] = {YA_SWP_TILE_MODELS(YA_SWP_LINKED, Tile_sim)};
static const Model<Factory> grid_models[] = {YA_SWP_GRID_MODELS(YA_SWP_ROW, Grid_sim)};
static const bool grid_linked[] = {YA_SWP_GRID_MODELS(YA_SWP_LINKED, Grid_sim)};
static const Model<Factory> gabriel_models[] = {YA_SWP_GABRIEL_MODELS(YA_SWP_ROW, Gabriel_sim)};
static const bool gabriel_linked[] = {YA_SWP_GABRIEL_MODELS(YA_SWP_LINKED, Gabriel_sim)};
#undef YA_SWP_ROW
#undef YA_SWP_LINKED

static const Form forms[] = {
    {"tile", tile_models, tile_linked, (int)(sizeof(tile_models) / sizeof(tile_models[0]))},
    {"grid", grid_models, grid_linked, (int)(sizeof(grid_models) / sizeof(grid_models[0]))},
    {"gabriel", gabriel_models, gabriel_linked, (int)(sizeof(gabriel_models) / sizeof(gabriel_models[0]))},
};
const Form* form_of(const char* name)
{
    if (!name) return nullptr;
    for (const Form& f : forms)
        if (std::string(name) == f.name) return &f;
    return nullptr;
}

}  // namespace swp_harness

struct ya_swp {
    std::unique_ptr<swp_harness::Sweep> p;
};

extern "C" {

int ya_swp_models_count(const char* form)
{
    const swp_harness::Form* f = swp_harness::form_of(form);
    return f ? f->n_models : -4;
}
const char* ya_swp_models_name(const char* form, int i)
{
    const swp_harness::Form* f = swp_harness::form_of(form);
    return f ? ens_harness::name_at(f->models, f->n_models, i) : nullptr;
}

int ya_swp_create(const char* form, const char* model, int n_replicas, int n_max, int slots_per_replica, int grid_size,
    float cube_size, float gabriel_coefficient, ya_swp** out)
{
    if (!form || !model || !out || slots_per_replica < 0) return -3;
    const swp_harness::Form* f = swp_harness::form_of(form);
    if (!f) return -4;
    // what the classes refuse (include/ensemble.cuh, include/ensemble_grid.cuh; no limit depends on the point type)
    if (n_replicas <= 0 || n_max <= 0) return -3;
    if ((size_t)n_replicas * (size_t)n_max > (size_t)0x7fffffff) return -3;
    if ((size_t)n_replicas * (size_t)((n_max + 3) / 4) > (size_t)0x7fffffff) return -3;
    if ((size_t)n_replicas * (size_t)slots_per_replica > (size_t)0x7fffffff) return -3;
    if (f != &swp_harness::forms[0]) {
        if (!Ensemble<float3, Grid_solver>::sizes_ok(n_replicas, n_max, grid_size) || !(cube_size > 0)) return -3;
        if (f == &swp_harness::forms[2] && !std::isfinite(gabriel_coefficient)) return -3;
    }
    const auto* row = ens_harness::find(f->models, f->n_models, model);
    if (!row) return -1;
    if (slots_per_replica > 0 && !f->linked[row - f->models]) return -3;  // (slots for a model without links)
    return ens_harness::create(f->models, f->n_models, model, out, n_replicas, n_max, slots_per_replica, grid_size,
        cube_size, gabriel_coefficient);
}
void ya_swp_destroy(ya_swp* ens) { delete ens; }

int ya_swp_n_floats(ya_swp* e) { return e->p->replicas().n_floats(); }
float* ya_swp_h_X(ya_swp* e) { return e->p->replicas().h_X(); }
int ya_swp_set_h_n(ya_swp* e, int r, int n) { return ens_harness::set_h_n(e->p->replicas(), r, n); }
int ya_swp_get_h_n(ya_swp* e, int r) { return ens_harness::get_h_n(e->p->replicas(), r); }
int ya_swp_get_d_n(ya_swp* e, int r) { return ens_harness::get_d_n(e->p->replicas(), r); }
int ya_swp_copy_to_device(ya_swp* e) { return ens_harness::copy_to_device(e->p->replicas()); }
int ya_swp_copy_to_host(ya_swp* e) { return ens_harness::copy_to_host(e->p->replicas()); }
int* ya_swp_h_link(ya_swp* e) { return e->p->h_link(); }
int ya_swp_set_n_links(ya_swp* e, int n_links)
{
    if (!e->p->h_n_links() || n_links < 0 || n_links > e->p->n_slots()) return -3;
    *e->p->h_n_links() = n_links;
    return 0;
}
int ya_swp_get_n_links(ya_swp* e) { return e->p->h_n_links() ? *e->p->h_n_links() : 0; }

int ya_swp_set_dt(ya_swp* e, const float* h_dt)
{
    if (!e) return -3;
    if (h_dt)
        e->p->dt.upload(h_dt, e->p->replicas().n_replicas());
    else
        e->p->dt.clear();
    return 0;
}
int ya_swp_set_gabriel_coefficients(ya_swp* e, const float* h)
{
    if (!e || !e->p->has_coefficients()) return -3;
    if (h)
        e->p->coefficients.upload(h, e->p->replicas().n_replicas());
    else
        e->p->coefficients.clear();
    return 0;
}
int ya_swp_scale_dt(ya_swp* e, float factor)
{
    if (!e || !e->p->dt.get()) return -3;
    const int n = e->p->replicas().n_replicas();
    swp_harness::scale_floats<<<(n + 255) / 256, 256>>>(n, e->p->dt.d, factor);  // queued, not waited for
    return 0;
}
int ya_swp_take_steps(ya_swp* e, float dt, int n_steps) { return (int)e->p->take_steps(dt, n_steps); }
int ya_swp_synchronize(ya_swp*) { return ens_harness::synchronize(); }
int ya_swp_set_fixed(ya_swp* e, int mode, int local_point)
{
    return ens_harness::set_fixed(e->p->replicas(), mode, local_point);
}
int ya_swp_get_old_v(ya_swp* e, float* out) { return ens_harness::get_old_v(e->p->replicas(), out); }
int ya_swp_set_old_v(ya_swp* e, const float* in) { return ens_harness::set_old_v(e->p->replicas(), in); }
int ya_swp_status(ya_swp* e, int r, int clear)
{
    return e->p->grid() ? ens_harness::status(*e->p->grid(), r, clear) : -3;
}
int ya_swp_get_grid(ya_swp* e, int r, int* cube_id, int* point_id, int* cube_start, int* cube_end)
{
    return e->p->grid() ? ens_harness::get_grid(*e->p->grid(), r, cube_id, point_id, cube_start, cube_end) : -3;
}
int ya_swp_lanes_used(ya_swp* e) { return e ? e->p->lanes_used() : -3; }
int ya_swp_dense_cells(ya_swp* e)
{
    if (!e) return -3;
    YA_CHECK(ya_device_synchronize());
    return e->p->dense_cells();
}
long long ya_swp_lds_dense_cells(ya_swp* e)
{
    if (!e) return -3;
    YA_CHECK(ya_device_synchronize());
    return e->p->lds_dense_cells();
}
int ya_swp_set_param(ya_swp* e, const char* name, double v)
{
    if (!name) return -3;
    const std::string which = name;
    const bool mode = which == "whole_steps" || which == "lds_steps";
    const bool lanes = which == "whole_step_lanes" || which == "lds_step_lanes";
    if (!mode && !lanes && which != "steps_per_launch" && which != "gabriel_coefficient" && which != "cube_size") return -2;
    if (!e) return -3;
    if (mode && v != -1 && v != 0 && v != 1) return -3;
    if (lanes && v != 0 && v != 1 && v != 4 && v != 16 && v != 64) return -3;
    if (which == "steps_per_launch" && (!(v >= 1 && v <= 0x7fffffff) || v != (double)(int)v)) return -3;
    if (which == "gabriel_coefficient" && !std::isfinite((float)v)) return -3;
    if (which == "cube_size" && !((float)v > 0)) return -3;
    return e->p->set_param(which, v);
}

}  // extern "C"
