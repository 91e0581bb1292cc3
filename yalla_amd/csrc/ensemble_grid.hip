// libyalla_ensemble_grid.so -- the grid ensemble harness (include/yalla_ensemble_grid.h): Ensemble<Pt, Grid_solver>
// (include/ensemble_grid.cuh) instantiated for the functor / friction / generic-force triples of the `*_grid`
// models of the same names in libyalla_models.so (model_functors.h is included read-only for the functors and
// their YA_STATELESS declarations).  Links against libyalla_hip.so.
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

#include "yalla_ensemble_grid.h"
#include "ensemble_harness.h"  // No_gen, Push_gen, Grid_replicas, Grid_replicas_of, Model, the entry points' bodies
#ifdef YA_MODELS_WIDTHS
#include "ensemble_widths_models.h"  // libyalla_ensemble_grid_widths.so: another table (tests only)
#endif

namespace gens_harness {
using ens_harness::No_gen;
using ens_harness::Push_gen;
using ens_harness::Grid_replicas;
using ens_harness::Grid_replicas_of;
using ens_harness::Model;

// What the grid form adds to the shared interface.
struct Base : public Grid_replicas {
    virtual long take_steps(float dt, int n_steps) = 0;  // returns the launches that stepped from LDS
    virtual void set_lanes(int lanes) = 0;
    virtual void set_sum_order(int order) = 0;
    virtual void set_lds_steps(int mode) = 0;
    virtual void set_lds_steps_max(int steps) = 0;
    virtual void set_lds_step_lanes(int lanes) = 0;
    virtual int lds_step_lanes_used() = 0;
};

template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Policy>
struct Sim : public Grid_replicas_of<Ensemble<Pt, Grid_solver>, Base> {
    using Grid_replicas_of<Ensemble<Pt, Grid_solver>, Base>::cells;
    // the harness's own defaults: the 14-launch step and one lane per cell in launches that step from LDS, so that
    // every caller runs what it ran before "lds_steps" and "lds_step_lanes" existed
    template<typename... Args>
    explicit Sim(Args... args) : Grid_replicas_of<Ensemble<Pt, Grid_solver>, Base>{args...}
    {
        cells.lds_steps = -1;
        cells.lds_step_lanes = 1;
    }
    long take_steps(float dt, int n_steps) override
    {
        Policy::before_steps(cells.n_max);
        const long before = cells.lds_step_launches;
        cells.template take_steps<pw_int, pw_friction>(dt, n_steps, Policy::gen(cells.n_replicas, cells.n_max));
        return cells.lds_step_launches - before;
    }
    void set_lds_steps(int mode) override { cells.lds_steps = mode; }
    void set_lds_steps_max(int steps) override { cells.lds_steps_max = steps; }
    void set_lds_step_lanes(int lanes) override { cells.lds_step_lanes = lanes; }
    int lds_step_lanes_used() override { return cells.lds_step_lanes_used; }
    void set_lanes(int lanes) override { cells.lanes_per_cell = lanes; }
    void set_sum_order(int order) override { cells.sum_order = order ? YA_SUM_BY_PLANE : YA_SUM_REFERENCE; }
};

#ifdef YA_MODELS_WIDTHS
#define YA_WIDTHS_ROW_HERE(name, Pt, pw_int, pw_friction, Policy) YA_ENSEMBLE_MODEL(name, Pt, pw_int, pw_friction, Policy),
static const Model<Base* (*)(int, int, int, float)> model_table[] = {YA_WIDTHS_GRID_ENSEMBLE_MODELS(YA_WIDTHS_ROW_HERE)};
#undef YA_WIDTHS_ROW_HERE
#else
static const Model<Base* (*)(int, int, int, float)> model_table[] = {
    YA_ENSEMBLE_MODEL("springs", float3, models::spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_ENSEMBLE_MODEL("clipped", float3, models::clipped_spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_ENSEMBLE_MODEL("fading", float3, models::fading_spring, friction_on_background<float3>, No_gen<float3>),
    YA_ENSEMBLE_MODEL("relu", float3, relu_force<float3>, friction_w_neighbour<float3>, No_gen<float3>),
    YA_ENSEMBLE_MODEL("relu_po", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, No_gen<Po_cell>),
    YA_ENSEMBLE_MODEL("relu_cell", Cell, relu_force<Cell>, friction_w_neighbour<Cell>, No_gen<Cell>),
    YA_ENSEMBLE_MODEL("push", float3, models::no_pw_int<float3>, friction_w_neighbour<float3>, Push_gen<float3>),
    YA_ENSEMBLE_MODEL("clipped_push", float3, models::clipped_spring, friction_w_neighbour<float3>, Push_gen<float3>),
    // user-written frictions (model_functors.h; tests/test_friction_functors_gpu.py): ids through local ids
    // (ensemble_harness.h), declared and `_plain`, and field on the wide point
    YA_ENSEMBLE_MODEL("friction_ids", float3, relu_force<float3>, ens_harness::friction_by_local_id<models::ids_friction>, ens_harness::Local_friction_ids),
    YA_ENSEMBLE_MODEL("friction_ids_plain", float3, relu_force<float3>, ens_harness::friction_by_local_id<models::ids_friction_plain>, ens_harness::Local_friction_ids),
    YA_ENSEMBLE_MODEL("friction_field", Po_cell, relu_force<Po_cell>, models::field_friction, No_gen<Po_cell>),
};
#endif
static const int n_models = sizeof(model_table) / sizeof(model_table[0]);

}  // namespace gens_harness

struct ya_gens {
    std::unique_ptr<gens_harness::Base> p;
};

extern "C" {

int ya_gens_models_count(void) { return gens_harness::n_models; }
const char* ya_gens_models_name(int i)
{
    return ens_harness::name_at(gens_harness::model_table, gens_harness::n_models, i);
}

int ya_gens_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size, ya_gens** out)
{
    if (!model || !out) return -3;
    // what the class refuses (include/ensemble_grid.cuh; the limits do not depend on the point type)
    if (!Ensemble<float3, Grid_solver>::sizes_ok(n_replicas, n_max, grid_size) || !(cube_size > 0)) return -3;
    return ens_harness::create(gens_harness::model_table, gens_harness::n_models, model, out,
        n_replicas, n_max, grid_size, cube_size);
}
void ya_gens_destroy(ya_gens* ens) { delete ens; }

int ya_gens_n_floats(ya_gens* e) { return e->p->n_floats(); }
float* ya_gens_h_X(ya_gens* e) { return e->p->h_X(); }
int ya_gens_set_h_n(ya_gens* e, int r, int n) { return ens_harness::set_h_n(*e->p, r, n); }
int ya_gens_get_h_n(ya_gens* e, int r) { return ens_harness::get_h_n(*e->p, r); }
int ya_gens_get_d_n(ya_gens* e, int r) { return ens_harness::get_d_n(*e->p, r); }
int ya_gens_copy_to_device(ya_gens* e) { return ens_harness::copy_to_device(*e->p); }
int ya_gens_copy_to_host(ya_gens* e) { return ens_harness::copy_to_host(*e->p); }
int ya_gens_take_steps(ya_gens* e, float dt, int n_steps) { return (int)e->p->take_steps(dt, n_steps); }
int ya_gens_synchronize(ya_gens*) { return ens_harness::synchronize(); }
int ya_gens_set_fixed(ya_gens* e, int mode, int local_point)
{
    return ens_harness::set_fixed(*e->p, mode, local_point);
}
int ya_gens_set_cube_size(ya_gens* e, float cube_size) { return ens_harness::set_cube_size(*e->p, cube_size); }
int ya_gens_get_old_v(ya_gens* e, float* out) { return ens_harness::get_old_v(*e->p, out); }
int ya_gens_set_old_v(ya_gens* e, const float* in) { return ens_harness::set_old_v(*e->p, in); }
int ya_gens_status(ya_gens* e, int r, int clear) { return ens_harness::status(*e->p, r, clear); }
int ya_gens_get_grid(ya_gens* e, int r, int* cube_id, int* point_id, int* cube_start, int* cube_end)
{
    return ens_harness::get_grid(*e->p, r, cube_id, point_id, cube_start, cube_end);
}
int ya_gens_set_param(ya_gens* e, const char* name, double v)
{
    if (!name) return -3;
    const std::string which = name;
    if (which != "lanes" && which != "sum_order" && which != "lds_steps" && which != "lds_steps_max" &&
        !ens_harness::lds_lanes_name(which))
        return -2;
    if (!e) return -3;
    if (ens_harness::lds_lanes_name(which)) return ens_harness::lds_lanes_param(*e->p, which, v);
    if (which == "lds_steps") {
        if (v != -1 && v != 0 && v != 1) return -3;
        e->p->set_lds_steps((int)v);
        return 0;
    }
    if (which == "lds_steps_max") {
        if (!(v >= 1 && v <= 0x7fffffff) || v != (double)(int)v) return -3;
        e->p->set_lds_steps_max((int)v);
        return 0;
    }
    if (which == "lanes") {
        const int lanes = (int)v;
        if (lanes != 0 && lanes != 1 && lanes != 4 && lanes != 8 && lanes != 16) return -3;
        e->p->set_lanes(lanes);
        return 0;
    }
    const int order = (int)v;  // "sum_order"
    if (order != 0 && order != 1) return -3;
    e->p->set_sum_order(order);
    return 0;
}
}  // extern "C"
