// libyalla_ensemble_gabriel.so -- the Gabriel ensemble harness (include/yalla_ensemble_gabriel.h):
// Ensemble<Pt, Gabriel_solver> (include/ensemble_gabriel.cuh) instantiated for the functor / friction /
// generic-force triples of the `*_gabriel` models of the same names in libyalla_models.so (model_functors.h is
// included read-only for the functors and their YA_STATELESS declarations).  Links against libyalla_hip.so.
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

#include "yalla_ensemble_gabriel.h"
#include "ensemble_harness.h"  // No_gen, Push_gen, Grid_replicas, Grid_replicas_of, Model, the entry points' bodies
#include "ensemble_gabriel_models.h"

namespace gabens_harness {
using ens_harness::No_gen;
using ens_harness::Push_gen;
using ens_harness::Grid_replicas;
using ens_harness::Grid_replicas_of;
using ens_harness::Model;

// What the Gabriel form adds to the shared interface.
struct Base : public Grid_replicas {
    virtual void take_steps(float dt, int n_steps) = 0;
    virtual void set_gabriel_coefficient(float coefficient) = 0;
    virtual int dense_cells() = 0;
};

template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Policy>
struct Sim : public Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Base> {
    using Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Base>::Grid_replicas_of;
    using Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Base>::cells;
    void take_steps(float dt, int n_steps) override
    {
        ens_harness::step_by_step<Pt, pw_int, pw_friction, Policy>(cells, dt, n_steps);
    }
    void set_gabriel_coefficient(float coefficient) override { cells.gabriel_coefficient = coefficient; }
    int dense_cells() override { return cells.dense_cells(); }
};

// (the table is ensemble_gabriel_models.h's, shared with ensemble_gabriel_lds.hip)
#define YA_GABRIEL_ROW(name, Pt, pw_int, pw_friction, Policy) YA_ENSEMBLE_MODEL(name, Pt, pw_int, pw_friction, Policy),
static const Model<Base* (*)(int, int, int, float, float)> model_table[] = {YA_GABRIEL_ENSEMBLE_MODELS(YA_GABRIEL_ROW)};
#undef YA_GABRIEL_ROW
static const int n_models = sizeof(model_table) / sizeof(model_table[0]);

}  // namespace gabens_harness

struct ya_gabens {
    std::unique_ptr<gabens_harness::Base> p;
};

extern "C" {

int ya_gabens_models_count(void) { return gabens_harness::n_models; }
const char* ya_gabens_models_name(int i)
{
    return ens_harness::name_at(gabens_harness::model_table, gabens_harness::n_models, i);
}

int ya_gabens_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size,
    float gabriel_coefficient, ya_gabens** out)
{
    if (!model || !out) return -3;
    // what the class refuses (include/ensemble_grid.cuh, Grid_form; the limits do not depend on the point type)
    if (!Ensemble<float3, Gabriel_solver>::sizes_ok(n_replicas, n_max, grid_size) || !(cube_size > 0)) return -3;
    if (!std::isfinite(gabriel_coefficient)) return -3;
    return ens_harness::create(gabens_harness::model_table, gabens_harness::n_models, model, out,
        n_replicas, n_max, grid_size, cube_size, gabriel_coefficient);
}
void ya_gabens_destroy(ya_gabens* ens) { delete ens; }

int ya_gabens_n_floats(ya_gabens* e) { return e->p->n_floats(); }
float* ya_gabens_h_X(ya_gabens* e) { return e->p->h_X(); }
int ya_gabens_set_h_n(ya_gabens* e, int r, int n) { return ens_harness::set_h_n(*e->p, r, n); }
int ya_gabens_get_h_n(ya_gabens* e, int r) { return ens_harness::get_h_n(*e->p, r); }
int ya_gabens_get_d_n(ya_gabens* e, int r) { return ens_harness::get_d_n(*e->p, r); }
int ya_gabens_copy_to_device(ya_gabens* e) { return ens_harness::copy_to_device(*e->p); }
int ya_gabens_copy_to_host(ya_gabens* e) { return ens_harness::copy_to_host(*e->p); }
int ya_gabens_take_steps(ya_gabens* e, float dt, int n_steps) { return ens_harness::take_steps(*e->p, dt, n_steps); }
int ya_gabens_synchronize(ya_gabens*) { return ens_harness::synchronize(); }
int ya_gabens_set_fixed(ya_gabens* e, int mode, int local_point)
{
    return ens_harness::set_fixed(*e->p, mode, local_point);
}
int ya_gabens_set_cube_size(ya_gabens* e, float cube_size) { return ens_harness::set_cube_size(*e->p, cube_size); }
int ya_gabens_get_old_v(ya_gabens* e, float* out) { return ens_harness::get_old_v(*e->p, out); }
int ya_gabens_set_old_v(ya_gabens* e, const float* in) { return ens_harness::set_old_v(*e->p, in); }
int ya_gabens_status(ya_gabens* e, int r, int clear) { return ens_harness::status(*e->p, r, clear); }
int ya_gabens_get_grid(ya_gabens* e, int r, int* cube_id, int* point_id, int* cube_start, int* cube_end)
{
    return ens_harness::get_grid(*e->p, r, cube_id, point_id, cube_start, cube_end);
}
int ya_gabens_dense_cells(ya_gabens* e)
{
    YA_CHECK(ya_device_synchronize());
    return e->p->dense_cells();
}
int ya_gabens_set_param(ya_gabens* e, const char* name, double v)
{
    if (!name) return -3;
    if (std::string(name) != "gabriel_coefficient") return -2;  // ("lanes", "sum_order": the grid ensemble's)
    if (!e || !std::isfinite((float)v)) return -3;
    e->p->set_gabriel_coefficient((float)v);
    return 0;
}

}  // extern "C"
