// libyalla_ensemble_gabriel_lds.so -- the Gabriel ensemble harness whose take_steps can step from LDS
// (include/yalla_ensemble_gabriel_lds.h): Ensemble<Pt, Gabriel_solver>::take_steps (include/ensemble_gabriel.cuh)
// instantiated for the model table of libyalla_ensemble_gabriel.so (ensemble_gabriel_models.h).  Links against
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

#include "yalla_ensemble_gabriel_lds.h"
#include "ensemble_harness.h"  // No_gen, Push_gen, Grid_replicas, Grid_replicas_of, Model, the entry points' bodies
#include "ensemble_gabriel_models.h"
#ifdef YA_MODELS_WIDTHS
#include "ensemble_widths_models.h"  // libyalla_ensemble_gabriel_lds_widths.so: another table (tests only)
#undef YA_GABRIEL_ENSEMBLE_MODELS
#define YA_GABRIEL_ENSEMBLE_MODELS(X) YA_WIDTHS_ENSEMBLE_MODELS(X)
#endif

namespace gablds_harness {
using ens_harness::No_gen;
using ens_harness::Push_gen;
using ens_harness::Grid_replicas;
using ens_harness::Grid_replicas_of;
using ens_harness::Model;

// What this harness adds to the shared interface.
struct Base : public Grid_replicas {
    virtual long take_steps(float dt, int n_steps) = 0;  // returns the launches that stepped from LDS
    virtual void set_gabriel_coefficient(float coefficient) = 0;
    virtual int dense_cells() = 0;
    virtual long long lds_dense_cells() = 0;
    virtual void set_lds_steps(int mode) = 0;
    virtual void set_lds_steps_max(int steps) = 0;
};

template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Policy>
struct Sim : public Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Base> {
    using Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Base>::cells;
    // the harness's own default: the 16-launch step, as libyalla_ensemble_gabriel.so runs
    template<typename... Args>
    explicit Sim(Args... args) : Grid_replicas_of<Ensemble<Pt, Gabriel_solver>, Base>{args...}
    {
        cells.lds_steps = -1;
    }
    long take_steps(float dt, int n_steps) override
    {
        Policy::before_steps(cells.n_max);
        const long before = cells.lds_step_launches;
        cells.template take_steps<pw_int, pw_friction>(dt, n_steps, Policy::gen(cells.n_replicas, cells.n_max));
        return cells.lds_step_launches - before;
    }
    void set_gabriel_coefficient(float coefficient) override { cells.gabriel_coefficient = coefficient; }
    int dense_cells() override { return cells.dense_cells(); }
    long long lds_dense_cells() override { return (long long)cells.lds_dense_cells(); }
    void set_lds_steps(int mode) override { cells.lds_steps = mode; }
    void set_lds_steps_max(int steps) override { cells.lds_steps_max = steps; }
};

template<typename Pt>
long lds_bytes_of(int n_max)
{
    return n_max <= ya::ens::WHOLE_STEP_MAX_ROWS ? (long)ya::ens::gabriel_lds_layout<Pt>(n_max).bytes : 0;
}

#define YA_GABRIEL_ROW(name, Pt, pw_int, pw_friction, Policy) YA_ENSEMBLE_MODEL(name, Pt, pw_int, pw_friction, Policy),
static const Model<Base* (*)(int, int, int, float, float)> model_table[] = {YA_GABRIEL_ENSEMBLE_MODELS(YA_GABRIEL_ROW)};
#undef YA_GABRIEL_ROW
static const int n_models = sizeof(model_table) / sizeof(model_table[0]);
// the LDS rule of each model's point type, in the table's order
#define YA_GABRIEL_ROW(name, Pt, pw_int, pw_friction, Policy) &lds_bytes_of<Pt>,
static long (*const lds_table[])(int) = {YA_GABRIEL_ENSEMBLE_MODELS(YA_GABRIEL_ROW)};
#undef YA_GABRIEL_ROW

}  // namespace gablds_harness

struct ya_gablds {
    std::unique_ptr<gablds_harness::Base> p;
};

extern "C" {

int ya_gablds_models_count(void) { return gablds_harness::n_models; }
const char* ya_gablds_models_name(int i)
{
    return ens_harness::name_at(gablds_harness::model_table, gablds_harness::n_models, i);
}

int ya_gablds_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size,
    float gabriel_coefficient, ya_gablds** out)
{
    if (!model || !out) return -3;
    // what the class refuses (include/ensemble_grid.cuh, Grid_form; the limits do not depend on the point type)
    if (!Ensemble<float3, Gabriel_solver>::sizes_ok(n_replicas, n_max, grid_size) || !(cube_size > 0)) return -3;
    if (!std::isfinite(gabriel_coefficient)) return -3;
    return ens_harness::create(gablds_harness::model_table, gablds_harness::n_models, model, out,
        n_replicas, n_max, grid_size, cube_size, gabriel_coefficient);
}
void ya_gablds_destroy(ya_gablds* ens) { delete ens; }

int ya_gablds_n_floats(ya_gablds* e) { return e->p->n_floats(); }
float* ya_gablds_h_X(ya_gablds* e) { return e->p->h_X(); }
int ya_gablds_set_h_n(ya_gablds* e, int r, int n) { return ens_harness::set_h_n(*e->p, r, n); }
int ya_gablds_get_h_n(ya_gablds* e, int r) { return ens_harness::get_h_n(*e->p, r); }
int ya_gablds_get_d_n(ya_gablds* e, int r) { return ens_harness::get_d_n(*e->p, r); }
int ya_gablds_copy_to_device(ya_gablds* e) { return ens_harness::copy_to_device(*e->p); }
int ya_gablds_copy_to_host(ya_gablds* e) { return ens_harness::copy_to_host(*e->p); }
int ya_gablds_take_steps(ya_gablds* e, float dt, int n_steps) { return (int)e->p->take_steps(dt, n_steps); }
int ya_gablds_synchronize(ya_gablds*) { return ens_harness::synchronize(); }
int ya_gablds_set_fixed(ya_gablds* e, int mode, int local_point)
{
    return ens_harness::set_fixed(*e->p, mode, local_point);
}
int ya_gablds_set_cube_size(ya_gablds* e, float cube_size) { return ens_harness::set_cube_size(*e->p, cube_size); }
int ya_gablds_get_old_v(ya_gablds* e, float* out) { return ens_harness::get_old_v(*e->p, out); }
int ya_gablds_set_old_v(ya_gablds* e, const float* in) { return ens_harness::set_old_v(*e->p, in); }
int ya_gablds_status(ya_gablds* e, int r, int clear) { return ens_harness::status(*e->p, r, clear); }
int ya_gablds_get_grid(ya_gablds* e, int r, int* cube_id, int* point_id, int* cube_start, int* cube_end)
{
    return ens_harness::get_grid(*e->p, r, cube_id, point_id, cube_start, cube_end);
}
int ya_gablds_dense_cells(ya_gablds* e)
{
    YA_CHECK(ya_device_synchronize());
    return e->p->dense_cells();
}
long long ya_gablds_lds_dense_cells(ya_gablds* e)
{
    if (!e) return -3;
    YA_CHECK(ya_device_synchronize());
    return e->p->lds_dense_cells();
}
int ya_gablds_set_param(ya_gablds* e, const char* name, double v)
{
    if (!name) return -3;
    const std::string which = name;
    if (which != "gabriel_coefficient" && which != "lds_steps" && which != "lds_steps_max") return -2;
    if (!e) return -3;
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
    if (!std::isfinite((float)v)) return -3;
    e->p->set_gabriel_coefficient((float)v);
    return 0;
}

long ya_gablds_lds_bytes(const char* model, int n_max)
{
    if (!model || n_max <= 0) return -3;
    for (int i = 0; i < gablds_harness::n_models; i++)
        if (std::string(model) == gablds_harness::model_table[i].name) return gablds_harness::lds_table[i](n_max);
    return -1;
}

}  // extern "C"
