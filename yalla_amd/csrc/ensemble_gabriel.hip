// libyalla_ensemble_gabriel.so -- the Gabriel ensemble harness (include/yalla_ensemble_gabriel.h):
// Ensemble<Pt, Gabriel_solver> (include/ensemble_gabriel.cuh) instantiated for the functor / friction /
// generic-force triples of the `*_gabriel` models of the same names in libyalla_models.so (model_functors.h is
// included read-only for the functors and their YA_STATELESS declarations).  Links against libyalla_hip.so.
#include <cmath>

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "dtypes.cuh"
#include "inits.cuh"
#include "links.cuh"
#include "property.cuh"
#include "solvers.cuh"
#include "ensemble.cuh"

#include "model_functors.h"

#include "yalla_ensemble_gabriel.h"
#include "ensemble_harness.h"  // No_gen, Push_gen

namespace gabens_harness {
using ens_harness::No_gen;
using ens_harness::Push_gen;

struct Base {
    virtual ~Base() {}
    virtual int n_floats() = 0;
    virtual int n_replicas() = 0;
    virtual int n_max() = 0;
    virtual int n_cubes() = 0;
    virtual float* h_X() = 0;
    virtual int* h_n() = 0;
    virtual void copy_to_device() = 0;
    virtual void copy_to_host() = 0;
    virtual int get_d_n(int r) = 0;
    virtual void take_steps(float dt, int n_steps) = 0;
    virtual void set_fixed(int mode, int point) = 0;
    virtual void set_cube_size(float cube_size) = 0;
    virtual float3* d_old_v() = 0;
    virtual void set_gabriel_coefficient(float coefficient) = 0;
    virtual int dense_cells() = 0;
    virtual int status(int r, bool clear) = 0;
    virtual const int* d_cube_id() = 0;
    virtual const int* d_point_id() = 0;
    virtual const int* d_offs() = 0;
};

template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Policy>
struct Sim : public Base {
    Ensemble<Pt, Gabriel_solver> cells;
    Sim(int n_replicas, int n_max, int grid_size, float cube_size, float coefficient)
        : cells{n_replicas, n_max, grid_size, cube_size, coefficient}
    {
    }
    int n_floats() override { return sizeof(Pt) / sizeof(float); }
    int n_replicas() override { return cells.n_replicas; }
    int n_max() override { return cells.n_max; }
    int n_cubes() override { return cells.n_cubes; }
    float* h_X() override { return reinterpret_cast<float*>(cells.h_X); }
    int* h_n() override { return cells.h_n; }
    void copy_to_device() override { cells.copy_to_device(); }
    void copy_to_host() override { cells.copy_to_host(); }
    int get_d_n(int r) override { return cells.get_d_n(r); }
    void take_steps(float dt, int n_steps) override
    {
        Policy::before_steps(cells.n_max);
        Generic_forces<Pt> gen = Policy::gen(cells.n_replicas, cells.n_max);
        for (int s = 0; s < n_steps; s++) cells.template take_step<pw_int, pw_friction>(dt, gen);
    }
    void set_fixed(int mode, int point) override
    {
        if (mode == 0) cells.set_fixed();
        if (mode == 1) cells.set_fixed(point);
        if (mode == 2) cells.set_fixed_xy(point);
    }
    void set_cube_size(float cube_size) override { cells.cube_size = cube_size; }
    float3* d_old_v() override { return cells.d_old_v; }
    void set_gabriel_coefficient(float coefficient) override { cells.gabriel_coefficient = coefficient; }
    int dense_cells() override { return cells.dense_cells(); }
    int status(int r, bool clear) override { return cells.status(r, clear); }
    const int* d_cube_id() override { return cells.d_cube_id; }
    const int* d_point_id() override { return cells.d_point_id; }
    const int* d_offs() override { return cells.d_offs; }
};

using Factory = Base* (*)(int, int, int, float, float);
struct Model {
    const char* name;
    Factory make;
};
template<typename S>
Base* make_sim(int n_replicas, int n_max, int grid_size, float cube_size, float coefficient)
{
    return new S{n_replicas, n_max, grid_size, cube_size, coefficient};
}
#define YA_GABENS_MODEL(name, Pt, pw_int, pw_friction, Policy) \
    Model { name, &make_sim<Sim<Pt, pw_int, pw_friction, Policy>> }

static const Model model_table[] = {
    YA_GABENS_MODEL("relu", float3, relu_force<float3>, friction_w_neighbour<float3>, No_gen<float3>),
    YA_GABENS_MODEL("clipped", float3, models::clipped_spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_GABENS_MODEL("relu_plain", float3, models::relu_plain, friction_w_neighbour<float3>, No_gen<float3>),
    YA_GABENS_MODEL("relu_po", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, No_gen<Po_cell>),
    YA_GABENS_MODEL("relu_cell", Cell, relu_force<Cell>, friction_w_neighbour<Cell>, No_gen<Cell>),
    YA_GABENS_MODEL("clipped_push", float3, models::clipped_spring, friction_w_neighbour<float3>, Push_gen<float3>),
};
static const int n_models = sizeof(model_table) / sizeof(model_table[0]);

}  // namespace gabens_harness

struct ya_gabens {
    std::unique_ptr<gabens_harness::Base> p;
};

extern "C" {

int ya_gabens_models_count(void) { return gabens_harness::n_models; }
const char* ya_gabens_models_name(int i)
{
    return (i >= 0 && i < gabens_harness::n_models) ? gabens_harness::model_table[i].name : nullptr;
}

int ya_gabens_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size,
    float gabriel_coefficient, ya_gabens** out)
{
    if (!model || !out) return -3;
    // what the class refuses (include/ensemble_grid.cuh, Grid_form; the limits do not depend on the point type)
    if (!Ensemble<float3, Gabriel_solver>::sizes_ok(n_replicas, n_max, grid_size) || !(cube_size > 0)) return -3;
    if (!std::isfinite(gabriel_coefficient)) return -3;
    for (int i = 0; i < gabens_harness::n_models; i++) {
        if (std::string(model) == gabens_harness::model_table[i].name) {
            ya_gabens* e = new ya_gabens;
            e->p.reset(gabens_harness::model_table[i].make(n_replicas, n_max, grid_size, cube_size, gabriel_coefficient));
            *out = e;
            return 0;
        }
    }
    return -1;
}
void ya_gabens_destroy(ya_gabens* ens) { delete ens; }

int ya_gabens_n_floats(ya_gabens* e) { return e->p->n_floats(); }
float* ya_gabens_h_X(ya_gabens* e) { return e->p->h_X(); }
int ya_gabens_set_h_n(ya_gabens* e, int r, int n)
{
    if (r < 0 || r >= e->p->n_replicas() || n < 0 || n > e->p->n_max()) return -3;
    e->p->h_n()[r] = n;
    return 0;
}
int ya_gabens_get_h_n(ya_gabens* e, int r)
{
    if (r < 0 || r >= e->p->n_replicas()) return -3;
    return e->p->h_n()[r];
}
int ya_gabens_get_d_n(ya_gabens* e, int r)
{
    if (r < 0 || r >= e->p->n_replicas()) return -3;
    return e->p->get_d_n(r);
}
int ya_gabens_copy_to_device(ya_gabens* e)
{
    e->p->copy_to_device();
    return 0;
}
int ya_gabens_copy_to_host(ya_gabens* e)
{
    e->p->copy_to_host();
    return 0;
}
int ya_gabens_take_steps(ya_gabens* e, float dt, int n_steps)
{
    e->p->take_steps(dt, n_steps);
    return 0;
}
int ya_gabens_synchronize(ya_gabens*)
{
    YA_CHECK(ya_device_synchronize());
    return 0;
}
int ya_gabens_set_fixed(ya_gabens* e, int mode, int local_point)
{
    if (mode < 0 || mode > 2) return -3;
    if (mode != 0 && (local_point < 0 || local_point >= e->p->n_max())) return -3;
    e->p->set_fixed(mode, local_point);
    return 0;
}
int ya_gabens_set_cube_size(ya_gabens* e, float cube_size)
{
    if (!(cube_size > 0)) return -3;
    e->p->set_cube_size(cube_size);
    return 0;
}
int ya_gabens_get_old_v(ya_gabens* e, float* out)
{
    if (!out) return -3;
    YA_CHECK(ya_device_synchronize());
    YA_CHECK(ya_memcpy_d2h(out, e->p->d_old_v(), (size_t)e->p->n_replicas() * e->p->n_max() * 3 * sizeof(float)));
    return 0;
}
int ya_gabens_set_old_v(ya_gabens* e, const float* in)
{
    if (!in) return -3;
    YA_CHECK(ya_device_synchronize());
    YA_CHECK(ya_memcpy_h2d(e->p->d_old_v(), in, (size_t)e->p->n_replicas() * e->p->n_max() * 3 * sizeof(float)));
    return 0;
}
int ya_gabens_status(ya_gabens* e, int r, int clear)
{
    if (r < 0 || r >= e->p->n_replicas()) return -3;
    YA_CHECK(ya_device_synchronize());
    return e->p->status(r, clear != 0);
}
int ya_gabens_get_grid(ya_gabens* e, int r, int* cube_id, int* point_id, int* cube_start, int* cube_end)
{
    if (r < 0 || r >= e->p->n_replicas()) return -3;
    const size_t n_max = e->p->n_max(), n_cubes = e->p->n_cubes();
    YA_CHECK(ya_device_synchronize());
    if (cube_id) YA_CHECK(ya_memcpy_d2h(cube_id, e->p->d_cube_id() + r * n_max, n_max * sizeof(int)));
    if (point_id) YA_CHECK(ya_memcpy_d2h(point_id, e->p->d_point_id() + r * n_max, n_max * sizeof(int)));
    if (cube_start || cube_end) {
        // Grid's cube_start / cube_end from the replica's offs (not on the step's path)
        std::vector<int> offs(n_cubes + 1);
        YA_CHECK(ya_memcpy_d2h(offs.data(), e->p->d_offs() + r * (n_cubes + 1), offs.size() * sizeof(int)));
        const bool built = offs[n_cubes] >= 0;  // (never built: what a fresh Grid holds)
        for (size_t c = 0; c < n_cubes; c++) {
            const bool some = built && offs[c + 1] > offs[c];
            if (cube_start) cube_start[c] = some ? offs[c] : -1;
            if (cube_end) cube_end[c] = some ? offs[c + 1] - 1 : (built ? -2 : -1);
        }
    }
    return 0;
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
