// libyalla_ensemble_grid_links.so -- the linked grid ensemble harness (include/yalla_ensemble_grid_links.h):
// Ensemble<Pt, Grid_solver> (include/ensemble_grid.cuh) with a Links object over the flat id space, stepped by
// take_steps(dt, K, ya::ens::Replica_links) (include/ensemble_links.cuh), for the functor / friction pairs of the
// `links_grid` / `springs_links_grid` models of libyalla_models.so, of three pairwise models and of one 8-float
// point type (model_functors.h is included read-only for the functors and their YA_STATELESS declarations).
// Links against libyalla_hip.so.
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

#include "yalla_ensemble_grid_links.h"
#include "ensemble_harness.h"  // Grid_replicas(_of), Model, the entry points' bodies

// 8 floats: with 1024 rows the step's arrays and the keys leave 896 bytes of the workgroup's LDS, no room for a list
MAKE_PT(Cell8, theta, phi, u, v, w);

namespace glens_harness {
using ens_harness::Grid_replicas;
using ens_harness::Grid_replicas_of;
using ens_harness::Model;

// What the linked grid form adds to the shared interface.
struct Base : public Grid_replicas {
    virtual long take_steps(float dt, int n_steps) = 0;  // returns the launches that stepped from LDS
    virtual void set_sum_order(int order) = 0;
    virtual void set_lds_steps(int mode) = 0;
    virtual void set_lds_steps_max(int steps) = 0;
    virtual void set_lds_step_lanes(int lanes) = 0;
    virtual int lds_step_lanes_used() = 0;
    virtual void set_links_path(int path) = 0;
    virtual int* h_link() = 0;
    virtual int* h_n_links() = 0;
    virtual int n_slots() = 0;  // n_replicas * slots_per_replica
};

// (Policy is unused, always void: the parameter list is the one YA_ENSEMBLE_MODEL instantiates; the generic force
// here is the links, chosen by links_path.)
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Policy>
struct Sim : public Grid_replicas_of<Ensemble<Pt, Grid_solver>, Base> {
    using Grid_replicas_of<Ensemble<Pt, Grid_solver>, Base>::cells;
    const int slots_per_replica;
    Links links;  // (at least one slot: an object of no slots has nothing to allocate or launch)
    int links_path = 0;
    // The defaults of the grid harness: the 14-launch step, one lane per cell in launches that step from LDS.
    Sim(int n_replicas, int n_max, int grid_size, float cube_size, int slots_per_replica, float strength)
        : Grid_replicas_of<Ensemble<Pt, Grid_solver>, Base>{n_replicas, n_max, grid_size, cube_size},
          slots_per_replica{slots_per_replica},
          links{n_replicas * slots_per_replica > 0 ? n_replicas * slots_per_replica : 1, strength}
    {
        static_assert(sizeof(Link) == 2 * sizeof(int), "h_link is handed out as pairs of ints");
        cells.lds_steps = -1;
        cells.lds_step_lanes = 1;
        *links.h_n = n_slots();
        links.set_d_n(n_slots());
    }
    long take_steps(float dt, int n_steps) override
    {
        const long launches_before = cells.lds_step_launches;
        if (links_path == 0) {
            cells.template take_steps<pw_int, pw_friction>(dt, n_steps, ya::ens::Replica_links{links, slots_per_replica});
        } else {  // the way before the ordered forces: atomics, a memset per step, never from LDS
            Links* l = &links;
            Generic_forces<Pt> gen = [l](const int, const Pt* __restrict__ d_X, Pt* d_dX) {
                link_forces<Pt>(*l, d_X, d_dX);
            };
            cells.template take_steps<pw_int, pw_friction>(dt, n_steps, gen);
        }
        return cells.lds_step_launches - launches_before;
    }
    void copy_to_device() override
    {
        cells.copy_to_device();
        links.copy_to_device();
    }
    void set_sum_order(int order) override { cells.sum_order = order ? YA_SUM_BY_PLANE : YA_SUM_REFERENCE; }
    void set_lds_steps(int mode) override { cells.lds_steps = mode; }
    void set_lds_steps_max(int steps) override { cells.lds_steps_max = steps; }
    void set_lds_step_lanes(int lanes) override { cells.lds_step_lanes = lanes; }
    int lds_step_lanes_used() override { return cells.lds_step_lanes_used; }
    void set_links_path(int path) override { links_path = path; }
    int* h_link() override { return reinterpret_cast<int*>(links.h_link); }
    int* h_n_links() override { return links.h_n; }
    int n_slots() override { return cells.n_replicas * slots_per_replica; }
};

template<typename Pt>
long lds_bytes_of(int n_max, int slots)
{
    return (long)ya::ens::lds_layout<Pt, true, true>(n_max, slots, 1).bytes;
}

// (name, point type, pairwise force, friction)
#define YA_LINKED_GRID_MODELS(X)                                                      \
    X("links", float3, models::no_pw_int<float3>, friction_w_neighbour<float3>)       \
    X("links4", float4, models::no_pw_int<float4>, friction_w_neighbour<float4>)      \
    X("springs_links", float3, models::spring, friction_w_neighbour<float3>)          \
    X("relu_links", float3, relu_force<float3>, friction_w_neighbour<float3>)         \
    X("relu_po_links", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>)   \
    X("relu_cell8_links", Cell8, relu_force<Cell8>, friction_w_neighbour<Cell8>)

#define YA_LINKED_ROW(name, Pt, pw_int, pw_friction) YA_ENSEMBLE_MODEL(name, Pt, pw_int, pw_friction, void),
static const Model<Base* (*)(int, int, int, float, int, float)> model_table[] = {YA_LINKED_GRID_MODELS(YA_LINKED_ROW)};
#undef YA_LINKED_ROW
static const int n_models = sizeof(model_table) / sizeof(model_table[0]);
// the LDS rule of each model's point type, in the table's order
#define YA_LINKED_ROW(name, Pt, pw_int, pw_friction) &lds_bytes_of<Pt>,
static long (*const lds_table[])(int, int) = {YA_LINKED_GRID_MODELS(YA_LINKED_ROW)};
#undef YA_LINKED_ROW

}  // namespace glens_harness

struct ya_glens {
    std::unique_ptr<glens_harness::Base> p;
};

extern "C" {

int ya_glens_models_count(void) { return glens_harness::n_models; }
const char* ya_glens_models_name(int i)
{
    return ens_harness::name_at(glens_harness::model_table, glens_harness::n_models, i);
}

int ya_glens_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size, int slots_per_replica,
    float strength, ya_glens** out)
{
    if (!model || !out || slots_per_replica < 0 || !std::isfinite(strength)) return -3;
    // what the class refuses (include/ensemble_grid.cuh; the limits do not depend on the point type)
    if (!Ensemble<float3, Grid_solver>::sizes_ok(n_replicas, n_max, grid_size) || !(cube_size > 0)) return -3;
    if ((size_t)n_replicas * (size_t)slots_per_replica > (size_t)0x7fffffff) return -3;  // (slots are ints)
    return ens_harness::create(glens_harness::model_table, glens_harness::n_models, model, out, n_replicas, n_max,
        grid_size, cube_size, slots_per_replica, strength);
}
void ya_glens_destroy(ya_glens* ens) { delete ens; }

int ya_glens_n_floats(ya_glens* e) { return e->p->n_floats(); }
float* ya_glens_h_X(ya_glens* e) { return e->p->h_X(); }
int ya_glens_set_h_n(ya_glens* e, int r, int n) { return ens_harness::set_h_n(*e->p, r, n); }
int ya_glens_get_h_n(ya_glens* e, int r) { return ens_harness::get_h_n(*e->p, r); }
int ya_glens_get_d_n(ya_glens* e, int r) { return ens_harness::get_d_n(*e->p, r); }
int ya_glens_copy_to_device(ya_glens* e) { return ens_harness::copy_to_device(*e->p); }
int ya_glens_copy_to_host(ya_glens* e) { return ens_harness::copy_to_host(*e->p); }
int* ya_glens_h_link(ya_glens* e) { return e->p->h_link(); }
int ya_glens_set_n_links(ya_glens* e, int n_links)
{
    if (n_links < 0 || n_links > e->p->n_slots()) return -3;
    *e->p->h_n_links() = n_links;
    return 0;
}
int ya_glens_get_n_links(ya_glens* e) { return *e->p->h_n_links(); }
int ya_glens_take_steps(ya_glens* e, float dt, int n_steps) { return (int)e->p->take_steps(dt, n_steps); }
int ya_glens_synchronize(ya_glens*) { return ens_harness::synchronize(); }
int ya_glens_set_fixed(ya_glens* e, int mode, int local_point)
{
    return ens_harness::set_fixed(*e->p, mode, local_point);
}
int ya_glens_set_cube_size(ya_glens* e, float cube_size) { return ens_harness::set_cube_size(*e->p, cube_size); }
int ya_glens_get_old_v(ya_glens* e, float* out) { return ens_harness::get_old_v(*e->p, out); }
int ya_glens_set_old_v(ya_glens* e, const float* in) { return ens_harness::set_old_v(*e->p, in); }
int ya_glens_status(ya_glens* e, int r, int clear) { return ens_harness::status(*e->p, r, clear); }
int ya_glens_get_grid(ya_glens* e, int r, int* cube_id, int* point_id, int* cube_start, int* cube_end)
{
    return ens_harness::get_grid(*e->p, r, cube_id, point_id, cube_start, cube_end);
}
int ya_glens_set_param(ya_glens* e, const char* name, double v)
{
    if (!name) return -3;
    const std::string which = name;
    if (which != "sum_order" && which != "lds_steps" && which != "lds_steps_max" && which != "links_path" &&
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
    if (v != 0 && v != 1) return -3;  // "sum_order", "links_path"
    if (which == "links_path")
        e->p->set_links_path((int)v);
    else
        e->p->set_sum_order((int)v);
    return 0;
}

long ya_glens_lds_bytes(const char* model, int n_max, int slots_per_replica)
{
    if (!model || n_max <= 0 || slots_per_replica < 0) return -3;
    for (int i = 0; i < glens_harness::n_models; i++)
        if (std::string(model) == glens_harness::model_table[i].name)
            return glens_harness::lds_table[i](n_max, slots_per_replica);
    return -1;
}

}  // extern "C"
