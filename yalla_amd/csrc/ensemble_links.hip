// libyalla_ensemble_links.so -- the linked ensemble harness (include/yalla_ensemble_links.h):
// Ensemble<Pt, Tile_solver> (include/ensemble.cuh) with a Links object over the flat id space, stepped by
// take_steps(dt, K, ya::ens::Replica_links) (include/ensemble_links.cuh), for the functor / friction pairs of the
// link models of libyalla_models.so and of three pairwise models (model_functors.h is included read-only for the
// functors and their YA_STATELESS declarations).  Links against libyalla_hip.so.
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

#include "yalla_ensemble_links.h"
#include "ensemble_harness.h"  // Tile_replicas(_of), Model, the entry points' bodies

namespace lens_harness {
using ens_harness::Model;
using ens_harness::Tile_replicas;
using ens_harness::Tile_replicas_of;

// What the linked all-pairs form adds to the shared interface.
struct Base : public Tile_replicas {
    virtual int whole_step_lanes_used() = 0;
    virtual void set_links_path(int path) = 0;
    virtual int* h_link() = 0;
    virtual int* h_n_links() = 0;
    virtual int n_slots() = 0;  // n_replicas * slots_per_replica
};

// (Policy is unused, always void: the parameter list is the one YA_ENSEMBLE_MODEL instantiates; the generic force
// here is the links, chosen by links_path.)
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Policy>
struct Sim : public Tile_replicas_of<Ensemble<Pt>, Base> {
    using Tile_replicas_of<Ensemble<Pt>, Base>::cells;
    const int slots_per_replica;
    Links links;  // (at least one slot: an object of no slots has nothing to allocate or launch)
    int links_path = 0;
    // The defaults of the all-pairs harness: the six-launch step, one lane per cell inside a whole-step launch.
    Sim(int n_replicas, int n_max, int slots_per_replica, float strength)
        : Tile_replicas_of<Ensemble<Pt>, Base>{n_replicas, n_max}, slots_per_replica{slots_per_replica},
          links{n_replicas * slots_per_replica > 0 ? n_replicas * slots_per_replica : 1, strength}
    {
        static_assert(sizeof(Link) == 2 * sizeof(int), "h_link is handed out as pairs of ints");
        cells.whole_steps = -1;
        cells.whole_step_lanes = 1;
        *links.h_n = n_slots();
        links.set_d_n(n_slots());
    }
    long take_steps(float dt, int n_steps) override
    {
        const long launches_before = cells.whole_step_launches;
        if (links_path == 0) {
            cells.template take_steps<pw_int, pw_friction>(dt, n_steps, ya::ens::Replica_links{links, slots_per_replica});
        } else {  // the way before the ordered forces: atomics, a memset per step, six launches
            Links* l = &links;
            Generic_forces<Pt> gen = [l](const int, const Pt* __restrict__ d_X, Pt* d_dX) {
                link_forces<Pt>(*l, d_X, d_dX);
            };
            cells.template take_steps<pw_int, pw_friction>(dt, n_steps, gen);
        }
        return cells.whole_step_launches - launches_before;
    }
    void copy_to_device() override
    {
        cells.copy_to_device();
        links.copy_to_device();
    }
    int whole_step_lanes_used() override { return cells.whole_step_lanes_used; }
    void set_links_path(int path) override { links_path = path; }
    int* h_link() override { return reinterpret_cast<int*>(links.h_link); }
    int* h_n_links() override { return links.h_n; }
    int n_slots() override { return cells.n_replicas * slots_per_replica; }
};

template<typename Pt>
long lds_bytes_of(int n_max, int slots, int lanes)
{
    return (long)ya::ens::lds_layout<Pt, false, true>(n_max, slots, lanes).bytes;
}

// (name, point type, pairwise force, friction)
#define YA_LINKED_MODELS(X)                                                          \
    X("links", float3, models::no_pw_int<float3>, friction_w_neighbour<float3>)      \
    X("links4", float4, models::no_pw_int<float4>, friction_w_neighbour<float4>)     \
    X("springs_links", float3, models::spring, friction_w_neighbour<float3>)         \
    X("relu_links", float3, relu_force<float3>, friction_w_neighbour<float3>)        \
    X("relu_po_links", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>)

#define YA_LINKED_ROW(name, Pt, pw_int, pw_friction) YA_ENSEMBLE_MODEL(name, Pt, pw_int, pw_friction, void),
static const Model<Base* (*)(int, int, int, float)> model_table[] = {YA_LINKED_MODELS(YA_LINKED_ROW)};
#undef YA_LINKED_ROW
static const int n_models = sizeof(model_table) / sizeof(model_table[0]);
// the LDS rule of each model's point type, in the table's order
#define YA_LINKED_ROW(name, Pt, pw_int, pw_friction) &lds_bytes_of<Pt>,
static long (*const lds_table[])(int, int, int) = {YA_LINKED_MODELS(YA_LINKED_ROW)};
#undef YA_LINKED_ROW

}  // namespace lens_harness

struct ya_lens {
    std::unique_ptr<lens_harness::Base> p;
};

extern "C" {

int ya_lens_models_count(void) { return lens_harness::n_models; }
const char* ya_lens_models_name(int i)
{
    return ens_harness::name_at(lens_harness::model_table, lens_harness::n_models, i);
}

int ya_lens_create(const char* model, int n_replicas, int n_max, int slots_per_replica, float strength, ya_lens** out)
{
    if (!model || !out || n_replicas <= 0 || n_max <= 0 || slots_per_replica < 0 || !std::isfinite(strength)) return -3;
    // ids, slots and launch sizes are ints (include/ensemble.cuh)
    if ((size_t)n_replicas * (size_t)n_max > (size_t)0x7fffffff) return -3;
    if ((size_t)n_replicas * (size_t)((n_max + 3) / 4) > (size_t)0x7fffffff) return -3;
    if ((size_t)n_replicas * (size_t)slots_per_replica > (size_t)0x7fffffff) return -3;
    return ens_harness::create(lens_harness::model_table, lens_harness::n_models, model, out, n_replicas, n_max,
        slots_per_replica, strength);
}
void ya_lens_destroy(ya_lens* ens) { delete ens; }

int ya_lens_n_floats(ya_lens* e) { return e->p->n_floats(); }
float* ya_lens_h_X(ya_lens* e) { return e->p->h_X(); }
int ya_lens_set_h_n(ya_lens* e, int r, int n) { return ens_harness::set_h_n(*e->p, r, n); }
int ya_lens_get_h_n(ya_lens* e, int r) { return ens_harness::get_h_n(*e->p, r); }
int ya_lens_get_d_n(ya_lens* e, int r) { return ens_harness::get_d_n(*e->p, r); }
int ya_lens_copy_to_device(ya_lens* e) { return ens_harness::copy_to_device(*e->p); }
int ya_lens_copy_to_host(ya_lens* e) { return ens_harness::copy_to_host(*e->p); }
int* ya_lens_h_link(ya_lens* e) { return e->p->h_link(); }
int ya_lens_set_n_links(ya_lens* e, int n_links)
{
    if (n_links < 0 || n_links > e->p->n_slots()) return -3;
    *e->p->h_n_links() = n_links;
    return 0;
}
int ya_lens_get_n_links(ya_lens* e) { return *e->p->h_n_links(); }
int ya_lens_take_steps(ya_lens* e, float dt, int n_steps) { return (int)e->p->take_steps(dt, n_steps); }
int ya_lens_synchronize(ya_lens*) { return ens_harness::synchronize(); }
int ya_lens_set_fixed(ya_lens* e, int mode, int local_point) { return ens_harness::set_fixed(*e->p, mode, local_point); }
int ya_lens_get_old_v(ya_lens* e, float* out) { return ens_harness::get_old_v(*e->p, out); }
int ya_lens_set_old_v(ya_lens* e, const float* in) { return ens_harness::set_old_v(*e->p, in); }
int ya_lens_set_param(ya_lens* e, const char* name, double v)
{
    if (!name) return -3;
    if (std::string(name) == "links_path") {
        if (v != 0 && v != 1) return -3;
        e->p->set_links_path((int)v);
        return 0;
    }
    return ens_harness::set_tile_param(*e->p, name, v);
}
int ya_lens_whole_step_lanes_used(ya_lens* e) { return e->p->whole_step_lanes_used(); }

long ya_lens_lds_bytes(const char* model, int n_max, int slots_per_replica, int lanes)
{
    if (!model || n_max <= 0 || slots_per_replica < 0) return -3;
    if (lanes != 1 && lanes != 4 && lanes != 16 && lanes != 64) return -3;
    for (int i = 0; i < lens_harness::n_models; i++)
        if (std::string(model) == lens_harness::model_table[i].name)
            return lens_harness::lds_table[i](n_max, slots_per_replica, lanes);
    return -1;
}

}  // extern "C"
