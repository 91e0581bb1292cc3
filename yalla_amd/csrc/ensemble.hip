// libyalla_ensemble.so -- the ensemble harness (include/yalla_ensemble.h): Ensemble<Pt, Tile_solver>
// (include/ensemble.cuh) instantiated for the functor / friction pairs of the `*_tile` models of the same
// names in libyalla_models.so (model_functors.h is included read-only for the functors and their
// YA_STATELESS declarations).  Links against libyalla_hip.so.
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

#include "yalla_ensemble.h"
#include "ensemble_harness.h"  // No_gen, Push_gen, Tile_replicas(_of), Model, the entry points' bodies
#ifdef YA_MODELS_WIDTHS
#include "ensemble_widths_models.h"  // libyalla_ensemble_widths.so: another table (tests only)
#endif

namespace ens_harness {

// What the all-pairs form adds to the shared interface.
struct Base : public Tile_replicas {
    virtual int whole_step_lanes_used() = 0;
};

// models::oscillator tells its two roles apart by `i == 0`, a LOCAL id.  An ensemble's functors get global ids
// (i = r * n_max + local), so the ensemble's model hands the functor the local ones: the same statements, hence
// the bits of oscillator_tile in every replica.  n_max travels in a device variable, set when it changes.
__device__ int oscillator_rows_per_replica = 1;
__device__ inline float4 oscillator_by_local_id(float4 Xi, float4 r, float dist, int i, int j)
{
    return models::oscillator(Xi, r, dist, i % oscillator_rows_per_replica, j % oscillator_rows_per_replica);
}
struct Oscillator_ids : public No_gen<float4> {
    static void before_steps(int n_max)
    {
        static int rows_set = 1;
        if (rows_set == n_max) return;
        YA_CHECK((int)hipMemcpyToSymbol(HIP_SYMBOL(oscillator_rows_per_replica), &n_max, sizeof(int)));
        rows_set = n_max;
    }
};
template<typename Pt, Pairwise_interaction<Pt> pw_int, Pairwise_friction<Pt> pw_friction, typename Policy>
struct Sim : public Tile_replicas_of<Ensemble<Pt>, Base> {
    using Tile_replicas_of<Ensemble<Pt>, Base>::cells;
    // The harness's own default is the six-launch step (whole_steps = -1): what its callers ran before the
    // whole-step launches existed; set_param("whole_steps", 0 | 1) opts in.  Likewise one lane per cell inside a
    // whole-step launch (whole_step_lanes = 1): the kernel its callers ran before there was a choice;
    // set_param("whole_step_lanes", 0 | 4 | 16 | 64) changes it.
    Sim(int n_replicas, int n_max) : Tile_replicas_of<Ensemble<Pt>, Base>{n_replicas, n_max}
    {
        cells.whole_steps = -1;
        cells.whole_step_lanes = 1;
    }
    long take_steps(float dt, int n_steps) override
    {
        const long launches_before = cells.whole_step_launches;
        Policy::before_steps(cells.n_max);
        Generic_forces<Pt> gen = Policy::gen(cells.n_replicas, cells.n_max);
        cells.template take_steps<pw_int, pw_friction>(dt, n_steps, gen);  // (push's generic force: never whole steps)
        return cells.whole_step_launches - launches_before;
    }
    int whole_step_lanes_used() override { return cells.whole_step_lanes_used; }
};

#ifdef YA_MODELS_WIDTHS
#define YA_WIDTHS_ROW_HERE(name, Pt, pw_int, pw_friction, Policy) YA_ENSEMBLE_MODEL(name, Pt, pw_int, pw_friction, Policy),
static const Model<Base* (*)(int, int)> model_table[] = {YA_WIDTHS_ENSEMBLE_MODELS(YA_WIDTHS_ROW_HERE)};
#undef YA_WIDTHS_ROW_HERE
#else
static const Model<Base* (*)(int, int)> model_table[] = {
    YA_ENSEMBLE_MODEL("springs", float3, models::spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_ENSEMBLE_MODEL("clipped", float3, models::clipped_spring, friction_w_neighbour<float3>, No_gen<float3>),
    YA_ENSEMBLE_MODEL("fading", float3, models::fading_spring, friction_on_background<float3>, No_gen<float3>),
    YA_ENSEMBLE_MODEL("relu", float3, relu_force<float3>, friction_w_neighbour<float3>, No_gen<float3>),
    YA_ENSEMBLE_MODEL("relu_po", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, No_gen<Po_cell>),
    YA_ENSEMBLE_MODEL("oscillator", float4, oscillator_by_local_id, friction_w_neighbour<float4>, Oscillator_ids),
    YA_ENSEMBLE_MODEL("push", float3, models::no_pw_int<float3>, friction_w_neighbour<float3>, Push_gen<float3>),
    // user-written frictions (model_functors.h; tests/test_friction_functors_gpu.py): ids through local ids
    // (ensemble_harness.h), declared and `_plain`, and field on the wide point
    YA_ENSEMBLE_MODEL("friction_ids", float3, relu_force<float3>, ens_harness::friction_by_local_id<models::ids_friction>, ens_harness::Local_friction_ids),
    YA_ENSEMBLE_MODEL("friction_ids_plain", float3, relu_force<float3>, ens_harness::friction_by_local_id<models::ids_friction_plain>, ens_harness::Local_friction_ids),
    YA_ENSEMBLE_MODEL("friction_field", Po_cell, relu_force<Po_cell>, models::field_friction, No_gen<Po_cell>),
};
#endif
static const int n_models = sizeof(model_table) / sizeof(model_table[0]);

}  // namespace ens_harness

struct ya_ens {
    std::unique_ptr<ens_harness::Base> p;
};

extern "C" {

int ya_ens_models_count(void) { return ens_harness::n_models; }
const char* ya_ens_models_name(int i)
{
    return ens_harness::name_at(ens_harness::model_table, ens_harness::n_models, i);
}

int ya_ens_create(const char* model, int n_replicas, int n_max, ya_ens** out)
{
    if (!model || !out || n_replicas <= 0 || n_max <= 0) return -3;
    // ids and launch sizes are ints (include/ensemble.cuh)
    if ((size_t)n_replicas * (size_t)n_max > (size_t)0x7fffffff) return -3;
    if ((size_t)n_replicas * (size_t)((n_max + 3) / 4) > (size_t)0x7fffffff) return -3;
    return ens_harness::create(ens_harness::model_table, ens_harness::n_models, model, out, n_replicas, n_max);
}
void ya_ens_destroy(ya_ens* ens) { delete ens; }

int ya_ens_n_floats(ya_ens* e) { return e->p->n_floats(); }
float* ya_ens_h_X(ya_ens* e) { return e->p->h_X(); }
int ya_ens_set_h_n(ya_ens* e, int r, int n) { return ens_harness::set_h_n(*e->p, r, n); }
int ya_ens_get_h_n(ya_ens* e, int r) { return ens_harness::get_h_n(*e->p, r); }
int ya_ens_get_d_n(ya_ens* e, int r) { return ens_harness::get_d_n(*e->p, r); }
int ya_ens_copy_to_device(ya_ens* e) { return ens_harness::copy_to_device(*e->p); }
int ya_ens_copy_to_host(ya_ens* e) { return ens_harness::copy_to_host(*e->p); }
// (at most n_steps launches; 0 with the harness's default of whole_steps = -1)
int ya_ens_take_steps(ya_ens* e, float dt, int n_steps) { return (int)e->p->take_steps(dt, n_steps); }
int ya_ens_synchronize(ya_ens*) { return ens_harness::synchronize(); }
int ya_ens_set_fixed(ya_ens* e, int mode, int local_point) { return ens_harness::set_fixed(*e->p, mode, local_point); }
int ya_ens_get_old_v(ya_ens* e, float* out) { return ens_harness::get_old_v(*e->p, out); }
int ya_ens_set_old_v(ya_ens* e, const float* in) { return ens_harness::set_old_v(*e->p, in); }
// "whole_step_lanes_used" is THE GETTER (as the grid harness's "lds_step_lanes_used": the exported functions are held
// to an exact list): it sets nothing and returns the lanes per cell of the last whole-step launch, 0 before any, 1
// where the term buffer of several lanes did not fit; the value handed over must be 0.
int ya_ens_set_param(ya_ens* e, const char* name, double v)
{
    if (name && std::string(name) == "whole_step_lanes_used") return e && v == 0 ? e->p->whole_step_lanes_used() : -3;
    return ens_harness::set_tile_param(*e->p, name, v);
}

}  // extern "C"
