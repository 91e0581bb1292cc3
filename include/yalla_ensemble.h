/* yalla_ensemble.h -- C ABI of the ensemble harness (libyalla_ensemble.so).
 *
 * Ensemble<Pt, Tile_solver> (include/ensemble.cuh) steps M independent all-pairs systems of one
 * model in one launch sequence.  As libyalla_models.so does for Solution, this library
 * instantiates that template for a table of named models so that Python (yalla_amd/ensemble.py,
 * tests/, tools/ensemble_bench.py) can drive it without a compiler in the loop.  The models are
 * the functor / friction pairs of the `*_tile` models of the same names in libyalla_models.so:
 * "springs", "clipped", "fading", "relu" (float3), "relu_po" (Po_cell), "oscillator" (float4; its
 * functor tells two roles apart by a local id, so it is handed i % n_max, j % n_max), and
 * "push" (no pairwise force; push_tile's generic force in one call on the flat arrays: the
 * right-hand side of cell 1 of EVERY replica, global row r * n_max + 1, is set to (1, 0, 0)).
 *
 * HIP only: there is no CPU build of this header.  All functions return 0 on success (ya_ens_take_steps:
 * 0 or a count, see there), a negative
 * value for a harness error (-1 unknown model, -2 unknown parameter, -3 bad argument), or abort
 * the process on a HIP error.
 */
#ifndef YALLA_ENSEMBLE_H
#define YALLA_ENSEMBLE_H

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; only this C ABI is exported. */
#pragma GCC visibility push(default)

typedef struct ya_ens ya_ens;

int ya_ens_models_count(void);
const char* ya_ens_models_name(int index);

/* Ensemble<Pt>{n_replicas, n_max} for the named model; n_max is the capacity of EACH replica.
 * An unknown name is refused (-1) before anything touches the device. */
int ya_ens_create(const char* model, int n_replicas, int n_max, ya_ens** out);
void ya_ens_destroy(ya_ens* ens);

int ya_ens_n_floats(ya_ens* ens); /* floats per point */
float* ya_ens_h_X(ya_ens* ens);   /* host mirror, n_replicas * n_max * n_floats floats, replica-major */
int ya_ens_set_h_n(ya_ens* ens, int replica, int n);
int ya_ens_get_h_n(ya_ens* ens, int replica);
int ya_ens_get_d_n(ya_ens* ens, int replica); /* blocking read of the device-side count */
int ya_ens_copy_to_device(ya_ens* ens);       /* every row and every count */
int ya_ens_copy_to_host(ya_ens* ens);

/* take_steps<pw_int, pw_friction>(dt, n_steps[, gen_forces]): the bits of n_steps calls of take_step; queued,
 * not waited for.  With "whole_steps" at its harness default of -1 it IS that loop of take_step.
 * Returns the number of whole-step launches the call made, by which Ensemble::whole_step_launches rose (>= 0,
 * at most n_steps; always 0 with whole_steps = -1): which path ran. */
int ya_ens_take_steps(ya_ens* ens, float dt, int n_steps);
int ya_ens_synchronize(ya_ens* ens);

/* mode 0 = set_fixed(), 1 = set_fixed(local_point), 2 = set_fixed_xy(local_point); the point id is
 * local to a replica and applies to every replica (it must exist in every replica that is not empty). */
int ya_ens_set_fixed(ya_ens* ens, int mode, int local_point);

/* d_old_v, n_replicas * n_max * 3 floats, replica-major. */
int ya_ens_get_old_v(ya_ens* ens, float* out);
int ya_ens_set_old_v(ya_ens* ens, const float* in);

/* "tile_lanes": Ensemble::lanes_per_cell (0 = the engine's choice, 1, 16, 64).
 * "whole_steps": Ensemble::whole_steps -- -1 (the harness's default) = six launches per step always, 1 = whole
 * steps from LDS in one launch (ya::ens::whole_steps) whenever the call is eligible (no generic forces, so never
 * "push"; n_max within the point type's capacity, 1024 for every model here), 0 = the engine's choice.
 * "steps_per_launch": Ensemble::steps_per_launch (>= 1), the most steps one such launch runs.
 * "whole_step_lanes": Ensemble::whole_step_lanes, the lanes per cell inside such a launch -- 1 (the harness's
 * default) = one thread per cell (ya::ens::whole_steps), 4, 16 or 64 = that many (ya::ens::whole_steps_coop, whatever
 * the functor declares), 0 = the engine's choice; any other value is refused (-3).
 * Any setting gives the same bits.
 * "whole_step_lanes_used" is the getter: with value 0 it sets nothing and returns the lanes per cell of the last
 * whole-step launch (0 before any; 1 where the term buffer of several lanes did not fit the workgroup's LDS). */
int ya_ens_set_param(ya_ens* ens, const char* name, double value);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif
