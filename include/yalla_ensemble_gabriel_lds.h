/* yalla_ensemble_gabriel_lds.h -- C ABI of the Gabriel ensemble harness whose take_steps can step from LDS
 * (libyalla_ensemble_gabriel_lds.so).
 *
 * Ensemble<Pt, Gabriel_solver>::take_steps (include/ensemble_gabriel.cuh) runs K Heun steps of M independent
 * Gabriel_solver systems either as K times the 16 launches of take_step or, where every replica fits one workgroup's
 * LDS, as launches of one workgroup per replica that run whole steps from LDS (ya::ens::gabriel_lds_steps), cells with
 * more than 64 candidates included.  The bits are the same either way.  This library instantiates the template for
 * the model table of libyalla_ensemble_gabriel.so (the same names, the same functors: yalla_ensemble_gabriel.h lists
 * them) so that Python (yalla_amd/ensemble.py GabrielLdsEnsemble, tests/, tools/ensemble_bench.py --solver gabriel
 * --lds-steps) can drive it; libyalla_ensemble_gabriel.so and its header stay as they are.
 *
 * The functions are those of yalla_ensemble_gabriel.h under the prefix ya_gablds_, except: take_steps returns a
 * count; set_param knows two names more; ya_gablds_lds_dense_cells and ya_gablds_lds_bytes are added.
 *
 * HIP only: there is no CPU build of this header.  All functions return 0 on success unless stated otherwise, a
 * negative value for a harness error (-1 unknown model, -2 unknown parameter, -3 bad argument), or abort the process
 * on a HIP error.
 */
#ifndef YALLA_ENSEMBLE_GABRIEL_LDS_H
#define YALLA_ENSEMBLE_GABRIEL_LDS_H

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; only this C ABI is exported. */
#pragma GCC visibility push(default)

typedef struct ya_gablds ya_gablds;

int ya_gablds_models_count(void);
const char* ya_gablds_models_name(int index);

/* As ya_gabens_create: Ensemble<Pt, Gabriel_solver>{n_replicas, n_max, grid_size, cube_size, gabriel_coefficient}. */
int ya_gablds_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size,
    float gabriel_coefficient, ya_gablds** out);
void ya_gablds_destroy(ya_gablds* ens);

int ya_gablds_n_floats(ya_gablds* ens); /* floats per point */
float* ya_gablds_h_X(ya_gablds* ens);   /* host mirror, n_replicas * n_max * n_floats floats, replica-major */
int ya_gablds_set_h_n(ya_gablds* ens, int replica, int n);
int ya_gablds_get_h_n(ya_gablds* ens, int replica);
int ya_gablds_get_d_n(ya_gablds* ens, int replica); /* blocking read of the device-side count */
int ya_gablds_copy_to_device(ya_gablds* ens);       /* every row and every count */
/* Every row and every count; ABORTS, naming the replica, if a replica's cell left its grid (ya_gablds_status
 * with clear = 1 beforehand forgives it). */
int ya_gablds_copy_to_host(ya_gablds* ens);

/* take_steps<pw_int, pw_friction>(dt, n_steps[, gen_forces]): queued, not waited for.  Returns the number of
 * launches that stepped from LDS (Ensemble<Pt, Gabriel_solver>::lds_step_launches rose by it): 0 where the call ran
 * as n_steps times the 16 launches -- "lds_steps" forbids it, the model has a generic force, or n_max is beyond the
 * point type's capacity (ya_gablds_lds_bytes is 0). */
int ya_gablds_take_steps(ya_gablds* ens, float dt, int n_steps);
int ya_gablds_synchronize(ya_gablds* ens);

/* mode 0 = set_fixed(), 1 = set_fixed(local_point), 2 = set_fixed_xy(local_point); the point id is
 * local to a replica and applies to every replica (it must exist in every replica that is not empty). */
int ya_gablds_set_fixed(ya_gablds* ens, int mode, int local_point);
int ya_gablds_set_cube_size(ya_gablds* ens, float cube_size); /* of every replica, from the next step on */

/* d_old_v, n_replicas * n_max * 3 floats, replica-major. */
int ya_gablds_get_old_v(ya_gablds* ens, float* out);
int ya_gablds_set_old_v(ya_gablds* ens, const float* in);

/* The replica's sticky status bits (YA_STATUS_OUT_OF_GRID = 1), or -3; clear != 0 forgets them.  Never aborts. */
int ya_gablds_status(ya_gablds* ens, int replica, int clear);

/* The replica's grid arrays of the last build, as ya_gabens_get_grid. */
int ya_gablds_get_grid(ya_gablds* ens, int replica, int* cube_id, int* point_id, int* cube_start, int* cube_end);

/* The cells the last force stage of the 16-LAUNCH path left to its dense kernel (more than 64 candidates), over all
 * replicas: a blocking read.  Launches that step from LDS leave it as it is. */
int ya_gablds_dense_cells(ya_gablds* ens);

/* The (cell, stage) pairs that took the dense path INSIDE launches that stepped from LDS, over all replicas, since
 * the ensemble was created: a blocking read, for tests and tools to see which path ran.  -3 for no handle. */
long long ya_gablds_lds_dense_cells(ya_gablds* ens);

/* "gabriel_coefficient" (finite; of every replica, from the next step on); "lds_steps" (-1 = never step from LDS,
 * this harness's default; 1 = whenever the call is eligible; 0 = the engine's choice,
 * ya::ens::gabriel_lds_steps_pay); "lds_steps_max" (>= 1: steps per such launch, 256 by default).  Every other name
 * is unknown (-2), whatever `ens` is; a known name with no handle or a value outside those is -3. */
int ya_gablds_set_param(ya_gablds* ens, const char* name, double value);

/* ya::ens::gabriel_lds_layout<Pt>(n_max).bytes for the model's point type: the dynamic LDS of a launch that steps
 * from LDS, 0 where n_max is beyond the capacity; -1 for an unknown model, -3 for n_max < 1.  No device is touched. */
long ya_gablds_lds_bytes(const char* model, int n_max);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif
