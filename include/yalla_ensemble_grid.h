/* yalla_ensemble_grid.h -- C ABI of the grid ensemble harness (libyalla_ensemble_grid.so).
 *
 * Ensemble<Pt, Grid_solver> (include/ensemble_grid.cuh) steps M independent Grid_solver systems of one model
 * in one launch sequence.  As libyalla_ensemble.so does for the all-pairs form, this library instantiates the
 * template for a table of named models so that Python (yalla_amd/ensemble.py GridEnsemble, tests/,
 * tools/ensemble_grid_bench.py) can drive it without a compiler in the loop.  The models are the functor /
 * friction / generic-force triples of the `*_grid` models of the same names in libyalla_models.so: "springs",
 * "clipped", "fading", "relu" (float3), "relu_po" (Po_cell), "relu_cell" (Cell), "push" (no pairwise force;
 * push_grid's generic force in one call on the flat arrays: the right-hand side of cell 1 of EVERY replica,
 * global row r * n_max + 1, is set to (1, 0, 0)) and "clipped_push" (clipped's pairwise force and push's
 * generic force).
 *
 * HIP only: there is no CPU build of this header.  All functions return 0 on success, a negative value for a
 * harness error (-1 unknown model, -2 unknown parameter, -3 bad argument), or abort the process on a HIP
 * error.
 */
#ifndef YALLA_ENSEMBLE_GRID_H
#define YALLA_ENSEMBLE_GRID_H

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; only this C ABI is exported. */
#pragma GCC visibility push(default)

typedef struct ya_gens ya_gens;

int ya_gens_models_count(void);
const char* ya_gens_models_name(int index);

/* Ensemble<Pt, Grid_solver>{n_replicas, n_max, grid_size, cube_size} for the named model; n_max is the
 * capacity of EACH replica, grid_size and cube_size hold for every replica.  An unknown name (-1) and sizes
 * the class refuses (-3: a size < 1, grid_size > 256, n_replicas * n_max or n_replicas * (grid_size^3 + 1)
 * beyond 2^31 - 1, cube_size not positive) are refused before anything touches the device. */
int ya_gens_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size, ya_gens** out);
void ya_gens_destroy(ya_gens* ens);

int ya_gens_n_floats(ya_gens* ens); /* floats per point */
float* ya_gens_h_X(ya_gens* ens);   /* host mirror, n_replicas * n_max * n_floats floats, replica-major */
int ya_gens_set_h_n(ya_gens* ens, int replica, int n);
int ya_gens_get_h_n(ya_gens* ens, int replica);
int ya_gens_get_d_n(ya_gens* ens, int replica); /* blocking read of the device-side count */
int ya_gens_copy_to_device(ya_gens* ens);       /* every row and every count */
/* Every row and every count; ABORTS, naming the replica, if a replica's cell left its grid (ya_gens_status
 * with clear = 1 beforehand forgives it). */
int ya_gens_copy_to_host(ya_gens* ens);

/* take_steps<pw_int, pw_friction>(dt, n_steps[, gen_forces]): n_steps calls of take_step, bit for bit; queued, not
 * waited for.  Returns the number of launches that stepped from LDS (Ensemble<Pt, Grid_solver>::lds_step_launches
 * rose by it): 0 unless "lds_steps" allows them and the call is eligible -- the model has no generic forces and
 * n_max <= ya::ens::grid_lds_capacity<Pt>() (1024) -- else ceil(n_steps / "lds_steps_max"). */
int ya_gens_take_steps(ya_gens* ens, float dt, int n_steps);
int ya_gens_synchronize(ya_gens* ens);

/* mode 0 = set_fixed(), 1 = set_fixed(local_point), 2 = set_fixed_xy(local_point); the point id is
 * local to a replica and applies to every replica (it must exist in every replica that is not empty). */
int ya_gens_set_fixed(ya_gens* ens, int mode, int local_point);
int ya_gens_set_cube_size(ya_gens* ens, float cube_size); /* of every replica, from the next step on */

/* d_old_v, n_replicas * n_max * 3 floats, replica-major. */
int ya_gens_get_old_v(ya_gens* ens, float* out);
int ya_gens_set_old_v(ya_gens* ens, const float* in);

/* The replica's sticky status bits (YA_STATUS_OUT_OF_GRID = 1: a cell left the grid and was kept inside it),
 * or -3; clear != 0 forgets them.  Never aborts. */
int ya_gens_status(ya_gens* ens, int replica, int clear);

/* The replica's grid arrays of the last build, in ya_sim_get_grid's conventions (any pointer may be NULL):
 * cube_id[n_max], point_id[n_max] (slots from the replica's count on are unspecified; ids are local),
 * cube_start[grid_size^3] / cube_end[grid_size^3] (first and last slot of the cube, -1 / -2 for an empty
 * one; -1 / -1 everywhere while the replica has never been built). */
int ya_gens_get_grid(ya_gens* ens, int replica, int* cube_id, int* point_id, int* cube_start, int* cube_end);

/* "lanes": lanes_per_cell (0 = the engine's choice, 1, 4, 8, 16); "sum_order": 0 = YA_SUM_REFERENCE,
 * 1 = YA_SUM_BY_PLANE.  Neither changes a result's bits against the single system with the same sum_order.
 * "lds_steps": -1 (this harness's default) = ya_gens_take_steps always runs the 14 launches per step, 1 = launches of
 * one workgroup per replica that step from LDS (ya::ens::grid_lds_steps) whenever the call is eligible, 0 = the
 * engine's choice (ya::ens::lds_steps_pay); "lds_steps_max" (>= 1, default 256): the steps of one such launch.
 * "lds_step_lanes": Ensemble<Pt, Grid_solver>::lds_step_lanes, the lanes per cell inside such a launch -- 1 (this
 * harness's default) = one thread per cell, the kernel every caller ran before the setting existed; 4, 16 or 64 =
 * that many lanes share a cell's candidates whatever the functor declares (ya::ens::grid_lds_walk_coop); 0 = the
 * engine's choice: one lane unless the model's functors are declared YA_STATELESS, else
 * ya::ens::grid_lds_lanes_for(n_max): 16 up to 32 cells, 4 up to 64, else 1 (measured).  Where the workgroup's LDS has no room
 * for the terms of 16 candidates behind the keys (ya::ens::lds_layout<Pt, true, false>(n_max, 0, lanes).bytes == 0: a 7-float
 * point at n_max = 1024 with 4 lanes, an 8-float point there with any) the launch runs with one lane, still from LDS.
 * None of them changes a bit of the positions, old_v, the grid arrays or the status.
 * "lds_step_lanes_used" is THE GETTER of Ensemble<Pt, Grid_solver>::lds_step_lanes_used: with value 0 the call sets
 * nothing and RETURNS the lanes per cell of the last launch that stepped from LDS -- 0 before any, 1 after the
 * fallback to one lane, else 4, 16 or 64 (the list of exported functions stays as it was).
 * Any other value of a known name, and a known name on a NULL handle, is -3; an unknown name -2. */
int ya_gens_set_param(ya_gens* ens, const char* name, double value);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif
