/* yalla_ensemble_gabriel.h -- C ABI of the Gabriel ensemble harness (libyalla_ensemble_gabriel.so).
 *
 * Ensemble<Pt, Gabriel_solver> (include/ensemble_gabriel.cuh) steps M independent Gabriel_solver systems of one
 * model in one launch sequence.  As libyalla_ensemble_grid.so does for the grid form, this library instantiates
 * the template for a table of named models so that Python (yalla_amd/ensemble.py GabrielEnsemble, tests/,
 * tools/ensemble_bench.py --solver gabriel) can drive it without a compiler in the loop.  The models are the
 * functor / friction / generic-force triples of the `*_gabriel` models of the same names in libyalla_models.so:
 * "relu", "clipped", "relu_plain" (relu's statements, NOT declared stateless: one lane evaluates a cell's
 * functors, in order), "relu_po" (Po_cell), "relu_cell" (Cell), and "clipped_push" (clipped's pairwise force and
 * the generic force of the ensemble harnesses' push models: the right-hand side of cell 1 of EVERY replica,
 * global row r * n_max + 1, is set to (1, 0, 0) before the pairwise force is added).
 *
 * The functions are those of yalla_ensemble_grid.h under the prefix ya_gabens_, except: create takes the
 * gabriel_coefficient; ya_gabens_dense_cells is added; set_param knows "gabriel_coefficient" only.
 *
 * HIP only: there is no CPU build of this header.  All functions return 0 on success, a negative value for a
 * harness error (-1 unknown model, -2 unknown parameter, -3 bad argument), or abort the process on a HIP
 * error.
 */
#ifndef YALLA_ENSEMBLE_GABRIEL_H
#define YALLA_ENSEMBLE_GABRIEL_H

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; only this C ABI is exported. */
#pragma GCC visibility push(default)

typedef struct ya_gabens ya_gabens;

int ya_gabens_models_count(void);
const char* ya_gabens_models_name(int index);

/* Ensemble<Pt, Gabriel_solver>{n_replicas, n_max, grid_size, cube_size, gabriel_coefficient} for the named model;
 * n_max is the capacity of EACH replica, the other three hold for every replica.  An unknown name (-1) and values
 * the class refuses (-3: a size < 1, grid_size > 256, n_replicas * n_max or n_replicas * (grid_size^3 + 1) beyond
 * 2^31 - 1, cube_size not positive, a coefficient that is not finite) are refused before anything touches the
 * device. */
int ya_gabens_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size,
    float gabriel_coefficient, ya_gabens** out);
void ya_gabens_destroy(ya_gabens* ens);

int ya_gabens_n_floats(ya_gabens* ens); /* floats per point */
float* ya_gabens_h_X(ya_gabens* ens);   /* host mirror, n_replicas * n_max * n_floats floats, replica-major */
int ya_gabens_set_h_n(ya_gabens* ens, int replica, int n);
int ya_gabens_get_h_n(ya_gabens* ens, int replica);
int ya_gabens_get_d_n(ya_gabens* ens, int replica); /* blocking read of the device-side count */
int ya_gabens_copy_to_device(ya_gabens* ens);       /* every row and every count */
/* Every row and every count; ABORTS, naming the replica, if a replica's cell left its grid (ya_gabens_status
 * with clear = 1 beforehand forgives it). */
int ya_gabens_copy_to_host(ya_gabens* ens);

/* n_steps calls of take_step<pw_int, pw_friction>(dt[, gen_forces]): queued, not waited for. */
int ya_gabens_take_steps(ya_gabens* ens, float dt, int n_steps);
int ya_gabens_synchronize(ya_gabens* ens);

/* mode 0 = set_fixed(), 1 = set_fixed(local_point), 2 = set_fixed_xy(local_point); the point id is
 * local to a replica and applies to every replica (it must exist in every replica that is not empty). */
int ya_gabens_set_fixed(ya_gabens* ens, int mode, int local_point);
int ya_gabens_set_cube_size(ya_gabens* ens, float cube_size); /* of every replica, from the next step on */

/* d_old_v, n_replicas * n_max * 3 floats, replica-major. */
int ya_gabens_get_old_v(ya_gabens* ens, float* out);
int ya_gabens_set_old_v(ya_gabens* ens, const float* in);

/* The replica's sticky status bits (YA_STATUS_OUT_OF_GRID = 1: a cell left the grid and was kept inside it),
 * or -3; clear != 0 forgets them.  Never aborts. */
int ya_gabens_status(ya_gabens* ens, int replica, int clear);

/* The replica's grid arrays of the last build, in ya_sim_get_grid's conventions (any pointer may be NULL):
 * cube_id[n_max], point_id[n_max] (slots from the replica's count on are unspecified; ids are local),
 * cube_start[grid_size^3] / cube_end[grid_size^3] (first and last slot of the cube, -1 / -2 for an empty
 * one; -1 / -1 everywhere while the replica has never been built). */
int ya_gabens_get_grid(ya_gabens* ens, int replica, int* cube_id, int* point_id, int* cube_start, int* cube_end);

/* The cells the last force stage left to the dense kernel (more than 64 candidates), over all replicas: a
 * blocking read, for tests and tools to see which path ran.  The step never reads it. */
int ya_gabens_dense_cells(ya_gabens* ens);

/* "gabriel_coefficient" (finite; of every replica, from the next step on).  Every other name, the grid
 * ensemble's "lanes" and "sum_order" among them, is unknown (-2), whatever `ens` is. */
int ya_gabens_set_param(ya_gabens* ens, const char* name, double value);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif
