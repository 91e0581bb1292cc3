/* yalla_ensemble_sweep.h -- C ABI of the sweep harness (libyalla_ensemble_sweep.so).
 *
 * The three forms of Ensemble behind one handle type, chosen at create: "tile" (Ensemble<Pt, Tile_solver>,
 * include/ensemble.cuh), "grid" (Ensemble<Pt, Grid_solver>, include/ensemble_grid.cuh) and "gabriel"
 * (Ensemble<Pt, Gabriel_solver>, include/ensemble_gabriel.cuh), stepped with A TIME STEP PER REPLICA
 * (ya::ens::Replica_dt) and, the Gabriel form, A COEFFICIENT PER REPLICA (d_gabriel_coefficients) where the handle holds
 * such arrays, with the scalars otherwise.  Each replica holds, bit for bit, what a lone Solution of its rows holds
 * when stepped with that replica's values.
 *
 * The models, per form: "tile": "relu" (float3, declared stateless), "springs" (float3, not declared), "relu_po"
 * (Po_cell), "links" (float3, no pairwise force, ordered link forces: links_tile of libyalla_models.so); "grid":
 * "relu", "springs", "relu_po", "springs_links" (float3, models::spring and ordered link forces: springs_links_grid);
 * "gabriel": "relu", "relu_plain" (not declared stateless), "relu_po".
 *
 * HIP only.  0 on success, -1 unknown model, -2 unknown parameter, -3 bad argument, -4 unknown form.
 */
#ifndef YALLA_ENSEMBLE_SWEEP_H
#define YALLA_ENSEMBLE_SWEEP_H

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; only this C ABI is exported. */
#pragma GCC visibility push(default)

typedef struct ya_swp ya_swp;

/* The form's model table; -4 / NULL for an unknown form, NULL for an index outside the table. */
int ya_swp_models_count(const char* form);
const char* ya_swp_models_name(const char* form, int index);

/* The form's Ensemble for the named model.  slots_per_replica: the link slots of each replica (0 = unlinked; > 0
 * only for a model with links; the links' strength is 0.2, every slot starts as the inert link (0, 0) and the
 * used-slot count as n_replicas * slots_per_replica).  grid_size, cube_size: of the grid and Gabriel forms (sizes as
 * ya_gens_create); gabriel_coefficient: of the Gabriel form, finite.  The all-pairs form ignores the three.  Every
 * argument is checked before the device is touched. */
int ya_swp_create(const char* form, const char* model, int n_replicas, int n_max, int slots_per_replica, int grid_size,
    float cube_size, float gabriel_coefficient, ya_swp** out);
void ya_swp_destroy(ya_swp* ens);

/* As the functions of include/yalla_ensemble.h, yalla_ensemble_grid.h and yalla_ensemble_links.h of these names. */
int ya_swp_n_floats(ya_swp* ens);
float* ya_swp_h_X(ya_swp* ens);
int ya_swp_set_h_n(ya_swp* ens, int replica, int n);
int ya_swp_get_h_n(ya_swp* ens, int replica);
int ya_swp_get_d_n(ya_swp* ens, int replica);
int ya_swp_copy_to_device(ya_swp* ens); /* rows and counts; a linked model's slots and used-slot count too */
int ya_swp_copy_to_host(ya_swp* ens);
int* ya_swp_h_link(ya_swp* ens); /* [n_replicas * slots_per_replica][2] ensemble-global ids; NULL without links */
int ya_swp_set_n_links(ya_swp* ens, int n_links);
int ya_swp_get_n_links(ya_swp* ens);
int ya_swp_synchronize(ya_swp* ens);
int ya_swp_set_fixed(ya_swp* ens, int mode, int local_point);
int ya_swp_get_old_v(ya_swp* ens, float* out);
int ya_swp_set_old_v(ya_swp* ens, const float* in);
int ya_swp_status(ya_swp* ens, int replica, int clear);                                                       /* -3: "tile" */
int ya_swp_get_grid(ya_swp* ens, int replica, int* cube_id, int* point_id, int* cube_start, int* cube_end); /* -3: "tile" */

/* h_dt: n_replicas floats, uploaded into a device array the handle owns; from then on ya_swp_take_steps steps replica r
 * with [r] as the device holds it at that time.  NULL: back to the scalar of ya_swp_take_steps. */
int ya_swp_set_dt(ya_swp* ens, const float* h_dt);
/* The same for the Gabriel form's coefficient (-3 on the other forms); NULL: back to "gabriel_coefficient". */
int ya_swp_set_gabriel_coefficients(ya_swp* ens, const float* h_coefficients);
/* Multiplies the device array of ya_swp_set_dt by `factor` in place, by a kernel that is queued and not waited for: what
 * a model's own adaptive-dt kernel would do.  -3 while no array is set. */
int ya_swp_scale_dt(ya_swp* ens, float factor);

/* n_steps Heun steps of every replica: with the array of ya_swp_set_dt if one is set (dt is ignored then), with dt
 * otherwise.  Returns the number of launches that stepped from LDS (whole-step launches of the all-pairs form). */
int ya_swp_take_steps(ya_swp* ens, float dt, int n_steps);
/* The lanes per cell of the last launch that stepped from LDS: 0 before any (the Gabriel form: 1 after one). */
int ya_swp_lanes_used(ya_swp* ens);
/* The Gabriel form's counts (-3 on the other forms): the cells the last force stage of the 16-launch path left to the
 * dense kernel; the (cell, stage) pairs done on the dense path inside launches from LDS since create.  Blocking. */
int ya_swp_dense_cells(ya_swp* ens);
long long ya_swp_lds_dense_cells(ya_swp* ens);

/* The names of the other harnesses, with their values: "whole_steps", "whole_step_lanes" ("tile"); "lds_steps" ("grid",
 * "gabriel"), "lds_step_lanes" ("grid"); "steps_per_launch" (every form: the most steps of one launch from LDS);
 * "gabriel_coefficient" ("gabriel"); "cube_size" ("grid", "gabriel").  This harness's defaults: never from LDS (-1),
 * one lane per cell.  -2 for a name that is none of these; -3 for a bad value, a NULL handle, or a name that the
 * handle's form does not have. */
int ya_swp_set_param(ya_swp* ens, const char* name, double value);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif
