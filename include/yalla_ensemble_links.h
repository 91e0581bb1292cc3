/* yalla_ensemble_links.h -- C ABI of the linked ensemble harness (libyalla_ensemble_links.so).
 *
 * Ensemble<Pt, Tile_solver> (include/ensemble.cuh) stepped with a Links object over the ensemble's flat id space as
 * its generic force: take_steps(dt, K, ya::ens::Replica_links{links, S}) (include/ensemble_links.cuh).  Slot s of
 * the links belongs to replica s / S; a slot is inert if a == b, unused from the used-slot count on, and SKIPPED if
 * either end lies outside the rows [r * n_max, r * n_max + n_r) of its own replica; a cell's terms are added in
 * ascending slot order.  The models: "links" (float3, no pairwise force: the functors of links_tile in
 * libyalla_models.so), "links4" (float4, as links4_tile), "springs_links" (float3, models::spring), "relu_links"
 * (float3, relu_force, declared stateless) and "relu_po_links" (Po_cell, relu_force).
 *
 * The functions of include/yalla_ensemble.h under the prefix ya_lens_, with the same meanings and codes, and what
 * the links add.  HIP only.  0 on success, -1 unknown model, -2 unknown parameter, -3 bad argument.
 */
#ifndef YALLA_ENSEMBLE_LINKS_H
#define YALLA_ENSEMBLE_LINKS_H

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; only this C ABI is exported. */
#pragma GCC visibility push(default)

typedef struct ya_lens ya_lens;

int ya_lens_models_count(void);
const char* ya_lens_models_name(int index);

/* Ensemble<Pt>{n_replicas, n_max} and Links{n_replicas * slots_per_replica, strength} for the named model.
 * slots_per_replica >= 0, strength finite.  Every slot starts as the inert link (0, 0) and the used-slot count as
 * n_replicas * slots_per_replica. */
int ya_lens_create(const char* model, int n_replicas, int n_max, int slots_per_replica, float strength, ya_lens** out);
void ya_lens_destroy(ya_lens* ens);

int ya_lens_n_floats(ya_lens* ens);
float* ya_lens_h_X(ya_lens* ens);
int ya_lens_set_h_n(ya_lens* ens, int replica, int n);
int ya_lens_get_h_n(ya_lens* ens, int replica);
int ya_lens_get_d_n(ya_lens* ens, int replica);
int ya_lens_copy_to_device(ya_lens* ens); /* every row, every count, every link slot and the used-slot count */
int ya_lens_copy_to_host(ya_lens* ens);   /* rows and counts */

/* Host mirror of the links, [n_replicas * slots_per_replica][2] ints (a, b) of ensemble-global ids. */
int* ya_lens_h_link(ya_lens* ens);
/* The host-side used-slot count (Links::h_n), 0 .. n_replicas * slots_per_replica; copy_to_device hands it over. */
int ya_lens_set_n_links(ya_lens* ens, int n_links);
int ya_lens_get_n_links(ya_lens* ens);

/* As ya_ens_take_steps: returns the number of whole-step launches the call made. */
int ya_lens_take_steps(ya_lens* ens, float dt, int n_steps);
int ya_lens_synchronize(ya_lens* ens);
int ya_lens_set_fixed(ya_lens* ens, int mode, int local_point);
int ya_lens_get_old_v(ya_lens* ens, float* out);
int ya_lens_set_old_v(ya_lens* ens, const float* in);

/* "tile_lanes", "whole_steps" (default -1), "steps_per_launch", "whole_step_lanes" (default 1): as
 * ya_ens_set_param.  "links_path": 0 (default) = the ordered link forces, inside whole-step launches where
 * whole_steps allows them and the incidence list fits (ya_lens_lds_bytes > 0 with one lane), else as the six-launch
 * step with ya::ens::link_forces_ordered; 1 = link_forces<Pt> (include/links.cuh: global atomics, no fixed order, no
 * skipping rule) as a Generic_forces lambda, never whole steps.  Path 0 gives the same bits whatever else is set. */
int ya_lens_set_param(ya_lens* ens, const char* name, double value);
/* Ensemble::whole_step_lanes_used: the lanes per cell of the last whole-step launch (0 before any). */
int ya_lens_whole_step_lanes_used(ya_lens* ens);

/* ya::ens::lds_layout<Pt, false, true>(n_max, slots_per_replica, lanes).bytes for the model's point type: the dynamic
 * LDS of a linked whole-step launch, 0 = no room.  Host arithmetic only: callable without a GPU.  -1 unknown model,
 * -3 bad argument (n_max <= 0, slots_per_replica < 0, lanes not 1, 4, 16 or 64). */
long ya_lens_lds_bytes(const char* model, int n_max, int slots_per_replica, int lanes);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif
