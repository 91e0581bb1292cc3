/* yalla_ensemble_grid_links.h -- C ABI of the linked grid ensemble harness (libyalla_ensemble_grid_links.so).
 *
 * Ensemble<Pt, Grid_solver> (include/ensemble_grid.cuh) stepped with a Links object over the ensemble's flat id space
 * as its generic force: take_steps(dt, K, ya::ens::Replica_links{links, S}) (include/ensemble_links.cuh).  Slot s of
 * the links belongs to replica s / S; a slot is inert if a == b, unused from the used-slot count on, and SKIPPED if
 * either end lies outside the rows [r * n_max, r * n_max + n_r) of its own replica; a cell's terms are added in
 * ascending slot order.  The models: "links" (float3, no pairwise force: the functors of links_grid in
 * libyalla_models.so), "links4" (float4), "springs_links" (float3, models::spring: springs_links_grid), "relu_links"
 * (float3, relu_force, declared stateless), "relu_po_links" (Po_cell, relu_force) and "relu_cell8_links" (a point of
 * 8 floats, relu_force: at n_max = 1024 its rows leave no room for an incidence list, so it never steps from LDS there).
 *
 * The functions of include/yalla_ensemble_grid.h under the prefix ya_glens_, with the same meanings and codes, and
 * what the links add (as include/yalla_ensemble_links.h).  HIP only.  0 on success, -1 unknown model, -2 unknown
 * parameter, -3 bad argument.
 */
#ifndef YALLA_ENSEMBLE_GRID_LINKS_H
#define YALLA_ENSEMBLE_GRID_LINKS_H

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; only this C ABI is exported. */
#pragma GCC visibility push(default)

typedef struct ya_glens ya_glens;

int ya_glens_models_count(void);
const char* ya_glens_models_name(int index);

/* Ensemble<Pt, Grid_solver>{n_replicas, n_max, grid_size, cube_size} and Links{n_replicas * slots_per_replica,
 * strength} for the named model.  Sizes as ya_gens_create; slots_per_replica >= 0, strength finite.  Every slot starts
 * as the inert link (0, 0) and the used-slot count as n_replicas * slots_per_replica. */
int ya_glens_create(const char* model, int n_replicas, int n_max, int grid_size, float cube_size, int slots_per_replica,
    float strength, ya_glens** out);
void ya_glens_destroy(ya_glens* ens);

int ya_glens_n_floats(ya_glens* ens);
float* ya_glens_h_X(ya_glens* ens);
int ya_glens_set_h_n(ya_glens* ens, int replica, int n);
int ya_glens_get_h_n(ya_glens* ens, int replica);
int ya_glens_get_d_n(ya_glens* ens, int replica);
int ya_glens_copy_to_device(ya_glens* ens); /* every row, every count, every link slot and the used-slot count */
int ya_glens_copy_to_host(ya_glens* ens);   /* rows and counts; aborts as ya_gens_copy_to_host does */

/* Host mirror of the links, [n_replicas * slots_per_replica][2] ints (a, b) of ensemble-global ids. */
int* ya_glens_h_link(ya_glens* ens);
/* The host-side used-slot count (Links::h_n), 0 .. n_replicas * slots_per_replica; copy_to_device hands it over. */
int ya_glens_set_n_links(ya_glens* ens, int n_links);
int ya_glens_get_n_links(ya_glens* ens);

/* As ya_gens_take_steps: returns the number of launches that stepped from LDS (ya::ens::grid_lds_steps_linked): 0
 * unless "lds_steps" allows them, "links_path" is 0, n_max <= 1024 and ya_glens_lds_bytes > 0, else
 * ceil(n_steps / "lds_steps_max"). */
int ya_glens_take_steps(ya_glens* ens, float dt, int n_steps);
int ya_glens_synchronize(ya_glens* ens);
int ya_glens_set_fixed(ya_glens* ens, int mode, int local_point);
int ya_glens_set_cube_size(ya_glens* ens, float cube_size);
int ya_glens_get_old_v(ya_glens* ens, float* out);
int ya_glens_set_old_v(ya_glens* ens, const float* in);
int ya_glens_status(ya_glens* ens, int replica, int clear);
int ya_glens_get_grid(ya_glens* ens, int replica, int* cube_id, int* point_id, int* cube_start, int* cube_end);

/* "sum_order", "lds_steps" (this harness's default: -1), "lds_steps_max", "lds_step_lanes" (this harness's default:
 * 1; the term buffer lies behind the incidence list: ya::ens::lds_layout<Pt, true, true>(n_max, slots_per_replica,
 * lanes).bytes, and where that is 0 -- a list that leaves no room for 16 candidates' terms -- the launch runs with one lane,
 * still from LDS), "lds_step_lanes_used" (the getter: value 0, returns the lanes of the last launch from LDS, 0 before
 * any, 1 after the fallback): as ya_gens_set_param.  "links_path": 0
 * (default) = the ordered link forces, inside launches that step from LDS where allowed and eligible, else as the
 * 14-launch step with ya::ens::link_forces_ordered; 1 = link_forces<Pt> (include/links.cuh: global atomics, no fixed
 * order, no skipping rule) as a Generic_forces lambda, never from LDS.  Path 0 gives the same bits whatever else is
 * set.  Any other value of a known name, and a known name on a NULL handle, is -3; an unknown name -2. */
int ya_glens_set_param(ya_glens* ens, const char* name, double value);

/* ya::ens::lds_layout<Pt, true, true>(n_max, slots_per_replica, 1).bytes for the model's point type: the dynamic LDS of a
 * linked launch that steps from LDS (the step's arrays, the keys, the incidence list), 0 = no room.  Host arithmetic only:
 * callable without a GPU.  -1 unknown model, -3 bad argument (n_max <= 0, slots_per_replica < 0). */
long ya_glens_lds_bytes(const char* model, int n_max, int slots_per_replica);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif
