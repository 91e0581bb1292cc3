// The model table of the two Gabriel ensemble harnesses (ensemble_gabriel.hip, ensemble_gabriel_lds.hip), written
// once: (name, point type, pairwise force, friction, generic-force policy of ensemble_harness.h).  Each harness
// expands it with its own Sim.
#pragma once

#define YA_GABRIEL_ENSEMBLE_MODELS(X)                                                                                  \
    X("relu", float3, relu_force<float3>, friction_w_neighbour<float3>, No_gen<float3>)                                \
    X("clipped", float3, models::clipped_spring, friction_w_neighbour<float3>, No_gen<float3>)                         \
    X("relu_plain", float3, models::relu_plain, friction_w_neighbour<float3>, No_gen<float3>)                          \
    X("relu_po", Po_cell, relu_force<Po_cell>, friction_w_neighbour<Po_cell>, No_gen<Po_cell>)                         \
    X("relu_cell", Cell, relu_force<Cell>, friction_w_neighbour<Cell>, No_gen<Cell>)                                   \
    X("clipped_push", float3, models::clipped_spring, friction_w_neighbour<float3>, Push_gen<float3>)                  \
    /* user-written frictions (model_functors.h; tests/test_friction_functors_gpu.py): ids through local ids */       \
    /* (ensemble_harness.h), declared and `_plain`, and field on the wide point */                                     \
    X("friction_ids", float3, relu_force<float3>, ens_harness::friction_by_local_id<models::ids_friction>,             \
        ens_harness::Local_friction_ids)                                                                               \
    X("friction_ids_plain", float3, relu_force<float3>, ens_harness::friction_by_local_id<models::ids_friction_plain>, \
        ens_harness::Local_friction_ids)                                                                               \
    X("friction_field", Po_cell, relu_force<Po_cell>, models::field_friction, No_gen<Po_cell>)
