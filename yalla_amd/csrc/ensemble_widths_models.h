// The model tables of libyalla_ensemble_widths.so, libyalla_ensemble_grid_widths.so and
// libyalla_ensemble_gabriel_lds_widths.so (test infrastructure, tests/test_ensemble_widths*.py): ensemble.hip,
// ensemble_grid.hip and ensemble_gabriel_lds.hip compiled a second time under -DYA_MODELS_WIDTHS, with
// models::field_coupling -- a non-zero force in EVERY field -- on the point types of widths_models.h (which
// model_functors.h has included by then: the MAKE_PT types and the YA_STATELESS lines are written there, once).
// Row fields_<type> steps what fields_<type>_tile | _grid | _gabriel of libyalla_models_widths.so steps.  The shipped
// libraries keep their own tables.  Included behind ensemble_harness.h; each .hip expands a list with its own Sim.
#pragma once

#define YA_WIDTHS_ENSEMBLE_ROW(X, name, Pt) X(name, Pt, models::field_coupling<Pt>, friction_w_neighbour<Pt>, No_gen<Pt>)
// the all-pairs and the Gabriel form: the types of the lone *_tile and *_gabriel rows
#define YA_WIDTHS_ENSEMBLE_MODELS(X)               \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_float4", float4) \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_w6", W6)     \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_w11", W11)   \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_w16", W16)
// the grid form
#define YA_WIDTHS_GRID_ENSEMBLE_MODELS(X)          \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_float4", float4) \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_w6", W6)     \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_w8", W8)     \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_w9", W9)     \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_w11", W11)   \
    YA_WIDTHS_ENSEMBLE_ROW(X, "fields_w16", W16)

// What the tests' shapes rest on (tests/test_ensemble_widths.py states the same table): the rows of a replica that
// the launches stepping from LDS hold, by point type -- all-pairs (whole_step_capacity), grid (grid_lds_capacity),
// Gabriel (gabriel_lds_capacity) -- and the first n_max at which the Gabriel launch's dense sets go 4 -> 2 -> 1.
// A change of the rule breaks the build and not a test's premise.
namespace ens_widths {
template<typename Pt>
constexpr bool capacities(const int tile, const int grid, const int gabriel)
{
    return ya::ens::whole_step_capacity<Pt>() == tile && ya::ens::grid_lds_capacity<Pt>() == grid &&
           ya::ens::gabriel_lds_capacity<Pt>() == gabriel && ya::ens::gabriel_lds_layout<Pt>(gabriel + 1).bytes == 0;
}
// (n_max <= GABRIEL_CAP lays out no set; from there up 4 sets until `two`, 2 until `one`, 1 up to the capacity)
template<typename Pt>
constexpr bool dense_sets(const int two, const int one)
{
    return ya::ens::gabriel_lds_layout<Pt>(ya::GABRIEL_CAP).dense_sets == 0 &&
           ya::ens::gabriel_lds_layout<Pt>(ya::GABRIEL_CAP + 1).dense_sets == 4 &&
           ya::ens::gabriel_lds_layout<Pt>(two - 1).dense_sets == 4 && ya::ens::gabriel_lds_layout<Pt>(two).dense_sets == 2 &&
           ya::ens::gabriel_lds_layout<Pt>(one - 1).dense_sets == 2 && ya::ens::gabriel_lds_layout<Pt>(one).dense_sets == 1 &&
           ya::ens::gabriel_lds_layout<Pt>(ya::ens::gabriel_lds_capacity<Pt>()).dense_sets == 1;
}
static_assert(sizeof(float4) == 16 && capacities<float4>(1024, 1024, 995) && dense_sets<float4>(530, 770), "float4");
static_assert(sizeof(W6) == 24 && capacities<W6>(1024, 1024, 696) && dense_sets<W6>(432, 568), "W6");
static_assert(sizeof(W8) == 32 && capacities<W8>(1024, 1024, 512) && dense_sets<W8>(343, 449), "W8");
static_assert(sizeof(W9) == 36 && capacities<W9>(970, 918, 459) && dense_sets<W9>(305, 394), "W9");
static_assert(sizeof(W11) == 44 && capacities<W11>(794, 750, 346) && dense_sets<W11>(249, 303), "W11");
static_assert(sizeof(W16) == 64 && capacities<W16>(537, 512, 176) && dense_sets<W16>(134, 160), "W16");
// W16's grid capacity: 513 rows lay out 1024 sort keys
static_assert(ya::ens::grid_lds_key_rows(512) == 512 && ya::ens::grid_lds_key_rows(513) == 1024, "the key array doubles");
}  // namespace ens_widths
