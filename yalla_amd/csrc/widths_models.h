// The model table of libyalla_models_widths.so and oracle/_build/liboracle_models_widths.so (test infrastructure,
// tests/test_point_widths*.py): models::field_coupling on points of 4, 6, 8, 9, 11 and 16 floats, the widths that
// libyalla_hip.so's per-width kernels and the solvers' per-type constants are built for beside the 3, 5 and 7 floats
// of libyalla_models.so's models.  Included at the end of model_functors.h when YA_MODELS_WIDTHS is defined;
// models_harness.inc then compiles YA_MODEL_TABLE instead of its own rows.
#pragma once

// float4 is built in: the one type whose cube-sorted entry has padding (32 bytes, the id in word 4).
MAKE_PT(W4, a);                                         // 20-byte entry, points of <= 16 bytes
MAKE_PT(W6, a, b, c);                                   // 28 bytes (the size of the reference's Po_cell4, wnt.cu)
MAKE_PT(W8, a, b, c, d, e);                             // 36 bytes: the first entry wider than 32
MAKE_PT(W9, a, b, c, d, e, f);                          // 40 bytes, 8-aligned
MAKE_PT(W11, a, b, c, d, e, f, g, h);                   // 48 bytes, 16-aligned
MAKE_PT(W16, a, b, c, d, e, f, g, h, k, l, m, n, o);    // 68 bytes: the widest point the engine takes

// Declared stateless for every type but W9 (a grid type) and W6 (the tile type; its grid and Gabriel rows follow):
// both the declared and the undeclared kernel choices are seen.
#ifdef YA_STATELESS
YA_STATELESS(float4, models::field_coupling<float4>)
YA_STATELESS(W4, models::field_coupling<W4>)
YA_STATELESS(W8, models::field_coupling<W8>)
YA_STATELESS(W11, models::field_coupling<W11>)
YA_STATELESS(W16, models::field_coupling<W16>)
static_assert(ya::stateless_pair<W16, models::field_coupling<W16>, friction_w_neighbour<W16>>() &&
                  !ya::stateless_pair<W9, models::field_coupling<W9>, friction_w_neighbour<W9>>() &&
                  !ya::stateless_pair<W6, models::field_coupling<W6>, friction_w_neighbour<W6>>(),
    "field_coupling is declared stateless but for W9 and W6");

// What the tests' shapes rest on (tests/test_point_widths.py states the same three capacities): the cells that
// grid_force_bits stages per plane, by entry size -- 352 up to 24 bytes, 256 up to 32, 176 beyond.
static_assert(sizeof(ya::Entry<float4>) == 32 && ya::bits::Stage<float4>::value == 256, "float4: padded entry, 256 cells");
static_assert(sizeof(ya::Entry<W4>) == 20 && ya::bits::Stage<W4>::value == 352, "W4: 352 staged cells");
static_assert(sizeof(ya::Entry<W6>) == 28 && ya::bits::Stage<W6>::value == 256, "W6: 256 staged cells");
static_assert(sizeof(ya::Entry<W8>) == 36 && ya::bits::Stage<W8>::value == 176, "W8: 176 staged cells");
static_assert(sizeof(ya::Entry<W9>) == 40 && ya::bits::Stage<W9>::value == 176, "W9: 176 staged cells");
static_assert(sizeof(ya::Entry<W11>) == 48 && ya::bits::Stage<W11>::value == 176, "W11: 176 staged cells");
static_assert(sizeof(ya::Entry<W16>) == 68 && ya::bits::Stage<W16>::value == 176, "W16: 176 staged cells");
#endif

#define YA_WIDTHS_ROW(name, Pt, SOLVER) \
    YA_MODEL(name, Pt, SOLVER, models::field_coupling<Pt>, friction_w_neighbour<Pt>, No_gen<Pt>)
#define YA_MODEL_TABLE                                   \
    YA_WIDTHS_ROW("fields_float4_grid", float4, true),   \
    YA_WIDTHS_ROW("fields_w4_grid", W4, true),           \
    YA_WIDTHS_ROW("fields_w6_grid", W6, true),           \
    YA_WIDTHS_ROW("fields_w8_grid", W8, true),           \
    YA_WIDTHS_ROW("fields_w9_grid", W9, true),           \
    YA_WIDTHS_ROW("fields_w11_grid", W11, true),         \
    YA_WIDTHS_ROW("fields_w16_grid", W16, true),         \
    YA_WIDTHS_ROW("fields_float4_tile", float4, false),  \
    YA_WIDTHS_ROW("fields_w6_tile", W6, false),          \
    YA_WIDTHS_ROW("fields_w11_tile", W11, false),        \
    YA_WIDTHS_ROW("fields_w16_tile", W16, false),        \
    YA_WIDTHS_ROW("fields_float4_gabriel", float4, GABRIEL), \
    YA_WIDTHS_ROW("fields_w6_gabriel", W6, GABRIEL),     \
    YA_WIDTHS_ROW("fields_w11_gabriel", W11, GABRIEL),   \
    YA_WIDTHS_ROW("fields_w16_gabriel", W16, GABRIEL)
