"""What a pass of ya::grid_force_bits may know about its hits before phase 2 (include/solvers.cuh, ya::bits::drain:
DISTINCT = no hit is the lane's own cell, NEAR = every hit has dist < 1) changes no bit: the device against the
oracle, bit for bit, with Grid_computer::pass_facts 1 (the default) and 0 (the generic bodies only), force_variant 2 so
that small systems reach the kernel.  The cases sit where a wrong fact would show:

  tiny grids      1^3: every row of every plane is the cell's own cube (row offsets -2 .. 2 of a one-cube grid), the
                  guard must fall back in the planes below and above too (a wrong `i != j` turns spring's self pair
                  into 0 / 0); 2^3, 3^3, 4^3: rows that leave the grid or wrap, never onto the own cube;
  cube size > 1   hits at distances in [1, cube_size): friction_w_neighbour gives 0 and clipped_spring no force there,
                  a wrong `dist < 1` would give 1 and a force; cube sizes 1 and 0.75 are the launches that use NEAR;
  the unit cut    pairs at squared distances pred(t), t, succ(t), t = cutoff_squared(1) = 1;
  other functors  relu_force on Po_cell and Cell (the own plane's sums in LDS), a user friction with a self term
                  (graded_friction), a friction that is not declared stateless (ids_friction_plain);
  other paths     both summation orders, half-tile tails, old_v from LDS / 32-bit offsets / 64-bit addresses, and a dense
                  system whose rows take one pass per stretch (the generic instantiation).

The tests without the `gpu` mark hold the cases to those shapes on the host, and the oracle to finite results."""
import grid_edge_cases as ge
import numpy as np
import pytest

from yalla_amd.solution import Solution

gpu = pytest.mark.gpu
f32 = np.float32
TINY = ("gs1", "gs2", "gs3", "gs4")
SIZES_ABOVE_1 = (1.25, 2.0)
SIZES_NEAR = (1.0, 0.75)
OLD_V_FORMS = {"lds": {"stage_v_max": 1 << 30}, "offsets32": {"stage_v_max": 0},
               "addresses64": {"stage_v_max": 0, "gather_offset_bits": 64}}
ALL_HALVES = 1 << 20


def setup_for(facts, params):
    def setup(s):
        assert s.set_param("force_variant", 2) == 0
        assert s.set_param("pass_facts", facts) == 0
        for name, value in params.items():
            assert s.set_param(name, value) == 0
    return setup


def both_settings(oracle, device, model, case, order=0, **params):
    want = ge.expected(oracle, model, case, order)
    for facts in (1, 0):
        Xd, vd, gd = ge.run(device, model, case, order, setup=setup_for(facts, params))
        what = (model, case.name, case.cs, order, params, "pass_facts", facts)
        assert ge.same_grid(gd, want[2], case.n), (what, "grid arrays")
        assert np.isfinite(Xd).all(), what
        assert ge.same_bits(Xd, want[0]), (what, "positions not bit-identical")
        assert ge.same_bits(vd, want[1]), (what, "old_v not bit-identical")


# ---- the cases' shapes, on the host ----------------------------------------------------------------------------------
def own_slot_in_side_rows(case):
    """How many cells have their own sorted slot in a row of the planes dz = -1, +1, by YA_ROW_BOUNDS' clamps."""
    gs, n_cubes = case.gs, case.gs ** 3
    cube = np.sort(ge.cube_of(case.X, case.cs, gs), kind="stable")
    offs = np.searchsorted(cube, np.arange(n_cubes + 1))
    at = lambda c: int(offs[min(max(c, 0), n_cubes)])  # noqa: E731
    found = 0
    for s, c in enumerate(cube):
        rows = [dz * gs * gs + dy * gs for dz in (-1, 1) for dy in (0, -1, 1)]
        found += any(at(c + off - 1) <= s < at(c + off + 2) for off in rows)
    return found


def test_side_rows_hold_the_own_cube_only_in_a_grid_of_one_cube():
    """(From two cubes an axis on, a row of another plane is at least gs cubes away and spans three.)"""
    counts = {name: own_slot_in_side_rows(ge.rim_case(name)) for name in TINY}
    assert counts["gs1"] == ge.rim_case("gs1").n
    assert counts["gs2"] == 0 and counts["gs3"] == 0 and counts["gs4"] == 0
    for name in TINY:
        case = ge.rim_case(name)
        assert len(np.unique(ge.cube_of(case.X, case.cs, case.gs))) == case.gs ** 3    # cells in every cube


def distances(case):
    d2, _ = ge.d2_of(case.X[:, None, :], case.X[None, :, :])
    return ge.sqrt32(d2[np.triu_indices(case.n, 1)])


@pytest.mark.parametrize("cs", SIZES_ABOVE_1)
def test_hits_between_1_and_the_cube_size(cs):
    case = ge.cut_off_case(cs)
    dist = distances(case)
    assert ((dist >= 1) & (dist < f32(cs))).sum() > 200 and (dist < 1).sum() > 200
    planted = {target for _, _, target, _ in case.pairs}
    assert {"pred_1", "1", "succ_1", "pred_t", "t", "succ_t"} <= planted


@pytest.mark.parametrize("cs", SIZES_NEAR)
def test_every_hit_is_near_at_cube_sizes_up_to_1(cs):
    """The statement NEAR rests on, for the case's own pairs: d2 < cutoff_squared(cs) implies sqrtf(d2) < 1."""
    case = ge.cut_off_case(cs)
    t = ge.cutoff_squared(cs)
    assert t <= ge.cutoff_squared(1.0) == f32(1)
    d2, _ = ge.d2_of(case.X[:, None, :], case.X[None, :, :])
    assert (ge.sqrt32(d2[d2 < t]) < 1).all()
    by_target = {target: (i, j) for i, j, target, _ in case.pairs}
    for target, hit in (("pred_t", True), ("t", False), ("succ_t", False)):
        i, j = by_target[target]
        assert (ge.d2_of(case.X[i], case.X[j])[0] < t) == hit


@pytest.mark.parametrize("name", TINY)
def test_oracle_keeps_tiny_grids_finite(oracle, name):
    X, v, _ = ge.expected(oracle, "springs_grid", ge.rim_case(name))
    assert np.isfinite(X).all() and np.isfinite(v).all()


# ---- the device against the oracle -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("model", ["springs_grid", "clipped_grid", "relu_po_grid"])
@pytest.mark.parametrize("name", TINY)
def test_tiny_grids(oracle, device, name, model):
    for order in (0, 1):
        both_settings(oracle, device, model, ge.rim_case(name), order)


@gpu
@pytest.mark.parametrize("model", ["springs_grid", "clipped_grid"])
@pytest.mark.parametrize("cs", SIZES_ABOVE_1 + SIZES_NEAR)
def test_cube_sizes_either_side_of_1(oracle, device, cs, model):
    """Above 1 NEAR must be off (friction 0 and, for clipped_spring, no force between 1 and the cube size); at 1 and
    0.75 it is on, with pairs planted one ulp either side of the cut-off (at cube size 1: of the unit cut itself)."""
    case = ge.cut_off_case(cs)
    for order in (0, 1):
        both_settings(oracle, device, model, case, order)


@gpu
@pytest.mark.parametrize("case", ["cut_off", "gs2", "gs8_filled"])
@pytest.mark.parametrize("model", ["relu_po_grid", "relu_cell_grid", "friction_graded_fading_grid",
                                   "friction_ids_plain_grid", "friction_ids_grid"])
def test_other_functors_and_point_types(oracle, device, model, case):
    case = ge.cut_off_case(1.0) if case == "cut_off" else ge.rim_case(case)
    for order in (0, 1):
        both_settings(oracle, device, model, case, order)


@gpu
@pytest.mark.parametrize("form", list(OLD_V_FORMS))
@pytest.mark.parametrize("case", ["cut_off", "gs2", "gs8_filled"])
def test_old_v_from_lds_offsets_and_addresses(oracle, device, case, form):
    case = ge.cut_off_case(1.0) if case == "cut_off" else ge.rim_case(case)
    for order in (0, 1):
        both_settings(oracle, device, "springs_grid", case, order, **OLD_V_FORMS[form])


@gpu
@pytest.mark.parametrize("tail", [2, ALL_HALVES])
@pytest.mark.parametrize("case", ["cut_off", "gs1", "gs2", "gs8_filled"])
def test_half_tile_tails(oracle, device, case, tail):
    """By plane with the last two tiles, or every tile, as two half-tile workgroups: half 0 walks the own plane (the
    self pair), half 1 the planes below and above (DISTINCT, except in the 1^3 grid)."""
    case = ge.cut_off_case(1.0) if case == "cut_off" else ge.rim_case(case)
    for stage_v_max in (0, 1 << 30):
        both_settings(oracle, device, "springs_grid", case, 1, tail_tiles=tail, stage_v_max=stage_v_max)


@gpu
@pytest.mark.parametrize("model", ["springs_grid", "relu_po_grid"])
def test_dense_rows_take_the_generic_pass(oracle, device, model):
    """3000 cells at spacing 0.08: hundreds per cube, every row beyond one pass (one pass per stretch, generic), the
    planes staged in chunks; cells at the rim of the ball have rows that fit, side by side with those that do not."""
    n, out = 3000, {}
    for lib, settings in ((oracle, (None,)), (device, (1, 0))):
        for facts in settings:
            for order in (0, 1):
                with Solution(model, n, 8, 1.0, lib=lib) as s:
                    if lib is oracle:
                        assert s.set_reduce_order(1) == 0
                    else:
                        setup_for(facts, {})(s)
                    if order:
                        assert s.set_param("sum_order", order) == 0
                    s.random_sphere(0.08, 7)
                    s.take_step(0.0005, 2)
                    out[facts, order] = (s.positions(), s.old_v()[:n].copy())
    for facts in (1, 0):
        for order in (0, 1):
            for got, want in zip(out[facts, order], out[None, order]):
                assert np.isfinite(got).all()
                assert ge.same_bits(got, want), (model, "pass_facts", facts, "sum_order", order)
