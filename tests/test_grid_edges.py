"""The cases of tests/grid_edge_cases.py hold the shapes they are for (so that a change of a generator cannot quietly
stop testing them), and the oracle takes the three decisions -- inside the cut-off, which cube, does the stencil row
exist -- as independent numpy statements of the reference do.  No GPU; tests/test_grid_edges_gpu.py holds the device against
the oracle on the same cases."""
from collections import Counter

import grid_edge_cases as ge
import numpy as np
import pytest
from test_core_abi_gpu import numpy_grid
from test_reference_statement_numpy import reference_forces

from yalla_amd.solution import Solution

f32 = np.float32


# ---- cut_off -------------------------------------------------------------------------------------------------------
def test_cutoff_squared_is_below_the_naive_square_for_two_cube_sizes():
    """What makes `d2 < cs * cs` a wrong shortcut that every other test lets pass."""
    for cs in ge.CUT_SIZES:
        t, naive = ge.cutoff_squared(cs), f32(f32(cs) * f32(cs))
        assert ge.sqrt32(t) >= f32(cs) > ge.sqrt32(ge.pred(t))
        assert (t < naive) == (cs in (0.7, 2.5)) and t <= naive


@pytest.mark.parametrize("cs", ge.CUT_SIZES)
def test_cut_off_case_has_the_pairs_it_is_for(cs):
    case = ge.cut_off_case(cs)
    X = case.X
    assert case.n <= 700 and case.n % ge.TILE != 0 and case.gs == 8
    assert len(np.unique(X, axis=0)) == case.n
    targets = ge.cut_targets(cs)
    assert {"pred_t", "t", "succ_t"} <= set(targets)
    assert ("cs_times_cs" in targets) == (cs in (0.7, 2.5)) and ("1" in targets) == (cs in (1.7, 2.5))
    cubes = ge.cube3_of(X, cs, 8)
    counts = Counter()
    for i, j, target, place in case.pairs:
        d2, tie = ge.d2_of(X[i], X[j])   # from the STORED positions
        assert not tie
        if place == "axis":
            axis = "xyz".index(target[5])
            sep = {"pred_cs": ge.pred(cs), "cs": f32(cs), "succ_cs": ge.succ(cs)}[target[7:]]
            r = X[i] - X[j]
            assert r[axis] == sep and (np.delete(r, axis) == 0).all() and d2 == f32(sep * sep)
        else:
            assert d2 == targets[target], (target, place)
            assert ge.PLACEMENTS[ge.placement_of(cubes[i][None], cubes[j][None])[0]] == place
        counts[(target, place)] += 1
    print("planted pairs per (cs, target, placement):")
    for key in sorted(counts):
        print("  ", cs, key, counts[key])
    # every (target, placement) combination, and every axis at pred(cs), cs, succ(cs)
    assert all(counts[(k, p)] >= 1 for k in targets for p in ge.PLACEMENTS)
    assert sum(1 for k in counts if k[1] == "axis") == 9
    # the background: 4 .. 8 cells in each of the central 4^3 cubes; the lone cell has nobody within the cut-off
    central = (np.abs(cubes[:-1] - 3.5) < 2).all(axis=1)
    per_cube = np.bincount(ge.cube_of(X[:-1][central], cs, 8), minlength=512).reshape(8, 8, 8)[2:6, 2:6, 2:6]
    assert per_cube.min() >= 4 and central.mean() > 0.95
    assert (ge.sqrt32(ge.d2_of(X[-1], X[:-1])[0]) > f32(2 * cs)).all()
    assert ge.max_candidates(X, cs) < 100        # (what gabriel_force_direct's list holds)


@pytest.mark.parametrize("cs", ge.CUT_SIZES)
def test_the_squared_threshold_decides_as_the_square_root_does(cs):
    """The property ya::cutoff_squared claims, on every pair of the case, the planted ones sitting on it: sqrtf(d2) <
    cs equals d2 < t.  For 0.7 and 2.5 some pair has t <= d2 < fl(cs * cs): the naive compare decides otherwise."""
    X = ge.cut_off_case(cs).X
    t = ge.cutoff_squared(cs)
    d2, _ = ge.d2_of(X[:, None, :], X[None, :, :])
    assert np.array_equal(ge.sqrt32(d2) < f32(cs), d2 < t)
    assert ((d2 == t).sum() >= 8) and ((d2 == ge.pred(t)).sum() >= 8) and ((d2 == ge.succ(t)).sum() >= 8)
    naive = f32(f32(cs) * f32(cs))
    assert ((d2 >= t) & (d2 < naive)).any() == (cs in (0.7, 2.5))
    if cs > 1:   # the functors' own cut: dist = sqrtf(d2) against 1
        for k, inside in (("pred_pred_1", True), ("pred_1", True), ("1", False), ("succ_1", False)):
            assert (ge.sqrt32(ge.cut_targets(cs)[k]) < 1) == inside


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("cs", ge.CUT_SIZES)
def test_oracle_forces_on_the_cut_off_are_the_numpy_statement(oracle, cs, sum_order):
    """A dt = 0 step with the lone cell held fixed leaves the stage's right-hand side F + sum_v / sum_friction in
    old_v (tests/test_reference_statement_numpy.py): bit for bit the statement's, whose cut is `dist >= f32(cs)`."""
    case = ge.cut_off_case(cs)
    X, got, _ = ge.run(oracle, "springs_grid", case, sum_order, dt=0.0, steps=1, fixed=case.n - 1)
    assert ge.same_bits(X, case.X)
    want = reference_forces(case.X, bool(sum_order), old_v=case.v, gs=8, cube_size=cs)
    assert (want[-1] == 0).all() and np.abs(want).max() > 0.1
    assert ge.same_bits(want, got)


# ---- faces ---------------------------------------------------------------------------------------------------------
def test_faces_cases_hold_coordinates_whose_cube_the_rounding_decides():
    sizes_with = 0
    for cs in ge.FACE_SIZES:
        case = ge.faces_case(cs)
        coords = ge.face_coordinates(cs)
        assert len(coords) == 7 * (2 * ge.ULPS + 1) + 1
        assert np.signbit(coords[coords == 0]).sum() == 1 and (coords == 0).sum() == 2    # +0 and -0
        for k in range(-3, 4):
            x = f32(f32(k) * f32(cs))
            ulps = coords.view(np.int32).astype(np.int64) - np.int64(x.view(np.int32))
            assert k == 0 or set(range(-ge.ULPS, ge.ULPS + 1)) <= set(ulps.tolist())
        X = case.X
        assert case.n <= 2100 and case.n % ge.TILE != 0
        on_face = np.isin(X, coords)
        for axis in range(3):     # every coordinate on every axis (the cells on one face, on edges and corners)
            assert set(coords.tolist()) <= set(X[on_face[:, axis], axis].tolist()), (cs, axis)
        assert (on_face.sum(axis=1) == 2).sum() >= 30 and (on_face.sum(axis=1) == 3).sum() >= 30
        decided = ge.rounding_decides(X, cs) & on_face
        print("cube size", cs, "cells whose cube the quotient's rounding decides, per axis:", decided.sum(axis=0))
        sizes_with += bool(decided.any(axis=0).all())
        assert not ge.rounding_decides(coords, 1.0).any()
        cubes = ge.cube3_of(X, cs, 8)
        assert cubes.min() >= 0 and cubes.max() <= 7
    assert sizes_with >= 2


@pytest.mark.parametrize("cs", ge.FACE_SIZES)
def test_oracle_grid_of_the_faces_case_is_numpy_grid(oracle, cs):
    case = ge.faces_case(cs)
    n = case.n
    with Solution("springs_grid", n, 8, cs, lib=oracle) as s:
        s.h_X[:n] = case.X
        s.h_n = n
        s.copy_to_device()
        got = s.build_grid(8, cs)
    want = numpy_grid(case.X, cs, 8)
    assert np.array_equal(want[0], ge.cube_of(case.X, cs, 8)[want[1]])
    for name, a, b in zip(("cube_id", "point_id", "cube_start", "cube_end"), want, got):
        assert np.array_equal(a, b[:len(a)]), name


# ---- rim -----------------------------------------------------------------------------------------------------------
def test_rim_cases_are_populated_as_described():
    for name in ge.RIM_NAMES:
        case = ge.rim_case(name)
        gs, X = case.gs, case.X
        assert case.cs == 1.0 and case.n <= 2100 and (case.n % ge.TILE != 0 or case.n < ge.TILE)
        lo, hi = -(gs // 2), gs - gs // 2
        assert X.min() >= lo + ge.RIM_MARGIN and X.max() <= hi - ge.RIM_MARGIN
        per_cube = np.bincount(ge.cube_of(X, 1.0, gs), minlength=gs ** 3)
        assert len(per_cube) == gs ** 3
        if name == "gs8_filled":
            assert 1500 <= case.n and per_cube.max() <= 9
            corners = [x + 8 * y + 64 * z for z in (0, 7) for y in (0, 7) for x in (0, 7)]
            assert 0 in corners and 511 in corners and (per_cube[corners] > 0).all()
            assert (per_cube <= 1).sum() >= 512 // 4
        elif name == "gs8_empty_ends":
            assert per_cube[:73].sum() == 0 and per_cube[440:].sum() == 0 and per_cube[73] > 0 and per_cube[439] > 0
        elif gs > 1:
            assert per_cube.min() >= 3 and per_cube.max() <= 8
        else:
            assert case.n == 30
    others = [ge.rim_case("gs8_filled", seed).n for seed in (0, 1, 2)] + [ge.rim_case("gs8_empty_ends").n]
    assert len(set(others)) == 4      # (the ensemble's replicas differ in n)


@pytest.mark.parametrize("name", ge.RIM_NAMES)
def test_rows_that_wrap_hold_candidates_and_none_of_them_hits(name):
    """A stencil row that leaves the grid at a face comes back, by its linear index, on the opposite face: those cells
    are staged and tested.  From 3 cubes per axis on none of them is within the cut-off; with 2 and 1 the same cube is
    visited more than once (the oracle's rule: an index inside [0, n_cubes) is taken as it is)."""
    case = ge.rim_case(name)
    seen, hits = ge.wrapped_candidates(case.X, 1.0, case.gs)
    if case.gs >= 3:
        assert seen > 100 and hits == 0
    h = ge.nhood(case.gs)
    assert (len(set(h)) < 27) == (case.gs <= 2)


@pytest.mark.parametrize("model", ["clipped_grid", "relu_grid"])
@pytest.mark.parametrize("name", ge.RIM_NAMES)
def test_oracle_keeps_the_rim_cells_inside_the_grid(oracle, name, model):
    case = ge.rim_case(name)
    X, v, _ = ge.expected(oracle, model, case)
    lo, hi = -(case.gs // 2), case.gs - case.gs // 2
    assert np.isfinite(X).all() and np.abs(X - case.X).max() > 0
    assert X.min() >= lo + 2.0 ** -5 and X.max() <= hi - 2.0 ** -5
    assert ge.max_candidates(case.X, 1.0) < 100


@pytest.mark.parametrize("model,functor", [("clipped_grid", "spring"), ("relu_grid", "relu")])
@pytest.mark.parametrize("name", ge.RIM_NAMES)
def test_oracle_rim_forces_are_the_numpy_statement(oracle, name, model, functor):
    """The rule for a stencil cube that does not exist, stated independently: the statement looks a cube up by its
    linear index, finds nothing below 0 and from n_cubes on, and takes every index in between as it is (also the
    wrapped ones, also the repeated ones of 2 and 1 cubes per axis).  A dt = 0 step with cell 0 held fixed leaves
    rhs - rhs[0] in old_v; clipped_spring is spring inside a cut-off of 1."""
    case = ge.rim_case(name)
    _, got, _ = ge.run(oracle, model, case, dt=0.0, steps=1, fixed=0)
    rhs = reference_forces(case.X, False, old_v=case.v, gs=case.gs, functor=functor)
    assert np.abs(rhs).max() > 0.1
    assert ge.same_bits(rhs - rhs[0], got)
