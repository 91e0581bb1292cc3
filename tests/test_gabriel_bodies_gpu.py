"""ya::gabriel_force's two bodies, the edges of its list and its fast tier (include/solvers.cuh).

A functor that is not declared YA_STATELESS takes gabriel::test_and_sum on the LDS lists (`relu_plain_gabriel`,
`count_gabriel`); a declared one has its terms evaluated by the lanes (`relu_gabriel`, `clipped_gabriel`, and
the wide point types `relu_po_gabriel` / `relu_cell_gabriel`).  Both are held bit for bit against each other,
the CPU restatement and the numpy statement (gabriel_statement.py), on inputs that put cells on either side of
GABRIEL_CAP = 64, on every boundary of the lane groups and of the dense kernel's 64-lane chunks (`clusters`), and
that carry tied distances into ya::gabriel_force_dense (`fine_lattice`).  The per-cell counters of the
reference's KAT are compared exactly.  The fast tier is held to the statement within the tier's tolerance away
from decision boundaries."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gabriel_statement as gab  # noqa: E402
from test_gabriel import (CASES, ball_5000, cluster_sizes, clusters, counts, fine_lattice, n_candidates,  # noqa: E402
                          random_260, run, same_bits, sphere, twins, widened)

from yalla_amd.solution import Solution  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
REL_TOL = 1e-5                                                # the fast tier's tolerance (test_fast_arith_gpu.py)
COEFFICIENTS = (0.5, 0.8, 1.0)
ALL_CASES = list(CASES) + ["sphere_5000"]


def case_input(case, oracle):
    if case == "twins":
        return twins()
    return sphere(5000, oracle) if case == "sphere_5000" else CASES[case]()


def whole_steps(case):
    """20 steps on the sparse cases; 2 short ones where cells sit 0.01 apart (clusters, the 0.25 lattice)."""
    return dict(steps=2, dt=1e-4) if case in ("clusters", "fine_lattice") else dict(steps=20, dt=0.05)


def differing(a, b, X, gs):
    """Which cells differ, by candidate count (on `clusters` that is the cluster's size K): {count: cells}."""
    a, b = np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32)
    rows = (a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1)
    if not rows.any():
        return {}
    c = n_candidates(X, gs)[rows]
    return {int(k): int((c == k).sum()) for k in np.unique(c)}


@pytest.mark.parametrize("coefficient", COEFFICIENTS)
@pytest.mark.parametrize("case", ALL_CASES)
def test_the_two_bodies_agree_with_each_other_the_oracle_and_the_statement(device, oracle, case, coefficient):
    X, gs = case_input(case, oracle)
    if case == "clusters":                                    # from the statement: both kernels have cells
        c = n_candidates(X, gs)
        assert (c <= 64).sum() == 861 and (c >= 65).sum() == 2566 and {63, 64, 65, 66} <= set(c)
    want = gab.forces(X, gs, coefficient, "relu_plain_gabriel")
    assert np.abs(want).max() > 0
    for model in ("relu_plain_gabriel", "relu_gabriel"):
        Xd, F = run(device, model, X, gs, coefficient)
        assert same_bits(Xd, X)
        assert same_bits(F, want), f"{model}: force differs; cells by candidate count: {differing(F, want, X, gs)}"
    Xo, vo = run(oracle, "relu_plain_gabriel", X, gs, coefficient, **whole_steps(case))
    assert not same_bits(Xo, X)
    Xp, vp = run(device, "relu_plain_gabriel", X, gs, coefficient, **whole_steps(case))
    Xr, vr = run(device, "relu_gabriel", X, gs, coefficient, **whole_steps(case))
    assert same_bits(Xp, Xr) and same_bits(vp, vr), f"plain != stateless; cells by candidate count: {differing(Xp, Xr, X, gs)}"
    assert same_bits(Xp, Xo) and same_bits(vp, vo), f"plain != oracle; cells by candidate count: {differing(Xp, Xo, X, gs)}"
    assert same_bits(Xr, Xo) and same_bits(vr, vo), f"stateless != oracle; cells by candidate count: {differing(Xr, Xo, X, gs)}"


def run_variant(lib, model, X, gs, coefficient, variant):
    n = len(X)
    with Solution(model, n, gs, 1.0, lib=lib) as s:
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        s.set_param("gabriel_coefficient", coefficient)
        s.set_param("force_variant", variant)
        s.set_fixed(n - 1)
        s.take_step(0.0, 1)
        return s.old_v()[:n].copy()


@pytest.mark.parametrize("coefficient", COEFFICIENTS)
def test_the_kept_baseline_agrees_up_to_the_capacity(device, coefficient):
    """gabriel_force_direct (force_variant 0: one thread per cell, a private list of 100) is a second,
    independent device path: on the clusters of K <= 64 -- exactly the cells the LDS kernel keeps, its last
    slot included -- it gives the statement's bits, and so does the default kernel."""
    X, gs = clusters(64)
    size = cluster_sizes(64)
    assert np.array_equal(n_candidates(X, gs), size) and size.max() == 64 and {63, 64, 48, 49, 16, 17} <= set(size)
    want = gab.forces(X, gs, coefficient, "relu_gabriel")
    for variant in (0, -1):
        F = run_variant(device, "relu_gabriel", X, gs, coefficient, variant)
        assert same_bits(F, want), f"force_variant {variant}; cells by cluster size: {differing(F, want, X, gs)}"


@pytest.mark.parametrize("coefficient", COEFFICIENTS)
@pytest.mark.parametrize("model", ["relu_gabriel", "clipped_gabriel", "relu_plain_gabriel"])
def test_ties_reach_the_dense_kernel(device, oracle, model, coefficient):
    """fine_lattice: 208 cells with 65 to 188 candidates, every one with tied distances -- the reference's
    unstable selection sort on gabriel_force_dense's global lists (`int` indices), in both of its callers."""
    X, gs = fine_lattice()
    assert (n_candidates(X, gs) > 64).sum() == 208
    _, F = run(device, model, X, gs, coefficient)
    want = gab.forces(X, gs, coefficient, model)
    assert np.abs(want).max() > 0.1
    assert same_bits(F, want), f"cells by candidate count: {differing(F, want, X, gs)}"
    Xo, vo = run(oracle, model, X, gs, coefficient, steps=2, dt=1e-4)
    Xd, vd = run(device, model, X, gs, coefficient, steps=2, dt=1e-4)
    assert not same_bits(Xo, X)
    assert same_bits(Xd, Xo) and same_bits(vd, vo), f"cells by candidate count: {differing(Xd, Xo, X, gs)}"


@pytest.mark.parametrize("case", ALL_CASES + ["twins"])
def test_the_per_cell_counters(device, oracle, case):
    """count_gabriel (`d_n_nbs[i] += 1` from inside the functor, tests/test_solvers.cu:339-381): one lane of 16
    (LDS kernel) or of 64 (dense kernel) calls the functor, once per kept pair.  Twice on one system and once
    more on a second one: the counters are zeroed every stage, nothing is left over.  `twins` has coincident
    cells: there the first entry of a sorted list can be a neighbour, not the cell itself."""
    X, gs = case_input(case, oracle)
    for coefficient in COEFFICIENTS:
        want = gab.neighbour_counts(X, gs, coefficient)
        assert want.max() > 0 and want[-1] == 0
        assert np.array_equal(counts(oracle, X, gs, coefficient), want), coefficient
        first, second = counts(device, X, gs, coefficient, repeat=2)
        assert np.array_equal(first, want), f"coefficient {coefficient}; cells by candidate count: {differing(first, want, X, gs)}"
        assert np.array_equal(second, want), f"coefficient {coefficient}, second step: {differing(second, want, X, gs)}"
    assert np.array_equal(counts(device, X, gs, 0.8), gab.neighbour_counts(X, gs, 0.8))
    if case == "hexagon":                                     # the reference's KAT: 6 / 3 / 4
        got = counts(device, X, gs, 0.8)
        assert (got[:7] == 6).all() and (got[7:19:2] == 3).all() and (got[8:19:2] == 4).all()


@pytest.mark.parametrize("case", ["random_260", "clusters", "sphere_5000"])
@pytest.mark.parametrize("model", ["relu_po_gabriel", "relu_cell_gabriel"])
def test_wide_point_types_through_the_stateless_body(device, oracle, model, case):
    """Po_cell (5 floats) and Cell (7): the kept pairs' terms lie over the position arrays as
    sh_list[cell][NF + 4][CAP].  xyz as relu_gabriel on the same xyz, the extra columns untouched."""
    X3, gs = case_input(case, oracle)
    X = widened(X3, model)
    for coefficient in COEFFICIENTS:
        _, F = run(device, model, X, gs, coefficient)
        want = gab.forces(X, gs, coefficient, model)
        assert same_bits(F, want[:, :3]), f"coefficient {coefficient}; cells by candidate count: {differing(F, want[:, :3], X3, gs)}"
    Xw, vw = run(device, model, X, gs, None, **whole_steps(case))
    Xr, vr = run(device, "relu_gabriel", X3, gs, None, **whole_steps(case))
    Xo, vo = run(oracle, model, X, gs, None, **whole_steps(case))
    assert not same_bits(Xr, X3)
    assert same_bits(Xw[:, :3], Xr) and same_bits(vw, vr), f"!= relu_gabriel: {differing(Xw[:, :3], Xr, X3, gs)}"
    assert same_bits(Xw[:, 3:], X[:, 3:])
    assert same_bits(Xw, Xo) and same_bits(vw, vo), f"!= oracle: {differing(Xw, Xo, X3, gs)}"


@pytest.mark.parametrize("coefficient", [0.6, 0.8])
@pytest.mark.parametrize("case", ["random_260", "ball_5000"])
@pytest.mark.parametrize("model", ["relu_gabriel", "clipped_gabriel", "relu_plain_gabriel"])
def test_fast_tier_force_is_the_statement_away_from_decisions(model, case, coefficient):
    """libyalla_models_fast.so (contracted multiply-adds, bare v_sqrt_f32 / v_rcp_f32): a dt = 0 force against the
    statement.  A cell is excused (held to finite) only if a decision of its own is within 1e-6, relative, of
    flipping (gab.decision_cells, from the positions in binary64): a 1-ulp v_sqrt_f32, half an ulp from a
    contracted radicand and half an ulp each for the midpoint and the radius are <= 4 ulp ~ 2.4e-7 per side, and
    1e-6 covers both sides twice.  At most 1 % of the cells may be excused (none is, on these inputs); every
    other cell is within the tier's tolerance, 1e-5 of the largest force.  Coefficient 1.0 is left out: there a
    cell's own position is ON the sphere of each of its pairs, and every cell is a decision.
    Worst observed |got - want| / max|want| (MI355X): see DESIGN.md, section 4, "Gabriel_solver"."""
    from yalla_amd import _ffi
    X, gs = {"random_260": random_260, "ball_5000": ball_5000}[case]()
    marked = gab.decision_cells(X, gs, coefficient)
    assert marked.mean() <= 0.01 and marked.sum() == 0
    want = gab.forces(X, gs, coefficient, model)
    Xf, F = run(_ffi.device_lib("fast"), model, X, gs, coefficient)
    assert same_bits(Xf, X) and np.isfinite(F).all()
    scale = np.abs(want).max()
    assert scale > 0.1
    ratio = np.abs(F - want).max(axis=1)[~marked].max() / scale
    print(f"fast tier {model} {case} coefficient {coefficient}: marked {int(marked.sum())} of {len(X)}, "
          f"worst ratio {ratio:.3g}")
    over = np.where(np.abs(F - want) > REL_TOL * scale, 1, 0)
    assert ratio <= REL_TOL, (f"worst |got - want| / max|want| = {ratio:.3g} on unmarked cells; cells over the "
                              f"tolerance by candidate count: {differing(over, np.zeros_like(over), X, gs)}")
