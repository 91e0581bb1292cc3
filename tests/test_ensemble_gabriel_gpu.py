"""GabrielEnsemble (yalla_amd/ensemble.py over include/ensemble_gabriel.cuh): M Gabriel_solver systems stepped by one
launch sequence.  THE REFERENCE of every comparison is the existing single-system path -- a
Solution("<model>_gabriel", n_max, grid_size, cube_size) per replica, given the same rows, the same old_v and the same
settings (tests/test_gabriel*.py hold that path against the CPU restatement and the numpy statement) -- and every
comparison is of bit patterns (uint32, array_equal): no tolerance anywhere, and positions, old_v[:n] AND the four grid
arrays of every compared replica are compared.

The inputs are those of tests/test_gabriel.py.  Each of them ends in a lone cell, which the single-system tests hold
fixed (set_fixed(n - 1): its force is exactly 0).  An ensemble's set_fixed takes ONE local id for every replica, and
the replicas here differ in size, so every input is rolled by one row -- the lone cell first -- and local id 0 is
held fixed, in the ensemble and in its singles alike: the same cell as in the single-system tests."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gabriel_statement as gab  # noqa: E402
from ensemble_support import DT, Lockstep, bits, compare, seeded_rows  # noqa: E402
from test_gabriel import clusters, fine_lattice, hexagon, lattice, random_260, widened  # noqa: E402

from yalla_amd.ensemble import GabrielEnsemble, gabriel_models  # noqa: E402
from yalla_amd.solution import Solution  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
MODELS = ["relu", "clipped", "relu_plain", "relu_po", "relu_cell", "clipped_push"]
CAP = 64   # GABRIEL_CAP: candidates of a cell the LDS list holds


def lone_first(X):
    """The input with its last row, the lone cell, first (this file's docstring)."""
    return np.ascontiguousarray(np.roll(np.asarray(X, f32), 1, axis=0))


def seeded_old_v(m, n_max, seed=5):
    return (np.random.default_rng(seed).random((m, n_max, 3)) * 0.2 - 0.1).astype(f32)


@functools.lru_cache(maxsize=None)
def mixed_rows():
    """The mixed ensemble's replicas, in the issue's order: hexagon, fine_lattice, empty, random_260, clusters, one
    cell, lattice.  All of them fit a 30^3 grid around the origin."""
    rows = [lone_first(hexagon()[0]), lone_first(fine_lattice()[0]), np.zeros((0, 3), f32),
            lone_first(random_260()[0]), lone_first(clusters()[0]), np.array([[0.25, -0.5, 0.75]], f32),
            lone_first(lattice()[0])]
    for X in rows:
        assert np.all(np.abs(X) < 14)
        X.setflags(write=False)
    return tuple(rows)


MIXED_GS = 30


def n_dense(X, gs):
    """Cells with more than CAP candidates (cube_size 1), from the statement's candidate lists."""
    if len(X) == 0:
        return 0
    ids, _ = gab.candidates(np.ascontiguousarray(X[:, :3], dtype=f32), gs)
    return int(((ids >= 0).sum(axis=1) > CAP).sum())


class GabrielLockstep(Lockstep):
    """A GabrielEnsemble and one Solution per compared replica, fed the same rows (given, not seeded), old_v, Gabriel
    coefficient and fixed cell; the four grid arrays are part of every result."""

    def __init__(self, model, rows, n_max, grid_size, cube_size=1.0, coefficient=0.8, singles=None,
                 single_model=None, old_v=None, fixed=0):
        super().__init__(GabrielEnsemble, "_gabriel", model, [len(X) for X in rows], n_max, (grid_size, cube_size),
                         ens_args=(coefficient,), grids=True, singles=singles, rows=rows, single_model=single_model)
        self.grid_size = grid_size
        for s in self.single.values():
            s.set_param("gabriel_coefficient", coefficient)
        if old_v is not None:
            self.set_old_v(old_v)
        if fixed is not None:
            self.each(lambda s: s.set_fixed(fixed))

    def set_coefficient(self, coefficient):
        self.ens.gabriel_coefficient = coefficient
        for s in self.single.values():
            s.set_param("gabriel_coefficient", coefficient)


def test_the_models_are_those_of_the_gabriel_harness():
    from yalla_amd import models as single_models
    from ensemble_support import FRICTION_MODELS
    assert gabriel_models() == MODELS + FRICTION_MODELS
    assert all(m + "_gabriel" in single_models() for m in MODELS + FRICTION_MODELS if m != "clipped_push")


def test_the_mixed_input_is_what_it_says():
    """Before the first step the dense cells are replicas 2 and 5's only (counting from 1): two dense replicas that
    are not neighbours."""
    dense = [n_dense(X, MIXED_GS) for X in mixed_rows()]
    assert [d > 0 for d in dense] == [False, True, False, False, True, False, False]
    assert dense[1] == 208 and dense[4] == 2 * (65 + 66 + 127 + 128 + 129 + 255 + 256 + 257)


@pytest.mark.parametrize("coefficient", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("model", ["relu", "clipped", "relu_plain"])
def test_the_mixed_ensemble_is_its_single_systems_bit_for_bit(model, coefficient):
    """3 steps of dt 0.05 from a seeded non-zero old_v, the lone cell of every replica held fixed.  dense_cells() is
    checked where it can be predicted exactly: after a dt = 0 step both force stages see the positions the host then
    reads, so it must be the number of cells with more than 64 candidates in the current positions."""
    rows = mixed_rows()
    n_max = len(clusters()[0])
    assert n_max == 3427
    run = GabrielLockstep(model, rows, n_max, MIXED_GS, coefficient=coefficient, old_v=seeded_old_v(len(rows), n_max))
    try:
        assert run.ens.dense_cells() == 0   # (nothing stepped yet)
        run.step(DT, 3)
        run.check("3 steps")
        moved = run.ens.h_X[3, :len(rows[3])]
        assert not np.array_equal(bits(moved), bits(rows[3]))
        run.step(0.0, 1)
        run.check("and a dt = 0 step")
        now = [run.ens.h_X[r, :n] for r, n in enumerate(run.counts)]
        want = sum(n_dense(X, MIXED_GS) for X in now)
        print("dense cells after the steps:", run.ens.dense_cells(), "statement:", want)
        assert run.ens.dense_cells() == want   # (may be 0 by now: relu spreads the clusters; the dense path's own
        #                                        check is test_a_right_hand_side_against_the_numpy_statement's)
    finally:
        run.close()


@pytest.mark.parametrize("model", ["relu", "clipped"])
def test_a_right_hand_side_against_the_numpy_statement(model):
    """The one comparison that does not pass through the single system's device code: a dt = 0 step of the mixed
    ensemble (old_v = 0, the lone cells fixed) leaves every replica's right-hand side in old_v."""
    rows = mixed_rows()
    n_max = len(clusters()[0])
    with GabrielEnsemble(model, len(rows), n_max, MIXED_GS, 1.0, 0.8) as ens:
        for r, X in enumerate(rows):
            ens.h_X[r, :len(X)] = X
            ens.h_n[r] = len(X)
        ens.copy_to_device()
        ens.set_fixed(0)
        ens.take_step(0.0, 1)
        dense = ens.dense_cells()
        ens.copy_to_host()
        v = ens.old_v()
        for r, X in enumerate(rows):
            n = len(X)
            assert np.array_equal(bits(ens.h_X[r, :n]), bits(X)), r   # dt = 0: nothing moved
            if n == 0:
                continue
            want = gab.forces(np.asarray(X), MIXED_GS, 0.8, model + "_gabriel")
            assert (want[0] == 0).all() and (n == 1 or np.abs(want).max() > 0)
            assert np.array_equal(bits(v[r, :n]), bits(want)), ("right-hand side of replica", r)
        assert dense == sum(n_dense(X, MIXED_GS) for X in rows)


def test_ragged_counts_around_the_workgroup_of_four_cells():
    sizes = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65]
    rows = [seeded_rows(3, n, 300 + r, lone=True) for r, n in enumerate(sizes)]
    run = GabrielLockstep("relu", rows, 65, 12, old_v=seeded_old_v(len(sizes), 65))
    try:
        run.step(DT, 3)
        run.check("M = 12")
    finally:
        run.close()
    run = GabrielLockstep("clipped", [seeded_rows(3, 800, 17, lone=True)], 800, 16, old_v=seeded_old_v(1, 800))
    try:
        run.step(DT, 3)
        run.check("M = 1")
    finally:
        run.close()


@pytest.mark.parametrize("model", ["relu_po", "relu_cell"])
def test_wide_point_types(model):
    """Po_cell / Cell: xyz as the single system's, the extra columns untouched."""
    wide = model + "_gabriel"
    rows = [lone_first(widened(random_260()[0], wide)), np.zeros((0, gab.WIDTH[wide]), f32),
            lone_first(widened(clusters()[0], wide, seed=10))]
    n_max = len(rows[2])
    run = GabrielLockstep(model, rows, n_max, MIXED_GS, old_v=seeded_old_v(3, n_max))
    try:
        run.step(DT, 3)
        run.check()
        for r, X in enumerate(rows):
            got = run.ens.h_X[r, :len(X)]
            assert np.array_equal(bits(got[:, 3:]), bits(X[:, 3:])), r
            assert len(X) == 0 or not np.array_equal(bits(got[:, :3]), bits(X[:, :3]))
    finally:
        run.close()


def test_a_generic_force_beside_the_pairwise_one():
    """There is no single `clipped_push_gabriel`: a dt = 0 step of `clipped_push` (old_v = 0, the lone cells fixed)
    is the ensemble's own `clipped` run in every row but cell 1 of every replica, whose right-hand side is
    (1, 0, 0) + F in binary32 -- store_rhs adds the pairwise sum to what the generic force left.  Then whole steps:
    the push moves cell 1, and only replicas that have a cell 1."""
    rows = [lone_first(random_260()[0]), np.zeros((0, 3), f32), lone_first(hexagon()[0]),
            np.array([[0.5, 0.5, 0.5]], f32), lone_first(fine_lattice()[0])]
    n_max = 260

    def stepped(model, dt, steps):
        with GabrielEnsemble(model, len(rows), n_max, MIXED_GS) as ens:
            for r, X in enumerate(rows):
                ens.h_X[r, :len(X)] = X
                ens.h_n[r] = len(X)
            ens.copy_to_device()
            ens.set_fixed(0)
            ens.take_step(dt, steps)
            ens.copy_to_host()
            return ens.h_X.copy(), ens.old_v()

    X0, v0 = stepped("clipped", 0.0, 1)
    X1, v1 = stepped("clipped_push", 0.0, 1)
    assert np.array_equal(bits(X0), bits(X1))
    for r, X in enumerate(rows):
        n = len(X)
        want = v0[r, :n].copy()
        if n > 1:
            want[1] = (np.array([1, 0, 0], f32) + want[1]) + f32(0)
            assert want[1, 0] != v0[r, 1, 0]
        assert np.array_equal(bits(v1[r, :n]), bits(want)), r
    Xa, _ = stepped("clipped", DT, 3)
    Xb, _ = stepped("clipped_push", DT, 3)
    for r, X in enumerate(rows):
        n = len(X)
        assert (n > 1) == (not np.array_equal(bits(Xa[r, :n]), bits(Xb[r, :n]))), r


def test_all_three_fixed_modes():
    """set_fixed() first (the default), set_fixed(i), set_fixed_xy(i) followed by steps, and back."""
    rows = [seeded_rows(3, n, 500 + r, lone=True) for r, n in enumerate([300, 70, 0, 64, 257, 5])]
    run = GabrielLockstep("clipped", rows, 300, 16, fixed=None)
    try:
        run.step(DT, 2)
        run.check("set_fixed()")
        run.each(lambda s: s.set_fixed(4))
        run.step(DT, 3)
        run.check("set_fixed(4)")
        run.each(lambda s: s.set_fixed_xy(2))
        run.step(DT, 3)
        run.check("set_fixed_xy(2)")
        run.each(lambda s: s.set_fixed(1))
        run.step(DT, 2)
        run.check("set_fixed(1) after xy")
        run.each(lambda s: s.set_fixed())
        run.step(DT, 2)
        run.check("set_fixed() after xy")
    finally:
        run.close()


def test_settings_changed_between_steps():
    """gabriel_coefficient and cube_size changed on a live ensemble: the change is visible (the step differs from
    that of an ensemble left alone) and there is no stale step (the singles, changed alike, agree)."""
    rows = [lone_first(random_260()[0]), np.zeros((0, 3), f32), lone_first(clusters(64)[0]),
            seeded_rows(3, 200, 8, lone=True)]
    n_max = max(len(X) for X in rows)
    run = GabrielLockstep("relu", rows, n_max, MIXED_GS)
    alone = GabrielLockstep("relu", rows, n_max, MIXED_GS, singles=[])
    try:
        run.step(DT, 2)
        alone.step(DT, 2)
        run.check("start")
        alone.ens.copy_to_host()
        assert np.array_equal(bits(alone.ens.h_X), bits(run.ens.h_X))
        run.set_coefficient(0.5)
        run.step(DT, 1)
        alone.step(DT, 1)
        run.check("coefficient 0.5")
        alone.ens.copy_to_host()
        assert not np.array_equal(bits(alone.ens.h_X[0]), bits(run.ens.h_X[0]))
        before = run.ens.h_X.copy()
        run.set_cube_size(1.25)
        run.step(DT, 1)
        run.check("cube_size 1.25")
        run.set_coefficient(1.0)
        run.set_cube_size(0.8)
        run.step(DT, 2)
        run.check("coefficient 1.0, cube_size 0.8")
        run.set_coefficient(0.8)
        run.set_cube_size(1.0)
        run.step(DT, 1)
        run.check("and back")
        assert not np.array_equal(bits(before), bits(run.ens.h_X))
    finally:
        run.close()
        alone.close()


def stepped_rows(rows, n_max, grid_size, steps=3):
    with GabrielEnsemble("relu", len(rows), n_max, grid_size) as ens:
        for r, X in enumerate(rows):
            ens.h_X[r, :len(X)] = X
            ens.h_n[r] = len(X)
        ens.copy_to_device()
        ens.set_fixed(0)
        ens.take_step(DT, steps)
        ens.copy_to_host()
        v = ens.old_v()
        return [(bits(ens.h_X[r, :len(X)]).copy(), bits(v[r, :len(X)]).copy()) for r, X in enumerate(rows)]


def test_replicas_are_independent():
    """Replica 4's rows perturbed (it is a dense one: its cells go through the one shared dense list): no bit of
    any other replica changes."""
    rows = list(mixed_rows())
    n_max = len(clusters()[0])
    forward = stepped_rows(rows, n_max, MIXED_GS)
    other = list(rows)
    other[4] = (np.asarray(rows[4]) * f32(1.01)).astype(f32)
    changed = stepped_rows(other, n_max, MIXED_GS)
    for r in range(len(rows)):
        same = np.array_equal(forward[r][0], changed[r][0]) and np.array_equal(forward[r][1], changed[r][1])
        assert same == (r != 4), r
    backward = stepped_rows(rows[::-1], n_max, MIXED_GS)
    for (X, v), (Xb, vb) in zip(forward, backward[::-1]):
        assert np.array_equal(X, Xb) and np.array_equal(v, vb)


def test_many_replicas():
    """4000 replicas of the hexagon in 5^3 grids (the flattened x index of the launch), replicas 0, 1, 1999 and 3999
    against ONE lone Solution run."""
    X = lone_first(hexagon()[0])
    m, n = 4000, len(X)
    with Solution("relu_gabriel", n, 5, 1.0) as s:
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        s.set_fixed(0)
        s.take_step(DT, 3)
        want = (bits(s.positions()).copy(), bits(s.old_v()[:n]).copy(), s.grid())
    assert not np.array_equal(want[0], bits(X))
    with GabrielEnsemble("relu", m, n, 5) as ens:
        ens.h_X[:] = X[None]
        ens.h_n[:] = n
        ens.copy_to_device()
        ens.set_fixed(0)
        ens.take_step(DT, 3)
        assert ens.dense_cells() == 0
        compare(ens, [n] * m, {r: want for r in (0, 1, 1999, 3999)}, "4000 hexagons")
        assert np.array_equal(bits(ens.h_X), np.broadcast_to(want[0], (m, n, 3)))


def face_rows(k, seed):
    """k^3 cells at spacing 1 filling cubes [-3, -3 + k)^3 of a 6^3 grid (one cell per cube, jittered inside it, and
    reaching within 0.002 of the grid's lower faces), after a lone cell in the far corner cube."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)
    X = (g - 3 + 0.002 + 0.3 * rng.random((k ** 3, 3))).astype(f32)
    if k == 6:
        X = X[~np.all(g == 5, axis=1)]   # (the far corner cube is the lone cell's)
        X = X[np.linalg.norm(X - np.array([2.9, 2.9, 2.9]), axis=1) > 1.0]
    return np.vstack([np.array([[2.9, 2.9, 2.9]], f32), X]).astype(f32)


def test_grid_faces_do_not_leak_into_the_next_replica():
    """Three replicas that fill 4^3, 5^3 and 6^3 of a 6^3 grid side by side, with cells on the grid's faces: replica
    r's last cubes and replica r + 1's first are populated, and every stencil row that leaves the grid at a face must
    come back empty or clamped into the replica's own cubes -- as the single system's does -- not with the next
    replica's cells.  (clipped: the clouds contract, nothing leaves the box.)"""
    rows = [face_rows(k, 60 + k) for k in (4, 5, 6)]
    for X in rows:
        assert X.min() < -2.99 and X.min() > -3 and X.max() < 3
    n_max = max(len(X) for X in rows)
    run = GabrielLockstep("clipped", rows, n_max, 6)
    try:
        run.step(DT, 3)
        for r in range(3):
            assert run.ens.status(r, clear=False) == 0, r
        run.check("faces")
    finally:
        run.close()


def test_a_replica_that_leaves_its_grid_is_reported_and_harms_nobody():
    counts = [100, 64, 257, 30]
    bad = 2
    rows = [seeded_rows(3, n, 90 + r, lone=True) for r, n in enumerate(counts)]
    rows[bad][5] = (0.0, 0.0, 100.0)  # far above the 12^3 grid: its cube id is past the last cube's
    run = GabrielLockstep("relu", rows, 300, 12, singles=[r for r in range(len(counts)) if r != bad])
    try:
        run.step(DT, 1)
        for r in range(len(counts)):
            assert (run.ens.status(r, clear=False) != 0) == (r == bad), r
        assert run.ens.status(bad, clear=True) != 0
        assert run.ens.status(bad, clear=False) == 0  # forgotten: copy_to_host will not abort
        run.check("beside a replica that left its grid")
    finally:
        run.close()
