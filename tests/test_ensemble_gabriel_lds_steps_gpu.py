"""GabrielLdsEnsemble (yalla_amd/ensemble.py over include/yalla_ensemble_gabriel_lds.h): Ensemble<Pt, Gabriel_solver>::
take_steps as launches of one workgroup per replica that step from LDS (ya::ens::gabriel_lds_steps), cells with more
than 64 candidates done inside the launch.

THE REFERENCE of every comparison is BOTH the same class with lds_steps = -1 (the 16-launch path: every row of positions
and old_v, used or not, every replica's four grid arrays and status) AND a lone Solution("<model>_gabriel") per
compared replica (positions, old_v[:n], the four grid arrays).  Every comparison is of bit patterns, no tolerance
anywhere.  Every run that expects launches from LDS asserts `lds_step_launches`; every fallback asserts that it did
not move.  The one comparison that does not pass through shared device code is the numpy statement's
(tests/gabriel_statement.py)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gabriel_statement as gab  # noqa: E402
from ensemble_support import DT, Lockstep, bits, same_grid, seeded_rows  # noqa: E402
from test_ensemble_gabriel_gpu import GabrielLockstep, lone_first, n_dense, seeded_old_v  # noqa: E402
from test_gabriel import CLUSTER_SIZES, fine_lattice, hexagon, lattice, random_260  # noqa: E402

from yalla_amd.ensemble import GabrielEnsemble, GabrielLdsEnsemble, gabriel_lds_models, gabriel_models  # noqa: E402
from yalla_amd.solution import Solution  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
CAP = 64
MODELS = ["relu", "relu_plain", "clipped", "relu_po", "relu_cell", "friction_ids", "friction_ids_plain", "friction_field"]
N_FLOATS = {"relu_po": 5, "relu_cell": 7, "friction_field": 5}


def widen(rows, model, seed=21):
    """The rows with the further fields of the model's point type, uniform in [0, 1)."""
    width = N_FLOATS.get(model, 3)
    if width == 3:
        return list(rows)
    rng = np.random.default_rng(seed)
    return [np.hstack([X, rng.random((len(X), width - 3)).astype(f32)]).astype(f32) for X in rows]


def capacity_of(model):
    """ya::ens::gabriel_lds_capacity of the model's point type, from the library's own rule (tests/
    test_ensemble_gabriel_lds_abi.py holds that rule against its restatement)."""
    fits = [n for n in range(1, 1026) if GabrielLdsEnsemble.lds_bytes(model, n) > 0]
    assert fits == list(range(1, len(fits) + 1))
    return len(fits)


class LdsTwins(Lockstep):
    """A GabrielLdsEnsemble with lds_steps = 1, its lone Solutions (GabrielLockstep's settings), and a second
    GabrielLdsEnsemble of the same rows that keeps the 16 launches (lds_steps = -1, the harness's default).  Unused
    rows hold a pattern of their own, to be found again."""

    set_coefficient_of_the_pair = GabrielLockstep.set_coefficient

    def __init__(self, model, rows, n_max, grid_size, cube_size=1.0, coefficient=0.8, singles=None, old_v=None,
                 fixed=0, lds_steps=1):
        super().__init__(GabrielLdsEnsemble, "_gabriel", model, [len(X) for X in rows], n_max, (grid_size, cube_size),
                         ens_args=(coefficient,), grids=True, singles=singles, rows=rows)
        self.grid_size = grid_size
        self.ens.set_param("lds_steps", lds_steps)
        self.twin = GabrielLdsEnsemble(model, len(rows), n_max, grid_size, cube_size, coefficient)
        unused = np.arange(n_max)[None, :] >= np.asarray(self.counts)[:, None]
        self.ens.h_X[unused] = f32(-7.25)
        self.twin.h_X[:] = self.ens.h_X
        self.twin.h_n[:] = self.counts
        self.ens.copy_to_device()
        self.twin.copy_to_device()
        for s in self.single.values():
            s.set_param("gabriel_coefficient", coefficient)
        if old_v is not None:
            self.set_old_v(old_v)
        if fixed is not None:
            self.each(lambda s: s.set_fixed(fixed))
        self.seen = 0

    def each(self, call):
        super().each(call)
        call(self.twin)

    def set_old_v(self, v):
        super().set_old_v(v)
        self.twin.set_old_v(v)

    def set_coefficient(self, coefficient):
        self.set_coefficient_of_the_pair(coefficient)
        self.twin.gabriel_coefficient = coefficient

    def expect_launches(self, n, what=""):
        """lds_step_launches rose by n since the last look; the 16-launch twin never made one."""
        assert self.ens.lds_step_launches - self.seen == n, (what, self.ens.lds_step_launches, self.seen, n)
        self.seen = self.ens.lds_step_launches
        assert self.twin.lds_step_launches == 0 and self.twin.lds_dense_cells() == 0

    def check(self, what="", statuses=True):
        """Against the lone Solutions (used rows, grids), and against the 16-launch twin: EVERY row, every grid."""
        super().check(what)
        if statuses:
            for r in range(len(self.counts)):
                assert self.ens.status(r, clear=False) == self.twin.status(r, clear=False), (what, "status", r)
        self.twin.copy_to_host()
        assert list(self.twin.h_n) == list(self.ens.h_n), what
        assert np.array_equal(bits(self.twin.h_X), bits(self.ens.h_X)), (what, self.model, "positions")
        assert np.array_equal(bits(self.twin.old_v()), bits(self.ens.old_v())), (what, self.model, "old_v")
        for r, n in enumerate(self.counts):
            assert same_grid(self.ens.grid(r), self.twin.grid(r), n), (what, self.model, "grid arrays of replica", r)

    def close(self):
        super().close()
        self.twin.close()


# ---- the inputs ------------------------------------------------------------------------------------------------------
BALLS_GS = 16


@functools.lru_cache(maxsize=None)
def balls():
    """One replica per (K, corner) for K in CLUSTER_SIZES: K cells inside a ball of radius 0.45 around a cube's centre
    (one cube) or a cube's corner (8 cubes), after a lone cell 3 cubes away.  48 replicas of K + 1 cells."""
    rng = np.random.default_rng(164)
    rows = []
    for K in CLUSTER_SIZES:
        for corner in (False, True):
            centre = 0.0 if corner else 0.5
            v = rng.standard_normal((K, 3))
            v *= (0.45 * rng.random(K) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
            X = np.vstack([np.array([[3.5, 3.5, 3.5]]), centre + v]).astype(f32) + f32(0)
            X.setflags(write=False)
            rows.append(X)
    return tuple(rows)


BALLS_N_MAX = 258
MIXED_GS = 30
MIXED_N_MAX = 260


@functools.lru_cache(maxsize=None)
def mixed():
    """hexagon, lattice, fine_lattice, an empty replica, one cell, random_260 (tests/test_gabriel.py), the lone cells
    first."""
    rows = [lone_first(hexagon()[0]), lone_first(lattice()[0]), lone_first(fine_lattice()[0]), np.zeros((0, 3), f32),
            np.array([[0.25, -0.5, 0.75]], f32), lone_first(random_260()[0])]
    for X in rows:
        assert np.all(np.abs(X) < 14) and len(X) <= MIXED_N_MAX
        X.setflags(write=False)
    return tuple(rows)


def candidate_counts(X, gs):
    return (gab.candidates(np.ascontiguousarray(X[:, :3], dtype=f32), gs)[0] >= 0).sum(axis=1)


def test_the_models_are_the_gabriel_harness_s():
    assert gabriel_lds_models() == gabriel_models()
    assert set(MODELS) | {"clipped_push"} == set(gabriel_lds_models())


def test_the_inputs_are_what_they_say():
    """A ball's cells have exactly K candidates each (the lone cell 1): the 64-entry list at 63 / 64 | 65 / 66, the
    lane groups at 15 / 16 / 17, the dense chunks at 127 ... 257.  lattice and fine_lattice are full of ties;
    fine_lattice's cells beyond the 8 corners are dense."""
    rows = balls()
    assert len(rows) == 48 and max(len(X) for X in rows) == BALLS_N_MAX
    for X, K in zip(rows, [K for K in CLUSTER_SIZES for _ in (0, 1)]):
        counts = candidate_counts(X, BALLS_GS)
        assert len(X) == K + 1 and counts[0] == 1 and (counts[1:] == K).all(), K
    assert {63, 64, 65, 66, 15, 16, 17, 127, 128, 129, 255, 256, 257} <= set(CLUSTER_SIZES)
    assert sum(n_dense(X, BALLS_GS) for X in rows) == 2 * (65 + 66 + 127 + 128 + 129 + 255 + 256 + 257)
    dense = [n_dense(X, MIXED_GS) for X in mixed()]
    assert dense == [0, 0, 208, 0, 0, 0]
    for X in (mixed()[1], mixed()[2]):
        _, dist = gab.candidates(np.ascontiguousarray(X), MIXED_GS)
        tied = [len(np.unique(d[np.isfinite(d)])) < np.isfinite(d).sum() for d in dist[1:]]
        assert all(tied)


# ---- balls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coefficient", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("model", MODELS)
def test_balls(model, coefficient):
    """1 step from old_v = 0, then 5 steps from a seeded non-zero old_v, then K = 2 steps of dt = 0, after which
    lds_dense_cells() has grown by exactly 2 K (cells with more than 64 candidates, by the statement)."""
    rows = widen(balls(), model)
    run = LdsTwins(model, rows, BALLS_N_MAX, BALLS_GS, coefficient=coefficient)
    try:
        run.step(DT, 1)
        run.expect_launches(1, "1 step")
        run.check("1 step")
        run.set_old_v(seeded_old_v(len(rows), BALLS_N_MAX))
        run.step(DT, 5)
        run.expect_launches(1, "5 steps")
        run.check("5 steps")
        assert not np.array_equal(bits(run.ens.h_X[20, :len(rows[20])]), bits(rows[20]))
        now = [run.ens.h_X[r, :n, :3].copy() for r, n in enumerate(run.counts)]
        want = sum(n_dense(X, BALLS_GS) for X in now)
        before = run.ens.lds_dense_cells()
        run.step(0.0, 2)
        run.expect_launches(1, "dt = 0")
        run.check("2 steps of dt = 0")
        print("dense cells:", want, "counter:", before, "->", run.ens.lds_dense_cells())
        assert run.ens.lds_dense_cells() - before == 2 * 2 * want
    finally:
        run.close()


# ---- mixed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coefficient", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("model", ["relu", "relu_plain", "clipped"])
def test_mixed(model, coefficient):
    """Ties in the LDS list (lattice, fine_lattice's corners), ties and cells exactly on a sphere in the dense lists
    (fine_lattice at coefficient 1.0), an empty replica -- whose grid arrays stay -1 / -1 -- and one cell."""
    rows = mixed()
    run = LdsTwins(model, rows, MIXED_N_MAX, MIXED_GS, coefficient=coefficient,
                   old_v=seeded_old_v(len(rows), MIXED_N_MAX))
    try:
        run.step(DT, 1)
        run.expect_launches(1)
        run.check("1 step")
        run.step(DT, 5)
        run.expect_launches(1)
        run.check("5 steps")
        assert run.ens.lds_dense_cells() > 0
        _, _, start, end = run.ens.grid(3)
        assert (start == -1).all() and (end == -1).all(), "the empty replica's grid was never built"
    finally:
        run.close()


# ---- the numpy statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["balls", "mixed"])
@pytest.mark.parametrize("model", ["relu", "clipped"])
def test_a_right_hand_side_against_the_numpy_statement(model, which):
    """A dt = 0 step with old_v = 0 and the lone cells fixed leaves every replica's right-hand side in old_v."""
    rows, n_max, gs = (balls(), BALLS_N_MAX, BALLS_GS) if which == "balls" else (mixed(), MIXED_N_MAX, MIXED_GS)
    with GabrielLdsEnsemble(model, len(rows), n_max, gs, 1.0, 0.8) as ens:
        for r, X in enumerate(rows):
            ens.h_X[r, :len(X)] = X
            ens.h_n[r] = len(X)
        ens.copy_to_device()
        ens.set_fixed(0)
        ens.set_param("lds_steps", 1)
        ens.take_step(0.0, 1)
        assert ens.lds_step_launches == 1
        ens.copy_to_host()
        v = ens.old_v()
        for r, X in enumerate(rows):
            n = len(X)
            assert np.array_equal(bits(ens.h_X[r, :n]), bits(X)), r   # dt = 0: nothing moved
            if n == 0:
                continue
            want = gab.forces(np.asarray(X), gs, 0.8, model + "_gabriel")
            assert (want[0] == 0).all() and (n <= 2 or np.abs(want).max() > 0)
            assert np.array_equal(bits(v[r, :n]), bits(want)), ("right-hand side of replica", r)
        assert ens.lds_dense_cells() == 2 * sum(n_dense(X, gs) for X in rows)
        assert ens.dense_cells() == 0  # (the 16-launch path's: it never ran)


# ---- counts ----------------------------------------------------------------------------------------------------------
def test_counts_in_one_ensemble():
    """Ragged counts around the round of 16 cells, the 64-entry list, the workgroup's 256 threads and the capacity."""
    capacity = capacity_of("relu")
    sizes = sorted({min(n, capacity) for n in (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024)})
    rows = [seeded_rows(3, n, 300 + r, lone=True) for r, n in enumerate(sizes)]
    run = LdsTwins("relu", rows, capacity, 16, old_v=seeded_old_v(len(sizes), capacity))
    try:
        run.step(DT, 3)
        run.expect_launches(1)
        run.check("counts")
    finally:
        run.close()


# ---- capacity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["relu", "relu_po", "relu_cell"])
def test_capacity_and_one_more(model):
    """One replica of capacity cells inside a ball of radius 0.45: every cell is dense, with n candidates, in both
    stages (dt = 0.001: no pair, at most 0.9 apart, gets beyond 1).  One row more is the 16-launch loop."""
    capacity = capacity_of(model)
    rng = np.random.default_rng(7)
    v = rng.standard_normal((capacity + 1, 3))
    v *= (0.45 * rng.random(capacity + 1) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    ball = (0.5 + v).astype(f32)
    assert (candidate_counts(ball[:capacity], 6) == capacity).all()
    for n, launches in ((capacity, 1), (capacity + 1, 0)):
        run = LdsTwins(model, widen([ball[:n]], model), n, 6, fixed=None)
        try:
            run.step(0.001, 1)
            run.expect_launches(launches, n)
            run.check(("capacity", n))
            assert run.ens.lds_dense_cells() == (2 * n if launches else 0)
            assert (run.ens.dense_cells() == n) == (launches == 0)
        finally:
            run.close()


# ---- other cases -----------------------------------------------------------------------------------------------------
def test_all_three_fixed_modes():
    rows = [seeded_rows(3, n, 500 + r, lone=True) for r, n in enumerate([300, 70, 0, 64, 257, 5])]
    run = LdsTwins("clipped", rows, 300, 16, fixed=None)
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
        run.expect_launches(5)
    finally:
        run.close()


@pytest.mark.parametrize("steps_max, launches", [(1, 5), (2, 3), (256, 1)])
def test_steps_per_launch(steps_max, launches):
    rows = [lone_first(random_260()[0]), np.zeros((0, 3), f32), balls()[35], seeded_rows(3, 100, 8, lone=True)]
    run = LdsTwins("relu", rows, MIXED_N_MAX, MIXED_GS, old_v=seeded_old_v(len(rows), MIXED_N_MAX))
    try:
        run.ens.set_param("lds_steps_max", steps_max)
        run.step(DT, 5)
        run.expect_launches(launches)
        run.check(("lds_steps_max", steps_max))
    finally:
        run.close()


def test_the_engine_s_choice_and_never():
    """lds_steps = 0 asks ya::ens::gabriel_lds_steps_pay, -1 never steps from LDS: the same bits, and the count says
    which path ran.  The rule answers true up to 16 rows per replica (one round) and 256 replicas."""
    rows = [lone_first(random_260()[0]), balls()[33]]
    small = [balls()[10], np.zeros((0, 3), f32), balls()[6]]
    assert [len(X) for X in small] == [16, 0, 5]
    for mode, these, n_max, gs, launches in ((0, rows, MIXED_N_MAX, MIXED_GS, 0), (-1, rows, MIXED_N_MAX, MIXED_GS, 0),
                                             (0, small, 16, BALLS_GS, 1), (0, small, 17, BALLS_GS, 0),
                                             (-1, small, 16, BALLS_GS, 0)):
        run = LdsTwins("relu", these, n_max, gs, lds_steps=mode)
        try:
            run.step(DT, 2)
            run.expect_launches(launches, (mode, n_max))
            run.check(("lds_steps", mode, n_max))
        finally:
            run.close()


def test_settings_changed_between_calls():
    rows = [lone_first(random_260()[0]), np.zeros((0, 3), f32), balls()[32], seeded_rows(3, 200, 8, lone=True)]
    run = LdsTwins("relu", rows, MIXED_N_MAX, MIXED_GS)
    try:
        run.step(DT, 2)
        run.check("start")
        before = run.ens.h_X.copy()
        run.set_coefficient(0.5)
        run.step(DT, 1)
        run.check("coefficient 0.5")
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
        run.expect_launches(5)
        assert not np.array_equal(bits(before), bits(run.ens.h_X))
    finally:
        run.close()


def test_a_cell_outside_the_grid():
    """The status bit and the clamped grid arrays are the 16-launch path's; the other replicas are their singles."""
    counts = [100, 64, 257, 30]
    bad = 2
    rows = [seeded_rows(3, n, 90 + r, lone=True) for r, n in enumerate(counts)]
    rows[bad][5] = (0.0, 0.0, 100.0)  # far above the 12^3 grid: its cube id is past the last cube's
    run = LdsTwins("relu", rows, 300, 12, singles=[r for r in range(len(counts)) if r != bad])
    try:
        run.step(DT, 1)
        run.expect_launches(1)
        for e in (run.ens, run.twin):
            for r in range(len(counts)):
                assert (e.status(r, clear=False) != 0) == (r == bad), r
            assert e.status(bad, clear=True) != 0
            assert e.status(bad, clear=False) == 0  # forgotten: copy_to_host will not abort
        run.check("beside a replica that left its grid")
    finally:
        run.close()


def test_a_generic_force_falls_back():
    """clipped_push: the 16-launch loop, the same bits as libyalla_ensemble_gabriel.so's."""
    rows = [lone_first(random_260()[0]), np.zeros((0, 3), f32), lone_first(hexagon()[0]), balls()[34]]
    results = []
    for cls in (GabrielLdsEnsemble, GabrielEnsemble):
        with cls("clipped_push", len(rows), MIXED_N_MAX, MIXED_GS) as ens:
            for r, X in enumerate(rows):
                ens.h_X[r, :len(X)] = X
                ens.h_n[r] = len(X)
            ens.copy_to_device()
            ens.set_fixed(0)
            if cls is GabrielLdsEnsemble:
                ens.set_param("lds_steps", 1)
            ens.take_step(DT, 3)
            if cls is GabrielLdsEnsemble:
                assert ens.lds_step_launches == 0 and ens.lds_dense_cells() == 0
            ens.copy_to_host()
            results.append((bits(ens.h_X).copy(), bits(ens.old_v()).copy(), [ens.grid(r) for r in range(len(rows))]))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    for r, X in enumerate(rows):
        assert same_grid(results[0][2][r], results[1][2][r], len(X)), r
    assert not np.array_equal(results[0][0][0, :260], bits(rows[0]))


def stepped_rows(rows, n_max, grid_size, steps=3):
    with GabrielLdsEnsemble("relu", len(rows), n_max, grid_size) as ens:
        for r, X in enumerate(rows):
            ens.h_X[r, :len(X)] = X
            ens.h_n[r] = len(X)
        ens.copy_to_device()
        ens.set_fixed(0)
        ens.set_param("lds_steps", 1)
        ens.take_step(DT, steps)
        assert ens.lds_step_launches == 1
        ens.copy_to_host()
        v = ens.old_v()
        return [(bits(ens.h_X[r, :len(X)]).copy(), bits(v[r, :len(X)]).copy()) for r, X in enumerate(rows)]


def test_replicas_are_independent():
    """Replica 2's rows perturbed (a dense one): no bit of any other replica changes; nor does the replicas' order."""
    rows = list(mixed())
    forward = stepped_rows(rows, MIXED_N_MAX, MIXED_GS)
    other = list(rows)
    other[2] = (np.asarray(rows[2]) * f32(1.01)).astype(f32)
    changed = stepped_rows(other, MIXED_N_MAX, MIXED_GS)
    for r in range(len(rows)):
        same = np.array_equal(forward[r][0], changed[r][0]) and np.array_equal(forward[r][1], changed[r][1])
        assert same == (r != 2 or len(rows[r]) == 0), r
    backward = stepped_rows(rows[::-1], MIXED_N_MAX, MIXED_GS)
    for (X, v), (Xb, vb) in zip(forward, backward[::-1]):
        assert np.array_equal(X, Xb) and np.array_equal(v, vb)


def test_many_replicas():
    """5000 replicas of 20 cells (the hexagon and its lone cell) against ONE lone Solution run."""
    X = lone_first(hexagon()[0])
    m, n = 5000, len(X)
    assert n == 20
    with Solution("relu_gabriel", n, 5, 1.0) as s:
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        s.set_fixed(0)
        s.take_step(DT, 3)
        want = (bits(s.positions()).copy(), bits(s.old_v()[:n]).copy(), s.grid())
    assert not np.array_equal(want[0], bits(X))
    with GabrielLdsEnsemble("relu", m, n, 5) as ens:
        ens.h_X[:] = X[None]
        ens.h_n[:] = n
        ens.copy_to_device()
        ens.set_fixed(0)
        ens.set_param("lds_steps", 1)
        ens.take_step(DT, 3)
        assert ens.lds_step_launches == 1 and ens.lds_dense_cells() == 0
        ens.copy_to_host()
        assert np.array_equal(bits(ens.h_X), np.broadcast_to(want[0], (m, n, 3)))
        assert np.array_equal(bits(ens.old_v()), np.broadcast_to(want[1], (m, n, 3)))
        for r in (0, 1, 2499, 4999):
            assert same_grid(ens.grid(r), want[2], n), r
