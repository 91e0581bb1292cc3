"""Several lanes per cell inside a whole-step launch (ya::ens::whole_steps_coop, include/ensemble.cuh):
set_param("whole_step_lanes", 4 | 16 | 64) shares a cell's pairs among that many lanes of the replica's workgroup, 0
leaves the number to the engine, 1 (the harness's default) is the one-thread-per-cell kernel.  The result must be the
bits of the six-launch step.  THE REFERENCES are code this feature does not touch -- the same Ensemble with
whole_steps = -1, a lone Solution("<model>_tile") per replica, and the CPU restatement -- and every comparison is of
bit patterns (uint32, array_equal): no tolerance anywhere.  Every case checks `whole_step_launches`."""
import functools

import numpy as np
import pytest
from ensemble_support import (DT, LDS, MIN_TILE, STATIC_LDS, WHOLE, Twins, bits, capacity, coop_rule_edges,
                              lds_layout, seeded_rows)

from yalla_amd.ensemble import Ensemble, YallaError
from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu

LANES = [4, 16, 64]
# n < L (lanes without a partner); 4, 16 and 64 cells per round, both sides; a wavefront; the longest tile and the
# fold's block; several tiles and several partial-sum blocks
RAGGED = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024]
N_FLOATS = {"springs": 3, "clipped": 3, "fading": 3, "relu": 3, "relu_po": 5, "oscillator": 4}


def rule_edges(n_floats, n_max_up_to):
    """Every n_max either side of a point where another term of ya::ens::lds_layout's term-buffer rule (restated in
    ensemble_support) starts to decide, for any of LANES."""
    return coop_rule_edges(n_floats, n_max_up_to, LANES)


def test_the_restated_rule():
    """What the comments of the header promise of the rule, on the restatement the cases below are derived from."""
    for n_floats in (3, 4, 5, 8):
        for lanes in LANES:
            for n_max in (1, 16, 17, 64, 300, capacity(n_floats)):
                tile = lds_layout(n_floats, n_max, lanes=lanes).tile
                assert tile % 4 == 0 and (tile == 0 or tile >= min(MIN_TILE, -(-n_max // 4) * 4))
                assert lds_layout(n_floats, n_max, lanes=lanes).bytes + STATIC_LDS <= LDS
    assert lds_layout(8, 1024, lanes=16).tile == 0 and lds_layout(8, 1024, lanes=64).tile > 0  # (about 9 KiB are left there)
    assert rule_edges(3, 1024) == [16, 17, 72, 73, 256, 257]
    assert rule_edges(5, 1024) == [16, 17, 56, 57, 224, 225]


# ---- parameter validation ------------------------------------------------------------------------------------------
def test_whole_step_lanes_is_validated():
    """0, 1, 4, 16 and 64 are taken, anything else is refused with -3 and leaves the setting as it was (the bits
    cannot show which lanes ran, the launches counted can show that the calls still run whole)."""
    with Ensemble("relu", 2, 10) as ens:
        ens.set_param("whole_steps", 1)
        for good in (0, 1, 4, 16, 64):
            assert ens.set_param("whole_step_lanes", good) == 0
        ens.set_param("whole_step_lanes", 16)
        for bad in (-1, 2, 8, 32, 128, 1.5):
            with pytest.raises(YallaError, match="-3"):
                ens.set_param("whole_step_lanes", bad)
        ens.h_X[:] = seeded_rows(3, 20, 1).reshape(2, 10, 3)
        ens.copy_to_device()
        ens.take_step(DT, 2)
        assert ens.whole_step_launches == 1
        with Ensemble("relu", 2, 10) as six:
            six.h_X[:] = seeded_rows(3, 20, 1).reshape(2, 10, 3)
            six.copy_to_device()
            six.take_step(DT, 2)
            assert six.whole_step_launches == 0
            six.copy_to_host()
            ens.copy_to_host()
            assert np.array_equal(bits(six.h_X), bits(ens.h_X))


# ---- ragged counts -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_reference(model, case):
    """RAGGED in one ensemble of n_max = 1024, stepped ONCE per model and case by the paths that are not under test
    (Twins: one lane per cell whole, the six launches, the lone Solutions, checked against each other): the rows it
    started from and the bits every lanes setting has to reproduce."""
    steps = 1 if case == "1 step" else 5
    run = Twins(model, RAGGED, 1024, seed=3)
    try:
        start = run.ens.h_X.copy()
        v0 = None
        if "old_v" in case:
            v0 = (np.random.default_rng(9).random((len(RAGGED), 1024, 3)) * 0.2 - 0.1).astype(np.float32)
            run.set_old_v(v0)
        run.step(DT, steps)
        run.expect_launches(1)
        run.check(case)
        singles = {r: (bits(s.positions()).copy(), bits(s.old_v()).copy()) for r, s in run.single.items()}
        return start, v0, bits(run.six.h_X).copy(), bits(run.six.old_v()).copy(), singles
    finally:
        run.close()


@pytest.mark.parametrize("case", ["1 step", "5 steps from a non-zero old_v"])
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("model", WHOLE)
def test_ragged_counts_bit_for_bit(model, lanes, case):
    """`oscillator` is not declared stateless and its functor reads (local) ids: the lanes are forced on it."""
    start, v0, six_X, six_v, singles = ragged_reference(model, case)
    steps = 1 if case == "1 step" else 5
    with Ensemble(model, len(RAGGED), 1024) as ens:
        assert ens.n_floats == N_FLOATS[model] and lds_layout(ens.n_floats, 1024, lanes=lanes).tile >= MIN_TILE
        ens.set_param("whole_steps", 1)
        ens.set_param("whole_step_lanes", lanes)
        ens.h_X[:] = start
        ens.h_n[:] = RAGGED
        ens.copy_to_device()
        if v0 is not None:
            ens.set_old_v(v0)
        ens.take_step(DT, steps)
        assert ens.whole_step_launches == 1
        ens.copy_to_host()
        v = bits(ens.old_v())
        # the six-launch twin: every row, used or not (unused rows still hold their pattern)
        assert list(ens.h_n) == RAGGED
        assert np.array_equal(bits(ens.h_X), six_X), (model, lanes, "positions")
        assert np.array_equal(v, six_v), (model, lanes, "old_v")
        unused = np.arange(1024)[None, :] >= np.asarray(RAGGED)[:, None]
        assert np.all(ens.h_X[unused] == np.float32(-7.25))
        if v0 is not None:
            assert np.array_equal(v[unused], bits(v0)[unused])
        for r, n in enumerate(RAGGED):  # the lone Solutions
            assert np.array_equal(bits(ens.h_X[r, :n]), singles[r][0]), (model, lanes, "positions of replica", r)
            assert np.array_equal(v[r, :n], singles[r][1][:n]), (model, lanes, "old_v of replica", r)


def test_push_still_falls_back():
    """Generic forces: no whole-step launch whatever the lanes, and the bits of the lone Solutions."""
    run = Twins("push", [0, 1, 2, 17, 64, 257], 300, seed=6)
    try:
        run.ens.set_param("whole_step_lanes", 16)
        run.step(DT, 3)
        run.expect_launches(0)
        run.check()
    finally:
        run.close()


# ---- small capacities: the LDS layout and the tile length come from n_max ----------------------------------------------
SMALL = [1, 3, 5, 16, 17, 64, 100, 300]


def small_capacities(model):
    return sorted(set(SMALL) | set(n for n in rule_edges(N_FLOATS[model], 300)))


@pytest.mark.parametrize("model, n_max", [(m, n) for m in ("relu", "relu_po") for n in small_capacities(m)])
def test_small_capacities(model, n_max):
    """A full replica, one a cell short and a lone cell, 5 steps with every setting in turn on one object.  The
    capacities are the issue's and those either side of every point below 300 cells where another term of the tile
    rule starts to decide (rule_edges)."""
    run = Twins(model, [n_max, n_max - 1, 1], n_max, seed=n_max)
    try:
        for lanes in (0, 4, 16, 64):
            run.ens.set_param("whole_step_lanes", lanes)
            run.step(DT, 5)
            run.expect_launches(1, lanes)
            run.check(f"lanes {lanes}")
    finally:
        run.close()


# ---- fixed modes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["clipped", "relu_po"])
def test_all_three_fixed_modes(model):
    run = Twins(model, [2, 17, 257], 257, seed=8)
    try:
        run.ens.set_param("whole_step_lanes", 16)
        for what, change, steps in [("set_fixed()", None, 2),
                                    ("set_fixed(1)", lambda s: s.set_fixed(1), 3),
                                    ("set_fixed_xy(0)", lambda s: s.set_fixed_xy(0), 3),
                                    ("set_fixed() after xy", lambda s: s.set_fixed(), 2)]:
            if change:
                run.each(change)
            run.step(DT, steps)
            run.expect_launches(1, what)
            run.check(what)
    finally:
        run.close()


# ---- settings changed between calls --------------------------------------------------------------------------------
def test_settings_changed_between_calls():
    """One object: lanes 1 -> 64 -> 4 -> 0, a 7-step request split by steps_per_launch 3 and 1, whole_steps to -1 and
    back, tile_lanes changed in between -- every call in lock-step with the six-launch twin and the lone Solutions."""
    run = Twins("relu", [200, 64, 0, 257, 31, 3], 300, seed=11)
    try:
        for what, settings, steps, launches in [
                ("lanes 1", {"whole_step_lanes": 1}, 2, 1),
                ("lanes 64, 3 steps per launch", {"whole_step_lanes": 64, "steps_per_launch": 3}, 7, 3),
                ("lanes 4, 1 step per launch", {"whole_step_lanes": 4, "steps_per_launch": 1, "tile_lanes": 16}, 7, 7),
                ("six launches", {"whole_steps": -1, "tile_lanes": 64}, 2, 0),
                ("lanes 0", {"whole_steps": 1, "whole_step_lanes": 0, "steps_per_launch": 256, "tile_lanes": 1}, 3, 1),
                ("lanes 16 again", {"whole_step_lanes": 16, "tile_lanes": 0}, 2, 1)]:
            for name, value in settings.items():
                run.ens.set_param(name, value)
            run.step(DT, steps)
            run.expect_launches(launches, what)
            run.check(what)
    finally:
        run.close()


# ---- many replicas -------------------------------------------------------------------------------------------------
def many(X, counts, lanes, whole, overwrite=None):
    with Ensemble("clipped", len(counts), X.shape[1]) as ens:
        ens.set_param("whole_steps", whole)
        ens.set_param("whole_step_lanes", lanes)
        ens.h_X[:] = X
        ens.h_n[:] = counts
        ens.copy_to_device()
        ens.take_step(DT, 1)
        if overwrite is not None:
            r, rows = overwrite
            ens.copy_to_host()
            ens.h_X[r, :len(rows)] = rows
            ens.copy_to_device()
        ens.take_step(DT, 2)
        assert ens.whole_step_launches == (2 if whole == 1 else 0)
        ens.copy_to_host()
        return bits(ens.h_X).copy(), bits(ens.old_v()).copy()


def test_more_replicas_than_resident_workgroups():
    """5000 replicas of up to 16 cells with 16 lanes per cell: every replica against whole_steps = -1; one replica's
    rows overwritten between calls change no bit of any other replica."""
    m, n_max, victim = 5000, 16, 2500
    rng = np.random.default_rng(23)
    counts = rng.integers(0, n_max + 1, size=m)
    counts[[0, 1, victim, m - 1]] = [16, 15, 16, 16]
    X = (rng.random((m, n_max, 3)) * 2).astype(np.float32)
    whole = many(X, counts, 16, 1)
    six = many(X, counts, 1, -1)
    assert np.array_equal(whole[0], six[0]) and np.array_equal(whole[1], six[1])
    unused = np.arange(n_max)[None, :] >= counts[:, None]
    assert np.array_equal(whole[0][unused], bits(X)[unused])
    changed = many(X, counts, 16, 1, overwrite=(victim, (rng.random((n_max, 3)) * 3).astype(np.float32)))
    others = np.arange(m) != victim
    assert np.array_equal(changed[0][others], whole[0][others]) and np.array_equal(changed[1][others], whole[1][others])
    assert not np.array_equal(changed[0][victim], whole[0][victim])


# ---- the CPU restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [4, 64])
@pytest.mark.parametrize("model", ["springs", "relu_po", "oscillator"])
def test_against_the_cpu_restatement(oracle, model, lanes):
    """Against `<model>_tile` of the CPU build of the model harness (read-only use of the fixture), with the device's
    reduction order: the one comparison that does not pass through the device functions the kernels share."""
    counts = [257, 64, 0, 800, 1, 5]
    with Ensemble(model, len(counts), 800) as ens:
        ens.set_param("whole_steps", 1)
        ens.set_param("whole_step_lanes", lanes)
        for r, n in enumerate(counts):
            ens.h_X[r, :n] = seeded_rows(ens.n_floats, n, 60 + r)
            ens.h_n[r] = n
        ens.copy_to_device()
        ens.take_step(DT, 3)
        assert ens.whole_step_launches == 1
        ens.copy_to_host()
        v = ens.old_v()
        for r, n in enumerate(counts):
            with Solution(model + "_tile", 800, lib=oracle) as s:
                assert s.set_reduce_order(1) == 0
                s.h_X[:n] = seeded_rows(ens.n_floats, n, 60 + r)
                s.h_n = n
                s.copy_to_device()
                s.take_step(DT, 3)
                assert np.array_equal(bits(s.positions()), bits(ens.h_X[r, :n])), r
                assert np.array_equal(bits(s.old_v()[:n]), bits(v[r, :n])), r
