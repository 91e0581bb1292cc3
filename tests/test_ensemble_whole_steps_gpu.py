"""Whole Heun steps of small all-pairs replicas in one launch (ya::ens::whole_steps, include/ensemble.cuh): one
workgroup per replica runs the steps from LDS.  set_param("whole_steps", 1) asks for it; the result must be the bits
of the six-launch step.  THE REFERENCES are the existing paths -- the same Ensemble with whole_steps = -1, a lone
Solution("<model>_tile") per replica, and the CPU restatement (the one comparison that does not pass through the
device functions the kernels share) -- and every comparison is of bit patterns (uint32, array_equal): no tolerance
anywhere.  Every case says which path it expects and checks `whole_step_launches` for it."""
import numpy as np
import pytest
from ensemble_support import DT, WHOLE, Twins, bits, capacity, launches_of, seeded_rows

from yalla_amd.ensemble import Ensemble, GridEnsemble, YallaError
from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu

# a lone cell, partial wavefronts, 1 / 2 / 3 / 4 cells per thread, B_r = 1 ... 4 partial-sum blocks, both sides of
# every boundary
COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024]


@pytest.mark.parametrize("case", ["1 step", "5 steps", "5 steps from a non-zero old_v"])
@pytest.mark.parametrize("model", WHOLE + ["push"])
def test_ragged_counts_bit_for_bit(model, case):
    """Every count of COUNTS in one ensemble of n_max = 1024 (the capacity of every point type here).  From step 2
    on stage 2 averages non-zero neighbour velocities.  `push` has generic forces: the fallback, and still right."""
    steps = 1 if case == "1 step" else 5
    run = Twins(model, COUNTS, 1024, seed=3)
    try:
        assert capacity(run.ens.n_floats) == 1024
        if "old_v" in case:
            rng = np.random.default_rng(9)
            v = (rng.random((len(COUNTS), 1024, 3)) * 0.2 - 0.1).astype(np.float32)
            run.set_old_v(v)
        run.step(DT, steps)
        run.expect_launches(launches_of(model, steps))
        run.check(case)
        if "old_v" in case:  # rows >= n_r and the empty replica: old_v untouched as well
            unused = np.arange(1024)[None, :] >= np.asarray(COUNTS)[:, None]
            assert np.array_equal(bits(run.ens.old_v())[unused], bits(v)[unused])
        unused = np.arange(1024)[None, :] >= np.asarray(COUNTS)[:, None]
        assert np.all(run.ens.h_X[unused] == np.float32(-7.25))
    finally:
        run.close()


@pytest.mark.parametrize("model", ["clipped", "relu_po", "push"])
def test_all_three_fixed_modes(model):
    """The sequence of test_ensemble_gpu.test_all_three_fixed_modes: set_fixed(i), set_fixed_xy(i) (x and y held in
    the first stage only, the whole point in the second), and back to set_fixed() with the xy mode's first stage still
    in force."""
    run = Twins(model, [300, 70, 0, 64, 257, 5], 300)
    try:
        for what, change, steps in [("set_fixed()", None, 2),
                                    ("set_fixed(4)", lambda s: s.set_fixed(4), 3),
                                    ("set_fixed_xy(2)", lambda s: s.set_fixed_xy(2), 3),
                                    ("set_fixed(1) after xy", lambda s: s.set_fixed(1), 2),
                                    ("set_fixed() after xy", lambda s: s.set_fixed(), 2)]:
            if change:
                run.each(change)
            run.step(DT, steps)
            run.expect_launches(launches_of(model, steps), what)
            run.check(what)
    finally:
        run.close()


def test_set_fixed_xy_from_a_fresh_object():
    run = Twins("springs", [129, 3, 800], 800)
    try:
        run.each(lambda s: s.set_fixed_xy(0))
        run.step(DT, 4)
        run.expect_launches(1)
        run.check()
    finally:
        run.close()


@pytest.mark.parametrize("steps_per_launch, launches", [(3, 3), (1, 7), (7, 1), (256, 1)])
def test_a_long_request_is_split_into_launches(steps_per_launch, launches):
    """7 steps with at most 3 per launch are three launches (3 + 3 + 1), with 1 per launch seven: the bits of seven
    single steps of the six-launch ensemble and of the lone Solutions."""
    run = Twins("relu", [257, 0, 64, 600, 1], 600, seed=2)
    try:
        run.ens.set_param("steps_per_launch", steps_per_launch)
        run.ens.take_step(DT, 7)
        for _ in range(7):
            run.six.take_step(DT, 1)
            for s in run.single.values():
                s.take_step(DT, 1)
        run.expect_launches(launches)
        run.check()
    finally:
        run.close()


@pytest.mark.parametrize("model", ["relu", "relu_po", "oscillator"])
def test_at_the_capacity_and_one_row_beyond(model):
    """n_max equal to the point type's capacity runs whole (full replicas: 4 cells per thread, and with 5 floats per
    point 97 KiB of dynamic LDS, beyond the 64 KiB a kernel gets unasked); n_max one row larger is not eligible: the
    six launches run, the counter stays, the bits are those of whole_steps = -1 and of the lone Solutions."""
    n_floats = {"relu": 3, "relu_po": 5, "oscillator": 4}[model]
    cap = capacity(n_floats)
    run = Twins(model, [cap, cap - 1, 300], cap, seed=5)
    try:
        assert run.ens.n_floats == n_floats
        run.step(DT, 2)
        run.expect_launches(1)
        run.check("capacity")
    finally:
        run.close()
    run = Twins(model, [cap + 1, cap, 300], cap + 1, seed=5)
    try:
        run.step(DT, 2)
        run.expect_launches(0)
        run.check("capacity + 1")
    finally:
        run.close()


def test_more_replicas_than_resident_workgroups():
    """5000 replicas of up to 100 cells, 2 steps: every replica against whole_steps = -1, eight against lone
    Solutions."""
    m, n_max = 5000, 100
    sampled = [0, 1, 255, 256, 2047, 2048, 4098, 4999]
    rng = np.random.default_rng(21)
    counts = rng.integers(0, n_max + 1, size=m)
    counts[sampled] = [100, 99, 100, 1, 64, 65, 37, 100]
    X = (rng.random((m, n_max, 3)) * 4).astype(np.float32)
    results = {}
    for whole in (1, -1):
        with Ensemble("clipped", m, n_max) as ens:
            ens.set_param("whole_steps", whole)
            ens.h_X[:] = X
            ens.h_n[:] = counts
            ens.copy_to_device()
            ens.take_step(DT, 2)
            assert ens.whole_step_launches == (1 if whole == 1 else 0)
            ens.copy_to_host()
            results[whole] = (bits(ens.h_X).copy(), bits(ens.old_v()).copy())
    assert np.array_equal(results[1][0], results[-1][0]) and np.array_equal(results[1][1], results[-1][1])
    unused = np.arange(n_max)[None, :] >= counts[:, None]
    assert np.array_equal(results[1][0][unused], bits(X)[unused])
    for r in sampled:
        n = int(counts[r])
        with Solution("clipped_tile", n_max) as s:
            s.h_X[:] = X[r]
            s.h_n = n
            s.copy_to_device()
            s.take_step(DT, 2)
            assert np.array_equal(bits(s.positions()), results[1][0][r, :n]), r
            assert np.array_equal(bits(s.old_v()[:n]), results[1][1][r, :n]), r


def stepped(rows, n_max, overwrite=None):
    with Ensemble("relu", len(rows), n_max) as ens:
        ens.set_param("whole_steps", 1)
        for r, X in enumerate(rows):
            ens.h_X[r, :len(X)] = X
            ens.h_n[r] = len(X)
        ens.copy_to_device()
        ens.take_step(DT, 1)
        if overwrite is not None:
            r, X = overwrite
            ens.copy_to_host()
            ens.h_X[r, :len(X)] = X
            ens.h_n[r] = len(X)
            ens.copy_to_device()
        ens.take_step(DT, 2)
        assert ens.whole_step_launches == 2
        ens.copy_to_host()
        v = ens.old_v()
        return [(bits(ens.h_X[r, :len(X)]).copy(), bits(v[r, :len(X)]).copy()) for r, X in enumerate(rows)]


def test_replicas_are_independent():
    sizes = [100, 257, 0, 64, 800, 33, 1]
    rows = [seeded_rows(3, n, 40 + r) for r, n in enumerate(sizes)]
    forward = stepped(rows, 800)
    backward = stepped(rows[::-1], 800)
    for (X, v), (Xb, vb) in zip(forward, backward[::-1]):
        assert np.array_equal(X, Xb) and np.array_equal(v, vb)
    # one replica's rows overwritten after the first step: every other replica's bits are untouched
    other = seeded_rows(3, sizes[4], 999) * np.float32(1.5)
    changed = stepped(rows, 800, overwrite=(4, other))
    for r in range(len(sizes)):
        same = np.array_equal(forward[r][0], changed[r][0]) and np.array_equal(forward[r][1], changed[r][1])
        assert same == (r != 4), r


def test_settings_changed_between_calls():
    """dt changed, counts changed on the host (a replica emptied, one back from empty, one filled), a fresh old_v,
    whole_steps toggled 1 -> -1 -> 1 on one object: in lock-step with the lone Solutions and the six-launch ensemble
    throughout."""
    counts = [200, 64, 0, 257, 31, 500]
    run = Twins("clipped", counts, 600)
    rng = np.random.default_rng(5)
    try:
        run.step(DT, 2)
        run.expect_launches(1, "start")
        run.check("start")
        run.set_counts({0: 260, 1: 17, 2: 40, 3: 0, 5: 600})
        run.step(0.02, 2)
        run.expect_launches(1, "counts changed, dt 0.02")
        run.check("counts changed, dt 0.02")
        run.ens.set_param("whole_steps", -1)
        run.set_old_v((rng.random((len(counts), 600, 3)) * 0.2 - 0.1).astype(np.float32))
        run.step(0.1, 2)
        run.expect_launches(0, "whole_steps -1")
        run.check("whole_steps -1, fresh old_v, dt 0.1")
        run.ens.set_param("whole_steps", 1)
        run.set_counts({3: 300, 0: 64})
        run.each(lambda s: s.set_fixed(3))
        run.step(DT, 3)
        run.expect_launches(1, "whole_steps 1 again")
        run.check("whole_steps 1 again, set_fixed(3), a replica back from empty")
    finally:
        run.close()


def test_the_engines_choice_gives_the_same_bits():
    """whole_steps = 0 leaves the path to ya::ens::whole_steps_pay: either way the bits are the lone Solutions'."""
    run = Twins("fading", [100, 0, 37, 64], 100, seed=4)
    try:
        run.ens.set_param("whole_steps", 0)
        run.step(DT, 3)
        assert run.ens.whole_step_launches in (0, 1)
        run.check()
    finally:
        run.close()


def test_settings_are_validated():
    with Ensemble("relu", 2, 10) as ens:
        for name, bad in [("whole_steps", 2), ("whole_steps", -2), ("whole_steps", 0.5), ("steps_per_launch", 0),
                          ("steps_per_launch", -1), ("steps_per_launch", 1.5)]:
            with pytest.raises(YallaError, match="-3"):
                ens.set_param(name, bad)
        for name, good in [("whole_steps", -1), ("whole_steps", 0), ("whole_steps", 1), ("steps_per_launch", 1)]:
            assert ens.set_param(name, good) == 0
    with GridEnsemble("relu", 2, 10, 8, 1.0) as grid:  # a grid ensemble knows neither
        for name in ("whole_steps", "steps_per_launch"):
            with pytest.raises(YallaError, match="-2"):
                grid.set_param(name, 1)
        with pytest.raises(AttributeError):
            grid.whole_step_launches


@pytest.mark.parametrize("model", ["springs", "relu_po", "oscillator"])
def test_against_the_cpu_restatement(oracle, model):
    """Replicas stepped whole against `<model>_tile` of the CPU build of the model harness (read-only use of the
    fixture), with the device's reduction order: the one comparison that does not pass through the shared device
    functions.  oscillator's functor reads i and j, so a wrong id offset shows there."""
    counts = [257, 64, 0, 800, 1]
    with Ensemble(model, len(counts), 800) as ens:
        ens.set_param("whole_steps", 1)
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
