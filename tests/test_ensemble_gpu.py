"""Ensemble (yalla_amd/ensemble.py over include/ensemble.cuh): M all-pairs systems stepped by one launch
sequence.  THE REFERENCE of every comparison is the existing single-system path -- a Solution("<model>_tile",
n_max) per replica given the same rows, the same old_v and the same settings -- and every comparison is of bit
patterns (uint32, array_equal): no tolerance anywhere."""
import functools

import numpy as np
import pytest
from ensemble_support import DT, bits, seeded_rows
from ensemble_support import Lockstep as AnyLockstep

from yalla_amd.ensemble import Ensemble, models
from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu

MODELS = ["springs", "clipped", "fading", "relu", "relu_po", "oscillator", "push"]
# a partial wavefront, exactly one tile of 64 / 256, more than one tile, B_r = 1, 2, 4, 6 partial-sum blocks
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 800, 1500]
# An Ensemble and one Solution("<model>_tile", n_max) per replica: (model, counts, n_max, seed=0, singles=None).  A
# check compares h_n, get_d_n, positions and old_v[:n].
Lockstep = functools.partial(AnyLockstep, Ensemble, "_tile")


def counts_for(m):
    """Ragged counts out of SIZES: 800 for a lone replica, every size once M >= 10."""
    return [SIZES[(3 * r + 8) % len(SIZES)] for r in range(m)]


def test_the_models_are_those_of_the_tile_harness():
    from yalla_amd import models as tile_models
    from ensemble_support import FRICTION_MODELS
    assert models() == MODELS + FRICTION_MODELS
    assert all(m + "_tile" in tile_models() for m in MODELS + FRICTION_MODELS)


@pytest.mark.parametrize("m", [1, 3, 64, 257])
@pytest.mark.parametrize("model", MODELS)
def test_every_replica_is_its_single_system_bit_for_bit(model, m):
    """Ragged counts (an empty replica, a lone cell, partial wavefronts and tiles, 1 to 6 partial-sum blocks), 4
    steps from rows that differ per replica, so that stage 2 averages non-zero neighbour velocities."""
    counts = counts_for(m)
    run = Lockstep(model, counts, 1500, seed=m)
    try:
        run.step(DT, 4)
        run.check()
        assert m == 1 or len({c for c in counts}) >= min(m, 3)
    finally:
        run.close()


@pytest.mark.parametrize("model", ["clipped", "relu_po", "push"])
def test_all_three_fixed_modes(model):
    """set_fixed(i), set_fixed_xy(i) followed by steps (the second stage then holds the whole point), and back to
    set_fixed() -- which Heun_solver leaves with the xy mode's first stage still in force."""
    counts = [300, 70, 0, 64, 257, 5]
    run = Lockstep(model, counts, 300)
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


def test_set_fixed_xy_from_a_fresh_object():
    run = Lockstep("springs", [129, 3, 800], 800)
    try:
        run.each(lambda s: s.set_fixed_xy(0))
        run.step(DT, 4)
        run.check()
    finally:
        run.close()


@pytest.mark.parametrize("model", ["relu", "relu_po", "oscillator", "push"])
def test_any_number_of_lanes_gives_the_same_bits(model):
    counts = counts_for(12)
    results = []
    for lanes in (0, 1, 16, 64):
        with Ensemble(model, len(counts), 1500) as ens:
            ens.set_param("tile_lanes", lanes)
            for r, n in enumerate(counts):
                ens.h_X[r, :n] = seeded_rows(ens.n_floats, n, r)
                ens.h_n[r] = n
            ens.copy_to_device()
            ens.take_step(DT, 3)
            ens.copy_to_host()
            results.append((bits(ens.h_X).copy(), bits(ens.old_v()).copy()))
    for X, v in results[1:]:
        assert np.array_equal(X, results[0][0]) and np.array_equal(v, results[0][1])
    # ... and they are the single systems' bits (lanes 64, the last one, in lock-step once more)
    run = Lockstep(model, counts, 1500)
    try:
        run.ens.set_param("tile_lanes", 64)  # (Lockstep's rows with seed 0 are seeded_rows(.., n, r) as above)
        run.step(DT, 3)
        run.check()
        assert np.array_equal(bits(run.ens.h_X), results[0][0])
    finally:
        run.close()


@pytest.mark.parametrize("model", ["clipped", "push"])
def test_settings_changed_between_steps(model):
    """h_n[r] up and down, a fresh old_v, dt changed, the fixed mode changed, lanes changed: both sides in lock-step."""
    counts = [200, 64, 0, 257, 31, 500]
    run = Lockstep(model, counts, 600)
    rng = np.random.default_rng(5)
    try:
        run.step(DT, 2)
        run.check("start")
        run.set_counts({0: 260, 1: 17, 2: 40, 3: 0, 5: 600})
        run.step(DT, 2)
        run.check("counts changed")
        run.set_old_v((rng.random((len(counts), 600, 3)) * 0.2 - 0.1).astype(np.float32))
        run.step(0.02, 1)
        run.check("fresh old_v, dt 0.02")
        run.each(lambda s: s.set_fixed(3))
        run.ens.set_param("tile_lanes", 16)
        run.step(0.1, 2)
        run.check("set_fixed(3), dt 0.1")
        run.set_counts({3: 300, 0: 64})
        run.each(lambda s: s.set_fixed_xy(1))
        run.ens.set_param("tile_lanes", 1)
        run.step(DT, 2)
        run.check("set_fixed_xy(1), a replica back from empty")
        run.each(lambda s: s.set_fixed())
        run.step(0.03, 3)
        run.check("set_fixed() again")
    finally:
        run.close()


def stepped(model, rows, n_max, steps=3, overwrite=None):
    with Ensemble(model, len(rows), n_max) as ens:
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
        ens.take_step(DT, steps - 1)
        ens.copy_to_host()
        v = ens.old_v()
        return [(bits(ens.h_X[r, :len(X)]).copy(), bits(v[r, :len(X)]).copy()) for r, X in enumerate(rows)]


def test_replicas_are_independent():
    sizes = [100, 257, 0, 64, 800, 33, 1]
    rows = [seeded_rows(3, n, 40 + r) for r, n in enumerate(sizes)]
    forward = stepped("relu", rows, 800)
    backward = stepped("relu", rows[::-1], 800)
    for (X, v), (Xb, vb) in zip(forward, backward[::-1]):
        assert np.array_equal(X, Xb) and np.array_equal(v, vb)
    # one replica's rows overwritten after the first step: every other replica's bits are untouched
    other = seeded_rows(3, sizes[4], 999) * np.float32(1.5)
    changed = stepped("relu", rows, 800, overwrite=(4, other))
    for r in range(len(sizes)):
        same = np.array_equal(forward[r][0], changed[r][0]) and np.array_equal(forward[r][1], changed[r][1])
        assert same == (r != 4), r


def test_more_replicas_than_a_grid_has_rows():
    """M = 70 000 replicas of up to 16 cells (gridDim.y ends at 65 535) against a handful run singly."""
    m, n_max = 70000, 16
    sampled = [0, 1, 4097, 65535, 65536, 69999]
    rng = np.random.default_rng(11)
    counts = rng.integers(0, n_max + 1, size=m)
    counts[sampled] = [16, 9, 16, 13, 16, 7]
    X = (rng.random((m, n_max, 3)) * 2).astype(np.float32)
    with Ensemble("clipped", m, n_max) as ens:
        ens.h_X[:] = X
        ens.h_n[:] = counts
        ens.copy_to_device()
        ens.take_step(DT, 4)
        ens.copy_to_host()
        v = ens.old_v()
        for r in sampled:
            n = int(counts[r])
            with Solution("clipped_tile", n_max) as s:
                s.h_X[:] = X[r]
                s.h_n = n
                s.copy_to_device()
                s.take_step(DT, 4)
                assert np.array_equal(bits(s.positions()), bits(ens.h_X[r, :n])), r
                assert np.array_equal(bits(s.old_v()[:n]), bits(v[r, :n])), r
        # rows past a replica's count are nobody's: left as they were
        unused = np.arange(n_max)[None, :] >= counts[:, None]
        assert np.array_equal(bits(ens.h_X)[unused], bits(X)[unused])


def test_generic_forces():
    """`push` against `push_tile`: the generic force called once on the flat arrays, the right-hand sides zeroed
    by the update kernels in between (and by a memset first), steps with changing counts in between."""
    counts = [2, 700, 0, 1, 64, 300]
    run = Lockstep("push", counts, 700)
    try:
        run.step(DT, 5)
        run.check()
        moved = run.ens.h_X[1, 1, 0] - seeded_rows(3, 700, 1)[1, 0]
        assert moved != 0  # (the push is felt)
        run.set_counts({0: 300, 1: 2})
        run.step(DT, 3)
        run.check("counts changed")
    finally:
        run.close()


# The single-system kernels and the ensemble's share their loop bodies (ya::tile_force_rows,
# ya::tile_force_coop_rows, ya::fold256, ya::heun_row), so "replica == lone Solution" cannot see a mistake made in
# a shared body: this is the ensemble's one comparison that does not pass through them.  800 rows cross a tile
# boundary with a ragged last tile in every instance (tile_force: tiles of 256; the coop kernels: 64 or 384
# partners for relu_po's 5 floats, 64 or 448 for oscillator's 4), which also runs the scalar tail of the
# sixteen-term sums; oscillator's functor reads i and j, so a wrong id offset shows there.
@pytest.mark.parametrize("model, tile_lanes", [("springs", 0), ("relu_po", 1), ("relu_po", 16), ("relu_po", 64),
                                               ("oscillator", 16), ("oscillator", 64)])
def test_against_the_cpu_restatement(oracle, model, tile_lanes):
    """Direct comparisons with the CPU build of the model harness (read-only use of the fixture): replicas
    against `<model>_tile` there, with the device's reduction order, bit for bit."""
    counts = [257, 64, 0, 800, 1]
    with Ensemble(model, len(counts), 800) as ens:
        ens.set_param("tile_lanes", tile_lanes)
        for r, n in enumerate(counts):
            ens.h_X[r, :n] = seeded_rows(ens.n_floats, n, 60 + r)
            ens.h_n[r] = n
        ens.copy_to_device()
        ens.take_step(DT, 3)
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
