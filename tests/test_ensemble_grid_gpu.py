"""GridEnsemble (yalla_amd/ensemble.py over include/ensemble_grid.cuh): M Grid_solver systems stepped by one launch
sequence.  THE REFERENCE of every comparison is the existing single-system path -- a Solution("<model>_grid", n_max,
grid_size, cube_size) per replica with all defaults, given the same rows, the same old_v and the same settings --
and every comparison is of bit patterns (uint32, array_equal): no tolerance anywhere, and positions, old_v AND the
four grid arrays of every compared replica are compared."""
import numpy as np
import pytest
from ensemble_support import DT, bits, compare, same_grid, seeded_rows
from ensemble_support import Lockstep as AnyLockstep

from yalla_amd.ensemble import GridEnsemble, grid_models
from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu

MODELS = ["springs", "clipped", "fading", "relu", "relu_po", "relu_cell", "push", "clipped_push"]
# partial and full tiles of 16, 32, 64 and 256 cells (the coop kernels' and the bit kernel's workgroups, the update
# kernels' blocks), an empty replica, a lone cell
SIZES = [0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 255, 256, 257, 800, 1500]
LANES = [0, 1, 4, 8, 16]


def counts_for(m):
    """Ragged counts out of SIZES: 800 for a lone replica; 800, 1500, 0 for three; every size from 15 replicas on."""
    return [SIZES[(r + 13) % len(SIZES)] for r in range(m)]


def Lockstep(model, counts, n_max, grid_size, cube_size=1.0, **kw):
    """A GridEnsemble and one Solution("<model>_grid", n_max, grid_size, cube_size) per replica; the four grid arrays
    are part of every result."""
    return AnyLockstep(GridEnsemble, "_grid", model, counts, n_max, (grid_size, cube_size), grids=True, **kw)


def stepped_ensemble(model, counts, n_max, grid_size, lanes, dt, steps, seed=0, rows=None, cube_size=1.0):
    """A fresh GridEnsemble with Lockstep's rows, `lanes` lanes per cell, stepped; the caller compares and closes."""
    ens = GridEnsemble(model, len(counts), n_max, grid_size, cube_size)
    ens.set_param("lanes", lanes)
    for r, n in enumerate(counts):
        ens.h_X[r, :n] = seeded_rows(ens.n_floats, n, 1000 * seed + r) if rows is None else rows[r]
        ens.h_n[r] = n
    ens.copy_to_device()
    ens.take_step(dt, steps)
    return ens


def against_singles(model, counts, n_max, grid_size, dt, steps, seed=0, rows=None, precondition=None):
    """The single systems once (with an ensemble of the engine's lanes in lock-step), then a fresh ensemble for
    each other number of lanes against the same reference."""
    run = Lockstep(model, counts, n_max, grid_size, seed=seed, rows=rows)
    try:
        run.step(dt, steps)
        reference = run.results()
        if precondition is not None:
            precondition(run, reference)
        run.check("lanes 0", reference)
    finally:
        run.close()
    for lanes in LANES[1:]:
        ens = stepped_ensemble(model, counts, n_max, grid_size, lanes, dt, steps, seed=seed, rows=rows)
        try:
            compare(ens, counts, reference, ("lanes", lanes, model))
        finally:
            ens.close()


def test_the_models_are_those_of_the_grid_harness():
    from yalla_amd import models as single_models
    from ensemble_support import FRICTION_MODELS
    assert grid_models() == MODELS + FRICTION_MODELS
    assert all(m + "_grid" in single_models() for m in MODELS + FRICTION_MODELS)


@pytest.mark.parametrize("m", [1, 3, 33])
@pytest.mark.parametrize("model", MODELS)
def test_every_replica_is_its_single_system_bit_for_bit(model, m):
    """Ragged counts (an empty replica, a lone cell, partial and full workgroups of every kernel), 4 steps from rows
    that differ per replica, with the engine's lanes and with 1, 4, 8 and 16 lanes per cell."""
    counts = counts_for(m)
    assert m < len(SIZES) or set(counts) == set(SIZES)
    against_singles(model, counts, 1500, 32, DT, 4, seed=m)


def box_rows(n, grid_size, seed):
    """Uniform over the WHOLE grid box [-gs/2, gs - gs/2) * 0.999 (gs/2 the integer the cube id uses)."""
    rng = np.random.default_rng(seed)
    lo = -(grid_size // 2)
    return ((lo + grid_size * rng.random((n, 3))) * 0.999).astype(np.float32)


@pytest.mark.parametrize("grid_size", [4, 5, 6])
@pytest.mark.parametrize("model", ["springs", "clipped"])
def test_grid_edges_do_not_leak_into_the_next_replica(model, grid_size):
    """Replicas that fill their whole grid, side by side: replica r's last plane of cubes and replica r + 1's first
    are both populated, and every stencil row that leaves the grid at a face must come back empty -- not with the
    neighbour replica's cells.  (springs and clipped: their clouds contract, so nothing leaves the box.)"""
    counts = [65, 130, 257, 300, 65, 130]
    # (seeds with which no cell is pushed out of its box in 4 steps, predictor positions included -- the
    # precondition asserted below; on the CPU oracle these rows keep 0.005 or more from every face)
    rows = [box_rows(n, grid_size, 1000 + 10 * grid_size + r) for r, n in enumerate(counts)]
    lo, hi = -(grid_size // 2), grid_size - grid_size // 2
    for X in rows:  # every replica starts with cells in its first and in its last plane of cubes
        assert X[:, 2].min() < lo + 1 and X[:, 2].max() >= hi - 1

    def inside(run, reference):
        for r, (X, _, _) in reference.items():
            P = X.view(np.float32)
            assert np.all(P > lo) and np.all(P < hi), ("a reference position left the box", r)
            assert run.ens.status(r, clear=False) == 0, r

    against_singles(model, counts, 300, grid_size, DT, 4, rows=rows, precondition=inside)


@pytest.mark.parametrize("model", ["springs", "relu_po"])
def test_a_dense_replica_among_sparse_ones(model):
    """300 cells inside a ball of radius 0.4: more than 128 candidates per plane (the bit kernel's stretches) and
    more than 96 hits per cell (coop's hit list in parts), between two sparse replicas."""
    counts = [40, 300, 40]
    n_floats = 5 if model == "relu_po" else 3
    dense = seeded_rows(n_floats, 300, 8)
    dense[:, :3] *= np.float32(0.4 / np.abs(np.linalg.norm(dense[:, :3], axis=1)).max())
    rows = [seeded_rows(n_floats, 40, 6), dense, seeded_rows(n_floats, 40, 7)]
    assert np.linalg.norm(dense[:, :3], axis=1).max() <= 0.4001
    against_singles(model, counts, 300, 8, 1e-4, 2, rows=rows)


@pytest.mark.parametrize("model", ["clipped", "relu_po", "push"])
def test_all_three_fixed_modes(model):
    """set_fixed(i), set_fixed_xy(i) followed by steps (the second stage then holds the whole point), and back to
    set_fixed() -- which Heun_solver leaves with the xy mode's first stage still in force."""
    counts = [300, 70, 0, 64, 257, 5]
    run = Lockstep(model, counts, 300, 16)
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


@pytest.mark.parametrize("model", ["clipped", "relu_po"])
def test_settings_changed_between_steps(model):
    """cube_size, sum_order both ways, lanes, counts up, down and back, a fresh old_v: one live ensemble and its
    singles in lock-step, a step after each change."""
    counts = [200, 64, 0, 257, 31, 500]
    run = Lockstep(model, counts, 600, 16)
    rng = np.random.default_rng(5)
    try:
        run.step(DT, 2)
        run.check("start")
        run.set_cube_size(1.25)
        run.step(DT, 1)
        run.check("cube_size 1.25")
        run.set_sum_order(1)
        run.ens.set_param("lanes", 4)
        run.step(DT, 2)
        run.check("sum_order by plane, 4 lanes")
        run.set_counts({0: 260, 1: 17, 2: 40, 3: 0, 5: 600})
        run.ens.set_param("lanes", 1)
        run.step(DT, 2)
        run.check("counts changed, by plane, 1 lane")
        run.set_sum_order(0)
        run.set_cube_size(0.8)
        run.ens.set_param("lanes", 16)
        run.step(DT, 1)
        run.check("the reference's order again, cube_size 0.8, 16 lanes")
        run.set_old_v((rng.random((len(counts), 600, 3)) * 0.2 - 0.1).astype(np.float32))
        run.ens.set_param("lanes", 8)
        run.step(0.02, 1)
        run.check("fresh old_v, dt 0.02, 8 lanes")
        run.set_counts({3: 300, 0: 64, 5: 500})
        run.set_cube_size(1.0)
        run.ens.set_param("lanes", 0)
        run.step(DT, 2)
        run.check("counts back, a replica back from empty, cube_size 1")
    finally:
        run.close()


def stepped(model, rows, n_max, grid_size, steps=3, overwrite=None):
    with GridEnsemble(model, len(rows), n_max, grid_size) as ens:
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
    forward = stepped("relu", rows, 800, 16)
    backward = stepped("relu", rows[::-1], 800, 16)
    for (X, v), (Xb, vb) in zip(forward, backward[::-1]):
        assert np.array_equal(X, Xb) and np.array_equal(v, vb)
    # one replica's rows overwritten after the first step: no bit of any other replica changes
    other = seeded_rows(3, sizes[4], 999) * np.float32(1.5)
    changed = stepped("relu", rows, 800, 16, overwrite=(4, other))
    for r in range(len(sizes)):
        same = np.array_equal(forward[r][0], changed[r][0]) and np.array_equal(forward[r][1], changed[r][1])
        assert same == (r != 4), r


def test_many_replicas():
    """M = 4000 replicas of up to 40 cells in 8^3 grids against six run singly, the first and the last among them."""
    m, n_max, grid_size = 4000, 40, 8
    sampled = [0, 1, 1023, 2048, 3998, 3999]
    rng = np.random.default_rng(11)
    counts = rng.integers(0, n_max + 1, size=m)
    counts[sampled] = [40, 9, 40, 13, 17, 33]
    X = (rng.random((m, n_max, 3)) * 2).astype(np.float32)
    with GridEnsemble("clipped", m, n_max, grid_size) as ens:
        ens.h_X[:] = X
        ens.h_n[:] = counts
        ens.copy_to_device()
        ens.take_step(DT, 4)
        ens.copy_to_host()
        v = ens.old_v()
        for r in sampled:
            n = int(counts[r])
            with Solution("clipped_grid", n_max, grid_size, 1.0) as s:
                s.h_X[:] = X[r]
                s.h_n = n
                s.copy_to_device()
                s.take_step(DT, 4)
                assert np.array_equal(bits(s.positions()), bits(ens.h_X[r, :n])), r
                assert np.array_equal(bits(s.old_v()[:n]), bits(v[r, :n])), r
                assert same_grid(ens.grid(r), s.grid(), n), r
        # rows past a replica's count are nobody's: left as they were
        unused = np.arange(n_max)[None, :] >= counts[:, None]
        assert np.array_equal(bits(ens.h_X)[unused], bits(X)[unused])


def test_a_replica_that_leaves_its_grid_is_reported_and_harms_nobody():
    counts = [100, 64, 257, 30]
    bad = 2
    rows = [seeded_rows(3, n, 90 + r) for r, n in enumerate(counts)]
    rows[bad][5] = (0.0, 0.0, 100.0)  # far above the 8^3 grid: its cube id is past the last cube's
    run = Lockstep("relu", counts, 300, 8, rows=rows, singles=[r for r in range(len(counts)) if r != bad])
    try:
        run.step(DT, 1)
        for r in range(len(counts)):
            assert (run.ens.status(r, clear=False) != 0) == (r == bad), r
        assert run.ens.status(bad, clear=True) != 0
        assert run.ens.status(bad, clear=False) == 0  # forgotten: copy_to_host will not abort
        run.check("beside a replica that left its grid")
    finally:
        run.close()


def test_generic_forces_with_a_pairwise_force():
    """`clipped_push` against `clipped_push_grid`: the generic force called once per stage on the flat arrays and
    the force kernel ADDING to what it left (has_gen).  Counts go down and up again in between: the rows a replica
    gives up and takes back hold the right-hand sides of earlier steps unless every row, used or not, is zeroed
    before the generic forces -- which the singles' comparison then shows."""
    counts = [2, 700, 0, 1, 64, 300]
    run = Lockstep("clipped_push", counts, 700, 24)
    try:
        run.step(DT, 3)
        run.check()
        moved = run.ens.h_X[1, 1, 0] - seeded_rows(3, 700, 1)[1, 0]
        assert moved != 0  # (the push is felt)
        run.set_counts({1: 10, 5: 1, 0: 300})
        run.step(DT, 2)
        run.check("counts down")
        run.set_counts({1: 650, 5: 280, 3: 90})
        run.step(DT, 3)
        run.check("counts up again")
    finally:
        run.close()
