"""Gabriel_solver on the device (ya::gabriel_force and, for cells with more candidates than its LDS list
holds, ya::gabriel_force_dense) held bit for bit against the CPU restatement, the numpy statement
(gabriel_statement.py) and the kept A/B baseline gabriel_force_direct (force_variant 0)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gabriel_statement as gab  # noqa: E402
from test_gabriel import hexagon, lattice, random_260, run, same_bits, sphere, wall_system, with_lone_cell  # noqa: E402

from yalla_amd.solution import Solution  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.mark.parametrize("model", ["relu_gabriel", "clipped_gabriel"])
@pytest.mark.parametrize("case", ["hexagon", "lattice", "random_260", "sphere_5000", "sphere_100000"])
def test_device_is_the_oracle(device, oracle, model, case):
    if case.startswith("sphere"):
        X, gs = sphere(int(case.split("_")[1]), oracle)
    else:
        X, gs = {"hexagon": hexagon, "lattice": lattice, "random_260": random_260}[case]()
    steps = 20 if len(X) <= 5001 else 2
    for coefficient in (0.5, 0.8, 1.0) if len(X) <= 5001 else (0.8,):
        Xo, vo = run(oracle, model, X, gs, coefficient, steps=steps, dt=0.05)
        Xd, vd = run(device, model, X, gs, coefficient, steps=steps, dt=0.05)
        assert np.abs(Xo - X).max() > 0, (coefficient, "nothing moved")
        assert same_bits(Xd, Xo), coefficient
        assert same_bits(vd, vo), coefficient


def test_device_is_the_baseline_kernel_at_a_million_cells(device):
    """One step each of ya::gabriel_force and gabriel_force_direct on the same 10^6-cell random_sphere(0.75)
    (at most ~20 candidates per cell: the baseline's 100-entry list is safe here)."""
    n = 1_000_000
    out = []
    for variant in (-1, 0):
        with Solution("relu_gabriel", n, 100, 1.0, lib=device) as s:
            s.random_sphere(0.75, 11)
            if variant == 0:
                s.set_param("force_variant", 0)
            s.take_step(0.05, 1)
            out.append((s.positions().copy(), s.old_v()[:n].copy()))
    assert np.abs(out[0][1]).max() > 0
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])


def dense_system():
    """600 cells in a cube of side 0.9: every cell has ~600 candidates (> 300), more than the LDS list holds."""
    rng = np.random.default_rng(17)
    X = (rng.random((600, 3)) * 0.9 - 0.45).astype(f32)
    return with_lone_cell(X, (3.5, 3.5, 3.5)), 10


def test_dense_cells_take_the_workspace_path(device):
    """Device against the statement where every cell has more than 300 candidates (never run on the baseline
    kernel: it overflows its 100-entry list)."""
    X, gs = dense_system()
    ids, _ = gab.candidates(X, gs)
    assert (ids[:-1] >= 0).sum(axis=1).min() > 300
    for model in ("relu_gabriel", "clipped_gabriel"):
        _, F = run(device, model, X, gs, 0.8)
        want = gab.forces(X, gs, 0.8, model)
        assert np.abs(want).max() > 0.1
        assert same_bits(F, want), model


def test_mixed_dense_and_sparse_cells(device, oracle):
    """A dense cluster inside a sparse system: both kernels in one launch sequence, whole steps."""
    Xd, _ = dense_system()
    rng = np.random.default_rng(4)
    Xs = (rng.random((2000, 3)) * 12 - 6).astype(f32)
    X = with_lone_cell(np.vstack([Xd[:-1], Xs]), (9.5, 9.5, 9.5))
    Xo, vo = run(oracle, "relu_gabriel", X, 24, None, steps=3, dt=0.01)
    Xg, vg = run(device, "relu_gabriel", X, 24, None, steps=3, dt=0.01)
    assert same_bits(Xg, Xo) and same_bits(vg, vo)


def test_changing_the_coefficient_takes_effect(device, oracle):
    """3 identical steps, then gabriel_coefficient 0.5: the next steps follow it (no stale step replayed)."""
    X, gs = random_260()
    res = []
    for lib in (oracle, device):
        n = len(X)
        with Solution("relu_gabriel", n, gs, 1.0, lib=lib) as s:
            s.h_X[:n] = X
            s.h_n = n
            s.copy_to_device()
            s.set_fixed(n - 1)
            s.take_step(0.05, 3)
            before = s.positions().copy()
            s.set_param("gabriel_coefficient", 0.5)
            s.take_step(0.05, 2)
            res.append((before, s.positions().copy(), s.old_v()[:n].copy()))
    (bo, Xo, vo), (bd, Xd, vd) = res
    assert same_bits(bo, bd) and same_bits(Xo, Xd) and same_bits(vo, vd)
    Xk, _ = run(oracle, "relu_gabriel", X, gs, None, steps=5, dt=0.05)
    assert not same_bits(Xk, Xo)                              # the change is visible


def test_wall_model_on_the_device(device, oracle):
    """dt = 0 step: every cell bit for bit with the statement; the wall node's atomic sum within 1e-6."""
    X, gs = wall_system(oracle)
    _, F = run(device, "wall_gabriel", X, gs)
    want = gab.forces(X, gs, 0.8, "wall_gabriel")
    assert same_bits(F[1:], want[1:])
    assert F[0, 2] != 0 and np.allclose(F[0], want[0], rtol=1e-6, atol=0)


def test_fast_tier_runs_the_gabriel_models(oracle):
    """libyalla_models_fast.so has the models too (held to running: a fast sqrt may flip a decision on the
    sphere's boundary)."""
    from yalla_amd import _ffi
    X, gs = random_260()
    for model in ("relu_gabriel", "clipped_gabriel"):
        Xf, vf = run(_ffi.device_lib("fast"), model, X, gs, None, steps=2, dt=0.05)
        assert np.isfinite(Xf).all() and np.abs(Xf - X).max() > 0
