"""Carried calls against one-step calls of the same library, shared by tests/test_bin_in_update_gpu.py (the exact
tier) and tests/test_fast_tier_carry_gpu.py (libyalla_models_fast.so).

`take_step(dt, k)` keeps the cells cube-sorted from step to step (include/solvers.cuh, Heun_solver::take_steps);
k calls of `take_step(dt, 1)` never enter that path and are the reference.  Compared are the bit patterns of X,
old_v, the count and the four public grid arrays (`snapshot`, `same`).  `tier` names the library: "exact" is the
default one, "fast" the fast-arithmetic tier; every helper that creates a system takes it, and it is part of the key
under which `single_steps` shares a reference run.
"""
import functools

import numpy as np

from yalla_amd import _ffi
from yalla_amd.solution import Solution

GS = 16
SPHERE = (0.5, 42)
GRID_KEYS = ("cube_id", "point_id", "cube_start", "cube_end")
TIERS = {"exact": 0, "fast": 1}  # tier -> ya_models_arith()


def lib_of(tier):
    lib = _ffi.device_lib(tier)
    assert lib.ya_models_arith() == TIERS[tier] and lib.ya_models_is_device() == 1
    return lib


def snapshot(s):
    X = s.positions()  # (copy_to_host: h_n becomes the device's count)
    n = s.get_d_n()
    cube_id, point_id, cube_start, cube_end = s.grid()
    return {"X": X, "old_v": s.old_v()[:n].copy(), "n": n, "cube_id": cube_id[:n].copy(),
            "point_id": point_id[:n].copy(), "cube_start": cube_start, "cube_end": cube_end}


def same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if key == "n":
            assert a[key] == b[key], key
        else:
            assert a[key].shape == b[key].shape, key
            assert np.array_equal(np.ascontiguousarray(a[key]).view(np.uint32),
                                  np.ascontiguousarray(b[key]).view(np.uint32)), key


def advance(model, n, calls, dt, *, n_max=None, gs=GS, params=(), sphere=SPHERE, between=None, tier="exact",
            seen=None):
    """The system after take_step(dt, c) for every c of `calls` (between(s) in between two of them): a snapshot after
    every call, the counters, and the positions it started from.  seen: a dict that gets the further counters
    (graph_launches) of the system at its end."""
    snaps = []
    with Solution(model, n_max or n, gs, 1.0, lib=lib_of(tier)) as s:
        for name, value in params:
            s.set_param(name, value)
        s.h_n = n
        s.random_sphere(*sphere)
        first = s.h_X[:n].copy()
        for i, c in enumerate(calls):
            if i and between:
                between(s)
            s.take_step(dt, c)
            snaps.append(snapshot(s))
        counters = {"carried": s.carried_steps(), "fused": s.fused_bin_rebuilds()}
        if seen is not None:
            seen.update(graph=s.graph_launches())
    return snaps, counters, first


@functools.lru_cache(maxsize=None)
def single_steps(model, n, n_max, steps, dt, params=(), gs=GS, sphere=SPHERE, tier="exact"):
    """Snapshots after each of `steps` one-step calls (the reference, shared by the cases that start alike)."""
    snaps, counters, first = advance(model, n, [1] * steps, dt, n_max=n_max, gs=gs, params=params, sphere=sphere,
                                     tier=tier)
    assert counters == {"carried": 0, "fused": 0}
    return snaps, first


def carried_and_fused(calls):
    carried = [c for c in calls if c >= 2]
    return {"carried": sum(c - 1 for c in carried), "fused": sum(2 * c - 1 for c in carried)}


def cube_changes(before, after):
    return int(np.any(np.floor(before[:, :3]) != np.floor(after[:, :3]), axis=1).sum())


class Before_call:
    """`between` of a run in single steps: `action` before the call-th call (0-based), nothing before the others."""

    def __init__(self, action, call):
        self.action, self.call, self.seen = action, call, 0

    def __call__(self, s):
        self.seen += 1
        if self.seen == self.call:
            self.action(s)
