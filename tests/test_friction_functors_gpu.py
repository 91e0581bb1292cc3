"""User-written friction functors (yalla_amd/csrc/model_functors.h: graded, ids, field) through every force kernel of
the HIP engine, BIT FOR BIT against the CPU restatement -- which tests/test_friction_functors.py holds against the
numpy statement of the reference's loops.  Positions, old_v and, for grids, the four grid arrays after 3 Heun steps
from an old_v drawn at random.

The two default frictions return 0 or 1 and read their ids through `i == j` only, so the product friction * old_v was
exact and the ids' values never mattered.  Here the coefficients are fractional (the product is rounded: once into
the running sum in the one-lane bodies, once into LDS in the several-lane ones), signed (sum_friction is negative,
or zero made of non-zero terms, for several cells of every ids input: the `sum_friction > 0` guard), asymmetric in
(i, j) and changed by any id offset that is no multiple of 8 (original id against sorted position, global against
local ids in ensembles), and they read theta of r and phi of Xi.  A name listed under YA_STATELESS_FRICTION and
its `_plain` twin reach the several-lane and the one-lane bodies with the same arithmetic.

Where the engine has a counter (whole_step_launches, lds_step_launches, dense_cells, graph_launches, carried_steps)
the case asserts through it that the intended path ran."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import friction_statement as fs  # noqa: E402
import gabriel_statement as gab  # noqa: E402
from ensemble_support import Lockstep, bits, compare  # noqa: E402
from test_friction_functors import COEFFICIENT, assert_field_pairs_on_both_sides, assert_ids_sums_have_every_sign  # noqa: E402

from yalla_amd import _ffi  # noqa: E402
from yalla_amd.ensemble import Ensemble, GabrielEnsemble, GridEnsemble  # noqa: E402
from yalla_amd.solution import Solution  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
STEPS = 3
DT = 0.02
WIDTH = {"graded": 3, "ids": 3, "field": 5}
SPACING = {"ids": 1.0}          # (ids: negative sums need cells with few neighbours, test_friction_functors.py)
FORCE = {"friction_graded_fading_grid": fs.fading_spring}


def functor_of(model):
    return model.split("_")[1]


def declared(model):
    """The model whose numbers a `_plain` twin has (the oracle's run is shared)."""
    return model.replace("_plain", "")


def rows_of(functor, n, seed=21):
    return fs.cloud(n, WIDTH[functor], seed, SPACING.get(functor, 0.75), lone=False)


def some_old_v(n, seed=22):
    return (fs.velocities(n, seed, lone=False) * f32(0.1)).astype(f32)


def same(a, b, what=""):
    for key in a:
        if key == "grid":
            for x, y in zip(a[key], b[key]):
                assert np.array_equal(x, y), (what, "grid arrays")
        else:
            assert np.array_equal(a[key], b[key]), (what, key, int((a[key] != b[key]).any(axis=1).sum()), "cells differ")


def run(lib, model, X, v, calls=(STEPS,), dt=DT, params=(), gs=50, cube_size=1.0, sum_order=0, counters=None):
    """take_step(dt, c) for every c of `calls` from rows X and old_v v, the centre of mass held (the default; the
    oracle sums it in the engine's tree order): bits of the positions and old_v, and a grid solver's arrays."""
    n = len(X)
    with Solution(model, n, gs, cube_size, lib=lib) as s:
        s.set_reduce_order(1)
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        if sum_order:
            s.set_param("sum_order", sum_order)
        if model.endswith("_gabriel"):
            s.set_param("gabriel_coefficient", COEFFICIENT)
        if lib.ya_models_is_device():
            for name, value in params:
                s.set_param(name, value)
        s.set_old_v(v)
        for c in calls:
            s.take_step(dt, c)
        out = {"X": bits(s.positions()).copy(), "v": bits(s.old_v()[:n]).copy()}
        if not model.endswith("_tile"):
            out["grid"] = s.grid()
        if counters is not None:
            counters.update(carried=s.carried_steps(), graph=s.graph_launches())
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(model, n, steps=STEPS, dt=DT, gs=50, cube_size=1.0, sum_order=0):
    """The CPU restatement's result, computed once per input (the tests share it and leave it unchanged)."""
    lib = _ffi.bind(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_build",
                                 "liboracle_models.so"))
    X = rows_of(functor_of(model), n)
    out = run(lib, model, X, some_old_v(n), (steps,), dt, gs=gs, cube_size=cube_size, sum_order=sum_order)
    P = out["X"].view(f32)
    assert np.isfinite(P).all() and np.abs(P[:, :3]).max() < gs // 2 - 1      # nothing left the grid
    if n > 1:
        assert not np.array_equal(out["X"], bits(X))
    return out


def check_inputs(model, n, cube_size=1.0, by_plane=False):
    """From the statement alone: what the input must contain for a wrong kernel to show."""
    functor = functor_of(model)
    X = rows_of(functor, n)
    if functor == "ids":
        solver = "tile" if model.endswith("_tile") else "grid"
        _, sf, terms = fs.stage_rhs(X, some_old_v(n), FORCE.get(model, fs.relu_force), fs.ids, solver, 50, cube_size, by_plane)
        assert_ids_sums_have_every_sign(sf, terms)
    if functor == "field":
        assert_field_pairs_on_both_sides(np.vstack([X, X[-1:]]))   # (that helper leaves a last, lone row out)


# ---- Tile_solver -----------------------------------------------------------------------------------------------------
TILE_MODELS = {"graded": ["friction_graded_tile"], "ids": ["friction_ids_tile", "friction_ids_plain_tile"],
               "field": ["friction_field_tile", "friction_field_plain_tile"]}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("functor", list(TILE_MODELS))
def test_tile_solver(oracle, device, functor, n):
    """ya::tile_force (one lane per cell: the running sum in tile_pair) and ya::tile_force_coop with 16 and 64 lanes
    (the products rounded into LDS, added in the one-lane order), the declared name and its plain twin; lanes 0 is
    the engine's choice from the declaration."""
    if n == 257:
        check_inputs(TILE_MODELS[functor][0], n)
    want = oracle_run(TILE_MODELS[functor][0], n)
    for model in TILE_MODELS[functor]:
        for lanes in (1, 16, 64, 0):
            got = run(device, model, rows_of(functor, n), some_old_v(n), params=[("tile_lanes", lanes)])
            same(got, want, (model, "tile_lanes", lanes))


# ---- Grid_solver -----------------------------------------------------------------------------------------------------
# (force_variant, coop_lanes, stage_v_max, tail_tiles): the engine's choice; grid_force_direct and grid_force (the A/B
# baselines); grid_force_bits with old_v from global memory and from LDS; grid_force_coop with 16, 8 and 4 lanes
KERNELS = [(-1, 0, 0, 0), (0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (2, 0, 1 << 30, 0), (3, 16, 0, 0), (3, 8, 0, 0),
           (3, 4, 0, 0)]
# by plane only: grid_force_bits with its last 2 tiles, and with every tile, as half tiles that meet through memory
HALF_TILES = [(2, 0, 0, 2), (2, 0, 1 << 30, 1 << 20)]
GRID_MODELS = ["friction_ids_grid", "friction_ids_plain_grid", "friction_field_grid", "friction_graded_fading_grid"]


def kernel_params(kernel):
    return list(zip(("force_variant", "coop_lanes", "stage_v_max", "tail_tiles"), kernel))


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("n", [301, 2003])
@pytest.mark.parametrize("model", GRID_MODELS)
def test_grid_solver_every_force_kernel(oracle, device, model, n, sum_order):
    """Every force_variant the harness accepts, in both summation orders; 5 and 32 tiles of 64 cells."""
    if n == 301:
        check_inputs(declared(model), n, by_plane=bool(sum_order))
    want = oracle_run(declared(model), n, sum_order=sum_order)
    for kernel in KERNELS + (HALF_TILES if sum_order else []):
        got = run(device, model, rows_of(functor_of(model), n), some_old_v(n), params=kernel_params(kernel),
                  sum_order=sum_order)
        same(got, want, (model, kernel))


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("model", ["friction_ids_grid", "friction_ids_plain_grid", "friction_field_grid"])
def test_grid_solver_with_cubes_wider_than_the_friction(oracle, device, model, sum_order):
    """cube_size 1.5: pairs inside a cube's reach that the friction's own `dist < 1` refuses."""
    n = 301
    check_inputs(declared(model), n, cube_size=1.5, by_plane=bool(sum_order))
    want = oracle_run(declared(model), n, cube_size=1.5, sum_order=sum_order)
    for kernel in KERNELS + (HALF_TILES if sum_order else []):
        got = run(device, model, rows_of(functor_of(model), n), some_old_v(n), params=kernel_params(kernel),
                  cube_size=1.5, sum_order=sum_order)
        same(got, want, (model, kernel))


@pytest.mark.parametrize("model", ["friction_ids_grid", "friction_ids_plain_grid", "friction_field_grid"])
def test_grid_solver_carried_steps_and_graph_replay(oracle, device, model):
    """take_step(dt, k), which keeps the cells cube-sorted from step to step (the functor must still get the original
    ids), against k single steps and the oracle; and captured steps replayed (more steps than it takes to capture)."""
    n, k = 2003, 6
    want = oracle_run(declared(model), n, steps=k)
    X, v = rows_of(functor_of(model), n), some_old_v(n)
    seen = {}
    same(run(device, model, X, v, [1] * k, counters=seen), want, "single steps")
    assert seen["carried"] == 0
    same(run(device, model, X, v, [k], counters=seen), want, "one call")
    assert seen["carried"] == k - 1
    same(run(device, model, X, v, [1] * k, params=[("graph", 1)], counters=seen), want, "graph, single steps")
    assert seen["graph"] >= k - 2 and seen["carried"] == 0
    same(run(device, model, X, v, [k], params=[("graph", 1)], counters=seen), want, "graph, one call")
    assert seen["graph"] >= k - 2 and seen["carried"] == 0       # (captured steps are not carried: the plain loop)


# ---- Gabriel_solver --------------------------------------------------------------------------------------------------
GABRIEL_MODELS = ["friction_graded_gabriel", "friction_ids_gabriel", "friction_ids_plain_gabriel", "friction_field_gabriel"]


@pytest.mark.parametrize("model", GABRIEL_MODELS)
def test_gabriel_solver_list_kernel(oracle, device, model):
    """At most 64 candidates per cell: the declared names' terms are evaluated by the lanes and summed from LDS, the
    plain twin goes through gabriel::test_and_sum."""
    n = 301
    X = rows_of(functor_of(model), n)
    assert (gab.candidates(np.ascontiguousarray(X[:, :3]), 50)[0] >= 0).sum(axis=1).max() <= 64
    for variant in (-1, 0):       # ya::gabriel_force; the kept baseline gabriel_force_direct (one thread, a private list)
        got = run(device, model, X, some_old_v(n), params=[("force_variant", variant)])
        same(got, oracle_run(declared(model), n), (model, "force_variant", variant))


def clump_rows(functor):
    """tests/test_gabriel.py's clusters up to 129 cells (every pair of a cluster closer than 1: 65, 66, 127, 128 and
    129 candidates reach the dense kernel), with the further fields of a wide point in [-2, 2)."""
    from test_gabriel import clusters
    X = np.asarray(clusters(129)[0], f32)
    extra = (np.random.default_rng(31).random((len(X), WIDTH[functor] - 3)) * 4 - 2).astype(f32)
    return np.hstack([X, extra])


@pytest.mark.parametrize("model", ["friction_ids_gabriel", "friction_ids_plain_gabriel", "friction_field_gabriel"])
def test_gabriel_solver_dense_kernel(oracle, device, model):
    X = clump_rows(functor_of(model))
    n = len(X)
    candidates = (gab.candidates(np.ascontiguousarray(X[:, :3]), 24)[0] >= 0).sum(axis=1)
    assert (candidates > 64).sum() >= 500 and (candidates <= 64).sum() >= 500      # dense cells exist, and others
    v = some_old_v(n)
    want = run(oracle, declared(model), X, v, dt=1e-4, gs=24)
    assert not np.array_equal(want["X"], bits(X))
    same(run(device, model, X, v, dt=1e-4, gs=24), want, model)


# ---- ensembles: every replica against a lone Solution of the same model ----------------------------------------------
COUNTS = [0, 1, 2, 37, 64, 65, 66]


def ensemble_rows(functor, counts, n_max, seed):
    return [rows_of(functor, min(n, n_max), seed + r) for r, n in enumerate(counts)]


def ensemble_old_v(m, n_max, seed=41):
    return (np.random.default_rng(seed).random((m, n_max, 3)) * 0.2 - 0.1).astype(f32)


def fresh(make, rows, n_max, v, params):
    ens = make()
    for name, value in params:
        ens.set_param(name, value)
    for r, X in enumerate(rows):
        ens.h_X[r, :len(X)] = X
        ens.h_n[r] = len(X)
    ens.copy_to_device()
    ens.set_old_v(v)
    return ens


@pytest.mark.parametrize("n_max", [100, 67])
@pytest.mark.parametrize("model", ["friction_ids", "friction_ids_plain", "friction_field"])
def test_all_pairs_ensemble(device, model, n_max):
    """Replica r's rows start at r * n_max, no multiple of 8 for r = 1: ids must reach the friction as local ids.  The
    six-launch step with 1, 16 and 64 lanes per cell, and whole-step launches with 1, 4, 16 and 64 (0: the engine's
    choice from the declaration) -- each against the lone Solutions."""
    functor = functor_of(model)
    counts = COUNTS + [n_max]
    rows = ensemble_rows(functor, counts, n_max, 50)
    v = ensemble_old_v(len(counts), n_max)
    if functor == "ids":
        _, sf, terms = fs.stage_rhs(rows[-1], v[-1, :n_max], fs.relu_force, fs.ids, "tile")
        assert (sf < 0).sum() >= 1 and ((sf == 0) & (terms > 0)).sum() >= 1 and (sf > 0).sum() >= 3
    run_ = Lockstep(Ensemble, "_tile", model, [len(X) for X in rows], n_max, rows=rows)
    try:
        run_.set_old_v(v)
        run_.step(DT, STEPS)
        reference = run_.results()
        run_.check("the harness's defaults", reference)
    finally:
        run_.close()
    paths = [({"whole_steps": -1, "tile_lanes": lanes}, False) for lanes in (1, 16, 64, 0)]
    paths += [({"whole_steps": 1, "whole_step_lanes": lanes}, True) for lanes in (1, 4, 16, 64, 0)]
    for params, whole in paths:
        ens = fresh(lambda: Ensemble(model, len(rows), n_max), rows, n_max, v, params.items())
        try:
            ens.take_step(DT, STEPS)
            assert (ens.whole_step_launches > 0) == whole, params
            compare(ens, [len(X) for X in rows], reference, (model, params))
        finally:
            ens.close()


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("n_max", [100, 67])
@pytest.mark.parametrize("model", ["friction_ids", "friction_ids_plain", "friction_field"])
def test_grid_ensemble(device, model, n_max, sum_order):
    """The 14-launch step with the engine's lanes and 1, 4, 8, 16 lanes per cell, and the launches that step from LDS
    (grid_lds_steps: the generic branch of pair_friction), with the grid arrays."""
    functor = functor_of(model)
    counts = COUNTS + [n_max]
    rows = ensemble_rows(functor, counts, n_max, 60)
    v = ensemble_old_v(len(counts), n_max)
    gs = 12
    run_ = Lockstep(GridEnsemble, "_grid", model, [len(X) for X in rows], n_max, (gs, 1.0), grids=True, rows=rows)
    try:
        run_.set_sum_order(sum_order)
        run_.set_old_v(v)
        run_.step(DT, STEPS)
        reference = run_.results()
        run_.check("the harness's defaults", reference)
        for r in range(len(rows)):
            assert run_.ens.status(r, clear=False) == 0
    finally:
        run_.close()
    paths = [({"lds_steps": -1, "lanes": lanes}, False) for lanes in (1, 4, 8, 16)]
    paths += [({"lds_steps": 1, "lanes": lanes}, True) for lanes in (0, 1, 4, 16)]
    for params, from_lds in paths:
        ens = fresh(lambda: GridEnsemble(model, len(rows), n_max, gs, 1.0), rows, n_max, v,
                    list(params.items()) + [("sum_order", sum_order)])
        try:
            ens.take_step(DT, STEPS)
            assert (ens.lds_step_launches > 0) == from_lds, params
            compare(ens, [len(X) for X in rows], reference, (model, params))
        finally:
            ens.close()


@pytest.mark.parametrize("model", ["friction_ids", "friction_ids_plain", "friction_field"])
def test_gabriel_ensemble_with_a_dense_replica(device, model):
    """A clump of 90 cells inside a ball of radius 0.45 (90 candidates each: the dense kernel) between sparse replicas,
    an empty one and a lone cell; n_max = 100."""
    functor = functor_of(model)
    n_max, gs = 100, 12
    rows = ensemble_rows(functor, [67, 90, 0, 1, 100], n_max, 70)
    rows[1][:, :3] *= f32(0.45 / np.linalg.norm(rows[1][:, :3], axis=1).max())
    candidates = (gab.candidates(np.ascontiguousarray(rows[1][:, :3]), gs)[0] >= 0).sum(axis=1)
    assert (candidates == 90).all()
    v = ensemble_old_v(len(rows), n_max)
    run_ = Lockstep(GabrielEnsemble, "_gabriel", model, [len(X) for X in rows], n_max, (gs, 1.0),
                    ens_args=(COEFFICIENT,), grids=True, rows=rows)
    try:
        for s in run_.single.values():
            s.set_param("gabriel_coefficient", COEFFICIENT)
        run_.set_old_v(v)
        run_.step(1e-3, STEPS)
        run_.check("3 steps")
        assert not np.array_equal(bits(run_.ens.h_X[1, :90]), bits(rows[1]))
        run_.step(0.0, 1)       # both stages see the positions the host reads: the clump is still one
        run_.check("and a dt = 0 step")
        now = [np.ascontiguousarray(run_.ens.h_X[r, :len(X), :3]) for r, X in enumerate(rows)]
        dense = [int(((gab.candidates(X, gs)[0] >= 0).sum(axis=1) > 64).sum()) if len(X) else 0 for X in now]
        assert dense[1] >= 64 and run_.ens.dense_cells() == sum(dense)
    finally:
        run_.close()


# ---- the fast-arithmetic tier ----------------------------------------------------------------------------------------
REL_TOL = 1e-5       # the project's bound for the fast tier (tests/test_fast_arith_gpu.py)


def test_fast_tier_graded_friction_in_lock_step(oracle):
    """libyalla_models_fast.so (contracted multiply-adds, bare v_sqrt_f32 / v_rcp_f32) in lock-step with the exact
    statement of the same model, as tests/test_fast_arith_gpu.py does: positions within 1e-5 of the cloud's size
    after every step, NO cell excluded -- neither fading_spring nor the graded friction jumps at the cut-off, and
    sum_friction >= 0.25 (the self term).  The ids friction is left out of this tier on purpose: its sums cross zero,
    where a last-bit difference of one term decides whether a cell gets any friction at all; field is left out
    because the tier has no force on Po_cell that fades at the cut-off (relu_force's jumps there)."""
    from test_fast_arith_gpu import lock_step
    fast = _ffi.device_lib("fast")
    assert fast.ya_models_arith() == 1
    worst = lock_step(oracle, fast, "friction_graded_fading_grid", 3000, 50, 0.6, 5, 0.1, 4, cut_off_pairs=0)
    print(f"fast tier, graded friction, lock-step: worst relative difference {worst:.3g}")
    assert worst <= REL_TOL


@pytest.mark.parametrize("sum_order", [0, 1])
def test_fast_tier_graded_friction_against_the_statement_in_binary64(sum_order):
    """One stage's right-hand side (a dt = 0 step, the lone last cell fixed, old_v drawn at random) against the
    statement evaluated in binary64: within 1e-5 of the largest right-hand side, every cell."""
    n = 301
    X, v = fs.cloud(n, 3, 23), fs.velocities(n, 24)
    want, sf, _ = fs.stage_rhs(X, v, fs.fading_spring, fs.graded, "grid", 50, 1.0, bool(sum_order), real=np.float64)
    assert sf.min() >= 0.25
    want = fs.as_old_v_after_a_dt_0_step(want, n - 1)
    with Solution("friction_graded_fading_grid", n, 50, 1.0, lib=_ffi.device_lib("fast")) as s:
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        s.set_param("sum_order", sum_order)
        s.set_old_v(v)
        s.set_fixed(n - 1)
        s.take_step(0.0, 1)
        got = s.old_v()[:n].astype(np.float64)
    scale = np.abs(want).max()
    assert scale > 0.1
    ratio = np.abs(got - want).max() / scale
    print(f"fast tier, graded friction, sum_order {sum_order}: worst |got - want| / max|want| = {ratio:.3g}")
    assert ratio <= REL_TOL
