"""The per-width code that libyalla_models.so's 3-, 5- and 7-float models never run, on the GPU: float4 (the one padded
entry) and MAKE_PT points of 4, 6, 8, 9, 11 and 16 floats through Grid_solver, Tile_solver and Gabriel_solver with
models::field_coupling, which reads and writes every field (yalla_amd/libyalla_models_widths.so against
oracle/_build/liboracle_models_widths.so; tests/test_point_widths.py holds that oracle to a numpy statement).

Every comparison is BIT FOR BIT (`view(np.uint32)`), over every field column of the positions, old_v and, for the
solvers with a grid, the four grid arrays; the oracle sums the centre of mass in the engine's tree order.  No tolerance.

What each type adds (include/solvers.cuh, yalla_amd/csrc/core.hip):

  type    entry  staged cells  staged_words    OWN_IN_LDS  grid SLOTS at 16 / 8 / 4 lanes  tile TILE at 16 / 64 lanes
  float4  32 B   256           one 16-byte     no          1 / 1 / 2                        64 / 448
  w4      20 B   352           three scalars   no          1 / 1 / 2                        (no tile model)
  w6      28 B   256           three scalars   yes         1 / 2 / 3                        64 / 320   (undeclared)
  w8      36 B   176           three scalars   yes         1 / 2 / 3                        (no tile model)
  w9      40 B   176           three scalars   yes         1 / 2 / 4                        (no tile model; undeclared)
  w11     48 B   176           one 16-byte     yes         1 / 2 / 4                        none / 192
  w16     68 B   176           three scalars   yes         2 / 3 / 5                        none / 128
"""
import numpy as np
import pytest

import widths_support as ws
from carry_support import same as same_snapshot
from carry_support import snapshot
from widths_support import widths_device, widths_oracle  # noqa: F401  (fixtures)
from yalla_amd.solution import Solution, YallaError

pytestmark = pytest.mark.gpu

_oracle_runs = {}


def oracle_run(lib, name, n, **kw):
    """An oracle run, made once for the cases that share it (the results are not written to)."""
    key = (name, n, tuple(sorted((k, v) for k, v in kw.items() if k != "setup")), kw.get("setup_key"))
    kw.pop("setup_key", None)
    if key not in _oracle_runs:
        _oracle_runs[key] = ws.run(lib, name, n, **kw)
    return _oracle_runs[key]


# ---- Grid_solver: sizes, densities, cube sizes -------------------------------------------------------------------------
GRID_CASES = {
    # n, random_sphere's distance, cube_size, dt
    "small": [(n, 0.5, 1.0, 0.05) for n in (1, 2, 63, 64, 65, 257)],
    "4000": [(4000, 0.5, 1.0, 0.05)],        # planes on both sides of the 176- and 256-cell capacities
    "dense": [(6000, 0.1, 1.0, 0.0005)],     # hundreds of cells per cube: every class chunks, rows beyond one pass
    "cube_2.5": [(3000, 0.5, 2.5, 0.05)],
}


@pytest.mark.parametrize("case", list(GRID_CASES))
@pytest.mark.parametrize("kind", ws.GRID_TYPES)
def test_grid_two_steps_against_the_oracle(widths_oracle, widths_device, kind, case):
    for n, dist, cs, dt in GRID_CASES[case]:
        kw = dict(dist=dist, cs=cs, dt=dt, steps=2)
        want = oracle_run(widths_oracle, ws.model(kind, "grid"), n, **kw)
        got = ws.run(widths_device, ws.model(kind, "grid"), n, **kw)
        ws.same(want, got, (kind, n))
        if n > 2:
            assert (np.abs(got["X"] - got["first"]).max(axis=0) > 0).all()     # every field has been stepped


# ---- Grid_solver: every kernel choice ----------------------------------------------------------------------------------
# (force_variant, coop_lanes, stage_v_max, tail_tiles, pass_facts, sorted_pipeline) under sum_order 0 and 1
BITS, COOP = 2, 3
CHOICES = [
    dict(force_variant=BITS),                                    # grid_force_bits, old_v from global memory ...
    dict(force_variant=BITS, stage_v_max=1 << 30),               # ... and staged in LDS
    dict(force_variant=BITS, pass_facts=0),                      # its generic bodies only
    dict(force_variant=BITS, pass_facts=1),
    dict(force_variant=BITS, sorted_pipeline=0),
    dict(force_variant=BITS, sorted_pipeline=1),
    dict(force_variant=BITS, sorted_pipeline=2),
    dict(force_variant=COOP, coop_lanes=16),                     # grid_force_coop
    dict(force_variant=COOP, coop_lanes=8),
    dict(force_variant=COOP, coop_lanes=4),
    dict(),                                                      # the engine's own choice
]
BY_PLANE_ONLY = [dict(force_variant=BITS, tail_tiles=-1), dict(force_variant=BITS, tail_tiles=0),
                 dict(force_variant=BITS, tail_tiles=1 << 20)]  # half tiles: chosen, none, every tile


def choose(s, choice, sum_order):
    assert s.set_param("sum_order", sum_order) == 0
    settings = dict(stage_v_max=0, tail_tiles=0) if choice else {}     # (nothing named: every default stays)
    settings.update(choice)
    for name, value in settings.items():
        assert s.set_param(name, value) == 0, name           # (also for the undeclared types: an explicit choice holds)


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("kind", ws.GRID_TYPES)
def test_grid_kernel_choices_agree(widths_oracle, widths_device, kind, sum_order):
    """4000 cells: grid_force_bits with old_v from global memory and from LDS, with and without its passes' facts,
    the three second-stage pipelines, grid_force_coop with 16, 8 and 4 lanes per cell and the engine's own choice --
    and, by plane, the tail of half tiles chosen, off and everywhere -- each against the oracle in the same order.
    For w9 and w6, whose functor is not declared stateless, the engine's own choice is the one-lane kernel; the
    several-lane kernels are taken when named, as for every undeclared functor, and give the same bits."""
    n = 4000
    name = ws.model(kind, "grid")
    order = lambda s: s.set_param("sum_order", sum_order)
    want = oracle_run(widths_oracle, name, n, dt=0.05, steps=2, setup=order, setup_key=("sum_order", sum_order))
    for choice in CHOICES + (BY_PLANE_ONLY if sum_order else []):
        got = ws.run(widths_device, name, n, dt=0.05, steps=2, setup=lambda s: choose(s, choice, sum_order))
        ws.same(want, got, (kind, sum_order, choice))


def test_the_two_orders_differ(widths_oracle):
    """(so that the cases under sum_order 1 are cases of their own)"""
    name = ws.model("w16", "grid")
    a = oracle_run(widths_oracle, name, 4000, dt=0.05, steps=2, setup=lambda s: s.set_param("sum_order", 0),
                   setup_key=("sum_order", 0))
    b = oracle_run(widths_oracle, name, 4000, dt=0.05, steps=2, setup=lambda s: s.set_param("sum_order", 1),
                   setup_key=("sum_order", 1))
    assert not np.array_equal(ws.bits(a["X"]), ws.bits(b["X"]))


# ---- Grid_solver: carried steps ----------------------------------------------------------------------------------------
def advance(lib, name, n, calls, dt, gs, params=()):
    """carry_support.advance for a library of one's own: a snapshot after every take_step(dt, c) and the counters."""
    snaps = []
    with Solution(name, n, gs, 1.0, lib=lib) as s:
        if lib.ya_models_is_device() == 0:
            assert s.set_reduce_order(1) == 0
        for key, value in params:
            assert s.set_param(key, value) == 0, key
        ws.start(s, n, 0.5, 42)
        for c in calls:
            s.take_step(dt, c)
            snaps.append(snapshot(s))
        return snaps, s.carried_steps(), s.fused_bin_rebuilds()


CARRY_SWITCHES = [(), (("carry_sorted", 0),), (("bin_in_update", 0),), (("trim_carried_stores", 0),)]


@pytest.mark.parametrize("kind", ws.GRID_TYPES)
def test_carried_steps_are_the_single_steps(widths_oracle, widths_device, kind):
    """take_step(dt, 6) keeps the cells cube-sorted from step to step -- the only way through the grid rebuild from
    entries (k_order_from<EW>), and through float4's id that is not the entry's last word -- against six one-step
    calls and the oracle, with carry_sorted, bin_in_update and trim_carried_stores each on (the default) and off."""
    n, k, dt, gs = 1500, 6, 0.05, 20
    name = ws.model(kind, "grid")
    ref, carried, fused = advance(widths_device, name, n, [1] * k, dt, gs)
    assert (carried, fused) == (0, 0)
    oracle, _, _ = advance(widths_oracle, name, n, [k], dt, gs)
    same_snapshot(ref[-1], oracle[-1])
    moved = int(np.any(np.floor(ref[-1]["X"][:, :3]) != np.floor(ref[0]["X"][:, :3]), axis=1).sum())
    assert moved > 20      # cells change cube on the way: a carried rebuild has something to re-sort
    for params in CARRY_SWITCHES:
        got, carried, fused = advance(widths_device, name, n, [k], dt, gs, params)
        on = dict(params).get("carry_sorted", 1) == 1
        assert carried == (k - 1 if on else 0), params
        assert carried > 0 or not on
        assert fused == (2 * k - 1 if on and dict(params).get("bin_in_update", 1) else 0), params
        same_snapshot(got[-1], ref[-1])


@pytest.mark.parametrize("kind", ["float4", "w9", "w16"])
def test_renumbered_steps(widths_oracle, widths_device, kind):
    """keep_in_cube_order(2): the cells are renumbered in cube order at every second step, every field with them."""
    n, dt, gs = 1500, 0.05, 20
    name = ws.model(kind, "grid")
    params = (("renumber_every", 2),)
    want, _, _ = advance(widths_oracle, name, n, [1] * 5, dt, gs, params)
    got, _, _ = advance(widths_device, name, n, [1] * 5, dt, gs, params)
    same_snapshot(got[-1], want[-1])
    plain, _, _ = advance(widths_oracle, name, n, [1] * 5, dt, gs)
    assert not np.array_equal(ws.bits(plain[-1]["X"]), ws.bits(want[-1]["X"]))     # (the ids did change)
    carried, count, _ = advance(widths_device, name, n, [5], dt, gs, params)
    same_snapshot(carried[-1], want[-1])


# ---- fixed points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["point", "xy"])
@pytest.mark.parametrize("kind,solver", [("w6", "grid"), ("w16", "grid"), ("w11", "tile")])
def test_fixed_points(widths_oracle, widths_device, kind, solver, mode):
    """set_fixed(i) and set_fixed_xy(i): the fixed cell's right-hand side travels behind the n_floats sums of the
    reduction's total (fix_from_total, heun_step)."""
    def setup(s):
        (s.set_fixed if mode == "point" else s.set_fixed_xy)(17)
    n = 500
    want = oracle_run(widths_oracle, ws.model(kind, solver), n, dist=0.6, dt=0.05, steps=3, setup=setup, setup_key=mode)
    got = ws.run(widths_device, ws.model(kind, solver), n, dist=0.6, dt=0.05, steps=3, setup=setup)
    ws.same(want, got, (kind, solver, mode))
    free = oracle_run(widths_oracle, ws.model(kind, solver), n, dist=0.6, dt=0.05, steps=3)
    assert not np.array_equal(ws.bits(free["X"]), ws.bits(want["X"]))
    if mode == "point":
        assert np.array_equal(ws.bits(got["X"][17, :3]), ws.bits(got["first"][17, :3]))


# ---- Tile_solver -------------------------------------------------------------------------------------------------------
# 64 m + 1 for m = 1 .. 8: one partner more than every size a tile of tile_force_coop can have
TILE_SIZES = [1, 2, 63, 64] + [64 * m + 1 for m in range(1, 9)] + [600]


@pytest.mark.parametrize("kind", ws.TILE_TYPES)
def test_tile_lanes_against_the_oracle(widths_oracle, widths_device, kind):
    """tile_force (one lane per cell) and tile_force_coop with 16 and 64 lanes per cell, and the solver's own choice.
    Points of 11 floats and more have no 16-lane kernel (64 partners' terms for 16 cells do not fit LDS):
    tile_lanes = 16 is refused for them, and the solver never picks it (test_wide_tile_models_above_4096_cells)."""
    name = ws.model(kind, "tile")
    has_16 = ws.WIDTH[kind] <= 10
    for n in TILE_SIZES:
        want = oracle_run(widths_oracle, name, n, dist=0.6, dt=0.05, steps=2)
        for lanes in (0, 1, 16, 64):
            def setup(s):
                s.set_param("tile_lanes", lanes)
            if lanes == 16 and not has_16:
                continue
            got = ws.run(widths_device, name, n, dist=0.6, dt=0.05, steps=2, setup=setup)
            ws.same(want, got, (kind, n, lanes))


@pytest.mark.parametrize("kind", ["w11", "w16"])
def test_sixteen_tile_lanes_are_refused_for_wide_points(widths_device, kind):
    with Solution(ws.model(kind, "tile"), 100, lib=widths_device) as s:
        ws.start(s, 100, 0.6, 7)
        with pytest.raises(YallaError):
            s.set_param("tile_lanes", 16)
        for lanes in (0, 1, 64):
            assert s.set_param("tile_lanes", lanes) == 0
        s.take_step(0.05, 1)      # (the refused value was not kept)
    with Solution(ws.model("w6", "tile"), 100, lib=widths_device) as s:
        assert s.set_param("tile_lanes", 16) == 0


@pytest.mark.parametrize("kind", ["w11", "w16"])
def test_wide_tile_models_above_4096_cells(widths_oracle, widths_device, kind):
    """Above 4096 cells the solver takes 16 lanes per cell for a stateless functor: for these types, which have no
    such kernel, it stays with 64."""
    n = 4100
    want = oracle_run(widths_oracle, ws.model(kind, "tile"), n, dist=0.6, dt=0.05, steps=1)
    got = ws.run(widths_device, ws.model(kind, "tile"), n, dist=0.6, dt=0.05, steps=1)
    ws.same(want, got, kind)


# ---- Gabriel_solver ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ws.GABRIEL_TYPES)
def test_gabriel_against_the_oracle(widths_oracle, widths_device, kind):
    """random_sphere(0.75) with 1, 2, 17 and 300 cells -- gabriel_force (w6, undeclared: its one-lane body) and the
    A/B baseline gabriel_force_direct -- and 600 cells in one cube, every one with more than 300 candidates (the
    dense kernel's lists in global memory)."""
    from test_gabriel_gpu import dense_system
    name = ws.model(kind, "gabriel")
    for n in (1, 2, 17, 300):
        want = oracle_run(widths_oracle, name, n, dist=0.75, gs=30, dt=0.05, steps=2)
        for variant in (-1, 0):
            got = ws.run(widths_device, name, n, dist=0.75, gs=30, dt=0.05, steps=2,
                         setup=lambda s: s.set_param("force_variant", variant))
            ws.same(want, got, (kind, n, variant))
    X, gs = dense_system()
    want = ws.run(widths_oracle, name, len(X), X=X, gs=gs, dt=0.0005, steps=2)
    got = ws.run(widths_device, name, len(X), X=X, gs=gs, dt=0.0005, steps=2)
    ws.same(want, got, (kind, "dense"))


# ---- no fallback -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,solver", [("w8", "grid"), ("w16", "tile")])
def test_device_kernels_really_ran(widths_device, kind, solver):
    """The force launches counted by the engine's own event profiler: 2 per take_step.  (Gabriel_computer's launches
    are not timed by it.)"""
    with Solution(ws.model(kind, solver), 2000, 50, 1.0, lib=widths_device) as s:
        assert widths_device.ya_models_is_device() == 1
        ws.start(s, 2000, 0.5, 1)
        s.profile(True)
        s.take_step(0.05, 3)
        ms, launches = s.profile_read()
        assert launches == 6 and ms > 0
