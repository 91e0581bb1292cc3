"""Every force-kernel choice of the fast-arithmetic tier (libyalla_models_fast.so: contracted multiply-adds, bare
v_sqrt_f32 / v_rcp_f32) against the statement of the operation in binary64, ONE force evaluation at a time.

The tier's other tests step whatever kernel the engine picks; the exact tier's tests of the kernel choices
(tests/test_friction_functors_gpu.py, test_force_hot_loops_gpu.py) say nothing about this build, a separate
compilation of every kernel.  Here, as test_fast_tier_graded_friction_against_the_statement_in_binary64 does: a
dt = 0 step with a drawn old_v and a lone cell held fixed leaves in old_v the stage's right-hand side, which is
compared with friction_statement.stage_rhs(..., real=numpy.float64): max |got - want| / max |want| <= REL_TOL, the
project's 1e-5 for the tier, EVERY cell counted -- fading_spring and the graded friction have no jump at the cut-off,
so a pair that one side counts and the other does not moves a sum by ~1e-7.

Two DIFFERENT force kernels need not give the same bits in this tier (grid_force_bits contracts `sum += f * v`, the
several-lane kernels add products that were rounded into LDS): whether they do is printed, not asserted.
"""
import numpy as np
import pytest

import friction_statement as fs
from test_fast_arith_gpu import REL_TOL
from test_fast_tier_kernels import grid_input, grid_statement, tile_input, tile_statement
from yalla_amd import _ffi
from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fast():
    lib = _ffi.device_lib("fast")
    assert lib.ya_models_arith() == 1 and lib.ya_models_is_device() == 1
    return lib


def right_hand_sides(lib, model, X, v, gs, params):
    """old_v after take_step(0) with the last cell fixed: ((dX - fix) + (dX - fix)) / 2 of one force evaluation."""
    n = len(X)
    with Solution(model, n, gs, 1.0, lib=lib) as s:
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        for name, value in params:
            s.set_param(name, value)       # (a refused value raises: no choice is silently another one)
        s.set_old_v(v)
        s.set_fixed(n - 1)
        s.take_step(0.0, 1)
        got = s.old_v()[:n].copy()
        assert np.array_equal(s.positions().view(np.uint32), X.view(np.uint32))  # dt = 0: nobody moved
    return got


def ratio_of(got, want):
    assert np.isfinite(got).all()
    scale = np.abs(want).max()
    assert scale > 0.1
    return float(np.abs(got.astype(np.float64) - want).max() / scale)


CHOICE = ("force_variant", "coop_lanes", "stage_v_max", "tail_tiles")
# name: (a value for each of CHOICE, further parameters)
GRID_KERNELS = {
    "bits_v_gathered": ((2, 0, 0, 0), ()),                       # grid_force_bits, old_v through 32-bit byte offsets
    "bits_v_in_lds": ((2, 0, 1 << 30, 0), ()),                   # ... old_v staged in LDS
    "bits_v_addresses64": ((2, 0, 0, 0), (("gather_offset_bits", 64),)),
    "coop_16": ((3, 16, 0, 0), ()),                              # grid_force_coop
    "coop_8": ((3, 8, 0, 0), ()),
    "coop_4": ((3, 4, 0, 0), ()),
    "direct": ((0, 0, 0, 0), ()),                                # grid_force_direct
    "grid_force": ((1, 0, 0, 0), ()),
}
HALF_TILES = {                                                   # by plane only
    "bits_last_2_tiles_halved": ((2, 0, 0, 2), ()),
    "bits_every_tile_halved_v_in_lds": ((2, 0, 1 << 30, 1 << 20), ()),
}


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("name", ["cloud", "dense"])
def test_grid_force_kernels_against_binary64(fast, name, sum_order):
    X, v, gs = grid_input(name)
    n = len(X)
    dX, sf = grid_statement(name, sum_order)
    want = fs.as_old_v_after_a_dt_0_step(dX, n - 1)
    kernels = dict(GRID_KERNELS, **(HALF_TILES if sum_order else {}))
    results, ratios = {}, {}
    for kernel, (choice, more) in kernels.items():
        params = (("sum_order", sum_order),) + tuple(zip(CHOICE, choice)) + more
        results[kernel] = right_hand_sides(fast, "friction_graded_fading_grid", X, v, gs, params)
        ratios[kernel] = ratio_of(results[kernel], want)
        print(f"fast tier, {name}, sum_order {sum_order}, {kernel}: worst |got - want| / max|want| = "
              f"{ratios[kernel]:.3g}")
    first = results["bits_v_gathered"]
    for kernel, got in results.items():
        differ = int((got.view(np.uint32) != first.view(np.uint32)).any(axis=1).sum())
        print(f"  {kernel} against bits_v_gathered: {differ} of {n} cells differ in some bit")
    assert max(ratios.values()) <= REL_TOL, ratios


@pytest.mark.parametrize("n", [301, 600])
def test_tile_force_kernels_against_binary64(fast, n):
    """tile_force (tile_lanes 1: one lane per cell, 256-point tiles) and tile_force_coop with 16 and 64 lanes (128- and
    512-partner tiles; 0 is the engine's choice from the declaration): fading_spring on friction_on_background, all
    pairs."""
    X = tile_input(n)
    want = fs.as_old_v_after_a_dt_0_step(tile_statement(n), n - 1)
    results, ratios = {}, {}
    for lanes in (1, 0, 16, 64):
        results[lanes] = right_hand_sides(fast, "fading_tile", X, np.zeros((n, 3), np.float32), 50,
                                          (("tile_lanes", lanes),))
        ratios[lanes] = ratio_of(results[lanes], want)
        print(f"fast tier, fading_tile, n {n}, tile_lanes {lanes}: worst |got - want| / max|want| = "
              f"{ratios[lanes]:.3g}")
    for lanes in (0, 16, 64):
        differ = int((results[lanes].view(np.uint32) != results[1].view(np.uint32)).any(axis=1).sum())
        print(f"  tile_lanes {lanes} against 1: {differ} of {n} cells differ in some bit")
    assert max(ratios.values()) <= REL_TOL, ratios
