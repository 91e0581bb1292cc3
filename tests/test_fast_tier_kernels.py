"""The inputs of tests/test_fast_tier_kernels_gpu.py and what they must contain for a wrong kernel to show, checked
on the host: the binary64 statement of one force evaluation (tests/friction_statement.py) and the layout of
grid_force_bits' candidate streams (tests/test_force_hot_loops_gpu.py, bit_streams).  No GPU.

Input 1 is the cloud of test_fast_tier_graded_friction_against_the_statement_in_binary64 (301 cells, grid 50); input 2
is the dense block of the hot-loop tests (a 2 x 2 x 2 block of cubes with 50 .. 130 cells each, grid 8) plus one cell
in the grid's corner cube with no partner inside the cut-off, which is held fixed.
"""
import functools

import numpy as np

import friction_statement as fs
from test_force_hot_loops_gpu import CAP, GS as DENSE_GS, PASS_BITS, TILE, bit_streams, overflow_case

f32 = np.float32
CLOUD_N, CLOUD_GS = 301, 50
LONE_AT = 3.9       # the corner cube [3, 4)^3; the hot-loop cases fill [-3, 3)^3 only
COOP_MAX_HITS = 96  # ya::coop::MAX_HITS (include/solvers.cuh): longer hit lists are worked off in parts


@functools.lru_cache(maxsize=None)
def grid_input(name):
    """(X, old_v, grid size), read-only; the last cell is the lone one."""
    if name == "cloud":
        X, gs = fs.cloud(CLOUD_N, 3, 23), CLOUD_GS
    else:
        X, gs = np.vstack([overflow_case(), np.full((1, 3), LONE_AT, f32)]).astype(f32), DENSE_GS
    v = fs.velocities(len(X), 24)
    X.setflags(write=False)
    v.setflags(write=False)
    return X, v, gs


@functools.lru_cache(maxsize=None)
def grid_statement(name, sum_order):
    """friction_graded_fading_grid's right-hand sides in binary64, and their divisors; computed once, read-only."""
    X, v, gs = grid_input(name)
    dX, sf, _ = fs.stage_rhs(X, v, fs.fading_spring, fs.graded, "grid", gs, 1.0, bool(sum_order), real=np.float64)
    dX.setflags(write=False)
    sf.setflags(write=False)
    return dX, sf


@functools.lru_cache(maxsize=None)
def tile_input(n):
    X = fs.cloud(n, 3, 25)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def tile_statement(n):
    """fading_tile's right-hand sides in binary64 (friction_on_background: the force alone)."""
    X = tile_input(n)
    dX, sf, _ = fs.stage_rhs(X, np.zeros((n, 3), f32), fs.fading_spring, fs.friction_on_background, "tile",
                             real=np.float64)
    assert (sf == 0).all()
    dX.setflags(write=False)
    return dX


def hits_in_binary64(X):
    """How many OTHER cells each cell has inside the cut-off."""
    P = X.astype(np.float64)
    d = P[:, None, :] - P[None, :, :]
    return ((d * d).sum(axis=2) < 1.0).sum(axis=1) - 1


def test_dense_block_has_the_shapes_it_is_for():
    X, _, gs = grid_input("dense")
    n = len(X)
    assert gs == 8 and n <= 2601 and n % TILE != 0 and (n - 1) % TILE != 0
    assert float(np.abs(X).max()) < gs // 2                       # nobody outside the grid
    lanes = bit_streams(X)
    assert any(fallback and len(bits) == PASS_BITS for _, bits, fallback, _ in lanes)  # > 128 candidate bits a plane
    assert any(total > CAP for _, _, _, total in lanes)                                # > 352 staged cells a plane
    hits = hits_in_binary64(X)
    print("hits per cell: max", int(hits.max()), " cells above", COOP_MAX_HITS, ":", int((hits > COOP_MAX_HITS).sum()))
    assert hits.max() > COOP_MAX_HITS                             # grid_force_coop's list worked off in parts
    assert hits[-1] == 0                                          # the fixed cell is alone


def test_cloud_has_a_lone_last_cell_and_a_ragged_last_tile():
    X, _, _ = grid_input("cloud")
    assert len(X) % TILE != 0 and hits_in_binary64(X)[-1] == 0


def test_grid_statements_are_finite_and_every_cell_has_friction():
    for name in ("cloud", "dense"):
        for sum_order in (0, 1):
            dX, sf = grid_statement(name, sum_order)
            assert np.isfinite(dX).all() and np.isfinite(sf).all()
            assert sf.min() >= 0.25                               # the self term: no division near zero
            assert np.abs(dX).max() > 0.1 and not dX[-1].any()    # (the lone cell: 0 * 0.25 / 0.25)


def test_tile_statements_are_finite_and_cross_the_tiles():
    """301 and 600 cells: two and three of tile_force's 256-point tiles, three and five of tile_force_coop's
    128-partner tiles, one and two of its 512-partner tiles, each with a ragged last one."""
    for n in (301, 600):
        assert n % 256 and n % 128 and n % 512 and n % 64
        dX = tile_statement(n)
        assert np.isfinite(dX).all() and np.abs(dX).max() > 0.1 and not dX[-1].any()
        assert (hits_in_binary64(tile_input(n))[:-1] > 0).mean() > 0.9
