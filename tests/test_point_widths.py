"""Point widths beside 3, 5 and 7 floats -- float4 and MAKE_PT types of 4, 6, 8, 9, 11 and 16 floats -- on the host:

  * an INDEPENDENT numpy binary32 statement of models::field_coupling (yalla_amd/csrc/model_functors.h) and of whole
    Heun steps with it on Tile_solver and Grid_solver, written from the functor's definition and the reference's
    step (the contract of tests/test_reference_statement_numpy.py and tests/gabriel_statement.py), held BIT FOR BIT
    against the oracle for every model of the widths library: the functor's source is shared by the oracle and the
    engine, so without this it could be wrong in both at once;
  * what the shapes of tests/test_point_widths_gpu.py claim -- planes that are staged in chunks, rows beyond one pass
    of the bit stream -- computed from the oracle's grid arrays;
  * the start states' extra fields; and the compile-time refusal of a 17-float point.
"""
import os
import subprocess

import numpy as np
import pytest

import gabriel_statement as gab
import widths_support as ws
from test_reference_statement_numpy import tree_sum
from widths_support import widths_oracle  # noqa: F401  (fixture)
from yalla_amd.solution import Solution, models

f32 = np.float32
f64 = np.float64
ROOT = ws.ROOT
N, GS = 300, 30


# ---- the statement ---------------------------------------------------------------------------------------------------
def field_coupling(r, dist, i, j):
    """x, y, z: relu_force (inits.cuh:78-93: scalar binary32, a true division per component).  Field k >= 3:
    -c_k * r[k] with c_k = 0.0625 * (k - 2) where i != j and dist < 1, else 0."""
    width = r.shape[-1]
    F = (np.maximum(f32(0.8) - dist, f32(0)) * f32(2) - np.maximum(dist - f32(0.8), f32(0))).astype(f32)
    out = np.zeros(r.shape, f32)
    out[..., :3] = np.where(((i != j) & ~(dist > f32(1)))[..., None], (r[..., :3] * F[..., None]) / dist[..., None], f32(0))
    coupled = (i != j) & (dist < f32(1))
    for k in range(3, width):
        c_k = f32(0.0625) * f32(k - 2)
        out[..., k] = np.where(coupled, (-c_k) * r[..., k], f32(0))
    return out


def friction_w_neighbour(dist, i, j):
    return np.where((i != j) & (dist < f32(1)), f32(1), f32(0)).astype(f32)


def tile_rhs(X, old_v):
    """compute_tile (solvers.cuh:284-322): every pair, j ascending, one running sum per cell; then add_rhs."""
    n = len(X)
    i = np.arange(n)
    F, sf, sv = np.zeros(X.shape, f32), np.zeros(n, f32), np.zeros((n, 3), f32)
    for j in range(n):
        r = (X - X[j]).astype(f32)
        dist = gab.dist3(r)
        F = F + field_coupling(r, dist, i, j)
        fr = friction_w_neighbour(dist, i, j)
        sf = sf + fr
        sv = sv + fr[:, None] * old_v[j]
    return add_rhs(F, sf, sv)


def grid_rhs(X, old_v, gs):
    """compute_cube (solvers.cuh:430-463): the 27 cubes in d_nhood order, ascending id inside a cube, the pairs with
    dist < cube_size (1) only -- the candidate lists of tests/gabriel_statement.py, in scan order."""
    n = len(X)
    ids, dist = gab.candidates(np.ascontiguousarray(X[:, :3]), gs)
    i = np.arange(n)
    F, sf, sv = np.zeros(X.shape, f32), np.zeros(n, f32), np.zeros((n, 3), f32)
    for m in range(ids.shape[1]):
        j = ids[:, m]
        on = j >= 0
        jj = np.maximum(j, 0)
        r = (X - X[jj]).astype(f32)
        d = np.where(on, dist[:, m], f32(1))
        F = np.where(on[:, None], F + field_coupling(r, d, i, j), F)
        fr = friction_w_neighbour(d, i, j)
        sf = np.where(on, sf + fr, sf)
        sv = np.where(on[:, None], sv + fr[:, None] * old_v[jj], sv)
    return add_rhs(F, sf, sv)


def add_rhs(F, sf, sv):
    dX = F.copy()
    dX[:, :3] = np.where((sf > 0)[:, None], F[:, :3] + sv / sf[:, None], F[:, :3])    # solvers.cuh:146-161
    return dX


def heun_steps(X, steps, dt, rhs, fixed):
    """Heun_solver::take_step (solvers.cuh:226-275): the fixed velocity -- the centre of mass' in the engine's tree
    order, `sum * float(1. / n)`, or cell `fixed`'s -- is taken from x, y, z alone; every field is stepped."""
    X = X.copy()
    n = len(X)
    old_v = np.zeros((n, 3), f32)
    dt = f32(dt)
    inv_n = f32(f64(1.0) / f64(f32(n)))

    def held(dX):
        fix = tree_sum(np.ascontiguousarray(dX[:, :3])) * inv_n if fixed is None else dX[fixed, :3].copy()
        dX[:, :3] = dX[:, :3] - fix
        return dX

    for _ in range(steps):
        dX = held(rhs(X, old_v))
        X1 = X + dX * dt
        dX1 = held(rhs(X1, old_v))
        X = X + ((dX + dX1) * f32(0.5)) * dt
        old_v = ((dX + dX1) * f32(0.5))[:, :3].copy()
    return X, old_v


@pytest.mark.parametrize("fixed", [None, 17])
@pytest.mark.parametrize("solver,kind", [("tile", t) for t in ws.TILE_TYPES] + [("grid", t) for t in ws.GRID_TYPES])
def test_oracle_steps_field_coupling_as_the_statement_does(widths_oracle, solver, kind, fixed):
    """Two Heun steps of every tile and grid model of the widths library, 300 cells: every field column of the positions
    and old_v, bit for bit.  The extra fields move (their force is not zero) and differ from column to column."""
    def setup(s):
        if fixed is not None:
            s.set_fixed(fixed)
    got = ws.run(widths_oracle, ws.model(kind, solver), N, dist=0.6, seed=3, gs=GS, dt=0.05, steps=2, setup=setup)
    X0 = got["first"]
    assert X0.shape == (N, ws.WIDTH[kind])
    with np.errstate(invalid="ignore", divide="ignore"):     # (the self pair's 0 / 0 is masked out)
        rhs = tile_rhs if solver == "tile" else (lambda X, v: grid_rhs(X, v, GS))
        X, v = heun_steps(X0, 2, 0.05, rhs, fixed)
    moved = np.abs(X - X0).max(axis=0)
    assert (moved > 1e-4).all(), moved          # every field column has been stepped
    for k in range(X.shape[1]):
        assert np.array_equal(ws.bits(X[:, k]), ws.bits(got["X"][:, k])), f"field {k}"
    assert np.array_equal(ws.bits(v), ws.bits(got["old_v"]))


def test_field_coupling_reads_every_field():
    """The statement itself: a change of r[k] changes component k and nothing else, for every k >= 3; c_k is exact."""
    rng = np.random.default_rng(1)
    r = (rng.random((50, 16)) - 0.5).astype(f32)
    dist = gab.dist3(r)
    assert (dist < 1).all()
    i, j = np.arange(50), np.arange(50) + 1
    base = field_coupling(r, dist, i, j)
    assert (base[:, 3:] != 0).all()
    for k in range(3, 16):
        assert float(f32(0.0625) * f32(k - 2)) == (k - 2) / 16
        other = r.copy()
        other[:, k] += f32(0.25)
        diff = field_coupling(other, dist, i, j) != base
        assert diff[:, k].all() and not np.delete(diff, k, axis=1).any()
    assert (field_coupling(r, dist, i, i) == 0).all()                      # the self pair
    assert (field_coupling(r, dist + f32(1), i, j) == 0).all()             # beyond the cut-off


# ---- the libraries -----------------------------------------------------------------------------------------------------
def test_the_widths_library_has_its_own_table(widths_oracle, oracle):
    names = models(widths_oracle)
    want = ([ws.model(t, "grid") for t in ws.GRID_TYPES] + [ws.model(t, "tile") for t in ws.TILE_TYPES] +
            [ws.model(t, "gabriel") for t in ws.GABRIEL_TYPES])
    assert names == want
    assert not set(names) & set(models(oracle))          # the main table is as it was: none of these rows
    for t in ws.GRID_TYPES:
        with Solution(ws.model(t, "grid"), 8, 10, 1.0, lib=widths_oracle) as s:
            assert s.n_floats == ws.WIDTH[t]


# ---- the start states ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 65, 4000, 6000])
def test_extra_fields_are_distinct_everywhere(n):
    """Every extra field starts non-zero, different in every cell, and no two columns are equal or constant."""
    E = ws.extra_fields(n, 16)
    assert E.dtype == f32 and E.shape == (n, 13) and (E != 0).all() and (np.abs(E) < 1).all()
    for a in range(13):
        assert len(np.unique(E[:, a])) == n                      # (so not constant for n >= 2)
        for b in range(a + 1, 13):
            assert not np.array_equal(E[:, a], E[:, b])
    assert np.array_equal(ws.extra_fields(n, 6), E[:, :3])     # a narrower type's fields are the first columns


def test_start_fills_every_field_of_the_model(widths_oracle):
    with Solution(ws.model("w16", "grid"), 300, GS, 1.0, lib=widths_oracle) as s:
        X0 = ws.start(s, 300, 0.5, 7)
        assert np.array_equal(s.positions(), X0)                     # the "device" has them
    assert X0.shape == (300, 16) and (X0[:, 3:] != 0).all() and np.abs(X0[:, :3]).max() > 1
    assert len({X0[:, k].tobytes() for k in range(16)}) == 16


# ---- what the GPU tests' shapes claim --------------------------------------------------------------------------------
def stencil_row_offsets(gs):
    """Rows of three consecutive cubes centred on 0, -gs, +gs, then shifted by -gs^2, by +gs^2 (solvers.cuh:472-483)."""
    return [dy + dz for dz in (0, -gs * gs, gs * gs) for dy in (0, -gs, gs)]


def tile_plane_totals(cube_id, n, gs):
    """Per 64-cell tile of the cube-sorted cells and per plane: the cells of the three rows of cubes that the tile's
    cubes [c_lo, c_hi] reach in that plane, which grid_force_bits stages (in chunks of the type's capacity)."""
    cubes = np.sort(cube_id[:n].astype(np.int64))
    assert np.array_equal(cubes, cube_id[:n])                   # the grid's cube ids come sorted
    def below(c):
        return np.searchsorted(cubes, c, "left")
    s0 = np.arange(0, n, 64)
    c_lo, c_hi = cubes[s0], cubes[np.minimum(s0 + 64, n) - 1]
    offs = np.array(stencil_row_offsets(gs)).reshape(3, 3)
    return np.stack([sum(below(c_hi + off + 2) - below(c_lo + off - 1) for off in offs[p]) for p in range(3)], axis=1)


def row_bits(cube_id, n, gs):
    """Per cell and plane: the bits its candidates take in one pass -- each of the three rows padded to four."""
    cubes = cube_id[:n].astype(np.int64)
    def below(c):
        return np.searchsorted(cubes, c, "left")
    offs = np.array(stencil_row_offsets(gs)).reshape(3, 3)
    return np.stack([sum((below(cubes + off + 2) - below(cubes + off - 1) + 3) // 4 * 4 for off in offs[p])
                     for p in range(3)], axis=1)


def grid_of(lib, kind, n, dist, seed, gs, cs):
    with Solution(ws.model(kind, "grid"), n, gs, cs, lib=lib) as s:
        ws.start(s, n, dist, seed)
        cube_id, point_id, cube_start, cube_end = s.build_grid(gs, cs)
    return cube_id


def test_stage_capacities_follow_the_entry_size():
    """352 staged cells for entries of up to 24 bytes, 256 up to 32, 176 beyond (ya::bits::Stage; held per type by
    the static_asserts of yalla_amd/csrc/widths_models.h): all three classes are among the new types."""
    assert ws.ENTRY_BYTES == {"float4": 32, "w4": 20, "w6": 28, "w8": 36, "w9": 40, "w11": 48, "w16": 68}
    assert ws.STAGE_CAPACITY == {"float4": 256, "w4": 352, "w6": 256, "w8": 176, "w9": 176, "w11": 176, "w16": 176}
    header = open(os.path.join(ROOT, "yalla_amd", "csrc", "widths_models.h")).read()
    for kind, name in (("float4", "float4"), ("w4", "W4"), ("w6", "W6"), ("w8", "W8"), ("w9", "W9"), ("w11", "W11"),
                       ("w16", "W16")):
        assert (f"sizeof(ya::Entry<{name}>) == {ws.ENTRY_BYTES[kind]} && ya::bits::Stage<{name}>::value == "
                f"{ws.STAGE_CAPACITY[kind]}") in header


@pytest.mark.parametrize("kind", [t for t in ws.GRID_TYPES if ws.STAGE_CAPACITY[t] < 352])
def test_4000_cells_have_planes_on_both_sides_of_the_stage_capacity(widths_oracle, kind):
    """random_sphere(0.5) with 4000 cells, about 10 per cube: for the 176- and the 256-cell class some tile stages a
    plane in chunks and some tile stages one at once."""
    totals = tile_plane_totals(grid_of(widths_oracle, kind, 4000, 0.5, 7, 50, 1.0), 4000, 50)
    cap = ws.STAGE_CAPACITY[kind]
    assert (totals > cap).any() and ((totals > 0) & (totals <= cap)).any(), (totals.min(), totals.max())
    assert (totals.max(axis=1) > cap).sum() >= 5


@pytest.mark.parametrize("kind", ws.GRID_TYPES)
def test_dense_cases_chunk_and_overflow_a_pass(widths_oracle, kind):
    """random_sphere(0.1) with 6000 cells (hundreds per cube) and the cube_size 2.5 case: planes beyond every type's
    capacity -- the 352-cell class included -- and, in the first, rows beyond one pass of the bit stream."""
    cap = ws.STAGE_CAPACITY[kind]
    cube_id = grid_of(widths_oracle, kind, 6000, 0.1, 7, 50, 1.0)
    assert (tile_plane_totals(cube_id, 6000, 50) > cap).any()
    assert (row_bits(cube_id, 6000, 50) > ws.PASS_BITS).any()
    cube_id = grid_of(widths_oracle, kind, 3000, 0.5, 7, 50, 2.5)
    assert (tile_plane_totals(cube_id, 3000, 50) > cap).any()


# ---- seventeen floats --------------------------------------------------------------------------------------------------
SNIPPET = r'''
#include "dtypes.cuh"
#include "inits.cuh"
#include "solvers.cuh"
MAKE_PT(W16, a, b, c, d, e, f, g, h, k, l, m, n, o);
MAKE_PT(W17, a, b, c, d, e, f, g, h, k, l, m, n, o, p);
void make()
{
    Solution<WIDE, Grid_solver> grid{100, 20, 1.f};
    Solution<WIDE, Tile_solver> tile{100};
    Solution<WIDE, Gabriel_solver> gabriel{100, 20, 1.f};
    grid.take_step<relu_force>(0.1f);
    tile.take_step<relu_force>(0.1f);
    gabriel.take_step<relu_force>(0.1f);
}
'''


def compile_snippet(tmp_path, wide):
    src = tmp_path / f"wide_{wide}.hip"
    src.write_text(SNIPPET)
    return subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only",
                           "-std=c++17", "-DYALLA_NO_THRUST", f"-DWIDE={wide}", "-I" + os.path.join(ROOT, "include"),
                           str(src)], capture_output=True, text=True)


def test_seventeen_floats_are_refused_at_compile_time(tmp_path):
    """libyalla_hip.so's per-width kernels end at 16 floats: a wider point used to reach hipErrorInvalidValue and an
    abort at the first step; now Solution<W17, ...> of every solver is a static_assert that names the limit, and the
    same lines with 16 floats compile.  (They did not: Tile_solver named tile_force_coop<..., 16> for every type, whose
    tile of 64 partners does not fit LDS from 11 floats on -- `static_assert(TILE >= 64)` in a user's model.  This
    is the narrowest case that showed it.)"""
    assert compile_snippet(tmp_path, "W16").returncode == 0
    bad = compile_snippet(tmp_path, "W17")
    assert bad.returncode != 0
    assert "static assertion failed" in bad.stderr and "16-float limit" in bad.stderr
    for solver in ("Grid_computer", "Tile_computer", "Gabriel_computer"):
        assert f"Heun_solver<W17, {solver}>" in bad.stderr, solver
