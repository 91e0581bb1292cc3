"""Solution::take_steps carries the cells in cube order from step to step (include/solvers.cuh,
Heun_solver::take_steps): `take_step(dt, k)` on a qualifying Grid_solver model must leave, bit for bit, what k calls
of `take_step(dt, 1)` leave -- positions, old_v, the count and the four public grid arrays.

The reference of every case is the same system advanced by one-step calls on the device library: a one-step call
never enters the carried path, so the reference is code the carried path does not touch.  `carried_steps()` says
whether the path was taken (k - 1 per qualifying call, 0 for every fallback): without it the equalities below could
pass on the plain loop.
"""
import functools

import numpy as np
import pytest

from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu

GS = 16
SPHERE = (0.5, 42)


# ---- running a system ------------------------------------------------------------------------------------------------

def snapshot(s, with_grid=True):
    X = s.positions()  # (copy_to_host: h_n becomes the device's count)
    n = s.get_d_n()
    out = {"X": X, "old_v": s.old_v()[:n].copy(), "n": n}
    if with_grid:
        cube_id, point_id, cube_start, cube_end = s.grid()
        out.update(cube_id=cube_id[:n].copy(), point_id=point_id[:n].copy(), cube_start=cube_start, cube_end=cube_end)
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if key == "n":
            assert a[key] == b[key], key
        else:
            assert a[key].shape == b[key].shape, key
            assert np.array_equal(np.ascontiguousarray(a[key]).view(np.uint32),
                                  np.ascontiguousarray(b[key]).view(np.uint32)), key


def start(model, n, n_max, gs, params, setup, X=None):
    s = Solution(model, n_max, gs, 1.0)
    for name, value in params:
        s.set_param(name, value)
    s.h_n = n
    if X is None:
        s.random_sphere(*SPHERE)
    else:
        s.h_X[:n, :3] = X
        s.copy_to_device()
    if setup:
        setup(s)
    return s


def advance(model, n, calls, dt, *, n_max=None, gs=GS, params=(), setup=None, X=None, between=None, every_call=False,
            with_grid=True):
    """The system after take_step(dt, c) for every c of `calls` (between(s) in between two of them): its snapshot --
    or one after every call --, and the counters."""
    snaps = []
    with start(model, n, n_max or n, gs, params, setup, X) as s:
        first = s.h_X[:n].copy()
        for i, c in enumerate(calls):
            if i and between:
                between(s)
            s.take_step(dt, c)
            if every_call:
                snaps.append(snapshot(s, with_grid))
        last = snaps[-1] if every_call else snapshot(s, with_grid)
        counters = {"carried": s.carried_steps(), "graph": s.graph_launches()}
    return (snaps if every_call else last), counters, first


@functools.lru_cache(maxsize=None)
def single_steps(model, n, n_max, steps, dt, params=()):
    """Snapshots after each of `steps` one-step calls (the reference, shared by the cases that start alike)."""
    snaps, counters, first = advance(model, n, [1] * steps, dt, n_max=n_max, params=params, every_call=True)
    assert counters["carried"] == 0
    return snaps, first


# ---- sizes at the kernels' edges ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("spare", [0, 37])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 3000])
def test_sizes(n, spare, k):
    ref, _ = single_steps("springs_grid", n, n + spare, 8, 0.001)
    got, counters, _ = advance("springs_grid", n, [k], 0.001, n_max=n + spare)
    assert counters["carried"] == k - 1
    same(got, ref[k - 1])


# ---- cells that change cube between steps ------------------------------------------------------------------------

def cube_changes(before, after):
    return int(np.any(np.floor(before[:, :3]) != np.floor(after[:, :3]), axis=1).sum())


@pytest.mark.parametrize("model, dt", [("springs_grid", 0.02), ("relu_grid", 0.05)])
def test_cells_that_change_cube(model, dt):
    """Large steps: hundreds of the 3000 cells sit in another cube after every step (CPU oracle: springs 192, 253, 332,
    462; relu 305, 213, 202, 176), so the carried order is re-sorted for real.  The count is taken from the reference
    run itself: a change of the case cannot quietly stop testing this."""
    n, k = 3000, 4
    ref, first = single_steps(model, n, n, k, dt)
    path = [first] + [r["X"] for r in ref]
    moved = [cube_changes(a, b) for a, b in zip(path, path[1:])]
    print("cells in another cube after steps 1 ..", k, ":", moved, " max |X|", float(np.abs(path[-1]).max()))
    assert min(moved) >= 100, moved
    assert float(np.abs(path[-1][:, :3]).max()) < GS // 2  # nobody left the grid
    got, counters, _ = advance(model, n, [k], dt)
    assert counters["carried"] == k - 1
    same(got, ref[k - 1])


# ---- dense cubes ---------------------------------------------------------------------------------------------------

def dense_block():
    """A 2 x 2 x 2 block of cubes with 50 .. 130 cells each in a sparse background, grid size 8: planes staged in
    chunks, lanes whose candidates overflow a pass (the layout of tests/test_force_hot_loops_gpu.py's overflow case)."""
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 7, size=(6, 6, 6))
    counts[2:4, 2:4, 2:4] = rng.integers(50, 131, size=(2, 2, 2))
    X = []
    for z, y, x in np.ndindex(counts.shape):
        lo = np.array([x, y, z], dtype=np.float64) - 3.0
        X.append(lo + 2.0 ** -10 + rng.random((counts[z, y, x], 3)) * (1.0 - 2.0 ** -9))
    X = np.concatenate(X).astype(np.float32)
    X = X[rng.permutation(len(X))]  # ids unrelated to cubes
    return X[:-1] if len(X) % 64 == 0 else X


@pytest.mark.parametrize("params", [(), (("force_variant", 2),)], ids=["default", "bits"])
def test_dense_cubes(params):
    X = dense_block()
    per_cube = np.bincount(np.ravel_multi_index((np.floor(X) + 4).astype(int).T, (8, 8, 8)))
    assert per_cube.max() >= 100 and np.sort(per_cube)[-8:].sum() > 352  # (chunks: more than 352 staged cells)
    k = 3
    ref, _, _ = advance("springs_grid", len(X), [1] * k, 0.001, gs=8, params=params, X=X)
    got, counters, _ = advance("springs_grid", len(X), [k], 0.001, gs=8, params=params, X=X)
    assert counters["carried"] == k - 1
    same(got, ref)


# ---- ids that matter, wider points ---------------------------------------------------------------------------------

@pytest.mark.parametrize("model, params", [
    ("sorting_grid", (("n_cells", 2000),)),  # the functor reads the id: `i < n_cells / 2`
    ("relu_po_grid", ()),                    # 24-byte entries
    ("relu_cell_grid", ()),                  # 32-byte entries
])
def test_ids_and_wider_points(model, params):
    n, k = 2000, 3
    ref, _ = single_steps(model, n, n, k, 0.01, params)
    got, counters, _ = advance(model, n, [k], 0.01, params=params)
    assert counters["carried"] == k - 1
    same(got, ref[k - 1])


# ---- kernel choices ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [
    (),
    (("sum_order", 1),),
    (("force_variant", 2),),
    (("force_variant", 2), ("sum_order", 1)),
    (("force_variant", 2), ("gather_offset_bits", 64)),
    (("force_variant", 2), ("stage_v_max", 0)),
], ids=["coop", "coop_by_plane", "bits", "bits_by_plane", "bits_64_bit_offsets", "bits_old_v_from_memory"])
def test_kernel_choices(params):
    n, k = 3000, 3
    ref, _ = single_steps("springs_grid", n, n, k, 0.001, params)
    got, counters, _ = advance("springs_grid", n, [k], 0.001, params=params)
    assert counters["carried"] == k - 1
    same(got, ref[k - 1])


# ---- nothing survives a call ---------------------------------------------------------------------------------------

class Before_call:
    """`between` of a run in single steps: `action` before the call-th call (0-based), nothing before the others."""

    def __init__(self, action, call):
        self.action, self.call, self.seen = action, call, 0

    def __call__(self, s):
        self.seen += 1
        if self.seen == self.call:
            self.action(s)


@pytest.mark.parametrize("fewer", [0, 500])
def test_nothing_survives_a_call(fewer):
    """Other positions, other old_v and (fewer > 0) a smaller n between two calls: the second call must start from
    the id-ordered arrays as they are then, not from anything the first one kept."""
    n = 3000

    def change(s):
        s.copy_to_host()
        s.h_X[:n, :3] += np.float32(0.25)
        s.h_n = n - fewer
        s.copy_to_device()
        s.set_old_v(np.random.default_rng(5).normal(0, 0.1, (s.n_max, 3)).astype(np.float32))

    ref, _, _ = advance("springs_grid", n, [1] * 5, 0.001, between=Before_call(change, 3))
    got, counters, _ = advance("springs_grid", n, [3, 2], 0.001, between=change)
    assert counters["carried"] == 2 + 1
    assert got["n"] == n - fewer
    same(got, ref)


# ---- fallbacks: the plain loop, whatever the switch says -------------------------------------------------------------

def ring_links(n):
    return np.stack([np.arange(n), (np.arange(n) + 7) % n], axis=1).astype(np.int32)


FALLBACKS = {
    "fixed_point": ("springs_grid", 2000, (), lambda s: s.set_fixed(5)),
    "fixed_point_xy": ("springs_grid", 2000, (), lambda s: s.set_fixed_xy(5)),
    "graph": ("springs_grid", 2000, (("graph", 1),), None),
    "id_order_pipeline": ("springs_grid", 2000, (("sorted_pipeline", 0),), None),
    "links": ("springs_links_grid", 2000, (), lambda s: s.set_links(ring_links(2000), 0.2)),
    "tile": ("springs_tile", 300, (), None),
    "gabriel": ("relu_gabriel", 1000, (), None),
    "renumber_every_2": ("springs_grid", 2000, (("renumber_every", 2),), None),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallbacks_are_the_plain_loop(case):
    model, n, params, setup = FALLBACKS[case]
    k, runs = 6, []
    for switch in (1, 0):
        runs.append(advance(model, n, [k], 0.001, params=params + (("carry_sorted", switch),), setup=setup,
                            with_grid=case != "tile"))
    (on, on_counters, _), (off, off_counters, _) = runs
    assert on_counters["carried"] == 0 and off_counters["carried"] == 0
    assert on_counters["graph"] == off_counters["graph"]
    if case == "graph":
        assert on_counters["graph"] >= k - 2  # captured at the third step, replayed from then on
    same(on, off)


def test_switched_off_is_the_plain_loop():
    n, k = 3000, 8
    ref, _ = single_steps("springs_grid", n, n, 8, 0.001)
    got, counters, _ = advance("springs_grid", n, [k], 0.001, params=(("carry_sorted", 0),))
    assert counters["carried"] == 0
    same(got, ref[k - 1])


# ---- the path is really taken --------------------------------------------------------------------------------------

def test_carried_call_launches_two_force_kernels_per_step():
    n, k = 3000, 5
    with start("springs_grid", n, n, GS, (), None) as s:
        assert s.carried_steps() == 0
        s.take_step(0.001, 1)
        assert s.carried_steps() == 0  # a one-step call is never carried
        s.profile(True, 1)
        s.take_step(0.001, k)
        _, launches = s.profile_read()
        s.profile(False)
        assert launches == 2 * k
        assert s.carried_steps() == k - 1
        s.take_step(0.001, k)
        assert s.carried_steps() == 2 * (k - 1)
