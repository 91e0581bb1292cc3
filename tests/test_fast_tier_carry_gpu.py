"""The fast-arithmetic tier's carried calls (libyalla_models_fast.so: -DYA_ARITH_FAST -ffp-contract=fast), which
`bench.py --arith fast` measures: take_step(dt, k) with the cells kept cube-sorted from step to step, binning inside
euler_step / heun_step_sorted, ya_grid_rebuild_sorted_binned, and graph replay -- a separate compilation of every
kernel of tests/test_bin_in_update_gpu.py under another contraction mode, which that file says nothing about.

The reference of every case is the SAME fast library advanced by one-step calls, which never enter the carried path.
Compared bit for bit: X, old_v, the count and the four public grid arrays.  That this tier can be held to bits at
all rests on ya::round_fix (include/solvers.cuh): every update kernel subtracts the ROUNDED mean velocity, whereas a
contracting build is otherwise free to fuse `sum * (1 / n)` into the subtraction in one instantiation
(heun_step, heun_step_sorted<.., 1>) and not in another (heun_step_sorted<.., 4>, which uses the product four times).

Every carried run asserts carried_steps() == k - 1, and with binning in the update kernels fused_bin_rebuilds() ==
2 k - 1: no case can pass on a fallback.  No case takes a cell out of its grid.
"""
import numpy as np
import pytest

from carry_support import GS, Before_call, advance, carried_and_fused, cube_changes, same, single_steps

pytestmark = pytest.mark.gpu

FAST = "fast"


# ---- sizes at the wavefront's and the workgroup's edges ------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("spare", [0, 37])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000])
def test_sizes(n, spare, k):
    ref, _ = single_steps("springs_grid", n, n + spare, 3, 0.001, tier=FAST)
    got, counters, _ = advance("springs_grid", n, [k], 0.001, n_max=n + spare, tier=FAST)
    assert counters == carried_and_fused([k])
    for key in ("X", "old_v"):
        print(f"n {n} spare {spare} k {k}: max |{key} carried - {key} single steps| =",
              float(np.abs(got[-1][key].astype(np.float64) - ref[k - 1][key]).max()))
    same(got[-1], ref[k - 1])


# ---- the switches: all give the same bits ---------------------------------------------------------------------------

@pytest.mark.parametrize("params, carried, fused", [
    ((), True, True),
    ((("four_tile_updates", 0),), True, True),
    ((("trim_carried_stores", 0),), True, True),
    ((("bin_in_update", 0),), True, False),
    ((("carry_sorted", 0),), False, False),
    ((("sorted_pipeline", 0),), False, False),  # (Grid_computer::carry_ready: nothing to carry without sorted cells)
], ids=["default", "one_tile", "every_store", "bin_off", "not_carried", "by_id"])
def test_switches(params, carried, fused):
    n, k = 3000, 4
    ref, _ = single_steps("springs_grid", n, n, 2 * k, 0.001, tier=FAST)
    got, counters, _ = advance("springs_grid", n, [k], 0.001, params=params, tier=FAST)
    assert counters == {"carried": k - 1 if carried else 0, "fused": 2 * k - 1 if fused else 0}
    same(got[-1], ref[k - 1])


def test_graph_replay():
    """Captured steps are the plain loop replayed, not carried; the second call replays what the first captured."""
    n, k = 3000, 4
    ref, _ = single_steps("springs_grid", n, n, 2 * k, 0.001, tier=FAST)
    seen = {}
    got, counters, _ = advance("springs_grid", n, [k, k], 0.001, params=(("graph", 1),), tier=FAST, seen=seen)
    assert counters == {"carried": 0, "fused": 0}
    assert seen["graph"] > 0
    same(got[0], ref[k - 1])
    same(got[1], ref[2 * k - 1])


# ---- cells that change cube between steps --------------------------------------------------------------------------

@pytest.mark.parametrize("model, dt", [("springs_grid", 0.02), ("relu_grid", 0.05)])
def test_cells_that_change_cube(model, dt):
    """Large steps: hundreds of the 3000 cells sit in another cube after every step, so an update kernel that binned
    a cell where it WAS -- or a contracted cube id that came out one off -- would sort it into the wrong cube.  The
    count is taken from the reference run itself."""
    n, k = 3000, 4
    ref, first = single_steps(model, n, n, k, dt, tier=FAST)
    path = [first] + [r["X"] for r in ref]
    moved = [cube_changes(a, b) for a, b in zip(path, path[1:])]
    print("cells in another cube after steps 1 ..", k, ":", moved, " max |X|", float(np.abs(path[-1]).max()))
    assert min(moved) >= 100, moved
    assert max(float(np.abs(X[:, :3]).max()) for X in path) < GS // 2  # nobody left the grid
    got, counters, _ = advance(model, n, [k], dt, tier=FAST)
    assert counters == carried_and_fused([k])
    same(got[-1], ref[k - 1])


# ---- runs of equal cube ids longer than a wavefront ----------------------------------------------------------------

def test_runs_longer_than_a_wavefront():
    """3000 cells in the eight cubes around the origin of an 8^3 grid (tests/test_bin_in_update_gpu.py's case): a run
    of equal cube ids spans several wavefronts and workgroups, most wavefronts issue ONE atomic for all 64 lanes."""
    n, k, gs, sphere, dt = 3000, 2, 8, (0.1, 42), 1e-4
    ref, first = single_steps("springs_grid", n, n, k, dt, gs=gs, sphere=sphere, tier=FAST)
    for X in [first] + [r["X"] for r in ref]:
        assert float(np.abs(X[:, :3]).max()) < 1.0  # the eight cubes, far from the border at 4
    per_cube = np.bincount(ref[0]["cube_id"], minlength=gs ** 3)
    print("cells per occupied cube:", per_cube[per_cube > 0])
    assert (per_cube > 0).sum() == 8 and per_cube.max() > 256
    got, counters, _ = advance("springs_grid", n, [k], dt, gs=gs, sphere=sphere, tier=FAST)
    assert counters == carried_and_fused([k])
    same(got[-1], ref[k - 1])


# ---- wider points and ids that matter ------------------------------------------------------------------------------

@pytest.mark.parametrize("model, params", [
    ("sorting_grid", (("n_cells", 2000),)),  # the functor reads the id: `i < n_cells / 2`
    ("relu_po_grid", ()),                    # 24-byte entries
    ("relu_cell_grid", ()),                  # 32-byte entries
])
def test_ids_and_wider_points(model, params):
    n, k = 2000, 3
    ref, _ = single_steps(model, n, n, k, 0.01, params, tier=FAST)
    got, counters, _ = advance(model, n, [k], 0.01, params=params, tier=FAST)
    assert counters == carried_and_fused([k])
    same(got[-1], ref[k - 1])


# ---- several calls on one system: count[] is left zero -------------------------------------------------------------

@pytest.mark.parametrize("calls", [(3, 1, 4), (2, 2, 2)])
def test_counters_are_zero_between_calls(calls):
    n = 3000
    ref, _ = single_steps("springs_grid", n, n, 2 * 4, 0.001, tier=FAST)
    got, counters, _ = advance("springs_grid", n, list(calls), 0.001, tier=FAST)
    assert counters == carried_and_fused(calls)
    for snap, steps in zip(got, np.cumsum(calls)):
        same(snap, ref[steps - 1])


def test_fewer_cells_and_other_positions_between_two_calls():
    n, fewer = 3000, 500

    def change(s):
        s.copy_to_host()
        s.h_X[:n, :3] += np.float32(0.25)
        s.h_n = n - fewer
        s.copy_to_device()
        s.set_old_v(np.random.default_rng(5).normal(0, 0.1, (s.n_max, 3)).astype(np.float32))

    ref, _, _ = advance("springs_grid", n, [1] * 5, 0.001, between=Before_call(change, 3), tier=FAST)
    got, counters, _ = advance("springs_grid", n, [3, 2], 0.001, between=change, tier=FAST)
    assert counters == carried_and_fused([3, 2])
    assert got[-1]["n"] == n - fewer
    same(got[-1], ref[-1])
