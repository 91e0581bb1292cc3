"""Carried steps bin in their update kernels (include/solvers.cuh, Heun_solver::bin_in_update): euler_step and
heun_step_sorted bin the entry they have just stored (ya::bin_entry, include/grid_bin.cuh -- the device text k_bin
runs), the rebuild behind them runs without k_bin (ya_grid_rebuild_sorted_binned), and the rebuilds whose public
point ids nobody can read do not store them (YA_REBUILD_PRIVATE).

The reference of every case is the same system advanced by one-step calls, which never enter the carried path.
Compared are the bit patterns of X, old_v, the count and the four public grid arrays.  `fused_bin_rebuilds()` says
that the rebuilds really ran without k_bin (2 k - 1 per carried call of k steps) and `carried_steps()` that the call
was carried: no case can pass on a fallback.  No case takes a cell out of its grid.
"""
import numpy as np
import pytest

from carry_support import GRID_KEYS, GS, Before_call, advance, carried_and_fused, cube_changes, same, single_steps

pytestmark = pytest.mark.gpu


# ---- the switch ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params, fused_per_call", [
    ((("bin_in_update", 1),), True),
    ((("bin_in_update", 1), ("trim_carried_stores", 0)), True),
    ((("bin_in_update", 1), ("four_tile_updates", 0)), True),
    ((("bin_in_update", 0),), False),
    ((("carry_sorted", 0),), None),
], ids=["on", "on_every_store", "on_one_tile", "off", "not_carried"])
def test_switch(params, fused_per_call):
    n, k = 3000, 4
    ref, _ = single_steps("springs_grid", n, n, k, 0.001)
    got, counters, _ = advance("springs_grid", n, [k], 0.001, params=params)
    assert counters["carried"] == (0 if fused_per_call is None else k - 1)
    assert counters["fused"] == (2 * k - 1 if fused_per_call else 0)
    same(got[-1], ref[k - 1])


def test_default_is_on():
    n, k = 500, 3
    _, counters, _ = advance("springs_grid", n, [k], 0.001)
    assert counters == carried_and_fused([k])


# ---- sizes at the wavefront's and the workgroup's edges ------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("spare", [0, 37])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000])
def test_sizes(n, spare, k):
    ref, _ = single_steps("springs_grid", n, n + spare, 3, 0.001)
    got, counters, _ = advance("springs_grid", n, [k], 0.001, n_max=n + spare)
    assert counters == carried_and_fused([k])
    same(got[-1], ref[k - 1])


# ---- runs of equal cube ids longer than a wavefront ----------------------------------------------------------------

def test_runs_longer_than_a_wavefront():
    """3000 cells in the eight cubes around the origin of an 8^3 grid: in storage order a run of equal cube ids spans
    several wavefronts and workgroups, so most wavefronts issue ONE atomic for all 64 lanes and a cube's counter is
    shared by many workgroups.  (CPU oracle for this start and 2 steps of 1e-4: max |X| 0.831, 0.807, 0.770, and 356 .. 400 cells per cube;
    the grid reaches to 4.)"""
    n, k, gs, sphere, dt = 3000, 2, 8, (0.1, 42), 1e-4
    ref, first = single_steps("springs_grid", n, n, k, dt, gs=gs, sphere=sphere)
    for X in [first] + [r["X"] for r in ref]:
        assert float(np.abs(X[:, :3]).max()) < 1.0  # the eight cubes, far from the border at 4
    per_cube = np.bincount(ref[0]["cube_id"], minlength=gs ** 3)
    print("cells per occupied cube:", per_cube[per_cube > 0])
    assert (per_cube > 0).sum() == 8 and per_cube.max() > 256
    got, counters, _ = advance("springs_grid", n, [k], dt, gs=gs, sphere=sphere)
    assert counters == carried_and_fused([k])
    same(got[-1], ref[k - 1])


# ---- cells that change cube between steps --------------------------------------------------------------------------

@pytest.mark.parametrize("model, dt", [("springs_grid", 0.02), ("relu_grid", 0.05)])
def test_cells_that_change_cube(model, dt):
    """Large steps: hundreds of the 3000 cells sit in another cube after every step, so an update kernel that binned
    a cell where it WAS would sort it into the wrong cube.  The count is taken from the reference run itself."""
    n, k = 3000, 4
    ref, first = single_steps(model, n, n, k, dt)
    path = [first] + [r["X"] for r in ref]
    moved = [cube_changes(a, b) for a, b in zip(path, path[1:])]
    print("cells in another cube after steps 1 ..", k, ":", moved, " max |X|", float(np.abs(path[-1]).max()))
    assert min(moved) >= 100, moved
    assert float(np.abs(path[-1][:, :3]).max()) < GS // 2  # nobody left the grid
    got, counters, _ = advance(model, n, [k], dt)
    assert counters == carried_and_fused([k])
    same(got[-1], ref[k - 1])


# ---- count[] is left zero ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("calls", [(3, 1, 4), (2, 2, 2)])
def test_counters_are_zero_between_calls(calls):
    """Several calls on one system, carried and plain: a binning that no scan followed (the call's last corrector
    must not bin) would leave count[] non-zero and every later build wrong.  Compared after every call."""
    n = 3000
    ref, _ = single_steps("springs_grid", n, n, sum(calls), 0.001)
    got, counters, _ = advance("springs_grid", n, list(calls), 0.001)
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

    ref, _, _ = advance("springs_grid", n, [1] * 5, 0.001, between=Before_call(change, 3))
    got, counters, _ = advance("springs_grid", n, [3, 2], 0.001, between=change)
    assert counters == carried_and_fused([3, 2])
    assert got[-1]["n"] == n - fewer
    same(got[-1], ref[-1])


# ---- the public arrays after a call, and the visit order they leave ------------------------------------------------

@pytest.mark.parametrize("k", [2, 5])
def test_public_arrays_and_the_next_build(k):
    """Only the call's last rebuild stores the public point ids and the order in which the next build by id visits
    the cells: both must be what k one-step calls leave, and a following one-step call -- whose build visits the
    cells in that order -- must agree too."""
    n = 3000
    ref, _ = single_steps("springs_grid", n, n, 6, 0.001)
    got, counters, _ = advance("springs_grid", n, [k, 1], 0.001)
    assert counters == carried_and_fused([k])
    for key in GRID_KEYS:
        assert np.array_equal(got[0][key], ref[k - 1][key]), key
    same(got[0], ref[k - 1])
    same(got[1], ref[k])


# ---- wider points and ids that matter ------------------------------------------------------------------------------

@pytest.mark.parametrize("model, params", [
    ("sorting_grid", (("n_cells", 2000),)),  # the functor reads the id: `i < n_cells / 2`
    ("relu_po_grid", ()),                    # 24-byte entries
    ("relu_cell_grid", ()),                  # 32-byte entries
])
def test_ids_and_wider_points(model, params):
    n, k = 2000, 3
    ref, _ = single_steps(model, n, n, k, 0.01, params)
    got, counters, _ = advance(model, n, [k], 0.01, params=params)
    assert counters == carried_and_fused([k])
    same(got[-1], ref[k - 1])
