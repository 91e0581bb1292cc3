"""Several lanes per cell inside GridEnsemble's launches that step from LDS (set_param("lds_step_lanes", 4 | 16 | 64);
include/ensemble_grid.cuh, ya::ens::grid_lds_walk_coop).  THE REFERENCES of every comparison: the same object type with
lds_step_lanes = 1 -- the kernel as it was -- and the 14-launch twin (tests/ensemble_grid_lds_lanes_support.py, Lanes).
Every comparison is of bit patterns -- positions of EVERY row, old_v, every replica's status and grid arrays -- and
every case asserts the launches counted and lds_step_lanes_used."""
import ensemble_grid_lds_lanes_support as ls
import grid_edge_cases as ge
import numpy as np
import pytest
from ensemble_grid_links_support import MODELS as LINKED_MODELS
from ensemble_grid_links_support import N_FLOATS as LINKED_N_FLOATS
from ensemble_grid_links_support import Run, box_rows as linked_box_rows, no_nan, random_links, same
from ensemble_grid_lds_lanes_support import LANES, Lanes
from ensemble_grid_lds_support import UNUSED
from ensemble_support import DT, FRICTION_MODELS, bits, lds_layout, seeded_rows
from test_ensemble_grid_gpu import MODELS
from test_ensemble_grid_lds_lanes_abi import LINKED_RULE_POINTS, RULE_POINTS
from test_ensemble_grid_lds_steps_gpu import (N_FLOATS, SMALL_DT, assert_the_inputs_can_show_a_wrong_order,
                                              inner_box_rows, some_old_v)

from yalla_amd.ensemble import GridEnsemble, YallaError

pytestmark = pytest.mark.gpu

f32 = np.float32
COUNTS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024]
PAIRWISE = [m for m in MODELS + FRICTION_MODELS if m != "push"]  # every harness model that has pairwise forces
N_FLOATS = dict(N_FLOATS, friction_field=5)


def ordered_sum(terms):
    total = f32(0)
    for t in terms:
        total = f32(total + t)
    return total


def some_cell_shows_the_order(X, cubes, t):
    for i in range(len(X)):
        near = np.abs(cubes - cubes[i]).max(axis=1) <= 1
        d2, _ = ge.d2_of(X[i][None, :], X)
        hits = np.flatnonzero(near & (d2 < t))
        terms = (X[i, 0] - X[hits, 0]).astype(f32)
        if len(hits) >= 3 and bits(ordered_sum(terms))[0] != bits(ordered_sum(terms[::-1]))[0]:
            return True
    return False


def assert_another_order_changes_a_bit(run, grid_size, cube_size=1.0):
    """In numpy, from the twin's positions: for some cell of the largest replicas, adding the displacements to its
    hits (what every pairwise force here is linear in) in descending instead of ascending order changes a bit of the
    binary32 sum -- a kernel that adds a cell's terms in another order cannot hide behind these inputs."""
    run.twin.copy_to_host()
    t = ge.cutoff_squared(cube_size)
    for r in [r for r, n in enumerate(run.counts) if n >= 1023]:
        n = run.counts[r]
        X = run.twin.h_X[r, :n, :3].copy()
        cubes = ge.cube3_of(X, cube_size, grid_size)
        assert some_cell_shows_the_order(X, cubes, t), r


# ---- the main sweep -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("model", PAIRWISE)
def test_every_model_count_and_lane_setting_is_the_one_lane_launch_and_the_fourteen_launches(model, sum_order):
    """One ensemble of n_max = 1024 with every count of COUNTS per setting of 4, 16, 64 lanes: 1 step, then 5 steps
    from a non-zero old_v; the references (one lane from LDS, the 14 launches) are computed once for the three.
    clipped_push carries a generic force: 0 launches, lds_step_lanes_used stays 0, the same bits."""
    grid_size = 9 if sum_order == 0 else 12
    n_floats = N_FLOATS.get(model, 3)
    rows = [inner_box_rows(n, n_floats, grid_size, 300 + 17 * r + sum_order) for r, n in enumerate(COUNTS)]
    run = Lanes(model, COUNTS, 1024, grid_size, rows=rows)
    try:
        run.set_sum_order(sum_order)
        expected = 0 if model == "clipped_push" else 1
        run.step(SMALL_DT, 1, launches=expected)
        run.check("one step")
        assert_the_inputs_can_show_a_wrong_order(run.base, grid_size)
        assert_another_order_changes_a_bit(run.base, grid_size)
        run.set_old_v(some_old_v((len(COUNTS), 1024), 9))
        run.step(SMALL_DT, 5, launches=expected)
        run.check("five steps from a non-zero old_v")
        assert_the_inputs_can_show_a_wrong_order(run.base, grid_size)
        for setting, ens in run.lanes.items():
            assert ens.lds_step_lanes_used == (0 if expected == 0 else ls.lanes_expected(model, n_floats, 1024, setting))
            assert np.all(ens.h_X[np.arange(1024)[None, :] >= np.asarray(COUNTS)[:, None]] == UNUSED)
    finally:
        run.close()


def test_push_stays_ineligible():
    run = Lanes("push", [40, 0, 300], 300, 8)
    try:
        run.step(DT, 2, launches=0)
        run.check("push")
        assert all(ens.lds_step_lanes_used == 0 and ens.lds_step_launches == 0 for ens in run.lanes.values())
    finally:
        run.close()


# ---- shapes that stress the new code --------------------------------------------------------------------------------
@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("model", ["springs", "relu_po"])
def test_one_cube_of_300_cells_isolated_cells_and_cells_that_all_miss_each_other(model, sum_order):
    """dense: 300 cells in one cube -- 300 candidates per row of each cell, several tiles of the term buffer (asserted
    from the rule), next to replicas whose cells have 1.  lonely: only the self pair is inside a stencil.  misses: 27
    cells, one per cube of a 3^3 block at cube size 2.5, 2.5 apart: every cell has 26 candidates besides itself and
    every one of them is a miss (asserted)."""
    n_floats = N_FLOATS.get(model, 3)
    rng = np.random.default_rng(3)
    dense = seeded_rows(n_floats, 300, 8)
    dense[:, :3] = (0.05 + 0.9 * rng.random((300, 3))).astype(f32)
    lonely = seeded_rows(n_floats, 125, 9)
    lonely[:, :3] = (np.stack(np.meshgrid(*[np.arange(5)] * 3), -1).reshape(-1, 3) * 2 - 4.5).astype(f32)
    rows = [seeded_rows(n_floats, 200, 6), dense, lonely, seeded_rows(n_floats, 64, 7)]
    counts = [len(X) for X in rows]
    assert len(np.unique(ge.cube_of(dense[:, :3], 1.0, 10))) == 1
    assert all(lds_layout(n_floats, 300, True, lanes=lanes).tile < 300 for lanes in LANES)  # (more than one tile per row)
    d2, _ = ge.d2_of(lonely[:, None, :3], lonely[None, :, :3])
    assert (d2 + 9 * np.eye(125) >= 4).all()
    run = Lanes(model, counts, 300, 10, rows=rows)
    try:
        run.set_sum_order(sum_order)
        run.step(1e-4, 2, launches=1)
        run.check("a single cube, isolated cells")
        for ens in run.lanes.values():
            assert np.array_equal(bits(ens.h_X[2, :125, :3]), bits(lonely[:, :3]))  # nobody moved an isolated cell
    finally:
        run.close()
    cs = 2.5
    misses = seeded_rows(n_floats, 27, 4)
    misses[:, :3] = ((np.stack(np.meshgrid(*[np.arange(3)] * 3), -1).reshape(-1, 3) - 1) * cs + 0.25).astype(f32)
    assert len(np.unique(ge.cube_of(misses[:, :3], cs, 6))) == 27
    d2, _ = ge.d2_of(misses[:, None, :3], misses[None, :, :3])
    assert (d2 + 99 * np.eye(27) >= ge.cutoff_squared(cs)).all()
    run = Lanes(model, [27, 27, 5], 27, 6, cs, rows=[misses, misses[::-1].copy(), misses[:5]])
    try:
        run.set_sum_order(sum_order)
        run.step(DT, 2, launches=1)
        run.check("all misses")
        for ens in run.lanes.values():
            assert np.array_equal(bits(ens.h_X[0, :27, :3]), bits(misses[:, :3]))
    finally:
        run.close()


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("cs", ge.CUT_SIZES)
def test_pairs_on_the_cut_off_and_cells_on_cube_faces_as_replicas(cs, sum_order):
    cases = [ge.cut_off_case(cs)] + ([ge.faces_case(cs)] if cs in ge.FACE_SIZES else [])
    cases = [cases[0]] + cases
    counts = [c.n for c in cases]
    n_max = max(counts)
    run = Lanes("springs", counts, n_max, ge.GS, cs, rows=[c.X for c in cases])
    try:
        run.set_sum_order(sum_order)
        v = np.zeros((len(cases), n_max, 3), f32)
        for r, c in enumerate(cases):
            v[r, :c.n] = c.v
        run.set_old_v(v)
        run.step(ge.DT, ge.STEPS, launches=1)
        run.check(("cut_off and faces", cs))
    finally:
        run.close()


@pytest.mark.parametrize("model", ["clipped", "relu"])
@pytest.mark.parametrize("name", ["gs4", "gs3", "gs2", "gs1"])
def test_grids_filled_to_their_outermost_cubes_as_replicas(name, model):
    """The rim cases that fit a workgroup, 1^3 grids included (every one of the nine rows holds the whole replica: a
    cell's candidates are nine times its replica), both summation orders on one ensemble."""
    cases = [ge.rim_case(name, seed) for seed in range(4)]
    counts = [c.n for c in cases]
    run = Lanes(model, counts, max(counts), cases[0].gs, 1.0, rows=[c.X for c in cases])
    try:
        for sum_order in (0, 1):
            run.set_sum_order(sum_order)
            run.step(ge.DT, ge.STEPS, launches=1)
            run.check((name, model, sum_order), in_grid=name != "gs1")
    finally:
        run.close()


# ---- other paths ----------------------------------------------------------------------------------------------------
def test_all_three_fixed_modes():
    counts = [300, 70, 0, 64, 257, 5]
    run = Lanes("relu_po", counts, 300, 16)
    try:
        for what, call, steps in (("set_fixed()", None, 2), ("set_fixed(4)", lambda s: s.set_fixed(4), 3),
                                  ("set_fixed_xy(2)", lambda s: s.set_fixed_xy(2), 3),
                                  ("set_fixed() after xy", lambda s: s.set_fixed(), 2)):
            if call:
                run.each(call)
            run.step(DT, steps, launches=1)
            run.check(what)
    finally:
        run.close()


def test_five_steps_of_at_most_two_per_launch_are_three_launches():
    run = Lanes("relu", [100, 0, 257, 33], 300, 12)
    try:
        run.each(lambda s: isinstance(s, GridEnsemble) and s.set_param("lds_steps_max", 2))
        run.step(DT, 5, launches=3)
        run.check("2 + 2 + 1")
        run.each(lambda s: isinstance(s, GridEnsemble) and s.set_param("lds_steps_max", 256))
        run.step(DT, 4, launches=1)
        run.check("4")
    finally:
        run.close()


@pytest.mark.parametrize("model", ["clipped", "relu_po"])
def test_settings_changed_between_calls_on_one_object(model):
    """lds_step_lanes 1 <-> 16 <-> 0 <-> 64 <-> 4, sum_order, cube size, lds_steps 1 <-> -1 on ONE ensemble (`ens`)
    against a twin that only ever runs the 14 launches: n_max = 40, so that 0 means 4 lanes for these stateless models."""
    counts = [40, 17, 0, 33, 1]
    n_floats = N_FLOATS.get(model, 3)
    rows = [seeded_rows(n_floats, n, 20 + r) for r, n in enumerate(counts)]

    def make(lds_steps):
        ens = GridEnsemble(model, len(counts), 40, 8)
        ens.set_param("lds_steps", lds_steps)
        ens.h_X[:] = UNUSED
        for r, X in enumerate(rows):
            ens.h_X[r, :len(X)] = X
            ens.h_n[r] = len(X)
        ens.copy_to_device()
        return ens

    ens, twin = make(1), make(-1)
    try:
        seen = 0
        script = [("lds_step_lanes", 16, 16), ("lds_step_lanes", 1, 1), ("lds_step_lanes", 0, 4), ("sum_order", 1, 4),
                  ("lds_step_lanes", 64, 64), ("cube_size", 1.25, 64), ("lds_steps", -1, 64), ("lds_steps", 1, 64),
                  ("lds_step_lanes", 4, 4), ("sum_order", 0, 4), ("cube_size", 0.8, 4), ("lds_step_lanes", 1, 1),
                  ("lds_step_lanes", 16, 16)]
        assert ens.lds_step_lanes_used == 0
        ens.take_step(DT, 1)
        twin.take_step(DT, 1)
        assert ens.lds_step_lanes_used == 1 and ens.lds_step_launches == 1  # (the harness's default)
        seen = 1
        for k, (name, value, used) in enumerate(script):
            for e in (ens, twin):
                if name == "cube_size":
                    e.cube_size = value
                elif name != "lds_steps" or e is ens:
                    e.set_param(name, value)
            steps = 1 + k % 3
            ens.take_step(DT, steps)
            twin.take_step(DT, steps)
            launched = 0 if (name, value) == ("lds_steps", -1) else 1
            assert ens.lds_step_launches - seen == launched and twin.lds_step_launches == 0, (k, name, value)
            seen = ens.lds_step_launches
            assert ens.lds_step_lanes_used == used and twin.lds_step_lanes_used == 0, (k, name, value)
            ls.same_state(ls.state_of(twin, counts), ls.state_of(ens, counts), counts, (k, name, value))
    finally:
        ens.close()
        twin.close()


def test_a_cell_that_leaves_the_grid_during_the_call_is_reported_and_harms_nobody():
    counts = [100, 64, 257, 30]
    bad = 2
    rows = [seeded_rows(3, n, 90 + r) for r, n in enumerate(counts)]
    rows[bad][5] = (0.0, 0.0, 3.995)
    rows[bad][6] = (0.0, 0.0, 3.5)
    run = Lanes("relu", counts, 300, 8, rows=rows, singles=[0, 1, 3])
    try:
        run.step(DT, 3, launches=1)
        status = run.check("beside a replica that left its grid", in_grid=False)
        assert [s != 0 for s in status] == [r == bad for r in range(len(counts))]
        for ens in run.lanes.values():
            assert ens.h_X[bad, 5, 2] >= 4.0  # (it did leave)
            assert [ens.status(r, clear=False) for r in range(len(counts))] == [0, 0, 0, 0]  # forgotten
    finally:
        run.close()


def test_four_thousand_replicas_of_16_cells_and_their_independence():
    m, n_max, grid_size = 4000, 16, 6
    rng = np.random.default_rng(11)
    counts = rng.integers(0, n_max + 1, size=m)
    counts[[0, 1, 3999]] = [16, 0, 16]
    X = (rng.random((m, n_max, 3)) * 2).astype(f32)
    some = (0, 1, 2047, 2048, 3999)

    def stepped(lds_steps, lanes, used, overwrite=None):
        with GridEnsemble("clipped", m, n_max, grid_size) as ens:
            ens.set_param("lds_steps", lds_steps)
            ens.set_param("lds_step_lanes", lanes)
            ens.h_X[:] = X
            if overwrite is not None:
                ens.h_X[overwrite] = X[overwrite][::-1] * f32(0.5)
            ens.h_n[:] = counts
            ens.copy_to_device()
            ens.take_step(DT, 4)
            assert ens.lds_step_launches == (1 if lds_steps == 1 else 0) and ens.lds_step_lanes_used == used
            assert all(ens.status(r) == 0 for r in some)
            ens.copy_to_host()
            return bits(ens.h_X).copy(), bits(ens.old_v()).copy(), [ens.grid(r) for r in some]

    Xt, vt, gt = stepped(-1, 1, 0)
    results = {lanes: stepped(1, lanes, used) for lanes, used in ((1, 1), (4, 4), (16, 16), (64, 64), (0, 16))}
    for lanes, (Xl, vl, gl) in results.items():
        assert np.array_equal(Xt, Xl) and np.array_equal(vt, vl), lanes
        for r, a, b in zip(some, gt, gl):
            assert ge.same_grid(a, b, int(counts[r])), (lanes, r)
    counts[2047] = 16
    Xo, vo, _ = stepped(1, 16, 16, overwrite=2047)
    others = np.arange(m) != 2047
    Xl, vl, _ = results[16]
    assert np.array_equal(Xo[others], Xl[others]) and np.array_equal(vo[others], vl[others])
    assert not np.array_equal(Xo[2047], Xl[2047])


def test_parameter_validation():
    with GridEnsemble("relu", 2, 10, 6) as ens:
        for value in (0, 1, 4, 16, 64):
            assert ens.set_param("lds_step_lanes", value) == 0
        for value in (-1, 2, 8, 32, 128, 0.5, 4.5):
            with pytest.raises(YallaError, match="-3"):
                ens.set_param("lds_step_lanes", value)
        assert ens.lds_step_lanes_used == 0
        with pytest.raises(AttributeError):
            ens.lds_step_lanes_used = 3
        ens.take_step(DT, 1)  # (the harness's default: the 14 launches)
        assert ens.lds_step_lanes_used == 0 and ens.lds_step_launches == 0


# ---- the LDS rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["relu", "relu_po", "relu_cell"])
def test_either_side_of_every_point_where_another_term_of_the_rule_decides(model):
    """The n_max that tests/test_ensemble_grid_lds_lanes_abi.py names for the model's point size, each with lanes 0,
    4, 16 and 64: lds_step_lanes_used is the rule's answer -- 1 where the term buffer has no room (the 7-float point
    from 809 rows on with 4 lanes), the launch still from LDS -- and the bits are the one-lane launch's and the twin's."""
    n_floats = N_FLOATS.get(model, 3)
    fell_back = False
    for n_max in RULE_POINTS[n_floats]:
        counts = [n_max, 40 if n_max > 40 else 3, n_max - 1]
        rows = [inner_box_rows(n, n_floats, 10, 50 + r) for r, n in enumerate(counts)]
        run = Lanes(model, counts, n_max, 10, rows=rows, settings=(0,) + LANES)
        try:
            run.step(SMALL_DT, 2, launches=1)
            run.check(("n_max", n_max))
            for setting, ens in run.lanes.items():
                want = ls.lanes_expected(model, n_floats, n_max, setting)
                assert ens.lds_step_lanes_used == want, (n_max, setting)
                fell_back |= setting > 1 and want == 1
        finally:
            run.close()
    assert fell_back == (n_floats == 7)


# ---- LinkedGridEnsemble ---------------------------------------------------------------------------------------------
def linked_state(model, rows, n_max, slots, links, grid_size, steps, **params):
    run = Run(model, rows, n_max, slots, links, grid_size, **params)
    try:
        run.ens.take_step(SMALL_DT, 1)
        run.ens.set_old_v(some_old_v((len(rows), n_max), 9))
        run.ens.take_step(SMALL_DT, steps)
        state = run.state()
        return state, run.ens.lds_step_launches, run.ens.lds_step_lanes_used
    finally:
        run.close()


def linked_case(model, n_max, grid_size=9, seed=0):
    n_floats = LINKED_N_FLOATS[model]
    counts = [n_max, 0, 1, max(n_max // 3, 2), n_max - 1]
    rows = [linked_box_rows(n, n_floats, grid_size, seed + 31 * r) for r, n in enumerate(counts)]
    links = [random_links(n, 2 * n, seed + 7 * r) for r, n in enumerate(counts)]  # two links per cell
    return counts, rows, links


@pytest.mark.parametrize("model", LINKED_MODELS)
def test_linked_launches_with_two_links_per_cell(model):
    """lanes 4, 16, 64 and 0 against one lane from LDS and against the 14-launch twin, at n_max = 300 (and for the
    4- and 8-float points at the rule's points below)."""
    n_floats, n_max, slots = LINKED_N_FLOATS[model], 300, 600
    counts, rows, links = linked_case(model, n_max)
    want, launches, used = linked_state(model, rows, n_max, slots, links, 9, 4, lds_steps=-1)
    assert launches == 0 and used == 0
    no_nan(want)
    for setting in (1, 0) + LANES:
        got, launches, used = linked_state(model, rows, n_max, slots, links, 9, 4, lds_steps=1, lds_step_lanes=setting)
        assert launches == 2 and used == ls.lanes_expected(model, n_floats, n_max, setting, slots), (setting, used)
        same(want, got, counts, (model, setting))


@pytest.mark.parametrize("model", ["links4", "relu_cell8_links"])
def test_linked_launches_either_side_of_the_points_of_the_rule(model):
    """Two slots per cell, the n_max that the CPU test names for 4- and 8-float points (the 8-float ones thinned to the
    points where the answer changes: a list that leaves no room for 16 candidates' terms is the fallback to one lane;
    from 902 rows on not even the list fits and the call is the 14 launches)."""
    n_floats = LINKED_N_FLOATS[model]
    points = LINKED_RULE_POINTS[n_floats]
    if n_floats == 8:
        points = [n for n in points if n >= 594]
    seen = set()
    for n_max in points:
        slots = 2 * n_max
        counts, rows, links = linked_case(model, n_max, seed=n_max)
        fits = lds_layout(n_floats, n_max, True, slots).bytes > 0
        want, launches, used = linked_state(model, rows, n_max, slots, links, 9, 2, lds_steps=-1)
        assert launches == 0 and used == 0
        for setting in (1,) + LANES:
            got, launches, used = linked_state(model, rows, n_max, slots, links, 9, 2, lds_steps=1, lds_step_lanes=setting)
            assert launches == (2 if fits else 0), (n_max, setting)
            expected = ls.lanes_expected(model, n_floats, n_max, setting, slots) if fits else 0
            assert used == expected, (n_max, setting, used, expected)
            seen.add((setting > 1, used))
            same(want, got, counts, (model, n_max, setting))
    if n_floats == 8:
        assert {(True, 1), (True, 0), (True, 4), (True, 16), (True, 64)} <= seen  # the fallback, the 14 launches, the lanes
