"""GridEnsemble's take_step as launches that step from LDS (set_param("lds_steps", 1); include/ensemble_grid.cuh,
ya::ens::grid_lds_steps): a workgroup per replica sorts the replica's (cube, id) keys in LDS, walks the stencil rows of
that order and runs the whole Heun steps there.  THE REFERENCE of every comparison is the twin: the same rows in a
GridEnsemble with lds_steps = -1, the 14-launch path (tests/ensemble_grid_lds_support.py, GridTwins).  Every
comparison is of bit patterns -- positions of EVERY row, old_v, the counts, every replica's status and grid arrays --
and every case asserts lds_step_launches for the path it expects."""
import grid_edge_cases as ge
import numpy as np
import pytest
from ensemble_grid_lds_support import UNUSED, GridTwins, grid_lds_capacity, launches_of
from ensemble_support import DT, bits, seeded_rows
from test_ensemble_grid_gpu import MODELS, box_rows

from yalla_amd.ensemble import GridEnsemble, YallaError
from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu

f32 = np.float32
COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024]
N_FLOATS = {"relu_po": 5, "relu_cell": 7}
SMALL_DT = 0.01  # (cells that start 0.4 or more inside their grid's faces stay inside for six steps)


def inner_box_rows(n, n_floats, grid_size, seed):
    """box_rows -- uniform over the WHOLE grid box -- drawn 8 % towards the origin: the outermost cubes stay
    populated, and no cell is pushed out of the grid within a test's steps (asserted: the status stays 0)."""
    rows = np.zeros((n, n_floats), f32)
    rows[:, :3] = box_rows(n, grid_size, seed) * f32(0.92)
    rows[:, 3:] = np.random.default_rng(seed + 5).random((n, n_floats - 3)).astype(f32)
    return rows


def some_old_v(shape, seed):
    return (np.random.default_rng(seed).random(shape + (3,)) * 0.2 - 0.1).astype(f32)


def assert_the_inputs_can_show_a_wrong_order(run, grid_size, cube_size=1.0, replicas=None):
    """In numpy, from the twin's grid arrays and positions: a cube with >= 3 cells (ids inside a cube have an order),
    a candidate pair inside the cut-off and one outside it in the same stencil (the test decides), cells in cubes on
    the grid's rim (rows leave the grid)."""
    run.twin.copy_to_host()
    replicas = [r for r, n in enumerate(run.counts) if n >= 1023] if replicas is None else replicas
    assert replicas
    t = ge.cutoff_squared(cube_size)
    for r in replicas:
        n = run.counts[r]
        X = run.twin.h_X[r, :n, :3].copy()
        _, _, start, end = run.twin.grid(r)
        assert (end - start + 1).max() >= 3, r
        cubes = ge.cube3_of(X, cube_size, grid_size)
        assert cubes.min() == 0 and cubes.max() == grid_size - 1, r
        near = (np.abs(cubes[:, None, :] - cubes[None, :, :]).max(axis=2) <= 1) & ~np.eye(n, dtype=bool)
        d2, _ = ge.d2_of(X[:, None, :], X[None, :, :])
        inside, outside = near & (d2 < t), near & ~(d2 < t)
        assert (inside.any(axis=1) & outside.any(axis=1)).any(), r


# ---- 1, 2: models and counts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_every_model_and_count_is_the_fourteen_launch_path_bit_for_bit(model, sum_order):
    """One ensemble of n_max = 1024 with every count of COUNTS: 1 step, then 5 steps from a non-zero old_v, against
    the twin and, for three of the replicas, against lone Solutions.  push and clipped_push carry a generic force: 0
    launches, the same bits."""
    grid_size = 9 if sum_order == 0 else 12
    n_floats = N_FLOATS.get(model, 3)
    rows = [inner_box_rows(n, n_floats, grid_size, 300 + 17 * r + sum_order) for r, n in enumerate(COUNTS)]
    run = GridTwins(model, COUNTS, 1024, grid_size, rows=rows, singles=[3, 8, 13])
    try:
        run.set_sum_order(sum_order)
        expected = 0 if model in ("push", "clipped_push") else 1
        run.step(SMALL_DT, 1, launches=expected)
        run.check("one step")
        assert_the_inputs_can_show_a_wrong_order(run, grid_size)
        run.set_old_v(some_old_v((len(COUNTS), 1024), 9))
        run.step(SMALL_DT, 5, launches=expected)
        run.check("five steps from a non-zero old_v")
        assert_the_inputs_can_show_a_wrong_order(run, grid_size)
        assert np.all(run.ens.h_X[np.arange(1024)[None, :] >= np.asarray(COUNTS)[:, None]] == UNUSED)
    finally:
        run.close()


# ---- 3: yes/no decisions at their edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("cs", ge.CUT_SIZES)
def test_pairs_on_the_cut_off_and_cells_on_cube_faces_as_replicas(cs, sum_order):
    """The cut_off case of the cube size (pairs on and one ulp either side of the cut-off) and, where there is one, its
    faces case (cells on cube faces, within 8 ulps of them) as replicas of one ensemble, with the cases' old_v."""
    cases = [ge.cut_off_case(cs)] + ([ge.faces_case(cs)] if cs in ge.FACE_SIZES else [])
    cases = [cases[0]] + cases  # (the first case twice: a replica that does not start at row 0 holds it too)
    counts = [c.n for c in cases]
    n_max = max(counts)
    run = GridTwins("springs", counts, n_max, ge.GS, cs, rows=[c.X for c in cases])
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
    """The rim cases that fit a workgroup (the two 8^3 ones hold more than 1024 cells), four seeds side by side: a row
    that leaves or wraps around replica r's grid holds what offs[] of replica r says, nothing of replica r - 1 or
    r + 1.  Both summation orders on one ensemble."""
    cases = [ge.rim_case(name, seed) for seed in range(4)]
    counts = [c.n for c in cases]
    # (a 1^3 grid: every one of the nine rows holds the whole replica, and under relu's ninefold repulsion the 14-launch
    # path reports a cell of the first replica outside the unit cube, though the final positions are inside: here the
    # status bits and the clamped results must be the twin's, whatever they are)
    stays_inside = name != "gs1"
    run = GridTwins(model, counts, max(counts), cases[0].gs, 1.0, rows=[c.X for c in cases],
                    singles=[1] if stays_inside else [])
    try:
        for sum_order in (0, 1):
            run.set_sum_order(sum_order)
            run.step(ge.DT, ge.STEPS, launches=1)
            run.check((name, model, sum_order), in_grid=stays_inside)
    finally:
        run.close()


# ---- 4: extremes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["springs", "relu_po"])
def test_one_cube_of_300_cells_and_a_replica_of_isolated_cells(model):
    n_floats = N_FLOATS.get(model, 3)
    rng = np.random.default_rng(3)
    dense = seeded_rows(n_floats, 300, 8)
    dense[:, :3] = (0.05 + 0.9 * rng.random((300, 3))).astype(f32)  # all of it in the cube [0, 1)^3
    lonely = seeded_rows(n_floats, 125, 9)
    lonely[:, :3] = (np.stack(np.meshgrid(*[np.arange(5)] * 3), -1).reshape(-1, 3) * 2 - 4.5).astype(f32)
    rows = [seeded_rows(n_floats, 200, 6), dense, lonely, seeded_rows(n_floats, 64, 7)]
    counts = [len(X) for X in rows]
    assert len(np.unique(ge.cube_of(dense[:, :3], 1.0, 10))) == 1
    d2, _ = ge.d2_of(lonely[:, None, :3], lonely[None, :, :3])
    assert (d2 + 9 * np.eye(125) >= 4).all()
    run = GridTwins(model, counts, 300, 10, rows=rows, singles=[1, 2])
    try:
        run.step(1e-4, 2, launches=1)
        run.check("a single cube, isolated cells")
        run.ens.copy_to_host()
        assert np.array_equal(bits(run.ens.h_X[2, :125, :3]), bits(lonely[:, :3]))  # nobody moved an isolated cell
    finally:
        run.close()


# ---- 5: fixed modes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["clipped", "relu_po"])
def test_all_three_fixed_modes(model):
    """set_fixed(i), set_fixed_xy(i) (x and y in the first stage only, the second stage holds the whole point), and
    back to set_fixed(), which Heun_solver leaves with the xy mode's first stage still in force."""
    counts = [300, 70, 0, 64, 257, 5]
    run = GridTwins(model, counts, 300, 16, singles=[0, 5])
    try:
        for what, call, steps in (("set_fixed()", None, 2), ("set_fixed(4)", lambda s: s.set_fixed(4), 3),
                                  ("set_fixed_xy(2)", lambda s: s.set_fixed_xy(2), 3),
                                  ("set_fixed(1) after xy", lambda s: s.set_fixed(1), 2),
                                  ("set_fixed() after xy", lambda s: s.set_fixed(), 2)):
            if call:
                run.each(call)
            run.step(DT, steps, launches=1)
            run.check(what)
    finally:
        run.close()


# ---- 6: launch splitting --------------------------------------------------------------------------------------------
def test_five_steps_of_at_most_two_per_launch_are_three_launches():
    counts = [100, 0, 257, 33]
    run = GridTwins("relu", counts, 300, 12)
    try:
        run.ens.set_param("lds_steps_max", 2)
        run.step(DT, 5, launches=3)
        run.check("2 + 2 + 1")
        run.ens.set_param("lds_steps_max", 1)
        run.step(DT, 3, launches=3)
        run.check("1 + 1 + 1")
        run.ens.set_param("lds_steps_max", 256)
        run.step(DT, 4, launches=1)
        run.check("4")
    finally:
        run.close()


# ---- 7: capacity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["relu", "relu_po", "relu_cell"])
def test_capacity_and_one_row_beyond(model):
    """ya::ens::grid_lds_capacity restated in Python: at the capacity the launches run, one row beyond they cannot and
    take_step is the 14 launches, with the same bits."""
    n_floats = N_FLOATS.get(model, 3)
    capacity = grid_lds_capacity(n_floats)
    assert capacity == 1024  # (an 8-float point's rows leave 896 bytes of the 160 KiB)
    for n_max in (capacity, capacity + 1):
        counts = [n_max, 40, n_max - 1]
        rows = [inner_box_rows(n, n_floats, 12, 50 + r) for r, n in enumerate(counts)]
        run = GridTwins(model, counts, n_max, 12, rows=rows)
        try:
            assert launches_of(model, 2, n_max, n_floats) == (1 if n_max == capacity else 0)
            run.step(SMALL_DT, 2)
            run.check(("n_max", n_max))
        finally:
            run.close()


# ---- 8: settings changed between calls ------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["clipped", "relu_po"])
def test_settings_changed_between_calls(model):
    """cube_size, the counts, sum_order, lds_steps 1 <-> -1 on the SAME ensemble (the 14-launch path must find the
    private build arrays as it needs them after launches that never touched them, and the other way round), and
    take_step(dt, 1) alternating with take_step(dt, 3)."""
    counts = [200, 64, 0, 257, 31, 500]
    run = GridTwins(model, counts, 600, 16, singles=[0, 3])
    try:
        run.step(DT, 1, launches=1)
        run.step(DT, 3, launches=1)
        run.check("start")
        run.set_cube_size(1.25)
        run.step(DT, 1, launches=1)
        run.check("cube_size 1.25")
        run.ens.set_param("lds_steps", -1)
        run.step(DT, 3, launches=0)
        run.check("the 14 launches on the same ensemble")
        run.set_sum_order(1)
        run.ens.set_param("lds_steps", 1)
        run.step(DT, 1, launches=1)
        run.check("from LDS again, by plane")
        run.set_counts({0: 260, 1: 17, 2: 40, 3: 0, 5: 600})
        run.step(DT, 3, launches=1)
        run.check("counts changed")
        run.ens.set_param("lds_steps", -1)
        run.step(DT, 1, launches=0)
        run.ens.set_param("lds_steps", 1)
        run.set_sum_order(0)
        run.set_cube_size(0.8)
        run.step(DT, 1, launches=1)
        run.check("the reference's order again, cube_size 0.8")
        run.set_old_v(some_old_v((len(counts), 600), 5))
        run.set_counts({3: 300, 0: 64, 5: 500})
        run.set_cube_size(1.0)
        run.step(0.02, 3, launches=1)
        run.check("counts back, a replica back from empty, a fresh old_v, dt 0.02")
    finally:
        run.close()


# ---- 9: out of grid -------------------------------------------------------------------------------------------------
def test_a_cell_that_leaves_the_grid_during_the_call_is_reported_and_harms_nobody():
    """Replica 2 starts inside its 8^3 grid (asserted) with one cell just below the top face and a neighbour half a
    diameter below it, whose repulsion pushes it out during the call's three steps (asserted: it ends above the
    face).  It gets its status bit, the clamped result equals the twin's, and the other replicas equal their lone
    Solutions."""
    counts = [100, 64, 257, 30]
    bad = 2
    rows = [seeded_rows(3, n, 90 + r) for r, n in enumerate(counts)]
    rows[bad][5] = (0.0, 0.0, 3.995)    # just below the top face (z < 4) ...
    rows[bad][6] = (0.0, 0.0, 3.5)      # ... and relu's repulsion from half a diameter below it
    run = GridTwins("relu", counts, 300, 8, rows=rows, singles=[0, 1, 3])
    try:
        assert (ge.cube3_of(np.asarray(rows[bad]), 1.0, 8).max() <= 7) and run.statuses(clear=False) == [0, 0, 0, 0]
        run.step(DT, 3, launches=1)
        status = run.check("beside a replica that left its grid", in_grid=False)
        assert [s != 0 for s in status] == [r == bad for r in range(len(counts))]
        assert run.ens.h_X[bad, 5, 2] >= 4.0   # (it did leave)
        assert run.statuses(clear=False) == [0, 0, 0, 0]  # forgotten
    finally:
        run.close()


# ---- 10: many replicas ----------------------------------------------------------------------------------------------
def test_four_thousand_replicas_and_their_independence():
    m, n_max, grid_size = 4000, 16, 6
    rng = np.random.default_rng(11)
    counts = rng.integers(0, n_max + 1, size=m)
    counts[[0, 1, 3999]] = [16, 0, 16]
    X = (rng.random((m, n_max, 3)) * 2).astype(f32)

    def stepped(lds_steps, overwrite=None):
        with GridEnsemble("clipped", m, n_max, grid_size) as ens:
            ens.set_param("lds_steps", lds_steps)
            ens.h_X[:] = X
            if overwrite is not None:
                ens.h_X[overwrite] = X[overwrite][::-1] * f32(0.5)
            ens.h_n[:] = counts
            ens.copy_to_device()
            ens.take_step(DT, 4)
            assert ens.lds_step_launches == (1 if lds_steps == 1 else 0)
            assert all(ens.status(r) == 0 for r in (0, 1, 2047, 3999))
            ens.copy_to_host()
            grids = [ens.grid(r) for r in (0, 1, 2047, 2048, 3999)]
            return bits(ens.h_X).copy(), bits(ens.old_v()).copy(), grids

    Xt, vt, gt = stepped(-1)
    Xl, vl, gl = stepped(1)
    assert np.array_equal(Xt, Xl) and np.array_equal(vt, vl)
    for r, a, b in zip((0, 1, 2047, 2048, 3999), gt, gl):
        assert ge.same_grid(a, b, int(counts[r])), r
    counts[2047] = 16
    Xo, vo, _ = stepped(1, overwrite=2047)
    others = np.arange(m) != 2047
    assert np.array_equal(Xo[others], Xl[others]) and np.array_equal(vo[others], vl[others])
    assert not np.array_equal(Xo[2047], Xl[2047])


# ---- 11: parameter validation ---------------------------------------------------------------------------------------
def test_parameter_validation():
    with GridEnsemble("relu", 2, 10, 6) as ens:
        for value in (-1, 0, 1):
            assert ens.set_param("lds_steps", value) == 0
        for name, value in (("lds_steps", 2), ("lds_steps", -2), ("lds_steps", 0.5), ("lds_steps_max", 0),
                            ("lds_steps_max", -1), ("lds_steps_max", 1.5), ("lds_steps_max", 2.0 ** 31)):
            with pytest.raises(YallaError, match="-3"):
                ens.set_param(name, value)
        for value in (1, 7, 256, 2 ** 31 - 1):
            assert ens.set_param("lds_steps_max", value) == 0
        for name in ("lds", "whole_steps", "steps_per_launch", "lds_step", ""):
            with pytest.raises(YallaError, match="-2"):
                ens.set_param(name, 1)
        assert ens.lds_step_launches == 0
        with pytest.raises(AttributeError):
            ens.lds_step_launches = 3
        with pytest.raises(AttributeError):
            ens.whole_step_launches


# ---- 12: the CPU restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["relu", "springs"])
def test_the_cpu_restatement_one_lone_system_per_replica(oracle, model):
    """The oracle's <model>_grid, tree reduce order, 5 steps, M = 3 with ragged counts: the one comparison that passes
    through no shared device code."""
    counts = [257, 64, 700]
    rows = [seeded_rows(3, n, 70 + r) for r, n in enumerate(counts)]
    old_v = some_old_v((3, 700), 2)
    with GridEnsemble(model, 3, 700, 12) as ens:
        ens.set_param("lds_steps", 1)
        for r, n in enumerate(counts):
            ens.h_X[r, :n] = rows[r]
            ens.h_n[r] = n
        ens.copy_to_device()
        ens.set_old_v(old_v)
        ens.take_step(DT, 5)
        assert ens.lds_step_launches == 1
        assert [ens.status(r) for r in range(3)] == [0, 0, 0]
        ens.copy_to_host()
        v = ens.old_v()
        for r, n in enumerate(counts):
            with Solution(model + "_grid", 700, 12, 1.0, lib=oracle) as s:
                assert s.set_reduce_order(1) == 0
                s.h_X[:n] = rows[r]
                s.h_n = n
                s.copy_to_device()
                s.set_old_v(old_v[r])
                s.take_step(DT, 5)
                assert np.array_equal(bits(s.positions()), bits(ens.h_X[r, :n])), (model, r)
                assert np.array_equal(bits(s.old_v()[:n]), bits(v[r, :n])), (model, r)
                assert ge.same_grid(ens.grid(r), s.grid(), n), (model, r)
