"""Ensembles of points of 4 to 16 floats with EVERY field coupled, on the GPU: models::field_coupling through the
all-pairs, the grid and the Gabriel form (yalla_amd/libyalla_ensemble_widths.so, libyalla_ensemble_grid_widths.so,
libyalla_ensemble_gabriel_lds_widths.so: yalla_amd/csrc/ensemble_widths_models.h), by the launch sequences and by the
launches that step from LDS, at the sizes where each type's LDS capacity, term buffer and dense sets change.

Every replica is compared with TWO references, bit for bit and field by field (a failure names the field), positions,
old_v[:n], h_n / get_d_n and, in the grid and Gabriel forms, the four grid arrays and the status:
  (a) a lone Solution("fields_<type>_<solver>") of libyalla_models_widths.so fed the same rows, and
  (b) the widths oracle's Solution in the engine's reduce order -- the comparison that does not pass through device
      code shared by the ensemble and the lone solvers.
No tolerance anywhere.  Every test seeds a non-zero old_v, asserts through the counters which path ran, and asserts
that the extra fields moved.  The shapes come from the restated LDS rule (tests/test_ensemble_widths.py), not from
trial."""
import numpy as np
import pytest

import ensemble_widths_support as ew
import widths_support as ws
from ensemble_support import bits
from ensemble_widths_support import Widths, capacity_of, lanes_expected, rows_of, seeded_old_v

pytestmark = pytest.mark.gpu

f32 = np.float32
DT = 0.05
GS = 12          # a 12^3 grid around the origin holds seeded_rows' 1025 cells (radius 4.4)
LANES = (1, 4, 16, 64, 0)
# Counts mixed in one ensemble: the edges of the up to four partial sums and of the fold.  The small mix leaves the
# engine's own lane choice several lanes (n_max <= 64) and has room for every term buffer; in the large one w16's four
# lanes have none.
SMALL, SMALL_N_MAX = [0, 1, 2, 63, 64], 64
LARGE, LARGE_N_MAX = [65, 255, 256, 257, 0, 1], 257
MIXES = {"small": (SMALL, SMALL_N_MAX), "large": (LARGE, LARGE_N_MAX)}
# all-pairs: an (n_max, lanes) with room for the term buffer and the next n_max, without (the restated rule's edges)
TILE_ROOM = {"w11": ((467, 4), (468, 4)), "w16": ((232, 4), (233, 4))}

PATH = {"tile": ("whole_steps", "whole_step_lanes"), "grid": ("lds_steps", "lds_step_lanes")}


def lane_variants(form, lanes=LANES):
    """The launch sequence, and one ensemble per lanes setting that steps from LDS."""
    on, lanes_name = PATH[form]
    variants = {"launches": {on: -1}}
    for setting in lanes:
        variants["lanes %d" % setting] = {on: 1, lanes_name: setting}
    return variants


def mix_rows(kind, counts, seed):
    return [rows_of(kind, n, 100 * seed + r) for r, n in enumerate(counts)]


def step_and_check(run, form, kind, n_max, dt, steps, what, lanes=LANES, from_lds=True):
    run.each(lambda s: s.take_step(dt, steps))
    run.expect("launches", 0)
    for setting in lanes:
        name = "lanes %d" % setting
        if name in run.variant:
            run.expect(name, 1 if from_lds else 0, lanes_expected(form, kind, n_max, setting) if from_lds else None)
    run.check(what)
    run.extras_moved(dt)


# ---- the all-pairs and the grid form: counts, lanes -----------------------------------------------------------------
@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("kind", ew.TYPES["tile"])
def test_tile_counts_and_lanes(kind, mix):
    """The six-launch step and whole steps with 1, 4, 16, 64 lanes per cell and the engine's choice."""
    counts, n_max = MIXES[mix]
    run = Widths("tile", kind, mix_rows(kind, counts, 1), n_max, lane_variants("tile"),
                 old_v=seeded_old_v(len(counts), n_max))
    try:
        step_and_check(run, "tile", kind, n_max, DT, 3, mix)
        if mix == "small":
            assert ew.lanes_used(run.variant["lanes 0"], "tile") == (1 if kind in ws.UNDECLARED else 4)
        elif kind == "w16":
            assert ew.lanes_used(run.variant["lanes 4"], "tile") == 1      # no room: it says so
    finally:
        run.close()


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("kind", ew.TYPES["grid"])
def test_grid_counts_and_lanes(kind, mix, sum_order):
    """The 14-launch step and steps from LDS with 1, 4, 16, 64 lanes per cell and the engine's choice, in both orders."""
    counts, n_max = MIXES[mix]
    run = Widths("grid", kind, mix_rows(kind, counts, 2), n_max, lane_variants("grid"), grid_size=GS,
                 old_v=seeded_old_v(len(counts), n_max), sum_order=sum_order)
    try:
        step_and_check(run, "grid", kind, n_max, DT, 3, (mix, sum_order))
        if mix == "small":
            assert ew.lanes_used(run.variant["lanes 0"], "grid") == (1 if kind in ws.UNDECLARED else 4)
    finally:
        run.close()


# ---- capacities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ew.TYPES["tile"])
def test_tile_capacity_and_one_more(kind):
    """One full replica of whole_step_capacity rows beside a small one: whole steps.  One row more: the same bits from
    the six launches, and whole_step_launches stays 0."""
    capacity = capacity_of("tile", kind)
    for n_max, from_lds in ((capacity, True), (capacity + 1, False)):
        rows = [rows_of(kind, n_max, 31), rows_of(kind, 70, 32)]
        run = Widths("tile", kind, rows, n_max, lane_variants("tile", (1, 0)), old_v=seeded_old_v(2, n_max))
        try:
            step_and_check(run, "tile", kind, n_max, DT, 2, n_max, (1, 0), from_lds)
        finally:
            run.close()


@pytest.mark.parametrize("kind", ["w11", "w16"])
def test_tile_term_buffer_with_and_without_room(kind):
    """The last n_max at which four lanes' term buffer fits, and the next: that launch runs one lane and says so."""
    for (n_max, lanes), room in zip(TILE_ROOM[kind], (True, False)):
        assert ew.has_room("tile", kind, n_max, lanes) == room
        rows = [rows_of(kind, n_max, 41), rows_of(kind, 33, 42)]
        run = Widths("tile", kind, rows, n_max, lane_variants("tile", (lanes,)), old_v=seeded_old_v(2, n_max))
        try:
            step_and_check(run, "tile", kind, n_max, DT, 2, (n_max, lanes), (lanes,))
            assert ew.lanes_used(run.variant["lanes %d" % lanes], "tile") == (lanes if room else 1)
        finally:
            run.close()


@pytest.mark.parametrize("kind", ew.TYPES["grid"])
def test_grid_capacity_and_one_more(kind):
    """grid_lds_capacity rows (w16: 512, one more lays out 1024 keys; w8: 1024 rows leave no room for any term
    buffer) and one more, which the 14 launches step."""
    capacity = capacity_of("grid", kind)
    for n_max, from_lds in ((capacity, True), (capacity + 1, False)):
        rows = [rows_of(kind, n_max, 51), rows_of(kind, 70, 52)]
        run = Widths("grid", kind, rows, n_max, lane_variants("grid", (1, 64)), grid_size=GS,
                     old_v=seeded_old_v(2, n_max))
        try:
            step_and_check(run, "grid", kind, n_max, DT, 2, n_max, (1, 64), from_lds)
            if from_lds and kind in ("w8", "w16"):
                assert ew.lanes_used(run.variant["lanes 64"], "grid") == 1
        finally:
            run.close()


# ---- the grid form: one dense replica among sparse ones --------------------------------------------------------------
@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("kind", ew.TYPES["grid"])
def test_grid_a_dense_replica_among_sparse_ones(kind, sum_order):
    """400 cells inside one cube (a ball of radius 0.45): 400 hits per cell, far beyond 96, and a plane of 400 cells,
    beyond the type's stage capacity of 256 or 176."""
    n_dense, n_max = 400, 400
    assert n_dense > ws.STAGE_CAPACITY[kind] and n_max <= capacity_of("grid", kind)
    rows = [rows_of(kind, 90, 61), rows_of(kind, n_dense, 62, positions=ew.ball(n_dense, (0.5, 0.5, 0.5), 63)),
            rows_of(kind, 0, 64), rows_of(kind, 200, 65)]
    lanes = (1, 16, 0)
    run = Widths("grid", kind, rows, n_max, lane_variants("grid", lanes), grid_size=GS, old_v=seeded_old_v(4, n_max),
                 sum_order=sum_order)
    try:
        step_and_check(run, "grid", kind, n_max, 0.0005, 2, ("dense", sum_order), lanes)
    finally:
        run.close()


# ---- the Gabriel form --------------------------------------------------------------------------------------------------
GABRIEL = {"launches": {"lds_steps": -1}, "lds": {"lds_steps": 1}}


def gabriel_step_and_check(run, dt, steps, what, from_lds=True, dense=None):
    run.each(lambda s: s.take_step(dt, steps))
    run.expect("launches", 0)
    run.expect("lds", 1 if from_lds else 0)
    assert run.variant["launches"].lds_dense_cells() == 0
    if dense is not None:
        assert (run.variant["lds"].lds_dense_cells() > 0) == (dense and from_lds), what
    run.check(what)
    run.extras_moved(dt)


@pytest.mark.parametrize("kind", ew.TYPES["gabriel"])
def test_gabriel_candidates_around_the_list_s_64(kind):
    """Balls of 63, 64, 65 and 66 candidates per cell, in one cube and around a corner (the replicas of
    tests/test_ensemble_gabriel_lds_steps_gpu.py that straddle the 64-entry list): the 16-launch step and lds_steps."""
    from test_ensemble_gabriel_lds_steps_gpu import BALLS_GS, balls
    chosen = [X for X in balls() if len(X) - 1 in (63, 64, 65, 66)]
    assert len(chosen) == 8
    n_max = 67
    rows = [rows_of(kind, len(X), 70 + r, positions=X) for r, X in enumerate(chosen)]
    run = Widths("gabriel", kind, rows, n_max, GABRIEL, grid_size=BALLS_GS, old_v=seeded_old_v(8, n_max))
    try:
        run.each(lambda s: s.set_fixed(0))      # (the lone cell, as in that file)
        gabriel_step_and_check(run, DT, 3, "balls", dense=True)
    finally:
        run.close()


def set_sizes(kind):
    _, _, capacity, two, one = ew.CAPACITY[kind]
    return [two - 1, two, one - 1, one, capacity, capacity + 1]


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("kind", ew.TYPES["gabriel"])
def test_gabriel_dense_cells_where_the_sets_change(kind, which):
    """n_max one below and at the change of the dense sets from 4 to 2 and from 2 to 1, at the capacity, and one above
    it (the 16 launches): a ball of 70 cells, each with 70 candidates, among sparse cells that fill the replica."""
    n_max = set_sizes(kind)[which]
    from_lds = n_max <= capacity_of("gabriel", kind)
    X = rows_of(kind, n_max, 81)
    X[:70, :3] = ew.ball(70, (8.5, 8.5, 8.5), 82)
    rows = [X, rows_of(kind, 40, 83)]
    run = Widths("gabriel", kind, rows, n_max, GABRIEL, grid_size=30, old_v=seeded_old_v(2, n_max))
    try:
        gabriel_step_and_check(run, 0.001, 2, n_max, from_lds, dense=True)
        if not from_lds:
            assert run.variant["lds"].dense_cells() > 0      # (the 16-launch path's dense kernel did them)
    finally:
        run.close()


# ---- every form: the fixed modes ---------------------------------------------------------------------------------------
FIXED_CASES = [("tile", "w6"), ("tile", "w16"), ("grid", "w9"), ("grid", "w16"), ("gabriel", "w6"), ("gabriel", "w16")]


@pytest.mark.parametrize("form,kind", FIXED_CASES)
def test_fixed_modes(form, kind):
    """The default centre-of-mass fix, set_fixed(i), set_fixed_xy(i) and back: with field_coupling the extra fields'
    right-hand sides have a mean, so every column of the fold carries values."""
    counts, n_max = [65, 0, 150, 5], 150
    variants = GABRIEL if form == "gabriel" else lane_variants(form, (1, 16))
    run = Widths(form, kind, mix_rows(kind, counts, 9), n_max, variants, grid_size=GS, old_v=seeded_old_v(4, n_max))
    try:
        for mode, call in (("centre of mass", None), ("set_fixed(4)", lambda s: s.set_fixed(4)),
                           ("set_fixed_xy(2)", lambda s: s.set_fixed_xy(2)), ("back", lambda s: s.set_fixed())):
            if call:
                run.each(call)
            if form == "gabriel":
                gabriel_step_and_check(run, DT, 2, mode)
            else:
                step_and_check(run, form, kind, n_max, DT, 2, mode, (1, 16))
    finally:
        run.close()


# ---- every form: replicas are independent ------------------------------------------------------------------------------
def stepped(form, kind, rows, n_max):
    """Every row of the positions and of old_v after 3 steps from LDS."""
    path, _, _, _, cls, _ = ew.FORMS[form]
    args = () if form == "tile" else (GS, 1.0)
    with cls(ew.model(kind), len(rows), n_max, *args, lib=ew.lib_of(form)) as ens:
        for r, X in enumerate(rows):
            ens.h_X[r, :len(X)] = X
            ens.h_n[r] = len(X)
        ens.copy_to_device()
        ens.set_old_v(seeded_old_v(len(rows), n_max))
        ens.set_param("whole_steps" if form == "tile" else "lds_steps", 1)
        if form != "gabriel":
            ens.set_param(PATH[form][1], 16)
        ens.take_step(DT, 3)
        assert (ens.whole_step_launches if form == "tile" else ens.lds_step_launches) == 1
        if form != "gabriel":
            assert ew.lanes_used(ens, form) == 16
        ens.copy_to_host()
        return bits(ens.h_X).copy(), bits(ens.old_v()).copy()


@pytest.mark.parametrize("form", list(ew.FORMS))
def test_replicas_are_independent(form):
    """One replica's rows perturbed, extra fields included: no bit of any other replica changes."""
    kind, counts, n_max = "w16", [65, 100, 3, 0, 100], 100
    rows = mix_rows(kind, counts, 11)
    before = stepped(form, kind, rows, n_max)
    other = list(rows)
    other[1] = (rows[1] * f32(1.01)).astype(f32)
    after = stepped(form, kind, other, n_max)
    for r in range(len(counts)):
        same = np.array_equal(before[0][r], after[0][r]) and np.array_equal(before[1][r], after[1][r])
        assert same == (r != 1), r
    n = counts[1]
    assert (after[0][1, :n, 3:] != bits(other[1][:, 3:])).any(axis=0).all()     # the extra fields moved
