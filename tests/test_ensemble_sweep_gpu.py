"""A time step and a Gabriel coefficient per replica (ya::ens::Replica_dt, Ensemble<Pt, Gabriel_solver>::
d_gabriel_coefficients; SweepEnsemble over libyalla_ensemble_sweep.so) on every path of the three forms.

THE REFERENCE is always a lone Solution("<model>_<form>") per compared replica from libyalla_models.so, stepped with
that replica's values: positions, old_v[:n] and -- forms "grid" and "gabriel" -- the four grid arrays, compared as bit
patterns (uint32, array_equal), never with a tolerance; the status of every replica is 0.  Every case that expects
launches from LDS asserts the launch count and the lanes that ran."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ensemble_grid_links_support import box_rows  # noqa: E402
from ensemble_support import bits, same_grid  # noqa: E402

from yalla_amd import SweepEnsemble  # noqa: E402
from yalla_amd.ensemble import Ensemble, GabrielEnsemble, GabrielLdsEnsemble, GridEnsemble  # noqa: E402
from yalla_amd.solution import Solution  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
GS = 10  # the grid forms' grid_size; the rows lie well inside it
FORMS = ["tile", "grid", "gabriel"]
MODELS = {"tile": ["relu", "springs", "relu_po"], "grid": ["relu", "springs", "relu_po"],
          "gabriel": ["relu", "relu_plain", "relu_po"]}
LINKED = {"tile": "links", "grid": "springs_links"}
N_FLOATS = {"relu_po": 5}
LDS_PARAM = {"tile": "whole_steps", "grid": "lds_steps", "gabriel": "lds_steps"}
LANES_PARAM = {"tile": "whole_step_lanes", "grid": "lds_step_lanes"}

# 2 update blocks per replica (n_max = 300): an index by block instead of by replica shows
N_MAX = 300
COUNTS = [0, 1, 37, 256, 300]
POINT_COUNTS = [5, 64, 37, 256, 300]  # (the point modes: cell 0 exists everywhere)
# no non-zero value is a power-of-two multiple of another: a swapped index changes bits
DTS = np.array([0.05, 0.1, 0.013, 0.2, 0.0], f32)
FIXED = {"com": lambda s: s.set_fixed(), "point": lambda s: s.set_fixed(0), "point_xy": lambda s: s.set_fixed_xy(0)}


def grid_args(form):
    return () if form == "tile" else (GS, 1.0)


def rows_of(model, counts, seed=0, shrink=0.45):
    """Seeded rows in a box around the origin, about three cells per unit volume at 300 cells."""
    return [box_rows(n, N_FLOATS.get(model, 3), GS, 100 * seed + 7 * r + 1, shrink) for r, n in enumerate(counts)]


def sweep(form, model, rows, n_max=N_MAX, slots=0, coefficient=0.8, **params):
    ens = SweepEnsemble(form, model, len(rows), n_max, slots, GS, 1.0, coefficient)
    for name, value in params.items():
        ens.set_param(name, value)
    load(ens, rows)
    return ens


def load(ens, rows):
    """The rows, the counts and a zero old_v: the state every run starts from."""
    ens.h_X[:] = f32(-7.25)
    for r, X in enumerate(rows):
        ens.h_X[r, :len(X)] = X
        ens.h_n[r] = len(X)
    ens.copy_to_device()
    ens.set_old_v(np.zeros((ens.n_replicas, ens.n_max, 3), f32))


def state(ens, counts, replicas=None, grids=None):
    """Per replica: (positions, old_v[:n], grid arrays or None), after every status was seen to be 0."""
    grids = getattr(ens, "form", None) in ("grid", "gabriel") if grids is None else grids
    if grids:
        assert [ens.status(r, clear=False) for r in range(len(counts))] == [0] * len(counts)
    ens.copy_to_host()
    v = ens.old_v()
    out = {}
    for r in range(len(counts)) if replicas is None else replicas:
        n = counts[r]
        assert ens.h_n[r] == n
        out[r] = (bits(ens.h_X[r, :n]).copy(), bits(v[r, :n]).copy(), ens.grid(r) if grids else None)
    return out


def same(got, want, counts, what=""):
    for r, (X, v, grid) in want.items():
        assert np.array_equal(got[r][0], X), (what, "positions of replica", r)
        assert np.array_equal(got[r][1], v), (what, "old_v of replica", r)
        assert grid is None or same_grid(got[r][2], grid, counts[r]), (what, "grid arrays of replica", r)


def differ(a, b):
    return not np.array_equal(a[0], b[0])


def lone(form, model, X, n_max, segments, coefficient=None, fixed="com", links=None):
    """A lone Solution of the rows X stepped through `segments` [(dt, steps), ...]: (positions, old_v, grid)."""
    with Solution(f"{model}_{form}", n_max, *grid_args(form)) as s:
        s.h_X[:len(X)] = X
        s.h_n = len(X)
        s.copy_to_device()
        if coefficient is not None:
            s.set_param("gabriel_coefficient", float(coefficient))
        if links is not None and len(links):
            s.set_links(links, 0.2)
        FIXED[fixed](s)
        for dt, steps in segments:
            s.take_step(float(f32(dt)), steps)
        X1 = bits(s.positions()).copy()
        assert s.h_n == len(X)
        return X1, bits(s.old_v()[:len(X)]).copy(), None if form == "tile" else s.grid()


@functools.lru_cache(maxsize=None)
def reference(form, model, fixed="com", steps=3):
    """Once per (form, model, fixed mode, step count): the M lone Solutions, replica r stepped with DTS[r]."""
    counts = COUNTS if fixed == "com" else POINT_COUNTS
    rows = rows_of(model, counts)
    return {r: lone(form, model, X, N_MAX, [(DTS[r], steps)], fixed=fixed) for r, X in enumerate(rows)}


def test_the_references_tell_replicas_and_time_steps_apart():
    want = reference("tile", "relu")
    other = lone("tile", "relu", rows_of("relu", COUNTS)[3], N_MAX, [(DTS[2], 3)])
    assert differ(want[3], other), "another replica's dt gives other bits"
    assert np.array_equal(want[4][0], bits(rows_of("relu", COUNTS)[4])), "dt = 0 leaves the positions"
    assert want[4][1].any(), "... and old_v is written all the same"


# ---- dt, launch-sequence paths ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", list(FIXED))
@pytest.mark.parametrize("form,model", [(form, model) for form in FORMS for model in MODELS[form]])
def test_launch_sequence(form, model, fixed):
    """The 6-, 14- and 16-launch steps: K = 3 steps, replica r with DTS[r], every model, every fixed mode."""
    counts = COUNTS if fixed == "com" else POINT_COUNTS
    with sweep(form, model, rows_of(model, counts)) as ens:
        FIXED[fixed](ens)
        ens.dt = DTS
        ens.take_step(steps=3)
        assert ens.lds_launches == 0 and ens.lanes_used == 0
        same(state(ens, counts), reference(form, model, fixed), counts, (form, model, fixed))


# ---- dt, LDS paths ---------------------------------------------------------------------------------------------------
def lds_cases():
    for form in ("tile", "grid"):
        for lanes in (1, 4, 16, 64):
            yield form, "relu", lanes
        for model in MODELS[form][1:]:
            yield form, model, 1
    for model in MODELS["gabriel"]:
        yield "gabriel", model, 1


@pytest.mark.parametrize("form,model,lanes", list(lds_cases()))
def test_steps_from_lds(form, model, lanes):
    """The same from LDS: K = 5 steps with steps_per_launch = 2, so three launches; the lanes asked for ran.  The
    Gabriel form with n_max = 100: several rounds of 16 cells."""
    n_max = 100 if form == "gabriel" else N_MAX
    counts = [0, 1, 37, 100, 64] if form == "gabriel" else COUNTS
    rows = rows_of(model, counts, shrink=0.3 if form == "gabriel" else 0.45)
    params = {LDS_PARAM[form]: 1, "steps_per_launch": 2}
    if form != "gabriel":
        params[LANES_PARAM[form]] = lanes
    with sweep(form, model, rows, n_max, **params) as ens:
        ens.dt = DTS
        ens.take_step(steps=5)
        assert ens.lds_launches == 3 and ens.lanes_used == lanes
        got = state(ens, counts)
    if form == "gabriel":
        want = {r: lone(form, model, X, n_max, [(DTS[r], 5)]) for r, X in enumerate(rows)}
    else:
        want = reference(form, model, steps=5)
    same(got, want, counts, (form, model, lanes))


@pytest.mark.parametrize("fixed", ["point", "point_xy"])
@pytest.mark.parametrize("form", FORMS)
def test_the_point_modes_from_lds(form, fixed):
    with sweep(form, "relu", rows_of("relu", POINT_COUNTS), **{LDS_PARAM[form]: 1}) as ens:
        FIXED[fixed](ens)
        ens.dt = DTS
        ens.take_step(steps=3)
        assert ens.lds_launches == 1
        same(state(ens, POINT_COUNTS), reference(form, "relu", fixed), POINT_COUNTS, (form, fixed))


# ---- dt, links -------------------------------------------------------------------------------------------------------
SLOTS = 4
LINK_COUNTS = [0, 1, 37, 256, 300]


def chain(n):
    """Up to three links of a chain: a cell has at most two terms, whose sum does not depend on their order (the lone
    Solution adds them with atomics)."""
    return np.array([(0, 1), (2, 1), (2, 3)][:max(min(n - 1, 3), 0)], np.int64).reshape(-1, 2)


@pytest.mark.parametrize("lanes", [1, 16])
@pytest.mark.parametrize("form", list(LINKED))
def test_links(form, lanes):
    """The linked models, S = 4 slots per replica: from LDS and outside, the same object, against each other and against
    lone Solutions with the same links."""
    model = LINKED[form]
    rows = rows_of(model, LINK_COUNTS)
    with sweep(form, model, rows, slots=SLOTS) as ens:
        for r, n in enumerate(LINK_COUNTS):
            ens.h_link[r, :len(chain(n))] = chain(n) + r * N_MAX
        ens.copy_to_device()
        ens.dt = DTS
        ens.take_step(steps=3)
        assert ens.lds_launches == 0
        outside = state(ens, LINK_COUNTS)
        load(ens, rows)
        ens.set_param(LDS_PARAM[form], 1)
        ens.set_param(LANES_PARAM[form], lanes)
        ens.take_step(steps=3)
        assert ens.lds_launches == 1 and ens.lanes_used == lanes
        inside = state(ens, LINK_COUNTS)
    want = {r: lone(form, model, X, N_MAX, [(DTS[r], 3)], links=chain(len(X))) for r, X in enumerate(rows)}
    same(outside, want, LINK_COUNTS, (form, "outside"))
    same(inside, want, LINK_COUNTS, (form, "from LDS"))
    bare = lone(form, model, rows[2], N_MAX, [(DTS[2], 3)])
    assert differ(want[2], bare), "the links did something"


# ---- one more replica than a wavefront has lanes, four times over -----------------------------------------------------
MANY, MANY_N_MAX = 257, 20
MANY_DTS = (f32(0.01) + np.arange(MANY, dtype=f32) * f32(2.0 ** -10)).astype(f32)
MANY_CHECKED = sorted(set(range(0, MANY, 16)) | {MANY - 1})


def many_rows():
    return [box_rows(MANY_N_MAX - r % 3, 3, GS, 5000 + r, 0.2) for r in range(MANY)]


@functools.lru_cache(maxsize=None)
def many_reference(form):
    rows = many_rows()
    return {r: lone(form, "relu", rows[r], MANY_N_MAX, [(MANY_DTS[r], 3)]) for r in MANY_CHECKED}


@pytest.mark.parametrize("form,lds", [("tile", -1), ("tile", 1), ("grid", 1)])
def test_257_replicas(form, lds):
    assert len(set(MANY_DTS.tolist())) == MANY
    rows = many_rows()
    counts = [len(X) for X in rows]
    with sweep(form, "relu", rows, MANY_N_MAX, **{LDS_PARAM[form]: lds}) as ens:
        ens.dt = MANY_DTS
        ens.take_step(steps=3)
        assert ens.lds_launches == (1 if lds > 0 else 0)
        same(state(ens, counts, MANY_CHECKED), many_reference(form), counts, (form, lds))


# ---- the coefficient --------------------------------------------------------------------------------------------------
COEFFICIENTS = np.array([0.5, 0.8, 1.0, 0.8], f32)  # tests/test_ensemble_gabriel_lds_steps_gpu.py's three and a repeat
COEFFICIENT_DTS = np.array([0.05, 0.013, 0.1, 0.02], f32)
BALLS_GS = 16


def four_balls():
    """Four of that file's balls: cells with 16, 64, 65 and 129 candidates (<= 64: the lists; > 64: the dense path)."""
    from test_ensemble_gabriel_lds_steps_gpu import balls
    by_size = {}
    for X in balls():
        by_size.setdefault(len(X), X)
    return [np.array(by_size[K + 1]) for K in (16, 64, 65, 129)]


@pytest.mark.parametrize("lds", [-1, 1])
def test_a_coefficient_and_a_time_step_per_replica(lds):
    rows = four_balls()
    counts = [len(X) for X in rows]
    ens = SweepEnsemble("gabriel", "relu", 4, 130, 0, BALLS_GS, 1.0, 0.123)  # (the scalar is ignored)
    with ens:
        ens.set_param("lds_steps", lds)
        load(ens, rows)
        ens.gabriel_coefficients = COEFFICIENTS
        ens.dt = COEFFICIENT_DTS
        ens.take_step(steps=3)
        assert ens.lds_launches == (1 if lds > 0 else 0)
        assert (ens.lds_dense_cells() if lds > 0 else ens.dense_cells()) > 0, "cells with more than 64 candidates"
        got = state(ens, counts)
    want = {}
    for r, X in enumerate(rows):
        with Solution("relu_gabriel", 130, BALLS_GS, 1.0) as s:
            s.h_X[:len(X)] = X
            s.h_n = len(X)
            s.copy_to_device()
            s.set_param("gabriel_coefficient", float(COEFFICIENTS[r]))
            s.take_step(float(COEFFICIENT_DTS[r]), 3)
            want[r] = (bits(s.positions()).copy(), bits(s.old_v()[:len(X)]).copy(), s.grid())
            if r == 3:  # the repeat's coefficient, this replica's rows: not what another coefficient gives
                s.h_X[:len(X)] = X
                s.copy_to_device()
                s.set_old_v(np.zeros((130, 3), f32))
                s.set_param("gabriel_coefficient", 0.5)
                s.take_step(float(COEFFICIENT_DTS[r]), 3)
                assert not np.array_equal(bits(s.positions()), want[r][0]), "the coefficient matters here"
    same(got, want, counts, lds)


# ---- equal values are the scalar path ---------------------------------------------------------------------------------
EXISTING = {("tile", -1): Ensemble, ("tile", 1): Ensemble, ("grid", -1): GridEnsemble, ("grid", 1): GridEnsemble,
            ("gabriel", -1): GabrielEnsemble, ("gabriel", 1): GabrielLdsEnsemble}


@pytest.mark.parametrize("lds", [-1, 1])
@pytest.mark.parametrize("form", FORMS)
def test_equal_values_are_the_scalar_path(form, lds):
    """An array of M equal values: the bits and the launch counts of the scalar call on the same object; and with no
    array the object is the existing class of its form."""
    n_max = 100 if form == "gabriel" else N_MAX
    counts = [0, 1, 37, 100, 64] if form == "gabriel" else COUNTS
    rows = rows_of("relu", counts, shrink=0.3 if form == "gabriel" else 0.45)
    with sweep(form, "relu", rows, n_max, **{LDS_PARAM[form]: lds}) as ens:
        ens.take_step(0.05, 3)
        scalar, launches = state(ens, counts), ens.lds_launches
        assert launches == (1 if lds > 0 else 0)
        load(ens, rows)
        ens.dt = np.full(len(counts), 0.05, f32)
        ens.take_step(steps=3)
        assert ens.lds_launches - launches == launches
        same(state(ens, counts), scalar, counts, "an array of equal values")
        load(ens, rows)
        ens.dt = None
        ens.take_step(0.05, 3)
        same(state(ens, counts), scalar, counts, "the array cleared")
    existing = EXISTING[form, lds](*(("relu", len(counts), n_max) + grid_args(form)))
    with existing:
        if lds > 0:
            existing.set_param(LDS_PARAM[form], 1)
        load(existing, rows)
        existing.take_step(0.05, 3)
        same(state(existing, counts, grids=form != "tile"), scalar, counts, "the existing class")


# ---- independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [-1, 1])
@pytest.mark.parametrize("form", FORMS)
def test_replicas_are_independent(form, lds):
    """All replicas start from the same rows: changing only dt[2] changes replica 2 and no other; distinct values give
    pairwise distinct positions."""
    n = 60
    rows = [box_rows(n, 3, GS, 77, 0.25)] * 5
    dts = np.array([0.05, 0.1, 0.013, 0.2, 0.07], f32)
    with sweep(form, "relu", rows, 64, **{LDS_PARAM[form]: lds}) as ens:
        ens.dt = dts
        ens.take_step(steps=3)
        first = state(ens, [n] * 5)
        load(ens, rows)
        dts[2] = 0.03
        ens.dt = dts
        ens.take_step(steps=3)
        second = state(ens, [n] * 5)
    for r in range(5):
        assert differ(first[r], second[r]) == (r == 2), r
        for q in range(r):
            assert differ(first[r], first[q]), (r, q)


# ---- the array changes on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [-1, 1])
@pytest.mark.parametrize("form", FORMS)
def test_the_array_is_scaled_on_the_device_between_two_calls(form, lds):
    """take_step(steps=2), scale_dt(0.5), take_step(steps=2), no synchronise in between: lone Solutions stepped twice
    with dt[r] and twice with 0.5f * dt[r]."""
    n_max = 100 if form == "gabriel" else N_MAX
    counts = [0, 1, 37, 100, 64] if form == "gabriel" else COUNTS
    rows = rows_of("relu", counts, shrink=0.3 if form == "gabriel" else 0.45)
    with sweep(form, "relu", rows, n_max, **{LDS_PARAM[form]: lds}) as ens:
        ens.dt = DTS
        ens.take_step(steps=2)
        ens.scale_dt(0.5)
        ens.take_step(steps=2)
        assert ens.lds_launches == (2 if lds > 0 else 0)
        assert np.array_equal(ens.dt, DTS), "dt reads back what was set"
        got = state(ens, counts)
    want = {r: lone(form, "relu", X, n_max, [(DTS[r], 2), (f32(0.5) * DTS[r], 2)]) for r, X in enumerate(rows)}
    same(got, want, counts, (form, lds))
    unscaled = lone(form, "relu", rows[3], n_max, [(DTS[3], 4)])
    assert differ(want[3], unscaled)
