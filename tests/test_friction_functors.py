"""User-written friction functors (yalla_amd/csrc/model_functors.h: graded, ids, field) through the CPU restatement,
held BIT FOR BIT against the numpy statement of the reference's loops (tests/friction_statement.py; for
Gabriel_solver tests/gabriel_statement.py).  The two default frictions return 0 or 1 and read their ids through
`i == j` only; these are fractional, signed, asymmetric in (i, j), and read the further fields of a wide point.

The harness is test_reference_statement_numpy.py's: one take_step with dt = 0 and the lone last cell held fixed
leaves the stage's right-hand side F + sum_v / sum_friction in old_v -- here of an old_v drawn at random.
What the inputs must contain is asserted from the statement alone, before anything is compared.
The device side is tests/test_friction_functors_gpu.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import friction_statement as fs  # noqa: E402
import gabriel_statement as gab  # noqa: E402

from yalla_amd.solution import Solution  # noqa: E402

f32 = np.float32
GS = 30
COEFFICIENT = 0.8
# functor -> (point width, {solver: (model, force)})
MODELS = {
    "graded": (3, {"tile": ("friction_graded_tile", fs.relu_force),
                   "grid": ("friction_graded_fading_grid", fs.fading_spring),
                   "gabriel": ("friction_graded_gabriel", None)}),
    "ids": (3, {"tile": ("friction_ids_tile", fs.relu_force),
                "grid": ("friction_ids_grid", fs.relu_force),
                "gabriel": ("friction_ids_gabriel", None)}),
    "field": (5, {"tile": ("friction_field_tile", fs.relu_force),
                  "grid": ("friction_field_grid", fs.relu_force),
                  "gabriel": ("friction_field_gabriel", None)}),
}
PLAIN_TWINS = {"friction_ids_tile": "friction_ids_plain_tile", "friction_field_tile": "friction_field_plain_tile",
               "friction_ids_grid": "friction_ids_plain_grid", "friction_ids_gabriel": "friction_ids_plain_gabriel"}
SIZES = {"tile": 150, "grid": 260, "gabriel": 260}
SPACING = {"ids": 1.0}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def inputs(functor, solver):
    """(X, old_v): a cloud at neighbour spacing 0.75 with the lone cell last, and non-zero velocities.  For ids the
    spacing is 1.0: its mean coefficient is positive, and only cells with few neighbours have a negative sum."""
    n = SIZES[solver]
    return fs.cloud(n, MODELS[functor][0], 11, SPACING.get(functor, 0.75)), fs.velocities(n, seed=12)


def rhs_of(lib, model, X, old_v, sum_order=0, cube_size=1.0, gs=GS, params=()):
    """old_v after set_old_v(old_v) and one take_step(0) with the last cell fixed: the stage's right-hand side."""
    n = len(X)
    with Solution(model, n, gs, cube_size, lib=lib) as s:
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        if sum_order:
            s.set_param("sum_order", sum_order)
        if model.endswith("_gabriel"):
            s.set_param("gabriel_coefficient", COEFFICIENT)
        for name, value in params:
            s.set_param(name, value)
        s.set_old_v(old_v)
        s.set_fixed(n - 1)
        s.take_step(0.0, 1)
        assert same_bits(s.positions(), X)                        # dt = 0: nothing moved
        return s.old_v()[:n].copy()


@functools.lru_cache(maxsize=None)
def statement(functor, solver, sum_order=0, cube_size=1.0):
    """(what a dt = 0 step leaves in old_v, sum_friction, non-zero friction terms per cell), computed once."""
    X, v = inputs(functor, solver)
    model, force = MODELS[functor][1][solver]
    if solver == "gabriel":
        dX = gab.rhs(X, GS, COEFFICIENT, model, old_v=v)
        out = (fs.as_old_v_after_a_dt_0_step(dX, len(X) - 1), None, None)
    else:
        dX, sf, terms = fs.stage_rhs(X, v, force, fs.FRICTIONS[functor], solver, GS, cube_size, bool(sum_order))
        out = (fs.as_old_v_after_a_dt_0_step(dX, len(X) - 1), sf, terms)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def gabriel_sums(X, functor):
    """sum_friction and the number of non-zero terms per cell over the kept pairs of the Gabriel statement"""
    ids, dist, kept = gab.gabriel_lists(X, GS, COEFFICIENT)
    i = np.arange(len(X))[:, None]
    jj = np.maximum(ids, 0)
    fr = fs.FRICTIONS[functor](X[:, None, :], (X[:, None, :] - X[jj]).astype(f32), np.where(kept, dist, f32(1)), i, ids)
    fr = np.where(kept, fr, f32(0))
    return fr.astype(np.float64).sum(axis=1), (fr != 0).sum(axis=1)   # (eighths: exact in any order)


def assert_ids_sums_have_every_sign(sf, terms):
    """At least 3 cells each whose sum_friction is negative, zero made of non-zero terms, and positive; the smallest
    positive sum is 0.125 (eighths)."""
    assert (sf < 0).sum() >= 3, (sf < 0).sum()
    assert ((sf == 0) & (terms > 0)).sum() >= 3, ((sf == 0) & (terms > 0)).sum()
    assert (sf > 0).sum() >= 3
    assert sf[sf > 0].min() >= 0.125


def assert_field_pairs_on_both_sides(X):
    """At least 3 interacting pairs each with |r.theta| < 1 and > 1 (and |Xi.phi| on both sides of 1)."""
    r = X[:, None, :] - X[None, :, :]
    near = (fs.dist3(r) < 1) & ~np.eye(len(X), dtype=bool)
    assert (near & (np.abs(r[..., 3]) < 1)).sum() >= 3 and (near & (np.abs(r[..., 3]) > 1)).sum() >= 3
    assert (np.abs(X[:-1, 4]) < 1).sum() >= 3 and (np.abs(X[:-1, 4]) > 1).sum() >= 3


def check_inputs(functor, solver, sf=None, terms=None):
    X, v = inputs(functor, solver)
    assert (v[:-1] != 0).all() and (v[-1] == 0).all()
    if functor == "ids":
        if solver == "gabriel":
            sf, terms = gabriel_sums(X, functor)
        assert_ids_sums_have_every_sign(sf, terms)
    if functor == "field":
        assert_field_pairs_on_both_sides(X)
    if functor == "graded" and sf is not None:
        assert sf.min() >= 0.25 and (sf != np.round(sf)).sum() >= 3     # the self term; fractional divisors


@pytest.mark.parametrize("functor", list(MODELS))
def test_oracle_tile_rhs_is_the_statement(oracle, functor):
    want, sf, terms = statement(functor, "tile")
    check_inputs(functor, "tile", sf, terms)
    X, v = inputs(functor, "tile")
    got = rhs_of(oracle, MODELS[functor][1]["tile"][0], X, v)
    assert np.abs(want).max() > 0.1 and (want[-1] == 0).all()
    assert same_bits(got, want)


@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("functor", list(MODELS))
def test_oracle_grid_rhs_is_the_statement(oracle, functor, sum_order):
    want, sf, terms = statement(functor, "grid", sum_order)
    check_inputs(functor, "grid", sf, terms)
    X, v = inputs(functor, "grid")
    got = rhs_of(oracle, MODELS[functor][1]["grid"][0], X, v, sum_order)
    assert np.abs(want).max() > 0.1 and (want[-1] == 0).all()
    assert same_bits(got, want)


@pytest.mark.parametrize("functor", list(MODELS))
def test_oracle_grid_rhs_with_cubes_wider_than_the_friction(oracle, functor):
    """cube_size 1.5: pairs the solver lets interact (dist < 1.5) that the friction's own `dist < 1` refuses"""
    want, sf, terms = statement(functor, "grid", 0, 1.5)
    X, v = inputs(functor, "grid")
    r = X[:, None, :3] - X[None, :, :3]
    d = fs.dist3(r)
    assert ((d >= 1) & (d < 1.5)).sum() >= 6
    got = rhs_of(oracle, MODELS[functor][1]["grid"][0], X, v, 0, cube_size=1.5)
    assert same_bits(got, want)


@pytest.mark.parametrize("functor", list(MODELS))
def test_oracle_gabriel_rhs_is_the_statement(oracle, functor):
    want, _, _ = statement(functor, "gabriel")
    check_inputs(functor, "gabriel")
    X, v = inputs(functor, "gabriel")
    got = rhs_of(oracle, MODELS[functor][1]["gabriel"][0], X, v)
    assert np.abs(want).max() > 0.1 and (want[-1] == 0).all()
    assert same_bits(got, want)


@pytest.mark.parametrize("model,twin", sorted(PLAIN_TWINS.items()))
def test_oracle_plain_twins_are_the_same_numbers(oracle, model, twin):
    """The `_plain` names differ from the declared ones only in what the device may do with them."""
    functor = model.split("_")[1]
    solver = model.split("_")[-1]
    X, v = inputs(functor, solver)
    assert same_bits(rhs_of(oracle, model, X, v), rhs_of(oracle, twin, X, v))


def test_the_frictions_differ_from_the_defaults():
    """What the statement's three frictions are that friction_w_neighbour is not: fractional, signed and
    asymmetric in (i, j), and dependent on the further fields."""
    X, _ = inputs("field", "grid")
    i, j = np.array([3, 5, 8, 8]), np.array([5, 3, 9, 8])
    r = (X[i] - X[j]).astype(f32)
    d = np.full(4, f32(0.5))
    assert list(fs.ids(X[i], r, d, i, j)) == [0.125 * (((5 * a + 2 * b) & 7) - 2) for a, b in zip(i, j)]
    assert fs.ids(X[i], r, d, i, j)[0] != fs.ids(X[i], r, d, i, j)[1]
    assert fs.ids(X[i], r, d, i + 3, j + 3)[0] != fs.ids(X[i], r, d, i, j)[0]          # an id offset of 3 shows
    assert (fs.ids(X[i], r, d, i + 8, j + 16) == fs.ids(X[i], r, d, i, j)).all()       # one of 8 does not
    assert list(fs.graded(X[i], r, d, i, j)) == [0.5, 0.5, 0.5, 0.25]
    swapped = fs.field(X[j], -r, d, j, i)
    assert fs.field(X[i], r, d, i, j)[3] == 0 and (fs.field(X[i], r, d, i, j)[:3] != swapped[:3]).any()
