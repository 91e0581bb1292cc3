"""Gabriel_solver as named models (relu_gabriel, clipped_gabriel, wall_gabriel; relu_plain_gabriel, whose
functor is not declared stateless; count_gabriel, the reference KAT's neighbour counter; relu_po_gabriel and
relu_cell_gabriel, the wide point types): the reference's KAT on the independent numpy statement
(gabriel_statement.py), and the CPU restatement held bit for bit against that statement -- single right-hand
sides through the dt = 0 / fixed-lone-cell trick of test_reference_statement_numpy.py, and whole Heun steps.
The device side is test_gabriel_gpu.py and test_gabriel_bodies_gpu.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gabriel_statement as gab  # noqa: E402

from yalla_amd.solution import Solution, YallaError  # noqa: E402

f32 = np.float32


def with_lone_cell(X, at=None):
    """X plus one cell far from all others (and from the wall plane): held fixed, its force is exactly 0."""
    lone = np.array(at if at is not None else X.max(axis=0) + 3.0, f32)
    return np.vstack([X, lone[None]]).astype(f32) + f32(0)   # (no -0: a dt = 0 step makes it +0)


def hexagon():
    return with_lone_cell(gab.regular_hexagon(19), (1.8, 1.8, 1.8)), 5


def lattice():
    """regular_rectangle-like lattice of spacing 0.5: full of exactly tied distances."""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    return with_lone_cell((g * 0.5 - 1.5).astype(f32), (4.2, 4.2, 4.2)), 12


def random_260():
    rng = np.random.default_rng(3)
    n = 259
    X = (rng.random((n, 3)) * 4.6 - 2.3).astype(f32)
    X[: n // 3] = (rng.random((n // 3, 3)) * 2.0 - 1.0).astype(f32)
    return with_lone_cell(X, (9.5, 8.5, 7.5)), 30


CLUSTER_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def _clusters(max_k):
    rng = np.random.default_rng(64)
    sites = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    sites = sites[rng.permutation(len(sites))]
    X, size = [], []
    for c, (K, corner) in enumerate((K, corner) for K in CLUSTER_SIZES for corner in (False, True)):
        centre = 3.0 * sites[c] + (0.0 if corner else 0.5)
        v = rng.standard_normal((K, 3))
        v *= (0.45 * rng.random(K) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
        if K <= max_k:                                         # (the draws do not depend on max_k)
            X.append(centre + v)
            size += [K] * K
    X, size = np.vstack(X).astype(f32), np.array(size)
    perm = rng.permutation(len(X))                              # ids are permuted
    lone = 3.0 * sites[2 * len(CLUSTER_SIZES)] + 0.5            # a free site: 2.5 or more from every centre
    X, size = with_lone_cell(X[perm], lone), np.append(size[perm], 1)
    X.setflags(write=False)
    size.setflags(write=False)
    return X, size


def clusters(max_k=257):
    """One ball of K cells (radius 0.45: every pair closer than 1) for each K of CLUSTER_SIZES <= max_k, once
    around a cube's centre (one cube) and once around a cube's corner (8 cubes: candidates come in through all
    stencil rows), the centres 2.5 or more apart: a cell's candidates are exactly its cluster, so K is its
    candidate count -- 63 / 64 | 65 / 66 on either side of the LDS list's capacity, the lane groups' 15 / 16 /
    17 ..., the dense kernel's 64-lane chunks 127 / 128 / 129, 255 / 256 / 257.  3426 cells and the lone one."""
    return _clusters(max_k)[0], 24


def cluster_sizes(max_k=257):
    return _clusters(max_k)[1]


def fine_lattice():
    """6 x 6 x 6 cells at spacing 0.25 (coordinates exact in binary32): every cell has tied distances, the 8
    corners 51 candidates (the LDS kernel's tie path), the 208 others 65 to 188 (the dense kernel's); at
    coefficient 1.0 full of cells exactly ON a pair's sphere, which the strict `<` keeps."""
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return with_lone_cell((g * 0.25 - 0.625).astype(f32), (2.5, 2.5, 2.5)), 8


def n_candidates(X, gs):
    return (gab.candidates(np.ascontiguousarray(X[:, :3]), gs)[0] >= 0).sum(axis=1)


def widened(X, model, seed=9):
    """X with the extra columns of a wide model's point type, uniform in [0, 1)."""
    extra = np.random.default_rng(seed).random((len(X), gab.WIDTH[model] - 3)).astype(f32)
    return np.hstack([X, extra])


def sphere(n, lib, dist=0.75, seed=5):
    with Solution("relu_gabriel", n, 60, 1.0, lib=lib) as s:
        s.random_sphere(dist, seed)
        X = s.positions()[:n].copy()
    return with_lone_cell(X), 60


def ball_5000():
    """5000 cells uniform in a ball at random_sphere(0.75)'s density (inits.cuh's radius), drawn with numpy.
    (Seeds 75 and 76 draw one pair of cells each within 1e-6 of a Gabriel decision, gab.decision_cells; 77 none at
    coefficients 0.6 and 0.8.  Chosen from the statement alone.)"""
    rng = np.random.default_rng(77)
    n = 5000
    r_max = (n / 0.64) ** (1 / 3) * 0.75 / 2
    v = rng.standard_normal((n, 3))
    v *= (r_max * rng.random(n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return with_lone_cell(v.astype(f32)), 30


def wall_system(lib, n=300, seed=1):
    """examples/growth_w_wall.cu:144-154: node 0 at (0, 0, -0.75), the others in random_sphere(0.5) with z >= 0."""
    with Solution("wall_gabriel", n, 30, 1.0, lib=lib) as s:
        s.random_sphere(0.5, seed)
        X = s.positions()[:n].copy()
    X[0] = (0, 0, -0.75)
    X[1:, 2] = np.abs(X[1:, 2])
    return with_lone_cell(X, (6.0, 6.0, 9.0)), 30


def run(lib, model, X, gs, coefficient=None, steps=1, dt=0.0):
    n = len(X)
    with Solution(model, n, gs, 1.0, lib=lib) as s:
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        if coefficient is not None:
            s.set_param("gabriel_coefficient", coefficient)
        s.set_fixed(n - 1)
        s.take_step(dt, steps)
        return s.positions()[:n].copy(), s.old_v()[:n].copy()


def counts(lib, X, gs, coefficient, repeat=1):
    """count_gabriel's n_nbs after a dt = 0 step (both stages see X), `repeat` times on one system."""
    n = len(X)
    out = []
    with Solution("count_gabriel", n, gs, 1.0, lib=lib) as s:
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        s.set_param("gabriel_coefficient", coefficient)
        s.set_fixed(n - 1)
        for _ in range(repeat):
            s.take_step(0.0, 1)
            out.append(s.get_prop("n_nbs", n))
        assert same_bits(s.positions()[:n], X)                # the functor returns zero
    return out if repeat > 1 else out[0]


def twins():
    """random_260 with 40 of its cells a second time: a coincident cell is a candidate at distance 0, so a cell's
    own entry is not always the first of its sorted list.  For count_gabriel only (its functor does not divide by
    the distance)."""
    X, gs = random_260()
    X = X.copy()
    X[200:240] = X[:40]
    return X, gs


CASES = {"hexagon": hexagon, "lattice": lattice, "fine_lattice": fine_lattice, "random_260": random_260,
         "clusters": clusters}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def test_statement_reproduces_the_reference_kat():
    """tests/test_solvers.cu:354-381: 19-cell hexagon, grid 5, coefficient 0.8: 6 / 3 / 4 neighbours."""
    c = gab.neighbour_counts(gab.regular_hexagon(19), 5, 0.8)
    assert (c[:7] == 6).all()
    assert (c[7::2] == 3).all() and (c[8::2] == 4).all()


def test_statement_selection_sort_is_not_stable():
    """The order the statement replays is the reference's swap sort, not a stable sort by distance."""
    ids = np.array([[10, 11, 12]])
    d = np.array([[f32(0.5), f32(0.5), f32(0.2)]])
    ids_s, d_s = gab.selection_sort(ids, d)
    assert ids_s.tolist() == [[12, 11, 10]]


@pytest.mark.parametrize("model", ["relu_gabriel", "clipped_gabriel"])
@pytest.mark.parametrize("coefficient", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("case", ["hexagon", "lattice", "random_260"])
def test_oracle_rhs_is_the_statement(oracle, model, coefficient, case):
    X, gs = {"hexagon": hexagon, "lattice": lattice, "random_260": random_260}[case]()
    Xo, F = run(oracle, model, X, gs, coefficient)
    assert same_bits(Xo, X)                                   # dt = 0: nothing moved
    want = gab.forces(X, gs, coefficient, model)
    assert np.abs(want).max() > 0 and (want[-1] == 0).all()   # (springs of rest length 0.5: ~0 on the hexagon)
    assert same_bits(F, want)


@pytest.mark.parametrize("coefficient", [0.5, 0.8, 1.0])
def test_oracle_rhs_is_the_statement_at_5000_cells(oracle, coefficient):
    X, gs = sphere(5000, oracle)
    for model in ("relu_gabriel", "clipped_gabriel"):
        _, F = run(oracle, model, X, gs, coefficient)
        assert same_bits(F, gab.forces(X, gs, coefficient, model)), model


def test_the_coefficient_matters(oracle):
    X, gs = random_260()
    _, a = run(oracle, "relu_gabriel", X, gs, 0.5)
    _, b = run(oracle, "relu_gabriel", X, gs)
    _, c = run(oracle, "relu_gabriel", X, gs, 0.8)
    assert same_bits(b, c) and not same_bits(a, b)           # the default is 0.8


@pytest.mark.parametrize("case", ["hexagon", "random_260", "sphere_5000"])
def test_oracle_takes_the_statement_steps(oracle, case):
    """20 whole Heun steps (the grid rebuilt from X and X1, old_v averaged from the second step on)."""
    X, gs = sphere(5000, oracle) if case == "sphere_5000" else {"hexagon": hexagon, "random_260": random_260}[case]()
    p = len(X) - 1
    for model in ("relu_gabriel", "clipped_gabriel"):
        Xo, vo = run(oracle, model, X, gs, None, steps=20, dt=0.05)
        Xs, vs = gab.steps(X, 20, 0.05, p, gs, 0.8, model)
        assert np.abs(Xs - X).max() > (1e-3 if model == "relu_gabriel" else 0), model
        assert same_bits(Xo, Xs), model
        assert same_bits(vo, vs), model


def test_oracle_wall_model_is_the_statement(oracle):
    X, gs = wall_system(oracle)
    _, F = run(oracle, "wall_gabriel", X, gs)
    want = gab.forces(X, gs, 0.8, "wall_gabriel")
    assert want[0, 2] != 0 and np.abs(want[1:, :2]).max() > 0.01
    assert same_bits(F, want)                                 # the wall node too: summed in index order here
    Xo, vo = run(oracle, "wall_gabriel", X, gs, None, steps=20, dt=0.1)
    Xs, vs = gab.steps(X, 20, 0.1, len(X) - 1, gs, 0.8, "wall_gabriel")
    assert same_bits(Xo, Xs) and same_bits(vo, vs)


def test_wall_node_prunes_but_feels_no_pair_force():
    """The wall node stays a Gabriel candidate: it can drop another pair although its functors return 0."""
    X = np.array([[0, 0, 0], [0.8, 0, 0], [0.4, 0.05, 0]], f32)  # node 0, a pair (1, ?) ... and a cell between
    ids, dist, kept = gab.gabriel_lists(X[[1, 0, 2]], 5, 0.8)      # as cells 1, 0, 2: pair (0, 1) via cell 2
    assert not kept[0][ids[0] == 1].any()                          # cell 2 at the midpoint prunes (0, 1)


def test_gabriel_models_refuse_the_grid_only_knobs(oracle):
    X, gs = random_260()
    with Solution("relu_gabriel", len(X), gs, 1.0, lib=oracle) as s:
        for knob in ("sorted_pipeline", "tile_lanes", "slab_global_ids", "sum_order", "force_variant"):
            with pytest.raises(YallaError, match="-2"):
                s.set_param(knob, 1)
    with Solution("relu_grid", len(X), gs, 1.0, lib=oracle) as s:
        with pytest.raises(YallaError, match="-2"):
            s.set_param("gabriel_coefficient", 0.5)


def test_the_cluster_input_is_what_it_says():
    """Every cell's candidate count is its cluster's K (so both sides of GABRIEL_CAP = 64 and every lane-group
    and chunk boundary are present), and the system stays far from the grid's edge."""
    X, gs = clusters()
    size = cluster_sizes()
    assert len(X) == 3427 and gs == 24 and np.abs(X).max() < 10
    assert np.array_equal(n_candidates(X, gs), size)
    assert sorted(set(size[:-1])) == CLUSTER_SIZES and (np.bincount(size[:-1])[CLUSTER_SIZES] == 2 * np.array(CLUSTER_SIZES)).all()
    Xs, _ = clusters(64)
    assert np.array_equal(n_candidates(Xs, gs), cluster_sizes(64)) and cluster_sizes(64).max() == 64
    assert len(Xs) == 2 * sum(K for K in CLUSTER_SIZES if K <= 64) + 1


def test_the_fine_lattice_is_what_it_says():
    X, gs = fine_lattice()
    c = n_candidates(X, gs)[:-1]
    assert (c == 51).sum() == 8 and ((c >= 65) & (c <= 188)).sum() == 208 and c.max() == 188
    ids, dist = gab.candidates(X, gs)
    d = np.sort(np.where(ids >= 0, dist, np.arange(dist.shape[1], dtype=f32)[None] + 10), axis=1)
    assert (d[:-1, 1:] == d[:-1, :-1]).any(axis=1).all()      # every cell has tied distances
    # coefficient 1.0: a candidate exactly on a pair's sphere (the midpoint of two cells 0.5 apart in x, and
    # a cell 0.25 above it: dist_mk == radius == 0.25), kept by the strict `<`
    assert gab.dist3(np.array([0, 0.25, 0], f32)) == f32(0.5) * f32(0.5) * f32(1.0)


@pytest.mark.parametrize("model", ["relu_plain_gabriel", "clipped_gabriel"])
@pytest.mark.parametrize("coefficient", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("case", ["clusters", "fine_lattice"])
def test_oracle_rhs_is_the_statement_at_the_list_edges_and_with_ties(oracle, model, coefficient, case):
    X, gs = CASES[case]()
    Xo, F = run(oracle, model, X, gs, coefficient)
    assert same_bits(Xo, X)
    want = gab.forces(X, gs, coefficient, model)
    assert np.abs(want).max() > 0.1 and (want[-1] == 0).all()
    assert same_bits(F, want)


def test_oracle_undeclared_functor_is_relu_force(oracle):
    """relu_plain is relu_force<float3> statement for statement: the same bits, whole steps."""
    X, gs = random_260()
    a = run(oracle, "relu_gabriel", X, gs, None, steps=5, dt=0.05)
    b = run(oracle, "relu_plain_gabriel", X, gs, None, steps=5, dt=0.05)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and not same_bits(a[0], X)


@pytest.mark.parametrize("coefficient", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("case", list(CASES) + ["twins"])
def test_oracle_counts_the_statement_neighbours(oracle, case, coefficient):
    """tests/test_solvers.cu:339-381 as a model: n_nbs == the statement's kept pairs, exactly."""
    X, gs = twins() if case == "twins" else CASES[case]()
    got = counts(oracle, X, gs, coefficient)
    want = gab.neighbour_counts(X, gs, coefficient)
    assert want.max() > 0 and want[-1] == 0
    assert np.array_equal(got, want)
    if case == "hexagon" and coefficient == 0.8:              # the reference's KAT: 6 / 3 / 4
        assert (got[:7] == 6).all() and (got[7:19:2] == 3).all() and (got[8:19:2] == 4).all()


@pytest.mark.parametrize("model", ["relu_po_gabriel", "relu_cell_gabriel"])
def test_oracle_wide_point_types(oracle, model):
    """Po_cell / Cell under Gabriel_solver: xyz as relu_gabriel on the same xyz, the extra columns untouched."""
    X3, gs = random_260()
    X = widened(X3, model)
    _, F = run(oracle, model, X, gs)
    assert same_bits(F, gab.forces(X, gs, 0.8, model)[:, :3])
    Xw, vw = run(oracle, model, X, gs, None, steps=3, dt=0.05)
    Xr, vr = run(oracle, "relu_gabriel", X3, gs, None, steps=3, dt=0.05)
    assert not same_bits(Xr, X3)
    assert same_bits(Xw[:, :3], Xr) and same_bits(vw, vr)
    assert same_bits(Xw[:, 3:], X[:, 3:])
    Xs, vs = gab.steps(X, 3, 0.05, len(X) - 1, gs, 0.8, model)
    assert same_bits(Xw, Xs) and same_bits(vw, vs)


@pytest.mark.parametrize("case", ["random_260", "ball_5000"])
@pytest.mark.parametrize("coefficient", [0.6, 0.8])
def test_the_fast_tier_inputs_have_few_cells_on_a_decision_boundary(case, coefficient):
    """The condition of test_gabriel_bodies_gpu.py's fast-tier comparison, from the statement alone: at most 1 %
    of the cells are within 1e-6 (relative) of a cut-off or Gabriel decision -- in fact none."""
    X, gs = {"random_260": random_260, "ball_5000": ball_5000}[case]()
    marked = gab.decision_cells(X, gs, coefficient)
    print(case, coefficient, "marked cells:", int(marked.sum()), "of", len(X))
    assert marked.mean() <= 0.01
    assert marked.sum() == 0
    X1, gs1 = fine_lattice()                                  # (the margin does mark what sits ON a sphere)
    assert gab.decision_cells(X1, gs1, 1.0)[:-1].all()
