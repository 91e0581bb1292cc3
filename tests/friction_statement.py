"""A numpy statement of ONE stage's right-hand side, F + sum_v / sum_friction, with the friction given as a Python
callable -- written from the reference's loops alone (include/solvers.cuh: compute_tile :284-322, all pairs with j
ascending; compute_cube :430-463 over the 27 cubes of the stencil table :472-483, ascending id inside a cube; add_rhs
:146-161), the same loops as reference_forces / reference_tile_rhs of tests/test_reference_statement_numpy.py, which
hard-code friction_w_neighbour.  Every pair the solver lets interact adds its three terms in the loop's order,

    F += pw_int(Xi, r, dist, i, j);  sum_friction += friction;  sum_v += friction * old_v[j]   (unconditionally),

one rounding per product and per add, and the stage ends with `if (sum_friction > 0) dX += sum_v / sum_friction`.

`real` is the number format of the evaluation: numpy.float32 states the bits (dist = sqrtf(fmaf(z, z, fmaf(y, y,
x * x))), fmaf through binary64; float3 `/ dist` is `* float(1. / dist)`, scalar `/` a true division), numpy.float64
is the same statement in binary64 -- the yardstick of the fast-arithmetic tier.  The binary32 constants of the
functors (0.8f) stay binary32 values in both.  Cube ids are always binary32's (the positions are).

The frictions restate yalla_amd/csrc/model_functors.h's graded / ids / field bodies; the forces are relu_force
(inits.cuh:78-93) and models::fading_spring.  All are vectorised over a cell's partners: arguments Xi (width,),
r (m, width), dist (m,), i (m,), j (m,); the Gabriel statement (tests/gabriel_statement.py) calls them with (n, width)
rows."""
import numpy as np

f32 = np.float32
f64 = np.float64


def dist3(r, real=f32):
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    if real is f64:
        return np.sqrt(x * x + y * y + z * z)
    inner = ((y.astype(f64) * y.astype(f64)) + (x * x).astype(f32).astype(f64)).astype(f32)
    return np.sqrt(((z.astype(f64) * z.astype(f64)) + inner.astype(f64)).astype(f32))


# ---- the friction functors ---------------------------------------------------------------------------------------
def graded(Xi, r, dist, i, j, real=f32):
    """if (i == j) return 0.25f; return dist < 1.f ? 1.f - dist : 0.f;"""
    return np.where(i == j, real(0.25), np.where(dist < real(1), real(1) - dist, real(0))).astype(real)


def ids(Xi, r, dist, i, j, real=f32):
    """if (!(dist < 1.f)) return 0.f; return 0.125f * float(((5 * i + 2 * j) & 7) - 2);"""
    k = ((5 * np.asarray(i, np.int64) + 2 * np.asarray(j, np.int64)) & 7) - 2
    return np.where(dist < real(1), real(0.125) * k.astype(real), real(0)).astype(real)


def field(Xi, r, dist, i, j, real=f32):
    """if (i == j || !(dist < 1.f)) return 0.f;
    return 0.25f + 0.5f * fminf(1.f, fabsf(r.theta)) + 0.25f * fminf(1.f, fabsf(Xi.phi));"""
    theta = np.minimum(real(1), np.abs(r[..., 3])).astype(real)
    phi = np.minimum(real(1), np.abs(Xi[..., 4])).astype(real)
    value = ((real(0.25) + (real(0.5) * theta).astype(real)).astype(real) + (real(0.25) * phi).astype(real)).astype(real)
    return np.where((i != j) & (dist < real(1)), value, real(0)).astype(real)


def friction_w_neighbour(Xi, r, dist, i, j, real=f32):
    return np.where((i != j) & (dist < real(1)), real(1), real(0)).astype(real)


def friction_on_background(Xi, r, dist, i, j, real=f32):
    """return 0;  (solvers.cuh:37-41: sum_friction stays 0 and the stage's right-hand side is F alone)"""
    return np.zeros(np.shape(dist), real)


# ---- the forces (on x, y, z; `Pt dF{0}` leaves the further fields of a wide point without force) ------------------
def relu_force(Xi, r, dist, i, j, real=f32):
    c = real(f32(0.8))
    F = (np.maximum(c - dist, real(0)) * real(2) - np.maximum(dist - c, real(0))).astype(real)
    with np.errstate(invalid="ignore", divide="ignore"):       # (the self pair's 0 / 0 is masked out)
        out = (r[..., :3] * F[..., None]).astype(real) / dist[..., None]
    return np.where(((i != j) & ~(dist > real(1)))[..., None], out, real(0)).astype(real)


def fading_spring(Xi, r, dist, i, j, real=f32):
    """dF = r * ((L_0 - dist) * (1 - dist)) / dist, zero for i == j and for dist >= 1"""
    s = ((real(0.5) - dist).astype(real) * (real(1) - dist).astype(real)).astype(real)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = (f64(1) / dist.astype(f64)).astype(real)
        out = ((r[..., :3] * s[..., None]).astype(real) * inv[..., None]).astype(real)
    return np.where(((i != j) & ~(dist >= real(1)))[..., None], out, real(0)).astype(real)


FRICTIONS = {"graded": graded, "ids": ids, "field": field}


# ---- the loops -----------------------------------------------------------------------------------------------------
def nhood(gs):
    h = [-1, 0, 1]                                                # solvers.cuh:472-483
    h = h + [h[i % 3] - gs for i in range(3)] + [h[i % 3] + gs for i in range(3)]
    return h + [h[i % 9] - gs * gs for i in range(9)] + [h[i % 9] + gs * gs for i in range(9)]


def cube_members(X, gs, cube_size):
    cube3 = np.floor(X[:, :3].astype(f32) / f32(cube_size)).astype(np.int64) + gs // 2   # solvers.cuh:357-360
    cube = cube3[:, 0] + cube3[:, 1] * gs + cube3[:, 2] * gs * gs
    members = {}
    for i in np.argsort(cube, kind="stable"):                    # stable sort: ascending id inside a cube
        members.setdefault(int(cube[i]), []).append(int(i))
    return cube, members


def _terms(X, old_v, i, ks, force, friction, real, cut):
    """The terms of cell i's pairs with `ks`, in that order, and which of them the solver lets interact."""
    ks = np.asarray(ks, np.int64)
    r = (X[i] - X[ks]).astype(real)
    dist = dist3(r, real)
    ii = np.full(len(ks), i, np.int64)
    on = np.ones(len(ks), bool) if cut is None else ~(dist >= real(f32(cut)))   # compute_cube :450
    fr = friction(X[i], r, dist, ii, ks, real)
    return on, force(X[i], r, dist, ii, ks, real), fr, (fr[:, None] * old_v[ks]).astype(real)


def _run(on, F_terms, fr, products, real):
    F, sv, sf = np.zeros(3, real), np.zeros(3, real), real(0)
    for m in np.nonzero(on)[0]:
        F = F + F_terms[m]
        sf = sf + fr[m]
        sv = sv + products[m]
    return F, sv, sf


def _add_rhs(F, sv, sf):
    return F + sv / sf if sf > 0 else F                          # add_rhs, :155-159


def stage_rhs(X, old_v, force, friction, solver="tile", gs=30, cube_size=1.0, by_plane=False, real=f32):
    """(dX, sum_friction, n_terms): dX (n, width) the stage's right-hand side of every cell, sum_friction its divisor
    and n_terms how many of a cell's pairs had a non-zero friction.  solver "tile": all pairs, j ascending, no cut;
    "grid": the 27 cubes in the reference's order with the cut at cube_size, as one running sum or (by_plane) as the
    own z-plane's 9 cubes | the other 18, each from zero, added at the end."""
    n, width = X.shape
    X = X.astype(real)
    old_v = np.asarray(old_v).astype(real)
    dX = np.zeros((n, width), real)
    sum_friction = np.zeros(n, real)
    n_terms = np.zeros(n, np.int64)
    if solver == "grid":
        cube, members = cube_members(X, gs, cube_size)
        offsets = nhood(gs)
    for i in range(n):
        if solver == "tile":
            parts = [np.arange(n)]
        else:
            lists = [members.get(int(cube[i]) + off, []) for off in offsets]
            parts = [sum(lists[:9], []), sum(lists[9:], [])] if by_plane else [sum(lists, [])]
        sums = []
        for ks in parts:
            on, F_terms, fr, products = _terms(X, old_v, i, ks, force, friction, real, None if solver == "tile" else cube_size)
            sums.append(_run(on, F_terms, fr, products, real))
            n_terms[i] += int((on & (fr != 0)).sum())
        F, sv, sf = sums[0]
        if len(sums) == 2:
            F, sv, sf = F + sums[1][0], sv + sums[1][1], sf + sums[1][2]
        dX[i, :3] = _add_rhs(F, sv, sf)
        sum_friction[i] = sf
    return dX, sum_friction, n_terms


def as_old_v_after_a_dt_0_step(dX, p):
    """What take_step(0) with set_fixed(p) leaves in old_v: both stages see the same state, each subtracts the fixed
    point's right-hand side, and heun_step stores ((dX - fix) + (dX - fix)) * 0.5 (solvers.cuh:113-144)."""
    d = (dX[:, :3] - dX[p, :3]).astype(dX.dtype)
    return ((d + d) * dX.dtype.type(0.5)).astype(dX.dtype)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def cloud(n, width, seed, spacing=0.75, lone=True):
    """n cells uniform in a ball at the density of random_sphere(spacing); further fields uniform in [-2, 2) (so that
    differences of them lie on both sides of 1); lone: the LAST cell far from all others, to be held fixed."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, width), f32)
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    radius = spacing * (n / 0.64) ** (1 / 3) / 2 * rng.random(n) ** (1 / 3)
    rows[:, :3] = (direction * radius[:, None]).astype(f32)
    rows[:, 3:] = (rng.random((n, width - 3)) * 4 - 2).astype(f32)
    if lone and n:
        rows[-1, :3] = np.abs(rows[:, :3]).max() + 3.0
    return rows


def velocities(n, seed, lone=True):
    """old_v drawn at random, no component zero; the lone cell's is zero (its right-hand side is then its own
    self term's: v * f / f of zero, or nothing)."""
    rng = np.random.default_rng(seed)
    v = (rng.random((n, 3)) * 2 - 1).astype(f32)
    v[v == 0] = f32(0.5)
    if lone and n:
        v[-1] = 0
    return v
