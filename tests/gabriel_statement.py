"""An independent numpy binary32 statement of the reference's Gabriel force, `compute_cube_gabriel`
(include/solvers.cuh:509-602), written from the reference alone, vectorised over cells (candidates padded per
cell to a fixed width), with the arithmetic contract of test_reference_statement_numpy.py:

  * candidates: every cell of the 27 cubes (d_nhood order, :472-483; ascending id inside a cube) with
    dist < cube_size, the cell itself included, dist = sqrtf(fmaf(z, z, fmaf(y, y, x * x))), fmaf through binary64;
  * order: the reference's selection sort (:550-566) -- strict `<`, swaps, NOT stable -- replayed step by step;
  * test: candidate m is dropped if a candidate q < m lies strictly inside the sphere around 0.5f * (Xi + Xj)
    with radius 0.5f * dist * coefficient (:572-593), never for j == i;
  * sum: the kept pairs, farthest first, F += pw_int, sum_friction += friction, sum_v += friction * old_v[j];
    float3 `/ dist` is `* float(1. / dist)` (dtypes.cuh), scalar `/` a true division.

Also examples/growth_w_wall.cu's relu_force and the wall of node 0 (links.cuh:142-210) for `wall_gabriel`."""
import numpy as np

f32 = np.float32
f64 = np.float64


def fma32(a, b, c):
    return (f64(1) * a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def dist3(r):
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    return np.sqrt(fma32(z, z, fma32(y, y, (x * x).astype(f32))))


def nhood(gs):
    h = [-1, 0, 1]
    h = h + [h[i % 3] - gs for i in range(3)] + [h[i % 3] + gs for i in range(3)]
    return h + [h[i % 9] - gs * gs for i in range(9)] + [h[i % 9] + gs * gs for i in range(9)]


def candidates(X, gs):
    """(ids, dist) per cell, (n, K): the candidates in the reference's order, padded with id -1 / dist inf."""
    n = len(X)
    cube3 = np.floor(X).astype(np.int64) + gs // 2               # cube_size 1 (solvers.cuh:357-360)
    cube = cube3[:, 0] + cube3[:, 1] * gs + cube3[:, 2] * gs * gs
    perm = np.argsort(cube, kind="stable")                       # ascending id inside a cube
    sc = cube[perm]
    cols = []
    for off in nhood(gs):
        lo = np.searchsorted(sc, cube + off, "left")
        hi = np.searchsorted(sc, cube + off, "right")
        width = int((hi - lo).max()) if n else 0
        t = np.arange(width)[None, :]
        at = lo[:, None] + t
        cols.append(np.where(t < (hi - lo)[:, None], perm[np.minimum(at, n - 1)], -1))
    idx = np.concatenate(cols, axis=1)
    r = X[:, None, :] - X[np.maximum(idx, 0)]
    d = dist3(r)
    hit = (idx >= 0) & ~(d >= f32(1.0))                          # :540
    K = max(int(hit.sum(axis=1).max()), 1)
    order = np.argsort(~hit, axis=1, kind="stable")[:, :K]       # the hits, in scan order
    ids = np.take_along_axis(np.where(hit, idx, -1), order, axis=1)
    dist = np.take_along_axis(np.where(hit, d, f32(np.inf)), order, axis=1)
    return ids, dist


def selection_sort(ids, dist):
    """:550-566 for every row at once: at step m the first minimum of m.. (strict `<` from d[m]) swaps with m."""
    ids, dist = ids.copy(), dist.copy()
    rows = np.arange(len(ids))
    K = ids.shape[1]
    for m in range(K - 1):
        sub = dist[:, m:]
        p = m + np.argmax(sub == sub.min(axis=1)[:, None], axis=1)
        for a in (ids, dist):
            t = a[rows, p].copy()
            a[rows, p] = a[rows, m]
            a[rows, m] = t
    return ids, dist


def relu_force(Xi, r, dist, i, j):                               # inits.cuh:78-93
    F = (np.maximum(f32(0.8) - dist, f32(0)) * f32(2) - np.maximum(dist - f32(0.8), f32(0))).astype(f32)
    out = (r * F[..., None]).astype(f32) / dist[..., None]
    return np.where(((i != j) & ~(dist > f32(1)))[..., None], out, f32(0)).astype(f32)


def clipped_spring(Xi, r, dist, i, j):                           # tests/test_solvers.cu:44-53
    inv = (f64(1) / dist.astype(f64)).astype(f32)
    out = ((r * (f32(0.5) - dist)[..., None]).astype(f32) * inv[..., None]).astype(f32)
    return np.where(((i != j) & ~(dist >= f32(1)))[..., None], out, f32(0)).astype(f32)


def wall_relu_force(Xi, r, dist, i, j):                          # examples/growth_w_wall.cu:45-63
    F = (np.maximum((f64(0.7) - dist.astype(f64)).astype(f32), f32(0))
         - np.maximum((dist.astype(f64) - f64(0.8)).astype(f32), f32(0))).astype(f32)
    out = f32(0) + (r * F[..., None]).astype(f32) / dist[..., None]
    keep = (i != 0) & (j != 0) & (i != j) & ~(dist > f32(1))
    return np.where(keep[..., None], out, f32(0)).astype(f32)


def friction_w_neighbour(dist, i, j, Xi=None, r=None):           # solvers.cuh:26-33
    return np.where((i != j) & (dist < f32(1)), f32(1), f32(0)).astype(f32)


def friction_on_background(dist, i, j, Xi=None, r=None):
    return np.zeros(dist.shape, f32)


def _user_friction(name):
    """A user-written friction of tests/friction_statement.py (Xi and r with every field of the point)."""
    def pw_friction(dist, i, j, Xi, r):
        import friction_statement
        return friction_statement.FRICTIONS[name](Xi, r, dist, i, j)
    return pw_friction


# relu_plain_gabriel: the same functor, not declared stateless on the device (another kernel body, the same
# numbers).  The two wide models (Po_cell: x y z theta phi; Cell: + u v): rows are xyz plus extra columns, the
# geometry is xyz alone and the force on the extra columns is zero (relu_force's `Pt dF{0}`).
MODELS = {"relu_gabriel": (relu_force, friction_w_neighbour),
          "relu_plain_gabriel": (relu_force, friction_w_neighbour),
          "relu_po_gabriel": (relu_force, friction_w_neighbour),
          "relu_cell_gabriel": (relu_force, friction_w_neighbour),
          "clipped_gabriel": (clipped_spring, friction_w_neighbour),
          "wall_gabriel": (wall_relu_force, friction_on_background),
          # user-written frictions (yalla_amd/csrc/model_functors.h), declared and not: the same numbers
          "friction_graded_gabriel": (relu_force, _user_friction("graded")),
          "friction_ids_gabriel": (relu_force, _user_friction("ids")),
          "friction_ids_plain_gabriel": (relu_force, _user_friction("ids")),
          "friction_field_gabriel": (relu_force, _user_friction("field"))}
WIDTH = {"relu_po_gabriel": 5, "relu_cell_gabriel": 7, "friction_field_gabriel": 5}

_memo = {}


def _memoised(key, make):
    """The lists of an input are made once (tests share them; the arrays are read-only)."""
    if key not in _memo:
        if len(_memo) >= 24:
            _memo.pop(next(iter(_memo)))
        out = make()
        for a in out:
            a.setflags(write=False)
        _memo[key] = out
    return _memo[key]


def _key(X, *rest):
    X = np.ascontiguousarray(X, f32)
    return (X.shape, hash(X.tobytes())) + rest


def gabriel_lists(X, gs, coefficient):
    """(ids, dist, kept) per cell, in the selection sort's order: kept[i, m] = pair (i, ids[i, m]) interacts."""
    X = np.ascontiguousarray(X[:, :3], f32)
    return _memoised(_key(X, gs, float(f32(coefficient))), lambda: _gabriel_lists(X, gs, coefficient))


def _gabriel_lists(X, gs, coefficient):
    n = len(X)
    ids, dist = _memoised(_key(X, gs), lambda: selection_sort(*candidates(X, gs)))
    kept = ids >= 0                                               # (a new array)
    coef = f32(coefficient)
    # cells in the order of their candidate counts, so that a chunk is padded to ITS widest list only (the
    # sorted lists hold their candidates first); the test of candidates m0 .. m1 needs q < m1 only
    count = kept.sum(axis=1)
    by_count = np.argsort(count, kind="stable")
    a = 0
    while a < n:
        b = min(n, a + max(1, 3_000_000 // max(int(count[by_count[a]]), 1) ** 2))
        while b > a + 1 and (b - a) * int(count[by_count[b - 1]]) ** 2 > 6_000_000:
            b = a + (b - a) // 2
        rows = by_count[a:b]
        K = max(int(count[rows[-1]]), 1)
        I, D = ids[rows, :K], dist[rows, :K]
        Xi = X[rows, None, :]
        Xj = X[np.maximum(I, 0)]                                  # (c, K, 3)
        mid = (f32(0.5) * (Xi + Xj)).astype(f32)
        radius = ((f32(0.5) * D).astype(f32) * coef).astype(f32)
        dropped = np.zeros(I.shape, bool)
        for m0 in range(0, K, 64):
            m1 = min(K, m0 + 64)
            r_mk = (mid[:, m0:m1, None, :] - Xj[:, None, :m1, :]).astype(f32)   # [c, m, q]
            inside = dist3(r_mk) < radius[:, m0:m1, None]
            earlier = (np.arange(m1)[None, :] < np.arange(m0, m1)[:, None])[None] & (I[:, :m1] >= 0)[:, None, :]
            dropped[:, m0:m1] = (inside & earlier).any(axis=2)
        kept[rows, :K] &= ~(dropped & (I != rows[:, None]))
        a = b
    return ids, dist, kept


def rhs(X, gs, coefficient, model, old_v=None, gen=None):
    """A stage's right-hand side: gen + F, then + sum_v / sum_friction where sum_friction > 0 (add_rhs)."""
    with np.errstate(invalid="ignore", divide="ignore"):     # (the self pair's 0 / 0 is masked out)
        return _rhs(X, gs, coefficient, model, old_v, gen)


def _rhs(X, gs, coefficient, model, old_v, gen):
    pw_int, pw_friction = MODELS[model]
    n = len(X)
    width = X.shape[1]
    assert width == WIDTH.get(model, 3)
    rows = np.ascontiguousarray(X, f32)                           # (every field: what a friction may read)
    X = np.ascontiguousarray(X[:, :3], f32)
    if gen is not None:
        assert width == 3
    ids, dist, kept = gabriel_lists(X, gs, coefficient)
    i = np.arange(n)
    F = np.zeros((n, 3), f32)
    sf = np.zeros(n, f32)
    sv = np.zeros((n, 3), f32)
    for m in range(ids.shape[1] - 1, -1, -1):                   # farthest first
        j = ids[:, m]
        on = kept[:, m]
        jj = np.maximum(j, 0)
        dm = np.where(on, dist[:, m], f32(1))
        r = (X - X[jj]).astype(f32)
        F = np.where(on[:, None], F + pw_int(X, r, dm, i, j), F)
        fr = pw_friction(dm, i, j, rows, (rows - rows[jj]).astype(f32))
        sf = np.where(on, sf + fr, sf)
        if old_v is not None:
            sv = np.where(on[:, None], sv + fr[:, None] * old_v[jj], sv)
    dX = F if gen is None else (gen + F).astype(f32)
    dX = np.where((sf > 0)[:, None], dX + sv / sf[:, None], dX).astype(f32)
    return np.hstack([dX, np.zeros((n, width - 3), f32)])         # no force on the extra columns


def wall_gen(X):
    """wall_forces<float3, xy_wall_relu_force>(n, X, dX, 0) on a zeroed dX: node 0's sum in index order."""
    n = len(X)
    dX = np.zeros((n, 3), f32)
    dw = np.abs(X[:, 2] - X[0, 2]).astype(f32)
    F = (np.maximum((f64(0.8) - dw.astype(f64)).astype(f32), f32(0))
         - np.maximum((dw.astype(f64) - f64(0.8)).astype(f32), f32(0))).astype(f32)
    near = dw < f32(1)
    near[0] = False
    dX[:, 2] = np.where(near, f32(0) + F, f32(0))
    acc, cnt = f32(0), 0
    for k in np.nonzero(near)[0]:
        acc = f32(acc + (-F[k]))
        cnt += 1
    if cnt:
        inv = f32(1) / f32(cnt)
        dX[0] = (dX[0] + np.array([0, 0, acc], f32)) * inv
    return dX


def forces(X, gs, coefficient, model):
    """What one dt = 0 step with a fixed lone cell leaves in old_v: the stage's right-hand side with old_v = 0."""
    return rhs(X, gs, coefficient, model, old_v=np.zeros_like(X[:, :3]),
               gen=wall_gen(X) if model == "wall_gabriel" else None)


def steps(X, steps_, dt, p, gs, coefficient, model):
    """Heun_solver::take_step with set_fixed(p), `steps_` times (as reference_grid_steps of the grid statement)."""
    X = X.copy()
    old_v = np.zeros_like(X[:, :3])
    dt = f32(dt)
    for _ in range(steps_):
        gen = wall_gen(X) if model == "wall_gabriel" else None
        dX = rhs(X, gs, coefficient, model, old_v, gen)
        dX = dX - dX[p]
        X1 = (X + dX * dt).astype(f32)
        gen1 = wall_gen(X1) if model == "wall_gabriel" else None
        dX1 = rhs(X1, gs, coefficient, model, old_v, gen1)
        dX1 = dX1 - dX1[p]
        X = (X + ((dX + dX1) * f32(0.5)) * dt).astype(f32)
        old_v = ((dX + dX1) * f32(0.5)).astype(f32)[:, :3]
    return X, old_v


def neighbour_counts(X, gs, coefficient):
    """tests/test_solvers.cu:354-381's count_neighbours: kept pairs with i != j and dist <= 1."""
    ids, dist, kept = gabriel_lists(X, gs, coefficient)
    i = np.arange(len(X))[:, None]
    return (kept & (ids != i) & ~(dist > f32(1))).sum(axis=1)


def decision_cells(X, gs, coefficient, margin=1e-6):
    """The cells with a decision that arithmetic within `margin` of binary32's could turn, from the positions in
    binary64: a pair distance within `margin` of cube_size (1), or a (pair, earlier candidate) with
    |dist_mk - radius| < margin * radius.  (What another rounding of sqrt or of its radicand may flip; the lists'
    order is the binary32 statement's.)"""
    X64 = np.ascontiguousarray(X[:, :3]).astype(f64)
    n = len(X64)
    mark = np.zeros(n, bool)
    for a in range(0, n, 400):
        d = np.sqrt(((X64[a:a + 400, None, :] - X64[None, :, :]) ** 2).sum(axis=2))
        mark[a:a + 400] |= (np.abs(d - 1.0) < margin).any(axis=1)
    ids, _, _ = gabriel_lists(X, gs, coefficient)
    K = ids.shape[1]
    coef = f64(f32(coefficient))
    lower = np.tril(np.ones((K, K), bool), -1)[None]
    chunk = max(1, 2_000_000 // (K * K))
    for a in range(0, n, chunk):
        I = ids[a:a + chunk]
        Xi = X64[a:a + len(I), None, :]
        Xj = X64[np.maximum(I, 0)]
        radius = 0.5 * np.sqrt(((Xi - Xj) ** 2).sum(axis=2)) * coef
        mid = 0.5 * (Xi + Xj)
        d_mk = np.sqrt(((mid[:, :, None, :] - Xj[:, None, :, :]) ** 2).sum(axis=3))      # [c, m, q]
        near = np.abs(d_mk - radius[:, :, None]) < margin * radius[:, :, None]
        pair = (I >= 0) & (I != np.arange(a, a + len(I))[:, None])
        mark[a:a + len(I)] |= (near & lower & pair[:, :, None] & (I >= 0)[:, None, :]).any(axis=(1, 2))
    return mark


def regular_hexagon(n, d=0.5):
    """inits.cuh:157-210 in binary32 (sinf / cosf of float(beta * j); the intermediate points through the
    binary64 modulus as written).  Only the KAT's neighbour counts depend on it, not bit patterns."""
    X = np.zeros((n, 3), f32)
    beta = np.pi / 3
    c, i = 1, 1
    d = f32(d)
    while c < n:
        for j in range(6):
            ang = f32(beta * j)
            p = np.array([-d * f32(i) * f32(np.sin(ang)), d * f32(i) * f32(np.cos(ang)), 0], f32)
            X[c] = p
            c += 1
            if c == n:
                return X
            n_int = i - 1
            if n_int < 1:
                continue
            ang2 = f32(beta * (j + 1))
            q = np.array([-d * f32(i) * f32(np.sin(ang2)), d * f32(i) * f32(np.cos(ang2)), 0], f32)
            v = q - p
            mod = np.sqrt(f64(v[0]) ** 2 + f64(v[1]) ** 2)
            v = (v * f32(1.0 / mod)).astype(f32)
            for k in range(1, n_int + 1):
                u = ((v * f32(mod)) * (f32(k) / f32(n_int + 1))).astype(f32)
                X[c] = p + u
                c += 1
                if c == n:
                    return X
        i += 1
    return X
