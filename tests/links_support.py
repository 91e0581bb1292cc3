"""What the link suites share (tests/test_ensemble_links_gpu.py, tests/test_links_order.py, tests/test_links_order_gpu.py):
the numpy binary32 statement of a step with link forces, the statement of how ya::link_forces_segmented lays its
entries out and cuts them (include/links.cuh's comment, restated here), the link layouts of the lone-Solution tests and
the lattice inputs on which every sum and update of a step is exact.  A plain module, imported as tests/ensemble_support.py
is."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_reference_statement_numpy import f32, fma32  # noqa: E402

CUT = 256  # ya::LINK_SEGMENT_CUT


# ---- the numpy statement -------------------------------------------------------------------------------------------
def reference_linked_steps(X, links, strength, steps, dt, p):
    """tests/test_reference_statement_numpy.reference_tile_steps with the link terms added before the pairwise sum:
    per stage L = 0; for every link in slot order (a == b skipped) r = Y[a] - Y[b], dist = sqrtf(fmaf(z, z, fmaf(y,
    y, x x))), f = strength r / dist, L[a] += -f, L[b] += f (links.cuh linear_force); the right-hand side is
    L + F (store_rhs on what the generic forces left), then the friction term."""
    n = len(X)
    X = X.copy()
    old_v = np.zeros((n, 3), f32)
    dt, strength = f32(dt), f32(strength)

    def rhs(Y):
        L = np.zeros((n, 3), f32)
        for a, b in links:
            if a == b:
                continue
            r = Y[a] - Y[b]
            dist = np.sqrt(fma32(r[2], r[2], fma32(r[1], r[1], f32(r[0] * r[0]))))
            f = (strength * r) / dist
            L[a] = L[a] + (-f)
            L[b] = L[b] + f
        dX = np.zeros((n, 3), f32)
        for i in range(n):
            F, sv, sf = np.zeros(3, f32), np.zeros(3, f32), f32(0)
            for k in range(n):
                r = Y[i] - Y[k]
                dist = np.sqrt(fma32(r[2], r[2], fma32(r[1], r[1], f32(r[0] * r[0]))))
                if k != i:
                    F = F + (r * (f32(0.5) - dist)) * f32(np.float64(1.0) / np.float64(dist))
                    if dist < f32(1.0):
                        sf = sf + f32(1)
                        sv = sv + old_v[k]
            dX[i] = L[i] + F
            if sf > 0:
                dX[i] = dX[i] + sv / sf
        return dX

    for _ in range(steps):
        dX = rhs(X)
        dX = dX - dX[p]
        X1 = X + dX * dt
        dX1 = rhs(X1)
        dX1 = dX1 - dX1[p]
        X = X + ((dX + dX1) * f32(0.5)) * dt
        old_v = (dX + dX1) * f32(0.5)
    return X, old_v


def dist32(r):
    """sqrtf(fmaf(z, z, fmaf(y, y, x x))) of every row of r, as fma32 does it."""
    x, y, z = (r[:, k].astype(np.float64) for k in range(3))
    xx = (r[:, 0] * r[:, 0]).astype(f32).astype(np.float64)
    return np.sqrt((z * z + (y * y + xx).astype(f32).astype(np.float64)).astype(f32))


def link_terms(Y, links, strength):
    """f of every link slot, strength r / dist in binary32 (zeros for inert slots)."""
    links = np.asarray(links).reshape(-1, 2)
    f = np.zeros((len(links), 3), f32)
    live = links[:, 0] != links[:, 1]
    r = Y[links[live, 0], :3] - Y[links[live, 1], :3]
    f[live] = (f32(strength) * r) / dist32(r)[:, None]
    return f


def serial_link_sums(Y, links, strength):
    """reference_linked_steps' L: every link in slot order, L[a] += -f, L[b] += f."""
    f = link_terms(Y, links, strength)
    L = np.zeros((len(Y), 3), f32)
    for (a, b), term in zip(np.asarray(links).reshape(-1, 2), f):
        if a != b:
            L[a] = L[a] + (-term)
            L[b] = L[b] + term
    return L


def reference_links_only_steps(X, links, strength, steps, dt, p, link_sums=serial_link_sums):
    """reference_linked_steps for a model without pairwise force (models::no_pw_int of links_tile): F = 0 and the
    rest statement for statement, a cell's row of distances at a time (the sum of the neighbours' old_v runs in
    ascending k, which numpy's cumsum does).  link_sums: the stage's L, by default in slot order."""
    n = len(X)
    X = X[:, :3].copy()
    old_v = np.zeros((n, 3), f32)
    dt = f32(dt)

    def rhs(Y):
        L = link_sums(Y, links, strength)
        dX = np.zeros((n, 3), f32)
        for i in range(n):
            near = dist32(Y[i] - Y) < f32(1.0)
            near[i] = False
            dX[i] = L[i] + np.zeros(3, f32)
            if near.any():
                sv = np.cumsum(np.concatenate([np.zeros((1, 3), f32), old_v[near]]), axis=0, dtype=f32)[-1]
                dX[i] = dX[i] + sv / f32(near.sum())
        return dX

    for _ in range(steps):
        dX = rhs(X)
        dX = dX - dX[p]
        X1 = X + dX * dt
        dX1 = rhs(X1)
        dX1 = dX1 - dX1[p]
        X = X + ((dX + dX1) * f32(0.5)) * dt
        old_v = (dX + dX1) * f32(0.5)
    return X, old_v


# ---- the segmented path's layout, from links.cuh's comment ---------------------------------------------------------
DEAD = 0xFFFFFFFF


def piece_layout(links, n_live=None):
    """Entries 2 i (cell a of slot i) and 2 i + 1 (cell b), inert slots and slots from n_live on dead, sorted stably by
    cell with the dead ones last; a piece ends where the cell changes and at every multiple of CUT of the sorted
    array.  Returns (cell, entry, first): the sorted live entries' cells, their entry numbers, and the index at which
    each piece starts (with the end of the live entries as the last element)."""
    links = np.asarray(links, np.int64).reshape(-1, 2)
    n_live = len(links) if n_live is None else n_live
    key = links.astype(np.uint32).reshape(-1).copy()
    dead = np.repeat((links[:, 0] == links[:, 1]) | (np.arange(len(links)) >= n_live), 2)
    key[dead] = DEAD
    entry = np.argsort(key, kind="stable")
    cell = key[entry]
    n = int((cell != DEAD).sum())
    cell, entry = cell[:n], entry[:n]
    at = np.arange(n)
    head = np.ones(n, bool)
    head[1:] = (cell[1:] != cell[:-1]) | (at[1:] % CUT == 0)
    return cell, entry, np.append(at[head], n)


def pieces_per_cell(links, n_cells, n_live=None):
    cell, _, first = piece_layout(links, n_live)
    return np.bincount(cell[first[:-1]].astype(np.int64), minlength=n_cells)


def no_segment_is_cut(links, n_live=None):
    """No run of equal cells in the sorted array contains a multiple of CUT other than at its start."""
    cell, _, _ = piece_layout(links, n_live)
    at = np.arange(1, len(cell))
    return not np.any((at % CUT == 0) & (cell[1:] == cell[:-1]))


def segmented_link_sums(Y, links, strength):
    """What ya::link_forces_segmented adds to a zeroed right-hand side: every piece summed from 0 in sorted order
    (entry 2 i: -f of slot i, entry 2 i + 1: +f), then the pieces of a cell added to its 0 -- for at most two pieces
    in either order the same bits.  Cells of three or more pieces: NaN (their order is not fixed)."""
    f = link_terms(Y, links, strength)
    cell, entry, first = piece_layout(links)
    L = np.zeros((len(Y), 3), f32)
    count = np.zeros(len(Y), int)
    for lo, hi in zip(first[:-1], first[1:]):
        s = np.zeros(3, f32)
        for e in entry[lo:hi]:
            s = s + (f[e >> 1] if e & 1 else -f[e >> 1])
        c = int(cell[lo])
        L[c] = L[c] + s
        count[c] += 1
    L[count > 2] = np.nan
    return L


# ---- layouts ---------------------------------------------------------------------------------------------------------
def rings(n, k1, k2):
    """(i, i + k1) and (i, i + k2) around all n cells: four entries per cell."""
    i = np.arange(n)
    return np.concatenate([np.stack([i, (i + k1) % n], 1), np.stack([(i + k2) % n, i], 1)])


def rings_with_hub(n, hub=64, partners=63):
    """rings, an inert link every 9 slots, and a hub of exactly 256 entries: its 4 ring entries and 4 links to each of
    `partners` = 63 cells above it.  Every cell below the hub has 4 entries, so the hub's segment starts at 4 hub =
    256; every segment's length is a multiple of 4, so no later multiple of 256 falls inside one."""
    hubs = [(hub, hub + 1 + k) if j % 2 else (hub + 1 + k, hub) for k in range(partners) for j in range(4)]
    live = np.concatenate([rings(n, 1, 5), hubs])
    out = []
    for k, link in enumerate(live):
        if k % 9 == 3:
            out.append((k % n, k % n))
        out.append(tuple(link))
    return np.array(out)


def few_random(n, count=127, seed=7):
    """127 links are 254 entries: no cut is possible."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, count)
    return np.stack([a, (a + 1 + rng.integers(0, n - 1, count)) % n], 1)


def shifted_rings(n):
    """rings behind one more link (0, 1): cells 0 and 1 have 5 entries, every later segment of 4 starts at 2 modulo 4,
    and every multiple of 256 cuts one into two pieces of two."""
    return np.concatenate([[(0, 1)], rings(n, 1, 5)])


UNCUT_LAYOUTS = {"rings": (1000, lambda n: rings(n, 1, 7)), "hub of 256": (600, rings_with_hub), "127 links": (500, few_random)}


# ---- lattice inputs: every sum and update of a step exact ---------------------------------------------------------
LATTICE_N, LATTICE_SPACING, LATTICE_STRENGTH, LATTICE_DT, LATTICE_HUB = 512, 8, 2.0 ** -7, 2.0 ** -2, 200


def lattice_rows(n_floats=3):
    """Cell i at x = 8 (i - 256), y = z = 0."""
    X = np.zeros((LATTICE_N, n_floats), f32)
    X[:, 0] = LATTICE_SPACING * (np.arange(LATTICE_N) - LATTICE_N // 2)
    return X


def lattice_links():
    """A chain, a hub of 300 links (cell 200 with cells 0 .. 99 and 300 .. 499, either way round), 150 random links
    and an inert link every 11 slots."""
    rng = np.random.default_rng(21)
    chain = [(i, i + 1) if i % 2 else (i + 1, i) for i in range(LATTICE_N - 1)]
    partners = list(range(100)) + list(range(300, 500))
    hub = [(LATTICE_HUB, k) if k % 3 else (k, LATTICE_HUB) for k in partners]
    a = rng.integers(0, LATTICE_N, 150)
    rand = np.stack([a, (a + 1 + rng.integers(0, LATTICE_N - 1, 150)) % LATTICE_N], 1)
    live = np.concatenate([chain, hub, rand])
    live = live[rng.permutation(len(live))]
    out = []
    for k, link in enumerate(live):
        if k % 11 == 4:
            out.append((k % LATTICE_N, k % LATTICE_N))
        out.append(tuple(link))
    return np.array(out)


def lattice_steps_float64(X, links, strength, steps, dt):
    """The step of links_tile in binary64 for cells on the x axis that never come within 1 of each other (asserted):
    a link's term is strength sign(x_a - x_b), no friction term, the mean right-hand side subtracted.  Returns the x
    coordinates and velocities, and the smallest distance between two cells seen."""
    x = X[:, 0].astype(np.float64)
    links = np.asarray(links).reshape(-1, 2)
    links = links[links[:, 0] != links[:, 1]]
    closest = np.inf

    def rhs(y):
        nonlocal closest
        closest = min(closest, np.diff(np.sort(y)).min())
        term = strength * np.sign(y[links[:, 0]] - y[links[:, 1]])
        d = np.zeros(len(y))
        np.add.at(d, links[:, 0], -term)
        np.add.at(d, links[:, 1], term)
        return d - d.sum() / len(y)

    v = np.zeros(len(x))
    for _ in range(steps):
        d = rhs(x)
        d1 = rhs(x + d * dt)
        v = (d + d1) * 0.5
        x = x + v * dt
    assert closest >= 1.0
    return x, v
