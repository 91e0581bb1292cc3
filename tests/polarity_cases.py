"""The cases of tests/test_polarity_pairs*.py: pairs of Po_cells, each pair alone at its own site of a lattice
with spacing 3, so that inside a force kernel with cut-off 1 every cell has exactly one partner and its force is
one pair term.  Seeded and deterministic.  `write(path)` stores them as a flat binary32 file, 12 numbers per case:
Xi[5], Xj[5], the function's tag (tests/polarity_statement.py) and a pref_angle; cell 2c is Xi and cell 2c + 1 is
Xj of case c, so every case is evaluated in both directions (r and -r).

Sweep cases, 400 per function: theta_i, theta_j in [0.2, pi - 0.2], phi in [-pi, pi], dist in [0.5, 1),
|r.z| / dist <= 0.95, pref_angle in pi/2 +- 0.25; for migration_force both dot products at least 1e-3 away from
+-0.15 and below 0.9 in size.  (The last two ranges are narrower than the others need: over 20 000 evaluations per
function pref_angle in pi/2 +- 0.5 carried a conditioning term of 1.05e-6, and migration_force's orthonormal(),
which loses 1 / sin of the angle between r and p, a host error of 6.1e-6 -- beyond the 1e-6 and 2.5e-6 the sweep
is held to.)  Edge cases carry names (`names`); tests/test_polarity_pairs.py holds the list to what the generator
promises.

What binary32 lets a site hold.  r = Xi - Xj is computed by the kernel, so an offset is exactly what the two
stored coordinates differ by.  Xj sits on the site and Xi = fl(site + r): the sites of the plane z = 0 give every
24-bit d as r.z; an offset in x is a multiple of ulp(site.x) (any binary32 number in the column x = 0, 2^-22 in
the columns x = +-3, ...; offsets in y sit in the rows y = +-3, ... and come on a grain of 2^-22 at best, the row
y = 0 being kept for the cases that need it), and a -0 in r.y needs site.y = 0.  Cases are therefore dealt to sites by what they
need (`_Sites`), the named values of d first, and every tiny offset is checked AS REALISED against the inequality
that defines it (eps^2 below a quarter ulp of d^2, just above half an ulp, 2^-12 d to the site's grain).

theta_i = 1e-9 and float(pi) (1 / sin of 1e9 and 1.1e7) go through the two polarization forces only: there no
quotient enters and the conditioning term is 0.  Through bending_force they would carry a conditioning term of
60 and 0.7, beyond the 1e-3 every case is held to.  Axis and cap cases draw theta in [0.8, pi - 0.8]: the pole's
3.5e-4 step of arccos times |prod| / sin(theta_i) stays below 1e-3."""
import numpy as np

import polarity_statement as st

SPACING = 3
HALF = 20                      # sites 3 * (-20 .. 20): inside a grid of 128 cubes of size 1
GRID_SIZE = 128
F32 = np.float32
PI32 = float(F32(np.pi))
THETA_EDGES = (0.0, 1e-11, 1e-9, 1e-3, float(F32(np.pi / 2)), PI32, float(F32(PI32 - 1e-3)))
AXIS_D = 64
NAMED_D = (0.5, 0.75, float(np.nextafter(F32(1), F32(0))))
# d at which the bare v_sqrt_f32 of an MI355X returns the root of RN(d * d) one ulp BELOW d (eight of the 171 143 in
# [0.5, 1) that a scan found; bit patterns): with these on the axis the fast tier's r.z / dist exceeds 1.
UNDERSHOOT_D = tuple(float(np.uint32(bits).view(np.float32)) for bits in (
    0x3f041725, 0x3f042800, 0x3f06f5eb, 0x3f07445b, 0x3f078184, 0x3f0b60ef, 0x3f1c9886, 0x3f1c99bd))
CAP_RATIOS = (0.95, 0.97, 0.99, 0.999, 0.9999, 1 - 2.0 ** -16, 1 - 2.0 ** -20, 1 - 2.0 ** -22, 1 - 2.0 ** -23)


def f32(x):
    return float(F32(x))


def ulp32(x):
    return float(np.spacing(F32(abs(x))))


class _Sites:
    """Lattice sites by what a case needs: 'x' / 'y' a tiny offset in x / y (plane z = 0, smallest |x| / |y|
    first), 'y0' a signed zero in r.y (row y = 0 of that plane, smallest |x| first), 'z0' an exact d only, None
    anything."""

    def __init__(self):
        span = range(-HALF, HALF + 1)
        plane = [(a, b) for a in span for b in span]
        self.x = sorted((s for s in plane if abs(s[0]) < abs(s[1])), key=lambda s: (abs(s[0]), abs(s[1]), s))[::-1]
        self.y = sorted((s for s in plane if 0 < abs(s[1]) < abs(s[0])), key=lambda s: (abs(s[1]), abs(s[0]), s))[::-1]
        self.row = sorted((s for s in plane if s[1] == 0 and s[0] != 0), key=lambda s: (abs(s[0]), s))[::-1]
        self.z0 = sorted((s for s in plane if abs(s[0]) == abs(s[1])), key=lambda s: (abs(s[0]), s))[::-1]
        self.rest = sorted(((a, b, c) for a in span for b in span for c in span if c != 0),
                           key=lambda s: (max(map(abs, s)), s))[::-1]

    def take(self, need):
        if need == "y0":
            a, b = self.row.pop()
        elif need == "x":
            a, b = self.x.pop()
        elif need == "y":
            a, b = self.y.pop()
        elif need == "z0":
            a, b = self.z0.pop() if self.z0 else self.x.pop(0)  # (the far end of the x list: coarse, exact in z)
        else:
            a, b, c = self.rest.pop()
            return np.array([a, b, c], np.float64) * SPACING
        return np.array([a, b, 0], np.float64) * SPACING


def _grain(site_coordinate):
    return ulp32(site_coordinate) if site_coordinate != 0 else 2.0 ** -60


def _eps(kind, d, site_coordinate):
    """The tiny offset of `kind` next to an axis pair of length d, on the grain of the site."""
    g = _grain(site_coordinate)
    dd = f32(F32(d) * F32(d))
    if kind == "quarter":
        e = max(2.0 ** -30, g)
        assert e * e < 0.25 * ulp32(dd)
    elif kind == "half":
        h = 0.5 * ulp32(dd)
        if g < 2.0 ** -40:
            e = f32(np.sqrt(h))
            while e * e <= h:
                e = float(np.nextafter(F32(e), F32(1)))
        else:
            e = np.ceil(np.sqrt(h) / g) * g
            if e * e <= h:
                e += g
        assert h < e * e < 1.25 * h, (e, h)
    else:
        e = 2.0 ** -12 * d if g < 2.0 ** -40 else np.round(2.0 ** -12 * d / g) * g
        assert abs(e / (2.0 ** -12 * d) - 1) < 2.0 ** -5
    return e


class _Builder:
    def __init__(self):
        self.sites = _Sites()
        self.rows, self.names, self.sweep = [], [], []

    def add(self, name, tag, r, pol_i, pol_j, need=None, pref=np.pi / 2, sweep=False, exact=()):
        """The pair with Xj on a site and Xi = fl(site + r); `exact` lists the components of r that must be
        realised bit for bit."""
        site = self.sites.take(need)
        Xj = np.array([*site, *pol_j], np.float64).astype(F32)
        Xi = np.array([*(site + np.asarray(r, np.float64)[:3]), *pol_i], np.float64).astype(F32)
        for k in range(3):  # signed zeros of r are the stored signs (site 0: -0 + -(+0) = -0)
            if r[k] == 0 and np.signbit(r[k]):
                assert site[k] == 0
                Xi[k] = F32(-0.0)
        realised = Xi + F32(-1) * Xj  # dtypes.cuh: a - b is a + (-1 * b)
        for k in exact:
            assert realised[k] == F32(r[k]) and np.signbit(realised[k]) == np.signbit(F32(r[k])), (name, k, r)
        self.rows.append(np.concatenate([Xi, Xj, [F32(tag), F32(pref)]]).astype(F32))
        self.names.append(name)
        self.sweep.append(sweep)
        return realised


def difference(Xi, Xj):
    """r as every backend computes it (include/dtypes.cuh: a - b is a + (-1 * b)), binary32."""
    return (np.asarray(Xi, F32) + F32(-1) * np.asarray(Xj, F32)).astype(F32)


def distance32(r):
    """sqrtf(fmaf(z, z, fmaf(y, y, x * x))) in binary32 (each step rounded once; the products are exact in
    float64 and the sums are rounded from float64, which differs from one rounding only in double-rounding
    ties -- the tests take the host program's dist as the fact, this one serves the generator's own margins)."""
    x, y, z = (np.float64(F32(v)) for v in r[:3])
    s = np.float64(F32(x * x))
    s = np.float64(F32(y * y + s))
    s = np.float64(F32(z * z + s))
    return float(F32(np.sqrt(s)))


def migration_margin(r, pol_i, pol_j, largest=1.0):
    """How far the four dot products of the pair (both directions) stay from -0.15 and 0.15; -1 if one exceeds
    `largest` in size."""
    Xi, Xj = np.array([*r[:3], *pol_i], np.float64), np.array([0, 0, 0, *pol_j], np.float64)
    dist = float(np.sqrt((Xi[:3] ** 2).sum()))
    dots = st.migration_dots(Xi, Xi - Xj, dist) + st.migration_dots(Xj, Xj - Xi, dist)
    return -1 if max(abs(x) for x in dots) > largest else min(abs(abs(x) - 0.15) for x in dots)


def build(seed=20251020, sweep_per_function=400):
    rng = np.random.default_rng(seed)
    b = _Builder()
    mid = lambda: rng.uniform(0.8, np.pi - 0.8)  # a polarity for axis and cap cases (module docstring)

    def pols(tag, r):
        """Two such polarities; for migration_force drawn again until no dot product is near +-0.15."""
        while True:
            pol_i, pol_j = (mid(), rng.uniform(-3, 3)), (mid(), rng.uniform(-3, 3))
            if tag != st.MIGRATION or migration_margin(r, pol_i, pol_j) >= 2e-3:
                return pol_i, pol_j

    # -- atan2f at zeros of either sign (a -0 in r needs a site coordinate 0), the smallest offset ----------------
    b.add("atan2f(-0,-0) at the origin", st.BENDING, (-0.0, -0.0, 0.75), (1.0, 0.3), (2.0, 0.5), "z0", exact=(0, 1, 2))
    b.add("atan2f(+0,-0)", st.BENDING, (-0.0, 0.0, -0.625), (1.0, 0.3), (2.0, 0.5), "x", exact=(0, 1, 2))
    b.add("axis r=(2^-30,0,+0.75)", st.BENDING, (2.0 ** -30, 0.0, 0.75), (1.3, 0.3), (1.9, -1.0), "x", exact=(0, 1, 2))

    # -- axis pairs ---------------------------------------------------------------------------------------------
    ds = np.unique(np.concatenate([np.asarray(NAMED_D, F32),
                                   (0.5 + 0.5 * rng.random(AXIS_D - len(NAMED_D))).astype(F32)])).astype(np.float64)
    assert len(ds) == AXIS_D and ds.min() == 0.5 and ds.max() < 1
    forms = [("0,0", None)] + [(f, e) for f in ("+e,0", "0,+e", "-e,+0") for e in ("quarter", "half", "2^-12d")]
    combos = [(f, e, s) for f, e in forms for s in (1, -1)]  # 20
    minus_zero = [("-e,-0", e, s) for e in ("quarter", "half", "2^-12d") for s in (1, -1)]  # 6, row y = 0 only
    axis_tags = (st.BENDING, st.APICAL, st.MIGRATION)
    todo = [(d, c) for d in NAMED_D for c in combos + minus_zero]  # the named d first: the finest sites
    todo += [(ds[k], minus_zero[m]) for m, k in enumerate((5, 18, 29, 40, 51, 61))]
    todo += [(d, c) for d in UNDERSHOOT_D for c in combos]
    todo += [(ds[k], combos[(4 * k + m) % 20]) for k in range(AXIS_D) for m in range(4)]
    for n, (d, (form, kind, sign)) in enumerate(todo):
        need = {"0,0": "z0", "+e,0": "x", "0,+e": "y", "-e,+0": "x", "-e,-0": "y0"}[form]
        site = b.sites
        # the offset depends on the site the case is about to get: look at it before taking it
        nxt = {"z0": None, "x": site.x[-1][0], "y": site.y[-1][1], "y0": site.row[-1][0]}[need]
        e = 0.0 if form == "0,0" else _eps(kind, d, nxt * SPACING)
        r = {"0,0": (0.0, 0.0), "+e,0": (e, 0.0), "0,+e": (0.0, e), "-e,+0": (-e, 0.0), "-e,-0": (-e, -0.0)}[form]
        tag = axis_tags[n % 3]
        b.add(f"axis r=({form},{'+' if sign > 0 else '-'}d) eps={kind} d={float(d)!r}", tag, (*r, sign * float(d)),
              *pols(tag, (*r, sign * d)), need, pref=rng.uniform(1.1, 2.0), exact=(0, 1, 2))

    # -- caps: |r.z| / dist from 0.95 up to 1 - 2^-23 ---------------------------------------------------------------
    for n, ratio in enumerate(CAP_RATIOS):
        for sign in (1, -1):
            for axis in ("x", "y"):
                d = f32(rng.uniform(0.5, 0.9))
                t = d * np.sqrt(1 - ratio * ratio) / ratio
                r = (t, 0.0, sign * d) if axis == "x" else (0.0, -t, sign * d)
                b.add(f"cap |r.z|/dist={ratio!r} z{'+' if sign > 0 else '-'} along {axis}", axis_tags[n % 3], r,
                      *pols(axis_tags[n % 3], r), axis, pref=rng.uniform(1.1, 2.0), exact=(2,))

    # -- theta_i at its edges; the unpolarised cell as Xi, as Xj and as both --------------------------------------
    generic_r = (0.31, -0.22, 0.43)  # |r.z| / dist = 0.75, phi_rhat = -0.617
    for theta in THETA_EDGES:
        tags = (st.UNIDIRECTIONAL, st.BIDIRECTIONAL) if theta in (1e-9, PI32) else range(5)
        for tag in tags:
            # phi_i - phi_rhat and phi_i - phi_j well away from 0 and +-pi: 1 / sin(theta_i) multiplies their sine
            b.add(f"theta_i={theta!r} {st.NAMES[tag]}", tag, generic_r, (theta, 0.4), (1.1, -0.7), pref=1.3)
    for who, pol_i, pol_j in (("Xi", (0, 0), (1.2, 0.8)), ("Xj", (0.9, -2.0), (0, 0)), ("both", (0, 0), (0, 0))):
        for tag in range(5):
            b.add(f"unpolarised {who} {st.NAMES[tag]}", tag, generic_r, pol_i, pol_j, pref=1.9)

    # -- phi_i - phi_rhat at 0 and +-pi (atan2f at a zero r.y of either sign), and across the wrap -----------------
    for tag in axis_tags:
        b.add(f"phi_i-phi_rhat=0 {st.NAMES[tag]}", tag, (0.5, 0.0, 0.3), (1.0, 0.0), (2.0, 0.5), None, exact=(1,))
        b.add(f"phi_i-phi_rhat=0 at pi {st.NAMES[tag]}", tag, (-0.5, 0.0, 0.3), (1.0, PI32), (2.0, 0.5), None,
              exact=(1,))
        b.add(f"phi_i-phi_rhat=-pi {st.NAMES[tag]}", tag, (-0.5, 0.0, -0.3), (1.0, 0.0), (0.7, -0.5), None, exact=(1,))
        b.add(f"phi_i-phi_rhat=+pi {st.NAMES[tag]}", tag, (-0.5, -0.0, 0.3), (2.0, 0.0), (0.7, 2.5), "y0", exact=(1,))
        b.add(f"atan2f(+0,+0) {st.NAMES[tag]}", tag, (0.0, 0.0, 0.6), (1.0, 0.3), (2.0, 0.5), None, exact=(0, 1))
        b.add(f"atan2f(-0,+0) {st.NAMES[tag]}", tag, (0.0, -0.0, -0.6), (1.0, 0.3), (2.0, 0.5), "y0", exact=(0, 1))
    for tag in range(5):
        b.add(f"phi across the wrap {st.NAMES[tag]}", tag, (0.2, 0.5, -0.4), (1.0, 3.1), (1.4, -3.1), pref=1.2)

    # -- migration_force's guards ----------------------------------------------------------------------------------
    for name, r in (("partner pushes", (0.3, 0.2, 0.6)), ("partner does not push", (0.3, 0.2, -0.6))):
        b.add(f"migration Xi.theta=Xi.phi=0, {name}", st.MIGRATION, r, (0, 0), (0.4, 1.0))
    for theta_j, phi_j in ((0, 0), (1e-11, 0), (1e-9, 0), (0, 1e-11), (0, 1e-9), (1e-11, 1e-11)):
        # Xi unpolarised: Xi - (Xi - Xj) recovers the partner's polarity bit for bit
        b.add(f"migration partner's polarity ({theta_j!r},{phi_j!r})", st.MIGRATION, (0.3, 0.2, 0.6), (0, 0),
              (theta_j, phi_j))
    for d in (0.5, 0.8125):
        b.add(f"migration r parallel to p (0/0) d={d!r}", st.MIGRATION, (0.0, 0.0, -d), (0.0, 1.0), (0.0, 1.0), "z0",
              exact=(0, 1, 2))
    n_edges = len(b.rows)

    # -- sweep ----------------------------------------------------------------------------------------------------------
    for tag in range(5):
        made = 0
        while made < sweep_per_function:
            dist = rng.uniform(0.5, 0.999)
            cos_t = rng.uniform(-0.949, 0.949)
            az = rng.uniform(-np.pi, np.pi)
            r = dist * np.array([np.sqrt(1 - cos_t ** 2) * np.cos(az), np.sqrt(1 - cos_t ** 2) * np.sin(az), cos_t])
            pol_i = (rng.uniform(0.2, np.pi - 0.2), rng.uniform(-np.pi, np.pi))
            pol_j = (rng.uniform(0.2, np.pi - 0.2), rng.uniform(-np.pi, np.pi))
            if tag == st.MIGRATION and migration_margin(r, pol_i, pol_j, largest=0.9) < 2e-3:
                continue  # (all four |dot| below 0.9: orthonormal() loses 1 / sin of the angle between r and p)
            b.add("", tag, r, pol_i, pol_j, pref=rng.uniform(np.pi / 2 - 0.25, np.pi / 2 + 0.25), sweep=True)
            made += 1

    cases = np.array(b.rows, F32)
    return {"cases": cases, "names": b.names, "sweep": np.array(b.sweep), "n_edges": n_edges}


def cells(cases):
    """(X, partner, tag, pref) per cell: cell 2c is Xi and cell 2c + 1 is Xj of case c."""
    n = 2 * len(cases)
    X = np.empty((n, 5), F32)
    X[0::2], X[1::2] = cases[:, 0:5], cases[:, 5:10]
    partner = np.arange(n) ^ 1
    return X, partner, np.repeat(cases[:, 10].astype(int), 2), np.repeat(cases[:, 11], 2)


def write(path, built=None):
    built = built or build()
    built["cases"].astype("<f4").tofile(path)
    return built


if __name__ == "__main__":
    import sys
    print(len(write(sys.argv[1])["cases"]), "cases")
