"""Shared by tests/test_polarity_pairs.py (CPU) and tests/test_polarity_pairs_gpu.py: the host evaluation of
tests/polarity_cases.py's cases (g++ against oracle/yalla_host.hpp, the style of tests/test_polarity_host.py), the
float64 statement of every cell computed once, and the tolerance rule

    |F_k - F64_k| <= 1e-5 * max(1, |F64_k|) + c_k

where 1e-5 is the project's contract for libm functors and for the fast tier, and c_k is the statement's own
change under +-1 binary32 ulp of the quotient r.z / dist (tests/polarity_statement.py)."""
import os
import subprocess

import numpy as np

import polarity_cases
import polarity_statement as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5

# include/polarity.cuh on the host with dist = sqrtf(fmaf(z, z, fmaf(y, y, x * x))) -- what ya::dist3 returns in
# the exact tier -- then with that dist one ulp lower and one ulp higher (what a <= 1 ulp square root may hand
# over).  Records as tests/native/test_polarity_pairs.cu writes them: per cell dist and the returned Po_cell.
HOST_SRC = r'''
#include <stdio.h>
#include <math.h>
#include <vector>
#include "yalla_host.hpp"
#include "polarity.cuh"
static Po_cell library(int tag, Po_cell Xi, Po_cell r, float dist, float pref)
{
    if (tag == 0) return unidirectional_polarization_force(Xi, Polarity{Xi.theta - r.theta, Xi.phi - r.phi});
    if (tag == 1) return bidirectional_polarization_force(Xi, Polarity{Xi.theta - r.theta, Xi.phi - r.phi});
    if (tag == 2) return bending_force(Xi, r, dist);
    if (tag == 3) return apical_constriction_force(Xi, r, dist, pref);
    return migration_force(Xi, r, dist);
}
int main(int argc, char** argv)
{
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<float> cases;
    float c[12];
    while (fread(c, sizeof(float), 12, in) == 12) cases.insert(cases.end(), c, c + 12);
    for (int shift = 0; shift < 3; shift++)  // dist, one ulp lower, one ulp higher
        for (size_t k = 0; k < cases.size(); k += 12)
            for (int side = 0; side < 2; side++) {
                const float* a = &cases[k + 5 * side];
                const float* b = &cases[k + 5 * (1 - side)];
                Po_cell Xi{a[0], a[1], a[2], a[3], a[4]}, Xj{b[0], b[1], b[2], b[3], b[4]};
                Po_cell r = Xi - Xj;
                float dist = sqrtf(fmaf(r.z, r.z, fmaf(r.y, r.y, r.x * r.x)));
                if (shift == 1) dist = nextafterf(dist, 0.f);
                if (shift == 2) dist = nextafterf(dist, 2.f);
                Po_cell F = library((int)cases[k + 10], Xi, r, dist, cases[k + 11]);
                float rec[6] = {dist, F.x, F.y, F.z, F.theta, F.phi};
                fwrite(rec, sizeof(float), 6, out);
            }
    fclose(out);
    return 0;
}
'''


def host_records(tmp_dir, cases_path):
    """(3, n, 6): the host program's records at dist, dist - 1 ulp and dist + 1 ulp.  -ffp-contract=off: the
    host yardsticks of test_polarity_pairs.py's docstring hold for uncontracted binary32 only."""
    src, exe, out = (os.path.join(tmp_dir, name) for name in ("pairs_host.cpp", "pairs_host", "host_records.bin"))
    with open(src, "w") as f:
        f.write(HOST_SRC)
    subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "oracle"),
                    "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True, capture_output=True)
    subprocess.run([exe, cases_path, out], check=True, timeout=120)
    return np.fromfile(out, "<f4").reshape(3, -1, 6)


class Cells:
    """The cases cell by cell, and the statement of each cell for a given recorded dist (cached per dist)."""

    def __init__(self, built):
        self.built = built
        self.X, self.partner, self.tag, self.pref = polarity_cases.cells(built["cases"])
        self.n = len(self.X)
        self.r = polarity_cases.difference(self.X, self.X[self.partner])
        self.sweep = np.repeat(built["sweep"], 2)
        self.names = [name for name in built["names"] for _ in range(2)]
        self.true_dist = np.sqrt((self.r[:, :3].astype(np.float64) ** 2).sum(axis=1))
        self._cache = {}

    def statement(self, dist):
        """(F64, c): (n, 5) each, with `dist` (n binary32 numbers) and its binary32 quotient as facts."""
        key = np.asarray(dist, np.float32).tobytes()
        if key not in self._cache:
            F, c = np.empty((self.n, 5)), np.empty((self.n, 5))
            for i in range(self.n):
                F[i], c[i] = st.evaluate(self.tag[i], self.X[i], self.r[i], dist[i], float(self.pref[i]))
            self._cache[key] = (F, c)
        return self._cache[key]


def documented_nan(cells):
    """The cells of the one documented NaN: migration_force with r parallel to p, where the reference divides 0 by 0."""
    return np.array([n.startswith("migration r parallel to p (0/0)") for n in cells.names])


def excess(records, F64, c):
    """|F - F64| - (1e-5 max(1, |F64|) + c) per cell and component; NaN where either side is NaN."""
    with np.errstate(invalid="ignore"):
        return np.abs(records[:, 1:].astype(np.float64) - F64) - (RTOL * np.maximum(1, np.abs(F64)) + c)


def worst(cells, bad):
    """A readable list of the cells of a boolean mask (for assertion messages)."""
    rows = np.flatnonzero(bad.any(axis=1) if bad.ndim == 2 else bad)
    return f"{len(rows)} cells, first: " + "; ".join(
        f"cell {i} {st.NAMES[cells.tag[i]]} {cells.names[i] or 'sweep'}" for i in rows[:6])


# ---- end to end: a column of epithelial cells exactly on the polar axis ------------------------------------------

def column_and_sheet(seed=11):
    """48 cells on the z axis (x = y = 0 exactly) at spacings in [0.55, 0.95] -- every neighbour pair is an
    axis pair, r.z / dist = +-1 -- and, 4 cube lengths aside, a 6 x 6 sheet in the xy plane (r.z / dist = 0).
    All epithelium; polarities roughly normal to the layer, as bending_force wants them."""
    rng = np.random.default_rng(seed)
    X = np.zeros((48 + 36, 5))
    # spacings on a grid of 2^-13, so that every z is exact and r.z IS the spacing; every sixth one a distance at
    # which the bare v_sqrt_f32 of an MI355X returns one ulp less than |r.z| (three of the 97 such in [0.5, 1) with
    # 11 trailing zero bits): there the fast tier's r.z / dist exceeds 1
    spacing = np.round(rng.uniform(0.55, 0.95, 48) * 2.0 ** 13) / 2.0 ** 13
    spacing[3::6] = np.array([0x3f123800, 0x3f1bf800, 0x3f1c2800] * 3, np.uint32).view(np.float32)[:len(spacing[3::6])]
    z = np.cumsum(spacing)
    X[:48, 2] = z - np.round(z.mean())
    X[:48, 3] = rng.uniform(0.9, np.pi - 0.9, 48)
    X[:48, 4] = rng.uniform(-0.5, 0.5, 48)
    gx, gy = np.meshgrid(np.arange(6), np.arange(6))
    X[48:, 0] = 4 + 0.75 * gx.ravel() + rng.normal(size=36) * 0.02
    X[48:, 1] = 0.75 * gy.ravel() + rng.normal(size=36) * 0.02
    X[48:, 3] = rng.uniform(0.2, 0.5, 36)
    X[48:, 4] = rng.uniform(-np.pi, np.pi, 36)
    X = X.astype(np.float32)
    assert (X[:48, :2] == 0).all() and np.array_equal(np.diff(X[:48, 2].astype(np.float64)), spacing[1:])
    return X, np.ones(len(X), np.int32)


def column_statement(X0, types, dt):
    """The Heun step of tests/test_model_functors_independent.py's statement (relu_w_epithelium on the grid), and
    per cell and component how far it moves when every pair's quotient r.z / dist -- as binary32 -- is one ulp
    lower or higher (clamped): the conditioning term pushed through the whole step."""
    import test_model_functors_independent as mfi

    def functor(toward):
        def shifted(Xi, r, dist, i, j, types, mes_nbs, epi_nbs):
            dF = mfi.relu_w_epithelium(Xi, r, dist, i, j, types, mes_nbs, epi_nbs)
            if toward and i != j and dist <= mfi.R_MAX:
                q = np.float32(min(max(st.quotient32(r[2], dist), -1.0), 1.0))
                moved = float(np.nextafter(q, np.float32(toward)))
                dF = dF + 0.15 * (st.bending_force(Xi, r, dist, moved) - st.bending_force(Xi, r, dist, float(q)))
            return dF
        return shifted

    X64 = X0.astype(np.float64)
    X_ref, mes, epi = mfi.heun_step(functor(0), X64, types, dt, cut_off=1.0)
    widening = np.zeros_like(X_ref)
    for toward in (-np.inf, np.inf):
        widening = np.maximum(widening, np.abs(mfi.heun_step(functor(toward), X64, types, dt, cut_off=1.0)[0] - X_ref))
    return X_ref, mes, epi, widening


def check_column(lib, statement, X0, types, dt=0.05):
    """One step of passive_growth_grid on `lib`: finite, inside test_model_functors_independent.py's bounds widened
    by the conditioning term, neighbour counters exact."""
    import test_model_functors_independent as mfi
    X_ref, mes_ref, epi_ref, widening = statement
    X, mes, epi = mfi.run_backend(lib, X0, types, dt, model="passive_growth_grid")
    assert np.isfinite(X).all(), np.argwhere(~np.isfinite(X))[:8]
    assert np.array_equal(mes, mes_ref) and np.array_equal(epi, epi_ref)
    assert (epi_ref[:48] >= 1).all() and np.abs(X_ref[:48, 3:] - X0[:48, 3:]).max() > 1e-4, "bending never acted"
    moved = np.abs(X_ref - X0).max()
    error = np.abs(X - X_ref)
    print(f"positions {error[:, :3].max():.2e}, polarities {error[:, 3:].max():.2e}, widening {widening.max():.2e}")
    assert (error[:, :3] <= 2e-5 * max(np.abs(X_ref[:, :3]).max(), 1.0) + widening[:, :3]).all()
    assert (error[:, 3:] <= 1e-4 * max(moved, 1e-3) + 2e-6 + widening[:, 3:]).all()
