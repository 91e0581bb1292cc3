"""The polarity force library (include/polarity.cuh) at the edges of its formulas, on the host: the cases of
tests/polarity_cases.py evaluated by a g++ build of the header against oracle/yalla_host.hpp (binary32,
-ffp-contract=off, dist = sqrtf(fmaf(z, z, fmaf(y, y, x * x))) as ya::dist3 gives it in the exact tier) and held to
the float64 statement of tests/polarity_statement.py by the rule of tests/polarity_pairs_support.py.  The same
cases run inside the force kernels in tests/test_polarity_pairs_gpu.py.

Host yardsticks on the sweep ranges (this CPU, glibc libm): max |F - F64| / max(1, |F64|) of the binary32
evaluation alone and the largest conditioning term c_k, over this module's 800 evaluations per function and over
20 000 per function drawn from the same ranges with another seed:

    function                             error, 800   c_k, 800    error, 20 000   c_k, 20 000
    unidirectional_polarization_force    3.0e-7       0           4.2e-7          0
    bidirectional_polarization_force     2.2e-7       0           4.1e-7          0
    bending_force                        4.8e-7       4.3e-7      5.2e-7          6.7e-7
    apical_constriction_force            5.1e-7       3.6e-7      9.0e-7          8.9e-7
    migration_force                      4.5e-7       0           3.5e-7          0

All below the 2.5e-6 the binary32 evaluation alone is allowed on the sweep and the 1e-6 of c_k.  Two ranges were
narrowed to get there (tests/polarity_cases.py): with pref_angle in pi/2 +- 0.5 apical_constriction_force's c_k
reached 1.05e-6, and with |dot| up to 1 migration_force's error reached 6.1e-6 (orthonormal() next to r parallel
to p).  Over all cases the largest c_k is 4.4e-4, at an axis pair.

With dist one ulp LOW -- what a <= 1 ulp square root may hand over, and what v_sqrt_f32 does hand over for 2 % of
the axis pairs (test_polarity_pairs_gpu.py) -- the quotient r.z / dist of an axis pair exceeds 1: before pt_to_pol
clamped it, 392 of these records were NaN."""
import numpy as np
import pytest

import polarity_cases
import polarity_pairs_support as sup
import polarity_statement as st


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("polarity_pairs")
    built = polarity_cases.write(str(tmp / "cases.bin"))
    cells = sup.Cells(built)
    host = sup.host_records(str(tmp), str(tmp / "cases.bin"))
    return cells, host


def test_the_generator_keeps_what_it_promises():
    built = polarity_cases.build()
    again = polarity_cases.build()
    assert np.array_equal(built["cases"].view(np.uint32), again["cases"].view(np.uint32))
    cells = sup.Cells(built)
    names = set(built["names"])
    # isolated pairs: Xj on a lattice site of its own, |r| < 1, so cells of different pairs are more than 1 apart
    sites = cells.X[1::2, :3]
    assert np.array_equal(sites, np.round(sites / 3) * 3) and len(np.unique(sites, axis=0)) == len(sites)
    assert cells.true_dist.max() < 1 and cells.true_dist.min() >= 0.5
    assert np.abs(cells.X[:, :3]).max() < polarity_cases.GRID_SIZE / 2 - 1
    # the sweep, as realised
    s = cells.sweep
    assert [int((s & (cells.tag == t)).sum()) for t in range(5)] == [800] * 5
    assert cells.X[s, 3].min() >= 0.2 and cells.X[s, 3].max() <= np.pi - 0.2 and np.abs(cells.X[s, 4]).max() <= np.pi + 1e-6
    assert (np.abs(cells.r[s, 2]) / cells.true_dist[s]).max() <= 0.95
    # migration_force: no dot product within 1e-3 of a threshold, edge cases included (NaN: the 0 / 0 cases)
    for i in np.flatnonzero(cells.tag == st.MIGRATION):
        dots = st.migration_dots(cells.X[i].astype(np.float64), cells.r[i].astype(np.float64), cells.true_dist[i])
        assert all(np.isnan(d) or abs(abs(d) - 0.15) >= 1e-3 for d in dots), cells.names[i]
        assert not s[i] or max(abs(d) for d in dots) <= 0.9 + 1e-3
    apical = s & (cells.tag == st.APICAL)
    assert np.abs(cells.pref[apical] - np.pi / 2).max() <= 0.25 + 1e-6
    # every named edge
    axis = [n for n in names if n.startswith("axis r=(")]
    ds = {n.split(" d=")[1] for n in axis if " d=" in n}
    assert len(ds) == polarity_cases.AXIS_D + len(polarity_cases.UNDERSHOOT_D)
    assert all(repr(d) in ds for d in polarity_cases.NAMED_D + polarity_cases.UNDERSHOOT_D)
    forms = [f"({f},{z}d) eps={e}" for f in ("+e,0", "0,+e", "-e,+0", "-e,-0") for z in "+-"
             for e in ("quarter", "half", "2^-12d")] + ["(0,0,+d) eps=None", "(0,0,-d) eps=None"]
    for d in polarity_cases.NAMED_D:
        for form in forms:
            assert f"axis r={form} d={d!r}" in names
    for form in forms:
        assert sum(n.startswith("axis r=" + form) for n in axis) >= 4, form
    for ratio in polarity_cases.CAP_RATIOS:
        assert sum(n.startswith(f"cap |r.z|/dist={ratio!r} ") for n in names) == 4
    top = [i for i, n in enumerate(cells.names) if n.startswith(f"cap |r.z|/dist={polarity_cases.CAP_RATIOS[-1]!r}")]
    q = np.abs(cells.r[top, 2]) / cells.true_dist[top]
    assert (q >= 1 - 2.0 ** -22).all() and (q < 1).all()
    for theta in polarity_cases.THETA_EDGES:
        assert sum(n.startswith(f"theta_i={theta!r} ") for n in names) >= 2
    for who in ("Xi", "Xj", "both"):
        assert sum(n.startswith(f"unpolarised {who} ") for n in names) == 5
    for head in ("phi_i-phi_rhat=0 ", "phi_i-phi_rhat=-pi", "phi_i-phi_rhat=+pi", "phi across the wrap", "atan2f(+0,+0)",
                 "atan2f(-0,+0)", "atan2f(+0,-0)", "atan2f(-0,-0)", "migration Xi.theta=Xi.phi=0",
                 "migration partner's polarity (0,0)", "migration partner's polarity (1e-11,0)",
                 "migration partner's polarity (1e-09,0)", "migration r parallel to p (0/0)"):
        assert any(n.startswith(head) for n in names), head


def test_conditioning_terms_stay_within_their_bounds(world):
    cells, host = world
    _, c = cells.statement(host[0, :, 0])
    assert c[cells.sweep].max() <= 1e-6
    assert c.max() <= 1e-3


def test_host_evaluation_against_the_statement(world):
    cells, host = world
    F64, c = cells.statement(host[0, :, 0])
    nan = np.isnan(host[0, :, 1:])
    assert np.array_equal(nan.any(axis=1), sup.documented_nan(cells)), sup.worst(cells, nan)
    assert np.array_equal(nan, np.isnan(F64))  # the statement divides 0 by 0 in the same components
    print("host: largest |F - F64| / max(1, |F64|) and largest c_k on the sweep, per function:")
    with np.errstate(invalid="ignore"):
        alone = np.abs(host[0, :, 1:] - F64) / np.maximum(1, np.abs(F64))
    for tag in range(5):
        mine = cells.sweep & (cells.tag == tag)
        print(f"  {st.NAMES[tag]:36s} sweep {alone[mine].max():.2e}  c {c[mine].max():.2e}")
    assert alone[cells.sweep].max() < 2.5e-6
    bad = sup.excess(host[0], F64, c) > 0
    assert not bad.any(), sup.worst(cells, bad)


def test_host_decisions_agree_with_the_statement(world):
    cells, host = world
    nan_case = sup.documented_nan(cells)
    for i in range(cells.n):
        zero = st.decided_zeros(cells.tag[i], cells.X[i].astype(np.float64), cells.r[i].astype(np.float64),
                                float(host[0, i, 0]), st.quotient32(cells.r[i, 2], host[0, i, 0]))
        if nan_case[i]:
            zero[:3] = False
        assert (host[0, i, 1:][zero] == 0).all(), cells.names[i]


def test_a_dist_one_ulp_off_stays_finite(world):
    """The NaN of an under-estimated dist on the CPU: every record at dist - 1 ulp and dist + 1 ulp is finite (the
    documented 0 / 0 of migration_force aside), and still meets the tolerance rule for the dist it was given."""
    cells, host = world
    for shifted in (host[1], host[2]):
        bad = ~np.isfinite(shifted[:, 1:]) & ~sup.documented_nan(cells)[:, None]
        assert not bad.any(), sup.worst(cells, bad)
        F64, c = cells.statement(shifted[:, 0])
        bad = sup.excess(shifted, F64, c) > 0
        assert not bad.any(), sup.worst(cells, bad)


def test_a_column_on_the_polar_axis_steps_in_the_oracle(oracle):
    """End to end (the device tiers: tests/test_polarity_pairs_gpu.py): passive_growth_grid, every neighbour pair
    of a 48-cell column an axis pair."""
    X0, types = sup.column_and_sheet()
    sup.check_column(oracle, sup.column_statement(X0, types, 0.05), X0, types)
