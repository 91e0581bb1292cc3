"""The polarity force library INSIDE the force kernels, both arithmetic tiers: tests/native/test_polarity_pairs.cu
(and its -DYA_ARITH_FAST build) steps the isolated pairs of tests/polarity_cases.py through Tile_solver,
Grid_solver (default kernel, force_variant 0 and 1) and Gabriel_solver under functors that record the `dist` the
kernel handed over and the Po_cell the library returned; the records are held to the float64 statement
(tests/polarity_statement.py) by the rule of tests/polarity_pairs_support.py, with the recorded dist as a fact.

Measured on an MI355X (the program prints it; the tests below assert what is a bound):

  exact tier  dist is the host's sqrtf(fmaf(z, z, fmaf(y, y, x * x))) bit for bit in all five kernels; ya::dist3
              never returns less than |z| for r = (0, 0, z) or (2^-13 z, 0, z), any binary32 z in [2^-6, 2^6).
  fast tier   dist (the bare v_sqrt_f32) is within 1.2 ulp of the float64 distance on these cases (bound: 2).
              It returns one ulp LESS than z for 2 053 716 of the 100 663 296 z on the axis (2.0 %; 171 143 of
              them in [0.5, 1)) and for 360 408 with x = 2^-13 z beside it: r.z / dist then exceeds 1.  Eight such
              d are among the axis cases (tests/polarity_cases.py UNDERSHOOT_D): 116 cells get a dist below
              |r.z|.  Built against pt_to_pol as it was before it clamped the quotient, the fast tier's program
              recorded NaN in dF.theta and dF.phi of 76 of those cells (bending_force and
              apical_constriction_force; migration_force lost its branches instead), in every kernel family;
              tests/test_polarity_pairs.py shows the same NaN on the CPU with dist lowered by one ulp.

Decisions: the components that are 0 by a decision of the code (tests/polarity_statement.py decided_zeros) are
exactly 0 in every record.  migration_force's branches need no record of their own: each fired branch adds a
vector of length 1, every case keeps its dot products 1e-3 away from the thresholds, so a record that fired
another set of branches than the statement misses the tolerance by about 1."""
import os
import re
import subprocess

import numpy as np
import pytest

import polarity_cases
import polarity_pairs_support as sup
import polarity_statement as st

NATIVE = os.path.join(sup.ROOT, "tests", "native")
SOLVERS = ("Tile_solver", "Grid_solver", "Grid_solver force_variant 0", "Grid_solver force_variant 1",
           "Gabriel_solver")
TIERS = {"exact": "test_polarity_pairs", "fast": "test_polarity_pairs_fast"}


def run_native(name, cases, records):
    exe = os.path.join(NATIVE, name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", NATIVE, name], check=True, capture_output=True)
    proc = subprocess.run([exe, cases, records], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "ALL POLARITY PAIR RUNS DONE" in proc.stdout, \
        proc.stdout[-2000:] + proc.stderr[-2000:]
    return proc.stdout


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("polarity_pairs_gpu")
    built = polarity_cases.write(str(tmp / "cases.bin"))
    cells = sup.Cells(built)
    host = sup.host_records(str(tmp), str(tmp / "cases.bin"))
    runs = {}
    for tier, name in TIERS.items():
        out = str(tmp / f"records_{tier}.bin")
        stdout = run_native(name, str(tmp / "cases.bin"), out)
        assert f"tier {tier}, {cells.n} cells" in stdout
        counts = re.search(r"dist3 below z: axis (\d+) offset (\d+) of (\d+)", stdout)
        lanes = re.search(r"several-lanes kernels against one lane: (\d+) cells differ", stdout)
        runs[tier] = {"records": np.fromfile(out, "<f4").reshape(len(SOLVERS), cells.n, 6), "stdout": stdout,
                      "undershoot": tuple(int(x) for x in counts.groups()), "lanes_differ": int(lanes.group(1))}
        print(tier, stdout)
    return cells, host, runs


@pytest.mark.gpu
@pytest.mark.parametrize("tier", TIERS)
def test_records_against_the_statement(world, tier):
    """Every record of every kernel family: finite (the documented 0 / 0 of migration_force aside, which must be
    NaN in the components where the host's is), within the tolerance rule, and 0 where a decision makes it 0."""
    cells, host, runs = world
    nan_case = sup.documented_nan(cells)
    for solver, records in zip(SOLVERS, runs[tier]["records"]):
        assert np.isfinite(records[:, 0]).all(), solver  # every cell met its partner
        bad = ~np.isfinite(records[:, 1:]) & ~nan_case[:, None]
        assert not bad.any(), solver + ": " + sup.worst(cells, bad)
        assert np.array_equal(np.isnan(records[nan_case, 1:]), np.isnan(host[0, nan_case, 1:])), solver
        F64, c = cells.statement(records[:, 0])
        assert c.max() <= 1e-3 and c[cells.sweep].max() <= 1e-6
        over = sup.excess(records, F64, c)
        print(f"{tier} {solver}: largest |F - F64| - c over max(1, |F64|): "
              f"{np.nanmax((over + sup.RTOL * np.maximum(1, np.abs(F64))) / np.maximum(1, np.abs(F64))):.2e}")
        assert not (over > 0).any(), solver + ": " + sup.worst(cells, over > 0)
        for i in range(cells.n):
            zero = st.decided_zeros(cells.tag[i], cells.X[i].astype(np.float64), cells.r[i].astype(np.float64),
                                    float(records[i, 0]), st.quotient32(cells.r[i, 2], records[i, 0]))
            if nan_case[i]:
                zero[:3] = False
            assert (records[i, 1:][zero] == 0).all(), (solver, cells.names[i])


@pytest.mark.gpu
@pytest.mark.parametrize("tier", TIERS)
def test_several_lanes_kernels_leave_the_one_lane_kernels_positions(world, tier):
    """The kernel bodies that may not record: the functors' twins without stores, one declared YA_STATELESS, one
    step with dt = 0.05 from the cases' state -- Tile_solver with the solver's choice, 16 and 64 lanes per cell,
    Grid_solver's grid_force_coop with its choice, 4, 8 and 16 -- bit for bit the one-lane kernels' positions."""
    assert world[2][tier]["lanes_differ"] == 0


@pytest.mark.gpu
def test_the_exact_tier_hands_over_the_correctly_rounded_dist(world):
    cells, host, runs = world
    records = runs["exact"]["records"]
    for solver, mine in zip(SOLVERS, records):
        assert np.array_equal(mine[:, 0].view(np.uint32), host[0, :, 0].view(np.uint32)), solver
        assert np.array_equal(mine.view(np.uint32), records[0].view(np.uint32)), solver  # dist and forces alike
    axis, offset, of = runs["exact"]["undershoot"]
    assert (axis, offset, of) == (0, 0, 12 << 23)


@pytest.mark.gpu
def test_the_fast_tier_hands_over_a_dist_within_two_ulp(world):
    """|dist - float64 distance| <= 2 ulp: the fused sum is good to 1.5 * 2^-24 relative, the square root halves
    that, the instruction adds 1 ulp.  The undershoot counts are printed (module docstring)."""
    cells, host, runs = world
    for solver, mine in zip(SOLVERS, runs["fast"]["records"]):
        ulps = np.abs(mine[:, 0].astype(np.float64) - cells.true_dist) / np.spacing(cells.true_dist.astype(np.float32))
        print(f"fast {solver}: dist within {ulps.max():.2f} ulp")
        assert ulps.max() <= 2, solver
    # the cases do meet the hazard: tests/polarity_cases.py UNDERSHOOT_D on the axis come back one ulp short
    short = runs["fast"]["records"][0][:, 0] < np.abs(cells.r[:, 2])
    print("fast tier: cells whose dist is below |r.z|:", int(short.sum()))
    assert short.sum() >= 2 * len(polarity_cases.UNDERSHOOT_D)
    print("fast tier, ya::dist3 below z (axis, 2^-13 z beside it, of):", runs["fast"]["undershoot"])
    assert runs["fast"]["undershoot"][2] == 12 << 23


@pytest.fixture(scope="module")
def column():
    X0, types = sup.column_and_sheet()
    return X0, types, sup.column_statement(X0, types, 0.05)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", TIERS)
def test_a_column_on_the_polar_axis_steps(column, tier):
    """End to end: passive_growth_grid (relu_w_epithelium, 0.15 bending_force), all epithelium, 48 cells exactly on
    the z axis -- every neighbour pair an axis pair -- and a 6 x 6 sheet; one step with dt = 0.05.  Finite,
    inside tests/test_model_functors_independent.py's bounds widened by the conditioning term pushed through the
    statement's Heun step, neighbour counters exact.  (The oracle: tests/test_polarity_pairs.py.)"""
    from yalla_amd import _ffi
    X0, types, statement = column
    sup.check_column(_ffi.device_lib() if tier == "exact" else _ffi.device_lib("fast"), statement, X0, types)
