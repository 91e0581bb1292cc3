#!/usr/bin/env python3
"""M small systems per step: M single Solutions stepped one after the other against one Ensemble.

    python tools/ensemble_bench.py [--out profiles/ensemble_bench.json] [--window 0.3] [--repeats 3]
    python tools/ensemble_bench.py --trace-shape 64 800 --steps 50     # what a rocprofv3 run wraps
    python tools/ensemble_bench.py --solver grid [--out profiles/ensemble_grid_bench.json]
    python tools/ensemble_bench.py --solver grid --trace-shape 64 2000 --steps 50
    python tools/ensemble_bench.py --solver gabriel [--out profiles/ensemble_gabriel_bench.json]
    python tools/ensemble_bench.py --whole-steps [--out profiles/ensemble_whole_step_bench.json]
    python tools/ensemble_bench.py --whole-steps --whole-step-lanes 0,1,4,16,64 [--out profiles/ensemble_whole_lanes_bench.json]
    python tools/ensemble_bench.py --solver grid --lds-steps [--out profiles/ensemble_grid_lds_steps_bench.json]
    python tools/ensemble_bench.py --solver grid --lds-steps --lds-step-lanes 0,1,4,16,64 [--out profiles/ensemble_grid_lds_lanes_bench.json]
    python tools/ensemble_bench.py --solver gabriel --lds-steps [--out profiles/ensemble_gabriel_lds_steps_bench.json]
    python tools/ensemble_bench.py --links [--out profiles/ensemble_links_bench.json]
    python tools/ensemble_bench.py --solver grid --links [--out profiles/ensemble_grid_links_bench.json]
    python tools/ensemble_bench.py --replica-dt [--baseline-libs DIR --baseline-commit HASH] [--out profiles/ensemble_replica_dt_bench.json]

In ONE process, after a warm-up of every shape, the two ways alternate (A, B with each lanes setting, A, B ...):
  A  M Solution("relu_tile", n) objects, one take_step each, round-robin -- how a sweep over M systems runs
     without the ensemble (each step begins with its blocking 4-byte read of n and queues six launches);
  B  one Ensemble("relu", M, n): six launches per step for all replicas, nothing read by the host;
     with tile_lanes 0 (the engine's choice, ya::ens::lanes_for), 1, 16 and 64.
A timed window is K steps between two synchronisations under a host clock, K calibrated so that a window lasts
at least --window seconds; --repeats windows per setting, the median reported with the spread
(max - min) / median.  Cells are a seeded random ball per replica (all-pairs cost does not depend on positions).
The figure is cell-updates per second: M * n * K / seconds.

--solver grid: the same protocol for Grid_solver systems -- Solution("relu_grid", n, grid_size) round-robin (below
YA_GRAPH_MAX_CELLS each of them replays a captured graph of its step) against one GridEnsemble("relu", M, n,
grid_size) with lanes 0 (ya::ens::grid_lanes_for), 1, 4, 8, 16; M in {1, 8, 64, 512} x n in {500, 2000, 10^4,
5 * 10^4} with M * n <= 5 * 10^6; grid_size fitted to the ball (the ensemble scans M * grid_size^3 counters per
stage).  The row's spread is that of the worse side.

--solver gabriel: the same protocol for Gabriel_solver systems -- Solution("relu_gabriel", n, grid_size) round-robin
(each stage of each step waits for the dense-cell count, 2 M blocking reads per step) against one
GabrielEnsemble("relu", M, n, grid_size) (16 launches and 2 memsets per step, nothing read by the host; there is no
lanes setting, so the one column is lanes 0); M in {1, 8, 64, 512} x n in {100, 500, 2000, 10^4} with
M * n <= 5 * 10^6; grid_size fitted to the ball.

--whole-steps: ONE Ensemble("relu", M, n) per shape, the same protocol, three settings alternating: the six-launch
step (whole_steps -1, the baseline), whole-step launches of one step each (whole_steps 1, steps_per_launch 1: no
launches between the stages) and of up to 256 steps each (steps_per_launch at its default: none between the steps
either).  M in {1, 16, 64, 256, 1024, 4096} x n in {32, 100, 256, 512, 1024} with M * n^2 <= 2^28, so that a window
stays short.  ratio_* = the setting's rate over the baseline's.

--whole-steps --whole-step-lanes 0,1,4,16,64: ONE Ensemble("relu", M, n) per shape with whole_steps 1 (up to 256 steps
per launch), the same protocol, the listed whole_step_lanes settings alternating; lanes 1 (one thread per cell, the
reference column) is always among them.  n in {4, 16, 32, 64, 100, 256, 1024} x the same M range, M * n^2 <= 2^28.
ratio_lanes_L = the rate with L lanes per cell over the rate with 1.

--solver grid --lds-steps --lds-step-lanes 0,1,4,16,64: ONE GridEnsemble("relu", M, n, grid_size fitted to the ball)
per shape with lds_steps 1 (up to 256 steps per launch), the protocol of --whole-step-lanes, the listed lds_step_lanes
settings alternating with each other and with the 14-launch step of the same object (lds_steps -1); lanes 1 is always
among them.  n in {4, 16, 32, 64, 100, 256, 1024} x M in {1, 16, 64, 256, 1024, 4096}.  ratio_* = the setting's rate
over the rate with one lane per cell; each lanes column records lds_step_lanes_used.

--links: ONE LinkedEnsemble("relu_links", M, n, S = n) per shape (every cell holds one link to a random other cell of
its replica), the same protocol, four settings alternating: link_forces with global atomics as a generic force of
the six-launch step (links_path 1, whole_steps -1: a memset and the atomics kernel per stage -- the way before the
ordered forces, the baseline), the ordered forces on the six-launch step (link_forces_ordered), and the ordered
forces inside whole-step launches of one step each (a model that renews its links every step) and of up to 256 steps
each.  M in {1, 16, 64, 256, 1024, 4096} x n in {32, 100, 256, 1024} with M * n^2 <= 2^28.  ratio_* = the setting's
rate over the baseline's.

--solver grid --links: ONE LinkedGridEnsemble("relu_links", M, n, S = 2 n, grid_size fitted to the ball) per shape
(every cell holds two links to random other cells of its replica), under the protocol of --lds-steps, three settings
alternating: the ordered forces on the 14-launch step (lds_steps -1: link_forces_ordered and a memset per stage, the
baseline) and inside launches that step from LDS of one step each (lds_steps 1, lds_steps_max 1: a model that renews
its links every step) and of up to 256 steps each.  M in {16, 256, 1024, 4096} x n in {100, 256, 512, 1024}.
ratio_* = the setting's rate over the baseline's.  A record, not a gate.

--solver gabriel --lds-steps: ONE GabrielLdsEnsemble("relu", M, n, grid_size fitted to the ball) per shape under the
protocol of --lds-steps, two settings alternating: the 16-launch step (lds_steps -1, the baseline) and launches that
step from LDS of up to 256 steps each (lds_steps 1).  M in {1, 16, 64, 256, 1024, 4096} x n in {20, 64, 100, 256,
1024} (`--shapes M:n,...` for others; `--steps-per-launch 1` adds launches of ONE step each as a third setting:
what a caller of take_steps(dt, 1) pays), then the balls ensemble of the tests (48 replicas of K + 1 <= 258 cells, K candidates per cell: the dense path
inside the launch from K = 65 on; its rates count n_max rows per replica).  Each setting's spread is recorded.

--replica-dt: what a time step per replica costs the scalar call.  Per shape ONE SweepEnsemble("relu") timed twice,
with a scalar dt and with an array of M equal values (ya::ens::Replica_dt), alternating with the existing class of the
same shape and settings (Ensemble / GabrielEnsemble, this tree's libraries) and -- with --baseline-libs DIR, a directory
that holds libyalla_ensemble.so and libyalla_ensemble_gabriel.so built from another commit (--baseline-commit HASH says
which, for the record) -- with that class on those libraries, all in one process under the protocol above.  The shapes: all-pairs M = 64, n = 800, six launches; all-pairs
M = 256, n = 64, whole steps with the engine's lanes; Gabriel M = 64, n = 256, 16 launches.  Each setting's rate and
spread are recorded; `agrees` says whether the sweep object's scalar rate and the baseline's (the existing class
where there is no DIR) differ by at most the larger of their two spreads.  A figure that was not taken is "not measured".
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yalla_amd import _ffi  # noqa: E402
from yalla_amd.ensemble import (Ensemble, GabrielEnsemble, GabrielLdsEnsemble, GridEnsemble, LinkedEnsemble,  # noqa: E402
                                LinkedGridEnsemble, SweepEnsemble)
from yalla_amd.solution import Solution  # noqa: E402

SHAPES = [(m, n) for n in (100, 800, 2000) for m in (1, 8, 64, 256)] + [(1024, 100)]
LANES = (0, 1, 16, 64)
GRID_SHAPES = [(m, n) for n in (500, 2000, 10000, 50000) for m in (1, 8, 64, 512) if m * n <= 5000000]
GRID_LANES = (0, 1, 4, 8, 16)
WHOLE_SHAPES = [(m, n) for n in (32, 100, 256, 512, 1024) for m in (1, 16, 64, 256, 1024, 4096) if m * n * n <= 2 ** 28]
WHOLE_SETTINGS = {"six_launches": (-1, 256), "whole_1_step_per_launch": (1, 1), "whole_256_steps_per_launch": (1, 256)}
# --solver grid --lds-steps: one GridEnsemble("relu", M, n), (lds_steps, lds_steps_max)
LDS_SHAPES = [(m, n) for n in (32, 100, 256, 512, 1024) for m in (1, 16, 64, 256, 1024, 4096)]
LDS_SETTINGS = {"fourteen_launches": (-1, 256), "lds_1_step_per_launch": (1, 1), "lds_256_steps_per_launch": (1, 256)}
# --solver grid --lds-steps --lds-step-lanes: one GridEnsemble("relu", M, n), lds_step_lanes settings and the 14 launches
LDS_LANES_SHAPES = [(m, n) for n in (4, 16, 32, 64, 100, 256, 1024) for m in (1, 16, 64, 256, 1024, 4096)]
WHOLE_LANES_SHAPES = [(m, n) for n in (4, 16, 32, 64, 100, 256, 1024) for m in (1, 16, 64, 256, 1024, 4096)
                      if m * n * n <= 2 ** 28]
LINKS_SHAPES = [(m, n) for n in (32, 100, 256, 1024) for m in (1, 16, 64, 256, 1024, 4096) if m * n * n <= 2 ** 28]
# (links_path, whole_steps, steps_per_launch)
LINKS_SETTINGS = {"atomics_six_launches": (1, -1, 256), "ordered_six_launches": (0, -1, 256),
                  "ordered_whole_1_step_per_launch": (0, 1, 1), "ordered_whole_256_steps_per_launch": (0, 1, 256)}
# --solver grid --links: one LinkedGridEnsemble("relu_links", M, n, 2 n), (lds_steps, lds_steps_max)
GRID_LINKS_SHAPES = [(m, n) for n in (100, 256, 512, 1024) for m in (16, 256, 1024, 4096)]
GRID_LINKS_SETTINGS = {"ordered_fourteen_launches": (-1, 256), "ordered_lds_1_step_per_launch": (1, 1),
                       "ordered_lds_256_steps_per_launch": (1, 256)}
GABRIEL_SHAPES = [(m, n) for n in (100, 500, 2000, 10000) for m in (1, 8, 64, 512) if m * n <= 5000000]
GABRIEL_LANES = (0,)  # (no lanes setting: one column)
# --solver gabriel --lds-steps: one GabrielLdsEnsemble("relu", M, n), (lds_steps, lds_steps_max); and the balls
GABRIEL_LDS_SHAPES = [(m, n) for n in (20, 64, 100, 256, 1024) for m in (1, 16, 64, 256, 1024, 4096)]
GABRIEL_LDS_SETTINGS = {"sixteen_launches": (-1, 256), "lds_256_steps_per_launch": (1, 256)}
# --steps-per-launch 1 adds launches of one step each (a caller of take_steps(dt, 1))
GABRIEL_LDS_ONE_STEP = {"lds_1_step_per_launch": (1, 1)}
BALL_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257]
GABRIEL_LDS = False  # --solver gabriel --lds-steps
DT = 0.01
GRID = False  # --solver grid
GABRIEL = False  # --solver gabriel


def grid_size_for(n):
    """The ball's diameter at the density of random_sphere(0.75), half as much again for relu's expansion, even."""
    radius = 0.75 * (n / 0.64) ** (1 / 3) / 2
    return 2 * int(np.ceil(1.5 * radius)) + 4


def ball(n, seed):
    rng = np.random.default_rng(seed)
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    radius = 0.75 * (n / 0.64) ** (1 / 3) / 2 * rng.random(n) ** (1 / 3)
    return (direction * radius[:, None]).astype(np.float32)


class Singles:
    def __init__(self, m, n):
        self.sims = [Solution("relu_gabriel", n, grid_size_for(n), 1.0) if GABRIEL
                     else Solution("relu_grid", n, grid_size_for(n), 1.0) if GRID else Solution("relu_tile", n)
                     for _ in range(m)]
        for r, s in enumerate(self.sims):
            s.h_X[:] = ball(n, r)
            s.copy_to_device()

    def steps(self, k):
        for _ in range(k):
            for s in self.sims:
                s.take_step(DT, 1)
        self.sims[0].synchronize()

    def close(self):
        for s in self.sims:
            s.close()


class Together:
    def __init__(self, m, n):
        self.ens = (GabrielLdsEnsemble("relu", m, n, grid_size_for(n), 1.0) if GABRIEL_LDS
                    else GabrielEnsemble("relu", m, n, grid_size_for(n), 1.0) if GABRIEL
                    else GridEnsemble("relu", m, n, grid_size_for(n), 1.0) if GRID else Ensemble("relu", m, n))
        for r in range(m):
            self.ens.h_X[r] = ball(n, r)
        self.ens.copy_to_device()

    def lanes(self, lanes):
        if GABRIEL:
            return
        self.ens.set_param("lanes" if GRID else "tile_lanes", lanes)

    def whole(self, whole_steps, steps_per_launch):
        self.ens.set_param("whole_steps", whole_steps)
        self.ens.set_param("steps_per_launch", steps_per_launch)

    def lds(self, lds_steps, lds_steps_max):
        self.ens.set_param("lds_steps", lds_steps)
        self.ens.set_param("lds_steps_max", lds_steps_max)

    def whole_lanes(self, lanes):
        self.ens.set_param("whole_step_lanes", lanes)

    def steps(self, k):
        self.ens.take_step(DT, k)
        self.ens.synchronize()

    def close(self):
        self.ens.close()


class Balls(Together):
    """One GabrielLdsEnsemble("relu", 48, 258, 16): for each K of BALL_SIZES two replicas of K cells inside a ball of
    radius 0.45 (K candidates per cell, the dense path from 65 on) and a lone cell, the shape of the tests' balls."""

    def __init__(self, m=48, n=258):
        self.ens = GabrielLdsEnsemble("relu", m, n, 16, 1.0)
        rng = np.random.default_rng(164)
        self.cells = 0
        for r, k in enumerate(k for k in BALL_SIZES for _ in (0, 1)):
            v = rng.standard_normal((k, 3))
            v *= (0.45 * rng.random(k) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
            self.ens.h_X[r, 0] = 3.5
            self.ens.h_X[r, 1:k + 1] = (0.5 * (r % 2) + v).astype(np.float32)
            self.ens.h_n[r] = k + 1
            self.cells += k + 1
        self.ens.copy_to_device()


class Linked:
    """One LinkedEnsemble("relu_links", m, n, n): cell i of every replica linked to a random other cell of it."""

    def __init__(self, m, n):
        self.ens = LinkedEnsemble("relu_links", m, n, n)
        rng = np.random.default_rng(m * 10007 + n)
        for r in range(m):
            self.ens.h_X[r] = ball(n, r)
        a = np.broadcast_to(np.arange(n), (m, n))
        b = (a + 1 + rng.integers(0, n - 1, (m, n))) % n
        self.ens.h_link[:] = np.stack([a, b], axis=2) + (np.arange(m) * n)[:, None, None]
        self.ens.n_links = m * n
        self.ens.copy_to_device()

    def setting(self, links_path, whole_steps, steps_per_launch):
        self.ens.set_param("links_path", links_path)
        self.ens.set_param("whole_steps", whole_steps)
        self.ens.set_param("steps_per_launch", steps_per_launch)

    def steps(self, k):
        self.ens.take_step(DT, k)
        self.ens.synchronize()

    def close(self):
        self.ens.close()


class LinkedGrid:
    """One LinkedGridEnsemble("relu_links", m, n, 2 n, grid_size fitted): cell i of every replica linked to two random
    other cells of it."""

    def __init__(self, m, n):
        self.ens = LinkedGridEnsemble("relu_links", m, n, 2 * n, grid_size=grid_size_for(n))
        rng = np.random.default_rng(m * 10007 + n)
        for r in range(m):
            self.ens.h_X[r] = ball(n, r)
        a = np.broadcast_to(np.repeat(np.arange(n), 2), (m, 2 * n))
        b = (a + 1 + rng.integers(0, n - 1, (m, 2 * n))) % n
        self.ens.h_link[:] = np.stack([a, b], axis=2) + (np.arange(m) * n)[:, None, None]
        self.ens.n_links = m * 2 * n
        self.ens.copy_to_device()

    def setting(self, lds_steps, lds_steps_max):
        self.ens.set_param("lds_steps", lds_steps)
        self.ens.set_param("lds_steps_max", lds_steps_max)

    def steps(self, k):
        self.ens.take_step(DT, k)
        self.ens.synchronize()

    def close(self):
        self.ens.close()


# --replica-dt: (name, form, M, n, the sweep object's settings, the existing class's)
REPLICA_DT_CASES = [
    ("all_pairs_six_launches", "tile", 64, 800, {"whole_steps": -1}, {"whole_steps": -1}),
    ("all_pairs_whole_steps", "tile", 256, 64, {"whole_steps": 1, "whole_step_lanes": 0},
     {"whole_steps": 1, "whole_step_lanes": 0}),
    ("gabriel_sixteen_launches", "gabriel", 64, 256, {"lds_steps": -1}, {}),
]


class Sweep:
    """One SweepEnsemble("relu") of the shape; array: stepped with M equal values of DT instead of the scalar."""

    def __init__(self, form, m, n, params):
        self.ens = SweepEnsemble(form, "relu", m, n, grid_size=grid_size_for(n))
        for name, value in params.items():
            self.ens.set_param(name, value)
        for r in range(m):
            self.ens.h_X[r] = ball(n, r)
        self.ens.copy_to_device()

    def setting(self, array):
        self.ens.dt = np.full(self.ens.n_replicas, DT, np.float32) if array else None

    def steps(self, k):
        self.ens.take_step(DT, k)
        self.ens.synchronize()

    def close(self):
        self.ens.close()


class Existing(Sweep):
    """The existing class of the form, on this tree's library or on the one in `libs` (another commit's build)."""

    def __init__(self, form, m, n, params, libs=None):
        name, table = (("libyalla_ensemble.so", _ffi.ENSEMBLE_ABI) if form == "tile"
                       else ("libyalla_ensemble_gabriel.so", _ffi.GABRIEL_ENSEMBLE_ABI))
        lib = _ffi._load(os.path.join(os.path.abspath(libs), name), table) if libs else None
        self.ens = Ensemble("relu", m, n, lib=lib) if form == "tile" else GabrielEnsemble(
            "relu", m, n, grid_size_for(n), 1.0, lib=lib)
        for name, value in params.items():
            self.ens.set_param(name, value)
        for r in range(m):
            self.ens.h_X[r] = ball(n, r)
        self.ens.copy_to_device()

    def setting(self, array):
        pass


def measure_replica_dt(case, window, repeats, libs):
    name, form, m, n, params, existing_params = case
    sweep = Sweep(form, m, n, params)
    runs = {"sweep_scalar_dt": (sweep, False), "sweep_array_of_equal_dt": (sweep, True),
            "existing_class": (Existing(form, m, n, existing_params), False)}
    if libs:
        runs["baseline_libs_existing_class"] = (Existing(form, m, n, existing_params, libs), False)
    try:
        ks = {}
        for key, (run, array) in runs.items():
            run.setting(array)
            run.steps(5)
            ks[key] = calibrate(run, window)
        samples = {key: [] for key in runs}
        for _ in range(repeats):  # scalar, array, existing[, baseline], scalar, ...
            for key, (run, array) in runs.items():
                run.setting(array)
                samples[key].append(timed(run, ks[key]))
        launches = sweep.ens.lds_launches
    finally:
        for run in {id(run): run for run, _ in runs.values()}.values():
            run.close()
    row = {"shape": name, "form": form, "n_replicas": m, "n": n, "launches_from_lds": launches}
    for key in runs:
        row[key] = summary(samples[key], m * n, ks[key])
    baseline = "baseline_libs_existing_class" if libs else "existing_class"
    if not libs:
        row["baseline_libs_existing_class"] = "not measured"
    mine, theirs = row["sweep_scalar_dt"], row[baseline]
    row["compared_with"] = baseline
    row["ratio_scalar_over_baseline"] = mine["cell_updates_per_s"] / theirs["cell_updates_per_s"]
    row["ratio_array_over_scalar"] = row["sweep_array_of_equal_dt"]["cell_updates_per_s"] / mine["cell_updates_per_s"]
    row["larger_spread"] = max(mine["spread"], theirs["spread"])
    row["agrees"] = abs(mine["cell_updates_per_s"] - theirs["cell_updates_per_s"]) <= row["larger_spread"] * max(
        mine["cell_updates_per_s"], theirs["cell_updates_per_s"])
    return row


def main_replica_dt(args):
    rows = []
    for case in REPLICA_DT_CASES:
        rows.append(measure_replica_dt(case, args.window, args.repeats, args.baseline_libs))
        r = rows[-1]
        keys = [key for key in r if isinstance(r[key], dict)]
        print(f"{r['shape']:26s} M {r['n_replicas']:4d}  n {r['n']:4d}   "
              + "  ".join(f"{key}: {r[key]['us_per_step']:8.2f} us/step ({r[key]['spread']:.3f})" for key in keys)
              + f"   scalar / {r['compared_with']} {r['ratio_scalar_over_baseline']:.3f}  agrees {r['agrees']}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py --replica-dt", "model": "relu", "dt": DT, "window_s": args.window,
                      "repeats": args.repeats,
                      "baseline_commit": (args.baseline_commit or "not recorded") if args.baseline_libs else "not measured",
                      "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows), "agree": [r["agrees"] for r in rows],
                      "ratio_scalar_over_baseline": [round(r["ratio_scalar_over_baseline"], 4) for r in rows]}))


def timed(run, k):
    t0 = time.perf_counter()
    run.steps(k)
    return time.perf_counter() - t0


def calibrate(run, window):
    k = 4
    while True:
        t = timed(run, k)
        if t >= window:
            return k
        k = max(k + 1, int(k * min(8.0, 1.25 * window / max(t, 1e-6))))


def summary(samples, cells_per_step, k):
    rates = sorted(cells_per_step * k / t for t in samples)
    median = rates[len(rates) // 2]
    return {"steps_per_window": k, "seconds": [round(t, 6) for t in samples],
            "cell_updates_per_s": median, "spread": (rates[-1] - rates[0]) / median,
            "us_per_step": 1e6 * sorted(samples)[len(samples) // 2] / k}


def measure(m, n, window, repeats):
    a, b = Singles(m, n), Together(m, n)
    try:
        a.steps(3)
        ks = {"A": calibrate(a, window)}
        for lanes in LANES:
            b.lanes(lanes)
            b.steps(3)
            ks[lanes] = calibrate(b, window)
        samples = {key: [] for key in ks}
        for _ in range(repeats):  # A, B0, B1, B16, B64, A, ...
            samples["A"].append(timed(a, ks["A"]))
            for lanes in LANES:
                b.lanes(lanes)
                samples[lanes].append(timed(b, ks[lanes]))
    finally:
        a.close()
        b.close()
    row = {"n_replicas": m, "n": n, "singles": summary(samples["A"], m * n, ks["A"])}
    if GRID or GABRIEL:
        row["grid_size"] = grid_size_for(n)
    for lanes in LANES:
        row[f"ensemble_lanes_{lanes}"] = summary(samples[lanes], m * n, ks[lanes])
    for lanes in LANES:
        row[f"ratio_lanes_{lanes}"] = row[f"ensemble_lanes_{lanes}"]["cell_updates_per_s"] / row["singles"]["cell_updates_per_s"]
    row["ratio"] = row["ratio_lanes_0"]  # the engine's choice against the sequential loop
    row["spread"] = max(row["singles"]["spread"], row["ensemble_lanes_0"]["spread"])  # of the worse side
    return row


def measure_whole(m, n, window, repeats, settings=None, apply=Together.whole, counter="whole_step_launches",
                  make=Together):
    """One ensemble, every setting of `settings` (the first is the baseline of the ratios) alternated."""
    settings = WHOLE_SETTINGS if settings is None else settings
    b = make(m, n)
    try:
        ks = {}
        for key, setting in settings.items():
            apply(b, *setting)
            b.steps(3)
            ks[key] = calibrate(b, window)
        samples = {key: [] for key in ks}
        for _ in range(repeats):  # six, whole 1, whole 256, six, ...
            for key, setting in settings.items():
                apply(b, *setting)
                samples[key].append(timed(b, ks[key]))
        launches = getattr(b.ens, counter)
    finally:
        b.close()
    row = {"n_replicas": m, "n": n, counter: launches}
    if GRID:
        row["grid_size"] = grid_size_for(n)
    for key in settings:
        row[key] = summary(samples[key], m * n, ks[key])
    baseline = list(settings)[0]
    for key in list(settings)[1:]:
        row["ratio_" + key] = row[key]["cell_updates_per_s"] / row[baseline]["cell_updates_per_s"]
    row["spread"] = max(row[key]["spread"] for key in settings)  # of the worst side
    return row


def main_lds(args):
    """--solver grid --lds-steps: launches that step from LDS against the 14-launch step of the same GridEnsemble."""
    shapes = LDS_SHAPES if not args.shapes else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    for m, n in shapes:  # the warm-up of every shape and setting
        run = Together(m, n)
        for setting in LDS_SETTINGS.values():
            run.lds(*setting)
            run.steps(5)
        run.close()
    rows = []
    for m, n in shapes:
        rows.append(measure_whole(m, n, args.window, args.repeats, LDS_SETTINGS, Together.lds, "lds_step_launches"))
        r = rows[-1]
        print(f"M {m:5d}  n {n:5d}   " + "  ".join(f"{key}: {r[key]['us_per_step']:10.1f} us/step" for key in LDS_SETTINGS)
              + f"   ratios {r['ratio_lds_1_step_per_launch']:.2f} {r['ratio_lds_256_steps_per_launch']:.2f}"
              + f"  spread {r['spread']:.3f}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py --solver grid --lds-steps", "model": "relu", "dt": DT,
                      "window_s": args.window, "repeats": args.repeats, "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows), "min_ratio": min(r["ratio_lds_256_steps_per_launch"] for r in rows),
                      "max_ratio": max(r["ratio_lds_256_steps_per_launch"] for r in rows)}))


def main_gabriel_lds(args):
    """--solver gabriel --lds-steps: launches that step from LDS (lds_steps 1) against the 16-launch step (lds_steps -1)
    of the same GabrielLdsEnsemble, alternating; after the sweep the balls ensemble (48 replicas, the dense path)."""
    shapes = GABRIEL_LDS_SHAPES if not args.shapes else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    cases = [(m, n, Together) for m, n in shapes] + ([] if args.shapes else [(48, 258, Balls)])
    settings = dict(GABRIEL_LDS_SETTINGS, **(GABRIEL_LDS_ONE_STEP if args.steps_per_launch == 1 else {}))
    for m, n, make in cases:  # the warm-up of every shape and setting
        run = make(m, n)
        for setting in settings.values():
            run.lds(*setting)
            run.steps(5)
        run.close()
    rows = []
    for m, n, make in cases:
        rows.append(measure_whole(m, n, args.window, args.repeats, settings, Together.lds,
                                  "lds_step_launches", make))
        r = rows[-1]
        r["input"] = "balls" if make is Balls else "ball of n cells at random_sphere(0.75)'s density"
        print(f"M {m:5d}  n {n:5d}   "
              + "  ".join(f"{key}: {r[key]['us_per_step']:10.1f} us/step" for key in settings)
              + "   ratios " + " ".join(f"{r['ratio_' + key]:.2f}" for key in list(settings)[1:]) + "  spreads "
              + " ".join(f"{r[key]['spread']:.3f}" for key in settings) + f"  {r['input'][:5]}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py --solver gabriel --lds-steps", "model": "relu", "dt": DT,
                      "window_s": args.window, "repeats": args.repeats, "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows), "min_ratio": min(r["ratio_lds_256_steps_per_launch"] for r in rows),
                      "max_ratio": max(r["ratio_lds_256_steps_per_launch"] for r in rows)}))


def main_whole(args):
    shapes = WHOLE_SHAPES if not args.shapes else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    for m, n in shapes:  # the warm-up of every shape and setting: code objects loaded, allocator and clocks settled
        run = Together(m, n)
        for setting in WHOLE_SETTINGS.values():
            run.whole(*setting)
            run.steps(5)
        run.close()
    rows = []
    for m, n in shapes:
        rows.append(measure_whole(m, n, args.window, args.repeats))
        r = rows[-1]
        print(f"M {m:5d}  n {n:5d}   " + "  ".join(f"{key}: {r[key]['us_per_step']:10.1f} us/step" for key in WHOLE_SETTINGS)
              + f"   ratios {r['ratio_whole_1_step_per_launch']:.2f} {r['ratio_whole_256_steps_per_launch']:.2f}"
              + f"  spread {r['spread']:.3f}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py --whole-steps", "model": "relu", "dt": DT,
                      "window_s": args.window, "repeats": args.repeats, "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows), "min_ratio": min(r["ratio_whole_256_steps_per_launch"] for r in rows),
                      "max_ratio": max(r["ratio_whole_256_steps_per_launch"] for r in rows)}))


def measure_links(m, n, window, repeats):
    b = Linked(m, n)
    try:
        ks = {}
        for key, setting in LINKS_SETTINGS.items():
            b.setting(*setting)
            b.steps(3)
            ks[key] = calibrate(b, window)
        samples = {key: [] for key in ks}
        for _ in range(repeats):  # atomics, ordered six, whole 1, whole 256, atomics, ...
            for key, setting in LINKS_SETTINGS.items():
                b.setting(*setting)
                samples[key].append(timed(b, ks[key]))
        launches = b.ens.whole_step_launches
    finally:
        b.close()
    row = {"n_replicas": m, "n": n, "slots_per_replica": n, "whole_step_launches": launches}
    for key in LINKS_SETTINGS:
        row[key] = summary(samples[key], m * n, ks[key])
    for key in list(LINKS_SETTINGS)[1:]:
        row["ratio_" + key] = row[key]["cell_updates_per_s"] / row["atomics_six_launches"]["cell_updates_per_s"]
    row["spread"] = max(row[key]["spread"] for key in LINKS_SETTINGS)  # of the worst side
    return row


def main_links(args):
    shapes = LINKS_SHAPES if not args.shapes else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    for m, n in shapes:  # the warm-up of every shape and setting
        run = Linked(m, n)
        for setting in LINKS_SETTINGS.values():
            run.setting(*setting)
            run.steps(5)
        run.close()
    rows = []
    for m, n in shapes:
        rows.append(measure_links(m, n, args.window, args.repeats))
        r = rows[-1]
        print(f"M {m:5d}  n {n:5d}   " + "  ".join(f"{key}: {r[key]['us_per_step']:9.1f}" for key in LINKS_SETTINGS)
              + " us/step   ratios " + " ".join(f"{r['ratio_' + key]:.2f}" for key in list(LINKS_SETTINGS)[1:])
              + f"  spread {r['spread']:.3f}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py --links", "model": "relu_links", "dt": DT,
                      "window_s": args.window, "repeats": args.repeats, "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows),
                      "min_ratio_whole_1": min(r["ratio_ordered_whole_1_step_per_launch"] for r in rows),
                      "max_ratio_whole_1": max(r["ratio_ordered_whole_1_step_per_launch"] for r in rows),
                      "min_ratio_whole_256": min(r["ratio_ordered_whole_256_steps_per_launch"] for r in rows),
                      "max_ratio_whole_256": max(r["ratio_ordered_whole_256_steps_per_launch"] for r in rows)}))


def measure_grid_links(m, n, window, repeats):
    b = LinkedGrid(m, n)
    try:
        ks = {}
        for key, setting in GRID_LINKS_SETTINGS.items():
            b.setting(*setting)
            b.steps(3)
            ks[key] = calibrate(b, window)
        samples = {key: [] for key in ks}
        for _ in range(repeats):  # fourteen, lds 1, lds 256, fourteen, ...
            for key, setting in GRID_LINKS_SETTINGS.items():
                b.setting(*setting)
                samples[key].append(timed(b, ks[key]))
        launches = b.ens.lds_step_launches
    finally:
        b.close()
    row = {"n_replicas": m, "n": n, "slots_per_replica": 2 * n, "grid_size": grid_size_for(n), "lds_step_launches": launches}
    for key in GRID_LINKS_SETTINGS:
        row[key] = summary(samples[key], m * n, ks[key])
    baseline = list(GRID_LINKS_SETTINGS)[0]
    for key in list(GRID_LINKS_SETTINGS)[1:]:
        row["ratio_" + key] = row[key]["cell_updates_per_s"] / row[baseline]["cell_updates_per_s"]
    row["spread"] = max(row[key]["spread"] for key in GRID_LINKS_SETTINGS)  # of the worst side
    return row


def main_grid_links(args):
    """--solver grid --links: linked launches that step from LDS against the 14-launch step of the same ensemble."""
    shapes = GRID_LINKS_SHAPES if not args.shapes else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    for m, n in shapes:  # the warm-up of every shape and setting
        run = LinkedGrid(m, n)
        for setting in GRID_LINKS_SETTINGS.values():
            run.setting(*setting)
            run.steps(5)
        run.close()
    rows = []
    for m, n in shapes:
        rows.append(measure_grid_links(m, n, args.window, args.repeats))
        r = rows[-1]
        print(f"M {m:5d}  n {n:5d}   " + "  ".join(f"{key}: {r[key]['us_per_step']:9.1f}" for key in GRID_LINKS_SETTINGS)
              + " us/step   ratios " + " ".join(f"{r['ratio_' + key]:.2f}" for key in list(GRID_LINKS_SETTINGS)[1:])
              + f"  spread {r['spread']:.3f}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py --solver grid --links", "model": "relu_links", "dt": DT,
                      "window_s": args.window, "repeats": args.repeats, "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows),
                      "min_ratio_lds_1": min(r["ratio_ordered_lds_1_step_per_launch"] for r in rows),
                      "max_ratio_lds_1": max(r["ratio_ordered_lds_1_step_per_launch"] for r in rows),
                      "min_ratio_lds_256": min(r["ratio_ordered_lds_256_steps_per_launch"] for r in rows),
                      "max_ratio_lds_256": max(r["ratio_ordered_lds_256_steps_per_launch"] for r in rows)}))


def measure_whole_lanes(m, n, lanes_list, window, repeats, steps_per_launch=256):
    b = Together(m, n)
    try:
        b.whole(1, steps_per_launch)
        ks = {}
        for lanes in lanes_list:
            b.whole_lanes(lanes)
            b.steps(3)
            ks[lanes] = calibrate(b, window)
        samples = {lanes: [] for lanes in lanes_list}
        for _ in range(repeats):  # L0, L1, L4, ..., L0, ...
            for lanes in lanes_list:
                b.whole_lanes(lanes)
                samples[lanes].append(timed(b, ks[lanes]))
        launches = b.ens.whole_step_launches
    finally:
        b.close()
    row = {"n_replicas": m, "n": n, "whole_step_launches": launches}
    for lanes in lanes_list:
        row[f"lanes_{lanes}"] = summary(samples[lanes], m * n, ks[lanes])
    for lanes in lanes_list:
        row[f"ratio_lanes_{lanes}"] = row[f"lanes_{lanes}"]["cell_updates_per_s"] / row["lanes_1"]["cell_updates_per_s"]
    row["spread"] = max(row[f"lanes_{lanes}"]["spread"] for lanes in lanes_list)  # of the worst side
    return row


def measure_lds_lanes(m, n, lanes_list, window, repeats, steps_per_launch=256):
    """One GridEnsemble: launches that step from LDS (up to 256 steps each) with every lds_step_lanes setting of
    lanes_list, and the 14-launch step of the same object, alternated."""
    b = Together(m, n)
    settings = [("lanes_%d" % lanes, 1, lanes) for lanes in lanes_list] + [("fourteen_launches", -1, 1)]

    def apply(lds_steps, lanes):
        b.lds(lds_steps, steps_per_launch)
        b.ens.set_param("lds_step_lanes", lanes)
    try:
        ks, used = {}, {}
        for key, lds_steps, lanes in settings:
            apply(lds_steps, lanes)
            b.steps(3)
            if lds_steps == 1:
                used[key] = b.ens.lds_step_lanes_used
            ks[key] = calibrate(b, window)
        samples = {key: [] for key in ks}
        for _ in range(repeats):  # L0, L1, L4, ..., the 14 launches, L0, ...
            for key, lds_steps, lanes in settings:
                apply(lds_steps, lanes)
                samples[key].append(timed(b, ks[key]))
        launches = b.ens.lds_step_launches
    finally:
        b.close()
    row = {"n_replicas": m, "n": n, "grid_size": grid_size_for(n), "lds_step_launches": launches}
    for key, _, _ in settings:
        row[key] = summary(samples[key], m * n, ks[key])
        if key in used:
            row[key]["lds_step_lanes_used"] = used[key]
    for key, _, _ in settings:
        row["ratio_" + key] = row[key]["cell_updates_per_s"] / row["lanes_1"]["cell_updates_per_s"]
    row["spread"] = max(row[key]["spread"] for key, _, _ in settings)  # of the worst side
    return row


def main_lds_lanes(args):
    """--solver grid --lds-steps --lds-step-lanes: several lanes per cell inside the launches that step from LDS against
    one lane per cell, and the 14-launch step beside them, of the same GridEnsemble."""
    lanes_list = sorted({int(v) for v in args.lds_step_lanes.split(",")} | {1})
    shapes = LDS_LANES_SHAPES if not args.shapes else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    for m, n in shapes:  # the warm-up of every shape and setting
        run = Together(m, n)
        for lanes in lanes_list:
            run.lds(1, 256)
            run.ens.set_param("lds_step_lanes", lanes)
            run.steps(5)
        run.lds(-1, 256)
        run.steps(5)
        run.close()
    rows = []
    keys = ["lanes_%d" % lanes for lanes in lanes_list] + ["fourteen_launches"]
    for m, n in shapes:
        rows.append(measure_lds_lanes(m, n, lanes_list, args.window, args.repeats, args.steps_per_launch))
        r = rows[-1]
        print(f"M {m:5d}  n {n:5d}   " + "  ".join(f"{key}: {r[key]['us_per_step']:9.2f}" for key in keys)
              + " us/step   ratios " + " ".join(f"{r['ratio_' + key]:.2f}" for key in keys)
              + f"  spread {r['spread']:.3f}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py --solver grid --lds-steps --lds-step-lanes " + args.lds_step_lanes,
                      "model": "relu", "dt": DT, "window_s": args.window, "repeats": args.repeats,
                      "ratios": "cell updates per second against lanes_1 of the same object", "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows), "min_ratio_lanes_0": min(r.get("ratio_lanes_0", 1.0) for r in rows),
                      "max_ratio_lanes_0": max(r.get("ratio_lanes_0", 1.0) for r in rows)}))


def main_whole_lanes(args):
    lanes_list = sorted({int(v) for v in args.whole_step_lanes.split(",")} | {1})
    shapes = WHOLE_LANES_SHAPES if not args.shapes else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    for m, n in shapes:  # the warm-up of every shape and setting
        run = Together(m, n)
        run.whole(1, 256)
        for lanes in lanes_list:
            run.whole_lanes(lanes)
            run.steps(5)
        run.close()
    rows = []
    for m, n in shapes:
        rows.append(measure_whole_lanes(m, n, lanes_list, args.window, args.repeats, args.steps_per_launch))
        r = rows[-1]
        print(f"M {m:5d}  n {n:5d}   " + "  ".join(f"L{lanes}: {r[f'lanes_{lanes}']['us_per_step']:9.2f}" for lanes in lanes_list)
              + " us/step   ratios " + " ".join(f"{r[f'ratio_lanes_{lanes}']:.2f}" for lanes in lanes_list)
              + f"  spread {r['spread']:.3f}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py --whole-steps --whole-step-lanes " + args.whole_step_lanes,
                      "model": "relu", "dt": DT, "window_s": args.window, "repeats": args.repeats, "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows), "min_ratio_lanes_0": min(r.get("ratio_lanes_0", 1.0) for r in rows),
                      "max_ratio_lanes_0": max(r.get("ratio_lanes_0", 1.0) for r in rows)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=None, help="M:n,M:n,... instead of the full sweep")
    ap.add_argument("--trace-shape", type=int, nargs=2, metavar=("M", "N"), default=None,
                    help="only step one Ensemble of this shape --steps times (for a kernel trace)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--steps-per-launch", type=int, default=256,
                    help="with --whole-step-lanes or --lds-step-lanes: steps_per_launch / lds_steps_max of the launches "
                         "(1: what a launch costs beside its steps)")
    ap.add_argument("--solver", choices=("tile", "grid", "gabriel"), default="tile")
    ap.add_argument("--whole-steps", action="store_true",
                    help="whole-step launches against the six-launch step of the same Ensemble (tile solver only)")
    ap.add_argument("--whole-step-lanes", default=None, metavar="L,L,...",
                    help="with --whole-steps: these whole_step_lanes settings against lanes 1 of the same Ensemble")
    ap.add_argument("--links", action="store_true",
                    help="ordered link forces (six launches, whole steps) against link_forces with atomics; with "
                         "--solver grid: ordered link forces from LDS against the 14-launch step of the same ensemble")
    ap.add_argument("--lds-steps", action="store_true",
                    help="with --solver grid (gabriel): launches that step from LDS against the 14-launch (16-launch) "
                         "step of the same ensemble")
    ap.add_argument("--lds-step-lanes", default=None, metavar="L,L,...",
                    help="with --solver grid --lds-steps: these lds_step_lanes settings against lanes 1 of the same "
                         "ensemble, the 14-launch step beside them")
    ap.add_argument("--replica-dt", action="store_true",
                    help="one SweepEnsemble with a scalar dt and with an array of equal values against the existing class")
    ap.add_argument("--baseline-libs", default=None, metavar="DIR",
                    help="with --replica-dt: libyalla_ensemble.so and libyalla_ensemble_gabriel.so of another commit's build")
    ap.add_argument("--baseline-commit", default=None, metavar="HASH", help="the commit those libraries were built from")
    args = ap.parse_args()
    if args.replica_dt:
        if args.trace_shape or args.whole_steps or args.links or args.lds_steps or args.solver != "tile":
            ap.error("--replica-dt measures its three shapes on its own")
        main_replica_dt(args)
        return
    global GRID, GABRIEL, GABRIEL_LDS, LANES, SHAPES
    if args.lds_step_lanes and not args.lds_steps:
        ap.error("--lds-step-lanes goes with --solver grid --lds-steps")
    if args.lds_steps and args.solver == "gabriel":
        if args.trace_shape or args.whole_steps or args.links or args.lds_step_lanes:
            ap.error("--solver gabriel --lds-steps measures the Gabriel ensemble on its own (it has no lanes setting)")
        GABRIEL = GABRIEL_LDS = True
        main_gabriel_lds(args)
        return
    if args.lds_steps:
        if args.solver != "grid" or args.trace_shape or args.whole_steps or args.links:
            ap.error("--lds-steps measures the grid or the Gabriel ensemble (--solver grid | gabriel) on its own")
        GRID = True
        if args.lds_step_lanes:
            if not set(args.lds_step_lanes.split(",")) <= {"0", "1", "4", "16", "64"}:
                ap.error("--lds-step-lanes takes a list out of 0,1,4,16,64")
            main_lds_lanes(args)
        else:
            main_lds(args)
        return
    if args.links:
        if args.solver == "gabriel" or args.trace_shape or args.whole_steps:
            ap.error("--links measures the linked all-pairs ensemble, or with --solver grid the linked grid ensemble, on its own")
        if args.solver == "grid":
            GRID = True
            main_grid_links(args)
        else:
            main_links(args)
        return
    if args.whole_step_lanes and not args.whole_steps:
        ap.error("--whole-step-lanes goes with --whole-steps")
    if args.whole_steps:
        if args.solver != "tile" or args.trace_shape:
            ap.error("--whole-steps measures the all-pairs ensemble, and takes no --trace-shape")
        if args.whole_step_lanes:
            if not set(args.whole_step_lanes.split(",")) <= {"0", "1", "4", "16", "64"}:
                ap.error("--whole-step-lanes takes a list out of 0,1,4,16,64")
            main_whole_lanes(args)
        else:
            main_whole(args)
        return
    if args.solver == "grid":
        GRID, LANES, SHAPES = True, GRID_LANES, GRID_SHAPES
    if args.solver == "gabriel":
        GABRIEL, LANES, SHAPES = True, GABRIEL_LANES, GABRIEL_SHAPES

    if args.trace_shape:
        b = Together(*args.trace_shape)
        b.steps(args.steps)
        b.close()
        print(json.dumps({"traced": {"n_replicas": args.trace_shape[0], "n": args.trace_shape[1], "steps": args.steps}}))
        return

    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    for m, n in shapes:  # the warm-up of every shape: code objects loaded, allocator and clocks settled
        for run in (Singles(m, n), Together(m, n)):
            run.steps(5)
            run.close()
    rows = []
    for m, n in shapes:
        rows.append(measure(m, n, args.window, args.repeats))
        r = rows[-1]
        print(f"M {m:5d}  n {n:5d}   singles {r['singles']['us_per_step']:10.1f} us/step   ensemble "
              + "  ".join(f"L{lanes}: {r[f'ensemble_lanes_{lanes}']['us_per_step']:9.1f}" for lanes in LANES)
              + f"   ratio {r['ratio']:.2f}  spread {r['spread']:.3f}", flush=True)
        if args.out:  # after every shape: a run that is cut short leaves the shapes it finished
            result = {"tool": "tools/ensemble_bench.py", "solver": args.solver, "model": "relu", "dt": DT,
                      "window_s": args.window, "repeats": args.repeats, "rows": rows}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(json.dumps({"shapes": len(rows), "min_ratio": min(r["ratio"] for r in rows)}))


if __name__ == "__main__":
    main()
