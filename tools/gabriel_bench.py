#!/usr/bin/env python3
"""Gabriel_solver timing: relu_gabriel per take_step with ya::gabriel_force (force_variant -1) and the kept
baseline gabriel_force_direct (force_variant 0) ALTERNATED on one evolving system in one process, after a
warm-up; the same system's relu_grid step for context; the candidates per cell (cells within the cut-off,
the cell itself included).  Run it under a time limit, e.g.
    timeout -k 10 900 python3 tools/gabriel_bench.py --out profiles/gabriel_bench.json
and the kernel times with a separate
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/gabriel_bench.py --rounds 2 ...
Systems: random_sphere(0.75) of 10^4 and 10^5 cells (as growth_w_wall starts) and the headline springs state,
random_sphere(0.5, seed 42) of 10^6 cells.  The baseline is skipped where a cell has 100 candidates or more
(its fixed list would overflow)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yalla_amd.solution import Solution  # noqa: E402

SYSTEMS = [("sphere0.75_1e4", 10_000, 0.75, 1), ("sphere0.75_1e5", 100_000, 0.75, 1),
           ("springs_headline_1e6", 1_000_000, 0.5, 42)]


def candidate_counts(X):
    from scipy.spatial import cKDTree
    return cKDTree(X.astype(np.float64)).query_ball_point(X.astype(np.float64), 1.0, return_length=True)


def timed(s, dt, steps):
    s.synchronize()
    t = time.perf_counter()
    s.take_step(dt, steps)
    s.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternations new / baseline")
    ap.add_argument("--steps", type=int, default=5, help="take_steps per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated system names")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dt = 0.01
    results = []
    for name, n, dist, seed in SYSTEMS:
        if args.only and name not in args.only.split(","):
            continue
        r_max = dist * (n / 0.64) ** (1 / 3) / 2
        gs = 2 * math.ceil(r_max + 3)
        with Solution("relu_gabriel", n, gs, 1.0) as s:
            s.random_sphere(dist, seed)
            X0 = s.positions()[:n].copy()
            counts = candidate_counts(X0)
            rec = {"system": name, "cells": n, "grid_size": gs, "candidates_max": int(counts.max()),
                   "candidates_mean": round(float(counts.mean()), 2)}
            variants = (-1, 0) if counts.max() < 100 else (-1,)
            s.take_step(dt, args.warmup)
            for v in variants:
                s.set_param("force_variant", v)
                s.take_step(dt, 1)
            times = {v: [] for v in variants}
            for _ in range(args.rounds):
                for v in variants:
                    s.set_param("force_variant", v)
                    times[v].append(timed(s, dt, args.steps))
            rec["gabriel_step_ms"] = round(float(np.median(times[-1])), 4)
            if 0 in times:
                rec["baseline_step_ms"] = round(float(np.median(times[0])), 4)
                rec["step_speedup"] = round(rec["baseline_step_ms"] / rec["gabriel_step_ms"], 2)
        with Solution("relu_grid", n, gs, 1.0) as g:
            g.h_X[:n] = X0
            g.h_n = n
            g.copy_to_device()
            g.take_step(dt, args.warmup)
            rec["relu_grid_step_ms"] = round(float(np.median([timed(g, dt, args.steps) for _ in range(args.rounds)])), 4)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
