"""Ensemble<Pt, Tile_solver>::whole_step_lanes as a model program uses the header
(tests/native_ensemble_whole_lanes/test_whole_lanes.cu, built by its own Makefile -- __graft_entry__.build() does it --
and run here on the GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_ensemble_whole_lanes")


def run(name, marker, args=(), cwd=None):
    exe = os.path.join(NATIVE, name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", NATIVE, name], check=True, capture_output=True)
    proc = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert proc.returncode == 0 and marker in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]


@pytest.mark.gpu
def test_the_lanes_that_ran_and_what_they_left():
    """A stateless functor that records the lanes that called it (every cell: exactly the min(L, n) lanes of its place
    in the round, forced and by the engine's rule; whole_step_lanes_used says the same); a functor with per-cell state
    that is not declared stateless (one lane per cell under the default, the counters of a take_step twin); a point
    type of 8 floats (no room for the terms of 16 lanes at n_max = 1024 and one row beyond the largest n_max the LDS
    rule admits: one lane per cell, still whole-step launches, the twin's bits); take_steps with 16 lanes per cell
    alternating with take_step carrying Links and a kernel that bumps d_n[r], in all three fixed modes."""
    run("test_whole_lanes", "ALL WHOLE-STEP LANES TESTS PASSED")
