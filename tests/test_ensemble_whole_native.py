"""Ensemble<Pt, Tile_solver>::take_steps as a model program uses the header
(tests/native_ensemble_whole/test_whole_steps.cu, built by its own Makefile -- __graft_entry__.build() does it -- and
run here on the GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_ensemble_whole")


def run(name, marker, args=(), cwd=None):
    exe = os.path.join(NATIVE, name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", NATIVE, name], check=True, capture_output=True)
    proc = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert proc.returncode == 0 and marker in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]


@pytest.mark.gpu
def test_a_sweep_that_alternates_whole_step_launches_with_linked_steps():
    """A sweep model on ONE Ensemble: stretches of take_steps (whole-step launches, counted) alternate with
    take_step carrying Links as generic forces; the functor reads its replica's rest length through i / n_max and
    counts neighbours in a per-cell array without atomics; a kernel bumps d_n[r] on the device in between -- every
    row, count and counter bit for bit those of a twin Ensemble that only ever calls take_step, in all three fixed
    modes."""
    run("test_whole_steps", "ALL WHOLE-STEP TESTS PASSED")
