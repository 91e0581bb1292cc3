"""Ensemble<Pt, Grid_solver> as a model program uses the header (tests/native_ensemble_grid/test_ensemble_grid.cu,
built by its own Makefile -- __graft_entry__.build() does it -- and run here on the GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_ensemble_grid")


def run(name, marker, args=(), cwd=None):
    exe = os.path.join(NATIVE, name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", NATIVE, name], check=True, capture_output=True)
    proc = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert proc.returncode == 0 and marker in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]


@pytest.mark.gpu
def test_a_grid_parameter_sweep_written_against_the_header():
    """A sweep model: the functor reads its replica's strength through i / n_max and a per-cell array by global
    id, Links over the flat id space are the generic forces, a kernel divides cells of some replicas by raising
    d_n[r] on the device between steps, a functor that counts neighbours with a plain `d_n_nbs[i] += 1` (not
    stateless: one lane) -- every replica memcmp-equal to a Solution<float3, Grid_solver> run of the same system,
    for 0 / 1 / 4 / 8 / 16 lanes per cell, with the centre of mass fixed and after set_fixed_xy."""
    run("test_ensemble_grid", "ALL GRID ENSEMBLE TESTS PASSED")
