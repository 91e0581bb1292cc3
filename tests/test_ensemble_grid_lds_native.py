"""Ensemble<Pt, Grid_solver>::take_steps as launches that step from LDS, as a model program uses the header
(tests/native_ensemble_grid_lds/test_grid_lds_steps.cu, built by that directory's Makefile -- __graft_entry__.build()
does it -- and run here on the GPU)."""
import os
import subprocess

import pytest
from ensemble_support import ROOT

NATIVE = os.path.join(ROOT, "tests", "native_ensemble_grid_lds")


@pytest.mark.gpu
def test_a_grid_sweep_that_alternates_both_paths_a_neighbour_counter_and_a_wide_point():
    """ONE Ensemble<float3, Grid_solver> alternating take_steps(dt, 4) from LDS with take_step(dt, link forces) and
    division on the device, memcmp-equal -- every row, old_v, counts, kinds, status, grid arrays -- to a twin that
    only calls take_step, in both summation orders; the counters of an undeclared `d_n_nbs[i] += 1` functor equal the
    twin's (one thread per cell); a MAKE_PT type of 8 floats at ya::ens::grid_lds_capacity and one row beyond."""
    exe = os.path.join(NATIVE, "test_grid_lds_steps")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", NATIVE], check=True, capture_output=True)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "ALL GRID LDS STEP TESTS PASSED" in proc.stdout, \
        proc.stdout[-2000:] + proc.stderr[-2000:]
