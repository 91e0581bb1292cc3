"""Ensemble<Pt, Grid_solver>::take_steps(dt, K, ya::ens::Replica_links) with launches that step from LDS, as a model
program uses the header (tests/native_ensemble_grid_links/test_grid_links.cu, built by that directory's Makefile --
__graft_entry__.build() does it -- and run here on the GPU)."""
import os
import subprocess

import pytest
from ensemble_support import ROOT

NATIVE = os.path.join(ROOT, "tests", "native_ensemble_grid_links")


@pytest.mark.gpu
def test_a_protrusion_sweep_on_a_grid_that_alternates_both_paths():
    """ONE Ensemble<float3, Grid_solver>: a kernel rewrites the links and their count before every call, replicas
    divide on the device, a `d_n_nbs[i] += 1` functor that is not declared stateless counts neighbours;
    take_steps(dt, K, Replica_links) from LDS alternates with take_step(dt, link_forces_ordered).  memcmp-equal --
    every row, old_v, counts, counters, status, grid arrays -- to a twin that never steps from LDS, in the three fixed
    modes and both summation orders, with 1 and 3 protrusions per cell."""
    exe = os.path.join(NATIVE, "test_grid_links")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", NATIVE], check=True, capture_output=True)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "ALL LINKED GRID LDS STEP TESTS PASSED" in proc.stdout, \
        proc.stdout[-2000:] + proc.stderr[-2000:]
