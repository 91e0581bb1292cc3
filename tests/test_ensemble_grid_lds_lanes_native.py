"""Ensemble<Pt, Grid_solver>::lds_step_lanes, several lanes per cell inside the launches that step from LDS, as a model
program uses the header (tests/native_ensemble_grid_lds/test_grid_lds_lanes.cu, built by that directory's lanes.mk --
__graft_entry__.build() does it -- and run here on the GPU)."""
import os
import subprocess

import pytest
from ensemble_support import ROOT

NATIVE = os.path.join(ROOT, "tests", "native_ensemble_grid_lds")


@pytest.mark.gpu
def test_which_lanes_call_a_stateless_functor_a_neighbour_counter_and_a_wide_point():
    """A YA_STATELESS functor that records the lanes that called it and counts its calls per pair: forced lanes and the
    rule under 0 show several lanes per cell, all of the cell's slot, and every candidate inside the cut-off exactly
    once per stage; an undeclared `d_n_nbs[i] += 1` functor keeps one thread per cell under the default and counts
    what the 14-launch twin counts; a MAKE_PT type of 8 floats at n_max = 1024 (one lane: no room for the terms), at
    the largest n_max the rule admits for 16 lanes and one beyond."""
    exe = os.path.join(NATIVE, "test_grid_lds_lanes")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", NATIVE, "-f", "lanes.mk"], check=True, capture_output=True)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "ALL GRID LDS LANES TESTS PASSED" in proc.stdout, \
        proc.stdout[-2000:] + proc.stderr[-2000:]
