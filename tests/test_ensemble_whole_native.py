"""Ensemble<Pt, Tile_solver>::take_steps as a model program uses the header
(tests/native_ensemble/test_whole_steps.cu, built by that directory's Makefile -- __graft_entry__.build() does it -- and
run here on the GPU)."""
import pytest
from ensemble_support import run_native


@pytest.mark.gpu
def test_a_sweep_that_alternates_whole_step_launches_with_linked_steps():
    """A sweep model on ONE Ensemble: stretches of take_steps (whole-step launches, counted) alternate with
    take_step carrying Links as generic forces; the functor reads its replica's rest length through i / n_max and
    counts neighbours in a per-cell array without atomics; a kernel bumps d_n[r] on the device in between -- every
    row, count and counter bit for bit those of a twin Ensemble that only ever calls take_step, in all three fixed
    modes."""
    run_native("test_whole_steps", "ALL WHOLE-STEP TESTS PASSED")
