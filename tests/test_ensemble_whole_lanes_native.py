"""Ensemble<Pt, Tile_solver>::whole_step_lanes as a model program uses the header
(tests/native_ensemble/test_whole_lanes.cu, built by that directory's Makefile -- __graft_entry__.build() does it --
and run here on the GPU)."""
import pytest
from ensemble_support import run_native


@pytest.mark.gpu
def test_the_lanes_that_ran_and_what_they_left():
    """A stateless functor that records the lanes that called it (every cell: exactly the min(L, n) lanes of its place
    in the round, forced and by the engine's rule; whole_step_lanes_used says the same); a functor with per-cell state
    that is not declared stateless (one lane per cell under the default, the counters of a take_step twin); a point
    type of 8 floats (no room for the terms of 16 lanes at n_max = 1024 and one row beyond the largest n_max the LDS
    rule admits: one lane per cell, still whole-step launches, the twin's bits); take_steps with 16 lanes per cell
    alternating with take_step carrying Links and a kernel that bumps d_n[r], in all three fixed modes."""
    run_native("test_whole_lanes", "ALL WHOLE-STEP LANES TESTS PASSED")
