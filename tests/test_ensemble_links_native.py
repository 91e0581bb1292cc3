"""Ensemble<Pt, Tile_solver>::take_steps with ya::ens::Replica_links as a model program uses the header
(tests/native_ensemble/test_links.cu, built by that directory's Makefile -- __graft_entry__.build() does it -- and run
here on the GPU)."""
import pytest
from ensemble_support import run_native


@pytest.mark.gpu
def test_a_protrusion_sweep_whole_against_the_six_launch_ordered_twin():
    """A protrusion sweep in the shape of the reference's intercalation model on ONE Ensemble, 1 and 3 protrusions
    per cell: a deterministic kernel renews the links (and their count) on the device before every step, replicas
    divide on the device in between, take_steps(dt, 1, Replica_links) -- whole-step launches, counted -- alternates
    with take_step(dt, gen) where gen calls link_forces_ordered; the functor counts neighbours in a per-cell array
    without atomics and is not declared stateless, so the launches keep one lane per cell.  Every row, count and
    counter bit for bit those of a twin that only ever takes the six-launch ordered path, in all three fixed
    modes.  Then replicas of at most 40 cells under the default lanes, where the rule gives a stateless functor 4
    lanes per cell: the counting functor keeps one lane and every counter, the same force declared stateless gets 4
    lanes, both with the twin's bits."""
    run_native("test_links", "ALL LINKED WHOLE-STEP TESTS PASSED")
