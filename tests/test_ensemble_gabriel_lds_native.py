"""Ensemble<Pt, Gabriel_solver>::take_steps as a model program uses the header
(tests/native_ensemble/test_gabriel_lds_steps.cu, built by that directory's Makefile -- __graft_entry__.build() does
it -- and run here on the GPU)."""
import pytest
from ensemble_support import run_native


@pytest.mark.gpu
def test_take_steps_alternating_with_take_step_under_a_counting_functor():
    """One Ensemble<float3, Gabriel_solver> alternates take_steps (launches that step from LDS) with take_step; its
    functor counts neighbours with a plain `d_n_nbs[i] += 1` (not stateless) at global ids and reads its replica's
    strength; cells divide on the device in between; one replica is dense.  A twin that only calls take_step holds
    the same positions, old_v, counts and neighbour counters, with the centre of mass fixed and after set_fixed_xy."""
    run_native("test_gabriel_lds_steps", "ALL GABRIEL LDS STEP TESTS PASSED")
