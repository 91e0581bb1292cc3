"""Ensemble<Pt, Gabriel_solver> as a model program uses the header
(tests/native_ensemble/test_ensemble_gabriel.cu, built by that directory's Makefile -- __graft_entry__.build() does
it -- and run here on the GPU)."""
import pytest
from ensemble_support import run_native


@pytest.mark.gpu
def test_a_gabriel_sweep_written_against_the_header():
    """The reference's known answer (19-cell hexagon, grid 5, coefficient 0.8: 6 / 3 / 4 neighbours) counted by a
    functor that is not stateless, at GLOBAL ids in every replica of one ensemble; then a sweep model: the functor
    reads its replica's strength through i / n_max and a per-cell array by global id, Links over the flat id space
    are the generic forces, a kernel divides cells of some replicas by raising d_n[r] on the device between steps,
    one replica is dense -- every replica memcmp-equal to a Solution<float3, Gabriel_solver> run of the same system,
    with the centre of mass fixed and after set_fixed_xy."""
    run_native("test_ensemble_gabriel", "ALL GABRIEL ENSEMBLE TESTS PASSED")
