"""Ensemble<Pt, Grid_solver> as a model program uses the header (tests/native_ensemble/test_ensemble_grid.cu,
built by that directory's Makefile -- __graft_entry__.build() does it -- and run here on the GPU)."""
import pytest
from ensemble_support import run_native


@pytest.mark.gpu
def test_a_grid_parameter_sweep_written_against_the_header():
    """A sweep model: the functor reads its replica's strength through i / n_max and a per-cell array by global
    id, Links over the flat id space are the generic forces, a kernel divides cells of some replicas by raising
    d_n[r] on the device between steps, a functor that counts neighbours with a plain `d_n_nbs[i] += 1` (not
    stateless: one lane) -- every replica memcmp-equal to a Solution<float3, Grid_solver> run of the same system,
    for 0 / 1 / 4 / 8 / 16 lanes per cell, with the centre of mass fixed and after set_fixed_xy."""
    run_native("test_ensemble_grid", "ALL GRID ENSEMBLE TESTS PASSED")
