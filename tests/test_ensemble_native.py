"""Ensemble<Pt, Tile_solver> as a model program uses the header (tests/native_ensemble/test_ensemble.cu, built by
that directory's Makefile -- __graft_entry__.build() does it -- and run here on the GPU)."""
import pytest
from ensemble_support import run_native


@pytest.mark.gpu
def test_a_parameter_sweep_written_against_the_header():
    """A sweep model: the functor reads its replica's rest length through i / n_max and a per-cell array by
    global id, Links over the flat id space are the generic forces, a kernel appends daughters to some replicas
    by bumping d_n[r] on the device between steps, nothing is read back until the end -- every replica bit for
    bit a Solution<float3, Tile_solver> run of the same system, for 0 / 1 / 16 / 64 lanes per cell, with the
    centre of mass fixed and after set_fixed_xy."""
    run_native("test_ensemble", "ALL ENSEMBLE TESTS PASSED")
