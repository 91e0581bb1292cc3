"""A time step and a Gabriel coefficient per replica as a model program uses the headers
(tests/native_ensemble/test_replica_dt.cu, built by that directory's Makefile -- __graft_entry__.build() does it -- and
run here on the GPU)."""
import pytest
from ensemble_support import run_native


@pytest.mark.gpu
def test_a_model_kernel_halves_the_time_steps_of_crowded_replicas_between_two_calls():
    """take_steps(ya::ens::Replica_dt{d_dt}, 3), a kernel that halves d_dt[r] where d_n[r] exceeds a bound, then
    take_steps(..., 2), nothing read by the host in between: every replica of an Ensemble<float3> and of an
    Ensemble<float3, Gabriel_solver> with d_gabriel_coefficients set holds the positions and old_v of a lone Solution
    stepped with its values, on the launch-sequence path and from LDS."""
    run_native("test_replica_dt", "ALL REPLICA DT TESTS PASSED")
