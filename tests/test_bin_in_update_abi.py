"""Where the counter of Heun_solver::bin_in_update lives: `ya_sim_fused_bin_rebuilds` is exported by the device
library alone (under YA_IS_DEVICE, as `ya_sim_carried_steps`), is not part of include/yalla_models.h, and reads -1
through `Solution.fused_bin_rebuilds()` on a library without it.  No GPU needed: nothing here computes."""
import ctypes
import os
import re

from yalla_amd import _ffi
from yalla_amd.solution import Solution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_oracle_has_no_such_counter(oracle):
    assert not hasattr(oracle, "ya_sim_carried_steps")
    assert not hasattr(oracle, "ya_sim_fused_bin_rebuilds")  # device build only
    with Solution("springs_grid", 100, 16, 1.0, lib=oracle) as s:
        assert s.fused_bin_rebuilds() == -1


def test_the_device_library_exports_it_outside_the_models_header():
    if not os.path.exists(_ffi.DEVICE_LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_ffi.DEVICE_LIB, mode=ctypes.RTLD_LOCAL)  # (loading alone touches no GPU)
    assert hasattr(lib, "ya_sim_carried_steps") and hasattr(lib, "ya_sim_fused_bin_rebuilds")
    header = open(os.path.join(ROOT, "include", "yalla_models.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "ya_sim_fused_bin_rebuilds" not in header and "ya_sim_fused_bin_rebuilds" not in _ffi.MODELS_ABI
