"""libyalla_ensemble.so (include/yalla_ensemble.h) loads without a GPU, exports exactly the C ABI its header
declares and the ctypes table mirrors, and refuses what it does not know (no compute calls here)."""
import ctypes
import os

import pytest
from ensemble_support import FRICTION_MODELS, ROOT, check_abi, check_models_name_bounds, check_only_the_c_abi_is_exported

LIB = os.path.join(ROOT, "yalla_amd", "libyalla_ensemble.so")


def test_header_table_and_library_agree():
    from yalla_amd import _ffi
    check_abi("yalla_ensemble.h", "ya_ens_", _ffi.ENSEMBLE_ABI, LIB, _ffi.ensemble_lib, 17, set())
    assert _ffi.ENSEMBLE_LIB == LIB


def test_only_the_ensemble_c_abi_is_exported():
    """No ya_sim_* / ya_models_* entry point of the model harness either."""
    check_only_the_c_abi_is_exported(LIB, "ya_ens_")


def test_the_model_table():
    from yalla_amd import ensemble
    names = ensemble.models()
    assert names == ["springs", "clipped", "fading", "relu", "relu_po", "oscillator", "push"] + FRICTION_MODELS
    check_models_name_bounds(ensemble._ffi.ensemble_lib().ya_ens_models_name, len(names))


def test_unknown_models_and_bad_sizes_are_refused_before_the_device_is_touched():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import Ensemble, YallaError
    lib = _ffi.ensemble_lib()
    handle = ctypes.c_void_p()
    for name in (b"springs_tile", b"relu_grid", b"", b"no_such_model"):
        assert lib.ya_ens_create(name, 4, 100, ctypes.byref(handle)) == -1
        assert not handle.value
    for m, n in ((0, 100), (4, 0), (-1, 5), (70000, 70000)):  # the last: ids are ints
        assert lib.ya_ens_create(b"springs", m, n, ctypes.byref(handle)) == -3
        assert not handle.value
    with pytest.raises(YallaError, match="unknown ensemble model"):
        Ensemble("springs_tile", 4, 100)
