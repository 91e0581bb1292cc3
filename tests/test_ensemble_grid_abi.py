"""libyalla_ensemble_grid.so (include/yalla_ensemble_grid.h) loads without a GPU, exports exactly the C ABI its
header declares and the ctypes table mirrors, and refuses what it does not know (no compute calls here)."""
import ctypes
import os

import pytest
from ensemble_support import FRICTION_MODELS, ROOT, check_abi, check_models_name_bounds, check_only_the_c_abi_is_exported

LIB = os.path.join(ROOT, "yalla_amd", "libyalla_ensemble_grid.so")
MODELS = ["springs", "clipped", "fading", "relu", "relu_po", "relu_cell", "push", "clipped_push"]


def test_header_table_and_library_agree():
    from yalla_amd import _ffi
    # the all-pairs harness's functions, and the grid's own
    check_abi("yalla_ensemble_grid.h", "ya_gens_", _ffi.GRID_ENSEMBLE_ABI, LIB, _ffi.grid_ensemble_lib, 20,
              {"ya_gens_set_cube_size", "ya_gens_status", "ya_gens_get_grid"})
    assert _ffi.GRID_ENSEMBLE_LIB == LIB


def test_only_the_grid_ensemble_c_abi_is_exported():
    check_only_the_c_abi_is_exported(LIB, "ya_gens_")


def test_the_model_table():
    from yalla_amd import GridEnsemble, ensemble  # noqa: F401  (the package exports the class)
    names = ensemble.grid_models()
    assert names == MODELS + FRICTION_MODELS
    check_models_name_bounds(ensemble._ffi.grid_ensemble_lib().ya_gens_models_name, len(names))


def test_unknown_models_and_bad_sizes_are_refused_before_the_device_is_touched():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import GridEnsemble, YallaError
    lib = _ffi.grid_ensemble_lib()
    handle = ctypes.c_void_p()
    for name in (b"springs_grid", b"relu_tile", b"oscillator", b"", b"no_such_model"):
        assert lib.ya_gens_create(name, 4, 100, 8, 1.0, ctypes.byref(handle)) == -1
        assert not handle.value
    bad = [
        (0, 100, 8), (4, 0, 8), (-1, 5, 8), (4, 100, 0),
        (70000, 70000, 8),     # n_replicas * n_max > 2^31 - 1: ids are ints
        (2 ** 24, 100, 8),     # n_replicas * (grid_size^3 + 1) > 2^31 - 1: 2^24 * 513
        (128, 10, 256),        # the same with the largest grid: 128 * (2^24 + 1)
        (4, 100, 257),         # grid_size > YA_MAX_GRID_SIZE: cube ids are binary32
    ]
    for m, n, gs in bad:
        assert lib.ya_gens_create(b"springs", m, n, gs, 1.0, ctypes.byref(handle)) == -3, (m, n, gs)
        assert not handle.value
    assert lib.ya_gens_create(b"springs", 4, 100, 8, 0.0, ctypes.byref(handle)) == -3  # cube_size
    assert not handle.value
    with pytest.raises(YallaError, match="unknown grid ensemble model"):
        GridEnsemble("springs_grid", 4, 100, 8)
