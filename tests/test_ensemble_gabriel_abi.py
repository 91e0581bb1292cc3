"""libyalla_ensemble_gabriel.so (include/yalla_ensemble_gabriel.h) loads without a GPU, exports exactly the C ABI its
header declares and the ctypes table mirrors, and refuses what it does not know (no compute calls here)."""
import ctypes
import os

import pytest
from ensemble_support import (FRICTION_MODELS, ROOT, check_abi, check_models_name_bounds, check_only_the_c_abi_is_exported,
                              declared_functions)

LIB = os.path.join(ROOT, "yalla_amd", "libyalla_ensemble_gabriel.so")
MODELS = ["relu", "clipped", "relu_plain", "relu_po", "relu_cell", "clipped_push"]


def test_header_table_and_library_agree():
    from yalla_amd import _ffi
    names = check_abi("yalla_ensemble_gabriel.h", "ya_gabens_", _ffi.GABRIEL_ENSEMBLE_ABI, LIB,
                      _ffi.gabriel_ensemble_lib, 21,
                      {"ya_gabens_set_cube_size", "ya_gabens_status", "ya_gabens_get_grid", "ya_gabens_dense_cells"})
    # the grid harness's twenty functions, and dense_cells
    from_grid = {n.replace("ya_gens_", "ya_gabens_") for n in declared_functions("yalla_ensemble_grid.h")}
    assert len(from_grid) == 20 and set(names) - from_grid == {"ya_gabens_dense_cells"}
    # create takes one value more than the grid's: the coefficient, a float before the handle
    grid_args = _ffi.GRID_ENSEMBLE_ABI["ya_gens_create"][1]
    args = _ffi.GABRIEL_ENSEMBLE_ABI["ya_gabens_create"][1]
    assert args == grid_args[:-1] + [ctypes.c_float] + grid_args[-1:]
    assert _ffi.GABRIEL_ENSEMBLE_LIB == LIB


def test_only_the_gabriel_ensemble_c_abi_is_exported():
    check_only_the_c_abi_is_exported(LIB, "ya_gabens_")


def test_the_model_table():
    from yalla_amd import GabrielEnsemble, GridEnsemble, ensemble
    assert issubclass(GabrielEnsemble, GridEnsemble)   # grid(r), status(r) and the cube_size setter come with it
    names = ensemble.gabriel_models()
    assert names == MODELS + FRICTION_MODELS
    check_models_name_bounds(ensemble._ffi.gabriel_ensemble_lib().ya_gabens_models_name, len(names))


def test_unknown_models_bad_sizes_and_bad_values_are_refused_before_the_device_is_touched():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import GabrielEnsemble, YallaError
    lib = _ffi.gabriel_ensemble_lib()
    handle = ctypes.c_void_p()
    for name in (b"relu_gabriel", b"springs", b"push", b"count", b"", b"no_such_model"):
        assert lib.ya_gabens_create(name, 4, 100, 8, 1.0, 0.8, ctypes.byref(handle)) == -1
        assert not handle.value
    bad = [
        (0, 100, 8), (4, 0, 8), (-1, 5, 8), (4, 100, 0),
        (70000, 70000, 8),     # n_replicas * n_max > 2^31 - 1: ids are ints
        (2 ** 24, 100, 8),     # n_replicas * (grid_size^3 + 1) > 2^31 - 1: 2^24 * 513
        (128, 10, 256),        # the same with the largest grid: 128 * (2^24 + 1)
        (4, 100, 257),         # grid_size > YA_MAX_GRID_SIZE: cube ids are binary32
    ]
    for m, n, gs in bad:
        assert lib.ya_gabens_create(b"relu", m, n, gs, 1.0, 0.8, ctypes.byref(handle)) == -3, (m, n, gs)
        assert not handle.value
    for cube_size in (0.0, -1.0, float("nan")):
        assert lib.ya_gabens_create(b"relu", 4, 100, 8, cube_size, 0.8, ctypes.byref(handle)) == -3
        assert not handle.value
    for coefficient in (float("nan"), float("inf"), float("-inf")):
        assert lib.ya_gabens_create(b"relu", 4, 100, 8, 1.0, coefficient, ctypes.byref(handle)) == -3
        assert not handle.value
    with pytest.raises(YallaError, match="unknown Gabriel ensemble model"):
        GabrielEnsemble("relu_gabriel", 4, 100, 8)


def test_the_grid_only_knobs_are_unknown_parameters():
    """set_param knows "gabriel_coefficient" only: a name it does not know is -2 whatever the handle is (so this
    needs no ensemble, hence no device), as the single-system Gabriel models refuse the grid-only knobs."""
    from yalla_amd import _ffi
    lib = _ffi.gabriel_ensemble_lib()
    for knob in (b"lanes", b"sum_order", b"whole_steps", b"cube_size"):
        assert lib.ya_gabens_set_param(None, knob, 1.0) == -2
    assert lib.ya_gabens_set_param(None, None, 1.0) == -3
    assert lib.ya_gabens_set_param(None, b"gabriel_coefficient", 0.5) == -3   # known, but no ensemble to set it on
