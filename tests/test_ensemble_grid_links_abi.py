"""libyalla_ensemble_grid_links.so (include/yalla_ensemble_grid_links.h) loads without a GPU, exports exactly the C ABI
its header declares and the ctypes table mirrors, refuses what it does not know, and answers ya_glens_lds_bytes -- host
arithmetic only -- with ya::ens::grid_lds_links_bytes, held here against a Python restatement of the rule (no compute
calls here)."""
import ctypes
import os

import pytest
from ensemble_grid_links_support import MODELS, N_FLOATS
from ensemble_grid_lds_support import grid_lds_capacity
from ensemble_support import (LDS, ROOT, STATIC_LDS, check_abi, check_models_name_bounds,
                              check_only_the_c_abi_is_exported, largest_slots, lds_layout)

LIB = os.path.join(ROOT, "yalla_amd", "libyalla_ensemble_grid_links.so")


def test_header_table_and_library_agree():
    from yalla_amd import _ffi
    check_abi("yalla_ensemble_grid_links.h", "ya_glens_", _ffi.LINKED_GRID_ENSEMBLE_ABI, LIB,
              _ffi.linked_grid_ensemble_lib, 24,
              {"ya_glens_set_cube_size", "ya_glens_status", "ya_glens_get_grid", "ya_glens_h_link",
               "ya_glens_set_n_links", "ya_glens_get_n_links", "ya_glens_lds_bytes"})
    assert _ffi.LINKED_GRID_ENSEMBLE_LIB == LIB
    # the functions of yalla_ensemble_grid.h, all of them, under the other prefix
    from ensemble_support import declared_functions
    grid = {n.replace("ya_gens_", "ya_glens_") for n in declared_functions("yalla_ensemble_grid.h")}
    assert grid <= set(_ffi.LINKED_GRID_ENSEMBLE_ABI)
    for name in grid - {"ya_glens_create"}:
        assert _ffi.LINKED_GRID_ENSEMBLE_ABI[name] == _ffi.GRID_ENSEMBLE_ABI[name.replace("ya_glens_", "ya_gens_")]


def test_only_the_c_abi_is_exported():
    check_only_the_c_abi_is_exported(LIB, "ya_glens_")


def test_the_model_table():
    from yalla_amd import ensemble
    names = ensemble.linked_grid_models()
    assert names == ["links", "links4", "springs_links", "relu_links", "relu_po_links", "relu_cell8_links"] == MODELS
    check_models_name_bounds(ensemble._ffi.linked_grid_ensemble_lib().ya_glens_models_name, len(names))


def test_unknown_models_and_bad_arguments_are_refused_before_the_device_is_touched():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import LinkedGridEnsemble, YallaError
    lib = _ffi.linked_grid_ensemble_lib()
    handle = ctypes.c_void_p()
    for name in (b"links_grid", b"relu", b"", b"no_such_model"):
        assert lib.ya_glens_create(name, 4, 100, 8, 1.0, 100, 0.2, ctypes.byref(handle)) == -1
        assert not handle.value
    bad = [(0, 100, 8, 1.0, 10, 0.2), (4, 0, 8, 1.0, 10, 0.2), (-1, 5, 8, 1.0, 10, 0.2),
           (70000, 70000, 8, 1.0, 1, 0.2),                                      # ids are ints,
           (4, 100, 8, 1.0, -1, 0.2), (70000, 10, 2, 1.0, 70000, 0.2),          # and so are slots
           (4, 100, 0, 1.0, 10, 0.2), (4, 100, 257, 1.0, 10, 0.2),              # the grid's size
           (4, 100, 8, 0.0, 10, 0.2), (4, 100, 8, -1.0, 10, 0.2), (4, 100, 8, float("nan"), 10, 0.2),
           (4, 100, 8, 1.0, 10, float("nan")), (4, 100, 8, 1.0, 10, float("inf"))]
    for args in bad:
        assert lib.ya_glens_create(b"links", *args, ctypes.byref(handle)) == -3, args
        assert not handle.value
    with pytest.raises(YallaError, match="unknown linked grid ensemble model"):
        LinkedGridEnsemble("links_grid", 4, 100, 100, grid_size=8)
    assert lib.ya_glens_lds_bytes(b"relu", 100, 100) == -1
    assert lib.ya_glens_lds_bytes(None, 100, 100) == -3
    for n_max, slots in ((0, 10), (-3, 10), (100, -1)):
        assert lib.ya_glens_lds_bytes(b"links", n_max, slots) == -3, (n_max, slots)
    with pytest.raises(YallaError, match="-3"):
        LinkedGridEnsemble.lds_bytes("links", 100, -1)
    # set_param: an unknown name is -2 even on no handle, a known one on no handle -3
    assert lib.ya_glens_set_param(None, b"lanes", 1.0) == -2
    assert lib.ya_glens_set_param(None, b"whole_steps", 1.0) == -2
    for name in (b"sum_order", b"lds_steps", b"lds_steps_max", b"links_path"):
        assert lib.ya_glens_set_param(None, name, 1.0) == -3
    assert lib.ya_glens_set_param(None, None, 1.0) == -3


# ---- ya::ens::grid_lds_links_bytes<Pt>(n_max, S) against its restatement (ensemble_grid_links_support) ----------------
def test_the_restated_rule():
    """What the header promises of the rule, on the restatement: the step's arrays, then the keys, then the list of
    4 (n_max + 1) + 8 S bytes, 4-byte aligned, within the workgroup's LDS beside the fold's static scratch."""
    for n_floats in (3, 4, 5, 8):
        assert grid_lds_capacity(n_floats) == 1024
        for n_max in (1, 16, 100, 256, 512, 1023):
            for slots in (0, 1, n_max, 3 * n_max):
                got = lds_layout(n_floats, n_max, True, slots).bytes
                whole = lds_layout(n_floats, n_max, keys=True).bytes + 4 * (n_max + 1) + 8 * slots
                assert got == (whole if whole + STATIC_LDS <= LDS else 0)
                assert (got > 0) == (n_floats < 8 or n_max < 1023)  # (these shapes: only the widest point runs out)
                assert got % 4 == 0 and lds_layout(n_floats, n_max, keys=True).bytes % 8 == 0


@pytest.mark.parametrize("model", MODELS)
def test_lds_bytes_is_the_rule_and_zero_exactly_where_it_should_be(model):
    """ya_glens_lds_bytes against the restatement at n_max in {1, 1023, 1024} and others, for S in {0, 1, n_max,
    3 n_max}, and for the largest S that fits (found here, on the CPU) and one more: non-zero, then 0."""
    from yalla_amd.ensemble import LinkedGridEnsemble
    n_floats = N_FLOATS[model]
    for n_max in (1, 2, 63, 64, 65, 255, 256, 257, 512, 513, 1023, 1024):
        for slots in (0, 1, n_max, 3 * n_max):
            assert LinkedGridEnsemble.lds_bytes(model, n_max, slots) == lds_layout(n_floats, n_max, True, slots).bytes, \
                (n_max, slots)
    for n_max in (1, 1023, 1024):
        fits = largest_slots(n_floats, n_max, keys=True)
        if fits is None:  # not even the offsets of a list of no slots
            assert n_floats == 8 and n_max >= 1023
            assert LinkedGridEnsemble.lds_bytes(model, n_max, 0) == 0
            continue
        room = LDS - STATIC_LDS - lds_layout(n_floats, n_max, keys=True).bytes - 4 * (n_max + 1)
        assert fits == room // 8 and 0 <= room - 8 * fits < 8
        want = lds_layout(n_floats, n_max, keys=True).bytes + 4 * (n_max + 1) + 8 * fits
        assert LinkedGridEnsemble.lds_bytes(model, n_max, fits) == want > 0, (n_max, fits)
        assert LinkedGridEnsemble.lds_bytes(model, n_max, fits + 1) == 0, (n_max, fits + 1)
        assert LinkedGridEnsemble.lds_bytes(model, n_max, 2 ** 31 - 1) == 0


def test_an_eight_float_point_at_1024_rows_has_no_room_for_a_list():
    """The step's arrays and the keys of 1024 rows of 8 floats leave 896 bytes: the 1025 offsets of a list of NO slots
    do not fit, so the rule is 0 for S = 0 (and every S); at 1023 rows the keys are as many and the arrays one row of
    140 bytes shorter, no room either.  The GPU tests pick their shapes by this: relu_cell8_links at n_max = 1024 never steps from LDS."""
    from yalla_amd.ensemble import LinkedGridEnsemble
    assert LDS - STATIC_LDS - lds_layout(8, 1024, keys=True).bytes == 896 < 4 * 1025
    assert lds_layout(8, 1024, True, 0).bytes == 0
    assert LinkedGridEnsemble.lds_bytes("relu_cell8_links", 1024, 0) == 0
    assert LinkedGridEnsemble.lds_bytes("relu_cell8_links", 1024, 1024) == 0
    assert 896 < LDS - STATIC_LDS - lds_layout(8, 1023, keys=True).bytes <= 896 + 140 < 4 * 1024
    assert LinkedGridEnsemble.lds_bytes("relu_cell8_links", 1023, 0) == 0
    # the largest n_max of 8 floats with room for a list of one slot per cell, found on the CPU
    n_max = max(n for n in range(1, 1025) if lds_layout(8, n, True, n).bytes > 0)
    assert LinkedGridEnsemble.lds_bytes("relu_cell8_links", n_max, n_max) == lds_layout(8, n_max, True, n_max).bytes > 0
    assert LinkedGridEnsemble.lds_bytes("relu_cell8_links", n_max + 1, n_max + 1) == 0
    # the 7-float and smaller points keep room at 1024 rows
    for model in MODELS[:-1]:
        assert LinkedGridEnsemble.lds_bytes(model, 1024, 1024) > 0


def test_the_python_class_mirrors_the_links_and_the_grid():
    """LinkedGridEnsemble over a stand-in library: create's arguments in the header's order, the links' view, the
    count and the launches counted."""
    import numpy as np
    from yalla_amd.ensemble import LinkedGridEnsemble, YallaError

    class StandIn:
        def __init__(self):
            self.rows = (ctypes.c_float * (2 * 4 * 3))()
            self.links = (ctypes.c_int * (2 * 5 * 2))(*range(20))
            self.n_links = 10
            self.cube_size = None

        def ya_glens_create(self, model, n_replicas, n_max, grid_size, cube_size, slots, strength, out):
            assert (n_replicas, n_max, grid_size, slots) == (2, 4, 7, 5)
            assert abs(cube_size.value - 1.5) < 1e-7 and abs(strength.value - 0.3) < 1e-7
            out._obj.value = 1
            return 0

        def ya_glens_n_floats(self, handle):
            return 3

        def ya_glens_h_X(self, handle):
            return ctypes.cast(self.rows, ctypes.POINTER(ctypes.c_float))

        def ya_glens_h_link(self, handle):
            return ctypes.cast(self.links, ctypes.POINTER(ctypes.c_int))

        def ya_glens_get_n_links(self, handle):
            return self.n_links

        def ya_glens_set_n_links(self, handle, n):
            if not 0 <= n <= 10:
                return -3
            self.n_links = n
            return 0

        def ya_glens_set_cube_size(self, handle, value):
            self.cube_size = value
            return 0

        def ya_glens_status(self, handle, r, clear):
            return 1 if r == 1 else 0

        def ya_glens_take_steps(self, handle, dt, steps):
            return 2

        def ya_glens_destroy(self, handle):
            pass

    lib = StandIn()
    ens = LinkedGridEnsemble("links", 2, 4, 5, strength=0.3, grid_size=7, cube_size=1.5, lib=lib)
    assert ens.grid_size == 7 and ens.slots_per_replica == 5
    assert ens.h_link.shape == (2, 5, 2) and ens.h_link.dtype == np.int32
    assert ens.h_link[1, 2].tolist() == [14, 15]
    ens.h_link[0, 0] = (3, 2)
    assert lib.links[0] == 3 and lib.links[1] == 2
    assert ens.n_links == 10
    ens.n_links = 7
    assert lib.n_links == 7
    with pytest.raises(YallaError, match="-3"):
        ens.n_links = 11
    ens.cube_size = 1.25
    assert lib.cube_size == 1.25
    assert [ens.status(0), ens.status(1)] == [0, 1]
    ens.take_step(0.1, 5)
    assert ens.lds_step_launches == 2
    with pytest.raises(AttributeError):
        ens.whole_step_launches
    ens.close()
