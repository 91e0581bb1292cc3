"""libyalla_ensemble_links.so (include/yalla_ensemble_links.h) loads without a GPU, exports exactly the C ABI its
header declares and the ctypes table mirrors, refuses what it does not know, and answers ya_lens_lds_bytes -- host
arithmetic only -- with ya::ens::lds_layout's bytes, held here against a Python restatement of the rule (no
compute calls here)."""
import ctypes
import os

import pytest
from ensemble_support import (LDS, LINKED_MODELS, ROOT, STATIC_LDS, check_abi, check_models_name_bounds,
                              check_only_the_c_abi_is_exported, largest_slots, lds_layout, up16)
from ensemble_support import LINKED_N_FLOATS as N_FLOATS
from ensemble_support import links_binding as binding

LIB = os.path.join(ROOT, "yalla_amd", "libyalla_ensemble_links.so")
LANES = [1, 4, 16, 64]


def test_header_table_and_library_agree():
    from yalla_amd import _ffi
    check_abi("yalla_ensemble_links.h", "ya_lens_", _ffi.LINKED_ENSEMBLE_ABI, LIB, _ffi.linked_ensemble_lib, 22,
              {"ya_lens_h_link", "ya_lens_set_n_links", "ya_lens_get_n_links", "ya_lens_whole_step_lanes_used",
               "ya_lens_lds_bytes"})
    assert _ffi.LINKED_ENSEMBLE_LIB == LIB


def test_only_the_c_abi_is_exported():
    check_only_the_c_abi_is_exported(LIB, "ya_lens_")


def test_the_model_table():
    from yalla_amd import ensemble
    names = ensemble.linked_models()
    assert names == ["links", "links4", "springs_links", "relu_links", "relu_po_links"] == LINKED_MODELS
    check_models_name_bounds(ensemble._ffi.linked_ensemble_lib().ya_lens_models_name, len(names))


def test_unknown_models_and_bad_arguments_are_refused_before_the_device_is_touched():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import LinkedEnsemble, YallaError
    lib = _ffi.linked_ensemble_lib()
    handle = ctypes.c_void_p()
    for name in (b"links_tile", b"relu", b"", b"no_such_model"):
        assert lib.ya_lens_create(name, 4, 100, 100, 0.2, ctypes.byref(handle)) == -1
        assert not handle.value
    bad = [(0, 100, 10, 0.2), (4, 0, 10, 0.2), (-1, 5, 10, 0.2), (70000, 70000, 1, 0.2),  # ids are ints,
           (4, 100, -1, 0.2), (70000, 10, 70000, 0.2),                                    # and so are slots
           (4, 100, 10, float("nan")), (4, 100, 10, float("inf"))]
    for m, n, slots, strength in bad:
        assert lib.ya_lens_create(b"links", m, n, slots, strength, ctypes.byref(handle)) == -3, (m, n, slots, strength)
        assert not handle.value
    with pytest.raises(YallaError, match="unknown linked ensemble model"):
        LinkedEnsemble("links_tile", 4, 100, 100)
    assert lib.ya_lens_lds_bytes(b"relu", 100, 100, 1) == -1
    for n_max, slots, lanes in ((0, 10, 1), (-3, 10, 1), (100, -1, 1), (100, 10, 0), (100, 10, 2), (100, 10, 8),
                                (100, 10, 32), (100, 10, 128)):
        assert lib.ya_lens_lds_bytes(b"links", n_max, slots, lanes) == -3, (n_max, slots, lanes)
    with pytest.raises(YallaError, match="-3"):
        LinkedEnsemble.lds_bytes("links", 100, 10, 2)


# ---- ya::ens::lds_layout<Pt, false, true>(n_max, S, lanes).bytes against its restatement (ensemble_support) ---------
def test_the_restated_rule():
    """What the header promises of the rule, on the restatement: 16-byte aligned, within the workgroup's LDS, the
    list's 4 (n_max + 1) + 8 S bytes behind the step's arrays, a tile of at least 4 partners where lanes fit."""
    for n_floats in (3, 4, 5):
        for n_max in (1, 16, 100, 256, 1024):
            for slots in (0, 1, n_max, 3 * n_max):
                one = lds_layout(n_floats, n_max, False, slots, 1).bytes
                assert one > 0 and one % 16 == 0 and one + STATIC_LDS <= LDS
                assert 0 <= one - up16(n_max * (16 * n_floats + 12) + n_floats * 1040) - 4 * (n_max + 1) - 8 * slots < 16
                for lanes in (4, 16, 64):
                    many = lds_layout(n_floats, n_max, False, slots, lanes).bytes
                    assert many == 0 or (many % 16 == 0 and many + STATIC_LDS <= LDS
                                         and (many - one) // ((256 // lanes) * (n_floats + 4) * 4) >= 4)
    # Po_cell at the capacity with three slots per cell: the list fits, the terms of 4 lanes do not, those of 16 do
    assert lds_layout(5, 1024, False, 3072, 1).bytes > 0 and lds_layout(5, 1024, False, 3072, 4).bytes == 0
    assert lds_layout(5, 1024, False, 3072, 16).bytes > 0
    assert lds_layout(3, 1024, False, largest_slots(3, 1024) + 1, 1).bytes == 0


@pytest.mark.parametrize("model", ["links", "links4", "relu_po_links"])  # (one per point type)
def test_lds_bytes_is_the_rule(model):
    """ya_lens_lds_bytes against the restatement: for lanes 1, 4, 16 and 64 at S in {0, 1, n_max, 3 n_max}, and on
    either side of every point -- along S and along n_max -- where another term of the rule starts to decide."""
    from yalla_amd.ensemble import LinkedEnsemble
    n_floats = N_FLOATS[model]
    points = set()
    for lanes in LANES:
        for n_max in (1, 2, 15, 16, 17, 100, 255, 256, 257, 1000, 1023, 1024):
            points |= {(n_max, slots, lanes) for slots in (0, 1, n_max, 3 * n_max)}
        for n_max in (16, 100, 256, 1024):  # along S, to beyond the LDS
            before = binding(n_floats, n_max, 0, lanes)
            for slots in range(1, LDS // 8 + 2):
                now = binding(n_floats, n_max, slots, lanes)
                if now != before:
                    points |= {(n_max, slots - 1, lanes), (n_max, slots, lanes)}
                    before = now
        for slots_per_cell in (0, 1, 3):  # along n_max
            before = binding(n_floats, 1, slots_per_cell, lanes)
            for n_max in range(2, 1025):
                now = binding(n_floats, n_max, slots_per_cell * n_max, lanes)
                if now != before:
                    points |= {(n_max - 1, slots_per_cell * (n_max - 1), lanes), (n_max, slots_per_cell * n_max, lanes)}
                    before = now
    seen = set()
    for n_max, slots, lanes in sorted(points):
        want = lds_layout(n_floats, n_max, False, slots, lanes).bytes
        assert LinkedEnsemble.lds_bytes(model, n_max, slots, lanes) == want, (n_max, slots, lanes)
        seen.add(binding(n_floats, n_max, slots, lanes))
    # every term decided somewhere (Po_cell's budget holds fewer partners than the longest tile, whatever the lanes)
    assert {-2, -1, 0, 2, 3, 4} | ({1} if n_floats < 5 else set()) <= seen


def test_the_python_class_mirrors_the_links():
    """LinkedEnsemble over a stand-in library: the links' view, the count and the launches counted."""
    import numpy as np
    from yalla_amd.ensemble import LinkedEnsemble

    class StandIn:
        def __init__(self):
            self.rows = (ctypes.c_float * (2 * 4 * 3))()
            self.links = (ctypes.c_int * (2 * 5 * 2))(*range(20))
            self.n_links = 10

        def ya_lens_create(self, model, n_replicas, n_max, slots, strength, out):
            assert (n_replicas, n_max, slots) == (2, 4, 5) and abs(strength.value - 0.3) < 1e-7
            out._obj.value = 1
            return 0

        def ya_lens_n_floats(self, handle):
            return 3

        def ya_lens_h_X(self, handle):
            return ctypes.cast(self.rows, ctypes.POINTER(ctypes.c_float))

        def ya_lens_h_link(self, handle):
            return ctypes.cast(self.links, ctypes.POINTER(ctypes.c_int))

        def ya_lens_get_n_links(self, handle):
            return self.n_links

        def ya_lens_set_n_links(self, handle, n):
            if not 0 <= n <= 10:
                return -3
            self.n_links = n
            return 0

        def ya_lens_take_steps(self, handle, dt, steps):
            return 2

        def ya_lens_destroy(self, handle):
            pass

    from yalla_amd.ensemble import YallaError
    lib = StandIn()
    ens = LinkedEnsemble("links", 2, 4, 5, strength=0.3, lib=lib)
    assert ens.h_link.shape == (2, 5, 2) and ens.h_link.dtype == np.int32
    assert ens.h_link[1, 2].tolist() == [14, 15]
    ens.h_link[0, 0] = (3, 2)
    assert lib.links[0] == 3 and lib.links[1] == 2
    assert ens.n_links == 10
    ens.n_links = 7
    assert lib.n_links == 7
    with pytest.raises(YallaError, match="-3"):
        ens.n_links = 11
    ens.take_step(0.1, 5)
    assert ens.whole_step_launches == 2
    ens.close()
