"""libyalla_ensemble_links.so (include/yalla_ensemble_links.h) loads without a GPU, exports exactly the C ABI its
header declares and the ctypes table mirrors, refuses what it does not know, and answers ya_lens_lds_bytes -- host
arithmetic only -- with ya::ens::whole_step_links_lds_bytes, held here against a Python restatement of the rule (no
compute calls here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "yalla_amd", "libyalla_ensemble_links.so")
MODELS = ["links", "links4", "springs_links", "relu_links", "relu_po_links"]
N_FLOATS = {"links": 3, "links4": 4, "springs_links": 3, "relu_links": 3, "relu_po_links": 5}
LANES = [1, 4, 16, 64]


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ya_[A-Za-z0-9_]+)\s*\(", text)))


def built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", built(path)], capture_output=True, text=True, check=True).stdout
    return [(line.split()[-2], line.split()[-1]) for line in out.splitlines() if line.strip()]


def test_header_table_and_library_agree():
    from yalla_amd import _ffi
    names = declared_functions("yalla_ensemble_links.h")
    assert len(names) == 22 and all(n.startswith("ya_lens_") for n in names)
    shared = {n.replace("ya_ens_", "ya_lens_") for n in declared_functions("yalla_ensemble.h")}
    assert shared < set(names), "the shared entry points of the other harnesses"
    assert set(names) - shared == {"ya_lens_h_link", "ya_lens_set_n_links", "ya_lens_get_n_links",
                                   "ya_lens_whole_step_lanes_used", "ya_lens_lds_bytes"}
    assert set(names) == set(_ffi.LINKED_ENSEMBLE_ABI), "ctypes table and header disagree"
    functions = {sym for kind, sym in exported(LIB) if kind == "T" and sym.startswith("ya_")}
    assert functions == set(names), "library and header disagree"
    lib = _ffi.linked_ensemble_lib()  # types every entry point; AttributeError if one is missing
    assert lib is _ffi.linked_ensemble_lib()
    assert _ffi.LINKED_ENSEMBLE_LIB == LIB


def test_only_the_c_abi_is_exported():
    for kind, sym in exported(LIB):
        if sym.startswith("ya_lens_") or sym.startswith("__hip") or kind in ("V", "D", "B", "R"):
            continue
        raise AssertionError(f"{kind} {sym}")
    assert not [sym for _, sym in exported(LIB) if sym.startswith("ya_") and not sym.startswith("ya_lens_")]


def test_the_model_table():
    from yalla_amd import ensemble
    names = ensemble.linked_models()
    assert names == MODELS
    lib = ensemble._ffi.linked_ensemble_lib()
    assert lib.ya_lens_models_name(-1) is None and lib.ya_lens_models_name(len(names)) is None


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


# ---- ya::ens::whole_step_links_lds_bytes<Pt>(n_max, S, lanes), restated from the headers ---------------------------
LDS, STATIC_LDS, MIN_TILE, MAX_TILE, BUDGET = 160 * 1024, 3 * 256 * 4, 16, 256, 32 * 1024


def up16(x):
    return -(-x // 16) * 16


def part_base(n_floats, n_max, slots):
    """Where the term buffer starts: the step's arrays (X, X1, dX, dX1, old_v; fold256's scratch; 4 partial sums),
    16-byte aligned, then the incidence list of n_max + 1 offsets and 2 S entries, 16-byte aligned."""
    whole = n_max * (4 * 4 * n_floats + 12) + n_floats * 256 * 4 + n_floats * 4 * 4
    return up16(up16(whole) + 4 * (n_max + 1) + 8 * slots)


def tile_of(n_floats, n_max, slots, lanes):
    """(start, bytes per partner, tile length, which bound cut last) by the coop rule's statements, in their order,
    behind that start: n_max rounded up to 4 (0); at most the longest tile (1); at most what the budget holds but no
    less than the shortest tile where it cuts (2); at most the room left in the workgroup's LDS (3)."""
    base = part_base(n_floats, n_max, slots)
    per_partner = (256 // lanes) * (n_floats + 4) * 4
    room = (LDS - STATIC_LDS - base) // per_partner // 4 * 4
    budget = BUDGET // per_partner // 4 * 4
    tile, which = -(-n_max // 4) * 4, 0
    if tile > MAX_TILE:
        tile, which = MAX_TILE, 1
    if tile > budget:
        tile, which = max(budget, MIN_TILE), 2
    if tile > room:
        tile, which = room, 3
    return base, per_partner, tile, which


def binding(n_floats, n_max, slots, lanes):
    """What decides the answer: -2 = the list does not fit (0), -1 = the shortest tile does not fit beside it (0),
    4 = one lane per cell (the list's end), 0 .. 3 = that bound of the tile length."""
    base = part_base(n_floats, n_max, slots)
    if base + STATIC_LDS > LDS:
        return -2
    if lanes == 1:
        return 4
    _, per_partner, _, which = tile_of(n_floats, n_max, slots, lanes)
    if base + STATIC_LDS + MIN_TILE * per_partner > LDS:
        return -1
    return which


def links_lds_bytes(n_floats, n_max, slots, lanes):
    if binding(n_floats, n_max, slots, lanes) < 0:
        return 0
    base, per_partner, tile, _ = tile_of(n_floats, n_max, slots, lanes)
    return base if lanes == 1 else base + tile * per_partner


def largest_slots(n_floats, n_max, lanes=1):
    """The largest S whose launch fits (the rule falls monotonically to 0 in S)."""
    lo, hi = 0, LDS  # fits, does not
    assert links_lds_bytes(n_floats, n_max, lo, lanes) > 0 and links_lds_bytes(n_floats, n_max, hi, lanes) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if links_lds_bytes(n_floats, n_max, mid, lanes) > 0 else (lo, mid)
    return lo


def test_the_restated_rule():
    """What the header promises of the rule, on the restatement: 16-byte aligned, within the workgroup's LDS, the
    list's 4 (n_max + 1) + 8 S bytes behind the step's arrays, a tile of at least 4 partners where lanes fit."""
    for n_floats in (3, 4, 5):
        for n_max in (1, 16, 100, 256, 1024):
            for slots in (0, 1, n_max, 3 * n_max):
                one = links_lds_bytes(n_floats, n_max, slots, 1)
                assert one > 0 and one % 16 == 0 and one + STATIC_LDS <= LDS
                assert 0 <= one - up16(n_max * (16 * n_floats + 12) + n_floats * 1040) - 4 * (n_max + 1) - 8 * slots < 16
                for lanes in (4, 16, 64):
                    many = links_lds_bytes(n_floats, n_max, slots, lanes)
                    assert many == 0 or (many % 16 == 0 and many + STATIC_LDS <= LDS
                                         and (many - one) // ((256 // lanes) * (n_floats + 4) * 4) >= 4)
    # Po_cell at the capacity with three slots per cell: the list fits, the terms of 4 lanes do not, those of 16 do
    assert links_lds_bytes(5, 1024, 3072, 1) > 0 and links_lds_bytes(5, 1024, 3072, 4) == 0
    assert links_lds_bytes(5, 1024, 3072, 16) > 0
    assert links_lds_bytes(3, 1024, largest_slots(3, 1024) + 1, 1) == 0


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
        want = links_lds_bytes(n_floats, n_max, slots, lanes)
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
