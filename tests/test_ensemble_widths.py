"""The ensemble harnesses of points of 4 to 16 floats (yalla_amd/csrc/ensemble_widths_models.h) through the layers that
need no GPU:

  * THE LDS RULES of the launches that step from LDS (ya::ens::lds_layout, ya::ens::gabriel_lds_layout and the three
    capacities), restated in tests/ensemble_support.py and tests/test_ensemble_gabriel_lds_abi.py, held line for line to
    what a stand-alone host program prints from the headers' constexpr functions for points of 4, 6, 8, 9, 11 and 16
    floats (sizeof 16, 24, 32, 36, 44, 64): both KEYS values, lanes 1 / 4 / 16 / 64, each type's capacity and one more,
    and the n_max at which the Gabriel launch's dense sets go 4 -> 2 -> 1 -- and to the literal table of capacities
    that the GPU tests' shapes rest on;
  * which (n_max, lanes) pairs have room for the term buffer of a several-lane launch, for every type: the shapes of
    tests/test_ensemble_widths_gpu.py are taken from here, not from trial;
  * the three libraries export every symbol of their headers, list exactly the rows fields_<type> and report the
    types' widths;
  * the start states' extra fields, and THE PREMISE that makes a dropped column visible: the oracle changes every extra
    field of every cell that has a neighbour within 1.
"""
import os
import subprocess

import numpy as np
import pytest

import ensemble_widths_support as ew
import widths_support as ws
from ensemble_support import (LDS, STATIC_LDS, capacity, check_models_name_bounds, check_only_the_c_abi_is_exported,
                              declared_functions, exported, grid_capacity, lds_layout, tile_behind)
from test_ensemble_gabriel_lds_abi import gabriel_lds_layout
from yalla_amd import _ffi
from yalla_amd.solution import Solution

ROOT = ws.ROOT
KINDS = list(ew.CAPACITY)
LANES = (1, 4, 16, 64)

# The capacities by point type, literally (the issue's table; ensemble_widths_models.h static_asserts the same):
#         floats sizeof  all-pairs  grid  Gabriel  Gabriel dense sets: first n_max with 2 / with 1
TABLE = {
    "float4": (4, 16, 1024, 1024, 995, 530, 770),
    "w6": (6, 24, 1024, 1024, 696, 432, 568),
    "w8": (8, 32, 1024, 1024, 512, 343, 449),
    "w9": (9, 36, 970, 918, 459, 305, 394),
    "w11": (11, 44, 794, 750, 346, 249, 303),
    "w16": (16, 64, 537, 512, 176, 134, 160),
}


def sizes(kind):
    """The n_max whose layouts are printed: small ones, the Gabriel list's 64 / 65, every capacity and one more, the
    dense sets' changes and the row before."""
    _, _, tile, grid, gabriel, two, one = TABLE[kind]
    return sorted({1, 2, 16, 63, 64, 65, 255, 256, 257, 512, 513, 1024, tile, tile + 1, grid, grid + 1, gabriel,
                   gabriel + 1, two - 1, two, one - 1, one})


SRC = r'''
#include <stdio.h>
#include "ensemble.cuh"
MAKE_PT(W6, a, b, c);
MAKE_PT(W8, a, b, c, d, e);
MAKE_PT(W9, a, b, c, d, e, f);
MAKE_PT(W11, a, b, c, d, e, f, g, h);
MAKE_PT(W16, a, b, c, d, e, f, g, h, k, l, m, n, o);
using ya::ens::Lds_layout;
template<typename Pt, bool KEYS>
void print(const int n_max)
{
    for (const int lanes : {1, 4, 16, 64}) {
        const Lds_layout l = ya::ens::lds_layout<Pt, KEYS, false>(n_max, 0, lanes);
        printf("%d %zu %d %d %d : %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %zu\n", ya::N_floats<Pt>::value, sizeof(Pt),
            (int)KEYS, n_max, lanes, l.X, l.X1, l.dX, l.dX1, l.old_v, l.fold, l.partials, l.keys, l.list, l.terms, l.tile,
            l.bytes);
    }
}
template<typename Pt>
void type(int argc, char** argv)
{
    for (int a = 1; a < argc; a++) {
        const int n = atoi(argv[a]);
        print<Pt, false>(n), print<Pt, true>(n);
        const ya::ens::Gabriel_lds_layout g = ya::ens::gabriel_lds_layout<Pt>(n);
        printf("gabriel %d %d : %zu %zu %zu %d %zu\n", ya::N_floats<Pt>::value, n, g.lists, g.dense_flags, g.dense,
            g.dense_sets, g.bytes);
    }
    printf("capacities %d : %d %d %d\n", ya::N_floats<Pt>::value, ya::ens::whole_step_capacity<Pt>(),
        ya::ens::grid_lds_capacity<Pt>(), ya::ens::gabriel_lds_capacity<Pt>());
}
int main(int argc, char** argv)
{
    const int floats = atoi(argv[1]);
    argc--, argv++;
    if (floats == 4) type<float4>(argc, argv);
    if (floats == 6) type<W6>(argc, argv);
    if (floats == 8) type<W8>(argc, argv);
    if (floats == 9) type<W9>(argc, argv);
    if (floats == 11) type<W11>(argc, argv);
    if (floats == 16) type<W16>(argc, argv);
    return 0;
}
'''


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ensemble_widths_layout")
    src, exe = tmp / "layout.hip", tmp / "layout"
    src.write_text(SRC)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1",
                    "-DYALLA_NO_THRUST", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    return str(exe)


@pytest.mark.parametrize("kind", KINDS)
def test_the_layouts_are_the_restatements_line_for_line(program, kind):
    floats, sizeof = TABLE[kind][:2]
    assert floats == ws.WIDTH[kind] and sizeof == 4 * floats == ew.SIZEOF[kind]
    ns = sizes(kind)
    printed = subprocess.run([program, str(floats)] + [str(n) for n in ns], check=True, capture_output=True,
                             text=True).stdout.splitlines()
    want = []
    for n in ns:
        for keys in (False, True):
            for lanes in LANES:
                want.append("%d %d %d %d %d : 0 " % (floats, sizeof, keys, n, lanes)
                            + " ".join(str(x) for x in lds_layout(floats, n, keys, None, lanes)))
        want.append("gabriel %d %d : " % (floats, n) + " ".join(str(x) for x in gabriel_lds_layout(floats, n)))
    want.append("capacities %d : %d %d %d" % ((floats,) + TABLE[kind][2:5]))
    assert len(printed) == len(want)
    for got, line in zip(printed, want):
        assert got == line


@pytest.mark.parametrize("kind", KINDS)
def test_the_capacities_are_the_table_s(kind):
    """The restated rules give the table: the rows fit up to each capacity and not one beyond (or 1024 is the ceiling),
    within a few hundred bytes of the workgroup's 160 KiB where the LDS and not the ceiling decides."""
    floats, _, tile, grid, gabriel, two, one = TABLE[kind]
    assert ew.CAPACITY[kind] == TABLE[kind][2:]
    assert (capacity(floats), grid_capacity(floats)) == (tile, grid)
    fits = [n for n in range(1, 1026) if n <= 1024 and gabriel_lds_layout(floats, n)[4] > 0]
    assert fits == list(range(1, gabriel + 1))
    sets = [gabriel_lds_layout(floats, n)[3] for n in range(0, gabriel + 1)]
    assert set(sets[1:65]) == {0} and set(sets[65:two]) == {4} and set(sets[two:one]) == {2}
    assert set(sets[one:]) == {1}
    for keys, rows in ((False, tile), (True, grid)):
        used = lds_layout(floats, rows, keys).bytes + STATIC_LDS
        assert used <= LDS
        if rows < 1024:
            assert lds_layout(floats, rows + 1, keys).bytes + STATIC_LDS > LDS
            assert LDS - used < (1024 if kind != "w16" or not keys else 4096)
    assert gabriel_lds_layout(floats, gabriel)[4] + STATIC_LDS <= LDS


def test_w16_s_grid_capacity_is_where_the_keys_double():
    a, b = lds_layout(16, 512, True), lds_layout(16, 513, True)
    assert a.bytes - a.keys == 8 * 512 and b.bytes - b.keys == 8 * 1024
    assert a.bytes + STATIC_LDS <= LDS < b.bytes + STATIC_LDS
    assert lds_layout(16, 513, False).bytes + STATIC_LDS <= LDS     # (the rows alone would fit)


# ---- which several-lane launches have room ---------------------------------------------------------------------------
def test_a_partner_s_terms_by_type_and_lanes():
    """(256 / lanes) cells x (floats + 4) components x 4 bytes: 16 floats and 4 lanes cost 5120 bytes per partner, so
    the shortest tile of 16 partners is 80 KiB."""
    assert tile_behind(0, 16, 100, 4)[0] == 5120 and 16 * 5120 == 80 * 1024
    assert tile_behind(0, 11, 100, 4)[0] == 3840
    assert tile_behind(0, 16, 100, 64)[0] == 320


def first_without_room(form, kind, lanes):
    """The smallest n_max within the capacity whose launch of `lanes` lanes has no room (None: all have), and that room
    never comes back beyond it."""
    top = ew.capacity_of(form, kind)
    room = [ew.has_room(form, kind, n, lanes) for n in range(1, top + 1)]
    if all(room):
        return None
    first = room.index(False) + 1
    assert not any(room[first - 1:])
    return first


# form, type -> the first n_max without room for 4 / 16 / 64 lanes, worked out from the restated rule: e.g. all-pairs
# w16 with 4 lanes needs 81920 bytes behind rows that end at 268 n + 16640 (rounded up to 16): n <= 232
ROOM_EDGES = {
    ("tile", "float4"): (None, None, None), ("tile", "w6"): (None, None, None),
    ("tile", "w11"): (468, 713, 774), ("tile", "w16"): (233, 462, 519),
    ("grid", "float4"): (None, None, None), ("grid", "w6"): (976, None, None), ("grid", "w8"): (680, 943, 1009),
    ("grid", "w9"): (577, 833, 897), ("grid", "w11"): (446, 670, 731), ("grid", "w16"): (225, 447, 504),
}


@pytest.mark.parametrize("form,kind", list(ROOM_EDGES))
def test_where_the_term_buffer_stops_fitting(form, kind):
    got = tuple(first_without_room(form, kind, lanes) for lanes in (4, 16, 64))
    assert got == ROOM_EDGES[(form, kind)], (form, kind, got)
    for lanes, edge in zip((4, 16, 64), got):
        if edge is not None:
            floats = ws.WIDTH[kind]
            base = lds_layout(floats, edge, ew.KEYS[form]).terms
            per_partner = (256 // lanes) * (floats + 4) * 4
            assert base + STATIC_LDS + 16 * per_partner > LDS
            assert lds_layout(floats, edge - 1, ew.KEYS[form]).terms + STATIC_LDS + 16 * per_partner <= LDS


def test_the_shapes_of_the_gpu_tests():
    """What tests/test_ensemble_widths_gpu.py takes for granted."""
    import test_ensemble_widths_gpu as gpu
    for kind, (with_room, without) in gpu.TILE_ROOM.items():
        assert ew.has_room("tile", kind, *with_room) and not ew.has_room("tile", kind, *without)
        assert without[0] <= ew.capacity_of("tile", kind)
    # an 8-float point's 1024 rows and keys: no term buffer at any lane count; 16 floats at 512 neither
    assert not any(ew.has_room("grid", "w8", 1024, lanes) for lanes in (4, 16, 64))
    assert not any(ew.has_room("grid", "w16", 512, lanes) for lanes in (4, 16, 64))
    # the small mix has room for every lane count in every type; the large one has none for w16's 4 lanes
    for form in ("tile", "grid"):
        for kind in ew.TYPES[form]:
            assert all(ew.has_room(form, kind, gpu.SMALL_N_MAX, lanes) for lanes in (4, 16, 64)), (form, kind)
            assert ew.has_room(form, kind, gpu.LARGE_N_MAX, 4) == (kind != "w16"), (form, kind)
            assert all(ew.has_room(form, kind, gpu.LARGE_N_MAX, lanes) for lanes in (16, 64)), (form, kind)


# ---- the libraries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(ew.FORMS))
def test_the_library_exports_its_header_and_lists_its_rows(form):
    path, header, prefix, table, _, suffix = ew.FORMS[form]
    names = declared_functions(header)
    assert set(names) == set(getattr(_ffi, table))
    functions = {sym for kind, sym in exported(path) if kind == "T" and sym.startswith("ya_")}
    assert functions == set(names), "library and header disagree"
    check_only_the_c_abi_is_exported(path, prefix)
    lib = ew.lib_of(form)       # types every entry point; AttributeError if one is missing
    assert ew.models_of(form) == [ew.model(kind) for kind in ew.TYPES[form]]
    check_models_name_bounds(getattr(lib, prefix + "models_name"), len(ew.TYPES[form]))
    from yalla_amd.solution import models
    lone = models(_ffi.bind(ws.WIDTHS_DEVICE_LIB))
    for kind in ew.TYPES[form]:
        assert ew.model(kind) + suffix in lone, "every row has its lone model"


def test_the_shipped_libraries_keep_their_tables():
    from yalla_amd.ensemble import gabriel_lds_models, grid_models, models
    for listed in (models(), grid_models(), gabriel_lds_models()):
        assert "relu_po" in listed and not any(name.startswith("fields_") for name in listed)


def test_the_types_are_written_once():
    """ensemble_widths_models.h declares no point type and no YA_STATELESS line of its own: widths_models.h's."""
    text = open(os.path.join(ROOT, "yalla_amd", "csrc", "ensemble_widths_models.h")).read()
    assert "MAKE_PT(" not in text and "YA_STATELESS(" not in text
    for source in ("ensemble.hip", "ensemble_grid.hip", "ensemble_gabriel_lds.hip"):
        assert '"fields_' not in open(os.path.join(ROOT, "yalla_amd", "csrc", source)).read()


# ---- the start states and the premise --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_start_states_extra_fields(kind):
    X = ew.rows_of(kind, 300, 3)
    extras = X[:, 3:]
    assert X.dtype == np.float32 and np.array_equal(extras, ws.extra_fields(300, ws.WIDTH[kind]))
    scaled = extras.astype(np.float64) * 2 ** 13
    assert (scaled == np.round(scaled)).all() and (np.round(scaled).astype(np.int64) % 2 == 1).all()   # odd multiples
    assert (extras != 0).all() and (np.abs(extras) < 1).all()
    for a in range(extras.shape[1]):
        for b in range(a + 1, extras.shape[1]):
            assert not np.array_equal(extras[:, a], extras[:, b])


@pytest.mark.parametrize("form,kind", [(form, kind) for form in ew.FORMS for kind in ew.TYPES[form]])
def test_the_oracle_moves_every_extra_field_of_every_cell_with_a_neighbour(form, kind):
    """One Heun step of replicas of 2, 65, 257 and 5 rows (start states of the GPU tests), each on its own: every
    extra field of every cell that has a neighbour within 1 changes its bits, and none of a cell without one (a cell's
    nearest neighbour is a Gabriel neighbour too)."""
    lib = ew.oracle_lib()
    suffix = ew.FORMS[form][5]
    for n, seed in ((2, 1), (65, 2), (257, 3), (5, 903)):
        X = ew.rows_of(kind, n, seed)
        if n == 2:
            X[1, :3] = X[0, :3] + np.float32(0.5)      # (a pair within 1)
        with Solution(ew.model(kind) + suffix, n, 30, 1.0, lib=lib) as s:
            assert s.set_reduce_order(1) == 0
            s.h_X[:n] = X
            s.h_n = n
            s.copy_to_device()
            s.take_step(0.05, 1)
            after = s.positions()
        near = ew.with_neighbour(X)
        changed = ws.bits(after[:, 3:]) != ws.bits(X[:, 3:])
        assert near.sum() >= min(n, 60) or n == 5
        if n != 5:
            assert changed[near].all(), (form, kind, n)
        if form != "gabriel":
            # what the GPU tests assert: the fields whose exact right-hand side is not zero.  In five cells a cell in
            # the middle of its neighbours' values has a zero one, which is why they do not ask every cell.
            must = ew.must_move(X, 0.05)
            assert changed[must].all() and must.any(axis=0).all() and (n != 5 or not must[near].all())
        alone = ~ew.with_neighbour(X, 1 + 1e-5)      # (no pair at all: no force in any extra field)
        assert not changed[alone].any()
