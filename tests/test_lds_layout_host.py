"""The LDS layout of the launches that step a replica from LDS (ya::ens::lds_layout, include/ensemble.cuh) is pure
arithmetic: host plans and kernels read the same function.  Compiled here into a stand-alone host program (no device, no
HIP runtime call) that prints the layout for point types of 3, 4, 5, 7 and 8 floats, with and without keys, n_max =
1 .. 1024, lanes 1, 4, 16, 64 and seven link settings -- and, without links, for points of 6, 9, 11 and 16 floats
(sizeof 24, 36, 44, 64: from 9 floats on fewer than 1024 rows fit, so the sweep crosses each type's capacity and runs
to 1025) --, and held line for line to the Python restatement
(ensemble_support.lds_layout, written from the function's comment) and to a table worked out by hand:

    step's arrays   X1 .. old_v at 1 .. 4 x n_max x 4 NF, fold at n_max (16 NF + 12), partials 1024 NF further, 16 NF more
    keys            rounded up to 8; 8 bytes per row of the power of two from n_max up
    list            all-pairs: rounded up to 16, and so is its end; grid: right behind the keys, end not rounded;
                    4 (n_max + 1) + 8 slots bytes; no room where end + 3072 > 163840
    term buffer     rounded up to 16; (256 / lanes) (NF + 4) 4 bytes per partner; tile = min(n_max up to 4, 256,
                    max(32768 / per partner down to 4, 16), (163840 - 3072 - start) / per partner down to 4); no room
                    where 16 partners do not fit
"""
import os
import subprocess

import pytest
from ensemble_support import Layout, capacity, grid_capacity, largest_slots, lds_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include "ensemble.cuh"
MAKE_PT(Pt7, a, b, c, d);
MAKE_PT(Pt8, a, b, c, d, e);
MAKE_PT(Pt6, a, b, c);
MAKE_PT(Pt9, a, b, c, d, e, f);
MAKE_PT(Pt11, a, b, c, d, e, f, g, h);
MAKE_PT(Pt16, a, b, c, d, e, f, g, h, k, l, m, n, o);
static_assert(sizeof(Pt6) == 24 && sizeof(Pt9) == 36 && sizeof(Pt11) == 44 && sizeof(Pt16) == 64, "no padding");
using ya::ens::Lds_layout;
using ya::ens::lds_layout;
template<typename Pt, bool KEYS, bool LINKED>
void print(const int n_max, const int slots)
{
    for (const int lanes : {1, 4, 16, 64}) {
        const Lds_layout l = lds_layout<Pt, KEYS, LINKED>(n_max, slots, lanes);
        printf("%d %d %d %d %d : %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %zu\n", ya::N_floats<Pt>::value, (int)KEYS, n_max,
            LINKED ? slots : -1, lanes, l.X, l.X1, l.dX, l.dX1, l.old_v, l.fold, l.partials, l.keys, l.list, l.terms, l.tile,
            l.bytes);
    }
}
template<typename Pt, bool KEYS>
void sweep()
{
    for (int n = 1; n <= 1024; n++) {
        print<Pt, KEYS, false>(n, 0);
        print<Pt, KEYS, true>(n, 0);
        print<Pt, KEYS, true>(n, n);
        print<Pt, KEYS, true>(n, 3 * n);
        if (lds_layout<Pt, KEYS, true>(n, 0, 1).bytes != 0) {  // the largest slot count that fits, and one more
            int fits = 0, too_many = 160 * 1024;
            while (too_many - fits > 1) {
                const int mid = (fits + too_many) / 2;
                (lds_layout<Pt, KEYS, true>(n, mid, 1).bytes != 0 ? fits : too_many) = mid;
            }
            print<Pt, KEYS, true>(n, fits);
            print<Pt, KEYS, true>(n, fits + 1);
        }
        print<Pt, KEYS, true>(n, 20000);
    }
}
// the wide types: without links, across the capacities (the rule itself does not stop there) and one row past 1024
template<typename Pt>
void wide()
{
    for (int n = 1; n <= 1025; n++) print<Pt, false, false>(n, 0), print<Pt, true, false>(n, 0);
    printf("capacities of %d floats: %d %d\n", ya::N_floats<Pt>::value, ya::ens::whole_step_capacity<Pt>(),
        ya::ens::grid_lds_capacity<Pt>());
}
int main()
{
    sweep<float3, false>(), sweep<float3, true>(), sweep<float4, false>(), sweep<float4, true>();
    sweep<Po_cell, false>(), sweep<Po_cell, true>(), sweep<Pt7, false>(), sweep<Pt7, true>();
    sweep<Pt8, false>(), sweep<Pt8, true>();
    printf("capacities %d %d %d %d\n", ya::ens::whole_step_capacity<float3>(), ya::ens::whole_step_capacity<Pt8>(),
        ya::ens::grid_lds_capacity<float3>(), ya::ens::grid_lds_capacity<Pt8>());
    wide<Pt6>(), wide<Pt9>(), wide<Pt11>(), wide<Pt16>();
    return 0;
}
'''

LANES = (1, 4, 16, 64)
WIDE = (6, 9, 11, 16)
# (all-pairs, grid) rows that fit one workgroup, worked out by hand from the formulas in this file's header: e.g. 16
# floats: (163840 - 3072 - 16640) / 268 = 537.8; with keys 512 rows end at 137216 + 16640 + 4096 = 157952, 513 rows lay
# out 1024 keys and end at 162320 > 160768
WIDE_CAPACITIES = {6: (1024, 1024), 9: (970, 918), 11: (794, 750), 16: (537, 512)}


def restated():
    """The program's lines from the Python restatement, in the program's order."""
    lines = []
    for n_floats in (3, 4, 5, 7, 8):
        for keys in (False, True):
            for n in range(1, 1025):
                settings = [None, 0, n, 3 * n]
                fits = largest_slots(n_floats, n, keys=keys)
                if fits is not None:
                    settings += [fits, fits + 1]
                for slots in settings + [20000]:
                    for lanes in LANES:
                        layout = lds_layout(n_floats, n, keys, slots, lanes)
                        lines.append("%d %d %d %d %d : 0 " % (n_floats, keys, n, -1 if slots is None else slots, lanes)
                                     + " ".join(str(x) for x in layout))
    return lines


def restated_wide():
    lines = []
    for n_floats in WIDE:
        for n in range(1, 1026):
            for keys in (False, True):
                for lanes in LANES:
                    layout = lds_layout(n_floats, n, keys, None, lanes)
                    lines.append("%d %d %d -1 %d : 0 " % (n_floats, keys, n, lanes) + " ".join(str(x) for x in layout))
        lines.append("capacities of %d floats: %d %d" % (n_floats, capacity(n_floats), grid_capacity(n_floats)))
    return lines


# (floats, keys, n_max, slots or None, lanes) -> the layout, by hand from the formulas in this file's header
TABLE = [
    # an 8-float point's 1024 rows and keys leave 163840 - 3072 - 159872 = 896 bytes
    ((8, True, 1024, None, 1), Layout(32768, 65536, 98304, 131072, 143360, 151552, 151680, 0, 159872, 0, 159872)),
    # ... which hold no list of 1025 offsets, and no 16 partners' terms at any lane count
    ((8, True, 1024, 0, 1), Layout(32768, 65536, 98304, 131072, 143360, 151552, 151680, 159872, 163984, 0, 0)),
    ((8, True, 1024, None, 64), Layout(32768, 65536, 98304, 131072, 143360, 151552, 151680, 0, 159872, 0, 0)),
    # a 7-float point's 1024 rows and keys leave 18320: 16 partners of 4 lanes cost 45056, 16 lanes fit 24, 64 lanes 104
    ((7, True, 1024, None, 4), Layout(28672, 57344, 86016, 114688, 126976, 134144, 134256, 0, 142448, 0, 0)),
    ((7, True, 1024, None, 16), Layout(28672, 57344, 86016, 114688, 126976, 134144, 134256, 0, 142448, 24, 159344)),
    ((7, True, 1024, None, 64), Layout(28672, 57344, 86016, 114688, 126976, 134144, 134256, 0, 142448, 104, 160752)),
    # the shortest tile: an 8-float point's 942 rows leave 12368 bytes behind 148400, 16 partners of 16 lanes cost 12288
    ((8, True, 942, None, 16), Layout(30144, 60288, 90432, 120576, 131880, 140072, 140200, 0, 148400, 16, 160688)),
    # an all-pairs linked launch of one lane: the list starts at 3420 rounded up, its end 3448 is rounded up too ...
    ((3, False, 5, 0, 1), Layout(60, 120, 180, 240, 300, 3372, 0, 3424, 3456, 0, 3456)),
    # ... the grid's list starts right behind 8 keys and its end stays
    ((3, True, 5, 0, 1), Layout(60, 120, 180, 240, 300, 3372, 3424, 3488, 3520, 0, 3512)),
    # small replicas: the tile is n_max rounded up to 4; 4 lanes' budget is 32768 / 1792 = 18 down to 16
    ((3, False, 5, None, 64), Layout(60, 120, 180, 240, 300, 3372, 0, 0, 3424, 8, 3424 + 8 * 112)),
    ((3, False, 300, None, 4), Layout(3600, 7200, 10800, 14400, 18000, 21072, 0, 0, 21120, 16, 21120 + 16 * 1792)),
    # a 16-float point's 512 rows and 512 keys end at 157952: 2816 bytes left beside the fold scratch, no term buffer
    ((16, True, 512, None, 1), Layout(32768, 65536, 98304, 131072, 137216, 153600, 153856, 0, 157952, 0, 157952)),
    ((16, True, 512, None, 64), Layout(32768, 65536, 98304, 131072, 137216, 153600, 153856, 0, 157952, 0, 0)),
    # ... 16 floats and 4 lanes: 64 cells x 20 floats = 5120 bytes per partner, 16 partners 80 KiB; 200 rows end at 70240
    # and leave 90528: room 17 down to 16; 250 rows end at 83640, the buffer would start at 83648 and have 77120 < 81920: no room
    ((16, False, 200, None, 4), Layout(12800, 25600, 38400, 51200, 53600, 69984, 0, 0, 70240, 16, 70240 + 16 * 5120)),
    ((16, False, 250, None, 4), Layout(16000, 32000, 48000, 64000, 67000, 83384, 0, 0, 83648, 0, 0)),
]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lds_layout")
    src, exe = tmp / "layout.hip", tmp / "layout"
    src.write_text(SRC)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1",
                    "-DYALLA_NO_THRUST", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


def test_the_layout_is_the_restatement_line_for_line(printed):
    want = restated()
    wide = restated_wide()
    assert len(printed) == len(want) + 1 + len(wide)
    for got, line in zip(printed, want):
        assert got == line
    assert printed[len(want)] == "capacities 1024 1024 1024 1024"
    for got, line in zip(printed[len(want) + 1:], wide):
        assert got == line


def test_the_wide_types_capacities():
    """The restatement's capacities are the hand-worked ones, the rows fit up to them and not beyond (beside the static
    fold scratch), and 1024 is the ceiling whatever fits."""
    from ensemble_support import LDS, STATIC_LDS
    for n_floats, (tile, grid) in WIDE_CAPACITIES.items():
        assert (capacity(n_floats), grid_capacity(n_floats)) == (tile, grid), n_floats
        for keys, rows in ((False, tile), (True, grid)):
            assert lds_layout(n_floats, rows, keys).bytes + STATIC_LDS <= LDS
            assert rows == 1024 or lds_layout(n_floats, rows + 1, keys).bytes + STATIC_LDS > LDS


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_the_layout_matches_the_table_worked_out_by_hand(printed, row):
    (n_floats, keys, n_max, slots, lanes), layout = TABLE[row]
    head = "%d %d %d %d %d : 0 " % (n_floats, keys, n_max, -1 if slots is None else slots, lanes)
    assert head + " ".join(str(x) for x in layout) in printed
    assert lds_layout(n_floats, n_max, keys, slots, lanes) == layout
