"""The launch plan of grid_force_bits (ya::bits::plan, include/solvers.cuh) is pure arithmetic: Grid_computer::forces
launches by it and Grid_computer::ready_to_capture asks the same function, so the two cannot disagree.  Compiled here
into a stand-alone host program (no device, no HIP runtime call) and held to a table worked out by hand from the
formulas:

    tiles   = ceil(n / 64)
    tail    = 0 unless summing by plane with stateless functors; force_tail_tiles t >= 0: -1 if t >= tiles else t;
              else -1 if 2 tiles <= resident; else (part 0 and tiles <= resident) ? resident - tiles : 768
    room    = tail < 0 ? tiles : tail
    blocks  = tail < 0 ? 16 * ((tiles + 7) / 8) : tiles + (tail > 0 ? min(tail, tiles) + 24 : 0)
    stage_v = n <= stage_v_max and tail >= 0
    off32   = gather_offset_bits != 64 and 16 n < 2^32      (ya::bits::offsets_fit_32_bits: flips at n = 2^28)
    ready to capture  <=>  room <= tail_room
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include "solvers.cuh"
// argv: groups of 8 ints: n part resident by_plane stateless tail_tiles stage_v_max gather_offset_bits
int main(int argc, char** argv)
{
    for (int a = 1; a + 8 <= argc; a += 8) {
        int v[8];
        for (int k = 0; k < 8; k++) v[k] = atoi(argv[a + k]);
        const ya::bits::Plan_settings s{v[3] != 0, v[4] != 0, v[5], v[6], v[7]};
        const ya::bits::Plan p = ya::bits::plan(v[0], v[1], v[2], s);
        printf("%d %d %d %d %d %d %d %d %d\n", p.tiles, p.tail, p.room, p.blocks, (int)p.stage_v, (int)p.off32,
            (int)p.fits(p.room), (int)p.fits(p.room + 1000), (int)p.fits(p.room - 1));
    }
    return 0;
}
'''

R = 5120         # resident one-wavefront workgroups (springs on an MI355X)
SV = 130000      # Grid_computer::stage_v_max's default
FLIP = 1 << 28   # the first n with 16 n >= 2^32

# (n, part, resident, by_plane, stateless, force_tail_tiles, stage_v_max, gather_offset_bits)
#     -> (tiles, tail, room, blocks, stage_v, off32)
TABLE = [
    # by plane, stateless, the engine's choice of the tail
    ((64 * 1, 0, R, 1, 1, -1, SV, 0), (1, -1, 1, 16, 0, 1)),            # stage_v is false whenever tail < 0
    ((64 * 2560, 0, R, 1, 1, -1, SV, 0), (2560, -1, 2560, 5120, 0, 1)),
    ((64 * 2561, 0, R, 1, 1, -1, SV, 0), (2561, 2559, 2559, 5144, 0, 1)),
    ((64 * 5120, 0, R, 1, 1, -1, SV, 0), (5120, 0, 0, 5120, 0, 1)),
    ((64 * 5121, 0, R, 1, 1, -1, SV, 0), (5121, 768, 768, 5913, 0, 1)),
    ((64 * 2560, 1, R, 1, 1, -1, SV, 0), (2560, -1, 2560, 5120, 0, 1)),   # a slab stage's parts
    ((64 * 2561, 1, R, 1, 1, -1, SV, 0), (2561, 768, 768, 3353, 0, 1)),
    ((64 * 2561, 2, R, 1, 1, -1, SV, 0), (2561, 768, 768, 3353, 0, 1)),
    ((64 * 2560 - 63, 0, R, 1, 1, -1, SV, 0), (2560, -1, 2560, 5120, 0, 1)),  # a last tile of one cell
    # force_tail_tiles = 3 (the occupancy is not asked for: resident 0)
    ((64 * 3, 0, 0, 1, 1, 3, SV, 0), (3, -1, 3, 16, 0, 1)),
    ((64 * 4, 0, 0, 1, 1, 3, SV, 0), (4, 3, 3, 31, 1, 1)),
    ((64 * 4, 0, 0, 1, 1, 0, SV, 0), (4, 0, 0, 4, 1, 1)),
    # the reference order, or functors with state: no tail at any size
    ((64 * 1, 0, 0, 0, 1, -1, SV, 0), (1, 0, 0, 1, 1, 1)),
    ((64 * 2561, 0, 0, 0, 1, -1, SV, 0), (2561, 0, 0, 2561, 0, 1)),
    ((64 * 5121, 0, 0, 0, 1, 3, SV, 0), (5121, 0, 0, 5121, 0, 1)),
    ((64 * 2561, 0, 0, 1, 0, -1, SV, 0), (2561, 0, 0, 2561, 0, 1)),
    # stage_v at its threshold
    ((SV, 0, 0, 0, 1, -1, SV, 0), (2032, 0, 0, 2032, 1, 1)),
    ((SV + 1, 0, 0, 0, 1, -1, SV, 0), (2032, 0, 0, 2032, 0, 1)),
    ((1000, 0, 0, 0, 1, -1, 999, 0), (16, 0, 0, 16, 0, 1)),
    # off32: the 64-bit form on request, and by n
    ((64 * 1, 0, 0, 0, 1, -1, SV, 64), (1, 0, 0, 1, 1, 0)),
    ((FLIP - 1, 0, 0, 0, 1, -1, SV, 0), (4194304, 0, 0, 4194304, 0, 1)),
    ((FLIP, 0, 0, 0, 1, -1, SV, 0), (4194304, 0, 0, 4194304, 0, 0)),
]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("force_plan")
    src, exe = tmp / "plan.hip", tmp / "plan"
    src.write_text(SRC)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1",
                    "-DYALLA_NO_THRUST", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    args = [str(x) for inputs, _ in TABLE for x in inputs]
    out = subprocess.run([str(exe), *args], check=True, capture_output=True, text=True).stdout
    rows = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    assert len(rows) == len(TABLE)
    return rows


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_plan_matches_the_formulas(plans, row):
    inputs, expected = TABLE[row]
    assert plans[row][:6] == expected, inputs


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_ready_to_capture_exactly_when_the_room_is_there(plans, row):
    fits_room, fits_more, fits_one_less = plans[row][6:]
    assert fits_room == 1 and fits_more == 1
    assert fits_one_less == 0
