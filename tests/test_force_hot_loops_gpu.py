"""The hot loops of ya::grid_force_bits (include/solvers.cuh, ya::bits::pass) on cells placed by hand where the
loops' bookkeeping can go wrong: candidate segments that end on, just before and just after a word of the bit
stream, hits in a word's last and first bit, words with exactly one hit, passes that overflow into the per-row
fallback, staging in chunks, and pairs so close that the square root and the reciprocal take their library paths.

Every case runs two steps of springs_grid in the oracle (tree reduction order) and on the device from the same
h_X, and compares positions, old_v and the four grid arrays bit for bit -- in both summation orders and with
force_variant 2 (no cooperative kernel), with old_v read from LDS, gathered through 32-bit byte offsets, and
gathered through 64-bit addresses (the form systems of 2^28 cells and more get).

`bit_streams` restates on the host which candidate gets which bit of which lane's stream; the non-GPU tests use
it to check that the shapes named above really occur in the cases, so that a change of the generator cannot
quietly stop testing them.
"""
import os
import subprocess

import numpy as np
import pytest

from yalla_amd.solution import Solution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GS = 8            # grid size: cubes -4 .. 3 per axis, cube size 1
CAP = 352         # staged cells per chunk (ya::bits::Stage, 16-byte entries)
PASS_BITS = 128   # candidate bits per lane and pass (32 * YA_MASK_WORDS)
TILE = 64         # cells per workgroup
DT = 0.001
STEPS = 2


# ---- the cases ---------------------------------------------------------------------------------------------------

def fill_cubes(rng, counts):
    """counts[z, y, x] cells placed uniformly inside cube (x, y, z) - 3 of the 6 x 6 x 6 interior cubes, a margin of
    2^-10 away from the faces (a cell's cube is then the same in any rounding)."""
    X = []
    for z, y, x in np.ndindex(counts.shape):
        k = counts[z, y, x]
        lo = np.array([x, y, z], dtype=np.float64) - 3.0
        X.append(lo + 2.0 ** -10 + rng.random((k, 3)) * (1.0 - 2.0 ** -9))
    X = np.concatenate(X).astype(np.float32)
    return X[rng.permutation(len(X))]  # ids unrelated to cubes


def boundaries_case():
    """Per-cube counts 0 .. 21, a third of the cubes nearly empty: a lane's row (three cubes along x) has 0 .. 45
    candidates and more, its three padded segments end all over the words of a pass."""
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 22, size=(6, 6, 6))
    sparse = rng.random((6, 6, 6)) < 0.3
    counts[sparse] = rng.integers(0, 4, size=(6, 6, 6))[sparse]
    X = fill_cubes(rng, counts)
    if len(X) % TILE == 0:
        X = X[:-1]
    return X


def overflow_case():
    """A 2 x 2 x 2 block of cubes with 50 .. 130 cells each in a sparse background: lanes with more than 128
    candidate bits per plane (one pass per row stretch), planes of more than 352 staged cells (chunks)."""
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 7, size=(6, 6, 6))
    counts[2:4, 2:4, 2:4] = rng.integers(50, 131, size=(2, 2, 2))
    X = fill_cubes(rng, counts)
    if len(X) % TILE == 0:
        X = X[:-1]
    return X


CLOSE_PAIRS = [  # (first cell, separation along x): three pairs of distinct cells next to the origin
    ((0.0, 0.0, 0.0), 2.0 ** -49),
    ((0.0, 2.0 ** -20, 0.0), 2.0 ** -50),
    ((0.0, 0.0, 2.0 ** -20), 2.0 ** -65),
]


def close_pairs_case():
    """Pairs at separations 2^-49, 2^-50 and 2^-65 (squared distance below 2^-96: the scaled branch of
    ya::exact_sqrt; distance below 2^-64: the library branch of ya::reciprocal) among ordinary neighbours."""
    rng = np.random.default_rng(3)
    X = fill_cubes(rng, rng.integers(6, 13, size=(6, 6, 6)))
    pairs = []
    for (x, y, z), sep in CLOSE_PAIRS:
        pairs += [(x, y, z), (x + sep, y, z)]
    pairs = np.array(pairs, dtype=np.float32)
    assert len(np.unique(pairs, axis=0)) == len(pairs)  # distinct in binary32: no coincident cells
    at = rng.choice(len(X), size=len(pairs), replace=False)
    X[at] = pairs  # somewhere among the ids
    if len(X) % TILE == 0:
        X = X[:-1]
    return X


CASES = {"boundaries": boundaries_case, "overflow": overflow_case, "close_pairs": close_pairs_case}


# ---- which candidate gets which bit: the kernel's layout restated ------------------------------------------------

def pad4(k):
    return (max(k, 0) + 3) & ~3


def bit_streams(X):
    """For every lane (cell) and plane of the first force evaluation: a list of passes, each
    (segment lengths [3], hit flags per bit of the padded stream).  Cells sorted by (cube, id) as Grid::build
    does; staging, chunks and the per-row fallback as grid_force_bits_tile lays them out."""
    n = len(X)
    cube = (np.floor(X[:, 0]) + GS // 2 + (np.floor(X[:, 1]) + GS // 2) * GS
            + (np.floor(X[:, 2]) + GS // 2) * GS * GS).astype(np.int64)
    order = np.lexsort((np.arange(n), cube))
    cube_sorted, Xs = cube[order], X[order].astype(np.float64)
    n_cubes = GS ** 3
    offs = np.searchsorted(cube_sorted, np.arange(n_cubes + 1))

    def off_at(c):
        return int(offs[min(max(c, 0), n_cubes)])

    lanes = []
    for s0 in range(0, n, TILE):
        tile = range(s0, min(s0 + TILE, n))
        c_lo, c_hi = int(cube_sorted[tile[0]]), int(cube_sorted[tile[-1]])
        for dz in (0, -GS * GS, GS * GS):
            rows = [dz + dy for dy in (0, -GS, GS)]
            wg_begin = [off_at(c_lo + o - 1) for o in rows]
            wg_end = [off_at(c_hi + o + 2) for o in rows]
            v0 = np.concatenate(([0], np.cumsum([e - b for b, e in zip(wg_begin, wg_end)])))
            total = int(v0[3])
            for chunk in range(0, total, CAP):
                chunk_n = min(CAP, total - chunk)
                segments = {}  # lane -> its three (begin, end, shift to sorted slots), clipped to the chunk
                for s in tile:
                    c = int(cube_sorted[s])
                    segments[s] = []
                    for r, o in enumerate(rows):
                        kb, ke = off_at(c + o - 1), off_at(c + o + 2)
                        sb = max(kb - wg_begin[r] + int(v0[r]), chunk) - chunk
                        se = min(ke - wg_begin[r] + int(v0[r]), chunk + chunk_n) - chunk
                        segments[s].append((sb, se, wg_begin[r] - int(v0[r]) + chunk))
                # one pass per lane, unless some lane of the wavefront needs more than PASS_BITS bits
                fallback = any(sum(pad4(se - sb) for sb, se, _ in segments[s]) > PASS_BITS for s in tile)
                for s in tile:
                    passes = []
                    if not fallback:
                        passes.append(segments[s])
                    else:
                        for sb, se, shift in segments[s]:
                            for b in range(sb, max(se, sb), PASS_BITS):
                                passes.append([(b, min(se, b + PASS_BITS), shift), (0, 0, 0), (0, 0, 0)])
                    for p in passes:
                        bits, lengths = [], []
                        for sb, se, shift in p:
                            k = max(se - sb, 0)
                            lengths.append(k)
                            if k:
                                d = Xs[sb + shift:se + shift] - Xs[s]
                                bits += list((d * d).sum(axis=1) < 1.0)
                            bits += [False] * (pad4(k) - k)
                        lanes.append((lengths, np.array(bits, dtype=bool), fallback, total))
    return lanes


def words_of(bits):
    padded = np.concatenate((bits, np.zeros(-len(bits) % 32, dtype=bool)))
    return padded.reshape(-1, 32)


def test_boundaries_case_has_the_shapes_it_is_for():
    X = boundaries_case()
    assert 1700 <= len(X) <= 2400 and len(X) % TILE != 0
    lanes = [lane for lane in bit_streams(X) if not lane[2]]  # the passes of three segments
    assert len(lanes) > 2 * len(X)
    # a lane's row lengths sweep 0 .. 45: around every multiple of 4 (the padding) and around 32
    lengths = {k for seg, _, _, _ in lanes for k in seg}
    assert lengths >= set(range(46))
    # the second and the third segment start exactly on a word, and the segment before them holds its last
    # candidate one bit before a word's end (.. 31), in a word's last bit (.. 32) and in the next word's first (.. 33)
    p1 = {pad4(seg[0]) for seg, _, _, _ in lanes if seg[1] > 0}
    p2 = {pad4(seg[0]) + pad4(seg[1]) for seg, _, _, _ in lanes if seg[2] > 0}
    assert 32 in p1 and {32, 64} <= p2
    ends = {seg[0] % 32 for seg, _, _, _ in lanes if seg[0] >= 31 and seg[1] > 0}
    ends |= {(pad4(seg[0]) + seg[1]) % 32 for seg, _, _, _ in lanes if pad4(seg[0]) + seg[1] >= 31 and seg[2] > 0}
    assert {31, 0, 1} <= ends
    last_then_first = one_then_some = one_then_none = False
    for _, bits, _, _ in lanes:
        w = words_of(bits)
        count = w.sum(axis=1)
        for k in range(len(w) - 1):
            last_then_first |= bool(w[k, 31] and w[k + 1, 0])
            one_then_some |= bool(count[k] == 1 and count[k + 1] > 0)
            one_then_none |= bool(count[k] == 1 and count[k + 1] == 0 and count[k + 2:].sum() > 0)
    assert last_then_first and one_then_some and one_then_none


def test_overflow_case_has_the_shapes_it_is_for():
    X = overflow_case()
    assert len(X) % TILE != 0 and len(X) <= 2600
    lanes = bit_streams(X)
    assert any(fallback and len(bits) == PASS_BITS for _, bits, fallback, _ in lanes)  # a full stretch, and more
    assert any(total > CAP for _, _, _, total in lanes)                                # staging in chunks
    assert any(not fallback for _, _, fallback, _ in lanes)


def test_close_pairs_case_has_the_pairs_it_is_for():
    X = close_pairs_case()
    assert len(np.unique(X, axis=0)) == len(X)
    d = X[:, None, :].astype(np.float64) - X[None, :, :]
    dist = np.sqrt((d * d).sum(axis=2))
    for _, sep in CLOSE_PAIRS:
        assert (dist == sep).sum() == 2  # the pair, seen from both cells
    close = dist[(dist > 0) & (dist < 2.0 ** -40)]
    assert (close ** 2 < 2.0 ** -96).all() and (close < 2.0 ** -64).sum() == 2
    # ordinary neighbours around them: tens of cells within the cut-off of the origin
    assert ((X.astype(np.float64) ** 2).sum(axis=1) < 1.0).sum() > 20


# ---- the offset guard --------------------------------------------------------------------------------------------

GUARD_SRC = r'''
#include <stdio.h>
#include "solvers.cuh"
static_assert(ya::bits::offsets_fit_32_bits(1), "");
static_assert(ya::bits::offsets_fit_32_bits((1 << 28) - 1), "16 (2^28 - 1) < 2^32");
static_assert(!ya::bits::offsets_fit_32_bits(1 << 28), "16 * 2^28 = 2^32 does not fit");
static_assert(!ya::bits::offsets_fit_32_bits(0x7fffffff), "");
int main()
{
    volatile long long n = (1 << 28) - 1;  // (and evaluated at run time, as Grid_computer::forces does)
    const bool below = ya::bits::offsets_fit_32_bits(n), at = ya::bits::offsets_fit_32_bits(n + 1);
    printf("below %d at %d\n", (int)below, (int)at);
    return !(below && !at);
}
'''


def test_gather_offsets_fall_back_to_64_bits_from_2_to_28_cells(tmp_path):
    """The launch choice of Grid_computer::forces through its predicate alone: 32-bit byte offsets while
    16 n < 2^32, the 64-bit form from n = 2^28 on.  Host code only; no system of that size is allocated."""
    src = tmp_path / "guard.hip"
    src.write_text(GUARD_SRC)
    exe = tmp_path / "guard"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-DYALLA_NO_THRUST",
                    "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "below 1 at 0" in out.stdout, out.stdout + out.stderr


# ---- device against oracle ---------------------------------------------------------------------------------------

def two_steps(lib, X, sum_order, setup=None, tree=False):
    n = len(X)
    with Solution("springs_grid", n, GS, 1.0, lib=lib) as s:
        if tree:
            assert s.set_reduce_order(1) == 0
        assert s.set_param("sum_order", sum_order) == 0
        if setup:
            setup(s)
        s.h_X[:n] = X
        s.h_n = n
        s.copy_to_device()
        s.take_step(DT, STEPS)
        return s.positions(), s.old_v()[:n], s.grid()


_expected = {}


def expected(oracle, case, sum_order):
    """The oracle's result of a case, computed once and shared."""
    key = (case, sum_order)
    if key not in _expected:
        _expected[key] = two_steps(oracle, CASES[case](), sum_order, tree=True)
        for a in _expected[key][:2] + _expected[key][2]:
            a.setflags(write=False)
    return _expected[key]


# how phase 2 reads old_v: from LDS (the engine's choice at these sizes), through 32-bit byte offsets from
# sorted_v (what systems above stage_v_max get), through 64-bit addresses (what 2^28 cells and more get)
OLD_V_FORMS = {"lds": {}, "offsets32": {"stage_v_max": 0}, "addresses64": {"stage_v_max": 0, "gather_offset_bits": 64}}


@pytest.mark.gpu
@pytest.mark.parametrize("old_v_form", list(OLD_V_FORMS))
@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_hot_loops_bit_exact(oracle, device, case, sum_order, old_v_form):
    Xo, vo, go = expected(oracle, case, sum_order)

    def setup(s):
        s.set_param("force_variant", 2)  # never the cooperative kernel, however small the system
        for name, value in OLD_V_FORMS[old_v_form].items():
            s.set_param(name, value)

    Xd, vd, gd = two_steps(device, CASES[case](), sum_order, setup=setup)
    n = len(Xo)
    for name, a, b in zip(("cube_id", "point_id", "cube_start", "cube_end"), go, gd):
        if name in ("cube_id", "point_id"):
            a, b = a[:n], b[:n]
        assert np.array_equal(a, b), f"{name} differs"
    assert np.isfinite(Xd).all()
    assert np.array_equal(Xo.view(np.uint32), Xd.view(np.uint32)), "positions not bit-identical"
    assert np.array_equal(vo.view(np.uint32), vd.view(np.uint32)), "old_v not bit-identical"
