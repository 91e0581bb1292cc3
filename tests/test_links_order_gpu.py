"""Links::link_forces inside whole steps of a lone Solution, bit for bit (tests/native/test_links_sums.cu holds the
kernels alone).  The segmented path sums a cell's entries in link slot order from 0 and adds the sum to a zeroed
right-hand side, which is the oracle's serial loop over the links -- as long as no cell's segment is cut (a cut every
256 entries of the sorted array; tests/links_support.no_segment_is_cut, asserted for every layout): positions and old_v
of links_tile, links_grid, links4_tile and springs_links_grid equal the oracle's, and links_tile's the numpy statement
of the step.  One layout WITH cut segments shows that this condition carries the equality.  The atomics path is held
bit for bit on lattice inputs, where every sum and update is exact in any order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ensemble_support import bits, seeded_rows  # noqa: E402
from links_support import (LATTICE_DT, LATTICE_N, LATTICE_STRENGTH, UNCUT_LAYOUTS, lattice_links,  # noqa: E402
                           lattice_rows, lattice_steps_float64, no_segment_is_cut, pieces_per_cell,
                           reference_links_only_steps, segmented_link_sums, serial_link_sums, shifted_rings)
from test_parity_gpu import REL_TOL  # noqa: E402

from yalla_amd.solution import Solution  # noqa: E402

pytestmark = pytest.mark.gpu

DT, STRENGTH = 0.01, 0.05
SEGMENTED, ATOMICS, DEFAULT = 1, 1 << 30, 1000000
N_FLOATS = {"links_tile": 3, "links_grid": 3, "links4_tile": 4, "springs_links_grid": 3}


def stepped(lib, model, X0, links, strength, calls, seg_min=None, fixed=None):
    """(positions, old_v[:n]) after take_step(dt, steps) for every (dt, steps) of `calls`, from X0 with `links`; on
    the device with links_segmented_min = seg_min (process-wide: put back to its default afterwards), on the oracle
    with the device's reduction order."""
    n = len(X0)
    with Solution(model, n, lib=lib) as s:
        try:
            if seg_min is None:
                assert s.set_reduce_order(1) == 0
            else:
                s.set_param("links_segmented_min", seg_min)
            s.h_X[:n] = X0
            s.copy_to_device()
            s.set_links(links, strength)
            if fixed is not None:
                s.set_fixed(fixed)
            for dt, steps in calls:
                s.take_step(dt, steps)
            return s.positions(), s.old_v()[:n]
        finally:
            if seg_min is not None:
                s.set_param("links_segmented_min", DEFAULT)


def same(a, b, what):
    assert np.array_equal(bits(a[0]), bits(b[0])), (what, "positions")
    assert np.array_equal(bits(a[1]), bits(b[1])), (what, "old_v")


@pytest.mark.parametrize("layout", list(UNCUT_LAYOUTS))
@pytest.mark.parametrize("model", list(N_FLOATS))
def test_segmented_path_is_the_serial_loop_bit_for_bit(oracle, device, model, layout):
    """No segment is cut: three steps of the segmented path are the oracle's, positions and old_v."""
    n, make = UNCUT_LAYOUTS[layout]
    links, X0 = make(n), seeded_rows(N_FLOATS[model], n, 31)
    assert no_segment_is_cut(links)
    want = stepped(oracle, model, X0, links, STRENGTH, [(DT, 3)])
    assert np.abs(want[0][:, :3] - X0[:, :3]).max() > 1e-4 and not np.isnan(want[0]).any()
    same(want, stepped(device, model, X0, links, STRENGTH, [(DT, 3)], SEGMENTED), (model, layout))


@pytest.mark.parametrize("model, steps", [("links_tile", 3), ("links_grid", 1)])
@pytest.mark.parametrize("layout", list(UNCUT_LAYOUTS))
def test_segmented_path_is_the_numpy_statement(device, layout, model, steps):
    """links_tile with set_fixed(p) against tests/links_support.reference_links_only_steps (reference_linked_steps
    without its spring: these models have no pairwise force), no oracle in between; links_grid for its first step,
    as far as that statement's order of the neighbours' velocities is the grid's (tests/test_links_order.py)."""
    n, make = UNCUT_LAYOUTS[layout]
    links, X0, p = make(n), seeded_rows(3, n, 31), 11
    want = reference_links_only_steps(X0, links, STRENGTH, steps, DT, p)
    same(want, stepped(device, model, X0, links, STRENGTH, [(DT, steps)], SEGMENTED, fixed=p), (model, layout))


def test_a_cut_segment_is_summed_in_two_pieces(oracle, device):
    """The counter-case: rings behind one more link, so that every multiple of 256 cuts a cell's four entries into
    two pieces of two.  A step of dt = 0 leaves the first stage's right-hand side in old_v (both stages see the same
    positions; the fixed cell 5 is in one piece): on the device it is the statement of the segmented sum, (t1 + t2) +
    (t3 + t4) on a cut cell -- NOT the oracle's ((t1 + t2) + t3) + t4 on some of them, the oracle's on every other
    cell.  Then a real step: positions within the tolerance of the lock-step tests."""
    n, p = 1000, 5
    links, X0 = shifted_rings(n), seeded_rows(3, n, 31)
    pieces = pieces_per_cell(links, n)
    two = pieces == 2
    assert not no_segment_is_cut(links) and pieces.max() == 2 and two.sum() >= 7 and not two[p]
    L = segmented_link_sums(X0, links, STRENGTH)
    assert np.array_equal(bits(L[~two]), bits(serial_link_sums(X0, links, STRENGTH)[~two]))
    rhs = L - L[p]
    Xo, _ = stepped(oracle, "links_tile", X0, links, STRENGTH, [(0.0, 1), (DT, 1)], fixed=p)
    Xd, vd = stepped(device, "links_tile", X0, links, STRENGTH, [(0.0, 1)], SEGMENTED, fixed=p)
    assert np.array_equal(bits(Xd), bits(X0))
    assert np.array_equal(bits(vd), bits(rhs))                      # the statement, every cell
    with_oracle = stepped(oracle, "links_tile", X0, links, STRENGTH, [(0.0, 1)], fixed=p)[1]
    assert np.array_equal(bits(vd[~two]), bits(with_oracle[~two]))   # the oracle, every cell in one piece
    assert (bits(vd[two]) != bits(with_oracle[two])).any()           # ... and not on every cut one
    Xd, vd = stepped(device, "links_tile", X0, links, STRENGTH, [(0.0, 1), (DT, 1)], SEGMENTED, fixed=p)
    assert np.abs(Xd - X0).max() > 1e-4
    assert np.abs(Xd - Xo).max() <= REL_TOL * np.abs(Xo).max()


def test_atomics_path_bit_for_bit_on_exact_inputs(oracle, device):
    """links_tile, 512 cells on the x axis at multiples of 8, strength 2^-7, dt 2^-2, a hub of 300 links: every term
    is +-2^-7 and every sum and update exact (checked here: the oracle's run is a binary64 run rounded once), so the
    one-thread-per-link kernel's atomics give the oracle's bits in whatever order they land.  The segmented path
    too, cut hub and all."""
    X0, links = lattice_rows(), lattice_links()
    want = stepped(oracle, "links_tile", X0, links, LATTICE_STRENGTH, [(LATTICE_DT, 3)])
    x, v = lattice_steps_float64(X0, links, LATTICE_STRENGTH, 3, LATTICE_DT)
    assert np.array_equal(want[0][:, 0].astype(np.float64), x) and np.array_equal(want[1][:, 0].astype(np.float64), v)
    assert np.abs(x - X0[:, 0]).max() > 0.1
    assert pieces_per_cell(links, LATTICE_N).max() >= 2      # (the hub is cut)
    same(want, stepped(device, "links_tile", X0, links, LATTICE_STRENGTH, [(LATTICE_DT, 3)], ATOMICS), "atomics")
    same(want, stepped(device, "links_tile", X0, links, LATTICE_STRENGTH, [(LATTICE_DT, 3)], SEGMENTED), "segmented")
