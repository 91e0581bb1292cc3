"""What tests/test_links_order_gpu.py leans on, checked without a GPU: the numpy statement of the segmented path's
layout (tests/links_support.piece_layout) on cases small enough to write the answer down, the link layouts' claims
about themselves, the two references of the GPU tests -- the oracle's links_tile and the numpy statement of the step --
against each other bit for bit, and the exactness of the lattice inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ensemble_support import bits, seeded_rows  # noqa: E402
from links_support import (CUT, LATTICE_DT, LATTICE_HUB, LATTICE_N, LATTICE_STRENGTH, UNCUT_LAYOUTS,  # noqa: E402
                           fma32, lattice_links, lattice_rows, lattice_steps_float64, no_segment_is_cut, piece_layout,
                           pieces_per_cell, reference_links_only_steps, rings, rings_with_hub, segmented_link_sums,
                           serial_link_sums, shifted_rings)

from yalla_amd.solution import Solution  # noqa: E402

DT, STRENGTH = 0.01, 0.05


# ---- the layout helper on cases with known answers ----------------------------------------------------------------
def test_piece_layout_of_three_links():
    """(2, 0), (1, 2), (0, 2): entries 0 .. 5 hold cells 2 0 1 2 0 2; sorted stably: cell 0 (entries 1, 4), cell 1
    (entry 2), cell 2 (entries 0, 3, 5)."""
    cell, entry, first = piece_layout([(2, 0), (1, 2), (0, 2)])
    assert cell.tolist() == [0, 0, 1, 2, 2, 2]
    assert entry.tolist() == [1, 4, 2, 0, 3, 5]
    assert first.tolist() == [0, 2, 3, 6]
    assert pieces_per_cell([(2, 0), (1, 2), (0, 2)], 4).tolist() == [1, 1, 1, 0]


def test_piece_layout_skips_inert_slots_and_slots_beyond_the_count():
    links = [(3, 3), (1, 0), (0, 1), (5, 4)]
    cell, entry, first = piece_layout(links)
    assert cell.tolist() == [0, 0, 1, 1, 4, 5] and entry.tolist() == [3, 4, 2, 5, 7, 6]
    cell, entry, first = piece_layout(links, n_live=3)
    assert cell.tolist() == [0, 0, 1, 1] and entry.tolist() == [3, 4, 2, 5] and first.tolist() == [0, 2, 4]
    cell, entry, first = piece_layout(links, n_live=0)
    assert len(cell) == 0 and first.tolist() == [0]
    assert no_segment_is_cut(links, n_live=0)


@pytest.mark.parametrize("front, length, pieces", [(0, 256, [256]), (0, 257, [256, 1]), (1, 255, [255]), (1, 256, [255, 1]),
                                                   (255, 2, [1, 1]), (255, 257, [1, 256]), (256, 256, [256]),
                                                   (2, 511, [254, 256, 1]), (0, 512, [256, 256]), (3, 4, [4])])
def test_pieces_of_a_hub_by_where_its_segment_starts(front, length, pieces):
    """`front` entries of cell 0 and `length` of cell 1 (links (0, 2) and (1, 2); the entries of cell 2 come last):
    the lengths of cell 1's pieces, written down by hand."""
    links = [(0, 2)] * front + [(1, 2)] * length
    cell, entry, first = piece_layout(links)
    lengths = np.diff(first)
    assert lengths[cell[first[:-1]] == 1].tolist() == pieces
    assert pieces_per_cell(links, 3)[1] == len(pieces)
    assert no_segment_is_cut(links) == bool((pieces_per_cell(links, 3) <= 1).all())


@pytest.mark.parametrize("count, uncut", [(1, True), (128, True), (129, False), (256, True), (257, False), (384, False)])
def test_no_segment_is_cut_on_two_cells(count, uncut):
    """`count` links (0, 1): cell 0 holds the entries 0 .. count - 1 and cell 1 the next `count`.  128: the segments
    end on 127 and 255; 129: cell 1's holds 256; 256: each fills a window; 257: cell 0's holds 256; 384: 256 too."""
    assert no_segment_is_cut([(0, 1)] * count) == uncut
    assert count <= CUT or not uncut


def test_the_layouts_are_what_they_say():
    for name, (n, make) in UNCUT_LAYOUTS.items():
        links = make(n)
        assert no_segment_is_cut(links), name
        assert (pieces_per_cell(links, n) <= 1).all(), name
        assert links.min() >= 0 and links.max() < n, name
    n, make = UNCUT_LAYOUTS["rings"]
    assert (np.bincount(make(n).reshape(-1), minlength=n) == 4).all()
    n = UNCUT_LAYOUTS["hub of 256"][0]
    links = rings_with_hub(n)
    cell, _, first = piece_layout(links)
    at = first[:-1][cell[first[:-1]] == 64]
    assert at.tolist() == [256] and int((cell == 64).sum()) == 256      # one piece that fills the window 256 .. 511
    assert (links[:, 0] == links[:, 1]).sum() > 50                       # inert links among them
    assert len(UNCUT_LAYOUTS["127 links"][1](500)) == 127
    # and the counter-case: cut cells, none in more than two pieces
    cut = pieces_per_cell(shifted_rings(1000), 1000)
    assert not no_segment_is_cut(shifted_rings(1000))
    assert cut.max() == 2 and (cut == 2).sum() == 2001 * 2 // CUT


# ---- the two references against each other ------------------------------------------------------------------------
@pytest.mark.parametrize("model, steps", [("links_tile", 3), ("links_grid", 1)])
@pytest.mark.parametrize("name", list(UNCUT_LAYOUTS))
def test_oracle_links_models_are_the_numpy_statement(oracle, name, model, steps):
    """links_tile of the CPU restatement, three steps with set_fixed(p), against reference_links_only_steps
    (reference_linked_steps without the spring) bit for bit.  links_grid: its first step, in which old_v is zero in
    both stages -- from the second on the grid adds the neighbours' velocities cube by cube, not in ascending k as
    the statement does."""
    n, make = UNCUT_LAYOUTS[name]
    links, X0, p = make(n), seeded_rows(3, n, 31), 11
    Xw, vw = reference_links_only_steps(X0, links, STRENGTH, steps, DT, p)
    assert np.abs(Xw - X0).max() > 1e-4
    with Solution(model, n, lib=oracle) as s:
        s.h_X[:n] = X0
        s.copy_to_device()
        s.set_links(links, STRENGTH)
        s.set_fixed(p)
        s.take_step(DT, steps)
        assert np.array_equal(bits(s.positions()), bits(Xw))
        assert np.array_equal(bits(s.old_v()[:n]), bits(vw))


def test_link_sums_of_the_links_only_statement_are_those_of_the_linked_statement():
    """serial_link_sums computes the terms of all links at once; reference_linked_steps computes them in its loop,
    scalar by scalar.  The same bits, on 30 cells with an inert link."""
    X = seeded_rows(3, 30, 2)
    links = np.concatenate([rings(30, 1, 4), [(3, 3)]])
    L = serial_link_sums(X, links, 0.2)
    want = np.zeros((30, 3), np.float32)
    for a, b in links:  # reference_linked_steps' loop, scalar by scalar
        if a == b:
            continue
        r = X[a] - X[b]
        dist = np.sqrt(fma32(r[2], r[2], fma32(r[1], r[1], np.float32(r[0] * r[0]))))
        f = (np.float32(0.2) * r) / dist
        want[a] = want[a] + (-f)
        want[b] = want[b] + f
    assert np.array_equal(bits(L), bits(want))


def test_a_cut_segment_changes_the_bits_and_only_its_own():
    """The counter-case of the GPU suite, on the CPU: the statement of the segmented sum predicts the oracle's serial
    sum on every cell in one piece bit for bit, and other bits on some of the cells in two (p1 + p2 is not t1 + t2 +
    t3 + t4 from the left)."""
    n = 1000
    links, X = shifted_rings(n), seeded_rows(3, n, 31)
    serial, cut_sum = serial_link_sums(X, links, STRENGTH), segmented_link_sums(X, links, STRENGTH)
    two = pieces_per_cell(links, n) == 2
    assert not np.isnan(cut_sum).any()
    assert np.array_equal(bits(serial[~two]), bits(cut_sum[~two]))
    differ = (bits(serial[two]) != bits(cut_sum[two])).any(axis=1)
    assert 0 < differ.sum() <= two.sum()
    assert np.abs(serial - cut_sum).max() <= 4 * 2.0 ** -24 * 4 * STRENGTH


# ---- the lattice inputs are exact -----------------------------------------------------------------------------------
def test_lattice_steps_are_exact_in_binary32(oracle):
    """Three steps of the oracle's links_tile on the lattice equal a binary64 run of the same statement rounded once:
    no sum and no update of the binary32 run rounded, so the order of the additions cannot show."""
    X0, links = lattice_rows(), lattice_links()
    assert (links[:, 0] == LATTICE_HUB).sum() + (links[:, 1] == LATTICE_HUB).sum() >= 300
    x, v = lattice_steps_float64(X0, links, LATTICE_STRENGTH, 3, LATTICE_DT)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)      # representable, every one of them
    assert np.abs(x - X0[:, 0]).max() > 0.1
    with Solution("links_tile", LATTICE_N, lib=oracle) as s:
        s.h_X[:LATTICE_N] = X0
        s.copy_to_device()
        s.set_links(links, LATTICE_STRENGTH)
        s.take_step(LATTICE_DT, 3)
        X = s.positions()
        assert np.array_equal(X[:, 0].astype(np.float64), x)
        assert np.array_equal(s.old_v()[:LATTICE_N, 0].astype(np.float64), v)
        assert (X[:, 1:] == 0).all()
    # and with the links in reverse slot order: the same bits (every sum exact)
    with Solution("links_tile", LATTICE_N, lib=oracle) as s:
        s.h_X[:LATTICE_N] = X0
        s.copy_to_device()
        s.set_links(links[::-1], LATTICE_STRENGTH)
        s.take_step(LATTICE_DT, 3)
        assert np.array_equal(bits(s.positions()), bits(X))
