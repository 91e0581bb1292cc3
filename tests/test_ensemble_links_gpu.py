"""Ordered link forces of ensembles (include/ensemble_links.cuh; LinkedEnsemble over libyalla_ensemble_links.so): a
cell's link terms are added in ascending slot order from +0, by a batched kernel on the six-launch path
(ya::ens::link_forces_ordered) and inside whole-step launches (ya::ens::whole_steps_linked), the same bits.  THE
REFERENCES: the six-launch ordered twin (every row, used or not), the twin with links_path = 1 (link_forces, global
atomics -- only where a cell has at most two terms, whose sum does not depend on the order), a lone
Solution("links_tile" / "links4_tile") per replica, the CPU restatement's links_tile, and a numpy binary32 statement
of the step.  Every comparison is of bit patterns (uint32, array_equal): no tolerance anywhere.  Every case checks
`whole_step_launches` for the path it expects."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ensemble_support import DT, bits, largest_slots, lds_layout, seeded_rows  # noqa: E402
from ensemble_support import LINKED_MODELS as MODELS  # noqa: E402
from ensemble_support import LINKED_N_FLOATS as N_FLOATS  # noqa: E402
from links_support import reference_linked_steps  # noqa: E402

from yalla_amd.ensemble import LinkedEnsemble, YallaError  # noqa: E402
from yalla_amd.solution import Solution  # noqa: E402

pytestmark = pytest.mark.gpu

UNUSED = np.float32(-7.25)  # what unused rows hold, to be found again


class Run:
    """A LinkedEnsemble fed seeded rows (replica r: seed 1000 * seed + r), unused rows a pattern of their own, and
    per-replica links given as LOCAL (a, b) pairs from slot 0 on (every other slot inert)."""

    def __init__(self, model, counts, n_max, slots, links, seed=0, strength=0.2, n_links=None, **params):
        self.counts = list(counts)
        self.ens = LinkedEnsemble(model, len(counts), n_max, slots, strength)
        for name, value in params.items():
            self.ens.set_param(name, value)
        self.ens.h_X[:] = UNUSED
        for r, n in enumerate(counts):
            self.ens.h_X[r, :n] = seeded_rows(self.ens.n_floats, n, 1000 * seed + r)
            self.ens.h_n[r] = n
        self.set_links(links, n_links)
        self.ens.copy_to_device()

    def set_links(self, links, n_links=None):
        ens = self.ens
        ens.h_link[:] = 0
        for r, pairs in enumerate(links):
            pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
            ens.h_link[r, :len(pairs)] = pairs + r * ens.n_max
        ens.n_links = ens.n_replicas * ens.slots_per_replica if n_links is None else n_links

    def state(self):
        self.ens.copy_to_host()
        return self.ens.h_X.copy(), self.ens.old_v()

    def close(self):
        self.ens.close()


def same(a, b, what=""):
    (Xa, va), (Xb, vb) = a, b
    assert np.array_equal(bits(Xa), bits(Xb)), (what, "positions")
    assert np.array_equal(bits(va), bits(vb)), (what, "old_v")


def no_nan(state):
    assert not np.isnan(state[0]).any() and not np.isnan(state[1]).any()


def random_links(n, count, seed):
    """`count` links between distinct cells of 0 .. n - 1 (none for n < 2)."""
    rng = np.random.default_rng(seed)
    if n < 2:
        return np.zeros((0, 2), np.int64)
    a = rng.integers(0, n, count)
    b = (a + 1 + rng.integers(0, n - 1, count)) % n
    return np.stack([a, b], axis=1)


# ---- chains: at most two terms per cell ----------------------------------------------------------------------------
CHAIN_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024]


def chains(counts):
    return [np.array([(k, k + 1) if k % 2 else (k + 1, k) for k in range(max(n - 1, 0))]).reshape(-1, 2) for n in counts]


def start_v(n_replicas, n_max):
    rng = np.random.default_rng(9)
    return (rng.random((n_replicas, n_max, 3)) * 0.2 - 0.1).astype(np.float32)


def chain_sequence(run):
    """1 step, then 5 steps from a non-zero old_v; the two states."""
    run.ens.take_step(DT, 1)
    first = run.state()
    run.ens.set_old_v(start_v(len(CHAIN_COUNTS), 1024))
    run.ens.take_step(DT, 5)
    return first, run.state()


@functools.lru_cache(maxsize=None)
def chain_reference(model):
    """Once per model, by the paths that do not run whole: the six-launch ordered twin, held against the twin with
    atomics and -- for links and links4 -- against a lone Solution per replica."""
    links = chains(CHAIN_COUNTS)
    six = Run(model, CHAIN_COUNTS, 1024, 1024, links, seed=3)
    atomics = Run(model, CHAIN_COUNTS, 1024, 1024, links, seed=3, links_path=1)
    try:
        want = chain_sequence(six)
        got = chain_sequence(atomics)
        assert six.ens.whole_step_launches == 0 and atomics.ens.whole_step_launches == 0
        for k in (0, 1):
            no_nan(want[k])
            same(want[k], got[k], "atomics")
    finally:
        six.close()
        atomics.close()
    if model in ("links", "links4"):
        v0 = start_v(len(CHAIN_COUNTS), 1024)
        for r, n in enumerate(CHAIN_COUNTS):
            if n == 0:
                continue
            with Solution(model + "_tile", 1024) as s:
                s.h_X[:n] = seeded_rows(N_FLOATS[model], n, 3000 + r)
                s.h_n = n
                s.copy_to_device()
                if n > 1:
                    s.set_links(links[r], 0.2)
                s.take_step(DT, 1)
                assert np.array_equal(bits(s.positions()), bits(want[0][0][r, :n])), r
                assert np.array_equal(bits(s.old_v()[:n]), bits(want[0][1][r, :n])), r
                s.set_old_v(v0[r])
                s.take_step(DT, 5)
                assert np.array_equal(bits(s.positions()), bits(want[1][0][r, :n])), r
                assert np.array_equal(bits(s.old_v()[:n]), bits(want[1][1][r, :n])), r
    return want


@pytest.mark.parametrize("lanes", [1, 4, 16, 64])
@pytest.mark.parametrize("model", MODELS)
def test_chains_bit_for_bit(model, lanes):
    """Links (k, k + 1) within a replica, every count of CHAIN_COUNTS in one ensemble of n_max = S = 1024, whole with
    1, 4, 16 and 64 lanes per cell: the bits of the six-launch ordered twin, of the atomics and of lone Solutions."""
    want = chain_reference(model)
    run = Run(model, CHAIN_COUNTS, 1024, 1024, chains(CHAIN_COUNTS), seed=3, whole_steps=1, whole_step_lanes=lanes)
    try:
        got = chain_sequence(run)
        assert run.ens.whole_step_launches == 2
        assert run.ens.whole_step_lanes_used == lanes
        same(want[0], got[0], "1 step")
        same(want[1], got[1], "5 steps from a non-zero old_v")
        unused = np.arange(1024)[None, :] >= np.asarray(CHAIN_COUNTS)[:, None]
        assert np.all(got[1][0][unused] == UNUSED)
        assert np.array_equal(bits(got[1][1])[unused], bits(start_v(len(CHAIN_COUNTS), 1024))[unused])
    finally:
        run.close()


# ---- hubs: 1023 terms in one cell ----------------------------------------------------------------------------------
HUB_COUNTS = [1024, 300, 1024, 2]
HUB_STRENGTH = 0.002  # (cell 0 is pulled by every other cell at once)


def hub_links(n, r, n_max=1024):
    """LOCAL pairs of replica r from slot 0 on, and which of them count (a != b, both ends among the replica's n
    cells): every cell k linked with cell 0 (either way round), doubled links, an inert slot, a link into ANOTHER
    replica and links to rows >= n (unused rows, or the next replica's first row): the last two kinds are skipped."""
    pairs = [(0, k) if k % 3 else (k, 0) for k in range(1, n)]
    pairs += [(0, 5), (0, 5), (7, 3), (3, 7), (1, 1), (1, (1 if r == 0 else -1) * n_max + 3), (n, 0), (0, 1)]
    pairs = np.array(pairs).reshape(-1, 2)
    a, b = pairs[:, 0], pairs[:, 1]
    return pairs, (a != b) & (a >= 0) & (a < n) & (b >= 0) & (b < n)


def hub_run(model, slots, **params):
    links = [hub_links(n, r)[0] for r, n in enumerate(HUB_COUNTS)]
    run = Run(model, HUB_COUNTS, 1024, slots, links, seed=5, strength=HUB_STRENGTH, **params)
    # slots beyond n_links that hold valid ids and must be ignored: the last 50 of the last replica
    run.ens.h_link[-1, -50:] = np.array([0, 1]) + (len(HUB_COUNTS) - 1) * 1024
    run.ens.n_links = len(HUB_COUNTS) * slots - 50
    run.ens.copy_to_device()
    return run


@functools.lru_cache(maxsize=None)
def hub_reference(model, slots):
    six = hub_run(model, slots)
    try:
        six.ens.take_step(DT, 3)
        assert six.ens.whole_step_launches == 0
        want = six.state()
        no_nan(want)
        return want
    finally:
        six.close()


@pytest.mark.parametrize("lanes", [1, 4, 16])
@pytest.mark.parametrize("model", MODELS)
def test_hubs_bit_for_bit(model, lanes):
    """Cell 0 of a full replica sums 1023 terms -- plus doubled links, inert slots, slots beyond n_links, a link
    into another replica and one to a row >= n_r -- with S = 3 n_max: whole against the six-launch ordered twin.
    Po_cell with 4 lanes: the term buffer does not fit beside the list, so the launches run with one lane."""
    slots = 3 * 1024
    n_floats = N_FLOATS[model]
    assert lds_layout(n_floats, 1024, False, slots, 1).bytes > 0
    want = hub_reference(model, slots)
    run = hub_run(model, slots, whole_steps=1, whole_step_lanes=lanes)
    try:
        run.ens.take_step(DT, 3)
        assert run.ens.whole_step_launches == 1
        fits = lds_layout(n_floats, 1024, False, slots, lanes).bytes > 0
        assert fits == (not (model == "relu_po_links" and lanes == 4))  # the lanes fallback to 1
        assert run.ens.whole_step_lanes_used == (lanes if fits else 1)
        same(want, run.state(), "hub")
    finally:
        run.close()


def test_hubs_against_the_cpu_restatement(oracle):
    """`links` stepped whole against the oracle's links_tile (its serial loop over the links in slot order, with the
    device's reduction order), fed the same links without the skipped ones: the comparison that does not pass
    through shared device code."""
    run = hub_run("links", 3 * 1024, whole_steps=1)
    try:
        run.ens.take_step(DT, 3)
        assert run.ens.whole_step_launches == 1
        X, v = run.state()
    finally:
        run.close()
    same(hub_reference("links", 3 * 1024), (X, v), "six launches")
    for r, n in enumerate(HUB_COUNTS):
        pairs, counted = hub_links(n, r)
        with Solution("links_tile", 1024, lib=oracle) as s:
            assert s.set_reduce_order(1) == 0
            s.h_X[:n] = seeded_rows(3, n, 5000 + r)
            s.h_n = n
            s.copy_to_device()
            s.set_links(pairs[counted], HUB_STRENGTH)
            s.take_step(DT, 3)
            assert np.array_equal(bits(s.positions()), bits(X[r, :n])), r
            assert np.array_equal(bits(s.old_v()[:n]), bits(v[r, :n])), r


# ---- the numpy statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", [1, -1])
def test_against_a_numpy_statement_of_the_step(whole):
    """springs_links, 40 cells, 60 slots: random links with a hub, a doubled link and a self-link, 3 steps of dt 0.05
    with set_fixed(p): positions and old_v of both ordered paths against numpy binary32, operation by operation."""
    n, slots, p = 40, 60, 7
    links = np.concatenate([random_links(n, 30, 1), [(4, k) for k in range(10, 30)], [(2, 9), (2, 9), (6, 6)],
                            random_links(n, 7, 2)])
    assert len(links) == slots
    X0 = seeded_rows(3, n, 11)
    Xw, vw = reference_linked_steps(X0, links, 0.2, 3, DT, p)
    assert np.abs(Xw - X0).max() > 1e-2
    run = Run("springs_links", [n, n], n, slots, [links, links], whole_steps=whole)
    try:
        for r in (0, 1):  # (the same rows in both replicas: the id offset must not show)
            run.ens.h_X[r] = X0
        run.ens.copy_to_device()
        run.ens.set_fixed(p)
        run.ens.take_step(DT, 3)
        assert run.ens.whole_step_launches == (1 if whole == 1 else 0)
        X, v = run.state()
        for r in (0, 1):
            assert np.array_equal(bits(Xw), bits(X[r])), r
            assert np.array_equal(bits(vw), bits(v[r])), r
    finally:
        run.close()


# ---- other cases: whole against the six-launch ordered twin -------------------------------------------------------
class Pair:
    """The same ensemble twice: stepped whole, and by the six launches."""

    def __init__(self, model, counts, n_max, slots, links, seed=0, **params):
        self.whole = Run(model, counts, n_max, slots, links, seed=seed, whole_steps=1, **params)
        self.six = Run(model, counts, n_max, slots, links, seed=seed)
        self.seen = 0

    def each(self, call):
        call(self.whole)
        call(self.six)

    def step(self, dt, steps, launches, what=""):
        self.each(lambda run: run.ens.take_step(dt, steps))
        assert self.whole.ens.whole_step_launches - self.seen == launches, what
        self.seen = self.whole.ens.whole_step_launches
        assert self.six.ens.whole_step_launches == 0
        same(self.six.state(), self.whole.state(), what)

    def close(self):
        self.whole.close()
        self.six.close()


MIXED = [300, 70, 0, 64, 257, 5]


def mixed_links(seed=0, per_cell=1):
    return [random_links(n, per_cell * n, 10 * seed + r) for r, n in enumerate(MIXED)]


@pytest.mark.parametrize("model", ["relu_links", "relu_po_links"])  # (all-pairs springs of 300 cells diverge at this dt)
def test_all_three_fixed_modes(model):
    pair = Pair(model, MIXED, 300, 300, mixed_links())
    try:
        for what, change, steps in [("set_fixed()", None, 2),
                                    ("set_fixed(4)", lambda run: run.ens.set_fixed(4), 3),
                                    ("set_fixed_xy(2)", lambda run: run.ens.set_fixed_xy(2), 3),
                                    ("set_fixed(1) after xy", lambda run: run.ens.set_fixed(1), 2),
                                    ("set_fixed() after xy", lambda run: run.ens.set_fixed(), 2)]:
            if change:
                pair.each(change)
            pair.step(DT, steps, 1, what)
        no_nan(pair.six.state())
    finally:
        pair.close()


def test_steps_per_launch_splits_a_call():
    pair = Pair("relu_links", MIXED, 300, 600, mixed_links(1, 2), steps_per_launch=3)
    try:
        pair.step(DT, 7, 3, "3 + 3 + 1")
        pair.step(DT, 3, 1, "3")
        pair.whole.ens.set_param("steps_per_launch", 1)
        pair.step(DT, 4, 4, "1 + 1 + 1 + 1")
    finally:
        pair.close()


def test_links_and_their_count_change_between_calls():
    """What copy_to_device hands over before a call is what the call's launches see: other links, then fewer slots
    in use (the slots beyond the count still hold their ids)."""
    pair = Pair("relu_links", MIXED, 300, 300, mixed_links(2))
    try:
        pair.step(DT, 2, 1, "the first links")
        before = pair.whole.state()

        def renew(run):
            run.ens.copy_to_host()
            run.set_links(mixed_links(3))
            run.ens.copy_to_device()
        pair.each(renew)
        pair.step(DT, 2, 1, "other links")

        def fewer(run):
            run.ens.copy_to_host()
            run.ens.n_links = 4 * 300 + 100  # replica 4 keeps 100 slots, replica 5 none
            run.ens.copy_to_device()
        pair.each(fewer)
        pair.step(DT, 2, 1, "fewer slots in use")
        no_nan(pair.whole.state())
        # and the count mattered: with every slot in use the same two steps end elsewhere
        other = Run("relu_links", MIXED, 300, 300, mixed_links(3), whole_steps=1)
        try:
            other.ens.h_X[:] = before[0]
            other.ens.copy_to_device()
            other.ens.set_old_v(before[1])
            other.ens.take_step(DT, 4)
            X, _ = other.state()
            now = pair.whole.state()[0]
            assert np.array_equal(bits(X[:4]), bits(now[:4]))
            assert not np.array_equal(bits(X[4, :257]), bits(now[4, :257]))
        finally:
            other.close()
    finally:
        pair.close()


def test_replicas_are_independent():
    """Other rows and other links in replica 1 change replica 1 alone."""
    links = mixed_links(4)
    a = Run("relu_links", MIXED, 300, 300, links, whole_steps=1)
    changed = list(links)
    changed[1] = random_links(70, 70, 99)
    b = Run("relu_links", MIXED, 300, 300, changed, whole_steps=1)
    try:
        b.ens.h_X[1, :70] = seeded_rows(3, 70, 77)
        b.ens.copy_to_device()
        for run in (a, b):
            run.ens.take_step(DT, 3)
            assert run.ens.whole_step_launches == 1
        (Xa, va), (Xb, vb) = a.state(), b.state()
        others = [0, 2, 3, 4, 5]
        assert np.array_equal(bits(Xa[others]), bits(Xb[others])) and np.array_equal(bits(va[others]), bits(vb[others]))
        assert not np.array_equal(bits(Xa[1, :70]), bits(Xb[1, :70]))
    finally:
        a.close()
        b.close()


def test_five_thousand_replicas_of_sixteen_cells():
    """The engine's choice of lanes for a stateless functor: 16 lanes per cell at n_max = 16."""
    m = 5000
    counts = [16 - (r % 5 == 0) * (r % 16) for r in range(m)]
    links = [random_links(n, 16, r) for r, n in enumerate(counts)]
    pair = Pair("relu_links", counts, 16, 16, links, whole_step_lanes=0)
    try:
        pair.step(DT, 4, 1)
        assert pair.whole.ens.whole_step_lanes_used == 16
        no_nan(pair.whole.state())
    finally:
        pair.close()


@pytest.mark.parametrize("model, lanes", [("links", 1), ("links4", 1), ("relu_links", 4), ("relu_po_links", 4)])
def test_the_default_lanes_follow_what_the_functor_declares(model, lanes):
    """whole_step_lanes = 0 at n_max = 40, where a stateless functor gets 4 lanes per cell: relu_force is declared
    YA_STATELESS, models::no_pw_int is not and keeps one lane per cell; the bits are the six-launch twin's."""
    counts = [40, 0, 17, 33, 1]
    links = [random_links(n, 80, 40 + r) for r, n in enumerate(counts)]
    pair = Pair(model, counts, 40, 80, links, whole_step_lanes=0)
    try:
        pair.step(DT, 3, 1)
        assert pair.whole.ens.whole_step_lanes_used == lanes
        no_nan(pair.whole.state())
    finally:
        pair.close()


def test_the_largest_list_that_fits_and_one_beyond():
    """n_max = 1024 of float3: the largest S the rule admits runs whole; one slot more is the six-launch loop with
    link_forces_ordered -- 0 launches -- and the same bits."""
    fits = largest_slots(3, 1024)
    assert lds_layout(3, 1024, False, fits, 1).bytes > 0 and lds_layout(3, 1024, False, fits + 1, 1).bytes == 0
    counts = [1024, 500]
    # every slot in use: eleven links per cell, all of them counted
    links = [random_links(n, fits, 20 + r) for r, n in enumerate(counts)]
    states = []
    for slots, launches in ((fits, 1), (fits + 1, 0)):
        run = Run("links", counts, 1024, slots, links, seed=8, strength=0.01, whole_steps=1, whole_step_lanes=16)
        try:
            assert LinkedEnsemble.lds_bytes("links", 1024, slots, 1) == lds_layout(3, 1024, False, slots, 1).bytes
            run.ens.take_step(DT, 2)
            assert run.ens.whole_step_launches == launches
            if launches:  # (no room for the terms of 16 lanes beside that list)
                assert run.ens.whole_step_lanes_used == 1
            states.append(run.state())
        finally:
            run.close()
    six = Run("links", counts, 1024, fits, links, seed=8, strength=0.01)
    try:
        six.ens.take_step(DT, 2)
        assert six.ens.whole_step_launches == 0
        states.append(six.state())
    finally:
        six.close()
    no_nan(states[0])
    same(states[0], states[1], "one slot beyond")
    same(states[0], states[2], "six launches")


def test_parameters_are_validated():
    with LinkedEnsemble("relu_links", 2, 10, 10) as ens:
        for name, good, bad in [("links_path", (0, 1), (-1, 2, 0.5)), ("whole_steps", (-1, 0, 1), (2, -2)),
                                ("whole_step_lanes", (0, 1, 4, 16, 64), (-1, 2, 8, 32, 128, 1.5)),
                                ("tile_lanes", (0, 1, 16, 64), (2, 4)), ("steps_per_launch", (1, 256), (0, -1, 1.5))]:
            for value in good:
                assert ens.set_param(name, value) == 0
            for value in bad:
                with pytest.raises(YallaError, match="-3"):
                    ens.set_param(name, value)
        with pytest.raises(YallaError, match="-2"):
            ens.set_param("gabriel_coefficient", 0.5)
        assert ens.n_links == 20
        for value in (-1, 21):
            with pytest.raises(YallaError, match="-3"):
                ens.n_links = value
        assert ens.n_links == 20
        # links_path = 1 never runs whole, whatever whole_steps says
        ens.set_param("whole_steps", 1)
        ens.set_param("links_path", 1)
        ens.h_X[:] = seeded_rows(3, 20, 1).reshape(2, 10, 3)
        ens.h_link[:, 0] = [[0, 1], [10, 11]]
        ens.copy_to_device()
        ens.take_step(DT, 2)
        assert ens.whole_step_launches == 0
        ens.set_param("links_path", 0)
        ens.take_step(DT, 2)
        assert ens.whole_step_launches == 1
    with LinkedEnsemble("links", 3, 10, 0) as none:  # no slots at all: the plain step
        assert none.h_link.shape == (3, 0, 2) and none.n_links == 0
        none.set_param("whole_steps", 1)
        none.h_X[:] = seeded_rows(3, 30, 2).reshape(3, 10, 3)
        none.copy_to_device()
        none.take_step(DT, 2)
        assert none.whole_step_launches == 1
