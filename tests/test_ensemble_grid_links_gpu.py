"""Ordered link forces of grid ensembles (include/ensemble_grid.cuh, include/ensemble_links.cuh; LinkedGridEnsemble over
libyalla_ensemble_grid_links.so): take_steps(dt, K, Replica_links) as launches that step from LDS
(ya::ens::grid_lds_steps_linked, lds_steps = 1) against THE REFERENCES: (a) the twin, the same object type with
lds_steps = -1 -- the 14-launch step with ya::ens::link_forces_ordered -- compared in every row of the positions and of
old_v, used or not, and in every replica's grid arrays and status; (b) the twin with links_path = 1 (link_forces,
global atomics) and a lone Solution("links_grid" / "springs_links_grid") per replica, ONLY for chains, where a cell has
at most two terms, whose sum does not depend on their order; (c) the oracle's links_grid / springs_links_grid per
replica, whose link loop is serial in slot order, for layouts where the order matters (every end inside the replica:
the oracle has no skipping rule).  Every comparison is of bit patterns, no tolerance anywhere; every case asserts
`lds_step_launches` for the path it expects."""
import functools

import numpy as np
import pytest
from ensemble_grid_links_support import MODELS, N_FLOATS, Pair, Run, box_rows, no_nan, random_links, same
from ensemble_grid_lds_support import UNUSED
from ensemble_support import DT, bits, largest_slots, lds_layout, same_grid, seeded_rows

from yalla_amd.ensemble import LinkedGridEnsemble, YallaError
from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu

f32 = np.float32
SMALL_DT = 0.01  # (cells that start 0.36 or more inside their grid's faces stay inside for six steps)


# ---- chains: at most two terms per cell -----------------------------------------------------------------------------
CHAIN_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024]
CHAIN_GRID = 9


def chain_shape(model):
    """(n_max, counts): n_max = S = 1024 where a list of 1024 slots fits beside the keys; for the 8-float point the
    largest n_max with room for a list of n_max slots (found here, on the CPU), the two largest counts cut to it."""
    n_floats = N_FLOATS[model]
    n_max = max(n for n in range(1, 1025) if lds_layout(n_floats, n, True, n).bytes > 0)
    assert (n_max == 1024) == (n_floats < 8) and n_max > 900
    return n_max, [n if n < 1023 else n_max - (1024 - n) for n in CHAIN_COUNTS]


def chains(counts):
    return [np.array([(k, k + 1) if k % 2 else (k + 1, k) for k in range(max(n - 1, 0))]).reshape(-1, 2) for n in counts]


def chain_rows(model, counts):
    return [box_rows(n, N_FLOATS[model], CHAIN_GRID, 300 + 17 * r) for r, n in enumerate(counts)]


def start_v(n_replicas, n_max):
    rng = np.random.default_rng(9)
    return (rng.random((n_replicas, n_max, 3)) * 0.2 - 0.1).astype(f32)


def chain_sequence(run):
    """1 step, then 5 steps from a non-zero old_v; the two states."""
    run.ens.take_step(SMALL_DT, 1)
    first = run.state()
    run.ens.set_old_v(start_v(len(run.counts), run.ens.n_max))
    run.ens.take_step(SMALL_DT, 5)
    return first, run.state()


@functools.lru_cache(maxsize=None)
def chain_reference(model):
    """Once per model, by the paths that do not step from LDS: the 14-launch ordered twin (a), held against the twin
    with atomics and -- for links and springs_links -- against a lone Solution per replica (b)."""
    n_max, counts = chain_shape(model)
    links, rows = chains(counts), chain_rows(model, counts)
    twin = Run(model, rows, n_max, n_max, links, CHAIN_GRID, lds_steps=-1)
    atomics = Run(model, rows, n_max, n_max, links, CHAIN_GRID, lds_steps=1, links_path=1)
    try:
        want = chain_sequence(twin)
        got = chain_sequence(atomics)
        assert twin.ens.lds_step_launches == 0 and atomics.ens.lds_step_launches == 0
        for k in (0, 1):
            no_nan(want[k])
            assert not any(want[k][2]), "a replica left its grid"
            same(want[k], got[k], counts, "atomics")
    finally:
        twin.close()
        atomics.close()
    if model in ("links", "springs_links"):
        v0 = start_v(len(counts), n_max)
        for r, n in enumerate(counts):
            if n == 0:
                continue
            with Solution(model + "_grid", n_max, CHAIN_GRID, 1.0) as s:
                s.h_X[:n] = rows[r]
                s.h_n = n
                s.copy_to_device()
                if n > 1:
                    s.set_links(links[r], 0.2)
                for k, steps in ((0, 1), (1, 5)):
                    if k:
                        s.set_old_v(v0[r])
                    s.take_step(SMALL_DT, steps)
                    assert np.array_equal(bits(s.positions()), bits(want[k][0][r, :n])), (r, k)
                    assert np.array_equal(bits(s.old_v()[:n]), bits(want[k][1][r, :n])), (r, k)
                    assert same_grid(s.grid(), want[k][3][r], n), (r, k)
    return want


@pytest.mark.parametrize("model", MODELS)
def test_chains_bit_for_bit(model):
    """Links (k, k + 1) within a replica, every count of CHAIN_COUNTS in one ensemble of n_max = S = 1024 (the 8-float
    point: the largest n_max with room for its list): from LDS, the bits of the 14-launch ordered twin, of the atomics
    and of lone Solutions -- 1 step, then 5 steps from a non-zero old_v."""
    want = chain_reference(model)
    n_max, counts = chain_shape(model)
    run = Run(model, chain_rows(model, counts), n_max, n_max, chains(counts), CHAIN_GRID, lds_steps=1)
    try:
        got = chain_sequence(run)
        assert run.ens.lds_step_launches == 2
        same(want[0], got[0], counts, "1 step")
        same(want[1], got[1], counts, "5 steps from a non-zero old_v")
        unused = np.arange(n_max)[None, :] >= np.asarray(counts)[:, None]
        assert np.all(got[1][0][unused] == UNUSED)
        assert np.array_equal(bits(got[1][1])[unused], bits(start_v(len(counts), n_max))[unused])
        # the links did something: without them the same steps end elsewhere
        bare = Run(model, chain_rows(model, counts), n_max, n_max, [[] for _ in counts], CHAIN_GRID, lds_steps=1)
        try:
            bare.ens.take_step(SMALL_DT, 1)
            assert not np.array_equal(bits(bare.state()[0][-1]), bits(got[0][0][-1]))
        finally:
            bare.close()
    finally:
        run.close()


def test_an_eight_float_point_of_1024_rows_never_steps_from_lds():
    """relu_cell8_links at n_max = 1024: the rule gives 0 even for a list of no slots, so lds_steps = 1 runs the 14
    launches -- 0 launches counted, the twin's bits -- whatever S is."""
    assert lds_layout(8, 1024, True, 0).bytes == 0 and LinkedGridEnsemble.lds_bytes("relu_cell8_links", 1024, 0) == 0
    rows = [box_rows(n, 8, CHAIN_GRID, 40 + r) for r, n in enumerate([1024, 70])]
    for slots in (0, 64):
        pair = Pair("relu_cell8_links", rows, 1024, slots, [random_links(len(X), slots, 3) for X in rows], CHAIN_GRID)
        try:
            pair.step(SMALL_DT, 2, 0, ("S", slots))
        finally:
            pair.close()


# ---- hubs: the order of a cell's terms matters ----------------------------------------------------------------------
HUB_COUNTS = [300, 280, 300]
HUB_GRID, HUB_CUBE = 12, 0.8
HUB_STRENGTH = 0.05


def hub_links(n, seed):
    """LOCAL pairs from slot 0 on, and which of them count: cell 0, the hub, linked with 210 other cells, as end a
    of some of its links and as end b of the others (more than 100 of each), an inert slot (a == b) after every third
    of them, then doubled links and links among the others.  Every end lies inside the replica."""
    pairs = []
    for k in range(1, 211):
        pairs.append((0, k) if k % 2 else (k, 0))
        if k % 3 == 0:
            pairs.append((k, k))
    pairs += [(0, 5), (0, 5), (7, 3), (3, 7), (1, 1)] + [tuple(p) for p in random_links(n, 60, seed)]
    pairs = np.array(pairs).reshape(-1, 2)
    as_a = int(((pairs[:, 0] == 0) & (pairs[:, 1] != 0)).sum())
    as_b = int(((pairs[:, 1] == 0) & (pairs[:, 0] != 0)).sum())
    assert as_a >= 100 and as_b >= 100 and (pairs >= 0).all() and (pairs < n).all()
    return pairs, pairs[:, 0] != pairs[:, 1]


def hub_rows(seed=0):
    """~300 cells in a ball of radius ~2.9 around the origin, the hub at its centre: several cubes of 0.8 each way."""
    rows = [seeded_rows(3, n, 5000 + 10 * seed + r) for r, n in enumerate(HUB_COUNTS)]
    for X in rows:
        X[0] = (0.05, -0.03, 0.02)
    return rows


@pytest.mark.parametrize("model", ["links", "springs_links"])
def test_hubs_bit_for_bit_and_against_the_oracle(oracle, model):
    """A hub of more than 100 terms on either end of its links, interleaved with inert slots, in replicas of ~300 cells
    over several cubes of size 0.8: 1 step, then 5 more, during which cells cross cube faces (asserted: the grid
    arrays change).  From LDS against the 14-launch twin (a) and the oracle's serial loop (c), fed the links that
    count in their order."""
    rows = hub_rows()
    links = [hub_links(n, 60 + r) for r, n in enumerate(HUB_COUNTS)]
    slots = max(len(p) for p, _ in links) + 5
    pair = Pair(model, rows, 300, slots, [p for p, _ in links], HUB_GRID, cube_size=HUB_CUBE, strength=HUB_STRENGTH)
    try:
        first = pair.step(DT, 1, 1, "1 step")
        last = pair.step(DT, 5, 1, "5 more steps")
        no_nan(last)
        for r, n in enumerate(HUB_COUNTS):
            assert len(np.unique(first[3][r][0][:n])) >= 27, "several cubes"
            assert not same_grid(first[3][r], last[3][r], n), ("no cell of replica", r, "crossed a cube face")
    finally:
        pair.close()
    for r, n in enumerate(HUB_COUNTS):
        pairs, counted = links[r]
        with Solution(model + "_grid", 300, HUB_GRID, HUB_CUBE, lib=oracle) as s:
            assert s.set_reduce_order(1) == 0
            s.h_X[:n] = rows[r]
            s.h_n = n
            s.copy_to_device()
            s.set_links(pairs[counted], HUB_STRENGTH)
            for k, (steps, state) in enumerate(((1, first), (5, last))):
                s.take_step(DT, steps)
                assert np.array_equal(bits(s.positions()), bits(state[0][r, :n])), (r, k)
                assert np.array_equal(bits(s.old_v()[:n]), bits(state[1][r, :n])), (r, k)
                assert same_grid(s.grid(), state[3][r], n), (r, k)


# ---- slots that must be skipped -------------------------------------------------------------------------------------
MIXED = [300, 70, 0, 64, 257, 5]
MIXED_GRID = 16


def mixed_rows(n_floats=3, seed=0):
    return [seeded_rows(n_floats, n, 1000 * seed + r) for r, n in enumerate(MIXED)]


def mixed_links(seed=0, per_cell=1):
    return [random_links(n, per_cell * n, 10 * seed + r) for r, n in enumerate(MIXED)]


def test_slots_that_name_rows_outside_their_replica_are_skipped():
    """Replica 1 (70 of 300 rows) holds, among good links, slots naming rows of replica 0 and of replica 2, rows >= n_r
    (unused rows of its own), rows >= n_replicas * n_max and negative ids: from LDS the twin's bits, and every replica
    -- replica 1 and its neighbours -- ends where a run WITHOUT those slots ends."""
    rows, good = mixed_rows(), mixed_links(1)
    n_max, m = 300, len(MIXED)
    stray = [(3, -n_max + 3), (-5, 4), (n_max + 1, 6), (7, 70), (299, 8), (9, (m - 1) * n_max + 2), (m * n_max, 10),
             (2 ** 31 - 1 - n_max, 11), (-2 ** 31 + 2 * n_max, 12)]  # (LOCAL to replica 1: + 300 = the global id)
    with_stray = [np.array(p) for p in good]
    mixed_in = []
    for k, p in enumerate(good[1]):  # a stray slot after every seventh good one
        mixed_in.append(tuple(p))
        if k % 7 == 0 and k // 7 < len(stray):
            mixed_in.append(stray[k // 7])
    assert len(mixed_in) == 70 + len(stray)
    with_stray[1] = np.array(mixed_in)
    pair = Pair("relu_links", rows, n_max, 300, with_stray, MIXED_GRID)
    clean = Run("relu_links", rows, n_max, 300, good, MIXED_GRID, lds_steps=1)
    try:
        got = pair.step(DT, 3, 1, "stray slots")
        clean.ens.take_step(DT, 3)
        assert clean.ens.lds_step_launches == 1
        same(clean.state(), got, MIXED, "a run without the stray slots")
        no_nan(got)
    finally:
        pair.close()
        clean.close()


def test_fewer_slots_in_use_and_none():
    """n_links below the slots that hold links: replica 4 keeps 100 of its slots, replica 5 none; then n_links = 0,
    the plain step.  The slots beyond the count still hold their ids."""
    pair = Pair("relu_links", mixed_rows(), 300, 300, mixed_links(2), MIXED_GRID)
    bare = Run("relu_links", mixed_rows(), 300, 300, [[] for _ in MIXED], MIXED_GRID, lds_steps=1)
    try:
        def use(count):
            def call(run):
                run.ens.n_links = count
                run.ens.copy_to_device()
            return call
        start = pair.lds.state()
        pair.each(use(4 * 300 + 100))
        some = pair.step(DT, 2, 1, "fewer slots in use")
        # and the count mattered: replica 5's links are off, replica 3's on
        bare.ens.take_step(DT, 2)
        none = bare.state()
        assert np.array_equal(bits(some[0][5]), bits(none[0][5])) and not np.array_equal(bits(some[0][3]), bits(none[0][3]))
        for run in (pair.lds, pair.twin):  # back to the start, no slot in use: the run without links
            run.ens.h_X[:] = start[0]
            run.ens.n_links = 0
            run.ens.copy_to_device()
            run.ens.set_old_v(start[1])
        same(none, pair.step(DT, 2, 1, "no slot in use"), MIXED, "a run without links")
    finally:
        pair.close()
        bare.close()


# ---- settings -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sum_order", [0, 1])
@pytest.mark.parametrize("model", ["springs_links", "relu_po_links"])
def test_both_summation_orders(model, sum_order):
    """A box filled to its outermost cubes, 1000 cells in 9^3 cubes, three links per cell."""
    counts = [1000, 513, 64]
    rows = [box_rows(n, N_FLOATS[model], 9, 70 + r) for r, n in enumerate(counts)]
    links = [random_links(n, 3 * n, 30 + r) for r, n in enumerate(counts)]
    pair = Pair(model, rows, 1000, 3000, links, 9, strength=0.05, sum_order=sum_order)
    try:
        pair.step(SMALL_DT, 3, 1, ("sum_order", sum_order))
    finally:
        pair.close()


@pytest.mark.parametrize("model", ["relu_links", "relu_po_links"])
def test_all_three_fixed_modes(model):
    pair = Pair(model, mixed_rows(N_FLOATS[model]), 300, 300, mixed_links(), MIXED_GRID)
    try:
        for what, change, steps in [("set_fixed()", None, 2),
                                    ("set_fixed(4)", lambda run: run.ens.set_fixed(4), 3),
                                    ("set_fixed_xy(2)", lambda run: run.ens.set_fixed_xy(2), 3),
                                    ("set_fixed(1) after xy", lambda run: run.ens.set_fixed(1), 2),
                                    ("set_fixed() after xy", lambda run: run.ens.set_fixed(), 2)]:
            if change:
                pair.each(change)
            no_nan(pair.step(DT, steps, 1, what))
    finally:
        pair.close()


@pytest.mark.parametrize("lds_steps_max", [1, 3])
def test_seven_steps_split_into_launches_equal_one_call(lds_steps_max):
    rows, links = mixed_rows(seed=1), mixed_links(1, 2)
    pair = Pair("relu_links", rows, 300, 600, links, MIXED_GRID, lds_steps_max=lds_steps_max)
    once = Run("relu_links", rows, 300, 600, links, MIXED_GRID, lds_steps=1)
    try:
        got = pair.step(DT, 7, -(-7 // lds_steps_max), ("lds_steps_max", lds_steps_max))
        once.ens.take_step(DT, 7)
        assert once.ens.lds_step_launches == 1
        same(once.state(), got, MIXED, "one call, one launch")
    finally:
        pair.close()
        once.close()


def test_the_largest_list_that_fits_and_one_beyond():
    """n_max = 1024 of float3: the largest S the rule admits -- the workgroup's whole LDS -- runs from LDS; one slot
    more is the 14-launch loop with link_forces_ordered, 0 launches counted; both give the twin's bits."""
    fits = largest_slots(3, 1024, keys=True)
    assert lds_layout(3, 1024, True, fits).bytes > 0 and lds_layout(3, 1024, True, fits + 1).bytes == 0
    counts = [1024, 500]
    rows = [box_rows(n, 3, CHAIN_GRID, 80 + r) for r, n in enumerate(counts)]
    links = [random_links(n, fits, 20 + r) for r, n in enumerate(counts)]  # every slot in use: ten links per cell
    states = []
    for slots, launches in ((fits, 1), (fits + 1, 0)):
        assert LinkedGridEnsemble.lds_bytes("links", 1024, slots) == lds_layout(3, 1024, True, slots).bytes
        pair = Pair("links", rows, 1024, slots, links, CHAIN_GRID, strength=0.01)
        try:
            states.append(pair.step(SMALL_DT, 2, launches, ("S", slots)))
        finally:
            pair.close()
    no_nan(states[0])
    same(states[0], states[1], counts, "one slot beyond")


def test_links_rewritten_and_cube_size_changed_between_calls():
    """What copy_to_device hands over before a call is what the call's launches see; cube_size holds from the next
    call on; lds_steps switched on the same object, and take_step with the links' 14-launch path in between."""
    pair = Pair("relu_links", mixed_rows(seed=2), 300, 300, mixed_links(2), MIXED_GRID)
    try:
        pair.step(DT, 2, 1, "the first links")

        def renew(run):
            run.ens.copy_to_host()
            run.set_links(mixed_links(3))
            run.ens.copy_to_device()
        pair.each(renew)
        before = pair.lds.state()
        after = pair.step(DT, 2, 1, "other links")

        def cube(run):
            run.ens.cube_size = 1.25
        pair.each(cube)
        pair.step(DT, 3, 1, "cube_size 1.25")
        pair.lds.ens.set_param("lds_steps", -1)
        pair.step(DT, 2, 0, "the 14 launches on the same object")
        pair.lds.ens.set_param("lds_steps", 1)
        pair.step(DT, 1, 1, "from LDS again")
        # and the links mattered: the first links from the same state end elsewhere
        other = Run("relu_links", mixed_rows(seed=2), 300, 300, mixed_links(2), MIXED_GRID, lds_steps=1)
        try:
            other.ens.h_X[:] = before[0]
            other.ens.copy_to_device()
            other.ens.set_old_v(before[1])
            other.ens.take_step(DT, 2)
            assert not np.array_equal(bits(other.state()[0][0]), bits(after[0][0]))
        finally:
            other.close()
    finally:
        pair.close()


def test_a_cell_outside_the_grid_raises_its_replicas_status_bit_on_both_paths():
    """Replica 2 starts with one cell beyond the top face of its 8^3 grid: clamped into it, its bit raised on both
    paths, the results the twin's; the other replicas' bits stay clear."""
    counts = [100, 64, 257, 30]
    rows = [seeded_rows(3, n, 90 + r) for r, n in enumerate(counts)]
    rows[2][5] = (0.0, 0.0, 4.25)
    links = [random_links(n, n, 50 + r) for r, n in enumerate(counts)]
    pair = Pair("relu_links", rows, 300, 300, links, 8)
    try:
        got = pair.step(DT, 3, 1, "beside a replica outside its grid", in_grid=False)
        assert [s != 0 for s in got[2]] == [False, False, True, False]
        assert [pair.lds.ens.status(r) for r in range(4)] == [0, 0, 0, 0]  # forgotten
    finally:
        pair.close()


# ---- many replicas, and their independence --------------------------------------------------------------------------
def test_three_hundred_replicas_of_forty_cells():
    m, n_max = 300, 40
    rng = np.random.default_rng(11)
    counts = rng.integers(0, n_max + 1, size=m)
    counts[[0, 1, 299]] = [40, 0, 40]
    rows = [seeded_rows(3, int(n), 7000 + r) for r, n in enumerate(counts)]
    links = [random_links(int(n), 80, r) for r, n in enumerate(counts)]
    pair = Pair("relu_links", rows, n_max, 80, links, 6)
    try:
        no_nan(pair.step(DT, 4, 1, "300 replicas"))
    finally:
        pair.close()


def test_replicas_are_independent():
    """Other links in replica 1 change replica 1 alone."""
    rows, links = mixed_rows(seed=4), mixed_links(4)
    changed = list(links)
    changed[1] = random_links(70, 70, 99)
    a = Run("relu_links", rows, 300, 300, links, MIXED_GRID, lds_steps=1)
    b = Run("relu_links", rows, 300, 300, changed, MIXED_GRID, lds_steps=1)
    try:
        for run in (a, b):
            run.ens.take_step(DT, 3)
            assert run.ens.lds_step_launches == 1
        sa, sb = a.state(), b.state()
        same(sa, sb, MIXED, "the other replicas", replicas=[0, 2, 3, 4, 5])
        assert not np.array_equal(bits(sa[0][1, :70]), bits(sb[0][1, :70]))
    finally:
        a.close()
        b.close()


def test_parameters_are_validated():
    with LinkedGridEnsemble("relu_links", 2, 10, 10, grid_size=6) as ens:
        for name, good, bad in [("links_path", (0, 1), (-1, 2, 0.5)), ("lds_steps", (-1, 0, 1), (2, -2, 0.5)),
                                ("sum_order", (0, 1), (-1, 2)), ("lds_steps_max", (1, 256), (0, -1, 1.5))]:
            for value in good:
                assert ens.set_param(name, value) == 0
            for value in bad:
                with pytest.raises(YallaError, match="-3"):
                    ens.set_param(name, value)
        for name in ("lanes", "whole_steps", "gabriel_coefficient"):
            with pytest.raises(YallaError, match="-2"):
                ens.set_param(name, 1)
        assert ens.n_links == 20
        for value in (-1, 21):
            with pytest.raises(YallaError, match="-3"):
                ens.n_links = value
        # links_path = 1 never steps from LDS, whatever lds_steps says
        ens.set_param("lds_steps", 1)
        ens.set_param("links_path", 1)
        ens.h_X[:] = seeded_rows(3, 20, 1).reshape(2, 10, 3)
        ens.h_n[:] = [10, 10]
        ens.h_link[:, 0] = [[0, 1], [10, 11]]
        ens.copy_to_device()
        ens.take_step(DT, 2)
        assert ens.lds_step_launches == 0
        ens.set_param("links_path", 0)
        ens.take_step(DT, 2)
        assert ens.lds_step_launches == 1
    with LinkedGridEnsemble("links", 3, 10, 0, grid_size=6) as none:  # no slots at all: the plain step, from LDS
        assert none.h_link.shape == (3, 0, 2) and none.n_links == 0
        none.set_param("lds_steps", 1)
        none.h_X[:] = seeded_rows(3, 30, 2).reshape(3, 10, 3)
        none.h_n[:] = [10, 10, 10]
        none.copy_to_device()
        none.take_step(DT, 2)
        assert none.lds_step_launches == 1
