"""What the tests of several lanes per cell inside the grid ensemble's launches that step from LDS share
(tests/test_ensemble_grid_lds_lanes*.py): which term of the LDS rule (ensemble_support.lds_layout) decides the
term buffer's tile and where that changes, and `Lanes`: one GridEnsemble per lane setting, fed the
same rows, beside THE REFERENCES -- the same object type with lds_step_lanes = 1 (today's kernel) and the 14-launch
twin (GridTwins).  A plain module, imported as tests/ensemble_support.py is."""
import numpy as np
from ensemble_grid_lds_support import GridTwins
from ensemble_support import LDS, STATIC_LDS, bits, lds_layout, same_grid, tile_behind

from yalla_amd.ensemble import GridEnsemble

LANES = (4, 16, 64)


# ---- the rule -------------------------------------------------------------------------------------------------------
def coop_binding(n_floats, n_max, lanes):
    """Which term of the rule decides the tile length: 0 = n_max rounded up to 4, 1 = the longest tile, 2 = the budget
    (or the shortest tile in its place), 3 = the room left in the workgroup's LDS (the first of those that are equal),
    -1 = no room at all."""
    _, tile, _, bounds = tile_behind(lds_layout(n_floats, n_max, keys=True).terms, n_floats, n_max, lanes)
    return bounds.index(min(bounds)) if tile else -1


def rule_edges(n_floats, lanes_of=LANES, up_to=1024):
    """Every n_max either side of a point where another term of the rule starts to decide, for any of the lanes."""
    edges = set()
    for lanes in lanes_of:
        for n_max in range(2, up_to + 1):
            if coop_binding(n_floats, n_max, lanes) != coop_binding(n_floats, n_max - 1, lanes):
                edges |= {n_max - 1, n_max}
    return sorted(edges)


def links_rule_binding(n_floats, n_max, slots_of, lanes):
    """What decides the linked rule at slots_of(n_max) slots: -2 = the list does not fit (never from LDS), -1 = not 16
    candidates' terms behind it (one lane), 0 .. 3 = the bound that cut the tile length last."""
    slots = slots_of(n_max)
    if lds_layout(n_floats, n_max, True, slots).bytes == 0:
        return -2
    base = lds_layout(n_floats, n_max, True, slots).terms
    if base + STATIC_LDS > LDS:
        return -1
    return tile_behind(base, n_floats, n_max, lanes)[2]


def links_rule_edges(n_floats, slots_of, lanes_of=LANES, up_to=1024):
    """rule_edges for linked launches of slots_of(n_max) slots per replica."""
    edges = set()
    for lanes in lanes_of:
        for n_max in range(2, up_to + 1):
            if links_rule_binding(n_floats, n_max, slots_of, lanes) != links_rule_binding(
                    n_floats, n_max - 1, slots_of, lanes):
                edges |= {n_max - 1, n_max}
    return sorted(edges)


def lanes_for(n_max):
    """ya::ens::grid_lds_lanes_for: the engine's choice for stateless functors."""
    return 16 if n_max <= 32 else 4 if n_max <= 64 else 1


# the harness models whose pair is stateless (ya::stateless_pair: the force declared YA_STATELESS in
# yalla_amd/csrc/model_functors.h, the friction a default one or declared): what lds_step_lanes = 0 may give several
# lanes.  Not among them: no_pw_int (push, links, links4), ids_friction_plain, relu_force of the 8-float point.
STATELESS = {"springs", "clipped", "fading", "relu", "relu_po", "relu_cell", "friction_ids", "friction_field",
             "springs_links", "relu_links", "relu_po_links"}


def lanes_expected(model, n_floats, n_max, setting, slots=None):
    """lds_step_lanes_used after a launch from LDS under lds_step_lanes = setting."""
    lanes = setting
    if lanes == 0:
        lanes = lanes_for(n_max) if model in STATELESS else 1
    if lanes == 1:
        return 1
    room = lds_layout(n_floats, n_max, True, slots, lanes).bytes
    return lanes if room else 1


# ---- one ensemble per lane setting -----------------------------------------------------------------------------------
def state_of(ens, counts):
    """Every replica's status (read and forgotten, so that copy_to_host can run), EVERY row of the positions and of
    old_v, every replica's four grid arrays."""
    status = [ens.status(r) for r in range(len(counts))]
    ens.copy_to_host()
    assert list(ens.h_n) == list(counts)
    return ens.h_X.copy(), ens.old_v(), status, [ens.grid(r) for r in range(len(counts))]


def same_state(a, b, counts, what=""):
    (Xa, va, sa, ga), (Xb, vb, sb, gb) = a, b
    assert sa == sb, (what, "status", sa, sb)
    assert np.array_equal(bits(Xa), bits(Xb)), (what, "positions")
    assert np.array_equal(bits(va), bits(vb)), (what, "old_v")
    for r, n in enumerate(counts):
        assert same_grid(ga[r], gb[r], n), (what, "grid arrays of replica", r)


class Lanes:
    """GridTwins (`base`: its `ens` steps from LDS with lds_step_lanes = 1, its `twin` is the 14-launch path, its
    lone Solutions where asked for) and one more GridEnsemble per setting of `settings`, lds_steps = 1 and
    lds_step_lanes = that, fed the same rows.  step() asserts the launches counted and lds_step_lanes_used on every
    object; check() holds the one-lane launches against the twin (GridTwins.check) and every setting's positions, old_v,
    status and grid arrays against the one-lane launches', on bit patterns."""

    def __init__(self, model, counts, n_max, grid_size, cube_size=1.0, rows=None, settings=LANES, seed=0, singles=()):
        self.model, self.counts, self.n_max = model, list(counts), n_max
        self.base = GridTwins(model, counts, n_max, grid_size, cube_size, seed=seed, singles=singles, rows=rows)
        self.base.ens.set_param("lds_step_lanes", 1)
        self.lanes = {}
        for setting in settings:
            ens = GridEnsemble(model, len(counts), n_max, grid_size, cube_size)
            ens.set_param("lds_steps", 1)
            ens.set_param("lds_step_lanes", setting)
            ens.h_X[:] = self.base.ens.h_X
            ens.h_n[:] = counts
            ens.copy_to_device()
            assert ens.lds_step_lanes_used == 0
            self.lanes[setting] = ens
        self.seen = {setting: 0 for setting in settings}

    def each(self, call):
        self.base.each(call)
        for ens in self.lanes.values():
            call(ens)

    def set_old_v(self, v):
        self.base.set_old_v(v)
        for ens in self.lanes.values():
            ens.set_old_v(v)

    def set_sum_order(self, order):
        self.each(lambda s: s.set_param("sum_order", order))

    def set_cube_size(self, cube_size):
        def assign(s):
            s.cube_size = cube_size
        self.each(assign)

    def used(self, setting):
        return lanes_expected(self.model, self.base.ens.n_floats, self.n_max, setting)

    def step(self, dt, steps=1, launches=None):
        self.base.step(dt, steps, launches=launches)
        made = self.base.ens.lds_step_launches  # (GridTwins asserted what this call added)
        if launches != 0:
            assert self.base.ens.lds_step_lanes_used == 1
        for setting, ens in self.lanes.items():
            before = ens.lds_step_launches
            ens.take_step(dt, steps)
            assert ens.lds_step_launches - before == made - self.seen[setting], (self.model, setting, "launches")
            self.seen[setting] = made
            if ens.lds_step_launches:
                assert ens.lds_step_lanes_used == self.used(setting), (self.model, setting, ens.lds_step_lanes_used)
            else:
                assert ens.lds_step_lanes_used == 0

    def check(self, what="", in_grid=True):
        status = self.base.check(what, in_grid=in_grid)  # (reads and forgets the statuses of ens and twin)
        want = (self.base.ens.h_X.copy(), self.base.ens.old_v(), status,
                [self.base.ens.grid(r) for r in range(len(self.counts))])
        for setting, ens in self.lanes.items():
            same_state(want, state_of(ens, self.counts), self.counts, (what, self.model, "lds_step_lanes", setting))
        return status

    def close(self):
        self.base.close()
        for ens in self.lanes.values():
            ens.close()
