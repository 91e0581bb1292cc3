"""What the tests of linked grid ensembles share (tests/test_ensemble_grid_links*.py): the model table and a
LinkedGridEnsemble with lds_steps = 1 beside its twin
with lds_steps = -1.  A plain module, imported as tests/ensemble_support.py is."""
import numpy as np
from ensemble_grid_lds_support import UNUSED
from ensemble_support import bits, same_grid

MODELS = ["links", "links4", "springs_links", "relu_links", "relu_po_links", "relu_cell8_links"]
N_FLOATS = {"links": 3, "links4": 4, "springs_links": 3, "relu_links": 3, "relu_po_links": 5, "relu_cell8_links": 8}


def box_rows(n, n_floats, grid_size, seed, shrink=0.92, cube_size=1.0):
    """Uniform over the grid's box drawn `shrink` towards the origin (the outermost cubes stay populated, nobody is
    pushed out within a test's few steps); further components uniform in [0, 1)."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, n_floats), np.float32)
    lo = -(grid_size // 2)
    rows[:, :3] = ((lo + grid_size * rng.random((n, 3))) * 0.999 * shrink * cube_size).astype(np.float32)
    rows[:, 3:] = rng.random((n, n_floats - 3)).astype(np.float32)
    return rows


def random_links(n, count, seed):
    """`count` links between distinct cells of 0 .. n - 1 (none for n < 2)."""
    rng = np.random.default_rng(seed)
    if n < 2:
        return np.zeros((0, 2), np.int64)
    a = rng.integers(0, n, count)
    b = (a + 1 + rng.integers(0, n - 1, count)) % n
    return np.stack([a, b], axis=1)


class Run:
    """A LinkedGridEnsemble fed `rows` (one array per replica; unused rows hold a pattern of their own) and
    per-replica links given as LOCAL (a, b) pairs from slot 0 on (every other slot inert)."""

    def __init__(self, model, rows, n_max, slots, links, grid_size, cube_size=1.0, strength=0.2, n_links=None, **params):
        from yalla_amd.ensemble import LinkedGridEnsemble
        self.counts = [len(X) for X in rows]
        self.ens = LinkedGridEnsemble(model, len(rows), n_max, slots, strength, grid_size, cube_size)
        for name, value in params.items():
            self.ens.set_param(name, value)
        self.ens.h_X[:] = UNUSED
        for r, X in enumerate(rows):
            self.ens.h_X[r, :len(X)] = X
            self.ens.h_n[r] = len(X)
        self.set_links(links, n_links)
        self.ens.copy_to_device()

    def set_links(self, links, n_links=None):
        """GLOBAL ids = local + r * n_max, whatever the local ones are (a test may point outside the replica)."""
        ens = self.ens
        ens.h_link[:] = 0
        for r, pairs in enumerate(links):
            pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
            ens.h_link[r, :len(pairs)] = pairs + r * ens.n_max
        ens.n_links = ens.n_replicas * ens.slots_per_replica if n_links is None else n_links

    def state(self):
        """Every replica's status (read and forgotten, so that copy_to_host can run), EVERY row of the positions and
        of old_v, every replica's four grid arrays."""
        status = [self.ens.status(r) for r in range(len(self.counts))]
        self.ens.copy_to_host()
        assert list(self.ens.h_n) == self.counts
        return self.ens.h_X.copy(), self.ens.old_v(), status, [self.ens.grid(r) for r in range(len(self.counts))]

    def close(self):
        self.ens.close()


def same(a, b, counts, what="", replicas=None):
    """Two states, bit for bit: positions and old_v of every row, every replica's status and grid arrays
    (replicas: only those)."""
    (Xa, va, sa, ga), (Xb, vb, sb, gb) = a, b
    which = range(len(counts)) if replicas is None else replicas
    for r in which:
        assert np.array_equal(bits(Xa[r]), bits(Xb[r])), (what, "positions of replica", r)
        assert np.array_equal(bits(va[r]), bits(vb[r])), (what, "old_v of replica", r)
        assert sa[r] == sb[r], (what, "status of replica", r, sa[r], sb[r])
        assert same_grid(ga[r], gb[r], counts[r]), (what, "grid arrays of replica", r)


def no_nan(state):
    assert not np.isnan(state[0]).any() and not np.isnan(state[1]).any()


class Pair:
    """The same linked grid ensemble twice: `lds` with lds_steps = 1, and `twin` with lds_steps = -1, THE REFERENCE
    (the 14-launch step with ya::ens::link_forces_ordered).  step() asserts which path ran and compares everything."""

    def __init__(self, model, rows, n_max, slots, links, grid_size, **kw):
        self.counts = [len(X) for X in rows]
        self.lds = Run(model, rows, n_max, slots, links, grid_size, lds_steps=1, **kw)
        self.twin = Run(model, rows, n_max, slots, links, grid_size, lds_steps=-1, **kw)
        self.seen = 0

    def each(self, call):
        call(self.lds)
        call(self.twin)

    def step(self, dt, steps, launches, what="", in_grid=True):
        self.each(lambda run: run.ens.take_step(dt, steps))
        made = self.lds.ens.lds_step_launches - self.seen
        assert made == launches, (what, "launches", made, "expected", launches)
        self.seen = self.lds.ens.lds_step_launches
        assert self.twin.ens.lds_step_launches == 0
        want, got = self.twin.state(), self.lds.state()
        same(want, got, self.counts, what)
        if in_grid:
            assert not any(want[2]), (what, "a replica left its grid", want[2])
        return got

    def close(self):
        self.lds.close()
        self.twin.close()
