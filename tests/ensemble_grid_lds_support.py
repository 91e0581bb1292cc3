"""What the tests of the grid ensemble's launches that step from LDS share (tests/test_ensemble_grid_lds_steps*.py): the
capacity by the LDS rule (ensemble_support.lds_layout), and a GridEnsemble with lds_steps = 1 beside its twin with
lds_steps = -1 (and lone Solutions where asked for).  A plain module, imported as tests/ensemble_support.py is."""
import numpy as np
from ensemble_support import LDS, STATIC_LDS, Lockstep, bits, lds_layout, same_grid

from yalla_amd.ensemble import GridEnsemble

MAX_ROWS = 1024
UNUSED = np.float32(-7.25)  # what rows past a replica's count hold, to be found again


def grid_lds_capacity(n_floats):
    """ya::ens::grid_lds_capacity: the largest n_max <= 1024 whose launch, the fold's static scratch included, fits a
    workgroup's 160 KiB."""
    return max(n for n in range(1, MAX_ROWS + 1) if lds_layout(n_floats, n, keys=True).bytes + STATIC_LDS <= LDS)


def launches_of(model, steps, n_max, n_floats=3, lds_steps_max=256):
    """What take_step(dt, steps) must report with lds_steps = 1."""
    if model in ("push", "clipped_push") or n_max > grid_lds_capacity(n_floats):
        return 0
    return -(-steps // lds_steps_max)


class GridTwins(Lockstep):
    """A GridEnsemble with lds_steps = 1 (`ens`), the same rows in a GridEnsemble with lds_steps = -1 (`twin`, THE
    REFERENCE: the 14-launch path), and a lone Solution("<model>_grid") for each replica of `singles`.  Unused rows
    hold a pattern of their own.  step() asserts which path ran; check() compares EVERY row of the positions, old_v,
    the counts, every replica's status and every replica's grid arrays, all on bit patterns."""

    def __init__(self, model, counts, n_max, grid_size, cube_size=1.0, seed=0, singles=(), rows=None, lds_steps=1):
        super().__init__(GridEnsemble, "_grid", model, counts, n_max, (grid_size, cube_size), grids=True, seed=seed,
                         singles=list(singles), rows=rows)
        self.ens.set_param("lds_steps", lds_steps)
        self.twin = GridEnsemble(model, len(counts), n_max, grid_size, cube_size)
        self.twin.set_param("lds_steps", -1)
        unused = np.arange(n_max)[None, :] >= np.asarray(counts)[:, None]
        self.ens.h_X[unused] = UNUSED
        self.twin.h_X[:] = self.ens.h_X
        self.twin.h_n[:] = counts
        self.ens.copy_to_device()
        self.twin.copy_to_device()
        self.seen = 0
        self.lds_steps_max = 256

    def each(self, call):
        super().each(call)
        call(self.twin)

    def set_old_v(self, v):
        super().set_old_v(v)
        self.twin.set_old_v(v)

    def set_counts(self, new):
        old = list(self.counts)
        self.twin.copy_to_host()
        super().set_counts(new)
        for r, n in new.items():
            self.twin.h_X[r, old[r]:n] = self.ens.h_X[r, old[r]:n]
            self.twin.h_n[r] = n
        self.twin.copy_to_device()

    def step(self, dt, steps=1, launches=None):
        """launches: what `ens` must report for this call (default: launches_of the model); the twin never makes one."""
        super().step(dt, steps)
        if launches is None:
            launches = launches_of(self.model, steps, self.n_max, self.ens.n_floats, self.lds_steps_max)
        made = self.ens.lds_step_launches - self.seen
        assert made == launches, (self.model, "launches", made, "expected", launches)
        self.seen = self.ens.lds_step_launches
        assert self.twin.lds_step_launches == 0

    def statuses(self, clear=True):
        """Every replica's status on both sides (equal), forgotten unless clear=False so that copy_to_host can run."""
        mine = [self.ens.status(r, clear=clear) for r in range(len(self.counts))]
        theirs = [self.twin.status(r, clear=clear) for r in range(len(self.counts))]
        assert mine == theirs, ("status", mine, theirs)
        return mine

    def check(self, what="", in_grid=True):
        status = self.statuses()
        if in_grid:
            assert not any(status), (what, "a replica left its grid", status)
        if self.single:
            assert not any(status[r] for r in self.single), what
            super().check(what)  # the lone Solutions: used rows, old_v, grid arrays
        self.ens.copy_to_host()
        self.twin.copy_to_host()
        assert list(self.twin.h_n) == list(self.ens.h_n) == list(self.counts), what
        for r in range(len(self.counts)):
            assert self.ens.get_d_n(r) == self.twin.get_d_n(r) == self.counts[r], (what, r)
        assert np.array_equal(bits(self.twin.h_X), bits(self.ens.h_X)), (what, self.model, "positions")
        assert np.array_equal(bits(self.twin.old_v()), bits(self.ens.old_v())), (what, self.model, "old_v")
        for r, n in enumerate(self.counts):
            assert same_grid(self.ens.grid(r), self.twin.grid(r), n), (what, self.model, "grid arrays of replica", r, n)
        return status

    def close(self):
        super().close()
        self.twin.close()
