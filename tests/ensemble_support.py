"""What the ensemble suites (tests/test_ensemble*.py) share: seeded rows and bit comparisons, an ensemble and its
lone Solutions in lock-step, the whole-step twins, THE LDS RULE of every launch that steps from LDS restated once,
the three checks of a harness library's C ABI, and the runner of the native programs.  A plain module, imported as
tests/kats.py is; the suites keep their cases, shapes and literal expectations."""
import collections
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_ensemble")

DT = 0.05
# the all-pairs models whose steps can run whole (no generic forces); `push` must fall back
WHOLE = ["springs", "clipped", "fading", "relu", "relu_po", "oscillator"]
# the rows of user-written frictions in the three unlinked harnesses' tables (tests/test_friction_functors_gpu.py steps them)
FRICTION_MODELS = ["friction_ids", "friction_ids_plain", "friction_field"]
LINKED_MODELS = ["links", "links4", "springs_links", "relu_links", "relu_po_links"]
LINKED_N_FLOATS = {"links": 3, "links4": 4, "springs_links": 3, "relu_links": 3, "relu_po_links": 5}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def seeded_rows(n_floats, n, seed, lone=False):
    """random_sphere-like: n points uniform in a ball whose density is that of random_sphere(0.75); further
    components (w, theta / phi, ...) uniform in [0, 1).  lone: the first one moved far away, a lone cell."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, n_floats), dtype=np.float32)
    if n == 0:
        return rows
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    radius = 0.75 * (n / 0.64) ** (1 / 3) / 2 * rng.random(n) ** (1 / 3)
    rows[:, :3] = (direction * radius[:, None]).astype(np.float32)
    rows[:, 3:] = rng.random((n, n_floats - 3)).astype(np.float32)
    if lone:
        rows[0, :3] = rows[:, :3].max(axis=0) + 3.0
    return rows


def same_grid(mine, theirs, n):
    """cube_id[:n], point_id[:n], and every cube's cube_start and cube_end"""
    return (np.array_equal(mine[0][:n], theirs[0][:n]) and np.array_equal(mine[1][:n], theirs[1][:n])
            and np.array_equal(mine[2], theirs[2]) and np.array_equal(mine[3], theirs[3]))


# ---- an ensemble and its lone Solutions ------------------------------------------------------------------------------
class Lockstep:
    """An ensemble -- ensemble(model, M, n_max, *args, *ens_args) -- and one Solution(<single_model or model> +
    suffix, n_max, *args) per compared replica (`singles`, default all), fed the same rows (`rows`, default
    seeded_rows with seed 1000 * seed + r), old_v and settings.  grids: the four grid arrays are part of a result.
    lib / single_lib: the libraries of the ensemble and of the Solutions where they are not the classes' own."""

    def __init__(self, ensemble, suffix, model, counts, n_max, args=(), ens_args=(), grids=False, seed=0,
                 singles=None, rows=None, single_model=None, lib=None, single_lib=None):
        from yalla_amd.solution import Solution
        self.model, self.n_max, self.grids = model, n_max, grids
        self.ens = ensemble(model, len(counts), n_max, *args, *ens_args, **({} if lib is None else {"lib": lib}))
        self.which = list(range(len(counts))) if singles is None else list(singles)
        self.single = {r: Solution((single_model or model) + suffix, n_max, *args, lib=single_lib) for r in self.which}
        self.counts = list(counts)
        for r, n in enumerate(counts):
            X = seeded_rows(self.ens.n_floats, n, 1000 * seed + r) if rows is None else rows[r]
            self.ens.h_X[r, :n] = X
            self.ens.h_n[r] = n
            if r in self.single:
                self.single[r].h_X[:n] = X
                self.single[r].h_n = n
        self.ens.copy_to_device()
        for s in self.single.values():
            s.copy_to_device()

    def each(self, call):
        call(self.ens)
        for s in self.single.values():
            call(s)

    def step(self, dt, steps=1):
        self.each(lambda s: s.take_step(dt, steps))

    def set_old_v(self, v):
        """v: (n_replicas, n_max, 3)"""
        self.ens.set_old_v(v)
        for r, s in self.single.items():
            s.set_old_v(v[r])

    def set_cube_size(self, cube_size):
        def assign(s):
            s.cube_size = cube_size
        self.each(assign)

    def set_sum_order(self, order):
        self.each(lambda s: s.set_param("sum_order", order))

    def set_counts(self, new):
        """h_n[r] changed on the host: the rows travel with it, as copy_to_device moves them (both sides hold
        the same rows, a replica that grows gets fresh ones at its end)."""
        self.ens.copy_to_host()
        for s in self.single.values():
            s.copy_to_host()
        for r, n in new.items():
            grown = seeded_rows(self.ens.n_floats, max(n - self.counts[r], 0), 77 + r)
            self.ens.h_X[r, self.counts[r]:n] = grown
            self.ens.h_n[r] = n
            if r in self.single:
                self.single[r].h_X[self.counts[r]:n] = grown
                self.single[r].h_n = n
            self.counts[r] = n
        self.ens.copy_to_device()
        for s in self.single.values():
            s.copy_to_device()

    def results(self):
        """Per compared replica: (positions, old_v[:n], grid arrays or None) of its Solution."""
        out = {}
        for r, s in self.single.items():
            n = self.counts[r]
            assert s.h_n == n
            out[r] = (bits(s.positions()).copy(), bits(s.old_v()[:n]).copy(), s.grid() if self.grids else None)
        return out

    def check(self, what="", reference=None):
        reference = self.results() if reference is None else reference
        compare(self.ens, self.counts, reference, (what, self.model))

    def close(self):
        self.ens.close()
        for s in self.single.values():
            s.close()


def compare(ens, counts, reference, what=""):
    """The ensemble's replicas against `reference` (Lockstep.results): h_n, get_d_n, positions, old_v[:n], and the
    four grid arrays where the reference holds them."""
    ens.copy_to_host()
    v = ens.old_v()
    for r, (X, old_v, grid) in reference.items():
        n = counts[r]
        assert ens.h_n[r] == n and ens.get_d_n(r) == n, (what, r)
        assert np.array_equal(bits(ens.h_X[r, :n]), X), (what, "positions of replica", r, n)
        assert np.array_equal(bits(v[r, :n]), old_v), (what, "old_v of replica", r, n)
        assert grid is None or same_grid(ens.grid(r), grid, n), (what, "grid arrays of replica", r, n)


def capacity(n_floats):
    """ya::ens::whole_step_capacity<Pt>() restated from the header's formula: four point arrays and old_v per row,
    fold256's scratch, <= 4 partial sums, and the 3 x 256 floats ya::fixed_velocity_from_partials folds in, within a
    workgroup's 160 KiB; at most 1024 rows."""
    return min((LDS - whole_step_bytes(n_floats, 0) - STATIC_LDS) // (4 * 4 * n_floats + 12), 1024)


def grid_capacity(n_floats):
    """ya::ens::grid_lds_capacity<Pt>() restated: the largest n_max <= 1024 whose step arrays and keys (one 64-bit key
    per row of the power of two from n_max up) fit a workgroup's 160 KiB beside the static fold scratch."""
    return max(n for n in range(1, 1025) if lds_layout(n_floats, n, keys=True).bytes + STATIC_LDS <= LDS)


def launches_of(model, steps, steps_per_launch=256):
    return 0 if model == "push" else -(-steps // steps_per_launch)


class Twins(Lockstep):
    """Lockstep's Ensemble with whole_steps = 1, its lone Solutions, and a second Ensemble of the same rows that keeps
    the six launches (whole_steps = -1).  Unused rows hold a pattern of their own, to be found again."""

    def __init__(self, model, counts, n_max, seed=0, singles=None):
        from yalla_amd.ensemble import Ensemble
        super().__init__(Ensemble, "_tile", model, counts, n_max, seed=seed, singles=singles)
        self.ens.set_param("whole_steps", 1)
        self.six = Ensemble(model, len(counts), n_max)
        self.six.set_param("whole_steps", -1)
        unused = np.arange(n_max)[None, :] >= np.asarray(counts)[:, None]
        self.ens.h_X[unused] = np.float32(-7.25)
        self.six.h_X[:] = self.ens.h_X
        self.six.h_n[:] = counts
        self.ens.copy_to_device()
        self.six.copy_to_device()
        self.seen = 0

    def each(self, call):
        super().each(call)
        call(self.six)

    def set_old_v(self, v):
        super().set_old_v(v)
        self.six.set_old_v(v)

    def set_counts(self, new):
        old = list(self.counts)
        self.six.copy_to_host()
        super().set_counts(new)
        for r, n in new.items():
            self.six.h_X[r, old[r]:n] = self.ens.h_X[r, old[r]:n]
            self.six.h_n[r] = n
        self.six.copy_to_device()

    def expect_launches(self, n, what=""):
        """whole_step_launches rose by n since the last look; the six-launch twin never made one."""
        assert self.ens.whole_step_launches - self.seen == n, (what, self.ens.whole_step_launches, self.seen, n)
        self.seen = self.ens.whole_step_launches
        assert self.six.whole_step_launches == 0

    def check(self, what=""):
        """Against the lone Solutions (used rows), and against the six-launch Ensemble: EVERY row, used or not."""
        super().check(what)
        self.six.copy_to_host()
        assert list(self.six.h_n) == list(self.ens.h_n), what
        assert np.array_equal(bits(self.six.h_X), bits(self.ens.h_X)), (what, self.model, "positions")
        assert np.array_equal(bits(self.six.old_v()), bits(self.ens.old_v())), (what, self.model, "old_v")

    def close(self):
        super().close()
        self.six.close()


# ---- THE LDS RULE of the launches that step a replica from LDS, restated once from ya::ens::lds_layout's comment -------
# (include/ensemble.cuh; the all-pairs whole steps and the grid form's lds steps, with links and several lanes per cell)
LDS, STATIC_LDS, MIN_TILE, MAX_TILE, BUDGET = 160 * 1024, 3 * 256 * 4, 16, 256, 32 * 1024
Layout = collections.namedtuple("Layout", "X1 dX dX1 old_v fold partials keys list terms tile bytes")


def up16(x):
    return -(-x // 16) * 16


def whole_step_bytes(n_floats, n_max):
    """The step's arrays (X, X1, dX, dX1, old_v), fold256's scratch, 4 partial sums."""
    return n_max * (4 * 4 * n_floats + 12) + n_floats * 256 * 4 + n_floats * 4 * 4


def tile_behind(base, n_floats, n_max, lanes):
    """The term buffer's rule for a buffer that starts at `base`, by its statements in their order: (bytes per partner,
    tile length, which bound cut last, the four bounds).  The tile is n_max rounded up to 4 (0); at most the longest
    tile (1); at most what the budget holds but no less than the shortest tile where it cuts (2); at most the room left
    in the workgroup's LDS (3).  Tile 0 and which -1: the shortest tile has no room."""
    per_partner = (256 // lanes) * (n_floats + 4) * 4
    room = (LDS - STATIC_LDS - base) // per_partner // 4 * 4
    budget = BUDGET // per_partner // 4 * 4
    bounds = [-(-n_max // 4) * 4, MAX_TILE, max(budget, MIN_TILE), room]
    if base + STATIC_LDS + MIN_TILE * per_partner > LDS:
        return per_partner, 0, -1, bounds
    tile, which = bounds[0], 0
    if tile > MAX_TILE:
        tile, which = MAX_TILE, 1
    if tile > budget:
        tile, which = max(budget, MIN_TILE), 2
    if tile > room:
        tile, which = room, 3
    return per_partner, tile, which, bounds


def lds_layout(n_floats, n_max, keys=False, slots=None, lanes=1):
    """ya::ens::lds_layout<Pt, keys, slots is not None>(n_max, slots, lanes): byte offsets of the regions in their
    order -- the step's arrays; the keys, 8-byte aligned, one 64-bit key per row of the power of two from n_max up; the
    incidence list of n_max + 1 offsets and 2 `slots` entries of 4 bytes (all-pairs: 16-byte aligned, its end rounded up
    to 16; grid: right behind the keys, its end not rounded; no room where the end and the static fold scratch exceed
    the workgroup's LDS); the term buffer, 16-byte aligned, of tile_behind's length -- the tile and the launch's
    dynamic LDS, 0 = no room.  keys and list are 0 where the launch has none; tile is 0 with one lane."""
    row = 4 * n_floats
    fold = n_max * (4 * row + 12)
    partials = fold + n_floats * 256 * 4
    end = partials + n_floats * 4 * 4
    assert end == whole_step_bytes(n_floats, n_max)
    at_keys = at_list = 0
    if keys:
        key_rows = 1
        while key_rows < n_max:
            key_rows *= 2
        at_keys = -(-end // 8) * 8
        end = at_keys + 8 * key_rows
    if slots is not None:
        at_list = end if keys else up16(end)
        end = at_list + 4 * (n_max + 1) + 8 * slots
    terms = up16(end)
    if slots is not None and not keys:
        end = terms

    def done(tile, total):
        return Layout(n_max * row, 2 * n_max * row, 3 * n_max * row, 4 * n_max * row, fold, partials, at_keys, at_list,
                      terms, tile, total)

    if slots is not None and end + STATIC_LDS > LDS:
        return done(0, 0)
    if lanes <= 1:
        return done(0, end)
    per_partner, tile, _, _ = tile_behind(terms, n_floats, n_max, lanes)
    return done(tile, terms + tile * per_partner if tile else 0)


def coop_binding(n_floats, n_max, lanes):
    """Which of the rule's terms decides the tile length: 0 = n_max, 1 = the longest tile, 2 = the budget, 3 = the
    room left in the LDS (the first of those that are equal), -1 = no room at all (one lane per cell)."""
    _, tile, _, bounds = tile_behind(lds_layout(n_floats, n_max).terms, n_floats, n_max, lanes)
    return bounds.index(min(bounds)) if tile else -1


def coop_rule_edges(n_floats, n_max_up_to, lanes_of=(4, 16, 64)):
    """Every n_max either side of a point where another term of the rule starts to decide, for any lanes."""
    edges = set()
    for lanes in lanes_of:
        for n_max in range(2, n_max_up_to + 1):
            if coop_binding(n_floats, n_max, lanes) != coop_binding(n_floats, n_max - 1, lanes):
                edges |= {n_max - 1, n_max}
    return sorted(edges)


def links_binding(n_floats, n_max, slots, lanes):
    """What decides a linked all-pairs launch's LDS: -2 = the list does not fit (0), -1 = the shortest tile does
    not fit beside it (0), 4 = one lane per cell (the list's end), 0 .. 3 = the bound that cut the tile length last."""
    base = lds_layout(n_floats, n_max, False, slots).terms
    if base + STATIC_LDS > LDS:
        return -2
    return 4 if lanes == 1 else tile_behind(base, n_floats, n_max, lanes)[2]


def largest_slots(n_floats, n_max, lanes=1, keys=False):
    """The largest S whose launch fits (the rule falls monotonically to 0 in S); None where not even S = 0 does."""
    lo, hi = 0, LDS  # fits, does not

    def fits(slots):
        return lds_layout(n_floats, n_max, keys, slots, lanes).bytes > 0

    if not fits(lo):
        return None
    assert not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


# ---- a harness library's C ABI ---------------------------------------------------------------------------------------
def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ya_[A-Za-z0-9_]+)\s*\(", text)))


def built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", built(path)], capture_output=True, text=True, check=True).stdout
    return [(line.split()[-2], line.split()[-1]) for line in out.splitlines() if line.strip()]


def check_abi(header, prefix, ctypes_table, lib_path, loader, n_functions, extras):
    """Header == ctypes table == nm -D: n_functions names, all with `prefix`, the all-pairs harness's under that
    prefix and `extras` beyond them (None: not held against the all-pairs harness); the loader types every entry
    point and hands out one library.  Returns the names."""
    names = declared_functions(header)
    assert len(names) == n_functions and all(n.startswith(prefix) for n in names)
    assert set(names) == set(ctypes_table), "ctypes table and header disagree"
    if extras is not None:
        from_tile = {n.replace("ya_ens_", prefix) for n in declared_functions("yalla_ensemble.h")}
        assert from_tile <= set(names), "the shared entry points of the all-pairs harness"
        assert set(names) - from_tile == set(extras)
    functions = {sym for kind, sym in exported(lib_path) if kind == "T" and sym.startswith("ya_")}
    assert functions == set(names), "library and header disagree"
    lib = loader()  # types every entry point; AttributeError if one is missing
    assert lib is loader()
    return names


def check_only_the_c_abi_is_exported(lib_path, prefix):
    """-fvisibility=hidden: nothing but `prefix`* and the HIP registration symbols (fatbin wrapper, kernel handles
    and stubs' data) leaves the library -- no engine or harness C++ symbol, no entry point of another harness."""
    for kind, sym in exported(lib_path):
        if sym.startswith(prefix) or sym.startswith("__hip") or kind in ("V", "D", "B", "R"):
            continue
        raise AssertionError(f"{kind} {sym}")
    assert not [sym for _, sym in exported(lib_path) if sym.startswith("ya_") and not sym.startswith(prefix)]


def check_models_name_bounds(name_at, n_models):
    assert name_at(-1) is None and name_at(n_models) is None


# ---- the native programs (tests/native_ensemble/, one Makefile) ------------------------------------------------------
def run_native(program, marker, args=(), cwd=None):
    exe = os.path.join(NATIVE, program)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", NATIVE, program], check=True, capture_output=True)
    proc = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert proc.returncode == 0 and marker in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
