"""Shared by tests/test_ensemble_widths.py (host) and tests/test_ensemble_widths_gpu.py: the three harness libraries
built from yalla_amd/csrc/ensemble_widths_models.h -- models::field_coupling, a non-zero force in EVERY field, on points
of 4 to 16 floats, as ensembles of the all-pairs, the grid and the Gabriel form --, the capacities of the launches that
step from LDS by point type, the start states, and `Widths`: ensembles of one model under several settings in
lock-step with BOTH references of every replica, a lone Solution of libyalla_models_widths.so
(ensemble_support.Lockstep's) and the widths oracle's Solution in the engine's reduce order.

The libraries are libyalla_ensemble.so's, libyalla_ensemble_grid.so's and libyalla_ensemble_gabriel_lds.so's translation
units with another model table (-DYA_MODELS_WIDTHS); the shipped libraries keep theirs."""
import functools
import os

import numpy as np

import widths_support as ws
from ensemble_support import Lockstep, bits, lds_layout, seeded_rows
from yalla_amd import _ffi
from yalla_amd.ensemble import Ensemble, GabrielLdsEnsemble, GridEnsemble
from yalla_amd.solution import Solution

f32 = np.float32
HERE = os.path.dirname(_ffi.ENSEMBLE_LIB)
# form -> (library, its C header, prefix, ctypes table, Python class, the lone model's suffix)
FORMS = {
    "tile": (os.path.join(HERE, "libyalla_ensemble_widths.so"), "yalla_ensemble.h", "ya_ens_", "ENSEMBLE_ABI",
             Ensemble, "_tile"),
    "grid": (os.path.join(HERE, "libyalla_ensemble_grid_widths.so"), "yalla_ensemble_grid.h", "ya_gens_",
             "GRID_ENSEMBLE_ABI", GridEnsemble, "_grid"),
    "gabriel": (os.path.join(HERE, "libyalla_ensemble_gabriel_lds_widths.so"), "yalla_ensemble_gabriel_lds.h",
                "ya_gablds_", "GABRIEL_LDS_ENSEMBLE_ABI", GabrielLdsEnsemble, "_gabriel"),
}
TYPES = {"tile": ["float4", "w6", "w11", "w16"], "grid": ["float4", "w6", "w8", "w9", "w11", "w16"],
         "gabriel": ["float4", "w6", "w11", "w16"]}
SIZEOF = {"float4": 16, "w6": 24, "w8": 32, "w9": 36, "w11": 44, "w16": 64}
# type -> rows of a replica that a launch stepping from LDS holds (all-pairs, grid, Gabriel), and the first n_max at
# which the Gabriel launch lays out 2 sets of dense lists / 1 set.  yalla_amd/csrc/ensemble_widths_models.h holds the
# headers to the same figures with static_asserts; tests/test_ensemble_widths.py holds the restatements to them.
CAPACITY = {
    "float4": (1024, 1024, 995, 530, 770),
    "w6": (1024, 1024, 696, 432, 568),
    "w8": (1024, 1024, 512, 343, 449),
    "w9": (970, 918, 459, 305, 394),
    "w11": (794, 750, 346, 249, 303),
    "w16": (537, 512, 176, 134, 160),
}
FORM_INDEX = {"tile": 0, "grid": 1, "gabriel": 2}
KEYS = {"tile": False, "grid": True}


def capacity_of(form, kind):
    return CAPACITY[kind][FORM_INDEX[form]]


@functools.lru_cache(maxsize=None)
def lib_of(form):
    path, _, _, table, _, _ = FORMS[form]
    return _ffi._load(path, getattr(_ffi, table))  # raises if it has not been built: there is no fallback


def model(kind):
    return "fields_" + kind


def models_of(form):
    lib, prefix = lib_of(form), FORMS[form][2]
    return [getattr(lib, prefix + "models_name")(i).decode() for i in range(getattr(lib, prefix + "models_count")())]


# ---- which launches have room (ensemble_support.lds_layout, the restated rule) -------------------------------------
def has_room(form, kind, n_max, lanes):
    """Whether a launch from LDS of `lanes` lanes per cell has room for its term buffer (tile > 0 and bytes > 0)."""
    layout = lds_layout(ws.WIDTH[kind], n_max, KEYS[form], None, lanes)
    assert (layout.tile == 0) == (layout.bytes == 0) or lanes == 1
    return layout.bytes > 0


def lanes_for(form, n_max):
    """ya::ens::whole_step_lanes_for / grid_lds_lanes_for: the engine's choice for a stateless pair."""
    if form == "tile":
        return 64 if n_max <= 4 else 16 if n_max <= 16 else 4 if n_max <= 64 else 1
    return 16 if n_max <= 32 else 4 if n_max <= 64 else 1


def lanes_expected(form, kind, n_max, setting):
    """The lanes per cell a launch from LDS says it ran with under the setting (0: the engine's choice, one lane for
    the types whose functor is not declared stateless)."""
    lanes = setting
    if lanes == 0:
        lanes = 1 if kind in ws.UNDECLARED else lanes_for(form, n_max)
    return lanes if lanes == 1 or has_room(form, kind, n_max, lanes) else 1


# ---- start states ----------------------------------------------------------------------------------------------------
def rows_of(kind, n, seed, positions=None):
    """n rows of the type: ensemble_support.seeded_rows' positions (or the ones given) and widths_support.extra_fields
    behind them."""
    width = ws.WIDTH[kind]
    X = seeded_rows(width, n, seed)
    if positions is not None:
        X[:, :3] = positions
    X[:, 3:] = ws.extra_fields(n, width)
    return X


def seeded_old_v(m, n_max, seed=5):
    return (np.random.default_rng(seed).random((m, n_max, 3)) * 0.2 - 0.1).astype(f32)


def ball(n, centre, seed, radius=0.45):
    """n positions inside a ball around `centre`: every pair is closer than 1."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v *= (radius * rng.random(n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return (np.asarray(centre, dtype=np.float64) + v).astype(f32)


def with_neighbour(X, within=1 - 1e-5):
    """Which cells have another cell closer than `within` (float64 on the binary32 positions; the default is a
    neighbour within 1 in binary32 too, whatever the rounding)."""
    P = X[:, :3].astype(np.float64)
    d = np.linalg.norm(P[:, None] - P[None], axis=2)
    np.fill_diagonal(d, np.inf)
    return (d < within).any(axis=1)


def must_move(X, dt):
    """(n, width - 3) booleans: the extra fields whose first right-hand side moves them for certain.  field_coupling's
    force on field k of cell i is -c_k sum_j (X[i, k] - X[j, k]) over the cells j within 1, c_k = (k - 2) / 16; the
    start values are multiples of 2^-13, so every term and the sum are exact in binary32 and the force is zero exactly
    where the integer sum is (a cell in the middle of its neighbours' values, which extra_fields' progressions do
    produce).  A step of dt moves the field for certain where |dt force| exceeds an ulp of 1.  Cells with a pair so
    close to 1 that binary32 may see it on either side are left out."""
    P = X[:, :3].astype(np.float64)
    d = np.linalg.norm(P[:, None] - P[None], axis=2)
    np.fill_diagonal(d, np.inf)
    unsure = (np.abs(d - 1) < 1e-5).any(axis=1)
    near = (d < 1).astype(np.int64)
    q = np.round(X[:, 3:].astype(np.float64) * 2 ** 13).astype(np.int64)
    sums = near.sum(axis=1)[:, None] * q - near @ q
    c = (np.arange(3, X.shape[1]) - 2) / 16.0
    return (np.abs(sums) * 2.0 ** -13 * c[None, :] * dt > 2.0 ** -23) & ~unsure[:, None]


# ---- ensembles under several settings and both references, in lock-step ---------------------------------------------
def oracle_lib():
    lib = _ffi.bind(ws.build_widths_oracle())
    assert lib.ya_models_is_device() == 0
    return lib


def device_lib():
    lib = _ffi.bind(ws.WIDTHS_DEVICE_LIB)
    assert lib.ya_models_is_device() == 1 and lib.ya_models_arith() == 0
    return lib


def lanes_used(ens, form):
    """The lanes per cell of the ensemble's last launch from LDS, by the harness's getter."""
    name = b"whole_step_lanes_used" if form == "tile" else b"lds_step_lanes_used"
    used = ens._f("set_param")(ens._h, name, 0.0)
    assert used >= 0, used
    return used


class Widths(Lockstep):
    """`variants`: name -> settings (set_param pairs) of one ensemble each, all of model fields_<kind> in the form's
    widths library and fed the same rows; Lockstep's lone Solutions of libyalla_models_widths.so; and one Solution of
    the widths oracle per replica that has cells, summing in the engine's reduce order.  Everything is stepped and set
    alike.  check() compares every variant's every replica with both references on bit patterns, field by field."""

    def __init__(self, form, kind, rows, n_max, variants, grid_size=30, cube_size=1.0, coefficient=0.8, old_v=None,
                 sum_order=None):
        self.form, self.kind = form, kind
        path, _, _, _, cls, suffix = FORMS[form]
        args = () if form == "tile" else (grid_size, cube_size)
        ens_args = (coefficient,) if form == "gabriel" else ()
        names = list(variants)
        make = lambda *a, **k: cls(*a, **k)
        super().__init__(make, suffix, model(kind), [len(X) for X in rows], n_max, args, ens_args,
                         grids=form != "tile", rows=rows, lib=lib_of(form), single_lib=device_lib())
        self.variant = {names[0]: self.ens}
        for name in names[1:]:
            ens = cls(model(kind), len(rows), n_max, *args, *ens_args, lib=lib_of(form))
            ens.h_X[:] = self.ens.h_X
            ens.h_n[:] = self.counts
            ens.copy_to_device()
            self.variant[name] = ens
        for name, settings in variants.items():
            for key, value in settings.items():
                self.variant[name].set_param(key, value)
        self.first = [np.array(X, dtype=f32) for X in rows]
        self.oracle = {}
        lib = oracle_lib()
        for r, X in enumerate(rows):
            if len(X) == 0:
                continue
            s = Solution(model(kind) + suffix, n_max, *args, lib=lib)
            assert s.set_reduce_order(1) == 0
            s.h_X[:len(X)] = X
            s.h_n = len(X)
            s.copy_to_device()
            self.oracle[r] = s
        if form == "gabriel":
            for s in list(self.single.values()) + list(self.oracle.values()):
                s.set_param("gabriel_coefficient", coefficient)
        if sum_order is not None:
            self.each(lambda s: s.set_param("sum_order", sum_order))
        if old_v is not None:
            self.set_old_v(old_v)
        self.seen = {name: 0 for name in names}

    def each(self, call):
        for ens in self.variant.values():
            call(ens)
        for s in list(self.single.values()) + list(self.oracle.values()):
            call(s)

    def set_old_v(self, v):
        for ens in self.variant.values():
            ens.set_old_v(v)
        for r in self.single:
            self.single[r].set_old_v(v[r])
        for r in self.oracle:
            self.oracle[r].set_old_v(v[r])

    def launches(self, name):
        ens = self.variant[name]
        return ens.whole_step_launches if self.form == "tile" else ens.lds_step_launches

    def expect(self, name, launches, lanes=None):
        """The variant's launches from LDS rose by `launches` since the last look; lanes: what the last one ran with."""
        now = self.launches(name)
        assert now - self.seen[name] == launches, (self.kind, name, "launches", now, self.seen[name], launches)
        self.seen[name] = now
        if lanes is not None:
            assert lanes_used(self.variant[name], self.form) == lanes, (self.kind, name, "lanes used")

    def check(self, what=""):
        lone = self.results()
        oracle = {r: want_of(s, self.counts[r], self.grids) for r, s in self.oracle.items()}
        for r, want in oracle.items():
            same_replica(lone[r], want, self.counts[r], (what, self.kind, "the lone Solution against the oracle, replica", r))
        for name, ens in self.variant.items():
            status = [ens.status(r, clear=False) for r in range(len(self.counts))] if self.grids else []
            assert not any(status), (what, self.kind, name, "status", status)
            ens.copy_to_host()
            v = ens.old_v()
            for r, n in enumerate(self.counts):
                assert ens.h_n[r] == n and ens.get_d_n(r) == n, (what, name, r)
                got = (bits(ens.h_X[r, :n]), bits(v[r, :n]), ens.grid(r) if self.grids else None)
                same_replica(got, lone[r], n, (what, self.kind, name, "against the lone Solution, replica", r))
                if r in oracle:
                    same_replica(got, oracle[r], n, (what, self.kind, name, "against the oracle, replica", r))

    def extras_moved(self, dt):
        """The extra fields moved, in every variant.  All-pairs and grid form: EVERY extra field of every cell whose
        first right-hand side there is certainly not lost in rounding (must_move).  Gabriel form, whose neighbours are
        a subset that this module does not restate: every extra column in some cell of every replica that has a pair
        within 1."""
        assert ws.WIDTH[self.kind] > 3
        some = False
        for ens in self.variant.values():
            ens.copy_to_host()
            for r, n in enumerate(self.counts):
                if n < 2:
                    continue
                changed = bits(ens.h_X[r, :n, 3:]) != bits(self.first[r][:, 3:])
                if self.form == "gabriel":
                    if with_neighbour(self.first[r]).any():
                        assert changed.any(axis=0).all(), (self.kind, "an extra column that did not move, replica", r)
                        some = True
                else:
                    must = must_move(self.first[r], dt)
                    assert changed[must].all(), (self.kind, "extra fields that did not move, replica", r)
                    some = some or bool(must.any(axis=0).all())
        assert some

    def close(self):
        for ens in self.variant.values():
            ens.close()
        for s in list(self.single.values()) + list(self.oracle.values()):
            s.close()


def want_of(s, n, grids):
    return bits(s.positions()), bits(s.old_v()[:n]), s.grid() if grids else None


def same_replica(got, want, n, what):
    """Positions field by field (a failure names the field), old_v[:n] and, where held, the four grid arrays."""
    (X, v, grid), (wX, wv, wgrid) = got, want
    assert X.shape == wX.shape, (what, "shape")
    for k in range(X.shape[1]):
        assert np.array_equal(X[:, k], wX[:, k]), (what, f"field {k}")
    assert np.array_equal(v, wv), (what, "old_v")
    if grid is not None:
        for a, b, name in zip(grid, wgrid, ("cube_id", "point_id", "cube_start", "cube_end")):
            cut = n if name in ("cube_id", "point_id") else None
            assert np.array_equal(a[:cut], b[:cut]), (what, name)
