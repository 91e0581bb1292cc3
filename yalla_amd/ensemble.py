"""Host-side mirror of `Ensemble<Pt, Tile_solver>` (include/ensemble.cuh) over the ensemble C ABI
(include/yalla_ensemble.h): M independent all-pairs systems of one model in one allocation, advanced
together by the same six launches per step whatever M is, with nothing read by the host.

It mirrors `Solution`: `h_X` is the host mirror, here an `(n_replicas, n_max, n_floats)` view;
`h_n[r]` the host-side count of replica r; `copy_to_device()` / `copy_to_host()` move every row and
every count; `take_step(dt, steps)` advances every replica; `set_fixed*` take an id LOCAL to a
replica and apply to every replica.  Each replica holds, bit for bit, what a
`Solution("<model>_tile", n_max)` given the same rows holds.

    with Ensemble("relu", n_replicas=64, n_max=800) as cells:
        cells.h_X[r, :n, :3] = ...; cells.h_n[r] = n
        cells.copy_to_device()
        cells.take_step(0.05, 100)
        X = cells.positions(r)

`set_param("whole_steps", 1)` lets `take_step(dt, steps)` run as whole-step launches (ya::ens::whole_steps: one
workgroup per replica runs up to `set_param("steps_per_launch", k)` steps from LDS, no launch boundary in between)
wherever the model has no generic forces and n_max is at most 1024; 0 leaves the choice to the engine, -1 (this
harness's default) never does.  The bits are the same either way; `whole_step_launches` counts the launches made.
`set_param("whole_step_lanes", L)` sets the lanes per cell inside such a launch (Ensemble::whole_step_lanes): 1 (this
harness's default) is one thread per cell, 4, 16 or 64 share a cell's pairs among that many lanes whatever the functor
declares (ya::ens::whole_steps_coop; for replicas of a few dozen cells, which leave most of a workgroup idle
otherwise), 0 leaves it to the engine: one lane unless the model's functors are declared YA_STATELESS, else the
largest L with n_max * L <= 256.  Any other value is refused (-3).  Every choice gives the same bits.

`GridEnsemble` (below) is the same for M Grid_solver systems (include/ensemble_grid.cuh), six launches and a grid
build per stage (or whole steps from LDS, `lds_steps`); `GabrielEnsemble` for M Gabriel_solver systems (include/ensemble_gabriel.cuh),
`GabrielLdsEnsemble` the same with whole steps from LDS (`lds_steps`, libyalla_ensemble_gabriel_lds.so);
`LinkedEnsemble` for M all-pairs systems with link forces summed in slot order (include/ensemble_links.cuh);
`LinkedGridEnsemble` the same for M Grid_solver systems, inside launches that step from LDS too;
`SweepEnsemble` any of the three forms with a time step (and a Gabriel coefficient) per replica.
"""
import ctypes as C

import numpy as np

from . import _ffi
from .solution import YallaError, _check


class _Counts:
    """h_n of an Ensemble: an array-like over the library's own host counts."""

    def __init__(self, ens):
        self._ens = ens

    def __len__(self):
        return self._ens.n_replicas

    def _index(self, r):
        r = int(r)
        if r < 0:
            r += len(self)
        if not 0 <= r < len(self):
            raise IndexError(r)
        return r

    def __getitem__(self, r):
        if isinstance(r, slice):
            return [self[k] for k in range(*r.indices(len(self)))]
        return self._ens._f("get_h_n")(self._ens._h, self._index(r))

    def __setitem__(self, r, n):
        if isinstance(r, slice):
            ks = range(*r.indices(len(self)))
            ns = np.broadcast_to(np.asarray(n), (len(ks),))
            for k, v in zip(ks, ns):
                self[k] = v
            return
        _check(self._ens._f("set_h_n")(self._ens._h, self._index(r), int(n)), "set h_n")

    def __iter__(self):
        return (self[r] for r in range(len(self)))

    def __array__(self, dtype=None, copy=None):
        return np.array(list(self), dtype=dtype or np.int32)


class Ensemble:
    # What tells the three classes apart: the prefix of the C ABI the class drives (the grid ones: the same functions
    # and more), the _ffi function that loads its library, and what an unknown model's message calls it.
    _PREFIX, _LOADER, _NOUN = "ya_ens_", "ensemble_lib", "ensemble"

    def _f(self, name):
        return getattr(self.lib, self._PREFIX + name)

    def __init__(self, model, n_replicas, n_max, lib=None):
        self._create(lib, model, n_replicas, n_max)

    def _create(self, lib, model, n_replicas, n_max, *values):
        """<prefix>create(model, n_replicas, n_max, *values, &handle) on `lib` (None: the class's own library), its
        codes turned into exceptions, and the handle attached."""
        self.lib = lib if lib is not None else getattr(_ffi, self._LOADER)()
        handle = C.c_void_p()
        code = self._f("create")(model.encode(), int(n_replicas), int(n_max), *values, C.byref(handle))
        if code == -1:
            raise YallaError(f"unknown {self._NOUN} model {model!r}; known: {_models(self.lib, self._PREFIX)}")
        _check(code, self._PREFIX + "create")
        self._attach(model, handle, n_replicas, n_max)

    def _attach(self, model, handle, n_replicas, n_max):
        self.model = model
        self._h = handle
        self.n_replicas = int(n_replicas)
        self.n_max = int(n_max)
        self.n_floats = self._f("n_floats")(self._h)
        ptr = self._f("h_X")(self._h)
        self.h_X = np.ctypeslib.as_array(ptr, shape=(self.n_replicas, self.n_max, self.n_floats))
        self.h_n = _Counts(self)
        self._whole_step_launches = 0

    def close(self):
        if getattr(self, "_h", None):
            self.h_X = None
            self._f("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def copy_to_device(self):
        _check(self._f("copy_to_device")(self._h), "copy_to_device")

    def copy_to_host(self):
        _check(self._f("copy_to_host")(self._h), "copy_to_host")

    def get_d_n(self, r):
        """Blocking read of replica r's device-side count (the step itself never reads it)."""
        n = self._f("get_d_n")(self._h, int(r))
        if n < 0:
            raise YallaError(f"get_d_n({r}) failed with harness code {n}")
        return n

    def take_step(self, dt, steps=1):
        launches = self._f("take_steps")(self._h, float(dt), int(steps))  # (>= 0: the whole-step launches it made)
        _check(min(launches, 0), "take_step")
        self._whole_step_launches += launches

    @property
    def whole_step_launches(self):
        """Whole-step launches made so far (Ensemble::whole_step_launches): 0 unless set_param("whole_steps", 0 | 1)
        allowed them and the call was eligible."""
        return self._whole_step_launches

    def synchronize(self):
        _check(self._f("synchronize")(self._h), "synchronize")

    def set_fixed(self, local_id=None):
        """set_fixed() holds every replica's centre of mass, set_fixed(i) cell i of every replica
        (i must exist in every replica that is not empty)."""
        if local_id is None:
            _check(self._f("set_fixed")(self._h, 0, 0), "set_fixed")
        else:
            _check(self._f("set_fixed")(self._h, 1, int(local_id)), "set_fixed")

    def set_fixed_xy(self, local_id):
        _check(self._f("set_fixed")(self._h, 2, int(local_id)), "set_fixed_xy")

    def set_param(self, name, value):
        _check(self._f("set_param")(self._h, name.encode(), float(value)), "set_param")
        return 0

    def positions(self, r=None):
        """copy_to_host() and a copy of replica r's rows h_X[r, :h_n[r]] (every replica's, as a list,
        without r)."""
        self.copy_to_host()
        if r is None:
            return [self.h_X[k, : self.h_n[k]].copy() for k in range(self.n_replicas)]
        return self.h_X[r, : self.h_n[r]].copy()

    def old_v(self):
        out = np.empty((self.n_replicas, self.n_max, 3), dtype=np.float32)
        _check(self._f("get_old_v")(self._h, out.ctypes.data_as(C.POINTER(C.c_float))), "get_old_v")
        return out

    def set_old_v(self, v):
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(self.n_replicas, self.n_max, 3)
        _check(self._f("set_old_v")(self._h, v.ctypes.data_as(C.POINTER(C.c_float))), "set_old_v")


class GridEnsemble(Ensemble):
    """Host-side mirror of `Ensemble<Pt, Grid_solver>` (include/ensemble_grid.cuh) over include/yalla_ensemble_grid.h:
    M independent Grid_solver systems of one model, every replica bit for bit what a
    `Solution("<model>_grid", n_max, grid_size, cube_size)` given the same rows holds.  Everything `Ensemble`
    offers, and: `grid(r)` (the replica's cube_id, point_id, cube_start, cube_end as `Solution.grid()` returns
    them, ids local to the replica), `status(r)` (1 = a cell of replica r left its grid; copy_to_host() aborts on
    a replica in that state unless status(r, clear=True) forgave it), a `cube_size` setter, and
    set_param("lanes", 0 | 1 | 4 | 8 | 16) / set_param("sum_order", 0 | 1).

    Every stage scans n_replicas * grid_size**3 counters: pick grid_size to fit the replicas, not 50.

    `set_param("lds_steps", 1)` lets `take_step(dt, steps)` run as launches of one workgroup per replica that step
    from LDS (ya::ens::grid_lds_steps: up to `set_param("lds_steps_max", k)` steps per launch, no counters, nothing of
    size grid_size**3 touched in between) wherever the model has no generic forces and n_max is at most 1024; 0 leaves
    the choice to the engine, -1 (this harness's default) never does.  The bits are the same either way, grid arrays
    and status included; `lds_step_launches` counts the launches made.

    `set_param("lds_step_lanes", L)` sets the lanes per cell inside such a launch (Ensemble<Pt, Grid_solver>::
    lds_step_lanes): 1 (this harness's default) is one thread per cell; 4, 16 or 64 share a cell's candidates among that
    many lanes whatever the functor declares (ya::ens::grid_lds_walk_coop; for replicas of a few dozen cells, which leave
    most of a workgroup idle otherwise); 0 leaves it to the engine: one lane unless the model's functors are declared
    YA_STATELESS, else 16 lanes up to n_max = 32, 4 up to 64, 1 beyond (ya::ens::grid_lds_lanes_for).  Any other value is refused (-3).  Every choice gives the
    same bits.  `lds_step_lanes_used` is what the last such launch ran with: 1 where the term buffer did not fit.
    """
    _PREFIX, _LOADER, _NOUN = "ya_gens_", "grid_ensemble_lib", "grid ensemble"

    def __init__(self, model, n_replicas, n_max, grid_size=50, cube_size=1.0, lib=None):
        self._create(lib, model, n_replicas, n_max, int(grid_size), float(cube_size))
        self.grid_size = int(grid_size)

    @property
    def cube_size(self):
        raise AttributeError("cube_size is write-only here")

    @cube_size.setter
    def cube_size(self, value):
        _check(self._f("set_cube_size")(self._h, float(value)), "set cube_size")

    @property
    def whole_step_launches(self):
        raise AttributeError("a grid ensemble has no whole-step launches")

    @property
    def lds_step_launches(self):
        """Launches that stepped from LDS so far (Ensemble<Pt, Grid_solver>::lds_step_launches): 0 unless
        set_param("lds_steps", 0 | 1) allowed them and the call was eligible."""
        return self._whole_step_launches

    @property
    def lds_step_lanes_used(self):
        """The lanes per cell of the last launch that stepped from LDS (Ensemble<Pt, Grid_solver>::lds_step_lanes_used):
        0 before any, 1 where the term buffer of several lanes did not fit the workgroup's LDS."""
        lanes = self._f("set_param")(self._h, b"lds_step_lanes_used", 0.0)  # (the getter: it sets nothing)
        if lanes < 0:
            raise YallaError(f"lds_step_lanes_used failed with harness code {lanes}")
        return lanes

    def status(self, r, clear=True):
        bits = self._f("status")(self._h, int(r), int(bool(clear)))
        if bits < 0:
            raise YallaError(f"status({r}) failed with harness code {bits}")
        return bits

    def grid(self, r):
        """cube_id, point_id (n_max each; ids local to the replica), cube_start, cube_end (grid_size**3 each) of
        replica r's last build."""
        a, b = np.empty(self.n_max, np.int32), np.empty(self.n_max, np.int32)
        c, d = np.empty(self.grid_size ** 3, np.int32), np.empty(self.grid_size ** 3, np.int32)
        ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
        _check(self._f("get_grid")(self._h, int(r), ip(a), ip(b), ip(c), ip(d)), "get_grid")
        return a, b, c, d


class GabrielEnsemble(GridEnsemble):
    """Host-side mirror of `Ensemble<Pt, Gabriel_solver>` (include/ensemble_gabriel.cuh) over
    include/yalla_ensemble_gabriel.h: M independent Gabriel_solver systems of one model, every replica bit for bit
    what a `Solution("<model>_gabriel", n_max, grid_size, cube_size)` with the same gabriel_coefficient, given the
    same rows, holds.  Everything `GridEnsemble` offers but its set_param knobs (the only parameter is
    "gabriel_coefficient"), and: a `gabriel_coefficient` setter (of every replica, from the next step on) and
    `dense_cells()`, the cells the last force stage left to the dense kernel (more than 64 candidates).
    """
    _PREFIX, _LOADER, _NOUN = "ya_gabens_", "gabriel_ensemble_lib", "Gabriel ensemble"

    def __init__(self, model, n_replicas, n_max, grid_size=50, cube_size=1.0, gabriel_coefficient=0.8, lib=None):
        self._create(lib, model, n_replicas, n_max, int(grid_size), float(cube_size), float(gabriel_coefficient))
        self.grid_size = int(grid_size)

    @property
    def gabriel_coefficient(self):
        raise AttributeError("gabriel_coefficient is write-only here")

    @gabriel_coefficient.setter
    def gabriel_coefficient(self, value):
        _check(self._f("set_param")(self._h, b"gabriel_coefficient", float(value)), "set gabriel_coefficient")

    @property
    def lds_step_launches(self):
        raise AttributeError("a Gabriel ensemble has no launches that step from LDS")

    @property
    def lds_step_lanes_used(self):
        raise AttributeError("a Gabriel ensemble has no launches that step from LDS")

    def dense_cells(self):
        """Blocking read: how many cells, over all replicas, the last force stage left to the dense kernel."""
        n = self._f("dense_cells")(self._h)
        if n < 0:
            raise YallaError(f"dense_cells() failed with harness code {n}")
        return n


class GabrielLdsEnsemble(GabrielEnsemble):
    """`GabrielEnsemble` over include/yalla_ensemble_gabriel_lds.h (libyalla_ensemble_gabriel_lds.so): the same models
    through `Ensemble<Pt, Gabriel_solver>::take_steps`.  `set_param("lds_steps", 1)` lets `take_step(dt, steps)` run
    as launches of one workgroup per replica that step from LDS (ya::ens::gabriel_lds_steps: up to
    `set_param("lds_steps_max", k)` steps per launch, cells with more than 64 candidates done inside the launch)
    wherever the model has no generic force and n_max is at most the point type's capacity
    (`GabrielLdsEnsemble.lds_bytes(model, n_max) > 0`); 0 leaves the choice to the engine, -1 (this harness's default)
    never does.  The bits are the same either way, grid arrays and status included.  `lds_step_launches` counts the
    launches made, `lds_dense_cells()` the (cell, stage) pairs that took the dense path inside them since the ensemble
    was created; `dense_cells()` keeps its meaning for the 16-launch path.

        with GabrielLdsEnsemble("relu", n_replicas=256, n_max=100, grid_size=12) as cells:
            ...; cells.copy_to_device(); cells.set_param("lds_steps", 1); cells.take_step(0.05, 100)
    """
    _PREFIX, _LOADER, _NOUN = "ya_gablds_", "gabriel_lds_ensemble_lib", "Gabriel ensemble"

    @property
    def lds_step_launches(self):
        """Launches that stepped from LDS so far (Ensemble<Pt, Gabriel_solver>::lds_step_launches): 0 unless
        set_param("lds_steps", 0 | 1) allowed them and the call was eligible."""
        return self._whole_step_launches

    def lds_dense_cells(self):
        """Blocking read: the (cell, stage) pairs done on the dense path inside launches that stepped from LDS, over
        all replicas, since the ensemble was created."""
        n = self._f("lds_dense_cells")(self._h)
        if n < 0:
            raise YallaError(f"lds_dense_cells() failed with harness code {n}")
        return n

    @staticmethod
    def lds_bytes(model, n_max, lib=None):
        """ya::ens::gabriel_lds_layout<Pt>(n_max).bytes for the model's point type: the dynamic LDS of a launch that
        steps from LDS, 0 where n_max is beyond the capacity.  Needs no GPU."""
        lib = lib if lib is not None else _ffi.gabriel_lds_ensemble_lib()
        code = lib.ya_gablds_lds_bytes(model.encode(), int(n_max))
        if code < 0:
            raise YallaError(f"ya_gablds_lds_bytes({model!r}, {n_max}) failed with {code}")
        return code


class LinkedEnsemble(Ensemble):
    """Host-side mirror of `Ensemble<Pt, Tile_solver>` stepped with `ya::ens::Replica_links` (include/ensemble_links.cuh)
    over include/yalla_ensemble_links.h: M all-pairs systems of one model, each with `slots_per_replica` link slots of
    one `Links` object over the flat id space.  Everything `Ensemble` offers, and: `h_link`, the host mirror of the
    links as an `(n_replicas, slots_per_replica, 2)` int32 view of ENSEMBLE-GLOBAL ids (replica r's cell i is
    r * n_max + i); `n_links`, the used-slot count (slots from it on are ignored; a slot with a == b is inert; a slot
    with an end outside its own replica's rows [r * n_max, r * n_max + n_r) is skipped); `copy_to_device()` hands both
    over.  A cell's link terms are added in ascending slot order, so results repeat bit for bit and equal the CPU
    restatement's serial loop; `set_param("whole_steps", 1)` runs them inside whole-step launches where the
    incidence list fits (`LinkedEnsemble.lds_bytes(...) > 0` with one lane), the same bits.
    `set_param("links_path", 1)` is `link_forces` with global atomics instead (no fixed order, never whole steps).

        with LinkedEnsemble("relu_links", n_replicas=64, n_max=200, slots_per_replica=200) as cells:
            cells.h_link[r, s] = (r * 200 + a, r * 200 + b); cells.n_links = 64 * 200
            cells.copy_to_device()
            cells.take_step(0.05, 100)
    """
    _PREFIX, _LOADER, _NOUN = "ya_lens_", "linked_ensemble_lib", "linked ensemble"

    def __init__(self, model, n_replicas, n_max, slots_per_replica, strength=0.2, lib=None):
        self._create(lib, model, n_replicas, n_max, int(slots_per_replica), C.c_float(strength))
        self.slots_per_replica = int(slots_per_replica)
        self.strength = float(strength)
        shape = (self.n_replicas, self.slots_per_replica, 2)
        if self.n_replicas * self.slots_per_replica > 0:
            self.h_link = np.ctypeslib.as_array(self._f("h_link")(self._h), shape=shape)
        else:
            self.h_link = np.zeros(shape, np.int32)

    def close(self):
        self.h_link = None
        super().close()

    @property
    def n_links(self):
        return self._f("get_n_links")(self._h)

    @n_links.setter
    def n_links(self, value):
        _check(self._f("set_n_links")(self._h, int(value)), "set n_links")

    @property
    def whole_step_lanes_used(self):
        """The lanes per cell of the last whole-step launch: 0 before any, 1 where the term buffer of several lanes
        did not fit beside the incidence list."""
        return self._f("whole_step_lanes_used")(self._h)

    @staticmethod
    def lds_bytes(model, n_max, slots_per_replica, lanes=1, lib=None):
        """ya::ens::lds_layout<Pt, false, true>(...).bytes for the model's point type: the dynamic LDS of a linked whole-step
        launch, 0 where there is no room.  Needs no GPU."""
        lib = lib if lib is not None else _ffi.linked_ensemble_lib()
        code = lib.ya_lens_lds_bytes(model.encode(), int(n_max), int(slots_per_replica), int(lanes))
        if code < 0:
            raise YallaError(f"ya_lens_lds_bytes({model!r}, {n_max}, {slots_per_replica}, {lanes}) failed with {code}")
        return code


class LinkedGridEnsemble(GridEnsemble):
    """Host-side mirror of `Ensemble<Pt, Grid_solver>` stepped with `ya::ens::Replica_links` (include/ensemble_grid.cuh,
    include/ensemble_links.cuh) over include/yalla_ensemble_grid_links.h: M Grid_solver systems of one model, each with
    `slots_per_replica` link slots of one `Links` object over the flat id space.  Everything `GridEnsemble` offers but
    set_param("lanes", ...), and what `LinkedEnsemble` adds: `h_link` (an `(n_replicas, slots_per_replica, 2)` int32
    view of ENSEMBLE-GLOBAL ids), `n_links` (the used-slot count), `copy_to_device()` hands both over,
    set_param("links_path", 0 | 1).  A cell's link terms are added in ascending slot order; a slot with a == b is inert,
    one with an end outside its own replica's rows is skipped.  `set_param("lds_steps", 1)` runs the steps as launches
    of one workgroup per replica that step from LDS (ya::ens::grid_lds_steps_linked) where n_max <= 1024 and the
    incidence list fits beside the keys (`LinkedGridEnsemble.lds_bytes(...) > 0`): the same bits, grid arrays and
    status included; `lds_step_launches` counts the launches made.  `set_param("lds_step_lanes", L)` and
    `lds_step_lanes_used` as `GridEnsemble`'s; the term buffer lies behind the incidence list, and a list that leaves
    no room for 16 candidates' terms leaves the launch one lane per cell.

        with LinkedGridEnsemble("relu_links", 64, 200, slots_per_replica=400, grid_size=12) as cells:
            cells.h_link[r, s] = (r * 200 + a, r * 200 + b); cells.copy_to_device()
            cells.set_param("lds_steps", 1); cells.take_step(0.05, 100)
    """
    _PREFIX, _LOADER, _NOUN = "ya_glens_", "linked_grid_ensemble_lib", "linked grid ensemble"

    def __init__(self, model, n_replicas, n_max, slots_per_replica, strength=0.2, grid_size=50, cube_size=1.0, lib=None):
        self._create(lib, model, n_replicas, n_max, int(grid_size), C.c_float(cube_size), int(slots_per_replica),
                     C.c_float(strength))
        self.grid_size = int(grid_size)
        self.slots_per_replica = int(slots_per_replica)
        self.strength = float(strength)
        shape = (self.n_replicas, self.slots_per_replica, 2)
        if self.n_replicas * self.slots_per_replica > 0:
            self.h_link = np.ctypeslib.as_array(self._f("h_link")(self._h), shape=shape)
        else:
            self.h_link = np.zeros(shape, np.int32)

    def close(self):
        self.h_link = None
        super().close()

    n_links = LinkedEnsemble.n_links

    @staticmethod
    def lds_bytes(model, n_max, slots_per_replica, lib=None):
        """ya::ens::lds_layout<Pt, true, true>(...).bytes for the model's point type: the dynamic LDS of a linked launch that steps
        from LDS, 0 where there is no room.  Needs no GPU."""
        lib = lib if lib is not None else _ffi.linked_grid_ensemble_lib()
        code = lib.ya_glens_lds_bytes(model.encode(), int(n_max), int(slots_per_replica))
        if code < 0:
            raise YallaError(f"ya_glens_lds_bytes({model!r}, {n_max}, {slots_per_replica}) failed with {code}")
        return code


class SweepEnsemble(GridEnsemble):
    """The three forms of Ensemble behind one class (include/yalla_ensemble_sweep.h, libyalla_ensemble_sweep.so), stepped
    with A TIME STEP PER REPLICA (ya::ens::Replica_dt) and, form "gabriel", A COEFFICIENT PER REPLICA
    (Ensemble<Pt, Gabriel_solver>::d_gabriel_coefficients).  form: "tile", "grid" or "gabriel"; the models of each:
    `sweep_models(form)`.  Replica r holds, bit for bit, what a lone `Solution("<model>_<form>", n_max, ...)` of its rows
    holds when stepped with dt[r] (and gabriel_coefficients[r]).

        with SweepEnsemble("tile", "relu", n_replicas=64, n_max=200) as cells:
            ...; cells.copy_to_device()
            cells.dt = np.linspace(0.01, 0.1, 64)     # uploaded; None returns to the scalar of take_step(dt)
            cells.take_step(steps=100)                # replica r with dt[r]
            cells.scale_dt(0.5); cells.take_step(steps=100)   # the array changed ON THE DEVICE, no synchronise

    `dt` and `gabriel_coefficients` read back what was set (float32), not what a kernel made of it since.  What the
    form's own class offers is here under the same names: grid(r), status(r) and the cube_size setter ("grid",
    "gabriel"), h_link and n_links (a model with links, slots_per_replica > 0), dense_cells() and lds_dense_cells()
    ("gabriel"), and set_param with "whole_steps", "whole_step_lanes" ("tile"), "lds_steps" ("grid", "gabriel"),
    "lds_step_lanes" ("grid"), "steps_per_launch" (every form), "gabriel_coefficient", "cube_size".  `lds_launches` counts
    the launches that stepped from LDS (whole-step launches of form "tile"), `lanes_used` is the lanes per cell of the
    last one."""
    _PREFIX, _LOADER, _NOUN = "ya_swp_", "sweep_ensemble_lib", "sweep ensemble"
    FORMS = ("tile", "grid", "gabriel")

    def __init__(self, form, model, n_replicas, n_max, slots_per_replica=0, grid_size=50, cube_size=1.0,
                 gabriel_coefficient=0.8, lib=None):
        self.lib = lib if lib is not None else _ffi.sweep_ensemble_lib()
        handle = C.c_void_p()
        code = self._f("create")(form.encode(), model.encode(), int(n_replicas), int(n_max), int(slots_per_replica),
                                 int(grid_size), C.c_float(cube_size), C.c_float(gabriel_coefficient), C.byref(handle))
        if code == -4:
            raise YallaError(f"unknown form {form!r}; known: {list(self.FORMS)}")
        if code == -1:
            raise YallaError(f"unknown {form} sweep model {model!r}; known: {sweep_models(form, self.lib)}")
        _check(code, "ya_swp_create")
        self._attach(model, handle, n_replicas, n_max)
        self.form = form
        self.grid_size = int(grid_size)
        self.slots_per_replica = int(slots_per_replica)
        self._dt = self._coefficients = None
        shape = (self.n_replicas, self.slots_per_replica, 2)
        if self.n_replicas * self.slots_per_replica > 0:
            self.h_link = np.ctypeslib.as_array(self._f("h_link")(self._h), shape=shape)
        else:
            self.h_link = np.zeros(shape, np.int32)

    def close(self):
        self.h_link = None
        super().close()

    n_links = LinkedEnsemble.n_links

    def _per_replica(self, values, what):
        values = np.ascontiguousarray(values, dtype=np.float32)
        if values.shape != (self.n_replicas,):
            raise ValueError(f"{what} takes {self.n_replicas} values, one per replica, not an array of shape {values.shape}")
        return values.copy()

    @property
    def dt(self):
        """The time steps set last, one per replica (float32), or None: take_step steps with its scalar."""
        return None if self._dt is None else self._dt.copy()

    @dt.setter
    def dt(self, values):
        if values is None:
            _check(self._f("set_dt")(self._h, None), "set dt")
            self._dt = None
            return
        values = self._per_replica(values, "dt")
        _check(self._f("set_dt")(self._h, values.ctypes.data_as(C.POINTER(C.c_float))), "set dt")
        self._dt = values

    @property
    def gabriel_coefficients(self):
        """The coefficients set last, one per replica (float32), or None: every replica uses "gabriel_coefficient"."""
        return None if self._coefficients is None else self._coefficients.copy()

    @gabriel_coefficients.setter
    def gabriel_coefficients(self, values):
        if values is None:
            _check(self._f("set_gabriel_coefficients")(self._h, None), "set gabriel_coefficients")
            self._coefficients = None
            return
        values = self._per_replica(values, "gabriel_coefficients")
        _check(self._f("set_gabriel_coefficients")(self._h, values.ctypes.data_as(C.POINTER(C.c_float))),
               "set gabriel_coefficients")
        self._coefficients = values

    def scale_dt(self, factor):
        """Multiplies the device's dt array by `factor` (binary32), by a kernel queued behind the steps so far and not
        waited for: what a model's own adaptive-dt kernel does.  `dt` keeps reading what was set."""
        _check(self._f("scale_dt")(self._h, C.c_float(factor)), "scale_dt")

    def take_step(self, dt=None, steps=1):
        """`steps` Heun steps of every replica: with the array `dt` was set to, or with the scalar given here."""
        if dt is None and self._dt is None:
            raise ValueError("take_step needs a dt: set the dt property or pass a scalar")
        super().take_step(0.0 if dt is None else dt, steps)

    @property
    def whole_step_launches(self):
        return self._whole_step_launches

    lds_launches = lds_step_launches = whole_step_launches

    @property
    def lanes_used(self):
        return self._f("lanes_used")(self._h)

    lds_step_lanes_used = whole_step_lanes_used = lanes_used

    @property
    def gabriel_coefficient(self):
        raise AttributeError("gabriel_coefficient is write-only here")

    @gabriel_coefficient.setter
    def gabriel_coefficient(self, value):
        self.set_param("gabriel_coefficient", value)

    @property
    def cube_size(self):
        raise AttributeError("cube_size is write-only here")

    @cube_size.setter
    def cube_size(self, value):
        self.set_param("cube_size", value)

    def dense_cells(self):
        n = self._f("dense_cells")(self._h)
        if n < 0:
            raise YallaError(f"dense_cells() failed with harness code {n}")
        return n

    def lds_dense_cells(self):
        n = self._f("lds_dense_cells")(self._h)
        if n < 0:
            raise YallaError(f"lds_dense_cells() failed with harness code {n}")
        return n


def sweep_models(form, lib=None):
    lib = lib if lib is not None else _ffi.sweep_ensemble_lib()
    count = lib.ya_swp_models_count(form.encode())
    if count < 0:
        raise YallaError(f"unknown form {form!r}; known: {list(SweepEnsemble.FORMS)}")
    return [lib.ya_swp_models_name(form.encode(), i).decode() for i in range(count)]


def linked_grid_models(lib=None):
    return _models(lib if lib is not None else _ffi.linked_grid_ensemble_lib(), "ya_glens_")


def _models(lib, prefix):
    names, count = getattr(lib, prefix + "models_name"), getattr(lib, prefix + "models_count")
    return [names(i).decode() for i in range(count())]


def models(lib=None):
    return _models(lib if lib is not None else _ffi.ensemble_lib(), "ya_ens_")


def grid_models(lib=None):
    return _models(lib if lib is not None else _ffi.grid_ensemble_lib(), "ya_gens_")


def gabriel_models(lib=None):
    return _models(lib if lib is not None else _ffi.gabriel_ensemble_lib(), "ya_gabens_")


def gabriel_lds_models(lib=None):
    return _models(lib if lib is not None else _ffi.gabriel_lds_ensemble_lib(), "ya_gablds_")


def linked_models(lib=None):
    return _models(lib if lib is not None else _ffi.linked_ensemble_lib(), "ya_lens_")
