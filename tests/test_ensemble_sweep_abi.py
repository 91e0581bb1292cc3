"""The sweep harness (include/yalla_ensemble_sweep.h, libyalla_ensemble_sweep.so, yalla_amd.SweepEnsemble) through the
layers that need no GPU: header, ctypes table and the library's exports agree; nothing but ya_swp_* leaves the library;
create refuses an unknown form, an unknown model and bad sizes before it touches the device; set_param knows the
names of the other harnesses; the Python class checks an array's length and clears it with None (against a stand-in
library, as tests/test_ensemble_grid_lds_steps_abi.py's); the engine headers no longer call a per-replica dt or
coefficient "not built"."""
import ctypes
import os

import numpy as np
import pytest
from ensemble_support import check_abi, check_models_name_bounds, check_only_the_c_abi_is_exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = {"ya_swp_status", "ya_swp_get_grid", "ya_swp_h_link", "ya_swp_set_n_links", "ya_swp_get_n_links",
          "ya_swp_set_dt", "ya_swp_set_gabriel_coefficients", "ya_swp_scale_dt", "ya_swp_lanes_used",
          "ya_swp_dense_cells", "ya_swp_lds_dense_cells"}
MODELS = {"tile": ["relu", "springs", "relu_po", "links"], "grid": ["relu", "springs", "relu_po", "springs_links"],
          "gabriel": ["relu", "relu_plain", "relu_po"]}


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_header_ctypes_table_and_library_agree():
    from yalla_amd import _ffi
    names = check_abi("yalla_ensemble_sweep.h", "ya_swp_", _ffi.SWEEP_ENSEMBLE_ABI, _ffi.SWEEP_ENSEMBLE_LIB,
                      _ffi.sweep_ensemble_lib, 17 + len(EXTRAS), EXTRAS)
    assert len(names) == 28


def test_only_the_c_abi_is_exported():
    from yalla_amd import _ffi
    check_only_the_c_abi_is_exported(_ffi.SWEEP_ENSEMBLE_LIB, "ya_swp_")


def test_the_model_tables():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import SweepEnsemble, YallaError, sweep_models
    lib = _ffi.sweep_ensemble_lib()
    assert SweepEnsemble.FORMS == tuple(MODELS)
    for form, models in MODELS.items():
        assert sweep_models(form) == models
        check_models_name_bounds(lambda i: lib.ya_swp_models_name(form.encode(), i), len(models))
    assert lib.ya_swp_models_count(b"cube") == -4 and lib.ya_swp_models_name(b"cube", 0) is None
    with pytest.raises(YallaError, match="unknown form"):
        sweep_models("cube")


def test_create_refuses_before_the_device_is_touched():
    """(No GPU here: a create that got as far as an allocation would abort the process.)"""
    from yalla_amd import _ffi
    from yalla_amd.ensemble import SweepEnsemble, YallaError
    lib = _ffi.sweep_ensemble_lib()
    out = ctypes.c_void_p()

    def create(form, model, n_replicas=2, n_max=4, slots=0, grid_size=8, cube_size=1.0, coefficient=0.8):
        return lib.ya_swp_create(form, model, n_replicas, n_max, slots, grid_size, cube_size, coefficient,
                                 ctypes.byref(out))

    assert create(b"cube", b"relu") == -4 and create(b"", b"relu") == -4
    for form in MODELS:
        assert create(form.encode(), b"no_such_model") == -1, form
        assert create(form.encode(), b"relu", n_replicas=0) == -3 and create(form.encode(), b"relu", n_max=0) == -3
        assert create(form.encode(), b"relu", n_replicas=-1) == -3 and create(form.encode(), b"relu", slots=-1) == -3
        assert create(form.encode(), b"relu", n_replicas=1 << 20, n_max=1 << 12) == -3  # (ids are ints)
        assert create(form.encode(), b"relu", slots=4) == -3, "slots for a model without links"
    assert create(b"tile", b"springs_links") == -1 and create(b"gabriel", b"links") == -1  # (another form's model)
    for form in (b"grid", b"gabriel"):
        assert create(form, b"relu", grid_size=0) == -3 and create(form, b"relu", cube_size=0.0) == -3
        assert create(form, b"relu", cube_size=float("nan")) == -3
    assert create(b"gabriel", b"relu", coefficient=float("inf")) == -3
    assert create(None, b"relu") == -3 and create(b"tile", None) == -3
    assert lib.ya_swp_create(b"tile", b"relu", 2, 4, 0, 8, 1.0, 0.8, None) == -3
    assert out.value is None
    with pytest.raises(YallaError, match="unknown form 'cube'"):
        SweepEnsemble("cube", "relu", 2, 4)
    with pytest.raises(YallaError, match="unknown tile sweep model 'nope'.*'relu', 'springs', 'relu_po', 'links'"):
        SweepEnsemble("tile", "nope", 2, 4)
    with pytest.raises(YallaError, match="-3"):
        SweepEnsemble("grid", "relu", 2, 4, grid_size=0)


def test_set_param_knows_the_names_of_the_other_harnesses():
    from yalla_amd import _ffi
    lib = _ffi.sweep_ensemble_lib()
    for name in (b"whole_steps", b"whole_step_lanes", b"lds_steps", b"lds_step_lanes", b"steps_per_launch",
                 b"gabriel_coefficient", b"cube_size"):
        assert lib.ya_swp_set_param(None, name, 1.0) == -3, name
    for name in (b"lds_steps_max", b"tile_lanes", b"dt", b"links_path", b""):
        assert lib.ya_swp_set_param(None, name, 1.0) == -2, name
    assert lib.ya_swp_set_param(None, None, 1.0) == -3
    # the entry points that take a handle say so on none
    assert lib.ya_swp_set_dt(None, None) == -3 and lib.ya_swp_set_gabriel_coefficients(None, None) == -3
    assert lib.ya_swp_scale_dt(None, 0.5) == -3 and lib.ya_swp_lanes_used(None) == -3


class StandInLibrary:
    """The few ya_swp_* entry points SweepEnsemble's constructor, its two array properties, scale_dt and take_step
    call; what the arrays' setters hand over is kept (a copy of the floats, or None)."""

    def __init__(self, n_replicas, n_max):
        self.rows = (ctypes.c_float * (n_replicas * n_max * 3))()
        self.n_replicas = n_replicas
        self.dt = self.coefficients = "never set"
        self.steps = []

    def __getattr__(self, name):
        if not name.startswith("ya_swp_"):
            raise AttributeError(name)
        return getattr(self, "_" + name[len("ya_swp_"):])

    def _create(self, form, model, n_replicas, n_max, slots, grid_size, cube_size, coefficient, out):
        out._obj.value = 1
        return 0

    def _n_floats(self, handle):
        return 3

    def _h_X(self, handle):
        return ctypes.cast(self.rows, ctypes.POINTER(ctypes.c_float))

    def _floats(self, pointer):
        return None if pointer is None else [pointer[r] for r in range(self.n_replicas)]

    def _set_dt(self, handle, pointer):
        self.dt = self._floats(pointer)
        return 0

    def _set_gabriel_coefficients(self, handle, pointer):
        self.coefficients = self._floats(pointer)
        return 0

    def _scale_dt(self, handle, factor):
        return 0 if self.dt not in (None, "never set") else -3

    def _take_steps(self, handle, dt, steps):
        self.steps.append((dt, steps))
        return 2

    def _destroy(self, handle):
        pass


def test_the_python_class_checks_an_arrays_length_and_none_clears_it():
    from yalla_amd import SweepEnsemble
    from yalla_amd.ensemble import YallaError
    lib = StandInLibrary(3, 4)
    ens = SweepEnsemble("gabriel", "relu", 3, 4, grid_size=8, lib=lib)
    assert ens.dt is None and ens.gabriel_coefficients is None and np.shape(ens.h_X) == (3, 4, 3)
    with pytest.raises(ValueError, match="a dt"):
        ens.take_step()  # neither an array nor a scalar
    with pytest.raises(YallaError, match="-3"):
        ens.scale_dt(0.5)  # no array to scale
    for wrong in ([0.1, 0.2], [0.1, 0.2, 0.3, 0.4], 0.1, [[0.1, 0.2, 0.3]], []):
        with pytest.raises(ValueError, match="3 values, one per replica"):
            ens.dt = wrong
        with pytest.raises(ValueError, match="3 values, one per replica"):
            ens.gabriel_coefficients = wrong
    assert lib.dt == "never set" and lib.coefficients == "never set" and ens.dt is None

    ens.dt = [0.05, 0.1, 0.0]  # (float64 in, binary32 handed over and read back)
    want = np.array([0.05, 0.1, 0.0], np.float32)
    assert lib.dt == list(want) and ens.dt.dtype == np.float32 and np.array_equal(ens.dt, want)
    ens.dt[0] = 7.0  # a copy: the property is set as a whole
    assert np.array_equal(ens.dt, want)
    ens.take_step(steps=5)
    ens.take_step(0.25, 2)
    assert lib.steps == [(0.0, 5), (0.25, 2)] and ens.lds_launches == 4
    ens.scale_dt(0.5)
    assert np.array_equal(ens.dt, want), "dt reads back what was set"
    ens.gabriel_coefficients = np.array([0.5, 0.8, 1.0])
    assert lib.coefficients == [0.5, np.float32(0.8), 1.0] and np.array_equal(
        ens.gabriel_coefficients, np.array([0.5, 0.8, 1.0], np.float32))

    ens.dt = None
    assert lib.dt is None and ens.dt is None and lib.coefficients is not None
    with pytest.raises(ValueError, match="a dt"):
        ens.take_step(steps=1)
    ens.take_step(0.1)
    assert lib.steps[-1] == (0.1, 1)
    ens.gabriel_coefficients = None
    assert lib.coefficients is None and ens.gabriel_coefficients is None
    ens.close()


def test_the_headers_say_it_is_built():
    """The three engine headers and DESIGN.md named a per-replica dt and coefficient as not built; the overloads, the
    member and the three places the values pass through are there instead."""
    shared, grid, gabriel = (text("include", name) for name in ("ensemble.cuh", "ensemble_grid.cuh", "ensemble_gabriel.cuh"))
    design = text("DESIGN.md")
    for source in (shared, grid, gabriel):
        assert "a per-replica dt" not in source and "per-replica gabriel_coefficient" not in source
        assert "void take_steps(ya::ens::Replica_dt dt, int n_steps" in source
    assert "a per-replica `dt`" not in design and "a per-replica `gabriel_coefficient`" not in design
    assert "Per-replica `dt` and coefficient" in design
    assert "struct Replica_dt {" in shared and "void take_step(Replica_dt dt" in shared
    assert "const float* d_gabriel_coefficients = nullptr;" in gabriel
    # resolved once per workgroup, by the replica: in the two update kernels and in the callers of whole_steps_in_lds,
    # which keeps its text (tests/test_ensemble_grid_lds_steps_abi.py counts it)
    assert shared.count("value_of(d_dt, dt, w.replica)") == 2 and shared.count("value_of(d_dt, dt, blockIdx.x)") == 1
    assert shared.count("whole_step_dt<REPLICA_DT>(d_dt, dt)") == 2  # (the two kernels where it had to be a template parameter)
    assert grid.count("value_of(d_dt, dt, replica)") == 1 and gabriel.count("value_of(d_dt, dt, replica)") == 1
    assert gabriel.count("value_of(d_coefficients, gabriel_coefficient, ") == 3
    assert "Step_dt" not in grid + gabriel, "the forms add overloads, not another plan"
