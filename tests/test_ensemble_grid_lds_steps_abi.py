"""The grid ensemble's launches that step from LDS through the layers that need no GPU: ya_gens_set_param knows the two
settings (and says so on a null handle, where nothing can be touched), the C header documents them and what
ya_gens_take_steps returns, the engine header defines the pieces, and the Python class counts the launches a (stand-in)
library reports.  The harness exports no new function for this -- the count travels as ya_gens_take_steps' return
value -- so tests/test_ensemble_grid_abi.py holds as it stands."""
import ctypes
import os

import numpy as np
import pytest
from ensemble_grid_lds_support import grid_lds_capacity
from ensemble_support import LDS, STATIC_LDS, lds_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_set_param_on_a_null_handle():
    """A known name is -3 (there is no ensemble to set it on), an unknown one -2, no name -3: decided before the handle
    is looked at."""
    from yalla_amd import _ffi
    lib = _ffi.grid_ensemble_lib()
    for name in (b"lds_steps", b"lds_steps_max", b"lanes", b"sum_order"):
        assert lib.ya_gens_set_param(None, name, 1.0) == -3, name
    for name in (b"lds", b"whole_steps", b"steps_per_launch", b"gabriel_coefficient", b""):
        assert lib.ya_gens_set_param(None, name, 1.0) == -2, name
    assert lib.ya_gens_set_param(None, None, 1.0) == -3


def test_the_gabriel_harness_knows_neither_name():
    from yalla_amd import _ffi
    lib = _ffi.gabriel_ensemble_lib()
    for name in (b"lds_steps", b"lds_steps_max", b"whole_steps"):
        assert lib.ya_gabens_set_param(None, name, 1.0) == -2, name


def test_the_header_documents_the_settings_and_the_count():
    header = text("include", "yalla_ensemble_grid.h")
    for name in ('"lds_steps"', '"lds_steps_max"', "lds_step_launches"):
        assert name in header, name
    comment_before_take_steps = header[:header.index("int ya_gens_take_steps(")].rsplit("/*", 1)[1]
    assert "Returns the number of launches that stepped from LDS" in comment_before_take_steps
    harness = text("yalla_amd", "csrc", "ensemble_grid.hip")
    assert '"lds_steps"' in harness and '"lds_steps_max"' in harness
    assert "cells.lds_steps = -1" in harness, "the harness keeps the 14-launch step as its default"
    gabriel = text("yalla_amd", "csrc", "ensemble_gabriel.hip") + text("include", "yalla_ensemble_gabriel.h")
    assert "lds_steps" not in gabriel


def test_the_engine_header_defines_the_pieces():
    engine = text("include", "ensemble_grid.cuh")
    for piece in ("void grid_lds_steps(", "lds_layout<Pt, true, LINKED>(", "constexpr int grid_lds_capacity()",
                  "inline bool lds_steps_pay(const int n_replicas, const int n_max, const int n_cubes)",
                  "int lds_steps = 0;", "int lds_steps_max = 256;", "long lds_step_launches = 0;",
                  "void take_steps(float dt, int n_steps"):
        assert piece in engine, piece
    # the step in LDS exists once: the all-pairs kernels and the grid kernel call the same function
    shared = text("include", "ensemble.cuh")
    assert shared.count("void whole_steps_in_lds(") == 1 and engine.count("whole_steps_in_lds<Pt>(") == 1
    # ... and so does the LDS rule, for both forms
    assert shared.count("constexpr Lds_layout lds_layout(") == 1 and "constexpr Lds_layout" not in engine
    assert shared.count("ya::heun_row(local, dt, fix_first") == 1 and "heun_row" not in engine


def test_the_lds_rule_restated():
    """3-, 5-, 7- and 8-float points: all of them fit 1024 rows, the 8-float one with 896 bytes to spare."""
    for n_floats in (3, 4, 5, 7, 8):
        assert grid_lds_capacity(n_floats) == 1024
    assert LDS - STATIC_LDS - lds_layout(8, 1024, keys=True).bytes == 896
    assert lds_layout(3, 600, keys=True).bytes - lds_layout(3, 514, keys=True).bytes == 86 * 60  # (both lay out 1024 keys)
    assert lds_layout(3, 514, keys=True).bytes - lds_layout(3, 512, keys=True).bytes == 2 * 60 + 8 * 512  # (512 rows lay out 512)


class StandInLibrary:
    """The few ya_gens_* entry points GridEnsemble's constructor and take_step call; take_steps reports a scripted
    number of launches."""
    prefix = "ya_gens_"

    def __init__(self, reports):
        self.reports = list(reports)
        self.rows = (ctypes.c_float * (2 * 4 * 3))()

    def __getattr__(self, name):
        if not name.startswith(self.prefix):
            raise AttributeError(name)
        return getattr(self, "_" + name[len(self.prefix):])

    def _create(self, model, n_replicas, n_max, *values_and_out):
        values_and_out[-1]._obj.value = 1
        return 0

    def _n_floats(self, handle):
        return 3

    def _h_X(self, handle):
        return ctypes.cast(self.rows, ctypes.POINTER(ctypes.c_float))

    def _take_steps(self, handle, dt, steps):
        return self.reports.pop(0)

    def _destroy(self, handle):
        pass


class GabrielStandIn(StandInLibrary):
    prefix = "ya_gabens_"


def test_the_python_class_counts_what_take_steps_reports():
    from yalla_amd.ensemble import GabrielEnsemble, GridEnsemble, YallaError
    ens = GridEnsemble("relu", 2, 4, 8, 1.0, lib=StandInLibrary([0, 3, 1, -3]))
    assert ens.lds_step_launches == 0 and np.shape(ens.h_X) == (2, 4, 3)
    ens.take_step(0.1, 5)
    assert ens.lds_step_launches == 0
    ens.take_step(0.1, 7)
    ens.take_step(0.1, 1)
    assert ens.lds_step_launches == 4
    with pytest.raises(YallaError, match="-3"):  # a harness error is still an error
        ens.take_step(0.1, 1)
    assert ens.lds_step_launches == 4
    with pytest.raises(AttributeError):
        ens.lds_step_launches = 0  # read-only
    with pytest.raises(AttributeError):
        ens.whole_step_launches
    ens.close()
    assert isinstance(GridEnsemble.lds_step_launches, property)
    # the Gabriel class has none
    gab = GabrielEnsemble("relu", 2, 4, 8, 1.0, 0.8, lib=GabrielStandIn([0]))
    gab.take_step(0.1, 1)
    with pytest.raises(AttributeError):
        gab.lds_step_launches
    with pytest.raises(AttributeError):
        GabrielEnsemble.lds_step_launches.fget(object())
    gab.close()
