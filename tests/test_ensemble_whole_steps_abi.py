"""Whole-step launches through the layers that need no GPU: the C header documents the two settings and what
ya_ens_take_steps returns, the harness source accepts them, the engine header defines the pieces, and the Python
class counts the launches a (stand-in) library reports.  The harness exports no new function for this -- the count
travels as ya_ens_take_steps' return value -- so tests/test_ensemble_abi.py holds as it stands."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_documents_the_settings_and_the_count():
    header = text("include", "yalla_ensemble.h")
    for name in ('"whole_steps"', '"steps_per_launch"', "whole_step_launches"):
        assert name in header, name
    comment_before_take_steps = header[:header.index("int ya_ens_take_steps(")].rsplit("/*", 1)[1]
    assert "Returns the number of whole-step launches" in comment_before_take_steps
    harness = text("yalla_amd", "csrc", "ensemble.hip") + text("yalla_amd", "csrc", "ensemble_harness.h")
    assert '"whole_steps"' in harness and '"steps_per_launch"' in harness
    assert re.search(r"cells\.whole_steps = -1", harness), "the harness keeps the six-launch step as its default"
    grid_harness = text("yalla_amd", "csrc", "ensemble_grid.hip") + text("include", "yalla_ensemble_grid.h")
    assert "whole_steps" not in grid_harness and "steps_per_launch" not in grid_harness


def test_the_engine_header_defines_the_pieces():
    engine = text("include", "ensemble.cuh")
    for piece in ("void whole_steps(", "constexpr int whole_step_capacity()", "inline bool whole_steps_pay(",
                  "void take_steps(float dt, int n_steps", "int whole_steps = 0;", "int steps_per_launch = 256;",
                  "long whole_step_launches = 0;"):
        assert piece in engine, piece
    # the pair body exists once, called by the tiled loop and by the whole-step kernel
    solvers = text("include", "solvers.cuh")
    assert solvers.count("void tile_pair(") == 1
    assert len(re.findall(r"tile_pair<Pt, pw_int, pw_friction>\(", solvers + engine)) == 2


class StandInLibrary:
    """The few ya_ens_* entry points Ensemble's constructor and take_step call; take_steps reports a scripted number
    of whole-step launches."""

    def __init__(self, reports):
        self.reports = list(reports)
        self.rows = (ctypes.c_float * (2 * 4 * 3))()

    def ya_ens_create(self, model, n_replicas, n_max, out):
        out._obj.value = 1
        return 0

    def ya_ens_n_floats(self, handle):
        return 3

    def ya_ens_h_X(self, handle):
        return ctypes.cast(self.rows, ctypes.POINTER(ctypes.c_float))

    def ya_ens_take_steps(self, handle, dt, steps):
        return self.reports.pop(0)

    def ya_ens_destroy(self, handle):
        pass


def test_the_python_class_counts_what_take_steps_reports():
    from yalla_amd.ensemble import Ensemble, GridEnsemble, YallaError
    ens = Ensemble("relu", 2, 4, lib=StandInLibrary([0, 3, 1, -3]))
    assert ens.whole_step_launches == 0 and np.shape(ens.h_X) == (2, 4, 3)
    ens.take_step(0.1, 5)
    assert ens.whole_step_launches == 0
    ens.take_step(0.1, 7)
    ens.take_step(0.1, 1)
    assert ens.whole_step_launches == 4
    with pytest.raises(YallaError, match="-3"):  # a harness error is still an error
        ens.take_step(0.1, 1)
    assert ens.whole_step_launches == 4
    with pytest.raises(AttributeError):
        ens.whole_step_launches = 0  # read-only
    ens.close()
    assert isinstance(Ensemble.whole_step_launches, property)
    with pytest.raises(AttributeError):  # a grid ensemble has none
        GridEnsemble.whole_step_launches.fget(object())
