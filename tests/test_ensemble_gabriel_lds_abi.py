"""libyalla_ensemble_gabriel_lds.so (include/yalla_ensemble_gabriel_lds.h) through the layers that need no GPU: the
library exports exactly its header's functions and the ctypes table mirrors it; set_param knows its three names (and
says so on a null handle, where nothing can be touched) while the old Gabriel library still knows one; THE LDS RULE of
ya::ens::gabriel_lds_steps (ya::ens::gabriel_lds_layout, include/ensemble_gabriel.cuh) restated here from its comment
and held to a stand-alone host program compiled from the header, as tests/test_lds_layout_host.py does for
ya::ens::lds_layout -- whose own values, printed by the same program, are still ensemble_support.lds_layout's; and
GabrielLdsEnsemble counts the launches a (stand-in) library's take_steps reports."""
import os
import subprocess

import numpy as np
import pytest
from ensemble_support import (LDS, STATIC_LDS, check_abi, check_models_name_bounds, check_only_the_c_abi_is_exported,
                              lds_layout, up16)
from test_ensemble_grid_lds_steps_abi import StandInLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER, PREFIX = "yalla_ensemble_gabriel_lds.h", "ya_gablds_"
EXTRAS = ["ya_gablds_set_cube_size", "ya_gablds_status", "ya_gablds_get_grid", "ya_gablds_dense_cells",
          "ya_gablds_lds_dense_cells", "ya_gablds_lds_bytes"]
CAP, GROUPS, DENSE_ARRAYS = 64, 16, 8
CAPACITY = {3: 1024, 4: 995, 5: 826, 7: 592, 8: 512}
MODEL_OF = {3: "relu", 5: "relu_po", 7: "relu_cell"}


def test_the_library_exports_exactly_its_header():
    from yalla_amd import _ffi
    names = check_abi(HEADER, PREFIX, _ffi.GABRIEL_LDS_ENSEMBLE_ABI, _ffi.GABRIEL_LDS_ENSEMBLE_LIB,
                      _ffi.gabriel_lds_ensemble_lib, 23, EXTRAS)
    old = {n.replace("ya_gabens_", PREFIX) for n in _ffi.GABRIEL_ENSEMBLE_ABI}
    assert set(names) - old == {"ya_gablds_lds_dense_cells", "ya_gablds_lds_bytes"} and old <= set(names)
    check_only_the_c_abi_is_exported(_ffi.GABRIEL_LDS_ENSEMBLE_LIB, PREFIX)


def test_the_models_are_the_gabriel_harness_s():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import gabriel_lds_models, gabriel_models
    assert gabriel_lds_models() == gabriel_models()
    lib = _ffi.gabriel_lds_ensemble_lib()
    check_models_name_bounds(lib.ya_gablds_models_name, lib.ya_gablds_models_count())
    # written once: both harnesses expand the shared header's table
    for source in ("ensemble_gabriel.hip", "ensemble_gabriel_lds.hip"):
        text = open(os.path.join(ROOT, "yalla_amd", "csrc", source)).read()
        assert "YA_GABRIEL_ENSEMBLE_MODELS(" in text and '"relu_plain"' not in text, source


def test_set_param_on_a_null_handle():
    """A known name is -3 (there is no ensemble to set it on), an unknown one -2, no name -3: decided before the handle
    is looked at.  The old Gabriel library still answers -2 to "lds_steps"."""
    from yalla_amd import _ffi
    lib = _ffi.gabriel_lds_ensemble_lib()
    for name in (b"gabriel_coefficient", b"lds_steps", b"lds_steps_max"):
        assert lib.ya_gablds_set_param(None, name, 1.0) == -3, name
    for name in (b"lds", b"lds_step_lanes", b"lds_step_lanes_used", b"lanes", b"sum_order", b"whole_steps", b""):
        assert lib.ya_gablds_set_param(None, name, 1.0) == -2, name
    assert lib.ya_gablds_set_param(None, None, 1.0) == -3
    assert lib.ya_gablds_lds_dense_cells(None) == -3
    old = _ffi.gabriel_ensemble_lib()
    assert old.ya_gabens_set_param(None, b"lds_steps", 1.0) == -2
    assert old.ya_gabens_set_param(None, b"lds_steps_max", 1.0) == -2
    assert old.ya_gabens_set_param(None, b"gabriel_coefficient", 1.0) == -3


# ---- THE LDS RULE of ya::ens::gabriel_lds_steps, restated from include/ensemble_gabriel.cuh's header -----------------
def gabriel_lds_layout(n_floats, n_max):
    """(lists, dense_flags, dense, dense_sets, bytes): behind the grid form's one-lane layout, 16-byte aligned, the 16
    groups' lists of 64 entries of n_floats + 4 floats, a 4-byte slot and three bytes; where n_max > 64 one flag byte
    per slot and then, 16-byte aligned, the most of 4, 2, 1 sets of 8 lists of n_max 4-byte entries that fit the
    workgroup's 160 KiB beside the static fold scratch; bytes 0 = no room."""
    step = lds_layout(n_floats, n_max, keys=True)
    lists = up16(step.bytes)
    end = lists + GROUPS * CAP * ((n_floats + 4) * 4 + 4 + 3)
    flags = dense = sets = 0
    if n_max > CAP:
        flags, dense, one = end, up16(end + n_max), DENSE_ARRAYS * 4 * n_max
        sets = next((s for s in (4, 2, 1) if dense + s * one + STATIC_LDS <= LDS), 0)
        if sets == 0:
            return lists, flags, dense, 0, 0
        end = dense + sets * one
    return lists, flags, dense, sets, (end if end + STATIC_LDS <= LDS else 0)


def sizes(n_floats):
    return [1, 16, 64, 65, 256, 1024, CAPACITY[n_floats], CAPACITY[n_floats] + 1]


SRC = r'''
#include <stdio.h>
#include "ensemble.cuh"
MAKE_PT(Pt7, a, b, c, d);
MAKE_PT(Pt8, a, b, c, d, e);
template<typename Pt>
void print(const int capacity)
{
    for (const int n : {1, 16, 64, 65, 256, 1024, capacity, capacity + 1}) {
        const ya::ens::Gabriel_lds_layout g = ya::ens::gabriel_lds_layout<Pt>(n);
        const ya::ens::Lds_layout l = ya::ens::lds_layout<Pt, true, false>(n, 0, 1);
        printf("%d %d : %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %zu : %zu %zu %zu %d %zu : %d\n", ya::N_floats<Pt>::value, n,
            l.X, l.X1, l.dX, l.dX1, l.old_v, l.fold, l.partials, l.keys, l.list, l.terms, l.tile, l.bytes,
            g.lists, g.dense_flags, g.dense, g.dense_sets, g.bytes, (int)(g.step.bytes == l.bytes && g.step.keys == l.keys));
    }
    printf("capacity %d %d\n", ya::N_floats<Pt>::value, ya::ens::gabriel_lds_capacity<Pt>());
}
int main()
{
    print<float3>(1024), print<float4>(995), print<Po_cell>(826), print<Pt7>(592), print<Pt8>(512);
    return 0;
}
'''


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gabriel_lds_layout")
    src, exe = tmp / "layout.hip", tmp / "layout"
    src.write_text(SRC)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1",
                    "-DYALLA_NO_THRUST", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


def test_the_rule_is_the_restatement_and_lds_layout_is_unchanged(printed):
    want = []
    for n_floats in (3, 4, 5, 7, 8):
        for n in sizes(n_floats):
            step = lds_layout(n_floats, n, keys=True)   # (ensemble_support's restatement, as it was)
            want.append("%d %d : 0 %s : %s : 1" % (n_floats, n, " ".join(str(x) for x in step),
                                                  " ".join(str(x) for x in gabriel_lds_layout(n_floats, n))))
        want.append("capacity %d %d" % (n_floats, CAPACITY[n_floats]))
    assert printed == want


def test_the_capacities():
    """The largest n_max with room, at most 1024 (WHOLE_STEP_MAX_ROWS: the step's partial sums); one more has none.
    float3 reaches 1024 rows with one set of dense lists (142384 bytes); an 8-float point stops at 512, where the keys
    double."""
    for n_floats, capacity in CAPACITY.items():
        fits = [n for n in range(1, 1025) if gabriel_lds_layout(n_floats, n)[4] > 0]
        assert fits == list(range(1, capacity + 1)), n_floats
    assert gabriel_lds_layout(3, 1024) == (72752, 108592, 109616, 1, 142384)
    assert gabriel_lds_layout(3, 64) == (7472, 0, 0, 0, 43312)     # no dense lists: small replicas share a CU
    assert gabriel_lds_layout(3, 65)[3] == 4 and gabriel_lds_layout(3, 700)[3] == 2
    assert gabriel_lds_layout(8, 512)[3:] == (1, 157312) and gabriel_lds_layout(8, 513)[3:] == (0, 0)


def test_lds_bytes_is_the_rule():
    from yalla_amd.ensemble import GabrielLdsEnsemble, YallaError
    for n_floats, model in MODEL_OF.items():
        for n in sizes(n_floats) + [2000]:
            want = gabriel_lds_layout(n_floats, n)[4] if n <= 1024 else 0
            assert GabrielLdsEnsemble.lds_bytes(model, n) == want, (model, n)
    with pytest.raises(YallaError, match="-1"):
        GabrielLdsEnsemble.lds_bytes("no_such_model", 10)
    with pytest.raises(YallaError, match="-3"):
        GabrielLdsEnsemble.lds_bytes("relu", 0)


def test_the_engine_header_defines_the_pieces():
    text = lambda *path: open(os.path.join(ROOT, *path)).read()
    engine = text("include", "ensemble_gabriel.cuh")
    for piece in ("void gabriel_lds_steps(", "constexpr Gabriel_lds_layout gabriel_lds_layout(const int n_max)",
                  "constexpr int gabriel_lds_capacity()", "int lds_steps = 0;", "int lds_steps_max = 256;",
                  "long lds_step_launches = 0;", "unsigned long long lds_dense_cells()",
                  "inline bool gabriel_lds_steps_pay(const int n_replicas, const int n_max, const int n_cubes)"):
        assert piece in engine, piece
    # the step in LDS exists once, and so do the Gabriel stages' decisions (include/solvers.cuh)
    assert engine.count("whole_steps_in_lds<Pt>(") == 1 and "heun_row" not in engine
    solvers = text("include", "solvers.cuh")
    for once in ("void selection_sort(", "bool occluded(", "void rank_list(", "void test_and_sum(", "int collect(",
                 "void cell_by_group(", "hit = !(dist >= cube_size)"):
        assert solvers.count(once) == 1 and once not in engine, once
    assert "selection_sort" not in engine and "dist >= cube_size" not in engine
    # the old harness and its header know nothing of this
    old = text("yalla_amd", "csrc", "ensemble_gabriel.hip") + text("include", "yalla_ensemble_gabriel.h")
    assert "lds_steps" not in old


class GabrielLdsStandIn(StandInLibrary):
    prefix = PREFIX


def test_the_python_class_counts_what_take_steps_reports():
    from yalla_amd.ensemble import GabrielEnsemble, GabrielLdsEnsemble, YallaError
    assert issubclass(GabrielLdsEnsemble, GabrielEnsemble)
    ens = GabrielLdsEnsemble("relu", 2, 4, 8, 1.0, 0.8, lib=GabrielLdsStandIn([0, 3, 1, -3]))
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
    with pytest.raises(AttributeError):
        ens.lds_step_lanes_used  # (there is no lanes knob)
    ens.close()
    assert isinstance(GabrielLdsEnsemble.lds_step_launches, property)
    assert isinstance(GabrielLdsEnsemble.__dict__["lds_bytes"], staticmethod)
