"""Shared by tests/test_point_widths.py (host) and tests/test_point_widths_gpu.py: the two libraries built from
yalla_amd/csrc/widths_models.h -- models::field_coupling on points of 4, 6, 8, 9, 11 and 16 floats -- bound through
the model harness's ctypes ABI, the point types' constants, and the start states with every extra field filled.

The libraries are libyalla_models.so's and the oracle's translation units with another model table
(-DYA_MODELS_WIDTHS); libyalla_models.so itself keeps its table."""
import os
import subprocess

import numpy as np
import pytest

from yalla_amd import _ffi
from yalla_amd.solution import Solution

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
WIDTHS_ORACLE_LIB = os.path.join(ORACLE_DIR, "_build", "liboracle_models_widths.so")
WIDTHS_DEVICE_LIB = os.path.join(ROOT, "yalla_amd", "libyalla_models_widths.so")

# type -> floats per point.  The order of yalla_amd/csrc/widths_models.h.
WIDTH = {"float4": 4, "w4": 4, "w6": 6, "w8": 8, "w9": 9, "w11": 11, "w16": 16}
GRID_TYPES = list(WIDTH)
TILE_TYPES = ["float4", "w6", "w11", "w16"]
GABRIEL_TYPES = TILE_TYPES
# field_coupling is declared YA_STATELESS for every type but these (widths_models.h): the solvers pick the
# one-lane-per-cell kernels for them by themselves
UNDECLARED = ("w9", "w6")

# Bytes of a cube-sorted entry {point, id}: the point and 4 bytes, padded to the point's alignment (float4: 16).
ENTRY_BYTES = {t: 4 * w + 4 for t, w in WIDTH.items()}
ENTRY_BYTES["float4"] = 32


def stage_capacity(entry_bytes):
    """Cells of a z-plane that grid_force_bits stages at once (include/solvers.cuh, ya::bits::Stage): 352 for
    entries of up to 24 bytes, 256 up to 32 bytes, 176 beyond.  widths_models.h holds each type to this with a
    static_assert, so a change of the rule breaks the build and not a test's premise."""
    return 352 if entry_bytes <= 24 else (256 if entry_bytes <= 32 else 176)


STAGE_CAPACITY = {t: stage_capacity(b) for t, b in ENTRY_BYTES.items()}
assert STAGE_CAPACITY == {"float4": 256, "w4": 352, "w6": 256, "w8": 176, "w9": 176, "w11": 176, "w16": 176}
PASS_BITS = 256  # candidates of a row that one pass of grid_force_bits' bit stream holds (YA_MASK_WORDS * 32)


def model(kind, solver):
    return f"fields_{kind}_{solver}"


def build_widths_oracle():
    srcs = [os.path.join(ORACLE_DIR, f) for f in ("oracle_models.cpp", "yalla_host.hpp")]
    srcs += [os.path.join(ROOT, "yalla_amd", "csrc", f)
             for f in ("model_functors.h", "models_harness.inc", "widths_models.h", "gabriel_host.h")]
    srcs.append(os.path.join(ROOT, "include", "slab_logic.inc"))
    stale = (not os.path.exists(WIDTHS_ORACLE_LIB) or
             any(os.path.getmtime(s) > os.path.getmtime(WIDTHS_ORACLE_LIB) for s in srcs))
    if stale:
        subprocess.run(["make", "-C", ORACLE_DIR, "_build/liboracle_models_widths.so"], check=True,
                       capture_output=True)
    return WIDTHS_ORACLE_LIB


@pytest.fixture(scope="module")
def widths_oracle():
    lib = _ffi.bind(build_widths_oracle())
    assert lib.ya_models_is_device() == 0
    return lib


@pytest.fixture(scope="module")
def widths_device():
    lib = _ffi.bind(WIDTHS_DEVICE_LIB)  # raises if it has not been built: there is no fallback
    assert lib.ya_models_is_device() == 1 and lib.ya_models_arith() == 0
    return lib


def extra_fields(n, width):
    """(n, width - 3) binary32 values for the fields behind x, y, z: odd multiples of 2^-13 in (-1, 1), so never 0, a
    different value in every cell of a column (n <= 6000), and no two columns alike."""
    assert n <= 8191
    i = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(3, width, dtype=np.int64)[None, :]
    q = (i * (2 * k + 1) + 97 * k) % 8191        # a bijection of i for every k: 8191 is prime, 2 k + 1 < 8191
    v = (q - 4095).astype(np.float64) / 4096.0 - 2.0 ** -13    # odd multiples of 2^-13: never 0
    return v.astype(f32)


def start(s, n, dist, seed, X=None):
    """random_sphere(dist) (or the rows X) with every extra field filled from extra_fields, on the host and the
    device."""
    s.h_n = n
    if X is None:
        s.random_sphere(dist, seed)
    else:
        s.h_X[:n, :3] = X[:, :3]
    s.h_X[:n, 3:] = extra_fields(n, s.n_floats)
    s.copy_to_device()
    return s.h_X[:n].copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def result(s, n, with_grid):
    X = s.positions()
    out = {"X": X, "old_v": s.old_v()[:n].copy()}
    if with_grid:
        cube_id, point_id, cube_start, cube_end = s.grid()
        out.update(cube_id=cube_id[:n].copy(), point_id=point_id[:n].copy(), cube_start=cube_start, cube_end=cube_end)
    return out


def same(a, b, what=""):
    """Every field column of the positions, old_v and, where present, the four grid arrays: bit for bit."""
    assert a.keys() == b.keys(), what
    for key in a:
        assert a[key].shape == b[key].shape, (what, key)
        if key == "X":
            for k in range(a[key].shape[1]):
                assert np.array_equal(bits(a[key][:, k]), bits(b[key][:, k])), (what, f"field {k}")
        else:
            assert np.array_equal(bits(a[key]), bits(b[key])), (what, key)


def run(lib, name, n, *, dist=0.5, seed=7, gs=50, cs=1.0, dt=0.05, steps=2, setup=None, tree=True, X=None, n_max=None):
    """The model's state after `steps` Heun steps from start(); the oracle in the engine's reduce order."""
    with Solution(name, n_max or n, gs, cs, lib=lib) as s:
        if lib.ya_models_is_device() == 0 and tree:
            assert s.set_reduce_order(1) == 0
        first = start(s, n, dist, seed, X)
        if setup:
            setup(s)
        s.take_step(dt, steps)
        out = result(s, n, "_tile" not in name)
    out["first"] = first
    return out
