"""libyalla_ensemble_grid.so (include/yalla_ensemble_grid.h) loads without a GPU, exports exactly the C ABI its
header declares and the ctypes table mirrors, and refuses what it does not know (no compute calls here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "yalla_amd", "libyalla_ensemble_grid.so")
MODELS = ["springs", "clipped", "fading", "relu", "relu_po", "relu_cell", "push", "clipped_push"]


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


def test_header_table_and_library_agree():
    from yalla_amd import _ffi
    names = declared_functions("yalla_ensemble_grid.h")
    assert len(names) == 20 and all(n.startswith("ya_gens_") for n in names)
    assert set(names) == set(_ffi.GRID_ENSEMBLE_ABI), "ctypes table and header disagree"
    # the all-pairs harness's functions, and the grid's own
    from_tile = {n.replace("ya_ens_", "ya_gens_") for n in _ffi.ENSEMBLE_ABI}
    assert set(names) - from_tile == {"ya_gens_set_cube_size", "ya_gens_status", "ya_gens_get_grid"}
    assert from_tile <= set(names)
    functions = {sym for kind, sym in exported(LIB) if kind == "T" and sym.startswith("ya_")}
    assert functions == set(names), "library and header disagree"
    lib = _ffi.grid_ensemble_lib()  # types every entry point; AttributeError if one is missing
    assert lib is _ffi.grid_ensemble_lib()
    assert _ffi.GRID_ENSEMBLE_LIB == LIB


def test_only_the_grid_ensemble_c_abi_is_exported():
    """-fvisibility=hidden: nothing but ya_gens_* and the HIP registration symbols (fatbin wrapper, kernel handles
    and stubs' data) leaves the library -- no engine or harness C++ symbol, no entry point of another harness."""
    for kind, sym in exported(LIB):
        if sym.startswith("ya_gens_") or sym.startswith("__hip") or kind in ("V", "D", "B", "R"):
            continue
        raise AssertionError(f"{kind} {sym}")
    assert not [sym for _, sym in exported(LIB) if sym.startswith("ya_") and not sym.startswith("ya_gens_")]


def test_the_model_table():
    from yalla_amd import GridEnsemble, ensemble  # noqa: F401  (the package exports the class)
    names = ensemble.grid_models()
    assert names == MODELS
    lib = ensemble._ffi.grid_ensemble_lib()
    assert lib.ya_gens_models_name(-1) is None and lib.ya_gens_models_name(len(names)) is None


def test_unknown_models_and_bad_sizes_are_refused_before_the_device_is_touched():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import GridEnsemble, YallaError
    lib = _ffi.grid_ensemble_lib()
    handle = ctypes.c_void_p()
    for name in (b"springs_grid", b"relu_tile", b"oscillator", b"", b"no_such_model"):
        assert lib.ya_gens_create(name, 4, 100, 8, 1.0, ctypes.byref(handle)) == -1
        assert not handle.value
    bad = [
        (0, 100, 8), (4, 0, 8), (-1, 5, 8), (4, 100, 0),
        (70000, 70000, 8),     # n_replicas * n_max > 2^31 - 1: ids are ints
        (2 ** 24, 100, 8),     # n_replicas * (grid_size^3 + 1) > 2^31 - 1: 2^24 * 513
        (128, 10, 256),        # the same with the largest grid: 128 * (2^24 + 1)
        (4, 100, 257),         # grid_size > YA_MAX_GRID_SIZE: cube ids are binary32
    ]
    for m, n, gs in bad:
        assert lib.ya_gens_create(b"springs", m, n, gs, 1.0, ctypes.byref(handle)) == -3, (m, n, gs)
        assert not handle.value
    assert lib.ya_gens_create(b"springs", 4, 100, 8, 0.0, ctypes.byref(handle)) == -3  # cube_size
    assert not handle.value
    with pytest.raises(YallaError, match="unknown grid ensemble model"):
        GridEnsemble("springs_grid", 4, 100, 8)
