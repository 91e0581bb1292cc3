"""libyalla_ensemble.so (include/yalla_ensemble.h) loads without a GPU, exports exactly the C ABI its header
declares and the ctypes table mirrors, and refuses what it does not know (no compute calls here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "yalla_amd", "libyalla_ensemble.so")


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
    names = declared_functions("yalla_ensemble.h")
    assert len(names) == 17 and all(n.startswith("ya_ens_") for n in names)
    assert set(names) == set(_ffi.ENSEMBLE_ABI), "ctypes table and header disagree"
    functions = {sym for kind, sym in exported(LIB) if kind == "T" and sym.startswith("ya_")}
    assert functions == set(names), "library and header disagree"
    lib = _ffi.ensemble_lib()  # types every entry point; AttributeError if one is missing
    assert lib is _ffi.ensemble_lib()
    assert _ffi.ENSEMBLE_LIB == LIB


def test_only_the_ensemble_c_abi_is_exported():
    """-fvisibility=hidden: nothing but ya_ens_* and the HIP registration symbols (fatbin wrapper, kernel
    handles and stubs' data) leaves the library -- no engine or harness C++ symbol, and no ya_sim_* / ya_models_*
    entry point of the model harness."""
    for kind, sym in exported(LIB):
        if sym.startswith("ya_ens_") or sym.startswith("__hip") or kind in ("V", "D", "B", "R"):
            continue
        raise AssertionError(f"{kind} {sym}")
    assert not [sym for _, sym in exported(LIB) if sym.startswith("ya_") and not sym.startswith("ya_ens_")]


def test_the_model_table():
    from yalla_amd import ensemble
    names = ensemble.models()
    assert names == ["springs", "clipped", "fading", "relu", "relu_po", "oscillator", "push"]
    lib = ensemble._ffi.ensemble_lib()
    assert lib.ya_ens_models_name(-1) is None and lib.ya_ens_models_name(len(names)) is None


def test_unknown_models_and_bad_sizes_are_refused_before_the_device_is_touched():
    from yalla_amd import _ffi
    from yalla_amd.ensemble import Ensemble, YallaError
    lib = _ffi.ensemble_lib()
    handle = ctypes.c_void_p()
    for name in (b"springs_tile", b"relu_grid", b"", b"no_such_model"):
        assert lib.ya_ens_create(name, 4, 100, ctypes.byref(handle)) == -1
        assert not handle.value
    for m, n in ((0, 100), (4, 0), (-1, 5), (70000, 70000)):  # the last: ids are ints
        assert lib.ya_ens_create(b"springs", m, n, ctypes.byref(handle)) == -3
        assert not handle.value
    with pytest.raises(YallaError, match="unknown ensemble model"):
        Ensemble("springs_tile", 4, 100)
