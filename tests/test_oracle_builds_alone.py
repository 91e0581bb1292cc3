"""The model harness (yalla_amd/csrc/models_harness.inc) is compiled into the CPU oracle too, whose Solution has
no take_steps: everything the harness does with it sits under `#if YA_IS_DEVICE`.  The guard: `make -C oracle`
into an empty output directory succeeds and the library it makes loads as the oracle."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_builds_from_nothing_and_loads(tmp_path):
    out = tmp_path / "oracle_build"
    proc = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), f"OUT={out}"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    from yalla_amd import _ffi
    lib = _ffi.bind(str(out / "liboracle_models.so"))  # (every entry point of include/yalla_models.h)
    assert lib.ya_models_is_device() == 0
    assert lib.ya_models_count() > 0
    assert not hasattr(lib, "ya_sim_carried_steps")  # device build only
