"""ctypes binding of the model-harness C ABI (include/yalla_models.h).

`bind(path)` loads any shared library that implements that header and declares
the argument types of every entry point.  `device_lib()` loads the HIP build,
yalla_amd/libyalla_models.so (which pulls in libyalla_hip.so through its
$ORIGIN rpath) and raises if it is missing: the product has no CPU fallback.
"""
import ctypes as C
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# YALLA_MODELS_LIB: another build of the same library (A/B of build flags, tools/gpu_*.sh)
DEVICE_LIB = os.environ.get("YALLA_MODELS_LIB") or os.path.join(_HERE, "libyalla_models.so")
DEVICE_LIB_FAST = os.path.join(_HERE, "libyalla_models_fast.so")  # the fast-arithmetic tier
CORE_LIB = os.path.join(_HERE, "libyalla_hip.so")
ENSEMBLE_LIB = os.path.join(_HERE, "libyalla_ensemble.so")  # include/yalla_ensemble.h
GRID_ENSEMBLE_LIB = os.path.join(_HERE, "libyalla_ensemble_grid.so")  # include/yalla_ensemble_grid.h
GABRIEL_ENSEMBLE_LIB = os.path.join(_HERE, "libyalla_ensemble_gabriel.so")  # include/yalla_ensemble_gabriel.h
GABRIEL_LDS_ENSEMBLE_LIB = os.path.join(_HERE, "libyalla_ensemble_gabriel_lds.so")  # include/yalla_ensemble_gabriel_lds.h
LINKED_ENSEMBLE_LIB = os.path.join(_HERE, "libyalla_ensemble_links.so")  # include/yalla_ensemble_links.h
LINKED_GRID_ENSEMBLE_LIB = os.path.join(_HERE, "libyalla_ensemble_grid_links.so")  # include/yalla_ensemble_grid_links.h
SWEEP_ENSEMBLE_LIB = os.path.join(_HERE, "libyalla_ensemble_sweep.so")  # include/yalla_ensemble_sweep.h

_pf = C.POINTER(C.c_float)
_pi = C.POINTER(C.c_int)
_sim = C.c_void_p

# name -> (restype, argtypes); mirrors include/yalla_models.h one to one.
MODELS_ABI = {
    "ya_models_is_device": (C.c_int, []),
    "ya_models_arith": (C.c_int, []),
    "ya_models_count": (C.c_int, []),
    "ya_models_name": (C.c_char_p, [C.c_int]),
    "ya_sim_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_float, C.POINTER(_sim)]),
    "ya_sim_destroy": (None, [_sim]),
    "ya_sim_n_floats": (C.c_int, [_sim]),
    "ya_sim_n_max": (C.c_int, [_sim]),
    "ya_sim_h_X": (_pf, [_sim]),
    "ya_sim_set_h_n": (C.c_int, [_sim, C.c_int]),
    "ya_sim_get_h_n": (C.c_int, [_sim]),
    "ya_sim_copy_to_device": (C.c_int, [_sim]),
    "ya_sim_copy_to_host": (C.c_int, [_sim]),
    "ya_sim_get_d_n": (C.c_int, [_sim]),
    "ya_sim_take_steps": (C.c_int, [_sim, C.c_float, C.c_int]),
    "ya_sim_synchronize": (C.c_int, [_sim]),
    "ya_sim_set_fixed": (C.c_int, [_sim, C.c_int, C.c_int]),
    "ya_sim_set_cube_size": (C.c_int, [_sim, C.c_float]),
    "ya_sim_random_sphere": (C.c_int, [_sim, C.c_float, C.c_uint]),
    "ya_sim_get_old_v": (C.c_int, [_sim, _pf]),
    "ya_sim_set_old_v": (C.c_int, [_sim, _pf]),
    "ya_sim_get_grid": (C.c_int, [_sim, _pi, _pi, _pi, _pi]),
    "ya_sim_build_grid": (C.c_int, [_sim, C.c_int, C.c_float, _pi, _pi, _pi, _pi]),
    "ya_sim_set_param": (C.c_int, [_sim, C.c_char_p, C.c_double]),
    "ya_sim_set_prop": (C.c_int, [_sim, C.c_char_p, _pi, C.c_int]),
    "ya_sim_get_prop": (C.c_int, [_sim, C.c_char_p, _pi, C.c_int]),
    "ya_sim_set_links": (C.c_int, [_sim, _pi, C.c_int, C.c_float]),
    "ya_sim_set_reduce_order": (C.c_int, [_sim, C.c_int]),
    "ya_slab_init": (C.c_int, [_sim, C.c_float, C.c_float, C.c_float, _pi]),
    "ya_slab_info": (C.c_long, [_sim, C.c_int]),
    "ya_slab_n_own": (C.c_int, [_sim]),
    "ya_slab_n_local": (C.c_int, [_sim]),
    "ya_slab_setup": (C.c_int, [_sim, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ya_slab_set_transport": (C.c_int, [_sim, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ya_slab_use_rccl": (C.c_int, [_sim, C.c_void_p]),
    "ya_slab_step": (C.c_int, [_sim, C.c_float, C.c_int]),
    "ya_slab_get_own": (C.c_int, [_sim, _pf, _pi]),
    "ya_slab_plan": (C.c_int, [_pf, C.c_int, C.c_int, C.c_int, C.c_float, _pf, _pi]),
    "ya_slab_decompose": (C.c_int, [_sim, _pf, C.c_int, C.c_int, C.c_int, C.c_float]),
    "ya_check_sqrt": (C.c_long, [C.c_uint, C.c_uint]),
    "ya_check_reciprocal": (C.c_long, [C.c_uint, C.c_uint]),
    "ya_sim_profile": (C.c_int, [_sim, C.c_int]),
    "ya_sim_profile_read": (C.c_int, [_sim, C.POINTER(C.c_double), _pi]),
    "ya_sim_graph_launches": (C.c_long, [_sim]),
}

# name -> (restype, argtypes); mirrors include/yalla_ensemble.h one to one.
_ens = C.c_void_p
ENSEMBLE_ABI = {
    "ya_ens_models_count": (C.c_int, []),
    "ya_ens_models_name": (C.c_char_p, [C.c_int]),
    "ya_ens_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(_ens)]),
    "ya_ens_destroy": (None, [_ens]),
    "ya_ens_n_floats": (C.c_int, [_ens]),
    "ya_ens_h_X": (_pf, [_ens]),
    "ya_ens_set_h_n": (C.c_int, [_ens, C.c_int, C.c_int]),
    "ya_ens_get_h_n": (C.c_int, [_ens, C.c_int]),
    "ya_ens_get_d_n": (C.c_int, [_ens, C.c_int]),
    "ya_ens_copy_to_device": (C.c_int, [_ens]),
    "ya_ens_copy_to_host": (C.c_int, [_ens]),
    "ya_ens_take_steps": (C.c_int, [_ens, C.c_float, C.c_int]),
    "ya_ens_synchronize": (C.c_int, [_ens]),
    "ya_ens_set_fixed": (C.c_int, [_ens, C.c_int, C.c_int]),
    "ya_ens_get_old_v": (C.c_int, [_ens, _pf]),
    "ya_ens_set_old_v": (C.c_int, [_ens, _pf]),
    "ya_ens_set_param": (C.c_int, [_ens, C.c_char_p, C.c_double]),
}

# name -> (restype, argtypes); mirrors include/yalla_ensemble_grid.h one to one: the ensemble's functions under
# another prefix, create with the grid's size and cube size, set_cube_size, status and get_grid.
GRID_ENSEMBLE_ABI = {name.replace("ya_ens_", "ya_gens_"): sig for name, sig in ENSEMBLE_ABI.items()}
GRID_ENSEMBLE_ABI["ya_gens_create"] = (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(_ens)])
GRID_ENSEMBLE_ABI["ya_gens_set_cube_size"] = (C.c_int, [_ens, C.c_float])
GRID_ENSEMBLE_ABI["ya_gens_status"] = (C.c_int, [_ens, C.c_int, C.c_int])
GRID_ENSEMBLE_ABI["ya_gens_get_grid"] = (C.c_int, [_ens, C.c_int, _pi, _pi, _pi, _pi])

# name -> (restype, argtypes); mirrors include/yalla_ensemble_gabriel.h one to one: the grid ensemble's functions
# under another prefix, create with the coefficient, and dense_cells.
GABRIEL_ENSEMBLE_ABI = {name.replace("ya_gens_", "ya_gabens_"): sig for name, sig in GRID_ENSEMBLE_ABI.items()}
GABRIEL_ENSEMBLE_ABI["ya_gabens_create"] = (
    C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(_ens)])
GABRIEL_ENSEMBLE_ABI["ya_gabens_dense_cells"] = (C.c_int, [_ens])

# name -> (restype, argtypes); mirrors include/yalla_ensemble_gabriel_lds.h one to one: the Gabriel ensemble's functions
# under another prefix (take_steps returns the launches that stepped from LDS), the in-launch dense count and the LDS
# rule.
GABRIEL_LDS_ENSEMBLE_ABI = {name.replace("ya_gabens_", "ya_gablds_"): sig for name, sig in GABRIEL_ENSEMBLE_ABI.items()}
GABRIEL_LDS_ENSEMBLE_ABI["ya_gablds_lds_dense_cells"] = (C.c_longlong, [_ens])
GABRIEL_LDS_ENSEMBLE_ABI["ya_gablds_lds_bytes"] = (C.c_long, [C.c_char_p, C.c_int])

# name -> (restype, argtypes); mirrors include/yalla_ensemble_links.h one to one: the ensemble's functions under
# another prefix, create with the slots per replica and the links' strength, the links' host mirror and count, the
# lanes of the last whole-step launch and the LDS rule.
LINKED_ENSEMBLE_ABI = {name.replace("ya_ens_", "ya_lens_"): sig for name, sig in ENSEMBLE_ABI.items()}
LINKED_ENSEMBLE_ABI["ya_lens_create"] = (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(_ens)])
LINKED_ENSEMBLE_ABI["ya_lens_h_link"] = (_pi, [_ens])
LINKED_ENSEMBLE_ABI["ya_lens_set_n_links"] = (C.c_int, [_ens, C.c_int])
LINKED_ENSEMBLE_ABI["ya_lens_get_n_links"] = (C.c_int, [_ens])
LINKED_ENSEMBLE_ABI["ya_lens_whole_step_lanes_used"] = (C.c_int, [_ens])
LINKED_ENSEMBLE_ABI["ya_lens_lds_bytes"] = (C.c_long, [C.c_char_p, C.c_int, C.c_int, C.c_int])

# name -> (restype, argtypes); mirrors include/yalla_ensemble_grid_links.h one to one: the grid ensemble's functions
# under another prefix, create with the slots per replica and the links' strength as well, the links' host mirror
# and count, and the LDS rule.
LINKED_GRID_ENSEMBLE_ABI = {name.replace("ya_gens_", "ya_glens_"): sig for name, sig in GRID_ENSEMBLE_ABI.items()}
LINKED_GRID_ENSEMBLE_ABI["ya_glens_create"] = (
    C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.POINTER(_ens)])
LINKED_GRID_ENSEMBLE_ABI["ya_glens_h_link"] = (_pi, [_ens])
LINKED_GRID_ENSEMBLE_ABI["ya_glens_set_n_links"] = (C.c_int, [_ens, C.c_int])
LINKED_GRID_ENSEMBLE_ABI["ya_glens_get_n_links"] = (C.c_int, [_ens])
LINKED_GRID_ENSEMBLE_ABI["ya_glens_lds_bytes"] = (C.c_long, [C.c_char_p, C.c_int, C.c_int])

# name -> (restype, argtypes); mirrors include/yalla_ensemble_sweep.h one to one: the shared entry points of the other
# harnesses under the prefix ya_swp_ (the model tables and create take the form's name), the grid forms' and the links'
# entry points, and what a time step and a Gabriel coefficient per replica add.
SWEEP_ENSEMBLE_ABI = {name.replace("ya_ens_", "ya_swp_"): sig for name, sig in ENSEMBLE_ABI.items()}
SWEEP_ENSEMBLE_ABI["ya_swp_models_count"] = (C.c_int, [C.c_char_p])
SWEEP_ENSEMBLE_ABI["ya_swp_models_name"] = (C.c_char_p, [C.c_char_p, C.c_int])
SWEEP_ENSEMBLE_ABI["ya_swp_create"] = (
    C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(_ens)])
SWEEP_ENSEMBLE_ABI["ya_swp_status"] = (C.c_int, [_ens, C.c_int, C.c_int])
SWEEP_ENSEMBLE_ABI["ya_swp_get_grid"] = (C.c_int, [_ens, C.c_int, _pi, _pi, _pi, _pi])
SWEEP_ENSEMBLE_ABI["ya_swp_h_link"] = (_pi, [_ens])
SWEEP_ENSEMBLE_ABI["ya_swp_set_n_links"] = (C.c_int, [_ens, C.c_int])
SWEEP_ENSEMBLE_ABI["ya_swp_get_n_links"] = (C.c_int, [_ens])
SWEEP_ENSEMBLE_ABI["ya_swp_set_dt"] = (C.c_int, [_ens, _pf])
SWEEP_ENSEMBLE_ABI["ya_swp_set_gabriel_coefficients"] = (C.c_int, [_ens, _pf])
SWEEP_ENSEMBLE_ABI["ya_swp_scale_dt"] = (C.c_int, [_ens, C.c_float])
SWEEP_ENSEMBLE_ABI["ya_swp_lanes_used"] = (C.c_int, [_ens])
SWEEP_ENSEMBLE_ABI["ya_swp_dense_cells"] = (C.c_int, [_ens])
SWEEP_ENSEMBLE_ABI["ya_swp_lds_dense_cells"] = (C.c_longlong, [_ens])

# include/yalla_hip.h, for the export check (no compute calls without a GPU).
CORE_ABI = [
    "ya_abi_version", "ya_malloc", "ya_free", "ya_memset_async", "ya_memcpy_h2d",
    "ya_memcpy_d2h", "ya_host_alloc", "ya_host_free", "ya_memcpy_d2d_async", "ya_device_synchronize", "ya_get_n",
    "ya_grid_create", "ya_grid_destroy", "ya_grid_arrays", "ya_grid_offsets",
    "ya_grid_build", "ya_grid_build_sorted", "ya_grid_build_sorted_begin", "ya_grid_build_sorted_begin_publish",
    "ya_grid_build_sorted_finish", "ya_grid_rebuild_sorted", "ya_grid_rebuild_sorted_map", "ya_grid_bin_target_get",
    "ya_grid_rebuild_sorted_binned", "ya_n_reader_create", "ya_n_reader_destroy",
    "ya_n_read_begin", "ya_n_read_end", "ya_grid_status", "ya_reduce_mean", "ya_reduce_sum_packed",
    "ya_reduce_workspace_bytes", "ya_select_z", "ya_select_workspace_bytes", "ya_gather_rows",
    "ya_gather_rows_pair",
    "ya_append_rows", "ya_comm_unique_id", "ya_comm_create", "ya_comm_create_loopback", "ya_comm_create_from_env",
    "ya_comm_destroy", "ya_comm_rank", "ya_comm_world", "ya_comm_exchange", "ya_comm_exchange_v",
    "ya_comm_allreduce_sum", "ya_comm_allreduce_host", "ya_comm_self_exchange", "ya_comm_info", "ya_reduce_partials",
    "ya_shader_clock_mhz", "ya_grid_set_cube_range", "ya_grid_forget_order", "ya_copy_component", "ya_pack_cells", "ya_append_cells", "ya_fill_holes", "ya_find_id", "ya_max_abs_diff", "ya_max_abs_diff_partials",
    "ya_slab_guard_update", "ya_slab_pack", "ya_async_read_create", "ya_async_read_destroy",
    "ya_async_read_begin", "ya_async_read_end", "ya_async_read_target", "ya_async_read_mark",
]


def _load(path, table):
    """Load `path` and type every entry point of `table`."""
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()')")
    lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    for name, (res, args) in table.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


def bind(path):
    """Load `path` and type every include/yalla_models.h entry point."""
    return _load(path, MODELS_ABI)


_device = {}


def device_lib(arith="exact"):
    """The HIP engine.  Raises if the extension has not been built.  arith "exact" (default:
    bit-comparable with the oracle) or "fast" (libyalla_models_fast.so: contracted multiply-adds,
    bare v_sqrt_f32 / v_rcp_f32; within 1e-5 relative of the exact tier)."""
    if arith not in ("exact", "fast"):
        raise ValueError("arith must be 'exact' or 'fast'")
    if arith not in _device:
        path = DEVICE_LIB if arith == "exact" else DEVICE_LIB_FAST
        lib = bind(path)
        if lib.ya_models_is_device() != 1 or lib.ya_models_arith() != (arith == "fast"):
            raise RuntimeError(f"{path} is not the {arith}-arithmetic HIP build")
        _device[arith] = lib
    return _device[arith]


@functools.lru_cache(maxsize=None)  # (the same object on every call)
def ensemble_lib():
    """The ensemble harness, yalla_amd/libyalla_ensemble.so (include/yalla_ensemble.h), every entry
    point typed.  Raises if it has not been built: there is no fallback."""
    return _load(ENSEMBLE_LIB, ENSEMBLE_ABI)


@functools.lru_cache(maxsize=None)  # (the same object on every call)
def grid_ensemble_lib():
    """The grid ensemble harness, yalla_amd/libyalla_ensemble_grid.so (include/yalla_ensemble_grid.h), every
    entry point typed.  Raises if it has not been built: there is no fallback."""
    return _load(GRID_ENSEMBLE_LIB, GRID_ENSEMBLE_ABI)


@functools.lru_cache(maxsize=None)  # (the same object on every call)
def gabriel_ensemble_lib():
    """The Gabriel ensemble harness, yalla_amd/libyalla_ensemble_gabriel.so (include/yalla_ensemble_gabriel.h),
    every entry point typed.  Raises if it has not been built: there is no fallback."""
    return _load(GABRIEL_ENSEMBLE_LIB, GABRIEL_ENSEMBLE_ABI)


@functools.lru_cache(maxsize=None)  # (the same object on every call)
def gabriel_lds_ensemble_lib():
    """The Gabriel ensemble harness whose take_steps can step from LDS, yalla_amd/libyalla_ensemble_gabriel_lds.so
    (include/yalla_ensemble_gabriel_lds.h), every entry point typed.  Raises if it has not been built: there is no
    fallback."""
    return _load(GABRIEL_LDS_ENSEMBLE_LIB, GABRIEL_LDS_ENSEMBLE_ABI)


@functools.lru_cache(maxsize=None)  # (the same object on every call)
def linked_ensemble_lib():
    """The linked ensemble harness, yalla_amd/libyalla_ensemble_links.so (include/yalla_ensemble_links.h), every
    entry point typed.  Raises if it has not been built: there is no fallback."""
    return _load(LINKED_ENSEMBLE_LIB, LINKED_ENSEMBLE_ABI)


@functools.lru_cache(maxsize=None)  # (the same object on every call)
def linked_grid_ensemble_lib():
    """The linked grid ensemble harness, yalla_amd/libyalla_ensemble_grid_links.so
    (include/yalla_ensemble_grid_links.h), every entry point typed.  Raises if it has not been built: there is no
    fallback."""
    return _load(LINKED_GRID_ENSEMBLE_LIB, LINKED_GRID_ENSEMBLE_ABI)


@functools.lru_cache(maxsize=None)  # (the same object on every call)
def sweep_ensemble_lib():
    """The sweep harness, yalla_amd/libyalla_ensemble_sweep.so (include/yalla_ensemble_sweep.h), every entry point
    typed.  Raises if it has not been built: there is no fallback."""
    return _load(SWEEP_ENSEMBLE_LIB, SWEEP_ENSEMBLE_ABI)
