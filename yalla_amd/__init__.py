"""yalla_amd -- MI355X-native step path for ya||a spheroid-cell models.

The engine is C++/HIP: include/*.cuh (header API, functor-templated kernels),
yalla_amd/csrc/core.hip -> libyalla_hip.so (C ABI, include/yalla_hip.h) and
yalla_amd/csrc/models.hip -> libyalla_models.so (named models, C ABI
include/yalla_models.h), yalla_amd/csrc/ensemble.hip -> libyalla_ensemble.so
(many small all-pairs systems stepped together, C ABI include/yalla_ensemble.h) and yalla_amd/csrc/ensemble_grid.hip ->
libyalla_ensemble_grid.so (the same for grid systems, C ABI include/yalla_ensemble_grid.h) and
yalla_amd/csrc/ensemble_gabriel.hip -> libyalla_ensemble_gabriel.so (the same for Gabriel systems, C ABI
include/yalla_ensemble_gabriel.h; ensemble_gabriel_lds.hip -> libyalla_ensemble_gabriel_lds.so the same with whole steps
from LDS, C ABI include/yalla_ensemble_gabriel_lds.h) and yalla_amd/csrc/ensemble_links.hip -> libyalla_ensemble_links.so (all-pairs systems
with ordered link forces, C ABI include/yalla_ensemble_links.h; what the four ensemble sources share is
yalla_amd/csrc/ensemble_harness.h).  This package is the thin Python host side used by
tests/ and bench.py: a ctypes binding and a mirror of the Solution facade.
"""
from ._ffi import device_lib, bind, DEVICE_LIB, CORE_LIB  # noqa: F401
from .solution import Solution, YallaError, models  # noqa: F401
from .ensemble import Ensemble, GabrielEnsemble, GabrielLdsEnsemble, GridEnsemble, LinkedEnsemble  # noqa: F401
from .ensemble import SweepEnsemble  # noqa: F401
