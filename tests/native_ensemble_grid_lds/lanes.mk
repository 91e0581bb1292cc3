# Ensemble<Pt, Grid_solver>::lds_step_lanes (include/ensemble_grid.cuh), as a model program uses the header;
# tests/test_ensemble_grid_lds_lanes_native.py runs it on the GPU.  (make -f lanes.mk; beside this directory's Makefile.)
HIPCC ?= /opt/rocm/bin/hipcc
FLAGS = -x hip --offload-arch=gfx950 -std=c++17 -O2 -ffp-contract=off -fno-slp-vectorize -I../../include
PROGRAMS = test_grid_lds_lanes

all: $(PROGRAMS)

%: %.cu ../native_ensemble/support.cuh $(wildcard ../../include/*.cuh) ../../include/yalla_hip.h
	$(HIPCC) $(FLAGS) $< -L../../yalla_amd -lyalla_hip -Wl,-rpath,'$$ORIGIN/../../yalla_amd' -o $@

clean:
	rm -f $(PROGRAMS)
