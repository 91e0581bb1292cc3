"""Several lanes per cell inside the grid ensemble's launches that step from LDS, through the layers that need no GPU:
both grid harnesses know "lds_step_lanes" and the getter "lds_step_lanes_used" (and say so on a null handle, where
nothing can be touched), the Gabriel harness does not; the exported functions are the ones they were (the getter is a
name of set_param that returns the value); the headers document the name and the getter; the Python restatement of
the term buffer's LDS rule (tests/ensemble_grid_lds_lanes_support.py) agrees with what the headers' comments quote and names the n_max either
side of every point where another term of the rule starts to decide, which tests/test_ensemble_grid_lds_lanes_gpu.py
runs."""
import os

import ensemble_grid_lds_lanes_support as ls
from ensemble_support import LDS, STATIC_LDS, lds_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_both_grid_harnesses_know_the_name_on_a_null_handle():
    from yalla_amd import _ffi
    assert _ffi.grid_ensemble_lib().ya_gens_set_param(None, b"lds_step_lanes", 1.0) == -3
    assert _ffi.linked_grid_ensemble_lib().ya_glens_set_param(None, b"lds_step_lanes", 1.0) == -3
    assert _ffi.grid_ensemble_lib().ya_gens_set_param(None, b"lds_step_lanes_used", 0.0) == -3
    assert _ffi.linked_grid_ensemble_lib().ya_glens_set_param(None, b"lds_step_lanes_used", 0.0) == -3
    for name in (b"lds_step_lane", b"lds_step_lanes_use", b"whole_step_lanes"):
        assert _ffi.grid_ensemble_lib().ya_gens_set_param(None, name, 1.0) == -2, name
        assert _ffi.linked_grid_ensemble_lib().ya_glens_set_param(None, name, 1.0) == -2, name


def test_the_gabriel_harness_does_not():
    from yalla_amd import _ffi
    assert _ffi.gabriel_ensemble_lib().ya_gabens_set_param(None, b"lds_step_lanes", 1.0) == -2
    assert _ffi.gabriel_ensemble_lib().ya_gabens_set_param(None, b"lds_step_lanes_used", 0.0) == -2
    gabriel = text("yalla_amd", "csrc", "ensemble_gabriel.hip") + text("include", "yalla_ensemble_gabriel.h")
    assert "lds_step_lanes" not in gabriel


class StandIn:
    """set_param of a harness that reports 16 lanes; everything else GridEnsemble's property does not need."""

    def __init__(self, answer):
        self.answer, self.calls = answer, []

    def ya_gens_set_param(self, handle, name, value):
        self.calls.append((name, value))
        return self.answer


def test_the_getter_travels_through_set_param_and_python_reads_it():
    from yalla_amd.ensemble import GabrielEnsemble, GridEnsemble, LinkedGridEnsemble, YallaError
    ens = GridEnsemble.__new__(GridEnsemble)
    ens.lib, ens._h = StandIn(16), 1
    assert ens.lds_step_lanes_used == 16 and ens.lib.calls == [(b"lds_step_lanes_used", 0.0)]
    ens.lib = StandIn(-3)
    try:
        ens.lds_step_lanes_used
        raise AssertionError("a harness error is an error")
    except YallaError:
        pass
    ens._h = None  # (nothing to destroy)
    assert isinstance(GridEnsemble.lds_step_lanes_used, property)
    assert LinkedGridEnsemble.lds_step_lanes_used is GridEnsemble.lds_step_lanes_used
    assert GabrielEnsemble.lds_step_lanes_used is not GridEnsemble.lds_step_lanes_used


def test_both_headers_document_the_name_and_the_getter():
    for header, prefix in (("yalla_ensemble_grid.h", "ya_gens_"), ("yalla_ensemble_grid_links.h", "ya_glens_")):
        h = text("include", header)
        comment = h[:h.index(f"int {prefix}set_param(")].rsplit("/*", 1)[1]
        assert '"lds_step_lanes"' in comment and '"lds_step_lanes_used"' in comment and "getter" in comment.lower(), header
        assert "0 before" in comment and "1 after the" in comment and "fallback" in comment, header
        assert f"{prefix}lds_step_lanes_used" not in h, "no new exported function"
        assert "Not here: several lanes" not in h and "several lanes per\n * cell" not in h
    for harness in ("ensemble_grid.hip", "ensemble_grid_links.hip"):
        assert "cells.lds_step_lanes = 1;" in text("yalla_amd", "csrc", harness), "the harness keeps one lane as its default"
    engine = text("include", "ensemble_grid.cuh")
    for piece in ("int lds_step_lanes = 0;", "int lds_step_lanes_used = 0;", "lds_layout<Pt, true, LINKED>(n_max, links.slots_per_replica, LANES)",
                  "const int tile = layout.tile;", "constexpr int grid_lds_lanes_for(",
                  "void grid_lds_walk_coop(", "int LANES = 1>\n__global__ __launch_bounds__(UPDATE_BLOCK) void grid_lds_steps(",
                  "int LANES = 1>\n__global__ __launch_bounds__(UPDATE_BLOCK) void grid_lds_steps_linked("):
        assert piece in engine, piece
    assert "Not here: several lanes per cell" not in engine


def test_the_restated_rule_agrees_with_what_the_comments_quote():
    """include/yalla_ensemble_grid.h: "a 7-float point at n_max = 1024 with 4 lanes, an 8-float point there with any";
    include/ensemble.cuh (ya::ens::lds_layout): "an 8-float point's 1024 rows and keys leave 896 bytes; a 7-float point's leave 18320: room for
    16 and 64 lanes, none for 4"; the issue of the rule: tile of candidates, 32 KiB budget, minimum 16."""
    assert "a 7-float\n * point at n_max = 1024 with 4 lanes, an 8-float point there with any" in text(
        "include", "yalla_ensemble_grid.h")
    assert "a 7-float point's leave 18320: room for 16 and 64 lanes, none for 4" in text("include", "ensemble.cuh")
    assert LDS - STATIC_LDS - lds_layout(8, 1024, True).terms == 896
    assert LDS - STATIC_LDS - lds_layout(7, 1024, True).terms == 18320
    assert [lds_layout(8, 1024, True, lanes=lanes).bytes for lanes in ls.LANES] == [0, 0, 0]
    assert lds_layout(7, 1024, True, lanes=4).bytes == 0
    assert lds_layout(7, 1024, True, lanes=16).tile == 24 and lds_layout(7, 1024, True, lanes=64).tile == 104
    for n_floats in (3, 4, 5):
        assert all(lds_layout(n_floats, 1024, True, lanes=lanes).bytes > 0 for lanes in ls.LANES)
    # a tile is a multiple of 4 candidates, 16 at the least, 256 at the most, within the budget unless that is the 16
    for n_floats in (3, 4, 5, 7, 8):
        for lanes in ls.LANES:
            per_candidate = (256 // lanes) * (n_floats + 4) * 4
            for n_max in range(1, 1025):
                layout = lds_layout(n_floats, n_max, True, lanes=lanes)
                tile, total = layout.tile, layout.bytes
                if tile == 0:
                    assert total == 0 and lds_layout(n_floats, n_max, True).terms + STATIC_LDS + 16 * per_candidate > LDS
                    continue
                assert tile % 4 == 0 and min(16, -(-n_max // 4) * 4) <= tile <= 256
                assert lds_layout(n_floats, n_max, True).terms % 16 == 0
                assert tile == 16 or tile * per_candidate <= 32 * 1024
                assert total == lds_layout(n_floats, n_max, True).terms + tile * per_candidate and total + STATIC_LDS <= LDS
    # the engine's choice for stateless functors: 16 lanes up to 32 cells, 4 up to 64, else 1 (the measured table)
    assert [ls.lanes_for(n) for n in (1, 4, 5, 16, 17, 32, 33, 64, 65, 1024)] == [16, 16, 16, 16, 16, 16, 4, 4, 1, 1]
    engine = text("include", "ensemble_grid.cuh")
    assert "if (n_max <= 32) return 16;\n    if (n_max <= 64) return 4;\n    return 1;" in engine
    # with links, the list lies in between: two slots per cell at 1024 rows of 3 floats cost 4100 + 16384 bytes
    assert lds_layout(3, 1024, True, 2048).terms - lds_layout(3, 1024, True).terms == 20496
    assert lds_layout(8, 1024, True, 0, 64).bytes == 0  # (no room for the list itself)


# The n_max either side of every point where another term of the rule starts to decide (0 = n_max, 1 = the longest
# tile, 2 = the budget, 3 = the room, -1 = no room: one lane), for any of 4, 16, 64 lanes.
RULE_POINTS = {
    3: [16, 17, 72, 73, 256, 257],
    4: [16, 17, 64, 65, 256, 257],
    5: [16, 17, 56, 57, 224, 225],
    7: [16, 17, 44, 45, 184, 185, 808, 809, 910, 911, 921, 922],
    8: [16, 17, 40, 41, 168, 169, 679, 680, 800, 801, 810, 811, 942, 943, 1008, 1009],
}
# the same for linked launches with two slots per cell (what the GPU test's 4- and 8-float models run)
LINKED_RULE_POINTS = {
    4: [16, 17, 64, 65, 256, 257],
    8: [8, 9, 40, 41, 168, 169, 594, 595, 699, 700, 709, 710, 824, 825, 882, 883, 901, 902],
}


def test_the_points_where_another_term_of_the_rule_starts_to_decide():
    for n_floats, points in RULE_POINTS.items():
        assert ls.rule_edges(n_floats) == points, n_floats
    for n_floats, points in LINKED_RULE_POINTS.items():
        assert ls.links_rule_edges(n_floats, lambda n_max: 2 * n_max) == points, n_floats
    # what they are, for the 8-float point: the fallback starts at 680 (4 lanes), 943 (16), 1009 (64)
    assert [(ls.coop_binding(8, n, 4), ls.coop_binding(8, n + 1, 4)) for n in (16, 679)] == [(0, 2), (2, -1)]
    assert [(ls.coop_binding(8, n, 16), ls.coop_binding(8, n + 1, 16)) for n in (40, 810, 942)] == [(0, 2), (2, 3), (3, -1)]
    assert [(ls.coop_binding(8, n, 64), ls.coop_binding(8, n + 1, 64)) for n in (168, 800, 1008)] == [(0, 2), (2, 3), (3, -1)]
    assert lds_layout(8, 942, True, lanes=16).tile == 16 and lds_layout(8, 1008, True, lanes=64).tile == 16
    # for three floats only n_max, the budget and the longest tile ever decide
    assert {ls.coop_binding(3, n, lanes) for n in range(1, 1025) for lanes in ls.LANES} == {0, 1, 2}
