"""Bit parity across settings changed between steps (tests/fuzz_sessions.py): a fixed slice of the generator,
every step against the oracle and a restart on the device, plus directed regression tests for what a captured
step (Heun_solver::graph_steps) bakes in -- the summation order and the tail of grid_force_bits (whose exchange
area must not be allocated inside a stream capture), and the grid's remembered visit order when a cell count
goes away and comes back.  Run under one time limit; SESSION_LOG names a file that gets each session's line
BEFORE its device part starts."""
import json
import os

import numpy as np
import pytest

import fuzz_sessions as fs
from yalla_amd.solution import Solution

pytestmark = pytest.mark.gpu

# sessions kept by name: (seed, the state that goes stale in them)
REGRESSIONS = [
    # the cell count leaves for one step and returns while the graph captured for it is alive: the graph holds the
    # visit order of a build of ITS cells (n_prev, d_prev_pid), the grid remembers the other count's build
    (7189, "the grid's remembered visit order baked into a captured step"),
]


def test_session_slice_bit_exact(oracle, device, tmp_path):
    cases = [fs.draw(seed) for seed in sorted(set(fs.SLICE) | {seed for seed, _ in REGRESSIONS})]
    assert len(cases) >= 200
    for seed, _ in REGRESSIONS:
        assert fs.stale_order_steps(fs.draw(seed)), seed   # (the generator still draws what the name says)
    failed, skipped = [], []
    with open(os.environ.get("SESSION_LOG") or tmp_path / "sessions.jsonl", "w") as log:
        for c in cases:
            o = fs.run_oracle(oracle, c)
            if o is None:
                skipped.append(c["seed"])
                continue
            assert o["restart_equal"], c["seed"]
            log.write(json.dumps(dict(fs.summary(c), device="starting")) + "\n")
            log.flush()
            line = dict(fs.summary(c), **fs.run_device(device, c, o["snaps"]))
            log.write(json.dumps(line) + "\n")
            if not (line["bit_exact"] and line["restart_equal"]):
                failed.append(line)
            # graph replay really happened where the session's description says it must
            elif line["must_replay"] and line["graph_launches"] <= 0:
                failed.append(dict(line, no_graph_launch=True))
    assert not failed, "%d sessions, first: %s\n%s" % (
        len(failed), json.dumps(failed[0]), json.dumps(fs.draw(failed[0]["seed"])))
    assert 20 * len(skipped) <= len(cases), skipped


_oracle_steps = {}


def directed(lib, n, gs, script, setup=()):
    """springs_grid, random_sphere(0.5): script = [("step", count) | (set_param name, value) | ("n", count)];
    a snapshot after every step"""
    snaps = []
    with Solution("springs_grid", n, gs, 1.0, lib=lib) as s:
        if lib.ya_models_is_device() == 0:
            s.set_reduce_order(1)
        for name, value in setup:
            s.set_param(name, value)
        s.random_sphere(0.5, 9)
        for what, value in script:
            if what == "step":
                for _ in range(value):
                    s.take_step(0.001, 1)
                    snaps.append(fs.snapshot(s, True))
            elif what == "n":
                s.copy_to_host(); s.h_n = value; s.copy_to_device()
            else:
                s.set_param(what, value)
        return snaps, s.graph_launches()


def against_oracle(oracle, device, n, gs, name, script, device_setup):
    both = [(what, value) for what, value in script if what != "tail_tiles"]   # (the oracle has no such knob)
    if (n, name) not in _oracle_steps:
        _oracle_steps[n, name] = directed(oracle, n, gs, both)[0]
    snaps, launches = directed(device, n, gs, script, device_setup)
    for k, (a, b) in enumerate(zip(_oracle_steps[n, name], snaps)):
        assert fs.first_difference(a, b) is None, (name, device_setup, "step", k, fs.first_difference(a, b))
    assert len(snaps) == len(_oracle_steps[n, name])
    return launches


SCRIPTS = {
    # a graph exists when the order changes: the step after the flip was the first to differ
    "late": [("step", 5), ("sum_order", 1), ("step", 3), ("sum_order", 0), ("step", 3)],
    # the second step, the one a graph is captured at, is the first that needs a tail exchange area
    "early": [("step", 1), ("sum_order", 1), ("step", 4), ("sum_order", 0), ("step", 3)],
    "tail": [("sum_order", 1), ("tail_tiles", 0), ("step", 1), ("tail_tiles", 5), ("step", 4)],
}


@pytest.mark.parametrize("name", ["late", "early", "tail"])
@pytest.mark.parametrize("variant", [2, -1])
@pytest.mark.parametrize("graph", [1, -1])
def test_graph_follows_sum_order_and_tail(oracle, device, graph, variant, name):
    """20 000 cells (below YA_GRAPH_MAX_CELLS): with the bit-stream kernel (2: the only one with a tail) and with
    the engine's choice (-1: grid_force_coop at this size, which has no tail -- the "tail" script is a control
    there: the knob must change nothing)"""
    launches = against_oracle(oracle, device, 20000, 50, name, SCRIPTS[name],
                              [("graph", graph), ("force_variant", variant)])
    assert launches > 0


@pytest.mark.parametrize("name", ["late", "early", "tail"])
def test_graph_follows_sum_order_where_every_tile_is_halves(oracle, device, name):
    """100 000 cells, everything the engine's choice: the bit-stream kernel with every tile as two halves under
    sum_order 1 -- the one default configuration that allocates a tail exchange area ("tail": none, then 5 tiles)"""
    assert against_oracle(oracle, device, 100000, 64, name, SCRIPTS[name], [("graph", -1)]) > 0


@pytest.mark.parametrize("counts", [(6000, 4000), (4000, 6000)])
@pytest.mark.parametrize("graph", [1, -1])
def test_graph_for_a_cell_count_that_comes_back(oracle, device, graph, counts):
    """A graph bakes in the visit order the grid remembered: that of a build of the SAME cells.  After a step with
    another count it must not be replayed straight away (cells would be binned twice, others not at all).  ONE
    step at the other count: a second one would capture a graph for that count and drop the first, and the step
    after the return would be a plain one whatever the engine does."""
    first, other = counts
    script = [("n", first), ("step", 4), ("n", other), ("step", 1), ("n", first), ("step", 4)]
    assert against_oracle(oracle, device, 6000, 40, "counts %d %d" % counts, script, [("graph", graph)]) > 0
