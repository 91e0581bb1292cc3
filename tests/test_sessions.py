"""tests/fuzz_sessions.py without a GPU: the generator (determinism, what the fixed slice of the GPU test
contains) and the oracle's side of the two checks (skip cap, restart equivalence, sensitivity).  Every number
here is a condition on the inputs, chosen against the oracle-only figures in fuzz_sessions' docstring."""
import json

import pytest

import fuzz_sessions as fs

FINAL = ("X", "old_v")


def final_bits_differ(a, b):
    return fs.first_difference({k: a[k] for k in FINAL}, {k: b[k] for k in FINAL}) is not None


@pytest.fixture(scope="module")
def cases():
    return [fs.draw(seed) for seed in fs.SLICE]


@pytest.fixture(scope="module")
def oracle_runs(oracle, cases):
    """seed -> run_oracle()'s result without the per-step snapshots but the last (None: no parity case)"""
    runs = {}
    for c in cases:
        o = fs.run_oracle(oracle, c)
        runs[c["seed"]] = o and {"final": o["snaps"][-1], "restart_equal": o["restart_equal"]}
    return runs


def test_draw_is_deterministic_and_survives_json(cases):
    assert len(cases) >= 200
    for c in cases[:60]:
        assert fs.draw(c["seed"]) == c
        assert json.loads(json.dumps(c)) == c
        assert 10 <= len(c["ops"]) <= 24 and 1 <= c["restart_at"] < len(c["ops"])
        assert c["n_max"] // 2 <= c["n"] <= c["n_max"] and not c["ops"][0]
    assert fs.draw(7000) != fs.draw(7001)


def test_slice_contains_what_the_gpu_test_is_for(cases):
    counts = fs.count_kinds(cases)
    for kind in fs.BOTH_KINDS + fs.DEVICE_KINDS:
        assert counts.get(kind, 0) >= 10, (kind, counts)
    grid = [c for c in cases if fs.is_grid(c)]
    with_graph = [c for c in grid if fs.initial(c, "graph") != 0]
    assert 2 * len(with_graph) >= len(grid), (len(with_graph), len(grid))
    # a graph must exist (>= 3 steps without any mutation, graph != 0) when a mutation changes the result
    after_quiet = [c["seed"] for c in cases if fs.result_change_after_quiet(c)]
    flips_after_quiet = [c["seed"] for c in cases
                         if any(kind == "sum_order" for _, kind in fs.result_change_after_quiet(c))]
    assert len(after_quiet) >= 20 and len(flips_after_quiet) >= 5, (len(after_quiet), len(flips_after_quiet))
    # ... and the first step that needs a tail exchange area is the one a graph would be captured at
    early = [c["seed"] for c in cases if fs.early_flip(c)]
    assert len(early) >= 5, early
    # ... and some sessions say that a graph must have been replayed (the GPU test reads the engine's counter)
    assert sum(fs.must_replay(c) for c in cases) >= 10
    # a count that comes back after exactly one step at another count while the graph captured for it is alive
    # (two steps away would capture a graph for the other count and drop this one): the step straight after the
    # return must be a plain one, the grid remembers the other count's build
    back = [c["seed"] for c in cases if fs.count_comes_back(c)]
    assert len(back) >= 10, back
    assert 7189 in back   # (kept by name in tests/test_sessions_gpu.py)


def test_at_most_one_in_twenty_sessions_leaves_its_grid(cases, oracle_runs):
    skipped = [seed for seed, run in oracle_runs.items() if run is None]
    assert 20 * len(skipped) <= len(cases), skipped


def test_oracle_restart_equivalence(oracle_runs):
    """a fresh Solution given state and settings at a drawn step ends the session on the same bits"""
    ran = {seed: run for seed, run in oracle_runs.items() if run is not None}
    assert len(ran) >= 40
    unequal = [seed for seed, run in ran.items() if not run["restart_equal"]]
    assert not unequal, unequal


@pytest.mark.parametrize("kind,share", [("sum_order", 1 / 3), ("renumber", 0.9), ("old_v", 0.9)])
def test_removing_a_kind_of_mutation_changes_the_final_bits(oracle, cases, oracle_runs, kind, share):
    """The parity check is not vacuous: an engine that ignored these mutations would be seen.  (sum_order: the
    flips to a DIFFERENT value only; a session may flip back before it ends, or hold no cell with neighbours in
    another plane.)"""
    def has(c):
        return fs.real_flips(c) if kind == "sum_order" else any(op[0] == kind for todo in c["ops"] for op in todo)
    chosen = [c for c in cases if oracle_runs[c["seed"]] is not None and has(c)]
    assert len(chosen) >= 20, len(chosen)
    differ, left = 0, []
    for c in chosen:
        snaps, _, _ = fs.play(oracle, c, False, drop=(kind,), every_step=False)
        if snaps is None:
            left.append(c["seed"])   # (without the mutation the session leaves its grid: no final bits to compare)
        else:
            differ += final_bits_differ(oracle_runs[c["seed"]]["final"], snaps[-1])
    assert differ >= share * len(chosen), (kind, differ, len(chosen), "left the grid:", left)
