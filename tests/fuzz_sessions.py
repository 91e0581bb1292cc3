#!/usr/bin/env python3
"""Session fuzz: bit parity, device engine vs CPU oracle, across settings changed BETWEEN steps (test
infrastructure; run on a GPU box: python tests/fuzz_sessions.py [sessions] [first_seed]).

tests/fuzz_parity.py sets every knob before the first step.  Here one Solution lives for 10 ... 24 steps and,
before a step, with probability 0.45 one mutation is applied: what Heun_solver and Grid_computer carry from one
step to the next (the captured hipGraph and its key, rhs_zeroed, the sorted copy of stage 1, the grid's remembered
visit order, the tail exchange areas) meets every public knob a model program may turn at any time.

  * mutations of BOTH libraries: dt, set_fixed() / set_fixed(p) / set_fixed_xy(p), sum_order, cube_size, h_n up or
    down through copy_to_host / copy_to_device (half of them back to a count the session had before: a graph
    captured for that count may still exist), renumber_now, a Gaussian nudge of all positions through the host
    mirror, a fresh old_v, gabriel_coefficient;
  * mutations of the DEVICE only (result-neutral by the engine's own claim; the oracle has no such knobs): graph,
    force_variant (+ coop_lanes), stage_v_max, tail_tiles, sorted_pipeline, tile_lanes, Gabriel's force_variant.

After EVERY step positions, old_v[:n] and (grid models) the four grid arrays must be bit-identical.  Second check,
independent of the oracle -- restart equivalence: at a drawn step the state (all n_max rows of h_X, h_n, old_v)
and the settings in force move into a FRESH Solution of the same library, which runs the rest of the session; its
final positions and old_v must equal the long-lived object's bit for bit.  That catches state surviving in the
solver object even where oracle and engine share a misconception.

draw(seed) is pure (numpy default_rng, no library call) and JSON-serialisable: a failing session is re-run from
its seed.  Parts of the draw are planted rather than left to chance (tests/test_sessions.py asserts the counts on
the slice the GPU test runs): quiet runs of >= 3 steps followed by a result-changing mutation while a graph must
exist, a sum_order flip 0 -> 1 between the first and the second step, a cell count that goes away for one step
and comes back while the graph captured for it is alive.

Models: every model of the harness whose functors use + - * / sqrt fma only and whose sums have a fixed order.
Left out: springs_links_grid (at its default threshold the link forces accumulate with atomics on the device, in no
fixed order; tests/native/test_links_sums.cu and tests/test_links_order_gpu.py hold both link paths, bit for bit
wherever the order is fixed or does not matter, and a model added to MODELS would change every drawn session), models with libm functors (sorting, branching, passive
growth: lock-step 1e-5 tests cover them), slab sessions (tests/fuzz_slab.py).

A session in which the ORACLE goes non-finite or (grid, Gabriel) comes within two cubes of the grid's edge is no
parity case: the oracle runs first, step by step, and the device is not started on such a session.

Oracle-only figures of this generator (seeds 7000-7199, the slice of the test suite; measured on the CPU):
skipped 0 of 200; restart equivalence 200 of 200; sessions whose final bits change when the mutations of one kind
are removed: sum_order flips (to a different value) 43 of 44, renumber_now 43 of 43, old_v 97 of 98.  The slice
holds 113 grid sessions (103 start with graph != 0).  By graph_trace() (the host's graph logic replayed over the
dict): 40 sessions with a result-changing mutation straight after three quiet steps while a graph is alive (19 of
them sum_order flips), 10 early flips on a capturing pipeline, 41 that must replay a graph, 17 in which a count
comes back after one step elsewhere while its graph is alive.  The oracle's part of a session takes about 0.2 s.
"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from yalla_amd.solution import Solution

GRID_MODELS = ["springs_grid", "clipped_grid", "relu_grid", "relu_po_grid", "relu_cell_grid",
               "clipped_push_grid"]   # (the last: a generic force -- the rhs_zeroed promise and the d_X1 path)
TILE_MODELS = ["springs_tile", "clipped_tile", "relu_po_tile"]
GABRIEL_MODELS = ["clipped_gabriel"]
MODELS = GRID_MODELS + TILE_MODELS + GABRIEL_MODELS

SLICE = range(7000, 7200)   # the sessions of tests/test_sessions.py and tests/test_sessions_gpu.py

BOTH_KINDS = ("dt", "fixed", "sum_order", "cube_size", "n", "renumber", "nudge", "old_v", "gabriel_coefficient")
DEVICE_KINDS = ("graph", "force_variant", "stage_v_max", "tail_tiles", "sorted_pipeline", "tile_lanes",
                "gabriel_variant")
RESULT_CHANGING = ("sum_order", "cube_size", "fixed", "dt")


def _variant(rng):
    """[force_variant, coop_lanes] as tests/fuzz_parity.py draws them"""
    variant, lanes = int(rng.choice([2, 2, 2, 1, 0])), int(rng.choice([0, 0, 0, 0, 4, 8, 16, 16]))
    if lanes:
        variant = 3
    if rng.random() < 0.33:
        variant, lanes = -1, 0
    return [variant, lanes]


def _tail(rng):
    tail = int(rng.integers(1, 21)) if rng.random() < 0.5 else 0
    return [tail, -1, 1 << 20][int(rng.integers(0, 3))]


def _mutation(rng, kind, st):
    """One op [kind, value...] of plain ints / floats; st = what draw() tracks (n, n_max, sum_order, earlier counts)"""
    n_max = st["n_max"]
    if kind == "dt":
        return ["dt", float(rng.choice([0.001, 0.002, 0.01]))]
    if kind == "fixed":
        return ["fixed", int(rng.integers(0, 3)), int(rng.integers(0, max(1, n_max // 2)))]   # (< any drawn n)
    if kind == "sum_order":
        return ["sum_order", int(rng.integers(0, 2))]
    if kind == "cube_size":
        return ["cube_size", float(rng.choice([1.0, 1.25, 1.5]))]
    if kind == "n":
        earlier = [m for m in st["counts"] if m != st["n"]]
        if earlier and rng.random() < 0.5:
            return ["n", int(earlier[rng.integers(len(earlier))])]
        return ["n", int(rng.integers(max(1, n_max // 2), n_max + 1))]
    if kind in ("nudge", "old_v"):
        return [kind, int(rng.integers(1 << 30))]
    if kind == "renumber":
        return ["renumber"]
    if kind == "gabriel_coefficient":
        return ["gabriel_coefficient", float(rng.choice([0.6, 0.8, 1.0]))]
    if kind == "graph":
        return ["graph", int(rng.choice([0, 1, -1]))]
    if kind == "force_variant":
        return ["force_variant"] + _variant(rng)
    if kind == "stage_v_max":
        return ["stage_v_max", int(rng.choice([0, 1 << 30]))]
    if kind == "tail_tiles":
        return ["tail_tiles", _tail(rng)]
    if kind == "sorted_pipeline":
        return ["sorted_pipeline", int(rng.integers(0, 3))]
    if kind == "tile_lanes":
        return ["tile_lanes", int(rng.choice([0, 1, 16, 64]))]
    if kind == "gabriel_variant":
        return ["gabriel_variant", int(rng.choice([-1, 0]))]
    raise ValueError(kind)


def kinds_of(model):
    """the mutation kinds a model offers"""
    if model in GRID_MODELS:
        kinds = ["dt", "fixed", "sum_order", "cube_size", "n", "nudge", "old_v",
                 "graph", "force_variant", "stage_v_max", "tail_tiles", "sorted_pipeline"]
        if model != "clipped_push_grid":   # (its generic force pushes cell 1: ids matter, the harness refuses)
            kinds.append("renumber")
        return kinds
    if model in TILE_MODELS:
        return ["dt", "fixed", "n", "nudge", "old_v", "tile_lanes"]
    return ["dt", "fixed", "cube_size", "n", "nudge", "old_v", "gabriel_coefficient", "gabriel_variant"]


def _track(st, op):
    if op[0] == "n":
        st["n"] = op[1]
        st["counts"].append(op[1])
    elif op[0] == "sum_order":
        st["sum_order"] = op[1]


def draw(seed):
    rng = np.random.default_rng(seed)
    model = MODELS[rng.integers(len(MODELS))]
    grid = model in GRID_MODELS
    n_max = int(rng.choice([70, 300, 1000, 3000, 9000]))
    if not grid:
        n_max = min(n_max, 1000)   # all pairs / a host-serial Gabriel graph on the CPU
    dist = float(rng.choice([0.5, 0.75, 1.2]))
    radius = (n_max / 0.64) ** (1 / 3) * dist / 2
    gs = 2 * (int(radius + 12) + 2)
    steps = int(rng.integers(10, 25))
    n = int(rng.integers(max(1, n_max // 2), n_max + 1))
    # the settings the session starts with: [kind, value...] like the mutations, applied after construction
    init = []
    if grid:
        init = [["sum_order", int(rng.random() < 0.34)], ["graph", int(rng.choice([0, 1, 1, -1]))],
                ["force_variant"] + _variant(rng), ["stage_v_max", int(rng.choice([0, 1 << 30]))],
                ["tail_tiles", _tail(rng)], ["sorted_pipeline", int(rng.choice([1, 1, 1, 0, 2]))]]
    elif model in TILE_MODELS:
        init = [["tile_lanes", int(rng.choice([0, 1, 16, 64]))]]
    else:
        init = [["gabriel_variant", int(rng.choice([-1, -1, 0]))]]
    kinds = kinds_of(model)
    # planted (grid sessions): 1 = a quiet run of >= 3 steps, then a result-changing mutation, with a graph asked
    # for; 2 = sum_order 0 -> 1 between the first and the second step with a graph asked for; 3 = the cell count
    # goes away after a quiet run, for ONE step (two would capture a graph for the other count and so drop the one
    # the quiet run left), and comes back while that graph is alive
    plant = int(rng.choice([0, 0, 0, 1, 1, 1, 1, 2, 3, 3])) if grid else 0
    if model == "clipped_push_grid":   # (a generic force: never the sorted pipeline, no captured step to plant for)
        plant = 0
    quiet_from = int(rng.integers(0, steps - 6))
    if plant:
        if init[1][1] == 0:
            init[1][1] = int(rng.choice([1, 1, -1]))
        if init[5][1] == 0:
            init[5][1] = 1
        if init[2][1] in (0, 1):   # (force_variant 0 has no sorted pipeline, hence no captured step)
            init[2][1:] = [2, 0]
    if plant == 2:
        init[0][1] = 0
        if rng.random() < 0.5:
            init[2][1:] = [2, 0]   # the bit-stream kernel: the only one with a tail to allocate
    st = dict(n=n, n_max=n_max, sum_order=init[0][1] if grid else 0, counts=[n])
    ops = []
    for k in range(steps):
        todo = []
        if plant == 1 and quiet_from <= k <= quiet_from + 3:
            if k == quiet_from + 3:
                kind = str(rng.choice(["sum_order", "sum_order", "sum_order", "cube_size", "fixed", "dt"]))
                todo.append(["sum_order", 1 - st["sum_order"]] if kind == "sum_order" else _mutation(rng, kind, st))
        elif plant == 2 and k <= 1:
            if k == 1:
                todo.append(["sum_order", 1])
        elif plant == 3 and quiet_from <= k <= quiet_from + 5:
            if k == quiet_from + 3:
                todo.append(["n", int(rng.integers(max(1, n_max // 2), n_max + 1))])
            if k == quiet_from + 4:
                todo.append(["n", st["counts"][-2]])
        elif k and rng.random() < 0.45:
            todo.append(_mutation(rng, str(kinds[rng.integers(len(kinds))]), st))
        for op in todo:
            _track(st, op)
        ops.append(todo)
    restart_at = int(rng.integers(1, steps))
    return dict(model=model, n_max=n_max, n=n, gs=gs, cs=1.0, dist=dist, seed=int(seed), init=init, ops=ops,
                restart_at=restart_at)


# ---- what a drawn session contains (from the dict alone) --------------------------------------------

def is_grid(c):
    return c["model"] in GRID_MODELS


def initial(c, kind, default=0):
    for op in c["init"]:
        if op[0] == kind:
            return op[1]
    return default


def count_kinds(cases):
    counts = {}
    for c in cases:
        for todo in c["ops"]:
            for op in todo:
                counts[op[0]] = counts.get(op[0], 0) + 1
    return counts


def walk(c):
    """(step, op, settings before the op) for every mutation; settings = the tracked values of every kind"""
    cur = {op[0]: op[1:] for op in c["init"]}
    for k, todo in enumerate(c["ops"]):
        for op in todo:
            yield k, op, dict(cur)
            if op[0] in DEVICE_KINDS or op[0] in ("sum_order", "cube_size", "dt", "gabriel_coefficient"):
                cur[op[0]] = op[1:]


def real_flips(c):
    """steps at which sum_order goes to a DIFFERENT value"""
    return [k for k, op, cur in walk(c) if op[0] == "sum_order" and op[1] != cur["sum_order"][0]]


def graph_trace(c):
    """Heun_solver::take_step's graph logic replayed over the drawn dict, one entry per step:
    {"event": "plain" | "capture" | "replay", "live": a graph exists when the step begins,
     "stale": the step's key equals the live graph's but not the step before's (the graph is NOT replayed: the grid
              remembers another build's visit order), "away": how many steps ran since that key was last stepped,
     "only_n": ... and those steps differed from it in the cell count alone}.
    A model of the host logic for the coverage conditions, not of the device: it takes ready_to_capture() for
    true (the plain step before allocated) and leaves the tail areas' generation out of the key."""
    out = []
    if not is_grid(c):
        return [{"event": "plain", "live": False, "stale": False} for _ in c["ops"]]
    cur = {op[0]: tuple(op[1:]) for op in c["init"]}
    cur.update(dt=(0.001,), cube_size=(1.0,), n=(c["n"],), fixed=(True, False, 0))
    graph_key = last_key = None
    history = []   # the keys of the steps so far (None: not on the sorted pipeline)
    for todo in c["ops"]:
        for op in todo:
            if op[0] == "fixed":   # set_fixed() / set_fixed(p) / set_fixed_xy(p): fix_com, fix_com_z (sticks), fix_point
                com, z, point = cur["fixed"]
                cur["fixed"] = [(True, z, point), (False, z, op[2]), (False, True, op[2])][op[1]]
            elif op[0] == "renumber":
                graph_key = last_key = None   # Heun_solver::renumber drops the graph
            elif op[0] in cur:
                cur[op[0]] = tuple(op[1:])
        eligible = c["model"] != "clipped_push_grid" and cur["sorted_pipeline"][0] != 0 and cur["force_variant"][0] != 0
        key = tuple(cur[k] for k in ("n", "dt", "cube_size", "fixed", "sum_order", "force_variant", "stage_v_max",
                                     "tail_tiles")) + (cur["sorted_pipeline"][0] == 2,)
        entry = {"event": "plain", "live": graph_key is not None, "stale": False}
        if not eligible:
            last_key = key = None
        elif cur["graph"][0] == 0 or last_key is None:
            last_key = key
        elif graph_key == key and key == last_key:
            entry["event"] = "replay"
        elif key == last_key:
            entry["event"] = "capture"
            graph_key = key
        else:
            if graph_key == key:
                since = history[::-1].index(key)
                entry.update(stale=True, away=since, only_n=all(
                    h is not None and h[1:] == key[1:] for h in history[len(history) - since:]))
            last_key = key
        history.append(key)
        out.append(entry)
    return out


def result_change_after_quiet(c):
    """[(step, kind)]: a result-changing mutation while a graph is alive that the step before captured or
    replayed (after >= 3 quiet steps with graph != 0 on a model and pipeline that capture: graph_trace)"""
    out = []
    trace = graph_trace(c)
    for k, op, cur in walk(c):
        if k < 3 or c["ops"][k - 1] or c["ops"][k - 2] or c["ops"][k - 3] or op[0] not in RESULT_CHANGING:
            continue
        if trace[k - 1]["event"] == "plain" or not trace[k]["live"]:
            continue
        if op[0] == "sum_order" and op[1] == cur["sum_order"][0]:
            continue
        out.append((k, op[0]))
    return out


def early_flip(c):
    """sum_order 0 -> 1 between the first and the second step, the second being the step a graph would have been
    captured at had the key not changed (graph != 0 on a model and pipeline that capture)"""
    if not is_grid(c) or c["model"] == "clipped_push_grid" or initial(c, "sum_order") != 0:
        return False
    return initial(c, "graph") != 0 and initial(c, "sorted_pipeline") != 0 and initial(c, "force_variant") != 0 and \
        c["ops"][1] == [["sum_order", 1]]


def count_comes_back(c):
    """steps at which a cell count returns after exactly ONE step at another count while the graph captured for
    it is alive: the step that must be a plain one (the grid remembers the other count's build)"""
    return [k for k, e in enumerate(graph_trace(c)) if e["stale"] and e["away"] == 1 and e["only_n"]]


def stale_order_steps(c):
    """every step whose key equals a live graph's after steps with other keys (count_comes_back and more)"""
    return [k for k, e in enumerate(graph_trace(c)) if e["stale"]]


def must_replay(c):
    """>= 4 identical steps (no mutation before the last three) with graph = 1 on the sorted pipeline without
    generic forces: the second of them captures, the third and fourth are replays"""
    if not is_grid(c) or c["model"] == "clipped_push_grid":
        return False
    cur = {op[0]: op[1:] for op in c["init"]}
    for k, todo in enumerate(c["ops"]):
        for op in todo:
            if op[0] in cur:
                cur[op[0]] = op[1:]
        if cur["graph"][0] == 1 and cur["sorted_pipeline"][0] != 0 and cur["force_variant"][0] != 0 and \
                k + 3 < len(c["ops"]) and not (c["ops"][k + 1] or c["ops"][k + 2] or c["ops"][k + 3]):
            return True
    return False


# ---- running a session --------------------------------------------------------------------------------

def _setting(s, device, op):
    """a setting of the solver: both libraries, or the device alone"""
    kind = op[0]
    if kind == "sum_order":
        s.set_param("sum_order", op[1])
    elif kind == "cube_size":
        s.cube_size = op[1]
    elif kind == "gabriel_coefficient":
        s.set_param("gabriel_coefficient", op[1])
    elif kind == "fixed":
        [lambda: s.set_fixed(), lambda: s.set_fixed(op[2]), lambda: s.set_fixed_xy(op[2])][op[1]]()
    elif not device:
        return
    elif kind == "force_variant":
        s.set_param("force_variant", op[1])
        s.set_param("coop_lanes", op[2])
    elif kind == "gabriel_variant":
        s.set_param("force_variant", op[1])
    else:   # graph, stage_v_max, tail_tiles, sorted_pipeline, tile_lanes
        s.set_param(kind, op[1])


def _state_op(s, op):
    """a change of the state (both libraries)"""
    if op[0] == "n":
        s.copy_to_host(); s.h_n = op[1]; s.copy_to_device()
    elif op[0] == "renumber":
        s.set_param("renumber_now", 1)
    elif op[0] == "nudge":
        s.copy_to_host()
        s.h_X[:, :3] += np.random.default_rng(op[1]).normal(0, 0.05, (s.n_max, 3)).astype(np.float32)
        s.copy_to_device()
    elif op[0] == "old_v":
        s.set_old_v(np.random.default_rng(op[1]).normal(0, 0.5, (s.n_max, 3)).astype(np.float32))


def snapshot(s, grid):
    X = s.positions()
    n = len(X)
    out = {"X": X, "old_v": s.old_v()[:n]}
    if grid:
        for name, a in zip(("cube_id", "point_id", "cube_start", "cube_end"), s.grid()):
            out[name] = a[:n] if name in ("cube_id", "point_id") else a
    return out


def first_difference(a, b):
    """the name of the first array of two snapshots that differs in any bit, or None"""
    for name in a:
        x, y = a[name], b[name]
        if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            return name
    return None


def left_the_grid(c, X):
    if not np.isfinite(X).all():
        return True
    if c["model"] in TILE_MODELS:
        return False   # no grid to leave
    # within two cubes of the edge at the smallest cube size of the session (1.0: cube_size only ever grows)
    return bool(np.abs(X[:, :3]).max() >= c["gs"] // 2 - 2)


def play(lib, c, device, first=0, resume=None, save_at=None, drop=(), every_step=True):
    """Steps first ... end of session c on lib.  resume = (state, settings) a play(save_at=first) returned: the
    session goes on in a fresh Solution.  drop = mutation kinds left out (sensitivity runs).  Returns
    (snapshots or None if the session left its grid, saved, graph launches); snapshots = one per step, or the
    final one alone."""
    grid = c["model"] not in TILE_MODELS
    with Solution(c["model"], c["n_max"], c["gs"], c["cs"], lib=lib) as s:
        if not device:
            assert s.set_reduce_order(1) == 0
        if resume is None:
            settings = {"dt": 0.001, "ops": [list(op) for op in c["init"]]}
            for op in settings["ops"]:
                _setting(s, device, op)
            s.h_n = c["n_max"]
            s.random_sphere(c["dist"], c["seed"])   # over ALL n_max rows: those above n are the reserve
            s.copy_to_host()
            s.h_n = c["n"]
            s.copy_to_device()
        else:
            state, settings = copy.deepcopy(resume)
            for op in settings["ops"]:
                _setting(s, device, op)
            s.h_X[:] = state["h_X"]
            s.h_n = state["h_n"]
            s.copy_to_device()
            s.set_old_v(state["old_v"])
        snaps, saved = [], None
        for k in range(first, len(c["ops"])):
            if k == save_at:
                s.copy_to_host()
                saved = ({"h_X": s.h_X.copy(), "h_n": s.h_n, "old_v": s.old_v()}, copy.deepcopy(settings))
            for op in c["ops"][k]:
                if op[0] in drop:
                    continue
                if op[0] == "dt":
                    settings["dt"] = op[1]
                elif op[0] in ("n", "renumber", "nudge", "old_v"):
                    _state_op(s, op)
                else:
                    settings["ops"].append(list(op))   # (every setting since the start, in order: set_fixed_xy sticks)
                    _setting(s, device, op)
            s.take_step(settings["dt"], 1)
            if every_step or k == len(c["ops"]) - 1:
                snap = snapshot(s, grid)
                if not device and left_the_grid(c, snap["X"]):
                    return None, None, 0
                snaps.append(snap)
            elif not device and left_the_grid(c, s.positions()):
                return None, None, 0
        return snaps, saved, (s.graph_launches() if device else 0)


def run_oracle(oracle, c):
    """the oracle's part of a session: {"snaps", "saved", "restart_equal"} or None (no parity case)"""
    snaps, saved, _ = play(oracle, c, False, save_at=c["restart_at"])
    if snaps is None:
        return None
    rest, _, _ = play(oracle, c, False, first=c["restart_at"], resume=saved, every_step=False)
    equal = rest is not None and first_difference(
        {k: snaps[-1][k] for k in ("X", "old_v")}, {k: rest[-1][k] for k in ("X", "old_v")}) is None
    return {"snaps": snaps, "saved": saved, "restart_equal": equal}


def run_device(device, c, oracle_snaps):
    """the device's part: every step against the oracle's, then the restart.  Returns a dict for the log."""
    snaps, saved, launches = play(device, c, True, save_at=c["restart_at"])
    out = {"bit_exact": True, "restart_equal": True, "graph_launches": int(launches)}
    for k, (a, b) in enumerate(zip(oracle_snaps, snaps)):
        name = first_difference(a, b)
        if name:
            out.update(bit_exact=False, first_diff=[k, name])
            break
    rest, _, _ = play(device, c, True, first=c["restart_at"], resume=saved, every_step=False)
    name = first_difference({k: snaps[-1][k] for k in ("X", "old_v")}, {k: rest[-1][k] for k in ("X", "old_v")})
    if name:
        out.update(restart_equal=False, restart_diff=name)
    return out


def summary(c):
    """the short description of a session for a log line (draw(seed) gives the rest)"""
    return {"seed": c["seed"], "model": c["model"], "n_max": c["n_max"], "n": c["n"], "steps": len(c["ops"]),
            "init": c["init"], "mutations": sum(len(t) for t in c["ops"]), "restart_at": c["restart_at"],
            "must_replay": must_replay(c)}


if __name__ == "__main__":
    from yalla_amd import _ffi
    from conftest import build_oracle
    sessions = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    first_seed = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    oracle, device = _ffi.bind(build_oracle()), _ffi.device_lib()
    log = open(os.environ["FUZZ_LOG"], "w") if os.environ.get("FUZZ_LOG") else None   # one JSON line per session
    bad = skipped = replays = 0
    for seed in range(first_seed, first_seed + sessions):   # one after another; a failed session is not retried
        c = draw(seed)
        if os.environ.get("FUZZ_VERBOSE"):
            print(json.dumps(c), flush=True)
        line = summary(c)
        o = run_oracle(oracle, c)
        if o is None:
            skipped += 1
            line["skipped"] = "left the grid on the oracle"
        else:
            if log:   # (before the device starts: should the process end there, this names the session)
                log.write(json.dumps(dict(line, device="starting")) + "\n")
                log.flush()
            line.update(run_device(device, c, o["snaps"]))
            line["oracle_restart_equal"] = o["restart_equal"]
            replays += line["graph_launches"] if line["graph_launches"] > 0 else 0
            if not (line["bit_exact"] and line["restart_equal"] and o["restart_equal"]) or \
                    (line["must_replay"] and line["graph_launches"] <= 0):
                bad += 1
                print("MISMATCH", json.dumps(line), flush=True)
        if log:
            log.write(json.dumps(line) + "\n")
            log.flush()
    total = {"sessions": sessions, "first_seed": first_seed, "skipped": skipped, "failed": bad,
             "bit_exact_and_restart_equal": sessions - skipped - bad, "graph_launches": replays}
    print(json.dumps(total))
    if log:
        log.write(json.dumps(total) + "\n")
        log.close()
    sys.exit(1 if bad else 0)
