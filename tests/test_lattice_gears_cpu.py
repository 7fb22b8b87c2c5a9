"""The lattice search with reverse moves and gear changes without a GPU: the restated rule (tests/lattice_gears_ref.py)
against hand values and against the consequences of the rule, the cases the device tests run (tests/lattice_gears_cases.py),
every host-side argument check of the C entries, the Python checks, and that header, binding, library and build agree."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import nfopp
from nfopp import _lib, lattice, torch_ops

import lattice_gears_cases as gc
import lattice_gears_ref as gr
import lattice_ref as lr
from grid_search_ref import Cost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-motion-planner_amd", "csrc")


def _start_cost(field, start, costs):
    return gr.trace_path(field, start, costs)[3]


# ---- the restated rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(gc.HAND)))
def test_hand_values(case):
    rows, cols, goal, costs, expected = gc.HAND[case]
    layers = np.zeros((1, rows, cols), np.uint8)
    field = gr.gear_field(layers, goal, costs)
    for start, pair in expected:
        cells, heads, gears, cost = gr.trace_path(field, start, costs)
        assert cost == pair, (start, cost)
        if pair != gc.UNREACHABLE:
            assert gr.check_path(layers, cells, heads, gears, start, goal, costs)[0] == pair
    # the forward-only search still cannot turn in three rows, nor back out of the corridor
    if (rows, cols) in ((3, 7), (1, 6)) and goal != (0, 5, 0):
        old = lr.lattice_field(layers, goal, costs[0])
        assert all(tuple(old[s[2], s[0], s[1]]) == gc.UNREACHABLE for s, _ in expected)


def test_the_hand_path_of_the_three_point_turn():
    layers, goal, costs = np.zeros((1, 3, 7), np.uint8), (0, 6, 0), (0, 1, 3)
    path = gc.HAND_PATH
    cells, heads = [p[:2] for p in path], [p[2] for p in path]
    gears = [path[1][3]] + [p[3] for p in path[1:]]
    cost, changes = gr.check_path(layers, np.asarray(cells), heads, gears, path[0][:3], goal, costs)
    assert cost == (11, 2) and changes == 2 and gr.gear_changes(gears, len(gears)) == 2
    assert tuple(map(sum, zip(*gc.HAND_PATH_MOVES))) == (11, 2)
    for k in range(1, len(path)):                            # move by move against the hand costs
        sub, _ = gr.check_path(layers, np.asarray(cells[k - 1:k + 1]), heads[k - 1:k + 1], [gears[k]] * 2, path[k - 1][:3],
                               (cells[k][0], cells[k][1], heads[k]), costs)
        cusp = costs[2] if k > 1 and gears[k] != gears[k - 1] else 0
        assert (sub[0] + cusp, sub[1]) == gc.HAND_PATH_MOVES[k - 1], k
    # the trace order happens to return this very path
    field = gr.gear_field(layers, goal, costs)
    got = gr.trace_path(field, path[0][:3], costs)
    assert [tuple(c) for c in got[0]] == cells and list(got[1]) == heads and list(got[2]) == gears and got[3] == (11, 2)


@pytest.mark.parametrize("n_layers,costs", [(1, (0, 0, 0)), (1, (1, 2, 3)), (8, (2, 1, 0)), (8, (0, 0, 4))])
def test_consequences_i_and_ii_on_random_maps(n_layers, costs):
    layers = gc.random_map(n_layers)
    _, rows, cols = layers.shape
    rng = np.random.default_rng(3)
    seen_equal = seen_lower = 0
    for goal in [(int(rng.integers(rows)), int(rng.integers(cols)), int(rng.integers(-1, 8))) for _ in range(6)]:
        field = gr.gear_field(layers, goal, costs)
        old = lr.lattice_field(layers, goal, costs[0])
        free = lr.free_mask(layers, goal)
        assert (field[:, ~free] == -1).all()
        for h in range(8):
            for r in range(rows):
                for c in range(cols):
                    cells, heads, gears, cost = gr.trace_path(field, (r, c, h), costs)
                    is_goal = tuple(field[0, h, r, c]) == (0, 0)
                    if free[h, r, c] and not is_goal:                         # (i)
                        both = [Cost(tuple(int(v) for v in field[s, h, r, c])) for s in range(2) if field[s, h, r, c, 0] >= 0]
                        assert cost == (tuple(min(both)) if both else gc.UNREACHABLE), (goal, r, c, h)
                    if old[h, r, c, 0] >= 0:                                  # (ii)
                        assert cost[0] >= 0 and not Cost(tuple(int(v) for v in old[h, r, c])) < Cost(cost)
                        if not gears.any():
                            assert cost == tuple(old[h, r, c])
                            seen_equal += 1
                        else:
                            seen_lower += Cost(cost) < Cost(tuple(int(v) for v in old[h, r, c]))
                    elif cost[0] >= 0:
                        seen_lower += 1                                       # reachable only with a reverse move
    assert seen_equal > 100 and seen_lower > 0


@pytest.mark.parametrize("n_layers,costs", [(1, (1, 0, 2)), (8, (0, 0, 3)), (8, (2, 0, 0))])
def test_consequence_iii_zero_reverse_cost_makes_the_cost_symmetric(n_layers, costs):
    layers = gc.random_map(n_layers)
    _, rows, cols = layers.shape
    rng = np.random.default_rng(9)
    states = [(r, c, h) for h in range(8) for r in range(rows) for c in range(cols) if not layers[h % n_layers, r, c]]
    states = [states[i] for i in rng.choice(len(states), 40, replace=False)]
    fields = {s: gr.gear_field(layers, s, costs) for s in states}
    finite = differ = 0
    for a in states:
        for b in states:
            ab, ba = _start_cost(fields[b], a, costs), _start_cost(fields[a], b, costs)
            assert ab == ba, (a, b, ab, ba)
            finite += ab[0] >= 0
    assert finite > 400
    # with a reverse cost the symmetry goes: the check above can fail
    costs = (costs[0], 2, costs[2])
    fields = {s: gr.gear_field(layers, s, costs) for s in states[:12]}
    for a in states[:12]:
        for b in states[:12]:
            differ += _start_cost(fields[b], a, costs) != _start_cost(fields[a], b, costs)
    assert differ > 0


# ---- the cases of the device tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,costs", gc.TRACE_SHAPES, ids=lambda v: str(v))
def test_every_traced_path_is_a_path_of_its_cost_and_follows_the_recursive_statement(name, costs):
    layers = gc.layers_of(name)
    fields = gc.fields_of(name, costs)
    starts, goals, fidx, (cells, heads, gears, count, status, cost) = gc.trace_case(name, costs)
    assert {0, 2} <= set(np.unique(status))                  # test_the_trace_cases_cover_the_rule asks for status 1 as well
    for p in range(len(starts)):
        if status[p] != 0:
            assert count[p] == 0 and tuple(cost[p]) == (-1, -1)
            continue
        k = count[p]
        got, changes = gr.check_path(layers, cells[p, :k], heads[p, :k], gears[p, :k], starts[p], goals[p], costs)
        assert got == tuple(cost[p]) and changes == gr.gear_changes(gears[p], k), p
        rec = gr.trace_recursive(fields[fidx[p]], tuple(starts[p]) + (None,), costs)
        assert [s[:3] for s in rec] == [(int(cells[p, j, 0]), int(cells[p, j, 1]), int(heads[p, j])) for j in range(k)], p
        assert [s[3] for s in rec[1:]] == [int(v) for v in gears[p, 1:k]], p


def test_the_trace_cases_cover_the_rule():
    seen = set()
    heads_seen, status_seen = set(), set()
    for name, costs in gc.TRACE_SHAPES:
        layers = gc.layers_of(name)
        L = layers.shape[0]
        starts, goals, fidx, (cells, heads, gears, count, status, cost) = gc.trace_case(name, costs)
        status_seen |= set(int(v) for v in status)
        for p in np.flatnonzero(status == 0):
            k = count[p]
            h, g = heads[p, :k], gears[p, :k]
            heads_seen |= set(int(v) for v in h)
            if k == 1:
                seen.add("start is a goal")
                continue
            seen.add("first move reverse" if g[0] else "first move forward")
            if layers[starts[p][2] % L, starts[p][0], starts[p][1]]:
                seen.add("blocked start")
            if layers[h[-1] % L, cells[p, k - 1, 0], cells[p, k - 1, 1]]:
                seen.add("goal on a wall")
            for j in range(1, k):
                if g[j]:
                    seen.add("reverse turn %+d" % (((h[j] - h[j - 1] + 4) % 8) - 4))
                if j > 1 and g[j] != g[j - 1]:
                    seen.add("gear change %d to %d" % (g[j - 1], g[j]))
                r, c = cells[p, j]
                if L == 8 and j < k - 1 and not layers[h[j], r, c] and layers[:, r, c].any():
                    seen.add("free at one heading, blocked at another")
    assert status_seen == {0, 1, 2} and heads_seen == set(range(8))
    assert seen == {"start is a goal", "first move reverse", "first move forward", "blocked start", "goal on a wall",
                    "reverse turn +0", "reverse turn +1", "reverse turn -1", "gear change 0 to 1", "gear change 1 to 0",
                    "free at one heading, blocked at another"}, seen


def test_the_device_shapes_sit_where_their_names_say():
    lib = _lib.load()
    for name, (rows, cols, _, _, cost_sets, _) in gc.SHAPES.items():
        for costs in cost_sets:
            ws = lib.nfopp_lattice_gear_fields_workspace_bytes(rows, cols, costs[0], costs[1], costs[2], 3)
            lds = gc.lds_words(name) <= gc.LG_LDS_WORDS and gc.counts(name, costs) <= 65535
            assert lds == ((name, costs) not in gc.WIDE), (name, costs)
            assert ws == (0 if lds else 3 * gc.lds_words(name) * 8), (name, costs, "the form moved: replace the shape")
            assert gc.counts(name, costs) < 2 ** 21
    assert {n for n, _ in gc.WIDE} < set(gc.SHAPES)
    # by words: exactly LG_LDS_WORDS, and one row more; by counts: the last packed count and the first wide one on 254 x 7
    assert gc.lds_words("254x7") == gc.LG_LDS_WORDS < gc.lds_words("255x7")
    assert gc.counts("254x7", (0, 1, 0)) <= 65535 < gc.counts("254x7", (1, 0, 1))
    assert gc.counts("9x65", (2, 1, 3)) == 65520 and gc.counts("9x65", (2, 1, 4)) > 65535
    assert lib.nfopp_lattice_gear_fields_workspace_bytes(9, 65, 2, 1, 3, 1) == 0 < lib.nfopp_lattice_gear_fields_workspace_bytes(9, 65, 2, 1, 4, 1)
    # the last square grid whose padded 16-layer field (odd row stride) fits 36864 words, and the first that does not
    assert lib.nfopp_lattice_gear_fields_workspace_bytes(45, 45, 0, 0, 0, 1) == 0 < lib.nfopp_lattice_gear_fields_workspace_bytes(46, 46, 0, 0, 0, 1)
    assert gc.n_lines("2x300") > gc.LG_THREADS and gc.n_lines("300x2") > gc.LG_THREADS
    assert max(gc.n_lines(n) for n in ("1x1", "1x2", "1x6", "2x7", "3x7", "5x5w", "20x23")) <= gc.LG_THREADS
    # 9 x 65 with a cost of 255 is beyond the 2^21 bound of the rule: 16 * 585 * 256
    assert 16 * 9 * 65 * 256 >= 2 ** 21 and lib.nfopp_lattice_gear_fields_workspace_bytes(9, 65, 0, 0, 255, 1) == 0
    assert _fields_rc(rows=9, cols=65, cc=255) != 0 and "2^21" in lib.nfopp_last_error().decode()
    for bad in ((0, 5, 0, 0, 0, 1), (5, 5, 256, 0, 0, 1), (5, 5, 0, 256, 0, 1), (5, 5, 0, 0, -1, 1), (5, 5, 0, 0, 0, 0), (256, 512, 0, 0, 0, 1)):
        assert lib.nfopp_lattice_gear_fields_workspace_bytes(*bad) == 0
    frame = open(os.path.join(CSRC, "lattice_field.h")).read()
    assert "constexpr int LATTICE_THREADS = %d;" % gc.LG_THREADS in frame and "constexpr int LATTICE_LDS_WORDS = %d;" % gc.LG_LDS_WORDS in frame
    src = open(os.path.join(CSRC, "lattice_gears.hip")).read()
    assert "constexpr int LG_STATES = 2 * LATTICE_HEADINGS;" in src and "for (int q = threadIdx.x; q < n_lines; q += LATTICE_THREADS)" in src


def test_the_seeding_knots_unwind_the_heading():
    q = np.pi / 4
    A = gr.heading_knots([7, 0, 1, 2, 3, 4, 5], 2 * np.pi - 0.8, 5 * q + 0.1 - 2 * np.pi)
    ths = np.float64(np.float32(2 * np.pi - 0.8))
    assert A[0] == ths and abs(A[1] - 7 * q) < 1e-12 and np.allclose(np.diff(A[1:-1]), q) and abs(A[-1] - (A[-2] + 0.1)) < 1e-6
    assert gr.wrap(np.pi) == np.pi and gr.wrap(-np.pi) == -np.pi and gr.wrap(-0.5) == -0.5         # rint: half to even
    assert abs(gr.wrap(2 * np.pi + 0.25) - 0.25) < 1e-15 and abs(gr.wrap(-4 * np.pi - 3.0) + 3.0) < 1e-14
    # a reverse run keeps the body heading: cells go west, headings stay 0
    th = gr.seed_theta([(0, c) for c in range(5, -1, -1)], [0] * 6, (5.5, 0.5, 0.0), (0.5, 0.5, 0.0), (0, 6, 0, 1), 1.0, 9)
    assert th.dtype == np.float32 and (th == 0).all()
    par = gr.chord_parameter(np.asarray([[0, 0], [3, 4], [3, 4], [6, 8]], np.float32))
    assert par[0] == 0 and par[-1] == 1 and (np.diff(par) > 0).all() and abs(par[1] - 0.5) < 1e-6


# ---- the C entries refuse before launch --------------------------------------------------------------------------------------
P = lambda v: ctypes.c_void_p(v) if v else None   # noqa: E731  (dummy device pointers: a refused call never reads them)


def _fields_rc(layers=8, n_layers=1, rows=5, cols=5, goals=8, n_goals=2, tc=0, rc=0, cc=0, out=8, ws=0, ws_bytes=0):
    return _lib.load().nfopp_lattice_gear_distance_fields(P(layers), n_layers, rows, cols, P(goals), n_goals, tc, rc, cc, P(out),
                                                          P(ws), ws_bytes, None)


def _trace_rc(fields=8, first=0, n_fields=1, n_total=1, rows=5, cols=5, tc=0, rc=0, cc=0, starts=8, goals=8, fidx=8, batch=3,
              max_len=4, cells=8, heads=8, gears=8, count=8, status=8, cost=8):
    return _lib.load().nfopp_lattice_gear_trace_paths(P(fields), first, n_fields, n_total, rows, cols, tc, rc, cc, P(starts),
                                                      P(goals), P(fidx), batch, max_len, P(cells), P(heads), P(gears), P(count),
                                                      P(status), P(cost), None)


def _seed_rc(cells=8, heads=8, count=8, status=8, batch=2, max_len=4, start=8, goal=8, n=5, res=1.0, traj=8, ws=0, ws_bytes=0):
    return _lib.load().nfopp_lattice_seed_trajectories(P(cells), P(heads), P(count), P(status), batch, max_len, P(start), P(goal),
                                                       n, 0.0, 0.0, res, P(traj), P(ws), ws_bytes, None)


def test_every_argument_check_of_the_field_entry():
    lib = _lib.load()
    wide = 16 * 42 * 133 * 8 * 2
    for kw, word in ((dict(tc=-1), "turn_cost"), (dict(tc=256), "turn_cost"), (dict(rc=-1), "reverse_cost"),
                     (dict(rc=256), "reverse_cost"), (dict(cc=-1), "cusp_cost"), (dict(cc=256), "cusp_cost"),
                     (dict(n_layers=2), "1 or 8"), (dict(n_layers=0), "1 or 8"), (dict(rows=0), "1..32768"),
                     (dict(cols=32769), "1..32768"), (dict(rows=256, cols=512), "2^21"), (dict(rows=128, cols=128, tc=7), "2^21"),
                     (dict(rows=128, cols=128, rc=7), "2^21"), (dict(rows=128, cols=128, tc=2, rc=2, cc=3), "2^21"),
                     (dict(n_goals=-1), "goal count"), (dict(layers=0), "null"), (dict(goals=0), "null"), (dict(out=0), "null"),
                     (dict(rows=40, cols=130), "workspace too small"),
                     (dict(rows=40, cols=130, ws=8, ws_bytes=wide - 1), "workspace too small"),
                     (dict(rows=40, cols=130, ws=12, ws_bytes=wide), "aligned")):
        assert _fields_rc(**kw) != 0, kw
        assert word in lib.nfopp_last_error().decode(), (kw, lib.nfopp_last_error())
    assert _fields_rc(rows=128, cols=128, cc=7, n_goals=0) != 0              # refused even with nothing to do
    assert _fields_rc(n_goals=0, layers=0, goals=0, out=0) == 0             # nothing to do, nothing launched
    # the edge of the bound: 16 * 510 * 257 = 2^21 - 32 and 16 * 128 * 128 * (1 + 6) pass it and are then stopped by their
    # missing workspace; 16 * 256 * 512 = 2^21 and 16 * 128 * 128 * (1 + 7) = 2^21 are refused (above)
    for kw in (dict(rows=510, cols=257), dict(rows=128, cols=128, tc=1, rc=2, cc=3)):
        assert _fields_rc(**kw) != 0 and "workspace" in lib.nfopp_last_error().decode(), kw
    assert 16 * 510 * 257 == 2 ** 21 - 32 and 16 * 128 * 128 * 8 == 2 ** 21


def test_every_argument_check_of_the_trace_entry():
    lib = _lib.load()
    for kw, word in ((dict(rows=0), "sizes"), (dict(max_len=-1), "sizes"), (dict(cols=32769), "sizes"),
                     (dict(rows=256, cols=512), "limit"), (dict(rows=128, cols=128, cc=7), "limit"),
                     (dict(tc=256), "turn_cost"), (dict(tc=-1), "turn_cost"), (dict(rc=256), "reverse_cost"),
                     (dict(rc=-1), "reverse_cost"), (dict(cc=256), "cusp_cost"), (dict(cc=-1), "cusp_cost"),
                     (dict(first=-1), "field range"), (dict(first=1, n_fields=1, n_total=1), "field range"),
                     (dict(n_fields=-1), "field range"), (dict(batch=-1), "batch"), (dict(batch=2 ** 31), "batch"),
                     (dict(starts=0), "null"), (dict(goals=0), "null"), (dict(fidx=0), "null"), (dict(count=0), "null"),
                     (dict(status=0), "null"), (dict(fields=0), "null"), (dict(cells=0), "null"), (dict(heads=0), "null"),
                     (dict(gears=0), "null")):
        assert _trace_rc(**kw) != 0, kw
        assert word in lib.nfopp_last_error().decode(), (kw, lib.nfopp_last_error())
    assert _trace_rc(batch=0, starts=0, goals=0, fidx=0, count=0, status=0) == 0


def test_every_argument_check_of_the_seeding_entry():
    lib = _lib.load()
    big = 1200                                               # 7 * 1202 + 3 doubles > 64 KiB: the global-workspace form
    need = (7 * (big + 2) + 3) * 8 * 2
    assert lib.nfopp_lattice_seed_workspace_bytes(2, big) == need == lib.nfopp_grid_seed_workspace_bytes(2, big)
    assert lib.nfopp_lattice_seed_workspace_bytes(2, 100) == 0 == lib.nfopp_lattice_seed_workspace_bytes(0, big)
    for kw, word in ((dict(res=0.0), "resolution"), (dict(batch=-1), "sizes"), (dict(n=0), "sizes"), (dict(max_len=-1), "sizes"),
                     (dict(cells=0), "null"), (dict(heads=0), "null"), (dict(count=0), "null"), (dict(status=0), "null"),
                     (dict(start=0), "null"), (dict(goal=0), "null"), (dict(traj=0), "null"),
                     (dict(max_len=big), "workspace too small"), (dict(max_len=big, ws=8, ws_bytes=need - 1), "workspace too small"),
                     (dict(max_len=big, ws=12, ws_bytes=need), "aligned")):
        assert _seed_rc(**kw) != 0, kw
        assert word in lib.nfopp_last_error().decode(), (kw, lib.nfopp_last_error())
    assert _seed_rc(batch=0, cells=0, heads=0, count=0, status=0, start=0, goal=0, traj=0) == 0


# ---- Python ------------------------------------------------------------------------------------------------------------------
def test_python_checks():
    lg = nfopp.LatticeGrid(np.zeros((8, 4, 6)), (0.0, 6.0, 0.0, 4.0), 1.0)
    s = np.zeros((2, 3), np.float32)
    for kw in (dict(turn_cost=256), dict(reverse_cost=-1), dict(reverse_cost=256), dict(cusp_cost=1.5), dict(cusp_cost=256),
               dict(goal_heading="any")):
        with pytest.raises(ValueError):
            nfopp.lattice_gear_search_paths(lg, s, s, **kw)
    with pytest.raises(ValueError, match="reverse_cost"):
        nfopp.lattice_gear_fields(lg, np.zeros((1, 3)), reverse_cost=300)
    with pytest.raises(TypeError):
        nfopp.lattice_gear_search_paths(nfopp.OccupancyGrid(np.zeros((4, 6)), (0, 6, 0, 4), 1.0), s, s)
    big = nfopp.LatticeGrid(np.zeros((1, 256, 512)), (0, 512, 0, 256), 1.0)
    with pytest.raises(ValueError, match="2\\^21"):
        nfopp.lattice_gear_search_paths(big, s, s)
    with pytest.raises(ValueError, match="2\\^21"):
        nfopp.lattice_gear_search_init(big, s, s, 8)
    with pytest.raises(ValueError, match="2\\^21"):
        nfopp.lattice_gear_fields(nfopp.LatticeGrid(np.zeros((1, 128, 128)), (0, 128, 0, 128), 1.0), np.zeros((1, 3)), 2, 2, 3)
    with pytest.raises(TypeError):
        nfopp.GearLattice(nfopp.OccupancyGrid(np.zeros((4, 6)), (0, 6, 0, 4), 1.0))
    with pytest.raises(ValueError, match="cusp_cost"):
        nfopp.GearLattice(lg, cusp_cost=256)
    gl = nfopp.GearLattice(lg, 2, 3)
    assert gl.lgrid is lg and gl.reverse_cost == 2 and gl.cusp_cost == 3


def test_python_names_and_defaults():
    def names(f):
        return list(inspect.signature(f).parameters)

    def defaults(f):
        return {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}

    assert names(nfopp.lattice_gear_fields) == ["lgrid", "goal_states", "turn_cost", "reverse_cost", "cusp_cost"]
    assert defaults(nfopp.lattice_gear_fields) == dict(turn_cost=0, reverse_cost=0, cusp_cost=0)
    assert names(nfopp.lattice_gear_search_paths) == ["lgrid", "starts", "goals", "turn_cost", "reverse_cost", "cusp_cost",
                                                      "goal_heading", "max_field_bytes"]
    assert defaults(nfopp.lattice_gear_search_paths) == dict(turn_cost=0, reverse_cost=0, cusp_cost=0, goal_heading="fixed",
                                                             max_field_bytes=2 ** 30)
    assert names(nfopp.seed_lattice_trajectories) == ["lgrid", "cells", "headings", "count", "status", "starts", "goals",
                                                      "n_waypoints", "out"]
    assert names(nfopp.lattice_gear_search_init) == ["lgrid", "starts", "goals", "n_waypoints", "out", "turn_cost", "reverse_cost",
                                                     "cusp_cost", "goal_heading"]
    assert defaults(nfopp.lattice_gear_search_init) == dict(out=None, turn_cost=0, reverse_cost=0, cusp_cost=0, goal_heading="fixed")
    assert names(nfopp.GearLattice.__init__) == ["self", "lgrid", "reverse_cost", "cusp_cost"]
    assert defaults(nfopp.GearLattice.__init__) == dict(reverse_cost=0, cusp_cost=0)
    for name in ("GearLattice", "lattice_gear_fields", "lattice_gear_search_paths", "lattice_gear_search_init",
                 "seed_lattice_trajectories"):
        assert name in nfopp.__all__ and getattr(nfopp, name) is getattr(lattice, name)
    assert nfopp.BatchPlanner.seed_gear_changes is None
    # the forward-only entry points keep their signatures
    assert names(nfopp.lattice_search_paths) == ["lgrid", "starts", "goals", "turn_cost", "goal_heading", "max_field_bytes"]
    assert names(nfopp.BatchPlanner.init)[-1] == "seed_turn_cost"


def test_gear_changes_are_counted_from_the_gears():
    gears = torch.tensor([[1, 1, 0, 0, 1, 9], [0, 0, 0, 0, 0, 0], [1, 1, 0, 1, 0, 1], [0, 0, 1, 1, 1, 1]], dtype=torch.int32)
    count = torch.tensor([5, 1, 6, 6], dtype=torch.int32)
    status = torch.tensor([0, 0, 1, 0], dtype=torch.int32)
    got = lattice.gear_changes(gears, count, status)
    assert got.dtype == torch.int32 and got.tolist() == [2, 0, 0, 1]
    assert [gr.gear_changes(gears[i].numpy(), count[i]) for i in (0, 1, 3)] == [2, 0, 1]


def test_header_binding_library_and_build_agree():
    lib = nfopp.load_library()
    header = open(os.path.join(ROOT, "include", "nfopp_hip.h")).read()
    for name, n_args, res, ctype in (("nfopp_lattice_gear_distance_fields", 13, "int", ctypes.c_int),
                                     ("nfopp_lattice_gear_trace_paths", 21, "int", ctypes.c_int),
                                     ("nfopp_lattice_gear_fields_workspace_bytes", 6, "size_t", ctypes.c_size_t),
                                     ("nfopp_lattice_seed_trajectories", 16, "int", ctypes.c_int),
                                     ("nfopp_lattice_seed_workspace_bytes", 2, "size_t", ctypes.c_size_t)):
        decl = re.search(r"\b%s %s\(([^;]*)\);" % (res, name), header)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == n_args and _lib._SIGNATURES[name][0] is ctype
    assert lib.nfopp_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert "lattice_gears.hip" in open(os.path.join(CSRC, "Makefile")).read()
    kernel = open(os.path.join(CSRC, "lattice_gears.hip")).read()
    # the direction table is the one of csrc/lattice_field.h, pinned against the restatement in test_lattice_cpu.py
    frame = open(os.path.join(CSRC, "lattice_field.h")).read()
    line_map = re.compile(r"int h = 0, i = q;.*?len = len_r < len_c \? len_r : len_c;", re.S)
    own, shared = line_map.search(kernel).group(0), line_map.search(frame).group(0)
    assert [t.strip() for t in own.split("\n")] == [t.strip() for t in shared.split("\n")]    # the gear file's own line map, kept for
    assert "const int n_lines = lattice_n_lines(rows, cols);" in kernel                          # its kernels' time, is the header's text
    assert '#include "lattice_field.h"' in kernel and "LATTICE_DR[" in kernel and "__constant__" not in kernel
    sources = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h")))
    for once in ("{0, 1, 1, 1, 0, -1, -1, -1}", "{1, 1, 0, -1, -1, -1, 0, 1}", "2 * rows + 2 * cols + 4 * (rows + cols - 1)",
                 "(cols + 2) | 1"):
        assert sources.count(once) == 1, once                               # one table, one n_lines formula, one odd stride
    assert '#include "pair_cost.h"' in kernel and "struct Packed" not in kernel and "pair_key(T v)" not in kernel
    for text in (header, kernel, open(os.path.join(ROOT, "tests", "lattice_gears_ref.py")).read()):
        for word in ("h' in {h, h + 1, h - 1}", "forced free", "BEFORE", "reverse_cost", "cusp_cost", "forward h, h + 1, h - 1",
                     "no cusp cost", "one-state path"):
            assert word in re.sub(r"\s*\n\s*(//|\*)?\s*", " ", text), word
    seed = open(os.path.join(CSRC, "grid_search.hip")).read()
    assert seed.count("void seed_body(") == 1 and "nfopp_lattice_seed_trajectories" in seed   # one seeding body, shared


def test_the_torch_ops_are_registered_and_refuse_cpu_tensors():
    for name in ("lattice_gear_fields", "lattice_gear_trace_paths", "lattice_seed_trajectories"):
        assert name in torch_ops.OPS
    ops = torch_ops.load()
    i32 = torch.int32
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lattice_gear_fields(torch.zeros(1, 5, 5, dtype=torch.uint8), torch.zeros(1, 3, dtype=i32), 0, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lattice_gear_trace_paths(torch.zeros(1, 2, 8, 5, 5, 2, dtype=i32), 0, 1, torch.zeros(2, 3, dtype=i32),
                                     torch.zeros(2, 3, dtype=i32), torch.zeros(2, dtype=i32), 0, 0, 0, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lattice_seed_trajectories(torch.zeros(2, 4, 2, dtype=i32), torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32),
                                      torch.zeros(2, dtype=i32), torch.zeros(2, 3), torch.zeros(2, 3), 8, 0.0, 0.0, 1.0)
