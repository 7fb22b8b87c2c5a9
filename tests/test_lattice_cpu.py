"""CPU: the heading-aware lattice search (csrc/lattice_search.hip, nfopp/lattice.py) without a GPU -- the restated rule
(tests/lattice_ref.py) against hand cases and its own properties, what the cases of the device tests cover, every host
argument check of the C entries, the Python checks, and that header, binding and library agree."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import nfopp
from nfopp import _lib, lattice, torch_ops

import grid_search_ref as gsr
import lattice_cases as lc
import lattice_ref as lr

CSRC = os.path.join(ROOT, "pytorch-motion-planner_amd", "csrc")


def _empty(rows, cols):
    return np.zeros((1, rows, cols), np.uint8)


# ---- the rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(lc.HAND)))
def test_hand_cases_have_their_exact_pairs(case):
    rows, cols, goal, tc, expected = lc.HAND[case]
    field = lr.lattice_field(_empty(rows, cols), goal, tc)
    for (r, c, h), pair in expected:
        assert tuple(field[h, r, c]) == pair, (lc.HAND[case][:4], (r, c, h), tuple(field[h, r, c]))
        cells, heads, cost = lr.trace_path(field, (r, c, h), tc)
        if pair == lc.UNREACHABLE:
            assert len(cells) == 0 and cost == (-1, -1)
        else:
            assert cost == pair and lr.check_path(_empty(rows, cols), cells, heads, (r, c, h), goal, tc) == pair


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (4, 7), (5, 5), (9, 12)])
def test_without_walls_the_best_heading_costs_what_the_8_connected_search_costs(shape):
    """L = 1, turn_cost 0, free goal heading: an octile path turns by 45 degrees only, so min over h of d(c, h) is the
    8-connected field, exactly and in every cell."""
    rows, cols = shape
    rng = np.random.default_rng(rows + cols)
    for _ in range(3):
        g = (int(rng.integers(rows)), int(rng.integers(cols)))
        field = lr.lattice_field(_empty(rows, cols), g + (-1,), 0)
        want = gsr.dijkstra_field(np.zeros(shape, np.uint8), g)
        for r in range(rows):
            for c in range(cols):
                best = min([gsr.Cost(tuple(int(v) for v in field[h, r, c])) for h in range(8) if field[h, r, c, 0] >= 0],
                           default=lc.UNREACHABLE)
                assert tuple(best) == tuple(want[r, c]), (shape, g, r, c)


def test_with_walls_no_heading_is_cheaper_than_the_8_connected_search():
    rng = np.random.default_rng(5)
    occ = (rng.random((12, 14)) < 0.25).astype(np.uint8)
    for g in ((0, 0), (11, 13), (6, 7)):
        field = lr.lattice_field(occ[None], g + (-1,), 0)
        want = gsr.dijkstra_field(occ, g)
        reached = field[..., 0] >= 0
        assert reached.any()
        for h, r, c in np.argwhere(reached):
            assert want[r, c, 0] >= 0
            assert not gsr.Cost(tuple(int(v) for v in field[h, r, c])) < gsr.Cost(tuple(int(v) for v in want[r, c]))


@pytest.mark.parametrize("name,tc", [("5x5w", 0), ("5x5", 2), ("20x23", 1)])
def test_every_traced_path_obeys_the_rule_and_the_recursive_statement_agrees(name, tc):
    layers, goals, fields = lc.layers_of(name), lc.goals_of(name), lc.fields_of(name, tc)
    starts, goal_states, fidx = lc.trace_problems(name)
    pick = np.arange(len(starts)) if len(starts) <= 700 else np.random.default_rng(3).choice(len(starts), 700, replace=False)
    seen = 0
    for p in pick:
        field, goal = fields[fidx[p]], tuple(int(v) for v in goal_states[p])
        cells, heads, cost = lr.trace_path(field, starts[p], tc)
        own = tuple(int(v) for v in field[starts[p][2], starts[p][0], starts[p][1]])
        if len(cells) == 0:
            assert own == (-1, -1)
            continue
        assert lr.check_path(layers, cells, heads, starts[p], goal, tc) == cost
        if own != (-1, -1):
            assert cost == own
            rec = lr.trace_recursive(field, starts[p], tc)
            assert [tuple(s[:2]) for s in rec] == [tuple(c) for c in cells] and [s[2] for s in rec] == list(heads)
        seen += 1
    assert seen > len(pick) // 4


def test_what_the_device_cases_cover():
    """Computed from the restatement: every status, every heading in some path, both turn directions, a state free at one
    heading and blocked at another on a path (L = 8), a goal on a wall, a blocked start, a start whose only way into a
    fixed-heading goal is blocked."""
    statuses, headings_seen, turns = set(), set(), set()
    layer_dependent = wall_goal = blocked_start = False
    for name, tc in lc.TRACE_SHAPES:
        layers, fields = lc.layers_of(name), lc.fields_of(name, tc)
        rows, cols = layers.shape[1:]
        starts, goal_states, fidx = lc.trace_problems(name)
        step = max(1, len(starts) // 1500)
        cells, heads, count, status, _ = lr.search(fields, (rows, cols), starts[::step], goal_states[::step], fidx[::step], tc)
        statuses |= set(int(s) for s in status)
        for p in np.flatnonzero(status == 0):
            hs = heads[p, :count[p]]
            headings_seen |= set(int(h) for h in hs)
            turns |= set(int(d) for d in np.diff(hs) % 8)
            s, g = starts[::step][p], goal_states[::step][p]
            blocked_start |= bool(layers[s[2] % layers.shape[0], s[0], s[1]]) and count[p] > 1
            wall_goal |= bool(layers[0, g[0], g[1]])
            if layers.shape[0] == 8:
                for k in range(1, count[p]):
                    r, c = cells[p, k]
                    layer_dependent |= bool(layers[:, r, c].any()) and not layers[hs[k], r, c]
    off = lr.search(lc.fields_of("5x5", 0), (5, 5), [(5, 0, 0), (0, 0, 8), (0, 0, -1), (0, 0, 0)], [(2, 4, 0)] * 3 + [(5, 0, 0)],
                    [0, 0, 0, 4])[3]
    assert list(off) == [2, 2, 2, 2]
    statuses |= set(int(s) for s in off)
    assert statuses == {0, 1, 2}
    assert headings_seen == set(range(8)) and {1, 7} <= turns
    assert layer_dependent and wall_goal and blocked_start
    # the LDS form at its stride and capacity edges, against the kernel's constants as the shared frame (csrc/lattice_field.h)
    # states them: some shape that relaxes in LDS has more lines than the kernel has threads (2x300 / 300x2: 1808, four trips),
    # one fills LATTICE_LDS_WORDS exactly (510x7), and the shapes on the other side of each dispatch edge are wide
    frame = open(os.path.join(CSRC, "lattice_field.h")).read()
    for text in ("constexpr int LATTICE_THREADS = %d;" % lc.LS_THREADS, "constexpr int LATTICE_LDS_WORDS = %d;" % lc.LS_LDS_WORDS,
                 "{ return 2 * rows + 2 * cols + 4 * (rows + cols - 1); }", "*stride = (cols + 2) | 1;",
                 "n_state_layers * *padded <= LATTICE_LDS_WORDS && counts <= 65535", "constexpr int LATTICE_HEADINGS = 8;"):
        assert text in frame, (text, "the kernel's constant or loop moved: replace the shape sized by it")
    kernel = open(os.path.join(CSRC, "lattice_search.hip")).read()
    for text in ("constexpr int LS_STATES = LATTICE_HEADINGS;", "const int n_lines = lattice_n_lines(rows, cols);",   # 8 state layers
                 "for (int q = threadIdx.x; q < n_lines; q += LATTICE_THREADS)", "LS_STATES, \"8 * rows * cols * (1 + turn_cost) reaches"):
        assert text in kernel, (text, "the kernel's layer count or loop moved: replace the shape sized by it")
    in_lds = [(n, tc) for n, s in lc.SHAPES.items() for tc in s[4] if (n, tc) not in lc.WIDE]
    assert all(lc.lds_words(n) <= lc.LS_LDS_WORDS and 8 * lc.SHAPES[n][0] * lc.SHAPES[n][1] * (1 + tc) <= 65535 for n, tc in in_lds)
    assert max(lc.n_lines(n) for n, _ in in_lds) > 3 * lc.LS_THREADS
    assert lc.n_lines("2x300") == lc.n_lines("300x2") == 1808 and ("2x300", 3) in in_lds and ("300x2", 3) in in_lds
    assert any(lc.lds_words(n) == lc.LS_LDS_WORDS for n, _ in in_lds) and lc.lds_words("510x7") == 8 * 512 * 9 == lc.LS_LDS_WORDS
    assert ("510x7", 1) in in_lds and 8 * 510 * 7 * 2 == 57120 <= 65535 < 8 * 510 * 7 * 3 and ("510x7", 2) in lc.WIDE
    assert lc.lds_words("511x7") == 8 * 513 * 9 > lc.LS_LDS_WORDS and ("511x7", 0) in lc.WIDE
    assert lc.lds_words("65x65") == 35912 and ("65x65", 0) in in_lds
    assert {("2x300", 0), ("510x7", 1)} <= set(lc.TRACE_SHAPES)
    layers, goal = lc.approach_case()
    fixed, free = lr.lattice_field(layers, goal, 0), lr.lattice_field(layers, goal[:2] + (-1,), 0)
    assert tuple(fixed[0, 1, 0]) == (-1, -1) and len(lr.trace_path(fixed, (1, 0, 0))[0]) == 0      # status 1
    assert (fixed[:, 1, 3] == np.where(np.arange(8)[:, None] == 0, 0, -1)).all()                   # only the goal state itself
    assert free[0, 1, 0, 0] >= 0                                                                   # any heading: reachable


def test_heading_index_rounds_half_to_even_in_float64():
    q = np.pi / 4
    theta = torch.tensor([0.0, q / 2, -q / 2, -q, 2 * np.pi, -np.pi, 7.6 * q, float("nan"), float("inf")], dtype=torch.float64)
    assert nfopp.heading_index(theta).tolist() == [0, 0, 0, 7, 0, 4, 0, -1, -1]
    assert nfopp.heading_index(theta).dtype == torch.int32
    rng = np.random.default_rng(0)
    th = rng.uniform(-20, 20, 500).astype(np.float32)
    assert nfopp.heading_index(torch.tensor(th)).tolist() == [lr.heading_index(t) for t in th]


# ---- the C entries refuse before launch ------------------------------------------------------------------------------------
P = lambda v: ctypes.c_void_p(v) if v else None   # noqa: E731  (dummy device pointers: a refused call never reads them)


def _fields_rc(layers=8, n_layers=1, rows=5, cols=5, goals=8, n_goals=2, tc=0, out=8, ws=0, ws_bytes=0):
    return _lib.load().nfopp_lattice_distance_fields(P(layers), n_layers, rows, cols, P(goals), n_goals, tc, P(out), P(ws),
                                                     ws_bytes, None)


def _trace_rc(fields=8, first=0, n_fields=1, n_total=1, rows=5, cols=5, tc=0, starts=8, goals=8, fidx=8, batch=3, max_len=4,
              cells=8, heads=8, count=8, status=8, cost=8):
    return _lib.load().nfopp_lattice_trace_paths(P(fields), first, n_fields, n_total, rows, cols, tc, P(starts), P(goals),
                                                 P(fidx), batch, max_len, P(cells), P(heads), P(count), P(status), P(cost), None)


def test_every_argument_check_of_the_field_entry():
    lib = _lib.load()
    for kw, word in ((dict(tc=-1), "turn_cost"), (dict(tc=256), "turn_cost"), (dict(n_layers=2), "1 or 8"),
                     (dict(n_layers=0), "1 or 8"), (dict(rows=0), "1..32768"), (dict(cols=32769), "1..32768"),
                     (dict(rows=512, cols=512), "2^21"), (dict(rows=128, cols=128, tc=15), "2^21"),
                     (dict(n_goals=-1), "goal count"), (dict(layers=0), "null"), (dict(goals=0), "null"), (dict(out=0), "null"),
                     (dict(rows=40, cols=130, tc=1), "workspace too small"),
                     (dict(rows=40, cols=130, tc=1, ws=8, ws_bytes=8 * 42 * 133 * 8 * 2 - 1), "workspace too small"),
                     (dict(rows=40, cols=130, tc=1, ws=12, ws_bytes=8 * 42 * 133 * 8 * 2), "aligned")):
        assert _fields_rc(**kw) != 0, kw
        assert word in lib.nfopp_last_error().decode(), (kw, lib.nfopp_last_error())
    assert _fields_rc(rows=128, cols=128, tc=15, n_goals=0) != 0            # refused even with nothing to do
    assert _fields_rc(n_goals=0, layers=0, goals=0, out=0) == 0             # nothing to do, nothing launched
    # 8 * rows * cols * (1 + turn_cost) = 2^21 - 8 passes the bound and is then stopped by its missing workspace
    assert _fields_rc(rows=511, cols=513, tc=0) != 0 and "workspace" in lib.nfopp_last_error().decode()


def test_every_argument_check_of_the_trace_entry():
    lib = _lib.load()
    for kw, word in ((dict(rows=0), "sizes"), (dict(max_len=-1), "sizes"), (dict(rows=512, cols=512), "limit"),
                     (dict(tc=256), "turn_cost"), (dict(tc=-1), "turn_cost"), (dict(first=-1), "field range"),
                     (dict(first=1, n_fields=1, n_total=1), "field range"), (dict(n_fields=-1), "field range"),
                     (dict(batch=-1), "batch"), (dict(batch=2 ** 31), "batch"), (dict(starts=0), "null"), (dict(goals=0), "null"),
                     (dict(fidx=0), "null"), (dict(count=0), "null"), (dict(status=0), "null"), (dict(fields=0), "null"),
                     (dict(cells=0), "null"), (dict(heads=0), "null")):
        assert _trace_rc(**kw) != 0, kw
        assert word in lib.nfopp_last_error().decode(), (kw, lib.nfopp_last_error())
    assert _trace_rc(batch=0, starts=0, goals=0, fidx=0, count=0, status=0) == 0


def test_the_workspace_query_names_the_form_of_every_device_shape():
    lib = _lib.load()
    for name, (rows, cols, _, _, tcs, _) in lc.SHAPES.items():
        for tc in tcs:
            ws = lib.nfopp_lattice_fields_workspace_bytes(rows, cols, tc, 3)
            if (name, tc) in lc.WIDE:
                assert ws == 3 * 8 * (rows + 2) * ((cols + 2) | 1) * 8, (name, tc, "now relaxes in LDS: replace the shape")
            else:
                assert ws == 0, (name, tc, "now needs a workspace: replace the shape")
    assert {n for n, _ in lc.WIDE} < set(lc.SHAPES)
    # the last square grid whose padded 8-layer field (odd row stride) fits 36864 words, and the first that does not
    assert lib.nfopp_lattice_fields_workspace_bytes(65, 65, 0, 1) == 0 < lib.nfopp_lattice_fields_workspace_bytes(66, 66, 0, 1)
    # counts: 8 * 30 * 30 * (1 + 8) = 64800 still packs, turn_cost 9 does not
    assert lib.nfopp_lattice_fields_workspace_bytes(30, 30, 8, 1) == 0 < lib.nfopp_lattice_fields_workspace_bytes(30, 30, 9, 1)
    for bad in ((0, 5, 0, 1), (5, 5, 256, 1), (5, 5, 0, 0), (512, 512, 0, 1)):
        assert lib.nfopp_lattice_fields_workspace_bytes(*bad) == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_python_shape_and_type_checks():
    b = (0.0, 5.0, 0.0, 5.0)
    for layers in (np.zeros((5, 5)), np.zeros((2, 5, 5)), np.zeros((8, 0, 5)), np.zeros((1, 1, 5, 5))):
        with pytest.raises(ValueError):
            nfopp.LatticeGrid(layers, b, 1.0)
    with pytest.raises(ValueError):
        nfopp.LatticeGrid(np.zeros((1, 5, 5)), b, 0.0)
    with pytest.raises(ValueError):
        nfopp.LatticeGrid(np.zeros((1, 5, 5)), b[:3], 1.0)
    lg = nfopp.LatticeGrid(np.zeros((8, 4, 6)), (0.0, 6.0, 0.0, 4.0), 1.0)
    assert lg.shape == (4, 6) and lg.n_layers == 8 and lg.layers_host.dtype == np.uint8
    one = nfopp.LatticeGrid.from_grid(nfopp.OccupancyGrid(np.eye(4), (0, 4, 0, 4), 1.0))
    assert one.n_layers == 1 and np.array_equal(one.layers_host[0], np.eye(4, dtype=np.uint8)) and one.resolution == 1.0
    s = np.zeros((2, 3), np.float32)
    for kw in (dict(turn_cost=256), dict(turn_cost=-1), dict(turn_cost=1.5), dict(goal_heading="any")):
        with pytest.raises(ValueError):
            nfopp.lattice_search_paths(lg, s, s, **kw)
    with pytest.raises(TypeError):
        nfopp.lattice_search_paths(nfopp.OccupancyGrid(np.zeros((4, 6)), (0, 6, 0, 4), 1.0), s, s)
    with pytest.raises(ValueError, match="2\\^21"):
        nfopp.lattice_search_paths(nfopp.LatticeGrid(np.zeros((1, 512, 512)), (0, 512, 0, 512), 1.0), s, s)
    with pytest.raises(ValueError, match="2\\^21"):
        nfopp.lattice_fields(nfopp.LatticeGrid(np.zeros((1, 128, 128)), (0, 128, 0, 128), 1.0), np.zeros((1, 3)), turn_cost=15)
    with pytest.raises(TypeError):
        nfopp.LatticeGrid.from_checker(object(), 0.5, boundaries=b)
    with pytest.raises(TypeError):
        nfopp.LatticeGrid.from_checker(object(), None)


def test_python_names_and_defaults():
    assert list(inspect.signature(nfopp.lattice_search_paths).parameters) == \
        ["lgrid", "starts", "goals", "turn_cost", "goal_heading", "max_field_bytes"]
    sig = inspect.signature(nfopp.lattice_search_paths).parameters
    assert sig["turn_cost"].default == 0 and sig["goal_heading"].default == "fixed" and sig["max_field_bytes"].default == 2 ** 30
    sig = inspect.signature(nfopp.lattice_search_init).parameters
    assert list(sig) == ["lgrid", "starts", "goals", "n_waypoints", "init_angles_with_trajectory", "out", "turn_cost", "goal_heading"]
    assert sig["init_angles_with_trajectory"].default is True and sig["out"].default is None
    assert list(inspect.signature(nfopp.lattice_fields).parameters) == ["lgrid", "goal_states", "turn_cost"]
    init = inspect.signature(nfopp.BatchPlanner.init).parameters
    assert list(init)[-1] == "seed_turn_cost" and init["seed_turn_cost"].default == 0
    # the 8-connected entry points keep their signatures
    assert list(inspect.signature(nfopp.grid_search_init).parameters)[-3:] == ["clearance", "any_angle", "lookahead"]
    assert lattice.HEADINGS == 8 and lr.DIRS[1] == (1, 1) and lr.DIRS[6] == (-1, 0)


def test_header_binding_library_and_build_agree():
    lib = nfopp.load_library()
    header = open(os.path.join(ROOT, "include", "nfopp_hip.h")).read()
    for name, n_args, res, ctype in (("nfopp_lattice_distance_fields", 11, "int", ctypes.c_int),
                                     ("nfopp_lattice_trace_paths", 18, "int", ctypes.c_int),
                                     ("nfopp_lattice_fields_workspace_bytes", 4, "size_t", ctypes.c_size_t)):
        decl = re.search(r"\b%s %s\(([^;]*)\);" % (res, name), header)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == n_args and _lib._SIGNATURES[name][0] is ctype
    assert lib.nfopp_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert "lattice_search.hip" in open(os.path.join(CSRC, "Makefile")).read()
    kernel = open(os.path.join(CSRC, "lattice_search.hip")).read()
    frame = open(os.path.join(CSRC, "lattice_field.h")).read()
    dirs = re.search(r"LATTICE_DR\[LATTICE_HEADINGS\] = \{([^}]*)\};\s*inline __constant__ int LATTICE_DC\[LATTICE_HEADINGS\] = "
                     r"\{([^}]*)\};", frame)
    got = tuple(zip(*[[int(v) for v in g.split(",")] for g in dirs.groups()]))
    assert got == lr.DIRS                                                   # the one direction table against the restatement
    assert '#include "lattice_field.h"' in kernel and "__constant__" not in kernel and "$(wildcard *.h)" in \
        open(os.path.join(CSRC, "Makefile")).read()                         # the object rule names every header of the directory
    for text in (header, kernel, open(os.path.join(ROOT, "tests", "lattice_ref.py")).read()):
        for word in ("h' in {h, h + 1, h - 1}", "forced free", "turn_cost", "AFTER"):
            assert word in text, word


def test_the_torch_ops_are_registered_and_refuse_cpu_tensors():
    assert "lattice_fields" in torch_ops.OPS and "lattice_trace_paths" in torch_ops.OPS
    ops = torch_ops.load()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lattice_fields(torch.zeros(1, 5, 5, dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.int32), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lattice_trace_paths(torch.zeros(1, 8, 5, 5, 2, dtype=torch.int32), 0, 1, torch.zeros(2, 3, dtype=torch.int32),
                                torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 0, 4)
