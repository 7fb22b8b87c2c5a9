"""GPU: the heading-aware lattice search (csrc/lattice_search.hip, nfopp/lattice.py) against the rule restated in
tests/lattice_ref.py (test_lattice_cpu.py checks the restatement and the cases without a GPU).

Everything compared here is an integer (fields, cells, headings, counts, costs, status) or comes from the same kernel on
the same input (seeded trajectories, checker labels): every comparison is `==` on the bits.

Measured on an MI355X: the whole file takes 6.6 s.  The shapes at the LDS form's stride and capacity edges (2x300, 300x2,
510x7, 511x7, 65x65: lattice_cases.SHAPES) take 2.2 s of it, mostly their restated fields and traces, none more than 0.6 s."""
import functools

import numpy as np
import pytest
import torch

import nfopp
from nfopp import _lib, torch_ops

import lattice_cases as lc
import lattice_ref as lr

pytestmark = pytest.mark.gpu
I32 = torch.int32
SENT = -7            # sentinel of integer output buffers
GUARD = 300          # sentinel entries after every integer output buffer


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _lgrid(name):
    rows, cols = lc.SHAPES[name][:2]
    return nfopp.LatticeGrid(lc.layers_of(name), (0.0, float(cols), 0.0, float(rows)), 1.0, device="cuda")


# ---- a. fields -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fields(name, tc):
    """-> device fields int32 [G, 8, rows, cols, 2] of the shape's goals; two runs, bit-identical."""
    lg, goals = _lgrid(name), _dev(lc.goals_of(name), I32)
    a = nfopp.lattice_fields(lg, goals, tc)
    b = nfopp.lattice_fields(lg, goals, tc)
    assert torch.equal(a, b), "two runs differ"
    return a


@pytest.mark.parametrize("name,tc", [(n, tc) for n, s in lc.SHAPES.items() for tc in s[4]], ids=lambda v: str(v))
def test_fields_equal_the_restated_rule_bit_for_bit(name, tc):
    rows, cols = lc.SHAPES[name][:2]
    goals = lc.goals_of(name)
    wide = _lib.load().nfopp_lattice_fields_workspace_bytes(rows, cols, tc, len(goals)) > 0
    assert wide == ((name, tc) in lc.WIDE)
    got, want = _fields(name, tc).cpu().numpy(), lc.fields_of(name, tc)
    assert got.shape == want.shape == (len(goals), 8, rows, cols, 2)
    for j, g in enumerate(goals):
        assert np.array_equal(got[j], want[j]), (name, tc, tuple(g), int((got[j] != want[j]).any(-1).sum()))
        if not lr.goal_ok((rows, cols), g):
            assert (got[j] == -1).all()                                   # off the grid, or a heading outside -1 .. 7
        else:
            forced = got[j][:, g[0], g[1]] if g[2] < 0 else got[j][g[2], g[0], g[1]][None]
            assert (forced == 0).all()                                    # goal states are free, on a wall too


@pytest.mark.parametrize("case", range(len(lc.HAND)))
def test_hand_cases_on_the_device(case):
    rows, cols, goal, tc, expected = lc.HAND[case]
    lg = nfopp.LatticeGrid(np.zeros((1, rows, cols), np.uint8), (0.0, cols, 0.0, rows), 1.0)
    field = nfopp.lattice_fields(lg, _dev([goal], I32), tc).cpu().numpy()[0]
    for (r, c, h), pair in expected:
        assert tuple(field[h, r, c]) == pair, ((r, c, h), tuple(field[h, r, c]))


# ---- b. trace --------------------------------------------------------------------------------------------------------------
def _trace(fields, first, n_total, rows, cols, tc, starts, goals, fidx, max_len):
    """nfopp_lattice_trace_paths on sentinel-filled buffers with GUARD sentinel entries behind each -> numpy (cells [B,
    max_len, 2], headings [B, max_len], count [B], status [B], cost [B, 2])."""
    lib = _lib.load()
    b = len(starts)
    sizes = (b * max_len * 2, b * max_len, b, b, 2 * b)
    bufs = [torch.full((n + GUARD,), SENT, dtype=I32, device="cuda") for n in sizes]
    starts, goals, fidx = _dev(starts, I32), _dev(goals, I32), _dev(fidx, I32)
    _lib.check(lib.nfopp_lattice_trace_paths(
        _lib.ptr(fields, I32), first, fields.shape[0], n_total, rows, cols, tc, _lib.ptr(starts, I32), _lib.ptr(goals, I32),
        _lib.ptr(fidx, I32), b, max_len, _lib.ptr(bufs[0], I32) if max_len else None, _lib.ptr(bufs[1], I32) if max_len else None,
        _lib.ptr(bufs[2], I32), _lib.ptr(bufs[3], I32), _lib.ptr(bufs[4], I32), _lib.stream_ptr()))
    out = [t.cpu().numpy() for t in bufs]
    for t, n in zip(out, sizes):
        assert (t[n:] == SENT).all(), "written behind the batch"
    return (out[0][:sizes[0]].reshape(b, max_len, 2), out[1][:sizes[1]].reshape(b, max_len), out[2][:b], out[3][:b],
            out[4][:2 * b].reshape(b, 2))


@functools.lru_cache(maxsize=None)
def _trace_case(name, tc):
    """Every state of the map as a start (blocked ones included) towards the first goals, then the refused problems."""
    rows, cols = lc.SHAPES[name][:2]
    starts, goals, fidx = lc.trace_problems(name)
    g0 = lc.goals_of(name)[0]
    n_goals = len(lc.goals_of(name))
    bad_starts = [(0, 0, 0), (0, 0, 0), (-1, 0, 0), (rows, 0, 0), (0, cols, 0), (0, -1, 0), (0, 0, -1), (0, 0, 8), (0, 0, 0)]
    bad_goals = [g0] * 8 + [(rows, 0, 0)]
    bad_fidx = [-1, n_goals, 0, 0, 0, 0, 0, 0, 4]
    starts = np.concatenate([starts, np.asarray(bad_starts, np.int32)])
    goals = np.concatenate([goals, np.asarray(bad_goals, np.int32)])
    fidx = np.concatenate([fidx, np.asarray(bad_fidx, np.int32)])
    want = lr.search(lc.fields_of(name, tc), (rows, cols), starts, goals, fidx, tc)
    assert (want[3][-9:] == 2).all()
    return starts, goals, fidx, want


@pytest.mark.parametrize("name,tc", lc.TRACE_SHAPES, ids=lambda v: str(v))
def test_trace_from_every_state_follows_the_restated_rule(name, tc):
    rows, cols = lc.SHAPES[name][:2]
    fields = _fields(name, tc)
    starts, goals, fidx, (w_cells, w_heads, w_count, w_status, w_cost) = _trace_case(name, tc)
    L = w_cells.shape[1]
    assert set(np.unique(w_status)) == {0, 1, 2} or name == "5x5"
    for max_len in (0, 1, L, L + 1):
        cells, heads, count, status, cost = _trace(fields, 0, len(fields), rows, cols, tc, starts, goals, fidx, max_len)
        assert np.array_equal(count, w_count) and np.array_equal(status, w_status) and np.array_equal(cost, w_cost), max_len
        for p in range(len(starts)):
            k = min(int(w_count[p]), max_len)
            assert np.array_equal(cells[p, :k], w_cells[p, :k]) and np.array_equal(heads[p, :k], w_heads[p, :k]), (max_len, p)
            assert (cells[p, k:] == SENT).all() and (heads[p, k:] == SENT).all(), (max_len, p)   # nothing behind the path
    # a batch of 257 cut from the same buffers, and one that starts in the middle of them
    for lo in (0, len(starts) - 257):
        sl = slice(lo, lo + 257)
        cells, heads, count, status, cost = _trace(fields, 0, len(fields), rows, cols, tc, starts[sl], goals[sl], fidx[sl], L)
        assert np.array_equal(count, w_count[sl]) and np.array_equal(status, w_status[sl]) and np.array_equal(cost, w_cost[sl])
        for p in range(257):
            k = int(count[p])
            assert np.array_equal(cells[p, :k], w_cells[lo + p, :k]) and np.array_equal(heads[p, :k], w_heads[lo + p, :k])


def test_trace_leaves_problems_of_other_field_chunks_alone():
    name, tc = "5x5w", 0
    rows, cols = lc.SHAPES[name][:2]
    fields = _fields(name, tc)
    starts, goals, fidx, (w_cells, w_heads, w_count, w_status, w_cost) = _trace_case(name, tc)
    L, n = w_cells.shape[1], len(fields)
    cells, heads, count, status, cost = _trace(fields[1:2].contiguous(), 1, n, rows, cols, tc, starts, goals, fidx, L)
    mine, refused = fidx == 1, w_status == 2
    assert refused[~mine].any() and (~refused[~mine]).any()
    assert np.array_equal(count[mine], w_count[mine]) and np.array_equal(cost[mine], w_cost[mine])
    assert np.array_equal(status[mine | refused], w_status[mine | refused])
    other = ~mine & ~refused
    assert (count[other] == SENT).all() and (status[other] == SENT).all() and (cost[other] == SENT).all()
    assert (cells[other] == SENT).all() and (heads[other] == SENT).all()


# ---- c. Python -------------------------------------------------------------------------------------------------------------
def _poses(states, rng, jitter=0.3):
    """(row, col, heading) -> poses off the cell centres: x = col + u, y = row + u, theta = h * pi / 4 + small."""
    s = np.asarray(states, np.float64)
    xy = s[:, [1, 0]] + rng.uniform(0.5 - jitter, 0.5 + jitter, (len(s), 2))
    th = s[:, 2] * (np.pi / 4) + rng.uniform(-0.3, 0.3, len(s))
    return np.concatenate([xy, th[:, None]], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _python_case():
    """257 problems on the 20 x 23 map with eight layers: random states as starts, goals among 12 distinct goal states."""
    name = "20x23"
    rows, cols = lc.SHAPES[name][:2]
    rng = np.random.default_rng(11)
    B = 257
    s = np.stack([rng.integers(0, rows, B), rng.integers(0, cols, B), rng.integers(0, 8, B)], 1)
    pool = np.stack([rng.integers(0, rows, 12), rng.integers(0, cols, 12), rng.integers(0, 8, 12)], 1)
    g = pool[rng.integers(0, 12, B)]
    starts, goals = _poses(s, rng), _poses(g, rng)
    starts[5, 0], goals[9, 1] = -2.0, rows + 3.0                             # outside the grid
    return name, s, g, starts, goals


def test_search_paths_in_three_chunks_equal_one_chunk_and_the_restated_rule():
    name, s, g, starts, goals = _python_case()
    lg = _lgrid(name)
    rows, cols = lg.shape
    for tc, mode in ((1, "fixed"), (0, "free")):
        one = nfopp.lattice_search_paths(lg, _dev(starts), _dev(goals), turn_cost=tc, goal_heading=mode)
        per_field = 8 * rows * cols * 8
        n_goals = len({tuple(v) for v in (g if mode == "fixed" else g[:, :2])})
        assert 7 <= n_goals <= 12
        three = nfopp.lattice_search_paths(lg, _dev(starts), _dev(goals), turn_cost=tc, goal_heading=mode,
                                           max_field_bytes=per_field * ((n_goals + 2) // 3))
        for a, b in zip(one, three):
            assert a.dtype == I32 and torch.equal(a, b)
        cells, heads, count, status, cost = [t.cpu().numpy() for t in one]
        gs = g.copy()
        if mode == "free":
            gs[:, 2] = -1
        ss = s.copy()
        ss[5, 1], gs[9, 0] = -2, rows + 3
        uniq = sorted({tuple(v) for v in gs})
        fields = np.stack([lr.lattice_field(lc.layers_of(name), u, tc) for u in uniq])
        want = lr.search(fields, (rows, cols), ss, gs, [uniq.index(tuple(v)) for v in gs], tc)
        assert list(want[3][[5, 9]]) == [2, 2] and {0, 1, 2} == set(np.unique(want[3]))
        for got, w in zip((cells, heads, count, status, cost), want):
            assert np.array_equal(got, w)


def test_lattice_from_checker_equals_eight_single_heading_label_calls():
    rng = np.random.default_rng(2)
    pts = rng.uniform(0.5, 7.5, (60, 2)).astype(np.float32)
    b = (0.0, 8.0, 0.0, 6.0)
    checker = nfopp.DeviceRectangleChecker(pts, (-0.2, 0.9, -0.25, 0.25), boundaries=b, device="cuda")
    lg = nfopp.LatticeGrid.from_checker(checker, 0.25)
    rows, cols = lg.shape
    assert lg.n_layers == 8 and lg.boundaries == b
    xs = (np.arange(cols) * 0.25 + 0.125 + b[0])
    ys = (np.arange(rows) * 0.25 + 0.125 + b[2])
    xy = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    differ = 0
    for h in range(8):
        poses = np.concatenate([xy, np.full((len(xy), 1), np.float32(h * np.pi / 4))], 1).astype(np.float32)
        want = (checker.labels(_dev(poses)) > 0).to(torch.uint8).reshape(rows, cols)
        assert torch.equal(lg.layers[h], want), h
        differ += int((lg.layers[h] != lg.layers[0]).sum())
    assert differ > 0 and 0 < int(lg.layers.sum()) < lg.layers.numel()       # the box is not a disc


def test_search_init_is_the_seeding_kernel_on_the_traced_cells():
    name, _, _, starts, goals = _python_case()
    lg = _lgrid(name)
    cells, _, count, status, _ = nfopp.lattice_search_paths(lg, _dev(starts), _dev(goals), turn_cost=1)
    line = nfopp.init_trajectories(_dev(starts), _dev(goals), 64, True)
    for directed in (True, False):
        traj, st = nfopp.lattice_search_init(lg, _dev(starts), _dev(goals), 64, directed, turn_cost=1)
        want = nfopp.seed_trajectories(lg, cells, count, status, _dev(starts), _dev(goals), 64, directed)
        assert traj.shape == (len(starts), 64, 3) and torch.equal(st, status) and torch.equal(traj, want)
    traj = nfopp.lattice_search_init(lg, _dev(starts), _dev(goals), 64, turn_cost=1)[0]     # directed by default
    bad = status != 0
    assert bool(bad.any()) and torch.equal(traj[bad], line[bad])                            # status != 0: the straight line
    out = torch.empty(len(starts), 64, 3, device="cuda")
    assert nfopp.lattice_search_init(lg, _dev(starts), _dev(goals), 64, out=out, turn_cost=1)[0].data_ptr() == out.data_ptr()
    assert torch.equal(out, traj)


def test_batch_planner_seeds_through_a_lattice_grid():
    import gpu_common as gc
    import grid_search_ref as gsr
    z = np.load(gsr.GOLDEN.replace("g19_astar_init", "g1_onf"), allow_pickle=False)
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    name, _, _, starts, goals = _python_case()
    lg = _lgrid(name)
    rows, cols = lg.shape
    bounds = (0.0, float(cols), 0.0, float(rows))
    bp = nfopp.BatchPlanner(onf, len(starts), 64, nfopp.TrajectoryHyper(), init_angles_with_trajectory=True)
    bp.init(starts, goals, bounds, initializer=lg, seed_turn_cost=1)
    want, status = nfopp.lattice_search_init(lg, _dev(starts), _dev(goals), 64, True, turn_cost=1)
    assert torch.equal(bp.seed_status, status) and torch.equal(bp.engine.traj.view(want.shape), want) and bp.seed_margin is None
    occ = nfopp.OccupancyGrid(lc.layers_of(name)[0], bounds, 1.0)
    for kw in (dict(initializer=lg, seed_clearance=0.5), dict(initializer=lg, seed_any_angle=True),
               dict(initializer=occ, seed_turn_cost=1), dict(seed_turn_cost=2)):
        with pytest.raises(ValueError):
            bp.init(starts, goals, bounds, **kw)
    onf2 = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=False).to("cuda")
    bp2 = nfopp.BatchPlanner(onf2, 4, 16, nfopp.TrajectoryHyper())
    with pytest.raises(ValueError, match="D = 3"):
        bp2.init(starts[:4, :2], goals[:4, :2], bounds, initializer=lg)


def test_the_torch_ops_equal_the_raw_calls():
    ops = torch_ops.load()
    name, tc = "20x23", 3
    rows, cols = lc.SHAPES[name][:2]
    lg, goals = _lgrid(name), _dev(lc.goals_of(name), I32)
    fields = ops.lattice_fields(lg.layers, goals, tc)
    assert torch.equal(fields, _fields(name, tc))
    starts, gstates, fidx, _ = _trace_case("20x23", 1)
    raw = _trace(fields, 0, len(fields), rows, cols, tc, starts, gstates, fidx, 30)
    got = ops.lattice_trace_paths(fields, 0, len(fields), _dev(starts, I32), _dev(gstates, I32), _dev(fidx, I32), tc, 30)
    for g, r in zip(got, raw):
        g = g.cpu().numpy()
        assert np.array_equal(np.where(r == SENT, 0, r), g)                  # the op's buffers start as zeros
    with pytest.raises(RuntimeError, match="goal_states"):
        ops.lattice_trace_paths(fields, 0, len(fields), _dev(starts, I32), _dev(gstates[:-1], I32), _dev(fidx, I32), tc, 30)
    with pytest.raises(RuntimeError, match="turn_cost"):
        ops.lattice_fields(lg.layers, goals, 256)


def test_the_5x5_seed_leaves_along_the_start_heading_and_the_8_connected_one_due_east():
    lg = nfopp.LatticeGrid(np.zeros((1, 5, 5), np.uint8), (0.0, 5.0, 0.0, 5.0), 1.0)
    grid = nfopp.OccupancyGrid(np.zeros((5, 5), np.uint8), (0.0, 5.0, 0.0, 5.0), 1.0)
    goal = [[4.5, 2.5, 0.0]]
    for h in (2, 6, 1, 7, 0):
        start = [[0.5, 2.5, h * np.pi / 4]]
        cells, heads, count, status, cost = [t.cpu().numpy() for t in nfopp.lattice_search_paths(lg, _dev(start), _dev(goal))]
        assert status[0] == 0 and heads[0, 0] == h and heads[0, count[0] - 1] == 0
        assert (heads[0, 1] - h) % 8 in (0, 1, 7)                            # within one heading step of the start heading
        assert tuple(cells[0, 1] - cells[0, 0]) == lr.DIRS[heads[0, 1]]
        if h in (2, 6):
            assert tuple(cost[0]) == (2, 2)
        g_cells, g_count, g_status, g_cost = [t.cpu().numpy() for t in nfopp.grid_search_paths(grid, _dev(start), _dev(goal))]
        assert g_status[0] == 0 and tuple(g_cells[0, 1] - g_cells[0, 0]) == (0, 1) and tuple(g_cost[0]) == (4, 0)   # due east
