"""GPU: the lattice search with reverse moves and gear changes (csrc/lattice_gears.hip, the seeding entry in
csrc/grid_search.hip, nfopp/lattice.py) against the rule restated in tests/lattice_gears_ref.py (test_lattice_gears_cpu.py
checks the restatement and the cases without a GPU).

Fields, cells, headings, gears, counts, costs and status are integers; the seeded xy comes from the same code on the same
cells; the seeded theta is float64 arithmetic without atan2, sin or cos, every operation rounded on its own, restated in numpy.
Every comparison is `==` on the bits.

9 x 65 at costs (0, 0, 255) cannot run: 16 * 585 * 256 >= 2^21, so the rule's own bound refuses it before launch
(test_lattice_gears_cpu.py asserts the refusal).  The cost of 255 runs on 7 x 65, the widest map of that family the bound admits.

Measured on an MI355X: the whole file takes 9 s, no case more than 1 s."""
import functools

import numpy as np
import pytest
import torch

import nfopp
from nfopp import _lib, torch_ops

import guarded as gd
import lattice_gears_cases as gc
import lattice_gears_ref as gr

pytestmark = pytest.mark.gpu
I32 = torch.int32
SENT = -7            # sentinel of integer output buffers
GUARD = 300          # sentinel entries after every integer output buffer


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _lgrid(name):
    rows, cols = gc.SHAPES[name][:2]
    return nfopp.LatticeGrid(gc.layers_of(name), (0.0, float(cols), 0.0, float(rows)), 1.0, device="cuda")


def _open_grid(rows, cols):
    return nfopp.LatticeGrid(np.zeros((1, rows, cols), np.uint8), (0.0, float(cols), 0.0, float(rows)), 1.0, device="cuda")


# ---- a. fields -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fields(name, costs):
    """-> device fields int32 [G, 2, 8, rows, cols, 2] of the shape's goals; two runs, bit-identical."""
    lg, goals = _lgrid(name), _dev(gc.goals_of(name), I32)
    a = nfopp.lattice_gear_fields(lg, goals, *costs)
    b = nfopp.lattice_gear_fields(lg, goals, *costs)
    assert torch.equal(a, b), "two runs differ"
    return a


@pytest.mark.parametrize("name,costs", [(n, c) for n, s in gc.SHAPES.items() for c in s[4]], ids=lambda v: str(v))
def test_fields_equal_the_restated_rule_bit_for_bit(name, costs):
    rows, cols = gc.SHAPES[name][:2]
    goals = gc.goals_of(name)
    wide = _lib.load().nfopp_lattice_gear_fields_workspace_bytes(rows, cols, costs[0], costs[1], costs[2], len(goals)) > 0
    assert wide == ((name, costs) in gc.WIDE)
    got, want = _fields(name, costs).cpu().numpy(), gc.fields_of(name, costs)
    assert got.shape == want.shape == (len(goals), 2, 8, rows, cols, 2)
    for j, g in enumerate(goals):
        assert np.array_equal(got[j], want[j]), (name, costs, tuple(g), int((got[j] != want[j]).any(-1).sum()))
        if not gr.goal_ok((rows, cols), g):
            assert (got[j] == -1).all()                                   # off the grid, or a heading outside -1 .. 7
        else:
            forced = got[j][:, :, g[0], g[1]] if g[2] < 0 else got[j][:, g[2], g[0], g[1]]
            assert (forced == 0).all()                                    # goal states are free at both gears, on a wall too


@pytest.mark.parametrize("case", range(len(gc.HAND)))
def test_hand_values_on_the_device(case):
    rows, cols, goal, costs, expected = gc.HAND[case]
    lg = _open_grid(rows, cols)
    starts = np.asarray([s for s, _ in expected], np.float64)
    poses = np.stack([starts[:, 1] + 0.5, starts[:, 0] + 0.5, starts[:, 2] * (np.pi / 4)], 1)
    gpose = np.asarray([[goal[1] + 0.5, goal[0] + 0.5, goal[2] * np.pi / 4]] * len(poses))
    out = nfopp.lattice_gear_search_paths(lg, _dev(poses), _dev(gpose), *costs)
    cost, status = out[5].cpu().numpy(), out[4].cpu().numpy()
    for p, (_, pair) in enumerate(expected):
        assert tuple(cost[p]) == pair and status[p] == (1 if pair == gc.UNREACHABLE else 0), (p, tuple(cost[p]))


# ---- b. trace --------------------------------------------------------------------------------------------------------------
def _trace(fields, first, n_total, rows, cols, costs, starts, goals, fidx, max_len):
    """nfopp_lattice_gear_trace_paths on sentinel-filled buffers with GUARD sentinel entries behind each -> numpy (cells [B,
    max_len, 2], headings [B, max_len], gears [B, max_len], count [B], status [B], cost [B, 2])."""
    lib = _lib.load()
    b = len(starts)
    sizes = (b * max_len * 2, b * max_len, b * max_len, b, b, 2 * b)
    bufs = [torch.full((n + GUARD,), SENT, dtype=I32, device="cuda") for n in sizes]
    starts, goals, fidx = _dev(starts, I32), _dev(goals, I32), _dev(fidx, I32)
    p = [_lib.ptr(t, I32) for t in bufs]
    _lib.check(lib.nfopp_lattice_gear_trace_paths(
        _lib.ptr(fields, I32), first, fields.shape[0], n_total, rows, cols, costs[0], costs[1], costs[2], _lib.ptr(starts, I32),
        _lib.ptr(goals, I32), _lib.ptr(fidx, I32), b, max_len, p[0] if max_len else None, p[1] if max_len else None,
        p[2] if max_len else None, p[3], p[4], p[5], _lib.stream_ptr()))
    out = [t.cpu().numpy() for t in bufs]
    for t, n in zip(out, sizes):
        assert (t[n:] == SENT).all(), "written behind the batch"
    return (out[0][:sizes[0]].reshape(b, max_len, 2), out[1][:sizes[1]].reshape(b, max_len), out[2][:sizes[2]].reshape(b, max_len),
            out[3][:b], out[4][:b], out[5][:2 * b].reshape(b, 2))


@pytest.mark.parametrize("name,costs", gc.TRACE_SHAPES, ids=lambda v: str(v))
def test_trace_from_every_state_follows_the_restated_rule(name, costs):
    rows, cols = gc.SHAPES[name][:2]
    fields = _fields(name, costs)
    starts, goals, fidx, (w_cells, w_heads, w_gears, w_count, w_status, w_cost) = gc.trace_case(name, costs)
    L = w_cells.shape[1]
    for max_len in (0, 1, L, L + 1):
        cells, heads, gears, count, status, cost = _trace(fields, 0, len(fields), rows, cols, costs, starts, goals, fidx, max_len)
        assert np.array_equal(count, w_count) and np.array_equal(status, w_status) and np.array_equal(cost, w_cost), max_len
        for p in range(len(starts)):
            k = min(int(w_count[p]), max_len)
            assert np.array_equal(cells[p, :k], w_cells[p, :k]) and np.array_equal(heads[p, :k], w_heads[p, :k]), (max_len, p)
            assert np.array_equal(gears[p, :k], w_gears[p, :k]), (max_len, p)
            assert (cells[p, k:] == SENT).all() and (heads[p, k:] == SENT).all() and (gears[p, k:] == SENT).all(), (max_len, p)
    # a batch of 257 cut from the same buffers, and one that ends with them
    for lo in (0, len(starts) - 257):
        sl = slice(lo, lo + 257)
        cells, heads, gears, count, status, cost = _trace(fields, 0, len(fields), rows, cols, costs, starts[sl], goals[sl], fidx[sl], L)
        assert np.array_equal(count, w_count[sl]) and np.array_equal(status, w_status[sl]) and np.array_equal(cost, w_cost[sl])
        for p in range(257):
            k = int(count[p])
            assert np.array_equal(cells[p, :k], w_cells[lo + p, :k]) and np.array_equal(heads[p, :k], w_heads[lo + p, :k])
            assert np.array_equal(gears[p, :k], w_gears[lo + p, :k])


def test_trace_leaves_problems_of_other_field_chunks_alone():
    name, costs = gc.TRACE_SHAPES[0]
    rows, cols = gc.SHAPES[name][:2]
    fields = _fields(name, costs)
    starts, goals, fidx, (w_cells, w_heads, w_gears, w_count, w_status, w_cost) = gc.trace_case(name, costs)
    L, n = w_cells.shape[1], len(fields)
    cells, heads, gears, count, status, cost = _trace(fields[1:2].contiguous(), 1, n, rows, cols, costs, starts, goals, fidx, L)
    mine, refused = fidx == 1, w_status == 2
    assert refused[~mine].any() and (~refused[~mine]).any()
    assert np.array_equal(count[mine], w_count[mine]) and np.array_equal(cost[mine], w_cost[mine])
    assert np.array_equal(status[mine | refused], w_status[mine | refused])
    for p in np.flatnonzero(mine):
        assert np.array_equal(gears[p, :w_count[p]], w_gears[p, :w_count[p]])
    other = ~mine & ~refused
    assert (count[other] == SENT).all() and (status[other] == SENT).all() and (cost[other] == SENT).all()
    assert (cells[other] == SENT).all() and (heads[other] == SENT).all() and (gears[other] == SENT).all()


def test_a_walk_that_does_not_reach_the_goal_is_not_reported_as_a_path():
    """fields_dev is the caller's: on one that is no fixed point of the rule the descent can find no successor that fits.
    1 x 3, goal (0, 2, 0); the state (0, 1, 0, forward) is given (5, 0) where the rule has (1, 0).  From (0, 0, 0) the first move
    goes there, and no successor of it costs (5, 0): status 1, count 0, cost (-1, -1), not a truncated path with status 0."""
    field = np.full((1, 2, 8, 1, 3, 2), -1, np.int32)
    field[0, :, 0, 0, 2] = 0
    field[0, 0, 0, 0, 1] = (5, 0)
    starts = np.asarray([(0, 0, 0), (0, 1, 0), (0, 2, 0)], np.int32)
    goals = np.asarray([(0, 2, 0)] * 3, np.int32)
    _, _, _, count, status, cost = _trace(_dev(field, I32), 0, 1, 1, 3, (0, 0, 0), starts, goals, np.zeros(3, np.int32), 0)
    assert status.tolist() == [1, 0, 0] and count.tolist() == [0, 2, 1] and cost.tolist() == [[-1, -1], [1, 0], [0, 0]]


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
    rows, cols = gc.SHAPES[name][:2]
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
    for costs, mode in (((1, 2, 1), "fixed"), ((0, 0, 3), "free")):
        kw = dict(turn_cost=costs[0], reverse_cost=costs[1], cusp_cost=costs[2], goal_heading=mode)
        one = nfopp.lattice_gear_search_paths(lg, _dev(starts), _dev(goals), **kw)
        per_field = 16 * rows * cols * 8
        n_goals = len({tuple(v) for v in (g if mode == "fixed" else g[:, :2])})
        assert 7 <= n_goals <= 12
        three = nfopp.lattice_gear_search_paths(lg, _dev(starts), _dev(goals), max_field_bytes=per_field * ((n_goals + 2) // 3), **kw)
        for a, b in zip(one, three):
            assert a.dtype == I32 and torch.equal(a, b)
        cells, heads, gears, count, status, cost = [t.cpu().numpy() for t in one]
        gs = g.copy()
        if mode == "free":
            gs[:, 2] = -1
        ss = s.copy()
        ss[5, 1], gs[9, 0] = -2, rows + 3
        uniq = sorted({tuple(v) for v in gs})
        fields = np.stack([gr.gear_field(gc.layers_of(name), u, costs) for u in uniq])
        want = gr.search(fields, (rows, cols), ss, gs, [uniq.index(tuple(v)) for v in gs], costs)
        assert list(want[4][[5, 9]]) == [2, 2] and {0, 2} <= set(np.unique(want[4]))
        for got, w in zip((cells, heads, gears, count, status, cost), want):
            assert np.array_equal(got, w)


def test_the_torch_ops_equal_the_raw_calls():
    ops = torch_ops.load()
    name, costs = "20x23", (1, 0, 2)
    rows, cols = gc.SHAPES[name][:2]
    lg, goals = _lgrid(name), _dev(gc.goals_of(name), I32)
    fields = ops.lattice_gear_fields(lg.layers, goals, *costs)
    assert torch.equal(fields, _fields(name, costs))
    starts, gstates, fidx, _ = gc.trace_case(name, costs)
    raw = _trace(fields, 0, len(fields), rows, cols, costs, starts, gstates, fidx, 30)
    got = ops.lattice_gear_trace_paths(fields, 0, len(fields), _dev(starts, I32), _dev(gstates, I32), _dev(fidx, I32),
                                       costs[0], costs[1], costs[2], 30)
    for g, r in zip(got, raw):
        assert np.array_equal(np.where(r == SENT, 0, r), g.cpu().numpy())    # the op's buffers start as zeros
    cells, heads, _, count, status, _ = got
    rng = np.random.default_rng(4)
    sp, gp = _dev(_poses(starts, rng)), _dev(_poses(np.where(gstates < 0, 0, gstates), rng))
    count = torch.minimum(count, torch.tensor(30, dtype=I32, device="cuda"))
    want = nfopp.seed_lattice_trajectories(lg, cells, heads, count, status, sp, gp, 16)
    assert torch.equal(ops.lattice_seed_trajectories(cells, heads, count, status, sp, gp, 16, 0.0, 0.0, 1.0), want)
    with pytest.raises(RuntimeError, match="goal_states"):
        ops.lattice_gear_trace_paths(fields, 0, len(fields), _dev(starts, I32), _dev(gstates[:-1], I32), _dev(fidx, I32), 0, 0, 0, 30)
    with pytest.raises(RuntimeError, match="cusp_cost"):
        ops.lattice_gear_fields(lg.layers, goals, 0, 0, 256)
    with pytest.raises(RuntimeError, match="headings"):
        ops.lattice_seed_trajectories(cells, heads[:, :-1].contiguous(), count, status, sp, gp, 16, 0.0, 0.0, 1.0)


# ---- d. seeding ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seed_case(long):
    """Lattice paths with their poses.  Short: the traced paths of 64 problems on the 20 x 23 map (status 0 and 2 among
    them).  Long: the 1300-state serpentine twice (forward, and its cells reversed at the same headings: a reverse run) and a
    short row, so the kernel takes its workspace from global memory.  -> (lgrid, cells, heads, count, status, starts, goals)"""
    if not long:
        name, _, _, starts, goals = _python_case()
        lg = _lgrid(name)
        starts, goals = starts[:64].copy(), goals[:64].copy()
        goals[:, 2] += np.float32(2 * np.pi) * (np.arange(64) % 3 - 1)       # goal angles a turn off: the knots unwind them
        cells, heads, _, count, status, _ = [t.cpu().numpy() for t in nfopp.lattice_gear_search_paths(
            lg, _dev(starts), _dev(goals), turn_cost=1, reverse_cost=0, cusp_cost=2)]
        assert {0, 2} <= set(status)
        return lg, cells, heads, count, status, starts, goals
    sc, sh = gc.serpentine()
    n = len(sc)
    lg = _open_grid(int(sc[:, 0].max()) + 1, 40)
    cells, heads = np.zeros((3, n, 2), np.int32), np.zeros((3, n), np.int32)
    cells[0], heads[0] = sc, sh
    cells[1], heads[1] = sc[::-1], sh[::-1]
    cells[2, :5], heads[2, :5] = sc[:5], sh[:5]
    count, status = np.asarray([n, n, 5], np.int32), np.zeros(3, np.int32)
    rng = np.random.default_rng(8)
    ends = np.stack([cells[np.arange(3), 0], cells[np.arange(3), count - 1]], 1)          # [3, 2, 2] first and last cell
    poses = np.concatenate([ends[..., ::-1] + rng.uniform(0.3, 0.7, (3, 2, 2)), rng.uniform(-7, 7, (3, 2, 1))], 2).astype(np.float32)
    return lg, cells, heads, count, status, poses[:, 0].copy(), poses[:, 1].copy()


@pytest.mark.parametrize("long", (False, True), ids=("lds", "global workspace"))
def test_seeding_xy_is_the_grid_seeding_and_theta_the_restated_body_heading(long):
    lg, cells, heads, count, status, starts, goals = _seed_case(long)
    lib = _lib.load()
    assert (lib.nfopp_lattice_seed_workspace_bytes(len(cells), cells.shape[1]) > 0) == long
    d = [_dev(cells, I32), _dev(heads, I32), _dev(count, I32), _dev(status, I32), _dev(starts), _dev(goals)]
    line = None
    for n in ((1, 2, 7, 64) if not long else (7,)):
        traj = nfopp.seed_lattice_trajectories(lg, *d, n)
        assert traj.shape == (len(cells), n, 3) and traj.dtype == torch.float32
        assert torch.equal(traj, nfopp.seed_lattice_trajectories(lg, *d, n))
        xy = nfopp.seed_trajectories(lg, d[0], d[2], d[3], d[4], d[5], n, False)
        assert torch.equal(traj[..., :2], xy[..., :2])
        line = nfopp.init_trajectories(d[4], d[5], n, False)
        got = traj.cpu().numpy()
        for p in range(len(cells)):
            if status[p] != 0:
                assert torch.equal(traj[p], line[p])
                continue
            k = count[p]
            want = gr.seed_theta(cells[p, :k], heads[p, :k], starts[p], goals[p], lg.boundaries, lg.resolution, n)
            assert np.array_equal(got[p, :, 2].view(np.uint32), want.view(np.uint32)), (n, p, got[p, :, 2], want)
    # a count the buffers do not hold gets the straight line too
    bad = d[2].clone()
    bad[0] = cells.shape[1] + 1
    traj = nfopp.seed_lattice_trajectories(lg, d[0], d[1], bad, d[3], d[4], d[5], n)
    assert torch.equal(traj[0], line[0]) and torch.equal(traj[1:], nfopp.seed_lattice_trajectories(lg, *d, n)[1:])
    out = torch.empty(len(cells), n, 3, device="cuda")
    assert nfopp.seed_lattice_trajectories(lg, *d, n, out=out).data_ptr() == out.data_ptr()


# ---- e. the reversing corridor and the three-point turn ----------------------------------------------------------------------
def _path_stats(traj, starts, goals):
    lib = _lib.load()
    b, n, _ = traj.shape
    stats = torch.empty(b, _lib.NUM_PATH_STATS, dtype=torch.float64, device="cuda")
    _lib.check(lib.nfopp_path_stats(_lib.ptr(traj), _lib.ptr(starts), _lib.ptr(goals), b, n, 3, None, 0,
                                    float(np.cos(np.pi - np.pi / 3)), _lib.ptr(stats, torch.float64), None, _lib.stream_ptr()))
    return stats.cpu().numpy()


def test_the_reversing_corridor():
    lg = _open_grid(1, 6)
    starts, goals = _dev([[5.5, 0.5, 0.0]]), _dev([[0.5, 0.5, 0.0]])
    n = 12
    traj, status, changes = nfopp.lattice_gear_search_init(lg, starts, goals, n)
    cells, heads, gears, count, st, cost = [t.cpu().numpy() for t in nfopp.lattice_gear_search_paths(lg, starts, goals)]
    assert status.tolist() == [0] and st.tolist() == [0] and changes.tolist() == [0] and changes.dtype == I32
    assert count[0] == 6 and (gears[0] == 1).all() and (heads[0] == 0).all() and tuple(cost[0]) == (5, 0)
    assert cells[0].tolist() == [[0, c] for c in range(5, -1, -1)]
    t = traj.cpu().numpy()[0]
    assert (t[:, 2] == 0).all()                                              # the body keeps facing east
    path = np.concatenate([[[5.5, 0.5, 0.0]], t, [[0.5, 0.5, 0.0]]]).astype(np.float64)
    assert (np.diff(path[:, 0]) < 0).all()                                   # x strictly decreasing
    # the sign nfopp_path_stats forms: s_i = cos(theta_i) * ex_i + sin(theta_i) * ey_i, negative throughout = one reverse run
    e = np.diff(path[:, :2], axis=0)
    s = np.cos(path[:-1, 2]) * e[:, 0] + np.sin(path[:-1, 2]) * e[:, 1]
    assert (s < 0).all()
    assert _path_stats(traj, starts, goals)[0, nfopp.PATH_STAT_REVERSALS] == 0
    # the forward-only search has no seed here, and its seeding would turn the body round
    _, old_status = nfopp.lattice_search_init(lg, starts, goals, n)
    assert old_status.tolist() == [1]
    turned = nfopp.seed_trajectories(lg, _dev(cells, I32), _dev(count, I32), _dev(st, I32), starts, goals, n, True).cpu().numpy()[0]
    assert np.array_equal(turned[:, :2], t[:, :2])
    assert abs(turned[n // 2, 2]) > 3.0 and not np.array_equal(turned[:, 2], t[:, 2])   # mid-path: towards pi, not 0


def test_the_three_point_turn_through_the_batch_planner():
    import gpu_common
    import grid_search_ref as gsr
    z = np.load(gsr.GOLDEN.replace("g19_astar_init", "g1_onf"), allow_pickle=False)
    onf, _ = gpu_common.make_onf(z["a_cfg"], z["a_params"])
    lg = _open_grid(3, 7)
    costs = (0, 1, 3)
    states = np.asarray([(0, c, 4) for c in range(7)])
    starts = np.stack([states[:, 1] + 0.5, states[:, 0] + 0.5, np.full(7, np.pi)], 1).astype(np.float32)
    goals = np.asarray([[6.5, 0.5, 0.0]] * 7, np.float32)
    bounds = (0.0, 7.0, 0.0, 3.0)
    bp = nfopp.BatchPlanner(onf, 7, 32, nfopp.TrajectoryHyper(), init_angles_with_trajectory=True)
    bp.init(starts, goals, bounds, initializer=nfopp.GearLattice(lg, reverse_cost=costs[1], cusp_cost=costs[2]))
    field = gr.gear_field(np.zeros((1, 3, 7), np.uint8), (0, 6, 0), costs)
    want = [gr.trace_path(field, s, costs) for s in states]
    assert bp.seed_status.tolist() == [0] * 7 and bp.seed_margin is None
    assert bp.seed_gear_changes.tolist() == [gr.gear_changes(w[2], len(w[2])) for w in want]
    assert bp.seed_gear_changes.dtype == I32 and min(bp.seed_gear_changes.tolist()) >= 1
    traj, status, changes = nfopp.lattice_gear_search_init(lg, _dev(starts), _dev(goals), 32, reverse_cost=costs[1], cusp_cost=costs[2])
    assert torch.equal(bp.engine.traj.view(traj.shape), traj) and torch.equal(status, bp.seed_status) and torch.equal(changes, bp.seed_gear_changes)
    assert (bp.path_stats().cpu().numpy()[:, nfopp.PATH_STAT_REVERSALS] >= 1).all()
    cost = nfopp.lattice_gear_search_paths(lg, _dev(starts), _dev(goals), *costs)[5].cpu().numpy()
    assert [tuple(c) for c in cost] == [w[3] for w in want] == [p for _, p in gc.HAND[7][4]]
    # the forward-only lattice has no seed for any of them; a plain LatticeGrid keeps its own route through init
    bp.init(starts, goals, bounds, initializer=lg)
    assert bp.seed_status.tolist() == [1] * 7 and bp.seed_gear_changes is None
    gl = nfopp.GearLattice(lg)
    for kw in (dict(initializer=gl, seed_clearance=0.5), dict(initializer=gl, seed_any_angle=True)):
        with pytest.raises(ValueError, match="do not go with a LatticeGrid"):
            bp.init(starts, goals, bounds, **kw)
    bp.init(starts, goals, bounds, initializer=gl, seed_turn_cost=2)
    assert torch.equal(bp.seed_status, nfopp.lattice_gear_search_init(lg, _dev(starts), _dev(goals), 32, turn_cost=2)[1])
    onf2 = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=False).to("cuda")
    bp2 = nfopp.BatchPlanner(onf2, 4, 16, nfopp.TrajectoryHyper())
    with pytest.raises(ValueError, match="D = 3"):
        bp2.init(starts[:4, :2], goals[:4, :2], bounds, initializer=gl)


# ---- f. extents --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,costs", [("20x23", (1, 0, 2)), ("7x65", (0, 0, 255))], ids=("lds", "wide"))
def test_the_entries_write_their_stated_extents_and_nothing_else(name, costs):
    lib = _lib.load()
    rows, cols = gc.SHAPES[name][:2]
    lg = _lgrid(name)
    goals_np = gc.goals_of(name)
    G = len(goals_np)
    starts_np, gstates_np, fidx_np = gc.trace_problems(name, max_goals=2)
    starts_np, gstates_np, fidx_np = starts_np[::3], gstates_np[::3], fidx_np[::3]
    B = len(starts_np)
    rng = np.random.default_rng(6)
    sp_np, gp_np = _poses(starts_np, rng), _poses(np.where(gstates_np < 0, 0, gstates_np), rng)
    results = []
    for fill in (0x00, 0xFF):
        layers, p_layers = gd.from_array(lg.layers_host, "cuda")
        goals, p_goals = gd.from_array(goals_np, "cuda")
        consts = [p_layers, p_goals]
        snaps = [gd.snapshot(p) for p in consts]
        fields, p_fields = gd.guarded((G, 2, 8, rows, cols, 2), I32, "cuda", fill)
        ws_bytes = lib.nfopp_lattice_gear_fields_workspace_bytes(rows, cols, costs[0], costs[1], costs[2], G)
        assert (ws_bytes > 0) == ((name, costs) in gc.WIDE)
        ws, p_ws = gd.guarded((max(ws_bytes, 8),), torch.uint8, "cuda", fill)
        _lib.check(lib.nfopp_lattice_gear_distance_fields(
            _lib.ptr(layers, torch.uint8), lg.n_layers, rows, cols, _lib.ptr(goals, I32), G, costs[0], costs[1], costs[2],
            _lib.ptr(fields, I32), _lib.ptr(ws, torch.uint8) if ws_bytes else None, ws_bytes, _lib.stream_ptr()))
        assert np.array_equal(fields.cpu().numpy(), gc.fields_of(name, costs))
        # the trace: sizing pass, then the paths
        ins = [gd.from_array(a, "cuda") for a in (starts_np, gstates_np, fidx_np)]
        consts += [p for _, p in ins] + [p_fields]
        snaps += [gd.snapshot(p) for p in consts[2:]]
        count, p_count = gd.guarded((B,), I32, "cuda", fill)
        status, p_status = gd.guarded((B,), I32, "cuda", fill)
        cost, p_cost = gd.guarded((B, 2), I32, "cuda", fill)

        def trace(max_len, cells, heads, gears):
            _lib.check(lib.nfopp_lattice_gear_trace_paths(
                _lib.ptr(fields, I32), 0, G, G, rows, cols, costs[0], costs[1], costs[2], _lib.ptr(ins[0][0], I32),
                _lib.ptr(ins[1][0], I32), _lib.ptr(ins[2][0], I32), B, max_len, _lib.ptr(cells, I32) if max_len else None,
                _lib.ptr(heads, I32) if max_len else None, _lib.ptr(gears, I32) if max_len else None, _lib.ptr(count, I32),
                _lib.ptr(status, I32), _lib.ptr(cost, I32), _lib.stream_ptr()))

        trace(0, None, None, None)
        L = int(count.max())
        cells, p_cells = gd.guarded((B, L, 2), I32, "cuda", fill)
        heads, p_heads = gd.guarded((B, L), I32, "cuda", fill)
        gears, p_gears = gd.guarded((B, L), I32, "cuda", fill)
        trace(L, cells, heads, gears)
        k = torch.arange(L, device="cuda")[None, :] < (count * (status == 0))[:, None]
        filled = torch.full_like(heads, -1 if fill else 0)
        for t in (cells[..., 0], cells[..., 1], heads, gears):
            assert torch.equal(torch.where(k, filled, t), filled), "an entry behind a path was written"
        # the seeding: every element of traj, nothing of the inputs
        sp, p_sp = gd.from_array(sp_np, "cuda")
        gp, p_gp = gd.from_array(gp_np, "cuda")
        consts += [p_sp, p_gp, p_cells, p_heads, p_gears, p_count, p_status]
        snaps += [gd.snapshot(p) for p in consts[-7:]]
        traj, p_traj = gd.guarded((B, 16, 3), torch.float32, "cuda", fill)
        assert lib.nfopp_lattice_seed_workspace_bytes(B, L) == 0
        _lib.check(lib.nfopp_lattice_seed_trajectories(
            _lib.ptr(cells, I32), _lib.ptr(heads, I32), _lib.ptr(count, I32), _lib.ptr(status, I32), B, L, _lib.ptr(sp), _lib.ptr(gp),
            16, 0.0, 0.0, 1.0, _lib.ptr(traj), None, 0, _lib.stream_ptr()))
        assert bool(torch.isfinite(traj).all())
        for p in (p_fields, p_ws, p_count, p_status, p_cost, p_cells, p_heads, p_gears, p_traj):
            assert gd.guards_intact(p)
        for p, snap in zip(consts, snaps):
            assert gd.unchanged(p, snap), "an input was written"
        m = k.cpu().numpy()
        results.append([gd.bits(fields), gd.bits(count), gd.bits(status), gd.bits(cost), gd.bits(traj)] +
                       [np.where(m, gd.bits(t), 0) for t in (cells[..., 0], cells[..., 1], heads, gears)])
    for a, b in zip(*results):
        assert np.array_equal(a, b), "a result depends on what the buffers held"
    assert {0, 1} <= set(results[0][2].tolist())


def test_the_seeding_entry_with_a_global_workspace_writes_its_stated_extents_and_nothing_else():
    lib = _lib.load()
    lg, cells_np, heads_np, count_np, status_np, starts_np, goals_np = _seed_case(True)
    B, L, n = len(cells_np), cells_np.shape[1], 9
    ws_bytes = lib.nfopp_lattice_seed_workspace_bytes(B, L)
    assert ws_bytes == (7 * (L + 2) + 3) * 8 * B > 0
    want = nfopp.seed_lattice_trajectories(lg, _dev(cells_np, I32), _dev(heads_np, I32), _dev(count_np, I32), _dev(status_np, I32),
                                           _dev(starts_np), _dev(goals_np), n)
    for fill in (0x00, 0xFF):
        ins = [gd.from_array(a, "cuda") for a in (cells_np, heads_np, count_np, status_np, starts_np, goals_np)]
        snaps = [gd.snapshot(p) for _, p in ins]
        traj, p_traj = gd.guarded((B, n, 3), torch.float32, "cuda", fill)
        ws, p_ws = gd.guarded((ws_bytes,), torch.uint8, "cuda", fill)
        _lib.check(lib.nfopp_lattice_seed_trajectories(
            _lib.ptr(ins[0][0], I32), _lib.ptr(ins[1][0], I32), _lib.ptr(ins[2][0], I32), _lib.ptr(ins[3][0], I32), B, L,
            _lib.ptr(ins[4][0]), _lib.ptr(ins[5][0]), n, lg.boundaries[0], lg.boundaries[2], lg.resolution, _lib.ptr(traj),
            _lib.ptr(ws, torch.uint8), ws_bytes, _lib.stream_ptr()))
        assert gd.guards_intact(p_traj) and gd.guards_intact(p_ws)
        for (_, p), snap in zip(ins, snaps):
            assert gd.unchanged(p, snap), "an input was written"
        assert np.array_equal(gd.bits(traj), gd.bits(want)), "the result depends on what the buffers held"

