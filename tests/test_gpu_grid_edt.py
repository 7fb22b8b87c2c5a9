"""GPU: the exact distance transform of an occupancy grid (csrc/grid_edt.hip), OccupancyGrid's distance_transform /
clearance_field / inflated, and grid-search seeding with a clearance margin (nfopp/grid_search.py), against the CPU
restatement of tests/edt_ref.py.  Everything is integer (or selected by integers): every comparison is `==`.

planner.seed_margin: None when no grid seeding ran, all zero when it ran without a clearance (the choice this file pins).

m4 problem 6 starts next to its goal; with the start cell untested and the goal cell forced free its search succeeds on any
image, so on the all-wall inflated m4 it alone is seeded "at the margin" -- along the very cells of the plain grid
(tests/test_grid_edt_cpu.py asserts this about the fixture).  m3 and m4 therefore equal the plain call bit for bit in
everything but that one seed_margin entry, which is held against the restatement."""
import numpy as np
import pytest
import torch

import nfopp
from nfopp import _lib

import edt_ref as er
import grid_search_ref as gsr

pytestmark = pytest.mark.gpu
FX = gsr.load_fixture()
I32 = torch.int32
M2_CELLS2 = 4   # as in tests/test_grid_edt_cpu.py
PAD, CANARY = 64, -7


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _grid(m):
    return nfopp.OccupancyGrid(m["occ"], m["boundaries"], m["resolution"], device="cuda")


def _run(occ_dev, rows, cols, border, want_nearest=True):
    """nfopp_grid_edt through ctypes -> (status, dist2, nearest or None); the outputs carry a tail that must stay untouched."""
    lib = _lib.load()
    n = rows * cols
    dist2 = torch.full((n + PAD,), CANARY, dtype=I32, device="cuda")
    nearest = torch.full((n + PAD,), CANARY, dtype=I32, device="cuda") if want_nearest else None
    ws_bytes = lib.nfopp_grid_edt_workspace_bytes(rows, cols)
    ws = torch.full((ws_bytes // 4 + PAD,), CANARY, dtype=I32, device="cuda")
    rc = lib.nfopp_grid_edt(_lib.ptr(occ_dev, torch.uint8), rows, cols, int(border), _lib.ptr(dist2, I32),
                            _lib.ptr(nearest, I32) if want_nearest else None, _lib.ptr(ws, I32), ws_bytes, _lib.stream_ptr())
    if rc != 0:
        return rc, None, None
    for buf in (dist2, nearest, ws):
        if buf is not None:
            assert bool((buf[-PAD:] == CANARY).all()), "wrote past the end"
    return rc, dist2[:n].cpu().numpy().reshape(rows, cols), nearest[:n].cpu().numpy().reshape(rows, cols) if want_nearest else None


def _check(occ, what):
    occ = np.ascontiguousarray(occ, np.uint8)
    rows, cols = occ.shape
    occ_dev = _dev(occ, torch.uint8)
    want_d, want_n = er.edt(occ)
    for border in (False, True):
        rc, d, n = _run(occ_dev, rows, cols, border)
        assert rc == 0, (what, _lib.load().nfopp_last_error())
        assert d.dtype == np.int32 and np.array_equal(d, er.with_border(want_d, border)), (what, border)
        assert np.array_equal(n, want_n), (what, border)
        _, d2, n2 = _run(occ_dev, rows, cols, border)
        assert d2.tobytes() == d.tobytes() and n2.tobytes() == n.tobytes(), (what, border)      # a second run: the same bytes
        _, d3, _ = _run(occ_dev, rows, cols, border, want_nearest=False)
        assert d3.tobytes() == d.tobytes(), (what, border)                                      # nearest is optional
        if not border:
            if occ.any():
                nr, nc = np.divmod(n.astype(np.int64), cols)
                r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
                assert np.array_equal(d, (r - nr) ** 2 + (c - nc) ** 2), what
                assert (occ[nr, nc] != 0).all(), what
            else:
                assert (d == np.iinfo(np.int32).max).all() and (n == -1).all(), what


def _fills(rows, cols, seed):
    rng = np.random.default_rng(seed)
    yield "empty", np.zeros((rows, cols), np.uint8)
    yield "full", np.ones((rows, cols), np.uint8)
    for r, c in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)):
        one = np.zeros((rows, cols), np.uint8)
        one[r, c] = 1
        yield "corner (%d, %d)" % (r, c), one
    yield "checkerboard", ((np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2).astype(np.uint8)
    yield "5 %", (rng.random((rows, cols)) < 0.05).astype(np.uint8)
    yield "50 %", (rng.random((rows, cols)) < 0.5).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (64, 64), (257, 3), (3, 257), (300, 513)])
def test_edt_equals_the_restatement(shape):
    for name, occ in _fills(shape[0], shape[1], seed=shape[0] * 10007 + shape[1]):
        _check(occ, "%s %s" % (shape, name))


@pytest.mark.parametrize("shape", [(1, 4096), (4096, 1)])
def test_edt_at_the_largest_side(shape):
    rng = np.random.default_rng(4096)
    _check((rng.random(shape) < 0.05).astype(np.uint8), "%s 5 %%" % (shape,))
    one = np.zeros(shape, np.uint8)
    one.reshape(-1)[4095] = 1
    _check(one, "%s last cell" % (shape,))


def test_edt_rejects_a_side_of_4097():
    occ = torch.zeros(4097, dtype=torch.uint8, device="cuda")
    for rows, cols in ((1, 4097), (4097, 1)):
        assert _lib.load().nfopp_grid_edt_workspace_bytes(rows, cols) == 0
        out = torch.full((4097,), CANARY, dtype=I32, device="cuda")
        rc = _lib.load().nfopp_grid_edt(_lib.ptr(occ, torch.uint8), rows, cols, 0, _lib.ptr(out, I32), None, _lib.ptr(out, I32),
                                        4 * 4097, _lib.stream_ptr())
        assert rc == -1 and b"4096" in _lib.load().nfopp_last_error()
        assert bool((out == CANARY).all())


def test_edt_long_scans_on_a_sparse_grid():
    rng = np.random.default_rng(1030)
    occ = (rng.random((257, 1030)) < 0.001).astype(np.uint8)
    assert 100 < occ.sum() < 1030 and (occ.sum(0) == 0).sum() > 700      # most columns are empty: scans cross many of them
    _check(occ, "257 x 1030 at 0.1 %")


@pytest.mark.parametrize("name", ["g16", "m1", "m2", "m3", "m4"])
def test_edt_on_the_committed_maps(name):
    if name == "g16":
        occ = np.load(gsr.GOLDEN.replace("g19_astar_init", "g16_grid_checker"), allow_pickle=False)["grid"]
    else:
        occ = FX[name + "_occupancy"]
    _check(np.asarray(occ) != 0, name)


# ---- OccupancyGrid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_inflated_clearance_field_and_cache(k):
    m = gsr.fixture_map(FX, k)
    grid = _grid(m)
    assert torch.equal(grid.inflated(cells2=0).occupancy, grid.occupancy)
    assert torch.equal(grid.inflated(0.0).occupancy, grid.occupancy)
    for border in (False, True):
        want_d, want_n = er.edt(m["occ"], border)
        d, n = grid.distance_transform(border)
        assert d.dtype == I32 and n.dtype == I32 and d.is_cuda
        assert np.array_equal(d.cpu().numpy(), want_d) and np.array_equal(n.cpu().numpy(), want_n)
        again = grid.distance_transform(border)
        assert again[0] is d and again[1] is n                                    # computed once per border value
        for c2 in (1, 2, 4, 8):
            inf = grid.inflated(cells2=c2, border=border)
            assert inf.boundaries == grid.boundaries and inf.resolution == grid.resolution and inf.shape == grid.shape
            assert inf.occupancy.dtype == torch.uint8
            assert np.array_equal(inf.occupancy.cpu().numpy(), er.inflate(m["occ"], c2, border)), (k, border, c2)
            assert np.array_equal(inf.occupancy_host, er.inflate(m["occ"], c2, border))         # the lazy host copy
            assert grid.inflated(cells2=c2, border=border) is inf
        assert torch.equal(grid.inflated(2 * grid.resolution, border=border).occupancy, grid.inflated(cells2=4, border=border).occupancy)
        field = grid.clearance_field(border)
        want = (m["resolution"] * np.sqrt(want_d.astype(np.float64))).astype(np.float32)
        assert field.dtype == torch.float32 and np.array_equal(field.cpu().numpy(), want)


def test_clearance_field_of_an_empty_grid():
    grid = nfopp.OccupancyGrid(np.zeros((5, 9), np.uint8), (0.0, 9.0, 0.0, 5.0), 0.5, device="cuda")
    assert bool(torch.isinf(grid.clearance_field()).all()) and bool((grid.clearance_field() > 0).all())
    assert bool((grid.distance_transform()[1] == -1).all())
    assert not bool(grid.inflated(cells2=1000).occupancy.any())
    want = 0.5 * np.sqrt(er.with_border(np.full((5, 9), er.NONE, np.int64)).astype(np.float64))
    assert np.array_equal(grid.clearance_field(border=True).cpu().numpy(), want.astype(np.float32))
    assert bool(grid.inflated(cells2=1, border=True).occupancy[0].all())


# ---- seeding with a margin -----------------------------------------------------------------------------------------------
def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same_paths(cells_a, counts_a, cells_b, counts_b, rows):
    assert np.array_equal(counts_a[rows], counts_b[rows])
    for i in rows:
        assert np.array_equal(cells_a[i, :counts_a[i]], cells_b[i, :counts_b[i]]), i


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_no_margin_is_todays_seeding_bit_for_bit(k):
    m = gsr.fixture_map(FX, k)
    grid = _grid(m)
    starts, goals = _dev(m["starts"]), _dev(m["goals"])
    for directed in (False, True):
        traj, status = nfopp.grid_search_init(grid, starts, goals, 100, directed)
        got = nfopp.grid_search_init(grid, starts, goals, 100, directed, clearance=None)
        assert len(got) == 2 and torch.equal(got[0], traj) and torch.equal(got[1], status)
        for clearance in (0.0, (), [], [0.0]):
            got = nfopp.grid_search_init(grid, starts, goals, 100, directed, clearance=clearance)
            assert len(got) == 3 and torch.equal(got[0], traj) and torch.equal(got[1], status)
            assert got[2].dtype == torch.float32 and got[2].shape == (len(m["starts"]),) and not bool(got[2].any())
    plain = nfopp.grid_search_paths(grid, starts, goals)
    assert len(plain) == 4 and len(nfopp.grid_search_paths(grid, starts, goals, clearance=None)) == 4
    for clearance in (0.0, ()):
        got = nfopp.grid_search_paths(grid, starts, goals, clearance=clearance)
        assert len(got) == 5 and all(torch.equal(a, b) for a, b in zip(got[:4], plain)) and not bool(got[4].any())


def test_margin_of_one_cell_on_the_corridor_map():
    m = gsr.fixture_map(FX, 1)
    grid = _grid(m)
    res = m["resolution"]
    assert nfopp.margin_cells2(res, res) == 1
    starts, goals = _dev(m["starts"]), _dev(m["goals"])
    p_cells, p_counts, p_status, p_costs = _np(nfopp.grid_search_paths(grid, starts, goals))
    cells, counts, status, costs, margin = _np(nfopp.grid_search_paths(grid, starts, goals, clearance=res))
    want = er.seed_levels(m["occ"], m["start_cells"], m["goal_cells"], [1]) == 0
    assert np.array_equal(margin > 0, want) and int((margin > 0).sum()) == int(want.sum()) >= 24
    assert np.array_equal(margin[want], np.full(int(want.sum()), res, np.float32))
    dist2 = er.edt(m["occ"])[0]
    for i in np.flatnonzero(margin > 0):
        assert status[i] == 0
        path = cells[i, :counts[i]]
        assert gsr.path_cost(path) == tuple(costs[i])
        assert tuple(path[0]) == tuple(m["start_cells"][i]) and tuple(path[-1]) == tuple(m["goal_cells"][i])
        own = (path == m["start_cells"][i]).all(1) | (path == m["goal_cells"][i]).all(1)
        assert (dist2[path[~own, 0], path[~own, 1]] > 1).all(), i                  # off the walls by more than one cell
        assert not gsr.Cost(tuple(int(v) for v in costs[i])) < gsr.Cost(tuple(int(v) for v in p_costs[i])), i
    back = np.flatnonzero(margin == 0)
    _same_paths(cells, counts, p_cells, p_counts, back)
    assert np.array_equal(status[back], p_status[back]) and np.array_equal(costs[back], p_costs[back])
    for directed in (False, True):
        p_traj = nfopp.grid_search_init(grid, starts, goals, 100, directed)[0].cpu().numpy()
        traj, st, mg = _np(nfopp.grid_search_init(grid, starts, goals, 100, directed, clearance=res))
        assert np.array_equal(mg, margin) and np.array_equal(st, status)
        assert np.array_equal(traj[back], p_traj[back])
        # the trajectory of the merged cells is the seeding stage on exactly those cells
        alone = nfopp.seed_trajectories(grid, _dev(cells, I32), _dev(counts, I32), _dev(status, I32), starts, goals, 100, directed)
        assert np.array_equal(traj, alone.cpu().numpy())
        assert not np.array_equal(traj, p_traj)


@pytest.mark.parametrize("k", [3, 4])
def test_one_cell_corridors_fall_back(k):
    m = gsr.fixture_map(FX, k)
    grid = _grid(m)
    res = m["resolution"]
    assert bool(grid.inflated(res).occupancy.all())
    starts, goals = _dev(m["starts"]), _dev(m["goals"])
    want = er.seed_levels(m["occ"], m["start_cells"], m["goal_cells"], [1]) == 0       # m4 problem 6 only (module docstring)
    plain = _np(nfopp.grid_search_paths(grid, starts, goals))
    for clearance in (res, [2 * res, res]):
        got = _np(nfopp.grid_search_paths(grid, starts, goals, clearance=clearance))
        _same_paths(got[0], got[1], plain[0], plain[1], range(len(want)))
        assert np.array_equal(got[2], plain[2]) and np.array_equal(got[3], plain[3])
        largest = np.max(clearance)          # a path that exists on the all-wall image exists at every margin
        assert np.array_equal(got[4], np.where(want, largest, 0.0).astype(np.float32))
        for directed in (False, True):
            traj, status = nfopp.grid_search_init(grid, starts, goals, 100, directed)
            g_traj, g_status, g_margin = nfopp.grid_search_init(grid, starts, goals, 100, directed, clearance=clearance)
            assert torch.equal(g_traj, traj) and torch.equal(g_status, status)
            assert np.array_equal(g_margin.cpu().numpy(), got[4])


@pytest.mark.parametrize("levels", [[M2_CELLS2], [4, 1]])
def test_mixed_map_takes_the_largest_reachable_margin(levels):
    m = gsr.fixture_map(FX, 2)
    grid = _grid(m)
    res = m["resolution"]
    margins = [float(np.sqrt(c2)) * res for c2 in levels]
    assert [nfopp.margin_cells2(mg, res) for mg in margins] == levels
    starts, goals = _dev(m["starts"]), _dev(m["goals"])
    want = er.seed_levels(m["occ"], m["start_cells"], m["goal_cells"], levels)
    assert all((want == lv).sum() >= 4 for lv in ([-1, 0] if len(levels) == 1 else [0, 1]))
    clearance = margins[0] if len(levels) == 1 else margins
    cells, counts, status, costs, margin = _np(nfopp.grid_search_paths(grid, starts, goals, clearance=clearance))
    want_margin = np.where(want >= 0, np.asarray(margins, np.float32)[np.maximum(want, 0)], np.float32(0))
    assert margin.dtype == np.float32 and np.array_equal(margin, want_margin)
    for lv in [-1] + list(range(len(levels))):
        rows = np.flatnonzero(want == lv)
        level_grid = grid if lv < 0 else grid.inflated(margins[lv])
        l_cells, l_counts, l_status, l_costs = _np(nfopp.grid_search_paths(level_grid, starts, goals))
        _same_paths(cells, counts, l_cells, l_counts, rows)
        assert np.array_equal(status[rows], l_status[rows]) and np.array_equal(costs[rows], l_costs[rows])
        if lv >= 0:
            assert (l_status[rows] == 0).all()
            occ = er.inflate(m["occ"], levels[lv])
            for i in rows:
                free_goal = occ.copy()
                free_goal[tuple(m["goal_cells"][i])] = 0
                assert gsr.check_path(free_goal, cells[i, :counts[i]], m["start_cells"][i], m["goal_cells"][i]) == tuple(costs[i])
    traj, st, mg = nfopp.grid_search_init(grid, starts, goals, 100, True, clearance=clearance)
    alone = nfopp.seed_trajectories(grid, _dev(cells, I32), _dev(counts, I32), _dev(status, I32), starts, goals, 100, True)
    assert torch.equal(traj, alone) and np.array_equal(mg.cpu().numpy(), margin) and np.array_equal(st.cpu().numpy(), status)


def _host_checker(m):
    """A host checker that reads the fixture's occupancy (cell = floor((x - b0) / resolution))."""
    class Checker(object):
        def get_boundaries(self):
            return m["boundaries"]

        def check_collision(self, positions):
            rc = gsr.cells_of(np.stack([np.asarray(positions.x), np.asarray(positions.y)], 1), m["boundaries"], m["resolution"])
            ok = (rc >= 0).all(1) & (rc[:, 0] < m["occ"].shape[0]) & (rc[:, 1] < m["occ"].shape[1])
            out = np.ones(len(rc), bool)
            out[ok] = m["occ"][rc[ok, 0], rc[ok, 1]] != 0
            return out
    return Checker()


def test_initializer_and_batch_planner_pass_the_margin_on():
    import gpu_common as gc
    m = gsr.fixture_map(FX, 1)
    grid = _grid(m)
    res = m["resolution"]
    B, N = 8, 32
    z = np.load(gsr.GOLDEN.replace("g19_astar_init", "g1_onf"), allow_pickle=False)
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    starts, goals = m["starts"][:B], m["goals"][:B]
    for directed in (False, True):
        plain, p_status = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), N, directed)
        want, w_status, w_margin = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), N, directed, clearance=res)
        assert bool((w_margin > 0).any()) and not torch.equal(want, plain)
        ini = nfopp.AstarTrajectoryInitializer(_host_checker(m), res, directed, clearance=res)
        assert ini.seed_margin is None
        got = ini.initialize_batch(_dev(starts), _dev(goals), N)
        assert torch.equal(got, want) and torch.equal(ini.status, w_status) and torch.equal(ini.seed_margin, w_margin)
        bp = nfopp.BatchPlanner(onf, B, N, nfopp.TrajectoryHyper(), init_angles_with_trajectory=directed)
        bp.init(starts, goals, m["boundaries"])
        assert bp.seed_status is None and bp.seed_margin is None                   # no grid seeding ran
        bp.init(starts, goals, m["boundaries"], initializer=ini)
        assert torch.equal(bp.engine.traj, want) and torch.equal(bp.seed_status, w_status) and torch.equal(bp.seed_margin, w_margin)
        bp.init(starts, goals, m["boundaries"], initializer=grid, seed_clearance=res)
        assert torch.equal(bp.engine.traj, want) and torch.equal(bp.seed_status, w_status) and torch.equal(bp.seed_margin, w_margin)
        bp.init(starts, goals, m["boundaries"], initializer=grid, seed_clearance=[2 * res, res])
        pair = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), N, directed, clearance=[2 * res, res])
        assert torch.equal(bp.engine.traj, pair[0]) and torch.equal(bp.seed_margin, pair[2])
        # without the argument: as today, and a margin of zero everywhere
        for initializer in (grid, nfopp.AstarTrajectoryInitializer(_host_checker(m), res, directed)):
            bp.init(starts, goals, m["boundaries"], initializer=initializer)
            assert torch.equal(bp.engine.traj, plain) and torch.equal(bp.seed_status, p_status)
            assert bp.seed_margin.shape == (B,) and not bool(bp.seed_margin.any())
        with pytest.raises(ValueError):
            bp.init(starts, goals, m["boundaries"], initializer=ini, seed_clearance=res)
        with pytest.raises(ValueError):
            bp.init(starts, goals, m["boundaries"], seed_clearance=res)
