"""GPU: the grid-search (A*) seeder (csrc/grid_search.hip, nfopp/grid_search.py) against the reference's results in
tests/golden/g19_astar_init.npz and the exact integer-pair Dijkstra of tests/grid_search_ref.py.

Gates.  Costs and fields are integers: `==`.  Seeded xy, fed the reference's own cell paths: the reference's spread
between its fp32 arithmetic and the same computation in float64 (`reparam_noise`, stored per problem by the generator)
plus one fp32 ulp of the coordinate for the final cast.  Undirected headings: bit-identical (torch.linspace's rounding, as
test_gpu_path_tools.py pins init_trajectories).  Directed headings: 1e-6 (atan2f rounding, same file)."""
import time

import numpy as np
import pytest
import torch

import nfopp

import grid_search_ref as gsr

pytestmark = pytest.mark.gpu
F32 = np.float32
FX = gsr.load_fixture()


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _grid(m):
    return nfopp.OccupancyGrid(m["occ"], m["boundaries"], m["resolution"], device="cuda")


def _padded(paths):
    cells = np.zeros((len(paths), max(len(p) for p in paths), 2), np.int32)
    for i, p in enumerate(paths):
        cells[i, :len(p)] = p
    return cells, np.asarray([len(p) for p in paths], np.int32)


def _check_traj(got, m, n, directed, rows=None, what=""):
    """got [B, n, 3] against the reference's trajectories of fixture map m."""
    want = m["traj"][(n, int(directed))]
    rows = range(len(want)) if rows is None else rows
    for j, i in enumerate(rows):
        bound = m["noise"][n][i] + np.spacing(np.abs(want[i][:, :2]).astype(F32)).astype(np.float64)
        err = np.abs(got[j][:, :2].astype(np.float64) - want[i][:, :2].astype(np.float64))
        print("%s problem %d N=%d dir=%d: max xy err %.3e, noise %.3e, worst err/bound %.3f" % (
            what, i, n, directed, err.max(), m["noise"][n][i], (err / bound).max()))
        assert (err <= bound).all(), (what, i, n, float(err.max()), float(m["noise"][n][i]))
        if directed:
            assert np.abs(got[j][:, 2].astype(np.float64) - want[i][:, 2]).max() < 1e-6
        else:
            assert np.array_equal(got[j][:, 2], want[i][:, 2]), (what, i, n)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_fields_equal_exact_dijkstra_and_repeat_bit_for_bit(k):
    m = gsr.fixture_map(FX, k)
    grid = _grid(m)
    goals = np.concatenate([m["goal_cells"][:6], m["goal_cells"][:3], m["start_cells"][:2]]).astype(np.int32)  # with duplicates
    if k == 4:
        goals = np.concatenate([goals, FX["m4_walled_cell"][None]]).astype(np.int32)
    a = nfopp.distance_fields(grid, _dev(goals, torch.int32)).cpu().numpy()
    b = nfopp.distance_fields(grid, _dev(goals, torch.int32)).cpu().numpy()
    assert np.array_equal(a, b)
    for j, g in enumerate(goals):
        want = gsr.dijkstra_field(m["occ"], g)
        assert np.array_equal(a[j], want), (k, j, int((a[j] != want).any(-1).sum()))
    assert (a[0][m["occ"] != 0][:, 0] <= 0).all()       # walls hold the sentinel (or are the forced-free goal)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_paths_are_valid_and_optimal(k):
    m = gsr.fixture_map(FX, k)
    cells, counts, status, costs = [t.cpu().numpy() for t in nfopp.grid_search_paths(_grid(m), _dev(m["starts"]), _dev(m["goals"]))]
    assert (status == 0).all()
    assert np.array_equal(costs, m["cost"])
    for i in range(len(counts)):
        occ = m["occ"].copy()
        occ[tuple(m["goal_cells"][i])] = 0
        path = cells[i, :counts[i]]
        assert gsr.check_path(occ, path, m["start_cells"][i], m["goal_cells"][i]) == tuple(m["cost"][i])
        if k >= 3:
            assert np.array_equal(path, m["paths"][i]), i


@pytest.mark.parametrize("k", [1, 2])
def test_seeding_stage_on_the_reference_paths(k):
    m = gsr.fixture_map(FX, k)
    grid = _grid(m)
    cells, counts = _padded(m["paths"])
    status = np.zeros(len(counts), np.int32)
    for n in (100, 256):
        for directed in (False, True):
            got = nfopp.seed_trajectories(grid, _dev(cells, torch.int32), _dev(counts, torch.int32), _dev(status, torch.int32),
                                          _dev(m["starts"]), _dev(m["goals"]), n, directed).cpu().numpy()
            _check_traj(got, m, n, directed, what="map %d seed stage" % k)


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


@pytest.mark.parametrize("k", [3, 4])
def test_end_to_end_on_the_unique_path_maps(k):
    m = gsr.fixture_map(FX, k)
    grid = _grid(m)
    z = np.load(gsr.GOLDEN.replace("g19_astar_init", "g1_onf"), allow_pickle=False)
    import gpu_common as gc
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    B = len(m["paths"])
    for n in (100, 256):
        for directed in (False, True):
            traj, status = nfopp.grid_search_init(grid, _dev(m["starts"]), _dev(m["goals"]), n, directed)
            assert (status.cpu().numpy() == 0).all()
            _check_traj(traj.cpu().numpy(), m, n, directed, what="map %d grid_search_init" % k)
            for ini in (grid, nfopp.AstarTrajectoryInitializer(_host_checker(m), m["resolution"], directed)):
                bp = nfopp.BatchPlanner(onf, B, n, nfopp.TrajectoryHyper(), init_angles_with_trajectory=directed)
                bp.init(m["starts"], m["goals"], m["boundaries"], initializer=ini)
                assert (bp.seed_status.cpu().numpy() == 0).all()
                _check_traj(bp.engine.traj.cpu().numpy(), m, n, directed, what="map %d BatchPlanner" % k)
            # the factory, the initialiser named in the parameters, B = 1
            from test_gpu_planner_api import _params
            p = _params(n)
            p.trajectory_initializer = nfopp.AttributeDict(name="AstarTrajectoryInitializer", resolution=m["resolution"],
                                                           init_angles_with_trajectory=directed)
            for i in (0, B - 1):
                planner = nfopp.PlannerFactory.make_constrained_onf_planner(_host_checker(m), p)
                planner.init(m["starts"][i], m["goals"][i], m["boundaries"])
                got = planner._trajectory.detach().cpu().numpy()[None]
                _check_traj(got, m, n, directed, rows=[i], what="map %d factory" % k)
    # the host protocol of the reference, on a CPU tensor
    tr = torch.zeros(100, 3)
    nfopp.AstarTrajectoryInitializer(_host_checker(m), m["resolution"]).initialize_trajectory(
        tr, torch.tensor(m["starts"][:1]), torch.tensor(m["goals"][:1]))
    _check_traj(tr.numpy()[None], m, 100, False, rows=[0], what="map %d host protocol" % k)


def test_status_and_straight_line_fallback():
    m = gsr.fixture_map(FX, 4)
    grid = _grid(m)
    b, res = m["boundaries"], m["resolution"]
    wr, wc = [int(v) for v in FX["m4_walled_cell"]]
    starts, goals = m["starts"].copy(), m["goals"].copy()
    goals[1, :2] = (b[0] + (wc + 0.4) * res, b[2] + (wr + 0.6) * res)        # the walled-off free cell
    starts[2, :2] = (b[0] - 3.0, b[2] + 1.0)                                 # outside the boundaries
    goals[5, :2] = (b[1] + 7.0, b[3] + 7.0)
    for directed in (False, True):
        traj, status = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), 100, directed)
        status, traj = status.cpu().numpy(), traj.cpu().numpy()
        assert list(status) == [0, 1, 2, 0, 0, 2, 0, 0]
        line = nfopp.init_trajectories(_dev(starts), _dev(goals), 100, directed).cpu().numpy()
        for i in (1, 2, 5):
            assert np.array_equal(traj[i], line[i])
        rest = [0, 3, 4, 6, 7]
        _check_traj(traj[rest], m, 100, directed, rows=rest, what="status batch")
    cells, counts, st, costs = [t.cpu().numpy() for t in nfopp.grid_search_paths(grid, _dev(starts), _dev(goals))]
    assert list(st) == [0, 1, 2, 0, 0, 2, 0, 0] and (counts[[1, 2, 5]] == 0).all() and (costs[[1, 2, 5]] == -1).all()


def test_scale_4096_problems_on_the_corridor_map():
    g16 = np.load(gsr.GOLDEN.replace("g19_astar_init", "g16_grid_checker"), allow_pickle=False)["grid"]
    checker = nfopp.DeviceGridChecker(g16, 0.0, 0.0, 1.0, device="cuda")
    grid = nfopp.OccupancyGrid.from_checker(checker, 1.0, boundaries=(0.5, 100.0, 0.5, 100.0))
    m1 = gsr.fixture_map(FX, 1)
    assert np.array_equal(grid.occupancy_host, m1["occ"])          # the device rasteriser gives the reference's map
    rng = np.random.default_rng(4096)
    B, N = 4096, 256
    free = np.argwhere(grid.occupancy_host == 0)
    pick = free[rng.integers(0, len(free), (2, B))]
    pts = [np.concatenate([0.5 + pick[j][:, ::-1] + rng.uniform(0.05, 0.95, (B, 2)), rng.uniform(-3, 3, (B, 1))], 1).astype(F32)
           for j in (0, 1)]
    starts, goals = _dev(pts[0]), _dev(pts[1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    traj, status = nfopp.grid_search_init(grid, starts, goals, N)
    torch.cuda.synchronize()
    print("4096 x 256 seeding, wall clock incl. host: %.1f ms" % (1e3 * (time.perf_counter() - t0)))
    assert traj.shape == (B, N, 3) and bool(torch.isfinite(traj).all())
    cells, counts, st, costs = [t.cpu().numpy() for t in nfopp.grid_search_paths(grid, starts, goals)]
    assert np.array_equal(st, status.cpu().numpy()) and set(np.unique(st)) <= {0, 1}
    ok = np.flatnonzero(st == 0)
    assert len(ok) > B // 2
    sc, gc_ = gsr.cells_of(pts[0], grid.boundaries, 1.0), gsr.cells_of(pts[1], grid.boundaries, 1.0)
    for i in ok:                                                   # every path valid ...
        occ = grid.occupancy_host
        assert gsr.check_path(occ, cells[i, :counts[i]], sc[i], gc_[i]) == tuple(costs[i])
    for i in rng.choice(ok, 64, replace=False):                    # ... and optimal on a random subset
        assert tuple(gsr.dijkstra_field(grid.occupancy_host, gc_[i])[sc[i, 0], sc[i, 1]]) == tuple(costs[i])
    for i in np.flatnonzero(st == 1)[:8]:
        assert gsr.dijkstra_field(grid.occupancy_host, gc_[i])[sc[i, 0], sc[i, 1], 0] < 0


def test_large_grid_uses_the_wide_global_memory_path():
    rng = np.random.default_rng(1024)
    occ = (rng.uniform(size=(1024, 1024)) < 0.3).astype(np.uint8)
    for j, r in enumerate(range(128, 1024, 128)):      # seven walls with a gap at alternating ends: paths of thousands of cells
        occ[r] = 1
        occ[r, (0 if j % 2 else 1016):(8 if j % 2 else 1024)] = 0
    grid = nfopp.OccupancyGrid(occ, (0.0, 1023.5, 0.0, 1023.5), 1.0, device="cuda")
    assert nfopp.load_library().nfopp_grid_fields_workspace_bytes(1024, 1024, 4) > 0
    free = np.argwhere(occ == 0)
    goals = free[rng.integers(0, len(free), 4)].astype(np.int32)
    fields = nfopp.distance_fields(grid, _dev(goals, torch.int32)).cpu().numpy()
    want = gsr.dijkstra_field(occ, goals[0])
    assert np.array_equal(fields[0], want)
    assert (want[..., 0] + want[..., 1]).max() > 2048                # far longer than a path of an LDS-sized grid
    # a long path through the seeding stage's global workspace
    far = np.unravel_index(np.argmax(want[..., 0] + want[..., 1]), want.shape[:2])
    start = np.asarray([[far[1] + 0.3, far[0] + 0.7, 0.0]], F32)     # off-centre: no zero-length segment
    goal = np.asarray([[goals[0, 1] + 0.6, goals[0, 0] + 0.2, 1.0]], F32)
    cells, counts, st, costs = [t.cpu().numpy() for t in nfopp.grid_search_paths(grid, _dev(start), _dev(goal))]
    assert st[0] == 0 and tuple(costs[0]) == tuple(want[far])
    assert gsr.check_path(occ, cells[0, :counts[0]], far, goals[0]) == tuple(costs[0])
    assert nfopp.load_library().nfopp_grid_seed_workspace_bytes(1, int(counts[0])) > 0
    traj, _ = nfopp.grid_search_init(grid, _dev(start), _dev(goal), 256)
    poly = gsr.polyline(cells[0, :counts[0]], start[0], goal[0], grid.boundaries, 1.0)
    ref = gsr.reparametrize(poly, 258)[1:-1]
    # same fp32 chord lengths as the reference; what differs is scipy's banded LU against the tridiagonal elimination in
    # float64 on a spline of thousands of points, and the fp32 cast (ulp 6e-5 at 1000 m): 1e-3 m is far above both
    assert np.abs(traj.cpu().numpy()[0, :, :2] - ref).max() < 1e-3


def test_torch_op_matches_the_ctypes_path():
    from nfopp import torch_ops
    ops = torch_ops.load()
    m = gsr.fixture_map(FX, 3)
    grid = _grid(m)
    starts, goals = _dev(m["starts"]), _dev(m["goals"])
    want, _ = nfopp.grid_search_init(grid, starts, goals, 100, True)
    sc, gc_ = grid.cells_of(starts), grid.cells_of(goals)
    uniq, inv = torch.unique(gc_[:, 0].long() * grid.shape[1] + gc_[:, 1].long(), return_inverse=True)
    ucells = torch.stack([uniq // grid.shape[1], uniq % grid.shape[1]], 1).to(torch.int32).contiguous()
    traj = torch.zeros_like(want)
    status = ops.grid_search_init(traj, starts, goals, grid.occupancy, sc, gc_, ucells, inv.to(torch.int32).contiguous(),
                                  grid.boundaries[0], grid.boundaries[2], grid.resolution, True)
    assert (status.cpu().numpy() == 0).all() and torch.equal(traj, want)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.grid_search_init(traj.cpu(), starts, goals, grid.occupancy, sc, gc_, ucells, inv.to(torch.int32), 0.0, 0.0, 1.0, False)
