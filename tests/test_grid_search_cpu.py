"""CPU: the grid-search seeder's host side and the tests' own restatement, against the reference's results in
tests/golden/g19_astar_init.npz (tests/golden/make_golden_astar.py).  No GPU is touched."""
import numpy as np
import pytest

import nfopp

import grid_search_ref as gsr

FX = gsr.load_fixture()


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_exact_dijkstra_gives_the_reference_cost(k):
    m = gsr.fixture_map(FX, k)
    assert len(m["paths"]) >= (32 if k <= 2 else 8)
    assert np.array_equal(gsr.cells_of(m["starts"], m["boundaries"], m["resolution"]), m["start_cells"])
    assert np.array_equal(gsr.cells_of(m["goals"], m["boundaries"], m["resolution"]), m["goal_cells"])
    fields = {}
    for i, ref_path in enumerate(m["paths"]):
        goal = tuple(int(v) for v in m["goal_cells"][i])
        if goal not in fields:
            fields[goal] = gsr.dijkstra_field(m["occ"], goal)
        s = m["start_cells"][i]
        assert tuple(fields[goal][s[0], s[1]]) == tuple(m["cost"][i]), i
        occ = m["occ"].copy()
        occ[goal] = 0
        assert gsr.check_path(occ, ref_path, s, goal) == tuple(m["cost"][i]), i


@pytest.mark.parametrize("k", [3, 4])
def test_unique_shortest_path_is_the_reference_path(k):
    m = gsr.fixture_map(FX, k)
    for i, ref_path in enumerate(m["paths"]):
        goal, cur = m["goal_cells"][i], tuple(int(v) for v in m["start_cells"][i])
        assert gsr.count_shortest_paths(m["occ"], goal, cur) == 1
        f = gsr.dijkstra_field(m["occ"], goal)
        walk = [cur]
        while cur != tuple(int(v) for v in goal):
            for j, (dr, dc) in enumerate(gsr.MOVES):
                n = (cur[0] + dr, cur[1] + dc)
                if 0 <= n[0] < f.shape[0] and 0 <= n[1] < f.shape[1] and f[n][0] >= 0 and \
                        f[n][0] + (j < 4) == f[cur][0] and f[n][1] + (j >= 4) == f[cur][1]:
                    cur = n
                    break
            else:
                raise AssertionError("descent is stuck")
            walk.append(cur)
        assert np.array_equal(np.asarray(walk), ref_path), i


def test_cost_order_is_exact():
    assert gsr.Cost((7, 0)) < gsr.Cost((0, 5)) and not gsr.Cost((0, 5)) < gsr.Cost((7, 0))      # 7 < 7.0711
    assert gsr.Cost((0, 5)) < gsr.Cost((8, 0))
    assert gsr.Cost((1393, 0)) < gsr.Cost((0, 985)) and gsr.Cost((0, 985)) < gsr.Cost((1394, 0))  # differ by 3.6e-4
    assert not gsr.Cost((3, 4)) < gsr.Cost((3, 4))


def _disc_checker():
    m = gsr.fixture_map(FX, 2)
    checker = nfopp.CircleDirectedCollisionChecker(0.35, m["boundaries"])
    checker.update_obstacle_points(FX["m2_obstacle_points"])
    return m, checker


def test_initializer_constructs_with_a_host_checker():
    _, checker = _disc_checker()
    ini = nfopp.AstarTrajectoryInitializer(checker, resolution=0.5)
    assert ini._resolution == 0.5 and ini._init_angles_with_trajectory is False
    with pytest.raises(TypeError):
        nfopp.AstarTrajectoryInitializer(checker)
    with pytest.raises(NotImplementedError, match="check_collision"):
        nfopp.AstarTrajectoryInitializer(object(), 0.5)


def test_factory_builds_the_initializer_by_name():
    _, checker = _disc_checker()
    spec = nfopp.AttributeDict(name="AstarTrajectoryInitializer", resolution=0.25, init_angles_with_trajectory=True)
    ini = nfopp.UniversalFactory([nfopp.TrajectoryInitializer, nfopp.AstarTrajectoryInitializer]).make_from_parameters(
        spec, collision_checker=checker)
    assert type(ini) is nfopp.AstarTrajectoryInitializer
    assert ini._resolution == 0.25 and ini._init_angles_with_trajectory is True


def test_host_rasteriser_reproduces_the_reference_occupancy():
    m, checker = _disc_checker()
    grid = nfopp.OccupancyGrid.from_checker(checker, m["resolution"])
    assert grid.occupancy_host.dtype == np.uint8 and grid.occupancy_host.shape == m["occ"].shape
    assert np.array_equal(grid.occupancy_host, m["occ"])
    assert grid._occupancy_dev is None            # nothing was uploaded
    assert grid.boundaries == m["boundaries"] and grid.resolution == m["resolution"]


def test_polyline_and_spline_restatement_match_the_reference_trajectory():
    # fed the reference's cells, the helper's fp32 arithmetic is the reference's own: xy bit for bit
    for k in (1, 2):
        m = gsr.fixture_map(FX, k)
        for i in range(0, len(m["paths"]), 5):
            poly = gsr.polyline(m["paths"][i], m["starts"][i], m["goals"][i], m["boundaries"], m["resolution"])
            for n in (100, 256):
                got = gsr.reparametrize(poly, n + 2)[1:-1].astype(np.float32)
                assert np.array_equal(got, m["traj"][(n, 0)][i][:, :2])
