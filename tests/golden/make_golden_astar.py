#!/usr/bin/env python3
"""Generate tests/golden/g19_astar_init.npz from the reference's AstarTrajectoryInitializer (PyTorch-CPU, pure Python).

Needs the reference checkout (NFOPP_REFERENCE, imported unmodified with the shims of make_golden.py).  Only inputs and
the numbers the reference computed from them are written: occupancy, endpoints, cell paths, costs, trajectories.

Four maps: (1) the committed g16 occupancy grid through a host MapCollisionChecker, (2) a disc map rasterised by the
reference's CircleDirectedCollisionChecker inside calculate_astar_path, boundaries not a multiple of the resolution,
(3) a 21 x 21 serpentine of one-cell corridors, (4) a one-cell maze with a dead end and a walled-off free cell.  On
maps 3 and 4 every problem has exactly one shortest path (asserted by counting them).

Usage:  python tests/golden/make_golden_astar.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NFOPP_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import grid_search_ref as gsr  # noqa: E402


class AttributeDict(dict):
    __getattr__ = dict.__getitem__


for name in ("pytorch_lightning", "pytorch_lightning.utilities", "pytorch_lightning.utilities.parsing"):
    mod = types.ModuleType(name)
    mod.AttributeDict = AttributeDict
    sys.modules[name] = mod
if not hasattr(np, "bool"):
    np.bool = bool
sys.path.insert(0, REF)
from neural_field_optimal_planner.astar.astar_trajectory_initializer import AstarTrajectoryInitializer  # noqa: E402
from neural_field_optimal_planner.collision_checker import CircleDirectedCollisionChecker  # noqa: E402
from neural_field_optimal_planner.utils.math import reparametrize_path  # noqa: E402


class MatrixChecker(object):
    """Host checker over an occupancy matrix: cell (row, col) covers [b0 + col res, b0 + (col + 1) res) x likewise."""

    def __init__(self, matrix, boundaries, resolution):
        self.matrix, self.boundaries, self.resolution = np.asarray(matrix) != 0, boundaries, resolution

    def get_boundaries(self):
        return self.boundaries

    def check_collision(self, positions):
        col = np.floor((np.asarray(positions.x) - self.boundaries[0]) / self.resolution).astype(int)
        row = np.floor((np.asarray(positions.y) - self.boundaries[2]) / self.resolution).astype(int)
        ok = (row >= 0) & (col >= 0) & (row < self.matrix.shape[0]) & (col < self.matrix.shape[1])
        out = np.ones(len(col), bool)
        out[ok] = self.matrix[row[ok], col[ok]]
        return out


class MapChecker(object):
    """MapCollisionChecker arithmetic on the g16 grid (oracle grid_check): origin (0, 0), cell 1 m."""

    def __init__(self, grid):
        self.grid = grid

    def get_boundaries(self):
        return (0.5, 100.0, 0.5, 100.0)

    def check_collision(self, positions):
        ix = ((np.asarray(positions.x, np.float64) - 0.5) / 1.0).astype(np.int32)
        iy = ((np.asarray(positions.y, np.float64) - 0.5) / 1.0).astype(np.int32)
        ok = (ix >= 0) & (iy >= 0) & (iy < self.grid.shape[0] - 1) & (ix < self.grid.shape[1] - 1)
        out = np.ones(len(ix), bool)
        out[ok] = self.grid[iy[ok], ix[ok]] > 0
        return out


def serpentine():
    m = np.ones((21, 21), bool)
    for k, r in enumerate(range(1, 20, 2)):
        m[r, 1:20] = False
        if r + 1 < 20:
            m[r + 1, 19 if k % 2 == 0 else 1] = False
    return m


def maze():
    rows = ["###############",
            "#.....#.......#",
            "#.###.#.#####.#",
            "#.#...#.#...#.#",
            "#.#.###.#.#.#.#",
            "#.#.....#.#...#",
            "#.#######.###.#",
            "#.........#...#",
            "#########.#.###",
            "#.......#.#...#",
            "#.#####.#.###.#",
            "#.#...#...#...#",
            "#.#.#.#####.#.#",
            "#...#.......#.#",
            "####.##########",
            "#####.#########",
            "###############"]
    # row 14 col 4 is a dead-end stub below the maze
    m = np.array([[ch == "#" for ch in row] for row in rows])
    m[15, 10] = False     # the walled-off free cell: all 8 neighbours are walls
    return m


def occupancy_of(checker, resolution):
    b = checker.get_boundaries()
    x_cells = int((b[1] - b[0]) // resolution) + 1
    y_cells = int((b[3] - b[2]) // resolution) + 1
    x, y = np.meshgrid(range(x_cells), range(y_cells))
    x = x.reshape(-1) * resolution + resolution / 2 + b[0]
    y = y.reshape(-1) * resolution + resolution / 2 + b[2]
    from neural_field_optimal_planner.utils.position2 import Position2
    return np.asarray(checker.check_collision(Position2(x, y, np.ones_like(x) * 3 * np.pi / 4))).reshape(y_cells, x_cells)


def sample_problems(rng, occ, boundaries, resolution, count, unique):
    free = np.argwhere(~occ)
    out = []
    tries = 0
    while len(out) < count:
        tries += 1
        assert tries < 100000, "cannot find enough problems"
        s, g = free[rng.integers(len(free))], free[rng.integers(len(free))]
        if tuple(s) == tuple(g):
            continue
        f = gsr.dijkstra_field(occ, g)
        if f[s[0], s[1], 0] < 0:
            continue           # only reachable problems: the reference's answer for the others is meaningless
        if unique and gsr.count_shortest_paths(occ, g, s) != 1:
            continue
        pts = []
        for cell in (s, g):
            frac = rng.uniform(0.05, 0.95, 2)
            pts.append([boundaries[0] + (cell[1] + frac[0]) * resolution, boundaries[2] + (cell[0] + frac[1]) * resolution,
                        rng.uniform(-np.pi, np.pi)])
        out.append(np.asarray(pts, np.float32))
    return np.stack(out)


def run_map(out, k, checker, resolution, count, rng, unique=False):
    boundaries = tuple(float(v) for v in checker.get_boundaries())
    occ = occupancy_of(checker, resolution)
    problems = sample_problems(rng, occ, boundaries, resolution, count, unique)
    starts, goals = problems[:, 0], problems[:, 1]
    # every endpoint at least 1e-3 resolution from a cell edge, as seen from the fp32 values
    for pts in (starts, goals):
        for axis, b0 in ((0, boundaries[0]), (1, boundaries[2])):
            frac = ((pts[:, axis].astype(np.float64) - b0) / resolution) % 1.0
            assert (frac > 1e-3).all() and (frac < 1 - 1e-3).all()
    start_cells, goal_cells = gsr.cells_of(starts, boundaries, resolution), gsr.cells_of(goals, boundaries, resolution)
    paths, costs, noise = [], [], {100: [], 256: []}
    traj = {(n, d): [] for n in (100, 256) for d in (0, 1)}
    for i in range(count):
        ini = AstarTrajectoryInitializer(checker, resolution)
        with contextlib.redirect_stdout(io.StringIO()):
            centres = ini.calculate_astar_path(starts[i], goals[i])
        col = np.rint((centres[:, 0].astype(np.float64) - boundaries[0] - resolution / 2) / resolution).astype(np.int64)
        row = np.rint((centres[:, 1].astype(np.float64) - boundaries[2] - resolution / 2) / resolution).astype(np.int64)
        cells = np.stack([row, col], 1)
        occ_i = occ.copy()
        occ_i[goal_cells[i, 0], goal_cells[i, 1]] = False
        ab = gsr.check_path(occ_i, cells, start_cells[i], goal_cells[i])
        exact = gsr.dijkstra_field(occ, goal_cells[i])[start_cells[i, 0], start_cells[i, 1]]
        assert tuple(exact) == ab, "reference path is not minimum-cost: %s vs %s" % (ab, tuple(exact))
        if unique:
            assert gsr.count_shortest_paths(occ, goal_cells[i], start_cells[i]) == 1
        paths.append(cells.astype(np.int32))
        costs.append(ab)
        poly = np.concatenate([starts[i][None, :2], centres, goals[i][None, :2]], axis=0)
        assert poly.dtype == np.float32
        for n in (100, 256):
            ref = reparametrize_path(poly, n + 2)
            noise[n].append(np.abs(ref - reparametrize_path(poly.astype(np.float64), n + 2)).max())
            for d in (0, 1):
                t = torch.zeros(n, 3)
                s, g = torch.tensor(starts[i][None]), torch.tensor(goals[i][None])
                with contextlib.redirect_stdout(io.StringIO()):
                    AstarTrajectoryInitializer(checker, resolution, bool(d)).initialize_trajectory(t, s, g)
                assert np.array_equal(t[:, :2].numpy(), ref[1:-1].astype(np.float32))
                traj[(n, d)].append(t.numpy().copy())
    p = "m%d_" % k
    out[p + "occupancy"] = occ.astype(np.uint8)
    out[p + "boundaries"] = np.asarray(boundaries, np.float64)
    out[p + "resolution"] = np.float64(resolution)
    out[p + "starts"], out[p + "goals"] = starts, goals
    out[p + "start_cells"], out[p + "goal_cells"] = start_cells.astype(np.int32), goal_cells.astype(np.int32)
    out[p + "cost"] = np.asarray(costs, np.int32)
    out[p + "path_cells"] = np.concatenate(paths, 0)
    out[p + "path_offsets"] = np.concatenate([[0], np.cumsum([len(q) for q in paths])]).astype(np.int64)
    for n in (100, 256):
        out[p + "reparam_noise_n%d" % n] = np.asarray(noise[n], np.float64)
        for d in (0, 1):
            out[p + "traj_n%d_dir%d" % (n, d)] = np.stack(traj[(n, d)]).astype(np.float32)
    print("map %d: %s cells, %d problems, path cells %d..%d, noise %.1e..%.1e" % (
        k, occ.shape, count, min(map(len, paths)), max(map(len, paths)), min(noise[100]), max(noise[256])))


def main():
    rng = np.random.default_rng(1909)
    out = {}
    g16 = np.load(os.path.join(HERE, "g16_grid_checker.npz"), allow_pickle=False)["grid"]
    run_map(out, 1, MapChecker(g16), 1.0, 32, rng)
    discs = CircleDirectedCollisionChecker(0.35, (-1.0, 6.3, -0.5, 4.9))
    pts = np.concatenate([c + 0.3 * np.stack([np.cos(a), np.sin(a)], 1) * r
                          for c in ([1.5, 1.2], [3.4, 2.9], [4.6, 0.9], [1.2, 3.6], [2.9, 0.4], [5.2, 3.8])
                          for a in [np.linspace(0, 2 * np.pi, 12, endpoint=False)] for r in (0.5, 1.0)])
    discs.update_obstacle_points(pts)
    run_map(out, 2, discs, 0.25, 32, rng)
    out["m2_obstacle_points"] = pts.astype(np.float64)
    out["m2_robot_radius"] = np.float64(0.35)
    run_map(out, 3, MatrixChecker(serpentine(), (0.0, 10.4, 0.0, 10.4), 0.5), 0.5, 8, rng, unique=True)
    # the issue's own check of map 3: end to end of the serpentine
    f = gsr.dijkstra_field(serpentine(), (19, 1 if serpentine()[19, 1] == 0 else 19))
    print("serpentine corner to corner:", tuple(int(v) for v in f[1, 1]))
    m4 = maze()
    run_map(out, 4, MatrixChecker(m4, (-2.0, -2.0 + 0.4 * 14 + 0.3, 1.0, 1.0 + 0.4 * 16 + 0.3), 0.4), 0.4, 8, rng, unique=True)
    out["m4_walled_cell"] = np.asarray([15, 10], np.int32)
    np.savez_compressed(os.path.join(HERE, "g19_astar_init.npz"), **out)
    print("wrote g19_astar_init.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "g19_astar_init.npz")))


if __name__ == "__main__":
    main()
