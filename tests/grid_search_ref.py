"""CPU restatement of the grid-search seeder, for the tests: exact integer-pair Dijkstra, path checks and the spline
re-sampling through scipy.  A cost is (a, b) = (straight, diagonal) moves; sqrt 2 is irrational, so two paths of equal
cost have the same pair and pairs are ordered exactly by the sign test da^2 <> 2 db^2."""
import heapq
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_astar_init.npz")
# neighbour order of the path trace (include/nfopp_hip.h): N, W, S, E, NW, NE, SW, SE in (row, col)
MOVES = ((-1, 0), (0, -1), (1, 0), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


class Cost(tuple):
    """(a, b) ordered by a + b sqrt 2, exactly."""
    __slots__ = ()

    def __lt__(self, other):
        da, db = self[0] - other[0], self[1] - other[1]
        if da <= 0 and db <= 0:
            return (da, db) != (0, 0)
        if da >= 0 and db >= 0:
            return False
        if da < 0:          # db > 0: da + db sqrt2 < 0  <=>  da^2 > 2 db^2
            return da * da > 2 * db * db
        return da * da < 2 * db * db


def dijkstra_field(occupancy, goal):
    """-> int32 [rows, cols, 2]: exact minimum cost from every cell to `goal` (row, col) over free cells, 8-connected,
    no corner rule, goal forced free; (-1, -1) for walls and cells that cannot reach it."""
    occ = np.asarray(occupancy) != 0
    rows, cols = occ.shape
    out = np.full((rows, cols, 2), -1, np.int32)
    gr, gc = int(goal[0]), int(goal[1])
    if not (0 <= gr < rows and 0 <= gc < cols):
        return out
    best = {(gr, gc): Cost((0, 0))}
    done = set()
    heap = [(Cost((0, 0)), gr, gc)]
    while heap:
        d, r, c = heapq.heappop(heap)
        if (r, c) in done:
            continue
        done.add((r, c))
        out[r, c] = d
        for i, (dr, dc) in enumerate(MOVES):
            nr, nc = r + dr, c + dc
            if not (0 <= nr < rows and 0 <= nc < cols) or occ[nr, nc] or (nr, nc) in done:
                continue
            nd = Cost((d[0] + (i < 4), d[1] + (i >= 4)))
            old = best.get((nr, nc))
            if old is None or nd < old:
                best[(nr, nc)] = nd
                heapq.heappush(heap, (nd, nr, nc))
    return out


def path_cost(cells):
    """(a, b) of a cell path; raises if a step is not one of the 8 moves."""
    cells = np.asarray(cells, np.int64)
    step = np.abs(np.diff(cells, axis=0))
    assert step.max(initial=0) <= 1 and (step.sum(1) > 0).all(), "not an 8-connected path"
    diag = int((step.sum(1) == 2).sum())
    return len(step) - diag, diag


def check_path(occupancy, cells, start_cell, goal_cell):
    """Starts and ends in the right cells, moves 8-connectedly, every cell after the first is free (the goal counts as
    free, the start cell is not tested).  -> (a, b)."""
    occ = np.asarray(occupancy) != 0
    cells = np.asarray(cells, np.int64)
    assert tuple(cells[0]) == tuple(int(v) for v in start_cell), "wrong first cell"
    assert tuple(cells[-1]) == tuple(int(v) for v in goal_cell), "wrong last cell"
    assert (cells >= 0).all() and (cells[:, 0] < occ.shape[0]).all() and (cells[:, 1] < occ.shape[1]).all()
    inner = cells[1:-1]
    assert not occ[inner[:, 0], inner[:, 1]].any(), "path crosses a wall"
    return path_cost(cells)


def count_shortest_paths(occupancy, goal, start):
    """Number of minimum-cost paths start -> goal (dynamic programming over the exact field)."""
    f = dijkstra_field(occupancy, goal)
    rows, cols = f.shape[:2]
    memo = {}

    def n(r, c):
        if (r, c) == (int(goal[0]), int(goal[1])):
            return 1
        if (r, c) not in memo:
            tot = 0
            for i, (dr, dc) in enumerate(MOVES):
                nr, nc = r + dr, c + dc
                if 0 <= nr < rows and 0 <= nc < cols and f[nr, nc, 0] >= 0 and \
                        f[nr, nc, 0] + (i < 4) == f[r, c, 0] and f[nr, nc, 1] + (i >= 4) == f[r, c, 1]:
                    tot += n(nr, nc)
            memo[(r, c)] = tot
        return memo[(r, c)]

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * rows * cols + 100))
    return n(int(start[0]), int(start[1]))


def cells_of(points, boundaries, resolution):
    """(row, col) int64 [B, 2] of xy points: floor division in float64."""
    p = np.asarray(points, np.float64)
    col = np.floor((p[:, 0] - boundaries[0]) / resolution)
    row = np.floor((p[:, 1] - boundaries[2]) / resolution)
    return np.stack([row, col], 1).astype(np.int64)


def polyline(cells, start, goal, boundaries, resolution):
    """[start xy, cell centres, goal xy] as the reference builds it: centres in float64, stored fp32."""
    cells = np.asarray(cells, np.int64)
    centres = np.zeros((len(cells), 2), np.float32)
    centres[:, 0] = cells[:, 1] * resolution + resolution / 2 + boundaries[0]
    centres[:, 1] = cells[:, 0] * resolution + resolution / 2 + boundaries[2]
    return np.concatenate([np.asarray(start, np.float32)[None, :2], centres, np.asarray(goal, np.float32)[None, :2]], 0)


def reparametrize(path, point_count):
    """Quadratic interpolating spline over the normalised chord length (each segment + 1e-6), in the dtype of `path`
    up to the running sum, float64 afterwards -- the arithmetic of utils/math.py:57-65."""
    import scipy.interpolate
    distances = np.linalg.norm(path[1:] - path[:-1], axis=1) + 1e-6
    cum = np.concatenate([np.zeros(1), np.cumsum(distances)], axis=0)
    par = cum / cum[-1]
    spline = scipy.interpolate.interp1d(par, path, kind="quadratic", axis=0, fill_value="extrapolate")
    return spline(np.linspace(0, 1, point_count))


def load_fixture():
    return np.load(GOLDEN, allow_pickle=False)


def fixture_map(fx, k):
    """-> dict(occ, boundaries, resolution, starts, goals, start_cells, goal_cells, cost, paths (list), traj dict, noise)."""
    p = "m%d_" % k
    off = fx[p + "path_offsets"]
    flat = fx[p + "path_cells"]
    return dict(occ=fx[p + "occupancy"], boundaries=tuple(float(v) for v in fx[p + "boundaries"]),
                resolution=float(fx[p + "resolution"]), starts=fx[p + "starts"], goals=fx[p + "goals"],
                start_cells=fx[p + "start_cells"], goal_cells=fx[p + "goal_cells"], cost=fx[p + "cost"],
                paths=[flat[off[i]:off[i + 1]] for i in range(len(off) - 1)],
                traj={(n, d): fx[p + "traj_n%d_dir%d" % (n, d)] for n in (100, 256) for d in (0, 1)},
                noise={n: fx[p + "reparam_noise_n%d" % n] for n in (100, 256)})
