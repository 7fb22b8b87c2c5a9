"""CPU restatement of the grid-search seeder, for the tests: exact integer-pair Dijkstra, path checks and the spline
re-sampling through scipy.  A cost is (a, b) = (straight, diagonal) moves; sqrt 2 is irrational, so two paths of equal
cost have the same pair and pairs are ordered exactly by the sign test da^2 <> 2 db^2.

For the shape tests (test_grid_search_shapes_cpu.py, test_gpu_grid_search_shapes.py) it also holds the documented trace
rule (`trace_path`, vectorised as `trace_paths`), a heap search fast enough for grids of 65536 cells whose result is
proved exact cell by cell (`fast_field`, `is_exact_field`), the map makers and the shape table around the LDS /
global-memory switch of the field kernel, and the seeding cases with `spline_longdouble`, the same spline solved in
extended precision.  SPREAD, the largest |reparametrize - spline_longdouble| over every waypoint of every seeding case,
measures 1.34e-13 m (x86-64 long double against scipy's banded LU in float64); the cases are kept below SPREAD_CAP."""
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


# ---- the trace rule (include/nfopp_hip.h), restated --------------------------------------------------------------------
def trace_path(field, start_cell):
    """The documented descent through one field [rows, cols, 2]: from a cell whose pair is (a, b) the first move in MOVES
    order whose neighbour holds exactly (a - straight, b - diagonal).  From a start whose entry is (-1, -1) the first
    move goes to the free in-grid neighbour with the smallest Cost of field + move (equal cost = equal pair: the first
    in MOVES order wins).  -> (cells int64 [count, 2], (a, b)); no such neighbour (status 1): (empty [0, 2], (-1, -1))."""
    f = np.asarray(field)
    rows, cols = f.shape[:2]
    r, c = int(start_cell[0]), int(start_cell[1])
    cells = [(r, c)]
    cur = (int(f[r, c, 0]), int(f[r, c, 1]))
    if cur[0] < 0:
        best = None
        for i, (dr, dc) in enumerate(MOVES):
            nr, nc = r + dr, c + dc
            if not (0 <= nr < rows and 0 <= nc < cols) or f[nr, nc, 0] < 0:
                continue
            cand = Cost((int(f[nr, nc, 0]) + (i < 4), int(f[nr, nc, 1]) + (i >= 4)))
            if best is None or cand < best[0]:
                best = (cand, nr, nc)
        if best is None:
            return np.zeros((0, 2), np.int64), (-1, -1)
        cost, r, c = tuple(best[0]), best[1], best[2]
        cells.append((r, c))
        cur = (int(f[r, c, 0]), int(f[r, c, 1]))
    else:
        cost = cur
    while cur != (0, 0):
        for i, (dr, dc) in enumerate(MOVES):
            nr, nc = r + dr, c + dc
            if 0 <= nr < rows and 0 <= nc < cols and f[nr, nc, 0] >= 0 and \
                    f[nr, nc, 0] + (i < 4) == cur[0] and f[nr, nc, 1] + (i >= 4) == cur[1]:
                r, c = nr, nc
                break
        else:
            raise AssertionError("descent is stuck at (%d, %d): not a fixed-point field" % (r, c))
        cells.append((r, c))
        cur = (int(f[r, c, 0]), int(f[r, c, 1]))
    return np.asarray(cells, np.int64), cost


def _lt(a1, b1, a2, b2):
    """Cost.__lt__ on int64 arrays."""
    da, db = a1 - a2, b1 - b2
    return np.where((da <= 0) & (db <= 0), (da != 0) | (db != 0),
                    np.where((da >= 0) & (db >= 0), False, np.where(da < 0, da * da > 2 * db * db, da * da < 2 * db * db)))


def _neighbours(field):
    """-> for each move i: (reached, a + straight, b + diagonal) of the neighbour in direction MOVES[i], [rows, cols] each;
    cells outside the grid are not reached."""
    f = np.asarray(field, np.int64)
    rows, cols = f.shape[:2]
    pad = np.full((rows + 2, cols + 2, 2), -1, np.int64)
    pad[1:-1, 1:-1] = f
    out = []
    for i, (dr, dc) in enumerate(MOVES):
        n = pad[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]
        out.append((n[..., 0] >= 0, n[..., 0] + (i < 4), n[..., 1] + (i >= 4)))
    return out


def trace_paths(field, starts):
    """trace_path for many starts at once, all walking in lockstep.  starts int [B, 2]; a start outside the grid gives
    status 2.  -> (cells int32 [B, max(count, 1), 2] zero-padded, count [B], status [B], cost [B, 2]) as
    nfopp_grid_trace_paths reports them (count 0 and cost (-1, -1) where status != 0)."""
    f = np.asarray(field, np.int64)
    rows, cols = f.shape[:2]
    starts = np.asarray(starts, np.int64).reshape(-1, 2)
    B = len(starts)
    nb = _neighbours(f)
    reached = np.stack([n[0] for n in nb])                                 # [8, rows, cols]
    na, nbb = np.stack([n[1] for n in nb]), np.stack([n[2] for n in nb])
    status = np.zeros(B, np.int32)
    inside = (starts[:, 0] >= 0) & (starts[:, 0] < rows) & (starts[:, 1] >= 0) & (starts[:, 1] < cols)
    status[~inside] = 2
    r, c = np.where(inside, starts[:, 0], 0), np.where(inside, starts[:, 1], 0)
    cost = np.full((B, 2), -1, np.int64)
    cost[inside] = f[r[inside], c[inside]]
    moves = np.asarray(MOVES, np.int64)
    steps = [np.stack([r, c], 1)]
    first = np.zeros(B, np.int64)                                          # 1 where the path starts with the wall move
    wall = inside & (cost[:, 0] < 0)
    for p in np.flatnonzero(wall):
        best = None
        for i in range(8):
            if reached[i, r[p], c[p]]:
                cand = Cost((int(na[i, r[p], c[p]]), int(nbb[i, r[p], c[p]])))
                if best is None or cand < best[0]:
                    best = (cand, i)
        if best is None:
            status[p] = 1
        else:
            cost[p] = best[0]
            first[p] = 1
    # the wall move: walkers that take it step first, the others wait one round
    ok = status == 0
    a, b = cost[:, 0].copy(), cost[:, 1].copy()
    take = np.flatnonzero(first == 1)
    for p in take:
        for i in range(8):
            if reached[i, r[p], c[p]] and na[i, r[p], c[p]] == a[p] and nbb[i, r[p], c[p]] == b[p]:
                r[p], c[p] = r[p] + moves[i, 0], c[p] + moves[i, 1]
                break
        a[p], b[p] = f[r[p], c[p]]
    count = np.where(ok, first + a + b + 1, 0).astype(np.int32)
    L = max(int(count.max(initial=0)), 1)
    cells = np.zeros((B, L, 2), np.int32)
    cells[ok, 0] = np.stack([starts[ok, 0], starts[ok, 1]], 1)
    pos = first.copy()                                                     # index of the cell (r, c) in its path
    active = ok & (count > 0)
    while True:
        idx = np.flatnonzero(active)
        if not len(idx):
            break
        cells[idx, pos[idx], 0], cells[idx, pos[idx], 1] = r[idx], c[idx]
        active[idx[(a[idx] == 0) & (b[idx] == 0)]] = False
        idx = np.flatnonzero(active)
        if not len(idx):
            break
        # neighbour i fits when its pair plus the move equals the current pair: na / nbb already hold pair + move
        fit = reached[:, r[idx], c[idx]] & (na[:, r[idx], c[idx]] == a[idx]) & (nbb[:, r[idx], c[idx]] == b[idx])
        assert fit.any(0).all(), "descent is stuck: not a fixed-point field"
        pick = fit.argmax(0)                                               # the first in MOVES order
        r[idx] += moves[pick, 0]
        c[idx] += moves[pick, 1]
        a[idx], b[idx] = f[r[idx], c[idx], 0], f[r[idx], c[idx], 1]
        pos[idx] += 1
    cost[~ok] = -1
    return cells, count, status, cost.astype(np.int32)


# ---- a fast exact field for the large shapes ----------------------------------------------------------------------------
def is_exact_field(occupancy, goal, field):
    """True iff `field` is THE cost-to-goal field, decided with the exact sign test, vectorised.  It is iff the goal holds
    (0, 0), every other reached cell is free, has a reached neighbour whose pair plus the move equals its own (so its
    pair is the cost of a real path: a + b falls by one per step and only the goal holds (0, 0)) and none whose pair plus
    the move is smaller (so no path is cheaper, by induction along a cheapest one), and no unreached free cell touches a
    reached one.  A goal outside the grid: nothing is reached."""
    occ = np.asarray(occupancy) != 0
    f = np.asarray(field, np.int64)
    rows, cols = occ.shape
    a, b = f[..., 0], f[..., 1]
    reached = a >= 0
    gr, gc = int(goal[0]), int(goal[1])
    if not (0 <= gr < rows and 0 <= gc < cols):
        return bool((f == -1).all())
    free = ~occ
    free[gr, gc] = True
    if (a[gr, gc], b[gr, gc]) != (0, 0) or (reached & ~free).any() or (f[~reached] != -1).any() or (b[reached] < 0).any():
        return False
    has_parent = np.zeros((rows, cols), bool)
    cheaper = np.zeros((rows, cols), bool)
    touches = np.zeros((rows, cols), bool)
    for ok, na, nb in _neighbours(f):
        touches |= ok
        has_parent |= ok & (na == a) & (nb == b)
        cheaper |= ok & _lt(na, nb, a, b)
    other = reached.copy()
    other[gr, gc] = False
    return bool(has_parent[other].all() and not cheaper[reached].any() and not touches[free & ~reached].any())


def fast_field(occupancy, goal):
    """dijkstra_field for grids of tens of thousands of cells: the heap is keyed by a + b sqrt 2 in float64 (plain floats
    compare quickly), and the result is then proved exact by is_exact_field, which does not depend on that key."""
    occ = np.asarray(occupancy) != 0
    rows, cols = occ.shape
    out = np.full((rows, cols, 2), -1, np.int32)
    gr, gc = int(goal[0]), int(goal[1])
    if not (0 <= gr < rows and 0 <= gc < cols):
        return out
    free = (~occ).tolist()
    free[gr][gc] = True
    root2 = float(np.sqrt(2.0))
    best = {}
    done = [[False] * cols for _ in range(rows)]
    heap = [(0.0, 0, 0, gr, gc)]
    while heap:
        k, a, b, r, c = heapq.heappop(heap)
        if done[r][c]:
            continue
        done[r][c] = True
        out[r, c, 0], out[r, c, 1] = a, b
        for i, (dr, dc) in enumerate(MOVES):
            nr, nc = r + dr, c + dc
            if not (0 <= nr < rows and 0 <= nc < cols) or not free[nr][nc] or done[nr][nc]:
                continue
            na, nb = a + (i < 4), b + (i >= 4)
            nk = na + nb * root2
            if nk < best.get((nr, nc), np.inf):
                best[(nr, nc)] = nk
                heapq.heappush(heap, (nk, na, nb, nr, nc))
    assert is_exact_field(occupancy, goal, out), "the float-keyed heap search is not exact here"
    return out


# ---- maps and shapes -----------------------------------------------------------------------------------------------------
MAP_KINDS = ("empty", "random", "serpentine", "full")


def make_map(kind, rows, cols):
    """uint8 [rows, cols], deterministic.  empty: no wall.  random: each cell a wall with p = 0.3 (seeded by the shape).
    serpentine: every other row a wall with a one-cell gap at alternating ends, a plain free corridor when one side is 1.
    full: all walls."""
    occ = np.zeros((rows, cols), np.uint8)
    if kind == "random":
        occ[:] = np.random.default_rng(1000003 * rows + cols).uniform(size=(rows, cols)) < 0.3
    elif kind == "serpentine":
        if rows > 1 and cols > 1:
            for j, r in enumerate(range(1, rows, 2)):
                occ[r] = 1
                occ[r, 0 if j % 2 else cols - 1] = 0
    elif kind == "full":
        occ[:] = 1
    elif kind != "empty":
        raise ValueError(kind)
    return occ


# (rows, cols) around every size-dependent branch of the field kernel.  The first SHAPES_LDS entries are relaxed in LDS
# (rows * cols <= 65535 and (rows + 2) * (cols rounded up to 7, + 2) <= 36864 words), the rest in global memory;
# (4094, 1) pads to exactly 36864 words.  test_grid_search_shapes_cpu.py asks the library and fails here if a constant moves.
SHAPES = ((1, 1), (1, 2), (2, 1), (1, 7), (1, 8), (7, 1), (3, 6), (3, 7), (3, 8), (13, 15), (64, 64),
          (189, 183), (184, 189), (5, 5264), (1, 12285), (4094, 1),
          (4095, 1), (1, 12286), (190, 190), (256, 256))
SHAPES_LDS = 16


def shape_goals(occ):
    """The goal cells of the field tests, int32 [6, 2]: the free cell nearest the centre (the centre on a map without
    one), the last cell, the first again, the wall cell nearest (rows / 3, cols / 3) (that cell itself on a map without
    walls), and two cells outside the grid: (-1, 0) and (0, cols)."""
    rows, cols = occ.shape

    def nearest(mask, r0, c0):
        rc = np.argwhere(mask)
        if not len(rc):
            return (r0, c0)
        return tuple(int(v) for v in rc[np.argmin((rc[:, 0] - r0) ** 2 + (rc[:, 1] - c0) ** 2)])

    centre = nearest(occ == 0, rows // 2, cols // 2)
    wall = nearest(occ != 0, rows // 3, cols // 3)
    return np.asarray([centre, (rows - 1, cols - 1), centre, wall, (-1, 0), (0, cols)], np.int32)


# ---- seeding cases ---------------------------------------------------------------------------------------------------------
SEED_BOUNDARIES = (-3.0, 400.0, 2.0, 400.0)     # x crosses zero at column 12
SEED_RESOLUTION = 0.25
SEED_NS = (1, 2, 255, 256, 257, 700)
SEED_DIRECTED_NS = (2, 257, 700)
SPREAD_CAP = 1e-9       # metres: the condition on the cases below
SPREAD = 1.4e-13        # metres: 1.34e-13 measured by test_grid_search_shapes_cpu.py, which fails if the cases exceed this


def _walk40():
    rng = np.random.default_rng(40)
    step = np.asarray([(0, 1), (1, 1), (-1, 1), (1, 0)])[rng.integers(0, 4, 39)]   # E, SE, NE, S: never back on itself
    cells = np.concatenate([[(30, 5)], (30, 5) + np.cumsum(step, 0)])
    return cells


def _serpentine3000(width=60):
    cells, r = [], 0
    while len(cells) < 3000:
        cols = range(width) if (r // 2) % 2 == 0 else range(width - 1, -1, -1)
        cells += [(r, c) for c in cols]
        cells.append((r + 1, cells[-1][1]))
        r += 2
    return np.asarray(cells[:3000])


def seed_cases():
    """-> list of dict(name, cells int32 [count, 2], start fp32 [3], goal fp32 [3], directed bool).  Cell paths made on the
    host: 1, 2, 3 and 40 cells, the 1167- and 1168-cell rows of a 1 x 1200 corridor, a 3000-cell serpentine.  Starts
    and goals lie inside the first / last cell at least 0.05 cell from its centre, so no segment has zero length.  The two
    cases marked `directed` carry headings that keep heading - th clear of +-pi (checked on the CPU)."""
    row = np.stack([np.zeros(1200, np.int64), np.arange(1200)], 1)
    paths = [("c1", np.asarray([(5, 7)]), (2.8, -2.9), False),
             ("c2", np.asarray([(5, 7), (6, 8)]), (-3.0, 3.1), False),
             ("c3", np.asarray([(5, 7), (5, 8), (6, 9)]), (0.0, 0.0), False),
             ("c40", _walk40(), (0.3, 0.9), True),
             ("row1167", row[:1167], (-1.0, 2.5), False),
             ("row1168", row[:1168], (3.0, -3.0), False),
             ("serp3000", _serpentine3000(), (0.4, 0.8), True)]
    b, res = SEED_BOUNDARIES, SEED_RESOLUTION
    out = []
    for name, cells, (th0, th1), directed in paths:
        first, last = cells[0], cells[-1]
        start = (b[0] + (first[1] + 0.5 + 0.3) * res, b[2] + (first[0] + 0.5 - 0.2) * res, th0)
        goal = (b[0] + (last[1] + 0.5 - 0.25) * res, b[2] + (last[0] + 0.5 + 0.35) * res, th1)
        out.append(dict(name=name, cells=cells.astype(np.int32), start=np.asarray(start, np.float32),
                        goal=np.asarray(goal, np.float32), directed=directed))
    return out


def seed_reference(case, n):
    """float64 [n, 2]: the reference's waypoints of one seeding case."""
    poly = polyline(case["cells"], case["start"], case["goal"], SEED_BOUNDARIES, SEED_RESOLUTION)
    return reparametrize(poly, n + 2)[1:-1]


def _basis2_ld(t, ell, x):
    """The three quadratic B-spline basis values B_{ell-2..ell}(x) on knots t (Cox - de Boor), arrays of longdouble."""
    def w(i, k):   # (x - t[i]) / (t[i + k] - t[i]), 0 where the span is empty
        span = t[i + k] - t[i]
        return np.where(span > 0, (x - t[i]) / np.where(span > 0, span, 1), 0)
    one = np.ones_like(x)
    b1 = {-1: (1 - w(ell, 1)) * one, 0: w(ell, 1) * one}         # degree 1: B_{ell-1}, B_ell
    return [(1 - w(ell - 1, 2)) * b1[-1],
            w(ell - 1, 2) * b1[-1] + (1 - w(ell, 2)) * b1[0],
            w(ell, 2) * b1[0]]


def spline_longdouble(path, point_count):
    """reparametrize with the linear algebra in np.longdouble: the same fp32 chord lengths + 1e-6, fp32 running sum,
    float64 parameter and midpoint knots, then the collocation system solved by plain dense elimination with row
    pivoting (rows whose entry is already zero are skipped) and the spline evaluated, all in longdouble.  It exists to
    measure how far the float64 reference is from the exact spline."""
    ld = np.longdouble
    path = np.asarray(path)
    distances = np.linalg.norm(path[1:] - path[:-1], axis=1) + 1e-6
    cum = np.concatenate([np.zeros(1), np.cumsum(distances)], axis=0)
    par = (cum / cum[-1]).astype(ld)
    m = len(par)
    t = np.concatenate([[par[0]] * 3, (par[1:-2] + par[2:-1]) / 2, [par[-1]] * 3]).astype(ld)   # m + 3 knots
    assert len(t) == m + 3

    def interval(x):
        return np.clip(np.searchsorted(t, x, side="right") - 1, 2, m - 1)

    A = np.zeros((m, m), ld)
    ell = interval(par)
    h = _basis2_ld(t, ell, par)
    for k in range(3):
        A[np.arange(m), ell - 2 + k] += h[k]
    rhs = path.astype(ld).copy()
    for k in range(m):
        below = k + np.flatnonzero(A[k:, k])
        p = below[np.argmax(np.abs(A[below, k]))]
        if p != k:
            A[[k, p]], rhs[[k, p]] = A[[p, k]], rhs[[p, k]]
        for i in k + 1 + np.flatnonzero(A[k + 1:, k]):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            rhs[i] -= f * rhs[k]
    coef = np.zeros_like(rhs)
    for k in range(m - 1, -1, -1):
        nz = k + 1 + np.flatnonzero(A[k, k + 1:])
        coef[k] = (rhs[k] - (A[k, nz, None] * coef[nz]).sum(0)) / A[k, k]
    x = np.linspace(0, 1, point_count).astype(ld)
    ell = interval(x)
    h = _basis2_ld(t, ell, x)
    return sum(h[k][:, None] * coef[ell - 2 + k] for k in range(3))
