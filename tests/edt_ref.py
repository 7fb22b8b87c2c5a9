"""CPU restatement of the grid distance transform (csrc/grid_edt.hip) and of seeding with a clearance margin
(nfopp/grid_search.py), for the tests.  All integer arithmetic.

The transform is stated twice: over all pairs (the definition) and separably (the form the kernel takes).  The CPU test
holds the two against each other; the GPU tests use whichever is cheaper for a shape (`edt`)."""
import numpy as np

import grid_search_ref as gsr

NONE = 2 ** 31 - 1   # dist2 when nothing is occupied
_FAR = 1 << 62


def with_border(dist2, border=True):
    """min(dist2, b^2), b = the distance to the nearest cell outside the matrix."""
    if not border:
        return dist2
    rows, cols = dist2.shape
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    b = np.minimum(np.minimum(r + 1, rows - r), np.minimum(c + 1, cols - c))
    return np.minimum(dist2, b * b)


def edt_all_pairs(occupancy, border=False):
    """-> (dist2, nearest) int32 [rows, cols]: the minimum over the occupied cells of (drow^2 + dcol^2, flat index)."""
    occ = np.asarray(occupancy) != 0
    rows, cols = occ.shape
    pts = np.argwhere(occ).astype(np.int64)              # row-major: ascending flat index
    if len(pts) == 0:
        dist2, nearest = np.full((rows, cols), NONE, np.int64), np.full((rows, cols), -1, np.int64)
    else:
        r, c = np.divmod(np.arange(rows * cols, dtype=np.int64), cols)
        flat = pts[:, 0] * cols + pts[:, 1]
        dist2, nearest = np.empty(rows * cols, np.int64), np.empty(rows * cols, np.int64)
        step = max(1, (1 << 22) // len(pts))
        for lo in range(0, rows * cols, step):
            d = (r[lo:lo + step, None] - pts[None, :, 0]) ** 2 + (c[lo:lo + step, None] - pts[None, :, 1]) ** 2
            k = np.argmin(d, axis=1)                      # the first minimum: the smallest flat index
            dist2[lo:lo + step] = d[np.arange(len(k)), k]
            nearest[lo:lo + step] = flat[k]
        dist2, nearest = dist2.reshape(rows, cols), nearest.reshape(rows, cols)
    return with_border(dist2, border).astype(np.int32), nearest.astype(np.int32)


def column_pass(occupancy):
    """-> int64 [rows, cols]: per cell the occupied row of its column nearest to it, the smaller row when the one above and
    the one below are equally far; -1 in a column without occupied cells."""
    occ = np.asarray(occupancy) != 0
    rows, cols = occ.shape
    r = np.arange(rows, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(occ, r, -1), axis=0)
    dn = np.minimum.accumulate(np.where(occ, r, _FAR)[::-1], axis=0)[::-1]
    take_dn = (dn < _FAR) & ((up < 0) | (dn - r < r - up))
    return np.where(take_dn, dn, up)


def edt_separable(occupancy, border=False):
    """-> (dist2, nearest): per row the minimum over col' of ((col - col')^2 + (row - g)^2, g, col'), g = column_pass."""
    occ = np.asarray(occupancy) != 0
    rows, cols = occ.shape
    g = column_pass(occ)
    c = np.arange(cols, dtype=np.int64)
    dcol2 = ((c[:, None] - c[None, :]) ** 2) << 24
    dist2, nearest = np.full((rows, cols), NONE, np.int64), np.full((rows, cols), -1, np.int64)
    for row in range(rows):
        have = g[row] >= 0
        if not have.any():
            continue
        key_of_column = np.where(have, (((row - g[row]) ** 2) << 24) | (g[row] << 12) | c, _FAR)   # (distance, g, col')
        key = (dcol2 + key_of_column[None, :]).min(axis=1)
        dist2[row] = key >> 24
        nearest[row] = ((key >> 12) & 0xfff) * cols + (key & 0xfff)
    return with_border(dist2, border).astype(np.int32), nearest.astype(np.int32)


def edt(occupancy, border=False):
    """The cheaper of the two statements for this image."""
    occ = np.asarray(occupancy) != 0
    return edt_all_pairs(occ, border) if int(occ.sum()) < occ.shape[1] else edt_separable(occ, border)


def inflate(occupancy, cells2, border=False):
    """uint8 image of the cells with dist2 <= cells2."""
    return (edt(occupancy, border)[0] <= cells2).astype(np.uint8)


def reachable(field, start_cell):
    """Whether the path trace of csrc/grid_search.hip reports status 0 for a start cell inside the grid: the start has a
    cost-to-goal, or -- the start cell is not tested for occupancy -- one of its neighbours has."""
    rows, cols = field.shape[:2]
    r, c = int(start_cell[0]), int(start_cell[1])
    if field[r, c, 0] >= 0:
        return True
    return any(0 <= r + dr < rows and 0 <= c + dc < cols and field[r + dr, c + dc, 0] >= 0 for dr, dc in gsr.MOVES)


def seed_levels(occupancy, start_cells, goal_cells, cells2_levels, border=False):
    """The seeding rule: for each problem the index into `cells2_levels` (descending thresholds) of the first level at which
    the goal is reachable on inflate(occupancy, k), -1 if it is at none (the problem is then seeded on the plain grid).
    Start and goal cells must lie inside the grid."""
    out = np.full(len(start_cells), -1, np.int64)
    for level in reversed(range(len(cells2_levels))):     # the largest threshold is applied last and wins
        occ = inflate(occupancy, cells2_levels[level], border)
        fields = {}
        for i, (s, g) in enumerate(zip(start_cells, goal_cells)):
            goal = (int(g[0]), int(g[1]))
            if goal not in fields:
                fields[goal] = gsr.dijkstra_field(occ, goal)
            if reachable(fields[goal], s):
                out[i] = level
    return out
