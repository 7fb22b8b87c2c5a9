"""CPU restatement of the any-angle shortening of cell paths (csrc/grid_any_angle.hip, the rule of include/nfopp_hip.h),
for the tests: the integer traversal of a segment between two cell centres, visibility with dist2 and a threshold, the
farthest-visible anchors and the dense points.  Integers are Python ints; the points are float64 with every operation
rounded on its own, in the order the header states, stored fp32.

`clipped_cells` is the definition the traversal is held to: exact rational clipping of the segment against every open
cell square.  AA_SPREAD is to the any-angle seeds what gsr.SPREAD is to the cell-path seeds: the largest distance between
gsr.reparametrize and gsr.spline_longdouble over the any-angle seeding cases (maps 1 and 2 of the g19 fixture, N = 100),
measured by tests/test_any_angle_cpu.py, which fails if the cases exceed it."""
from fractions import Fraction

import numpy as np

import edt_ref as er
import grid_search_ref as gsr

AA_SPREAD = 3.0e-14      # metres: 2.85e-14 measured (test_any_angle_cpu.py)
SEED_N = 100             # waypoints of the any-angle seeding cases
INF = float("inf")


def traverse(a, b):
    """The cells whose open interior the segment between the centres of a and b (row, col) meets, in order, a and b
    included: the merge of column crossing i = 1..ac at (2i - 1) / (2 ac) and row crossing j = 1..ar at (2j - 1) / (2 ar),
    compared as (2i - 1) ar <> (2j - 1) ac; equal steps both (a lattice corner: only the diagonal cell)."""
    r, c = int(a[0]), int(a[1])
    dr, dc = int(b[0]) - r, int(b[1]) - c
    ar, ac = abs(dr), abs(dc)
    sr, sc = (1 if dr > 0 else -1), (1 if dc > 0 else -1)
    i = j = 1
    out = [(r, c)]
    while i <= ac or j <= ar:
        ck, rk = (2 * i - 1) * ar, (2 * j - 1) * ac
        col = i <= ac and (j > ar or ck <= rk)
        row = j <= ar and (i > ac or rk <= ck)
        if col:
            c, i = c + sc, i + 1
        if row:
            r, j = r + sr, j + 1
        out.append((r, c))
    return out


def clipped_cells(a, b):
    """The definition: the set of cells (r, c) whose OPEN square (c, c + 1) x (r, r + 1) contains a point of the closed
    segment between the centres of a and b, by exact rational clipping of the segment against every cell of the bounding
    box of a and b and one ring of cells around it (the segment does not leave the box)."""
    x0, y0 = Fraction(2 * int(a[1]) + 1, 2), Fraction(2 * int(a[0]) + 1, 2)
    dx, dy = int(b[1]) - int(a[1]), int(b[0]) - int(a[0])

    def span(p0, d, k):      # the open parameter interval in which p0 + t d lies in (k, k + 1); None = empty
        if d == 0:
            return (-INF, INF) if k < p0 < k + 1 else None
        t0, t1 = (k - p0) / d, (k + 1 - p0) / d
        return (min(t0, t1), max(t0, t1))

    out = set()
    for r in range(min(a[0], b[0]) - 1, max(a[0], b[0]) + 2):
        sy = span(y0, dy, r)
        if sy is None:
            continue
        for c in range(min(a[1], b[1]) - 1, max(a[1], b[1]) + 2):
            sx = span(x0, dx, c)
            if sx is None:
                continue
            t_lo, t_hi = max(sx[0], sy[0]), min(sx[1], sy[1])
            if t_lo < t_hi and t_hi > 0 and t_lo < 1:      # the open interval meets [0, 1]
                out.add((r, c))
    return out


def sees(dist2, threshold, a, b):
    """a sees b: no cell of the traversal other than a and b has dist2 <= threshold."""
    return all(dist2[r, c] > threshold for r, c in traverse(a, b)[1:-1])


def anchors(dist2, threshold, path, lookahead):
    """a_0 = 0, a_{k+1} = the largest j in (a_k, min(a_k + lookahead, n - 1)] that path[a_k] sees, a_k + 1 if none."""
    n = len(path)
    out = [0]
    while out[-1] < n - 1:
        at = out[-1]
        nxt = at + 1
        for j in range(min(at + lookahead, n - 1), at, -1):
            if sees(dist2, threshold, path[at], path[j]):
                nxt = j
                break
        out.append(nxt)
    return out


def centre(u, resolution, origin):
    """(float)((u * res + res / 2) + origin) with float64 `u` (array or scalar)."""
    res = np.float64(resolution)
    return (((np.asarray(u, np.float64) * res) + res / np.float64(2.0)) + np.float64(origin)).astype(np.float32)


def dense_points(path, anchor_list, boundaries, resolution):
    """fp32 [points, 2] xy: per segment A -> B of consecutive anchors, m = max(|dr|, |dc|) points at
    u = (double)A + (double)(d * t) / (double)m, t = 0 .. m - 1; then the centre of the last anchor."""
    path = np.asarray(path, np.int64)
    xs, ys = [], []
    for k0, k1 in zip(anchor_list[:-1], anchor_list[1:]):
        (r0, c0), (r1, c1) = path[k0], path[k1]
        dr, dc = int(r1 - r0), int(c1 - c0)
        m = max(abs(dr), abs(dc))
        if m == 0:
            continue
        t = np.arange(m, dtype=np.int64)
        xs.append(centre(np.float64(c0) + (dc * t).astype(np.float64) / np.float64(m), resolution, boundaries[0]))
        ys.append(centre(np.float64(r0) + (dr * t).astype(np.float64) / np.float64(m), resolution, boundaries[2]))
    r, c = path[anchor_list[-1]]
    xs.append(centre([np.float64(c)], resolution, boundaries[0]))
    ys.append(centre([np.float64(r)], resolution, boundaries[2]))
    return np.stack([np.concatenate(xs), np.concatenate(ys)], 1)


def in_grid(path, shape):
    path = np.asarray(path, np.int64).reshape(-1, 2)
    return bool(((path >= 0) & (path < np.asarray(shape))).all())


def shorten(dist2, threshold, path, lookahead, boundaries, resolution):
    """One row of nfopp_grid_shorten_paths -> (anchors list, points fp32 [point_count, 2])."""
    a = anchors(dist2, threshold, path, lookahead)
    return a, dense_points(path, a, boundaries, resolution)


def traced_paths(m, occupancy=None):
    """The documented paths of fixture map `m` (gsr.fixture_map) on `occupancy` (default: the map's own): one exact field
    per distinct goal cell and the trace rule.  -> list of int64 [count, 2], an empty array where there is no way."""
    occ = m["occ"] if occupancy is None else occupancy
    fields, out = {}, []
    for s, g in zip(m["start_cells"], m["goal_cells"]):
        goal = (int(g[0]), int(g[1]))
        if goal not in fields:
            fields[goal] = gsr.dijkstra_field(occ, goal)
        out.append(gsr.trace_path(fields[goal], s)[0])
    return out


def polyline(points, start, goal):
    """[start xy, points, goal xy] fp32: what the spline stage interpolates."""
    return np.concatenate([np.asarray(start, np.float32)[None, :2], np.asarray(points, np.float32),
                           np.asarray(goal, np.float32)[None, :2]], 0)


def seed_reference(points, start, goal, n):
    """float64 [n, 2]: the reference's waypoints of one shortened polyline."""
    return gsr.reparametrize(polyline(points, start, goal), n + 2)[1:-1]


def level_paths(m, levels):
    """Seeding with clearance levels (descending thresholds on dist2) restated: -> (paths, thresholds): per problem the
    traced path on the image of the first level at which its goal is reachable (er.seed_levels), on the plain grid with
    threshold 0 if at none."""
    lv = er.seed_levels(m["occ"], m["start_cells"], m["goal_cells"], levels)
    per_level = {-1: traced_paths(m)}
    for k in set(int(v) for v in lv if v >= 0):
        per_level[k] = traced_paths(m, er.inflate(m["occ"], levels[k]))
    paths = [per_level[int(v)][i] for i, v in enumerate(lv)]
    return paths, [0 if v < 0 else int(levels[v]) for v in lv]
