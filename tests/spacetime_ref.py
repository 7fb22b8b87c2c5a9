"""The rule of nfopp_spacetime_reservation_init / nfopp_spacetime_reserve / nfopp_spacetime_plan_fleet
(csrc/spacetime_search.hip, stated in include/nfopp_hip.h) restated in numpy.  The pair arithmetic is
tests/track_conflict_ref.py's, applied to two-sample tracks (a robot's move over one interval against a mover's): it is not
stated a second time here.  Everything else is booleans and integers, so the device is compared with this bit for bit
(tests/test_gpu_spacetime.py)."""
import numpy as np

import track_conflict_ref as tr

F32, F64, U64 = np.float32, np.float64, np.uint64
STATUS_OK, STATUS_BAD_CELL, STATUS_UNREACHED, STATUS_NOT_ORDERED = 0, 1, 2, 3
# (drow, dcol) of direction d; the wait is last
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (0, 0))
WAIT = 8


class Geometry(object):
    """rows, cols, the boundaries' origin (b0, b2) and the resolution of an OccupancyGrid."""

    def __init__(self, rows, cols, b0=0.0, b2=0.0, res=1.0):
        self.rows, self.cols, self.b0, self.b2, self.res = int(rows), int(cols), float(b0), float(b2), float(res)

    @property
    def words(self):
        return (self.cols + 63) // 64

    def centres(self):
        """-> (x [cols], y [rows]) fp32: cell_centres' float64 expression (nfopp/_grid.py), rounded once."""
        x = np.arange(self.cols) * self.res + self.res / 2 + self.b0
        y = np.arange(self.rows) * self.res + self.res / 2 + self.b2
        return x.astype(F32), y.astype(F32)

    def centre_grid(self):
        """-> [rows, cols, 2] fp32 (x, y)."""
        x, y = self.centres()
        return np.stack(np.broadcast_arrays(x[None, :], y[:, None]), -1)

    def centre_of(self, row, col):
        """One cell, inside the image or not (the same expression)."""
        return np.array([F32(col * self.res + self.res / 2 + self.b0), F32(row * self.res + self.res / 2 + self.b2)], F32)


def shifted(a, d, fill):
    """out[r, c] = a[r + drow, c + dcol] (the value at the cell direction d leads to), `fill` outside the image."""
    dr, dc = DIRS[d]
    rows, cols = a.shape
    out = np.full_like(a, fill)
    r0, r1, c0, c1 = max(0, -dr), min(rows, rows - dr), max(0, -dc), min(cols, cols - dc)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = a[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def static_blocked(occ, T):
    """[T - 1, 9, rows, cols] bool: edge (u, d, h) leads outside the image or onto a wall."""
    wall = np.asarray(occ) != 0
    one = np.stack([shifted(wall, d, True) for d in range(9)])
    return np.broadcast_to(one, (T - 1,) + one.shape).copy()


def good_tracks(tracks, radius, visible=None):
    """[M] bool: finite coordinates and radius, and visible."""
    t = np.asarray(tracks, F32)[:, :, :2]
    ok = np.isfinite(t).all(axis=(1, 2)) & np.isfinite(tr._radii(radius, len(t)))
    return ok if visible is None else ok & (np.asarray(visible) != 0)


def _interval_hits(a, b, ra, rb, margin):
    """a [Na, 2, 2], b [Nb, 2, 2]: two-sample tracks -> (hit [Na, Nb] bool: m < R2 on the one interval, s [Na, Nb]: the
    fraction of its closest approach).  tr.pairs folds the last-instant term e = |d1|^2 into its minimum; the interval's own m
    is that minimum whenever it is attained at k = 0, and where it is not (e < m: a rounding anomaly, the interval's m is the
    minimum over a segment that ends at d1) e >= R2 still decides "not blocked".  The case left over raises."""
    p = tr.pairs(a, b, dt=1.0, radius_a=ra, radius_b=rb, margin=margin)
    own = p["kstar"] == 0
    if (~own & (p["M"] < p["R2"])).any():
        raise AssertionError("the last-instant term of a two-sample pair undercuts its interval: state the interval directly")
    return own & (p["M"] < p["R2"]), p["sstar"]


def mover_bits(geo, T, tracks, radius, visible, robot_radius, margin, want_branches=False):
    """The movers' part of a reservation -> (blocked [T - 1, 9, rows, cols] bool, last [rows, cols] bool[, branches]).
    Only edges that stay inside the image are evaluated (the others are blocked statically)."""
    rows, cols = geo.rows, geo.cols
    blocked = np.zeros((max(T - 1, 0), 9, rows, cols), bool)
    last = np.zeros((rows, cols), bool)
    branches = dict(start=np.zeros_like(blocked), end=np.zeros_like(blocked), interior=np.zeros_like(blocked))
    t = np.asarray(tracks, F32)[:, :, :2] if tracks is not None and len(tracks) else np.zeros((0, T, 2), F32)
    assert t.shape[1] == T
    good = np.flatnonzero(good_tracks(t, radius, visible)) if len(t) else np.zeros(0, np.int64)
    if len(good):
        t = t[good]
        rad = tr._radii(radius, len(tracks)).astype(F32)[good]
        centre = geo.centre_grid()
        flat = centre.reshape(-1, 2)
        rr = F32(robot_radius)
        hit = tr.pairs(flat[:, None, :], t[:, -1:, :], dt=1.0, radius_a=rr, radius_b=rad, margin=margin)["tc"] < np.inf
        last = hit.any(axis=1).reshape(rows, cols)
        if T > 1:
            # movers' intervals as two-sample tracks [M * (T - 1), 2, 2]
            seg = np.stack([t[:, :-1], t[:, 1:]], 2).reshape(-1, 2, 2)
            seg_rad = np.repeat(rad, T - 1)
            for d in range(9):
                dr, dc = DIRS[d]
                inside = shifted(np.ones((rows, cols), bool), d, False).reshape(-1)
                src = np.flatnonzero(inside)
                if not len(src):
                    continue
                dest = src + dr * cols + dc
                a = np.stack([flat[src], flat[dest]], 1)
                hit, s = _interval_hits(a, seg, rr, seg_rad, margin)
                hit = hit.reshape(len(src), len(good), T - 1)
                s = s.reshape(hit.shape)
                out = np.zeros((rows * cols, T - 1), bool)
                out[src] = hit.any(axis=1)
                blocked[:, d] = out.T.reshape(T - 1, rows, cols)
                if want_branches:
                    for name, sel in (("start", s == 0.0), ("end", s == 1.0), ("interior", (s > 0.0) & (s < 1.0))):
                        out = np.zeros((rows * cols, T - 1), bool)
                        out[src] = (hit & sel).any(axis=1)
                        branches[name][:, d] = out.T.reshape(T - 1, rows, cols)
    return (blocked, last, branches) if want_branches else (blocked, last)


class Reservation(object):
    """blocked [T - 1, 9, rows, cols] bool and last [rows, cols] bool, accumulated."""

    def __init__(self, occ, geo, T, robot_radius, margin=0.0):
        occ = np.asarray(occ)
        assert T >= 1 and occ.shape == (geo.rows, geo.cols)
        self.occ, self.geo, self.T, self.robot_radius, self.margin = occ != 0, geo, int(T), F32(robot_radius), float(margin)
        self.blocked = static_blocked(occ, self.T)
        self.last = np.zeros(occ.shape, bool)

    def add(self, tracks, radius=None, visible=None):
        b, l = mover_bits(self.geo, self.T, tracks, radius, visible, self.robot_radius, self.margin)
        self.blocked |= b
        self.last |= l
        return self

    def copy(self):
        other = Reservation.__new__(Reservation)
        other.__dict__.update(self.__dict__)
        other.blocked, other.last = self.blocked.copy(), self.last.copy()
        return other

    def words(self):
        """-> (blocked [T - 1, 9, rows, W] uint64, last [rows, W] uint64): the device's layout.  Padding bits are 1 in blocked
        and 0 in last."""
        return pack_rows(self.blocked, True), pack_rows(self.last, False)


def pack_rows(bits, pad):
    """[..., cols] bool -> [..., W] uint64: bit c % 64 of word c // 64 is column c; the padding bits of a row are `pad`."""
    cols = bits.shape[-1]
    w = (cols + 63) // 64
    full = np.full(bits.shape[:-1] + (w * 64,), bool(pad))
    full[..., :cols] = bits
    return (full.reshape(bits.shape[:-1] + (w, 64)).astype(U64) << np.arange(64, dtype=U64)).sum(axis=-1, dtype=U64)


def unpack_rows(words, cols):
    words = np.asarray(words, U64)
    bits = ((words[..., :, None] >> np.arange(64, dtype=U64)) & U64(1)).astype(bool)
    return bits.reshape(words.shape[:-1] + (words.shape[-1] * 64,))[..., :cols]


def reach_sets(res, start):
    """[T, rows, cols] bool: reach_0 = {s}, reach_{h+1}[v] = OR_d reach_h[v - d] & !blocked[h, d, v - d]."""
    rows, cols = res.geo.rows, res.geo.cols
    reach = np.zeros((res.T, rows, cols), bool)
    reach[0, start[0], start[1]] = True
    for h in range(res.T - 1):
        nxt = np.zeros((rows, cols), bool)
        for d in range(9):
            open_ = reach[h] & ~res.blocked[h, d]          # by source; move it to its destination: the opposite shift
            dr, dc = DIRS[d]
            moved = np.zeros((rows, cols), bool)
            r0, r1, c0, c1 = max(0, dr), min(rows, rows + dr), max(0, dc), min(cols, cols + dc)
            if r0 < r1 and c0 < c1:
                moved[r0:r1, c0:c1] = open_[r0 - dr:r1 - dr, c0 - dc:c1 - dc]
            nxt |= moved
        reach[h + 1] = nxt
    return reach


def inside(geo, cell):
    return 0 <= cell[0] < geo.rows and 0 <= cell[1] < geo.cols


def search(res, start, goal):
    """One robot -> dict(status, arrival, cells [T] int32 flat, track [T, 2] fp32, dirs: the directions of the path's moves)."""
    geo, T = res.geo, res.T
    out = dict(status=STATUS_OK, arrival=-1, cells=np.full(T, -1, np.int32), track=np.full((T, 2), np.nan, F32), dirs=[])
    start, goal = (int(start[0]), int(start[1])), (int(goal[0]), int(goal[1]))
    if not (inside(geo, start) and inside(geo, goal)) or res.occ[start] or res.occ[goal]:
        out["status"] = STATUS_BAD_CELL
        return out
    reach = reach_sets(res, start)
    park = np.zeros(T, bool)
    park[T - 1] = not res.last[goal]
    for h in range(T - 2, -1, -1):
        park[h] = park[h + 1] and not res.blocked[h, WAIT, goal[0], goal[1]]
    ok = np.flatnonzero(reach[:, goal[0], goal[1]] & park)
    if not len(ok):
        out["status"] = STATUS_UNREACHED
        return out
    ha = int(ok[0])
    path = [None] * T
    for h in range(ha, T):
        path[h] = goal
    v, dirs = goal, []
    for h in range(ha, 0, -1):
        for d in range(9):
            u = (v[0] - DIRS[d][0], v[1] - DIRS[d][1])
            if inside(geo, u) and reach[h - 1][u] and not res.blocked[h - 1, d, u[0], u[1]]:
                break
        else:
            raise AssertionError("a reached cell has no predecessor")
        dirs.append(d)
        v = u
        path[h - 1] = v
    assert v == start
    centre = geo.centre_grid()
    out.update(arrival=ha, cells=np.array([r * geo.cols + c for r, c in path], np.int32), dirs=dirs[::-1],
               track=np.stack([centre[r, c] for r, c in path]).astype(F32))
    return out


def plan_fleet(res, starts, goals, order=None):
    """The fleet pass; `res` is accumulated in place -> dict(cells [R, T], arrival [R], status [R], tracks [R, T, 2], dirs)."""
    starts, goals = np.asarray(starts, np.int64).reshape(-1, 2), np.asarray(goals, np.int64).reshape(-1, 2)
    R, T = len(starts), res.T
    order = np.arange(R, dtype=np.int32) if order is None else np.asarray(order, np.int32)
    assert order.shape == (R,)
    cells = np.full((R, T), -1, np.int32)
    arrival = np.full(R, -1, np.int32)
    status = np.full(R, STATUS_NOT_ORDERED, np.int32)
    tracks = np.full((R, T, 2), np.nan, F32)
    dirs = [[] for _ in range(R)]
    visited = np.zeros(R, bool)
    for i in order:
        if i < 0 or i >= R or visited[i]:
            continue
        visited[i] = True
        one = search(res, starts[i], goals[i])
        status[i], arrival[i], cells[i], tracks[i], dirs[i] = one["status"], one["arrival"], one["cells"], one["track"], one["dirs"]
        if one["status"] == STATUS_OK:
            res.add(tracks[i:i + 1], radius=res.robot_radius)
    return dict(cells=cells, arrival=arrival, status=status, tracks=tracks, dirs=dirs)
