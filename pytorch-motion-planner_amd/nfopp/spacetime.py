"""Space-time grid search for the robots a fleet schedule cannot place (csrc/spacetime_search.hip): such a robot gets another
path, chosen with time in it -- an earliest-arrival search on an occupancy grid against what is already reserved, robot after
robot in priority order.  The rule is stated in include/nfopp_hip.h; nothing here synchronises when the inputs are device
tensors.  The uint64 words of a reservation travel in int64 tensors (the same bits).

A planned track runs over cell centres: it starts up to res / sqrt(2) from where the robot stands (the snap), which the caller
adds to `margin`.  Grid tracks are seeds and timetables, not smooth trajectories."""
import numpy as np
import torch

from . import _lib
from ._grid import int32_on, workspace
from ._tracks import check_tracks, per_row, raw_ptr

# values of SpaceTimePlan.status (NFOPP_SPACETIME_*)
SPACETIME_OK, SPACETIME_BAD_CELL, SPACETIME_UNREACHED, SPACETIME_NOT_ORDERED = 0, 1, 2, 3
SPACETIME_DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (0, 0))   # (drow, dcol); the wait is last


def _check_count(count):
    if int(count) != count or int(count) < 1:
        raise ValueError("count must be an integer >= 1 (the instants of the time grid), got %r" % (count,))
    return int(count)


def _finite(v, name):
    v = float(v)
    if not np.isfinite(v):
        raise ValueError("%s must be finite, got %r" % (name, v))
    return v


class SpaceTimeReservation(object):
    """What is reserved on `grid` over `count` instants for a fleet of robots of one `robot_radius`: which edges (cell,
    direction, instant) are blocked -- by a wall, the image edge, or a mover -- and which cells are taken at the last instant.

    `blocked` [count - 1, 9, rows, W] and `last` [rows, W] are int64 views of one device buffer, W = (cols + 63) // 64 words a
    row, bit c % 64 of word c // 64 is column c; the padding bits of a row are 1 in `blocked` and 0 in `last`.  `add` ORs tracks
    in; `spacetime_plan` adds every robot it plans."""

    def __init__(self, grid, count, robot_radius, margin=0.0):
        self.grid, self.count = grid, _check_count(count)
        self.robot_radius = float(np.float32(_finite(robot_radius, "robot_radius")))   # the fp32 value the kernels and the tracks carry
        self.margin = _finite(margin, "margin")
        lib = _lib.load()
        rows, cols = grid.shape
        nbytes = int(lib.nfopp_spacetime_reservation_bytes(rows, cols, self.count))
        if nbytes == 0:
            raise ValueError("a %d x %d image over %d instants is more than an int32 indexes" % (rows, cols, self.count))
        occ = grid.occupancy
        self.words = torch.empty(nbytes // 8, dtype=torch.int64, device=occ.device)
        _lib.check(lib.nfopp_spacetime_reservation_init(_lib.ptr(occ, torch.uint8), rows, cols, self.count,
                                                        _lib.ptr(self.words, torch.int64), nbytes, _lib.stream_ptr()))

    @property
    def row_words(self):
        return (self.grid.shape[1] + 63) // 64

    @property
    def blocked(self):
        rows = self.grid.shape[0]
        n = (self.count - 1) * 9 * rows * self.row_words
        return self.words[:n].view(self.count - 1, 9, rows, self.row_words)

    @property
    def last(self):
        rows = self.grid.shape[0]
        return self.words[(self.count - 1) * 9 * rows * self.row_words:].view(rows, self.row_words)

    def clone(self):
        other = SpaceTimeReservation.__new__(SpaceTimeReservation)
        other.__dict__.update(self.__dict__)
        other.words = self.words.clone()
        return other

    def add(self, tracks, radius=0.0, visible=None):
        """tracks [M, count, >= 2]: fp32 HIP tensor in absolute time; `radius`: a number or [M]; `visible`: None or [M] bool /
        uint8, a zero hides the track.  A track with a non-finite coordinate or radius is skipped.  -> self."""
        m, k, stride = check_tracks(tracks, "tracks")
        if k != self.count:
            raise ValueError("tracks must cover count = %d instants, got %d" % (self.count, k))
        device = self.words.device
        if not tracks.is_cuda or tracks.device != device:
            raise _lib.NfoppError("SpaceTimeReservation.add needs HIP tensors on the reservation's device (there is no CPU path)")
        radius = per_row(radius, m, device, "radius")
        if visible is not None:
            visible = torch.as_tensor(visible, device=device).reshape(-1).ne(0).to(torch.uint8).contiguous()
            if visible.numel() != m:
                raise ValueError("visible must be [M] = [%d], got %d values" % (m, visible.numel()))
        lib = _lib.load()
        rows, cols = self.grid.shape
        ws = workspace(lib.nfopp_spacetime_reserve_workspace_bytes(m), device)
        _lib.check(lib.nfopp_spacetime_reserve(
            rows, cols, self.count, *self.grid.origin_resolution, self.robot_radius, self.margin, raw_ptr(tracks) if m else None, m,
            stride, _lib.ptr(radius), _lib.ptr(visible, torch.uint8), _lib.ptr(self.words, torch.int64), self.words.numel() * 8,
            ws.ptr, ws.nbytes, _lib.stream_ptr()))
        return self


class SpaceTimePlan(object):
    """What `spacetime_plan` decided.  Device tensors: `cells` [R, T] int32 (the flat index row * cols + col of the robot's
    cell at every instant; -1 = not planned), `arrival` [R] int32 (the instant from which it stands on its goal; -1), `status`
    [R] int32 (0, SPACETIME_BAD_CELL, SPACETIME_UNREACHED, SPACETIME_NOT_ORDERED), `tracks` [R, T, 2] fp32 (cell centres; NaN
    rows = not planned), and the `reservation` with every planned robot in it."""
    OK, BAD_CELL, UNREACHED, NOT_ORDERED = SPACETIME_OK, SPACETIME_BAD_CELL, SPACETIME_UNREACHED, SPACETIME_NOT_ORDERED

    def __init__(self, cells, arrival, status, tracks, reservation):
        self.cells, self.arrival, self.status, self.tracks, self.reservation = cells, arrival, status, tracks, reservation

    @property
    def planned(self):
        """[R] bool device tensor: the robots that got a path."""
        return self.status == SPACETIME_OK


def _cells(grid, v, name, device):
    """Points [R, 2 or 3] (floating) or cells [R, 2] (integers, (row, col)) -> int32 [R, 2] on the device."""
    if not isinstance(v, torch.Tensor):
        a = np.asarray(v)
        v = torch.from_numpy(np.ascontiguousarray(a if a.dtype.kind in "iu" else a.astype(np.float32)))
    if v.dim() != 2 or v.shape[1] not in (2, 3):
        raise ValueError("%s must be [R, 2] cells (row, col) or [R, 2 or 3] points, got %s" % (name, tuple(v.shape)))
    v = v.to(device)
    if v.is_floating_point():
        return grid.cells_of(v)
    if v.shape[1] != 2:
        raise ValueError("%s: integer cells are [R, 2] (row, col), got %s" % (name, tuple(v.shape)))
    return int32_on(device, v)[0]


def spacetime_plan(grid, starts, goals, count, *, robot_radius, margin=0.0, tracks=None, track_radius=None, visible=None, order=None,
                   reservation=None):
    """R robots of one `robot_radius` on `grid` (an OccupancyGrid, inflated by the caller for the robot's footprint) over
    `count` instants: in priority `order` (None: robot 0 first; [R] integers, an entry out of range or repeated is skipped on the
    device) each robot gets the path that arrives at its goal earliest and stays clear of the walls, of the visible `tracks`
    [M, count, >= 2] (radius `track_radius`) and of every robot planned before it.  `starts` / `goals`: points [R, 2 or 3]
    (floating) or cells [R, 2] (integers, (row, col)).  `reservation`: a SpaceTimeReservation to go on from -- it is written
    to -- in place of a fresh one (then `robot_radius` and `margin` must be its own) -> `SpaceTimePlan`."""
    count = _check_count(count)
    if reservation is None:
        reservation = SpaceTimeReservation(grid, count, robot_radius, margin)
    else:
        if reservation.grid is not grid or reservation.count != count:
            raise ValueError("the reservation was made for another grid or count")
        if reservation.robot_radius != float(np.float32(robot_radius)) or reservation.margin != float(margin):
            raise ValueError("the reservation was made for another robot_radius or margin")
    device = reservation.words.device
    if tracks is not None:
        reservation.add(tracks, 0.0 if track_radius is None else track_radius, visible)
    elif track_radius is not None or visible is not None:
        raise ValueError("track_radius and visible belong to tracks")
    starts, goals = _cells(grid, starts, "starts", device), _cells(grid, goals, "goals", device)
    if starts.shape != goals.shape:
        raise ValueError("starts and goals must have the same number of rows, got %d and %d" % (starts.shape[0], goals.shape[0]))
    r = starts.shape[0]
    if order is not None:
        if not isinstance(order, torch.Tensor):
            order = torch.from_numpy(np.array(order, np.int64).reshape(-1))
        if order.dim() != 1 or order.numel() != r or order.is_floating_point():
            raise ValueError("order must be [R] = [%d] integers, got %s %s" % (r, tuple(order.shape), order.dtype))
        order, = int32_on(device, order)
    lib = _lib.load()
    rows, cols = grid.shape
    i32 = dict(dtype=torch.int32, device=device)
    cells, arrival, status = torch.empty(r, count, **i32), torch.empty(r, **i32), torch.empty(r, **i32)
    out = torch.empty(r, count, 2, dtype=torch.float32, device=device)
    ws = workspace(lib.nfopp_spacetime_plan_workspace_bytes(rows, cols, count, r), device)
    _lib.check(lib.nfopp_spacetime_plan_fleet(
        _lib.ptr(grid.occupancy, torch.uint8), rows, cols, count, *grid.origin_resolution, reservation.robot_radius,
        reservation.margin, _lib.ptr(starts, torch.int32), _lib.ptr(goals, torch.int32), _lib.ptr(order, torch.int32), r,
        _lib.ptr(reservation.words, torch.int64), reservation.words.numel() * 8, _lib.ptr(cells, torch.int32),
        _lib.ptr(arrival, torch.int32), _lib.ptr(status, torch.int32), _lib.ptr(out), ws.ptr, ws.nbytes, _lib.stream_ptr()))
    return SpaceTimePlan(cells, arrival, status, out, reservation)
