"""Grid-search (A*) trajectory seeding for whole batches on the device (csrc/grid_search.hip).

B (start, goal) problems on one shared occupancy grid give B initial trajectories [B, N, D] with the semantics of the
reference's AstarTrajectoryInitializer (nfop/astar/astar_trajectory_initializer.py, astar/jps.py with jps=False,
utils/math.py reparametrize_path): exact minimum-cost 8-connected paths, re-sampled by a quadratic spline.  Which of
several minimum-cost paths is taken is this library's own fixed rule (include/nfopp_hip.h), not the reference's heap
order.  A problem whose goal cannot be reached is reported in `status` and seeded with the straight line."""

import numpy as np
import torch

from . import _lib
from ._grid import (GridFrame, as_device_points, cell_centres, cell_keys, checker_boundaries, checker_device, goal_table, int32_on,
                    seed_launch, traced_search, workspace)
from .host_utils import Position2

STATUS_OK, STATUS_UNREACHABLE, STATUS_OUTSIDE = 0, 1, 2
RASTER_HEADING = 3 * np.pi / 4   # astar_trajectory_initializer.py:37
_MISSING = object()


class OccupancyGrid(GridFrame):
    """uint8 occupancy [rows = y cells, cols = x cells] (non-zero = wall) with the geometry of the reference's raster
    (GridFrame: `cells_of`, `cell_centres`).

    The occupancy of a grid never changes after construction, so its distance transform (csrc/grid_edt.hip) and the images
    inflated from it are computed once and kept."""

    def __init__(self, occupancy_uint8, boundaries, resolution, device="cuda"):
        occ = np.ascontiguousarray(np.asarray(occupancy_uint8) != 0, dtype=np.uint8)
        if occ.ndim != 2 or occ.size == 0:
            raise ValueError("occupancy must be a non-empty [rows, cols] array")
        self._occupancy_host = occ
        self._shape = occ.shape
        GridFrame.__init__(self, boundaries, resolution)
        self.device = device
        self._occupancy_dev = None
        self._edt = {}        # border -> (dist2, nearest)
        self._inflated = {}   # (cells2, border) -> OccupancyGrid
        self._sdf = {}        # border -> signed distance image

    @classmethod
    def _from_device(cls, occupancy_dev, boundaries, resolution):
        """A grid around a uint8 0 / 1 device image; the host copy is read back only if someone asks for it."""
        grid = cls.__new__(cls)
        grid._occupancy_host = None
        grid._shape = tuple(occupancy_dev.shape)
        grid.boundaries, grid.resolution, grid.device = boundaries, resolution, occupancy_dev.device
        grid._occupancy_dev = occupancy_dev
        grid._edt, grid._inflated, grid._sdf = {}, {}, {}
        return grid

    @property
    def shape(self):
        return self._shape

    @property
    def occupancy_host(self):
        if self._occupancy_host is None:
            self._occupancy_host = self._occupancy_dev.cpu().numpy()
        return self._occupancy_host

    @property
    def occupancy(self):
        """The device copy (uploaded on first use)."""
        if self._occupancy_dev is None:
            _lib.require_gpu()
            self._occupancy_dev = torch.tensor(self.occupancy_host, device=self.device)
        return self._occupancy_dev

    @classmethod
    def from_checker(cls, checker, resolution, boundaries=None, device=None):
        """Rasterises a collision checker the way calculate_astar_path does (:27-39): the checker's answer for the pose
        (cell centre, heading 3 pi / 4).  Device checkers (`labels`) are asked once on the device, host checkers
        (`check_collision`) once on the host."""
        if resolution is None:
            raise TypeError("from_checker() needs a resolution")
        boundaries = checker_boundaries(checker, boundaries)
        x, y, x_cells, y_cells = cell_centres(boundaries, resolution)
        if hasattr(checker, "labels") and not hasattr(checker, "check_collision"):
            dev = checker_device(checker, device)
            poses = torch.tensor(np.stack([x, y, np.full_like(x, RASTER_HEADING)], 1).astype(np.float32), device=dev)
            occ = (checker.labels(poses) > 0).to(torch.uint8).reshape(y_cells, x_cells)
            grid = cls(occ.cpu().numpy(), boundaries, resolution, dev)
            grid._occupancy_dev = occ.contiguous()
            return grid
        if not hasattr(checker, "check_collision"):
            raise TypeError("the checker offers neither check_collision nor labels")
        hit = np.asarray(checker.check_collision(Position2(x, y, np.ones_like(x) * RASTER_HEADING)))
        return cls(hit.reshape(y_cells, x_cells), boundaries, resolution, device or "cuda")

    def distance_transform(self, border=False):
        """-> (dist2, nearest), int32 [rows, cols] on the device (nfopp_grid_edt): the squared Euclidean distance, in cells,
        to the nearest wall cell (INT32_MAX on a grid without walls) and that cell's flat index row * cols + col, the
        smallest among equidistant ones (-1 without walls).  With `border` the cells outside the grid count as walls for
        dist2; nearest still names cells of the grid.  Computed once per `border` value."""
        border = bool(border)
        if border not in self._edt:
            self._edt[border] = _edt_of(self.occupancy, border)
        return self._edt[border]

    def signed_distance_field(self, border=False):
        """-> fp32 [rows, cols] on the device: the signed distance in metres at each cell's centre, positive in free cells
        and negative in walls, resolution * (sqrt(dist2 to the nearest wall cell) - sqrt(dist2 to the nearest free cell))
        formed in float64 and rounded once.  Of two edge-adjacent cells on either side of a wall's edge one holds
        +resolution and the other -resolution: a linear interpolation crosses zero on the edge.  `border` counts the cells
        outside the grid as walls for the first distance.  Where there is no wall, or no free cell, at all the missing
        distance is taken as rows + cols cells, so every value is finite and an interpolation never forms inf * 0.
        Computed once per `border` value (nfopp.DistanceField plans on it)."""
        border = bool(border)
        if border not in self._sdf:
            to_wall = self.distance_transform(border)[0]
            to_free = _edt_of(1 - self.occupancy, False)[0]
            far = float(self.shape[0] + self.shape[1])
            cells = [torch.where(d2 == EDT_NONE, torch.full_like(d2, far, dtype=torch.float64), torch.sqrt(d2.double()))
                     for d2 in (to_wall, to_free)]
            self._sdf[border] = ((cells[0] - cells[1]) * self.resolution).float()
        return self._sdf[border]

    def clearance_field(self, border=False):
        """-> fp32 [rows, cols] on the device: the distance in metres from each cell's centre to the centre of the nearest
        wall cell, resolution * sqrt(dist2) formed in float64 and rounded once; +inf on a grid without walls."""
        dist2, _ = self.distance_transform(border)
        metres = (torch.sqrt(dist2.double()) * self.resolution).float()
        return torch.where(dist2 == EDT_NONE, torch.full_like(metres, float("inf")), metres)

    def inflated(self, margin=None, *, cells2=None, border=False):
        """-> the OccupancyGrid (same boundaries and resolution) whose walls are the cells with dist2 <= k: every cell
        within sqrt(k) cells of a wall.  k = `cells2`, or margin_cells2(margin, resolution) for a `margin` in metres.
        k = 0 gives an image equal to this one.  Decided on the device; nothing is read back."""
        if (margin is None) == (cells2 is None):
            raise TypeError("inflated() takes a margin in metres or cells2=k, not both and not neither")
        k = margin_cells2(margin, self.resolution) if cells2 is None else int(cells2)
        if k < 0 or k >= EDT_NONE or (cells2 is not None and k != cells2):
            raise ValueError("cells2 must be a non-negative integer below 2^31 - 1")
        key = (k, bool(border))
        if key not in self._inflated:
            dist2, _ = self.distance_transform(border)
            self._inflated[key] = OccupancyGrid._from_device((dist2 <= k).to(torch.uint8), self.boundaries, self.resolution)
        return self._inflated[key]


EDT_NONE = 2 ** 31 - 1   # dist2 on a grid without walls (INT32_MAX)


def _edt_of(occ, border):
    """nfopp_grid_edt of a uint8 0 / 1 device image -> (dist2, nearest), int32 [rows, cols]."""
    lib = _lib.load()
    rows, cols = occ.shape
    dist2 = torch.empty(rows, cols, dtype=torch.int32, device=occ.device)
    nearest = torch.empty(rows, cols, dtype=torch.int32, device=occ.device)
    ws = workspace(lib.nfopp_grid_edt_workspace_bytes(rows, cols), occ.device)
    _lib.check(lib.nfopp_grid_edt(_lib.ptr(occ, torch.uint8), rows, cols, int(border), _lib.ptr(dist2, torch.int32),
                                  _lib.ptr(nearest, torch.int32), ws.ptr, ws.nbytes, _lib.stream_ptr()))
    return dist2, nearest


def margin_cells2(margin, resolution):
    """The threshold on dist2 for a margin in metres: floor((margin / resolution)^2 * (1 + 1e-9)).  The slack keeps a
    margin that is a whole number of cells up to the rounding of the division (0.7 / 0.1) at its square (49); dist2 is an
    integer, so it admits nothing else."""
    margin = float(margin)
    if not (margin >= 0.0 and np.isfinite(margin)):
        raise ValueError("a clearance margin must be finite and >= 0")
    q = margin / float(resolution)
    return int(np.floor(q * q * (1.0 + 1e-9)))


def distance_fields(grid, goal_cells):
    """goal_cells int32 [G, 2] (row, col) on the device -> int32 [G, rows, cols, 2] exact costs-to-goal (a, b);
    (-1, -1) = wall or unreachable."""
    lib = _lib.load()
    occ = grid.occupancy
    rows, cols = grid.shape
    goal_cells = goal_cells.to(torch.int32).contiguous()
    g = goal_cells.shape[0]
    fields = torch.empty(g, rows, cols, 2, dtype=torch.int32, device=occ.device)
    ws = workspace(lib.nfopp_grid_fields_workspace_bytes(rows, cols, g), occ.device)
    _lib.check(lib.nfopp_grid_distance_fields(_lib.ptr(occ, torch.uint8), rows, cols, _lib.ptr(goal_cells, torch.int32), g,
                                              _lib.ptr(fields, torch.int32), ws.ptr, ws.nbytes, _lib.stream_ptr()))
    return fields


def _search(grid, starts, goals):
    """-> (cells [B, max_len, 2], count, status, cost, starts, goals), all on the device."""
    lib = _lib.load()
    starts, goals = as_device_points(grid, starts), as_device_points(grid, goals)
    if starts.shape != goals.shape:
        raise ValueError("starts and goals must have the same shape")
    rows, cols = grid.shape
    b = starts.shape[0]
    i32 = torch.int32
    start_cells, goal_cells = grid.cells_of(starts), grid.cells_of(goals)
    # the key of a goal: its flat cell index
    inside, flat = cell_keys(goal_cells, grid.shape)
    uniq, field_index = goal_table(torch.where(inside, flat, torch.full_like(flat, -1)))
    unique_cells = torch.stack([uniq // cols, uniq % cols], 1).to(i32).contiguous()

    def trace(fields, first, paths, count, status, cost):
        _lib.check(lib.nfopp_grid_trace_paths(
            _lib.ptr(fields, i32), 0 if fields is None else fields.shape[0], rows, cols, _lib.ptr(start_cells, i32),
            _lib.ptr(goal_cells, i32), _lib.ptr(field_index, i32), b, paths[0].shape[1] if paths else 0,
            _lib.ptr(paths[0], i32) if paths else None, _lib.ptr(count, i32), _lib.ptr(status, i32), _lib.ptr(cost, i32),
            _lib.stream_ptr()))

    n = unique_cells.shape[0]   # every field at once: one chunk
    (cells,), count, status, cost = traced_search(b, starts.device, n, max(n, 1), ((2,),),
                                                  lambda first, last: distance_fields(grid, unique_cells), trace)
    return cells, count, status, cost, starts, goals


def _margins(clearance):
    """clearance (a margin in metres or a descending sequence of them) -> list of floats."""
    margins = [float(clearance)] if np.ndim(clearance) == 0 else [float(m) for m in clearance]
    for m in margins:
        if not (m >= 0.0 and np.isfinite(m)):
            raise ValueError("a clearance margin must be finite and >= 0")
    if any(a <= b for a, b in zip(margins, margins[1:])):
        raise ValueError("clearance margins must be strictly descending")
    return margins


def _search_with_clearance(grid, starts, goals, clearance):
    """_search on the plain grid and on grid.inflated(margin) for every margin; each problem keeps the result of the largest
    margin at which its search returns status 0, else the plain grid's (with its status 1 / 2).  The levels are merged on
    the device.  -> (cells, count, status, cost, starts, goals, seed_margin fp32 [B], seed_cells2 int32 [B]): the margin each
    problem was seeded at and the threshold on dist2 of that level, both 0 for the plain grid."""
    starts, goals = as_device_points(grid, starts), as_device_points(grid, goals)
    cells, count, status, cost = _search(grid, starts, goals)[:4]
    seed_margin = torch.zeros(count.shape[0], dtype=torch.float32, device=count.device)
    seed_cells2 = torch.zeros(count.shape[0], dtype=torch.int32, device=count.device)
    levels = []
    for m in _margins(clearance):
        if margin_cells2(m, grid.resolution) > 0:   # k = 0 is the plain grid
            levels.append((m, _search(grid.inflated(m), starts, goals)[:4]))
    if not levels:
        return cells, count, status, cost, starts, goals, seed_margin, seed_cells2
    max_len = max([cells.shape[1]] + [lv[1][0].shape[1] for lv in levels])

    def padded(c):
        return c if c.shape[1] == max_len else torch.nn.functional.pad(c, (0, 0, 0, max_len - c.shape[1]))

    cells = padded(cells)
    for m, (l_cells, l_count, l_status, l_cost) in reversed(levels):   # ascending: the largest margin is applied last
        ok = l_status == STATUS_OK
        cells = torch.where(ok[:, None, None], padded(l_cells), cells)
        count = torch.where(ok, l_count, count)
        cost = torch.where(ok[:, None], l_cost, cost)
        status = torch.where(ok, l_status, status)
        seed_margin = torch.where(ok, torch.full_like(seed_margin, m), seed_margin)
        seed_cells2 = torch.where(ok, torch.full_like(seed_cells2, margin_cells2(m, grid.resolution)), seed_cells2)
    return cells.contiguous(), count.contiguous(), status.contiguous(), cost.contiguous(), starts, goals, seed_margin, seed_cells2


def grid_search_paths(grid, starts, goals, clearance=None):
    """-> (cells int32 [B, max_len, 2] (row, col), counts [B], status [B], costs [B, 2] = (straight, diagonal) moves).
    With a `clearance` (see grid_search_init) also seed_margin fp32 [B] at the end."""
    if clearance is None:
        return _search(grid, starts, goals)[:4]
    r = _search_with_clearance(grid, starts, goals, clearance)
    return r[:4] + r[6:7]


def seed_trajectories(grid, cells, counts, status, starts, goals, n_waypoints, init_angles_with_trajectory=False, out=None):
    """The seeding stage alone: cell paths -> [B, N, D] trajectories (reparametrize_path + initialize_angle)."""
    lib = _lib.load()
    starts, goals = as_device_points(grid, starts), as_device_points(grid, goals)
    cells, counts, status = int32_on(starts.device, cells, counts, status)
    directed = 1 if (init_angles_with_trajectory and starts.shape[1] == 3) else 0
    return seed_launch(lib.nfopp_grid_seed_workspace_bytes, lib.nfopp_grid_seed_trajectories, [cells], counts, status, starts, goals,
                       n_waypoints, (starts.shape[1], directed) + grid.origin_resolution, out)


def _shorten_paths(grid, cells, counts, status, cells2, lookahead, max_points=None):
    """shorten_paths on int32 device tensors that are already contiguous; cells2 is not looked at on the host."""
    lib = _lib.load()
    i32 = torch.int32
    dev = cells.device
    b, max_len = cells.shape[0], cells.shape[1]
    max_points = max_len if max_points is None else int(max_points)
    dist2, _ = grid.distance_transform(False)
    rows, cols = grid.shape
    anchors = torch.zeros(b, max_len, dtype=i32, device=dev)
    anchor_counts = torch.zeros(b, dtype=i32, device=dev)
    points = torch.zeros(b, max_points, 2, dtype=torch.float32, device=dev)
    point_counts = torch.zeros(b, dtype=i32, device=dev)
    _lib.check(lib.nfopp_grid_shorten_paths(
        _lib.ptr(dist2, i32), rows, cols, _lib.ptr(cells, i32), _lib.ptr(counts, i32), _lib.ptr(status, i32),
        _lib.ptr(cells2, i32), b, max_len, int(lookahead), _lib.ptr(anchors, i32), _lib.ptr(anchor_counts, i32),
        *grid.origin_resolution, max_points, _lib.ptr(points), _lib.ptr(point_counts, i32), _lib.stream_ptr()))
    return points, point_counts, anchors, anchor_counts


def shorten_paths(grid, cells, counts, status, cells2=None, lookahead=256, max_points=None):
    """Any-angle shortening of cell paths by exact line of sight (csrc/grid_any_angle.hip; the rule: include/nfopp_hip.h).
    cells int32 [B, max_len, 2], counts, status as grid_search_paths returns them; cells2 int32 [B] the threshold on the
    grid's dist2 at or below which a cell blocks the view for that problem (None = 0 everywhere: walls only); from each
    anchor the farthest cell within `lookahead` that it sees is the next.  -> (points fp32 [B, max_points, 2] xy in
    metres, point_counts [B], anchors int32 [B, max_len] indices into the cell path, anchor_counts [B]), all on the device;
    what lies behind a row's count is zero.  max_points defaults to max_len, which holds every traced path; a caller-made
    list may have more points than cells, point_counts then still reports them all.  Uses grid.distance_transform(False),
    which is computed once per grid."""
    if int(lookahead) < 1:
        raise ValueError("lookahead must be at least 1")
    dev = grid.occupancy.device
    cells, counts, status = int32_on(dev, cells, counts, status)
    if cells.dim() != 3 or cells.shape[2] != 2 or counts.shape != (cells.shape[0],) or status.shape != counts.shape:
        raise ValueError("cells must be [B, max_len, 2], counts and status [B]")
    if cells2 is not None:
        cells2, = int32_on(dev, cells2)
        if cells2.shape != counts.shape:
            raise ValueError("cells2 must be [B]")
        if bool((cells2 < 0).any()):
            raise ValueError("a threshold on dist2 must be >= 0")
    return _shorten_paths(grid, cells, counts, status, cells2, lookahead, max_points)


def seed_polylines(grid, points, point_counts, status, starts, goals, n_waypoints, init_angles_with_trajectory=False, out=None):
    """The seeding stage on given polylines: [start, the first point_counts[b] of points[b], goal] -> [B, N, D]
    trajectories, with the arithmetic of seed_trajectories (which forms the points from cell centres).  points fp32
    [B, max_len, 2] xy in metres; rows with status != 0 or a count outside 1..max_len get the straight line."""
    lib = _lib.load()
    starts, goals = as_device_points(grid, starts), as_device_points(grid, goals)
    points = torch.as_tensor(points, dtype=torch.float32, device=starts.device).contiguous()
    point_counts, status = int32_on(starts.device, point_counts, status)
    if points.dim() != 3 or points.shape[0] != starts.shape[0] or points.shape[2] != 2:
        raise ValueError("points must be [B, max_len, 2]")
    directed = 1 if (init_angles_with_trajectory and starts.shape[1] == 3) else 0
    return seed_launch(lib.nfopp_grid_seed_workspace_bytes, lib.nfopp_grid_seed_polylines, [points], point_counts, status, starts,
                       goals, n_waypoints, (starts.shape[1], directed), out)


def grid_search_init(grid, starts, goals, n_waypoints, init_angles_with_trajectory=False, out=None, clearance=None,
                     any_angle=False, lookahead=256):
    """Batched `AstarTrajectoryInitializer.initialize_trajectory`: -> (traj [B, N, D] fp32, status [B] int32), on the
    device.  status 0 = seeded along a shortest grid path; 1 = goal unreachable, 2 = start or goal outside the grid: those
    problems get the straight line of `init_trajectories`.

    `clearance` is a margin in metres or a strictly descending sequence of margins: each problem is seeded along a shortest
    path of grid.inflated(margin) for the largest margin at which that search succeeds, and on the plain grid, exactly as
    without the argument, if none does.  The start cell stays untested and the goal cell forced free on every level.  The
    call then returns (traj, status, seed_margin): seed_margin fp32 [B] is the margin each problem was seeded at, 0 for
    the plain grid.

    `any_angle`: the cell path is shortened by line of sight before the spline (shorten_paths with the given `lookahead`):
    cells between two path cells that see each other are replaced by points on the straight segment.  A cell blocks the
    view iff it is a wall of the level the problem was searched on, so a seed keeps the clearance it was found with.
    What is returned does not change; without the flag nothing changes, down to the bits."""
    if any_angle and int(lookahead) < 1:
        raise ValueError("lookahead must be at least 1")
    if clearance is None:
        cells, count, status, _, starts, goals = _search(grid, starts, goals)
        seed_margin = cells2 = None
    else:
        cells, count, status, _, starts, goals, seed_margin, cells2 = _search_with_clearance(grid, starts, goals, clearance)
    if any_angle:
        points, point_counts = _shorten_paths(grid, cells, count, status, cells2, lookahead)[:2]
        traj = seed_polylines(grid, points, point_counts, status, starts, goals, n_waypoints, init_angles_with_trajectory, out)
    else:
        traj = seed_trajectories(grid, cells, count, status, starts, goals, n_waypoints, init_angles_with_trajectory, out)
    return (traj, status) if clearance is None else (traj, status, seed_margin)


class AstarTrajectoryInitializer(object):
    """Drop-in for nfop/astar/astar_trajectory_initializer.py (same constructor, same `initialize_trajectory`); the
    search runs on the device, and BatchPlanner / ConstrainedNERFOptPlanner seed whole batches through it.  `clearance`
    (after the reference's own arguments) is grid_search_init's, as are `any_angle` and `lookahead`; `seed_margin` then holds
    the margin of each problem of the last call, all zero without a clearance."""

    def __init__(self, collision_checker, resolution=_MISSING, init_angles_with_trajectory=False, clearance=None,
                 any_angle=False, lookahead=256):
        if not hasattr(collision_checker, "check_collision") and not hasattr(collision_checker, "labels"):
            raise NotImplementedError("AstarTrajectoryInitializer rasterises its collision checker: %r offers no "
                                      "check_collision, so there is no map to search" % (collision_checker,))
        if resolution is _MISSING:   # the reference's signature has no default: a usable checker without one is a TypeError
            raise TypeError("AstarTrajectoryInitializer.__init__() missing 1 required positional argument: 'resolution'")
        self._collision_checker = collision_checker
        self._resolution = resolution
        self._init_angles_with_trajectory = init_angles_with_trajectory
        self._clearance = clearance
        self._any_angle, self._lookahead = bool(any_angle), lookahead
        self._grid = None
        self.status = None
        self.seed_margin = None

    def grid(self, boundaries=None, device=None):
        """The rasterised map (built on first use; the reference rasterises on every call, the checker is static)."""
        if self._grid is None:
            self._grid = OccupancyGrid.from_checker(self._collision_checker, self._resolution, boundaries=boundaries,
                                                    device=device)
        return self._grid

    def initialize_batch(self, starts, goals, n_waypoints, out=None, boundaries=None):
        device = out.device if out is not None else None
        traj, self.status, self.seed_margin = grid_search_init(
            self.grid(boundaries, device), starts, goals, n_waypoints, self._init_angles_with_trajectory, out=out,
            clearance=() if self._clearance is None else self._clearance, any_angle=self._any_angle,
            lookahead=self._lookahead)
        return traj

    def initialize_trajectory(self, trajectory, start_point, goal_point):
        """Host protocol of the reference: `trajectory` [N, 3] is filled in place from start_point / goal_point [1, 3]."""
        _lib.require_gpu()
        grid = self.grid(device=trajectory.device if trajectory.is_cuda else None)
        traj = self.initialize_batch(start_point[:1].detach(), goal_point[:1].detach(), trajectory.shape[0])
        with torch.no_grad():
            trajectory.copy_(traj[0, :, :trajectory.shape[1]].to(trajectory.device))
        del grid
