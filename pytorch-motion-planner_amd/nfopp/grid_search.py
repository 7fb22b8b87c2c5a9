"""Grid-search (A*) trajectory seeding for whole batches on the device (csrc/grid_search.hip).

B (start, goal) problems on one shared occupancy grid give B initial trajectories [B, N, D] with the semantics of the
reference's AstarTrajectoryInitializer (nfop/astar/astar_trajectory_initializer.py, astar/jps.py with jps=False,
utils/math.py reparametrize_path): exact minimum-cost 8-connected paths, re-sampled by a quadratic spline.  Which of
several minimum-cost paths is taken is this library's own fixed rule (include/nfopp_hip.h), not the reference's heap
order.  A problem whose goal cannot be reached is reported in `status` and seeded with the straight line."""

import numpy as np
import torch

from . import _lib
from .host_utils import Position2

STATUS_OK, STATUS_UNREACHABLE, STATUS_OUTSIDE = 0, 1, 2
RASTER_HEADING = 3 * np.pi / 4   # astar_trajectory_initializer.py:37
_MISSING = object()


def _cell_counts(boundaries, resolution):
    # astar_trajectory_initializer.py:29-30
    x_cells = int((boundaries[1] - boundaries[0]) // resolution) + 1
    y_cells = int((boundaries[3] - boundaries[2]) // resolution) + 1
    return x_cells, y_cells


def _cell_centres(boundaries, resolution):
    # astar_trajectory_initializer.py:35-37 (float64, x fastest)
    x_cells, y_cells = _cell_counts(boundaries, resolution)
    x, y = np.meshgrid(range(x_cells), range(y_cells))
    x = x.reshape(-1) * resolution + resolution / 2 + boundaries[0]
    y = y.reshape(-1) * resolution + resolution / 2 + boundaries[2]
    return x, y, x_cells, y_cells


class OccupancyGrid(object):
    """uint8 occupancy [rows = y cells, cols = x cells] (non-zero = wall) with the geometry of the reference's raster:
    cell of a point = int((x - b0) // resolution), cell centre = j * resolution + resolution / 2 + b0.

    The occupancy of a grid never changes after construction, so its distance transform (csrc/grid_edt.hip) and the images
    inflated from it are computed once and kept."""

    def __init__(self, occupancy_uint8, boundaries, resolution, device="cuda"):
        occ = np.ascontiguousarray(np.asarray(occupancy_uint8) != 0, dtype=np.uint8)
        if occ.ndim != 2 or occ.size == 0:
            raise ValueError("occupancy must be a non-empty [rows, cols] array")
        self._occupancy_host = occ
        self._shape = occ.shape
        self.boundaries = tuple(float(b) for b in boundaries)
        self.resolution = float(resolution)
        if not self.resolution > 0:
            raise ValueError("resolution must be positive")
        self.device = device
        self._occupancy_dev = None
        self._edt = {}        # border -> (dist2, nearest)
        self._inflated = {}   # (cells2, border) -> OccupancyGrid

    @classmethod
    def _from_device(cls, occupancy_dev, boundaries, resolution):
        """A grid around a uint8 0 / 1 device image; the host copy is read back only if someone asks for it."""
        grid = cls.__new__(cls)
        grid._occupancy_host = None
        grid._shape = tuple(occupancy_dev.shape)
        grid.boundaries, grid.resolution, grid.device = boundaries, resolution, occupancy_dev.device
        grid._occupancy_dev = occupancy_dev
        grid._edt, grid._inflated = {}, {}
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
        if boundaries is None:
            if hasattr(checker, "get_boundaries"):
                boundaries = checker.get_boundaries()
            else:
                boundaries = getattr(checker, "boundaries", None)
        if boundaries is None:
            raise ValueError("the checker carries no boundaries: pass boundaries=(x0, x1, y0, y1)")
        boundaries = tuple(float(b) for b in boundaries)
        x, y, x_cells, y_cells = _cell_centres(boundaries, resolution)
        if hasattr(checker, "labels") and not hasattr(checker, "check_collision"):
            dev = device or getattr(getattr(checker, "grid", None), "device", None) or \
                getattr(getattr(checker, "obstacles", None), "device", None) or "cuda"
            poses = torch.tensor(np.stack([x, y, np.full_like(x, RASTER_HEADING)], 1).astype(np.float32), device=dev)
            occ = (checker.labels(poses) > 0).to(torch.uint8).reshape(y_cells, x_cells)
            grid = cls(occ.cpu().numpy(), boundaries, resolution, dev)
            grid._occupancy_dev = occ.contiguous()
            return grid
        if not hasattr(checker, "check_collision"):
            raise TypeError("the checker offers neither check_collision nor labels")
        hit = np.asarray(checker.check_collision(Position2(x, y, np.ones_like(x) * RASTER_HEADING)))
        return cls(hit.reshape(y_cells, x_cells), boundaries, resolution, device or "cuda")

    def cells_of(self, points):
        """[B, >= 2] device points -> int32 [B, 2] (row, col); float64 floor division as the reference's `//`."""
        b = self.boundaries
        xy = points[:, :2].double()
        col = torch.floor((xy[:, 0] - b[0]) / self.resolution)
        row = torch.floor((xy[:, 1] - b[2]) / self.resolution)
        lim = float(2 ** 30)
        return torch.stack([row, col], 1).clamp_(-lim, lim).to(torch.int32).contiguous()

    def distance_transform(self, border=False):
        """-> (dist2, nearest), int32 [rows, cols] on the device (nfopp_grid_edt): the squared Euclidean distance, in cells,
        to the nearest wall cell (INT32_MAX on a grid without walls) and that cell's flat index row * cols + col, the
        smallest among equidistant ones (-1 without walls).  With `border` the cells outside the grid count as walls for
        dist2; nearest still names cells of the grid.  Computed once per `border` value."""
        border = bool(border)
        if border not in self._edt:
            lib = _lib.load()
            occ = self.occupancy
            rows, cols = self.shape
            dist2 = torch.empty(rows, cols, dtype=torch.int32, device=occ.device)
            nearest = torch.empty(rows, cols, dtype=torch.int32, device=occ.device)
            ws_bytes = lib.nfopp_grid_edt_workspace_bytes(rows, cols)
            ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=occ.device) if ws_bytes else None
            _lib.check(lib.nfopp_grid_edt(_lib.ptr(occ, torch.uint8), rows, cols, int(border), _lib.ptr(dist2, torch.int32),
                                          _lib.ptr(nearest, torch.int32), _lib.ptr(ws, torch.int32), ws_bytes, _lib.stream_ptr()))
            self._edt[border] = (dist2, nearest)
        return self._edt[border]

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


def margin_cells2(margin, resolution):
    """The threshold on dist2 for a margin in metres: floor((margin / resolution)^2 * (1 + 1e-9)).  The slack keeps a
    margin that is a whole number of cells up to the rounding of the division (0.7 / 0.1) at its square (49); dist2 is an
    integer, so it admits nothing else."""
    margin = float(margin)
    if not (margin >= 0.0 and np.isfinite(margin)):
        raise ValueError("a clearance margin must be finite and >= 0")
    q = margin / float(resolution)
    return int(np.floor(q * q * (1.0 + 1e-9)))


def _as_device_points(grid, pts):
    if not torch.is_tensor(pts):
        pts = torch.as_tensor(np.asarray(pts, np.float32))
    if not pts.is_cuda:
        _lib.require_gpu()
        pts = pts.to(grid.device)
    pts = pts.detach().float().contiguous()
    if pts.dim() != 2 or pts.shape[1] not in (2, 3):
        raise ValueError("starts / goals must be [B, 2] or [B, 3]")
    return pts


def distance_fields(grid, goal_cells):
    """goal_cells int32 [G, 2] (row, col) on the device -> int32 [G, rows, cols, 2] exact costs-to-goal (a, b);
    (-1, -1) = wall or unreachable."""
    lib = _lib.load()
    occ = grid.occupancy
    rows, cols = grid.shape
    goal_cells = goal_cells.to(torch.int32).contiguous()
    g = goal_cells.shape[0]
    fields = torch.empty(g, rows, cols, 2, dtype=torch.int32, device=occ.device)
    ws_bytes = lib.nfopp_grid_fields_workspace_bytes(rows, cols, g)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=occ.device) if ws_bytes else None
    _lib.check(lib.nfopp_grid_distance_fields(_lib.ptr(occ, torch.uint8), rows, cols, _lib.ptr(goal_cells, torch.int32), g,
                                              _lib.ptr(fields, torch.int32),
                                              _lib.ptr(ws, torch.int64) if ws is not None else None, ws_bytes,
                                              _lib.stream_ptr()))
    return fields


def _search(grid, starts, goals):
    """-> (cells [B, max_len, 2], count, status, cost, starts, goals), all on the device."""
    lib = _lib.load()
    starts, goals = _as_device_points(grid, starts), _as_device_points(grid, goals)
    if starts.shape != goals.shape:
        raise ValueError("starts and goals must have the same shape")
    rows, cols = grid.shape
    b = starts.shape[0]
    dev = starts.device
    start_cells, goal_cells = grid.cells_of(starts), grid.cells_of(goals)
    # problems that share a goal cell share a field
    inside = (goal_cells[:, 0] >= 0) & (goal_cells[:, 0] < rows) & (goal_cells[:, 1] >= 0) & (goal_cells[:, 1] < cols)
    key = torch.where(inside, goal_cells[:, 0].long() * cols + goal_cells[:, 1].long(), torch.full_like(inside, -1, dtype=torch.long))
    uniq, inverse = torch.unique(key, return_inverse=True)
    if uniq.numel() and int(uniq[0]) < 0:
        uniq, inverse = uniq[1:], inverse - 1
    field_index = inverse.to(torch.int32).contiguous()
    unique_cells = torch.stack([uniq // cols, uniq % cols], 1).to(torch.int32).contiguous()
    fields = distance_fields(grid, unique_cells) if uniq.numel() else torch.empty(0, rows, cols, 2, dtype=torch.int32, device=dev)
    count = torch.empty(b, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    cost = torch.empty(b, 2, dtype=torch.int32, device=dev)
    i32 = torch.int32

    def trace(max_len, cells):
        _lib.check(lib.nfopp_grid_trace_paths(_lib.ptr(fields, i32) if fields.numel() else None, fields.shape[0], rows, cols,
                                              _lib.ptr(start_cells, i32), _lib.ptr(goal_cells, i32), _lib.ptr(field_index, i32),
                                              b, max_len, _lib.ptr(cells, i32) if cells is not None else None,
                                              _lib.ptr(count, i32), _lib.ptr(status, i32), _lib.ptr(cost, i32), _lib.stream_ptr()))

    trace(0, None)
    max_len = max(int(count.max()) if b else 0, 1)
    cells = torch.zeros(b, max_len, 2, dtype=i32, device=dev)
    trace(max_len, cells)
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
    starts, goals = _as_device_points(grid, starts), _as_device_points(grid, goals)
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


def _seed_out(b, n_waypoints, d, dev, out):
    if out is None:
        return torch.empty(b, int(n_waypoints), d, dtype=torch.float32, device=dev)
    if out.numel() != b * int(n_waypoints) * d or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous fp32 tensor of B * N * D elements")
    return out


def seed_trajectories(grid, cells, counts, status, starts, goals, n_waypoints, init_angles_with_trajectory=False, out=None):
    """The seeding stage alone: cell paths -> [B, N, D] trajectories (reparametrize_path + initialize_angle)."""
    lib = _lib.load()
    starts, goals = _as_device_points(grid, starts), _as_device_points(grid, goals)
    b, d = starts.shape
    dev = starts.device
    i32 = torch.int32
    cells = torch.as_tensor(cells, dtype=i32, device=dev).contiguous()
    counts = torch.as_tensor(counts, dtype=i32, device=dev).contiguous()
    status = torch.as_tensor(status, dtype=i32, device=dev).contiguous()
    max_len = cells.shape[1]
    out = _seed_out(b, n_waypoints, d, dev, out)
    ws_bytes = lib.nfopp_grid_seed_workspace_bytes(b, max_len)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev) if ws_bytes else None
    bd = grid.boundaries
    _lib.check(lib.nfopp_grid_seed_trajectories(
        _lib.ptr(cells, i32), _lib.ptr(counts, i32), _lib.ptr(status, i32), b, max_len, _lib.ptr(starts), _lib.ptr(goals),
        int(n_waypoints), d, 1 if (init_angles_with_trajectory and d == 3) else 0, bd[0], bd[2], grid.resolution,
        _lib.ptr(out), _lib.ptr(ws, torch.float64) if ws is not None else None, ws_bytes, _lib.stream_ptr()))
    return out.view(b, int(n_waypoints), d)


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
    bd = grid.boundaries
    _lib.check(lib.nfopp_grid_shorten_paths(
        _lib.ptr(dist2, i32), rows, cols, _lib.ptr(cells, i32), _lib.ptr(counts, i32), _lib.ptr(status, i32),
        _lib.ptr(cells2, i32), b, max_len, int(lookahead), _lib.ptr(anchors, i32), _lib.ptr(anchor_counts, i32), bd[0], bd[2],
        grid.resolution, max_points, _lib.ptr(points), _lib.ptr(point_counts, i32), _lib.stream_ptr()))
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
    i32 = torch.int32
    dev = grid.occupancy.device
    cells = torch.as_tensor(cells, dtype=i32, device=dev).contiguous()
    counts = torch.as_tensor(counts, dtype=i32, device=dev).contiguous()
    status = torch.as_tensor(status, dtype=i32, device=dev).contiguous()
    if cells.dim() != 3 or cells.shape[2] != 2 or counts.shape != (cells.shape[0],) or status.shape != counts.shape:
        raise ValueError("cells must be [B, max_len, 2], counts and status [B]")
    if cells2 is not None:
        cells2 = torch.as_tensor(cells2, dtype=i32, device=dev).contiguous()
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
    starts, goals = _as_device_points(grid, starts), _as_device_points(grid, goals)
    b, d = starts.shape
    dev = starts.device
    i32 = torch.int32
    points = torch.as_tensor(points, dtype=torch.float32, device=dev).contiguous()
    point_counts = torch.as_tensor(point_counts, dtype=i32, device=dev).contiguous()
    status = torch.as_tensor(status, dtype=i32, device=dev).contiguous()
    if points.dim() != 3 or points.shape[0] != b or points.shape[2] != 2:
        raise ValueError("points must be [B, max_len, 2]")
    max_len = points.shape[1]
    out = _seed_out(b, n_waypoints, d, dev, out)
    ws_bytes = lib.nfopp_grid_seed_workspace_bytes(b, max_len)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev) if ws_bytes else None
    _lib.check(lib.nfopp_grid_seed_polylines(
        _lib.ptr(points), _lib.ptr(point_counts, i32), _lib.ptr(status, i32), b, max_len, _lib.ptr(starts), _lib.ptr(goals),
        int(n_waypoints), d, 1 if (init_angles_with_trajectory and d == 3) else 0, _lib.ptr(out),
        _lib.ptr(ws, torch.float64) if ws is not None else None, ws_bytes, _lib.stream_ptr()))
    return out.view(b, int(n_waypoints), d)


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
