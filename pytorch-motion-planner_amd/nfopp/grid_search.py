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
    cell of a point = int((x - b0) // resolution), cell centre = j * resolution + resolution / 2 + b0."""

    def __init__(self, occupancy_uint8, boundaries, resolution, device="cuda"):
        occ = np.ascontiguousarray(np.asarray(occupancy_uint8) != 0, dtype=np.uint8)
        if occ.ndim != 2 or occ.size == 0:
            raise ValueError("occupancy must be a non-empty [rows, cols] array")
        self.occupancy_host = occ
        self.boundaries = tuple(float(b) for b in boundaries)
        self.resolution = float(resolution)
        if not self.resolution > 0:
            raise ValueError("resolution must be positive")
        self.device = device
        self._occupancy_dev = None

    @property
    def shape(self):
        return self.occupancy_host.shape

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


def grid_search_paths(grid, starts, goals):
    """-> (cells int32 [B, max_len, 2] (row, col), counts [B], status [B], costs [B, 2] = (straight, diagonal) moves)."""
    return _search(grid, starts, goals)[:4]


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
    if out is None:
        out = torch.empty(b, int(n_waypoints), d, dtype=torch.float32, device=dev)
    elif out.numel() != b * int(n_waypoints) * d or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous fp32 tensor of B * N * D elements")
    ws_bytes = lib.nfopp_grid_seed_workspace_bytes(b, max_len)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev) if ws_bytes else None
    bd = grid.boundaries
    _lib.check(lib.nfopp_grid_seed_trajectories(
        _lib.ptr(cells, i32), _lib.ptr(counts, i32), _lib.ptr(status, i32), b, max_len, _lib.ptr(starts), _lib.ptr(goals),
        int(n_waypoints), d, 1 if (init_angles_with_trajectory and d == 3) else 0, bd[0], bd[2], grid.resolution,
        _lib.ptr(out), _lib.ptr(ws, torch.float64) if ws is not None else None, ws_bytes, _lib.stream_ptr()))
    return out.view(b, int(n_waypoints), d)


def grid_search_init(grid, starts, goals, n_waypoints, init_angles_with_trajectory=False, out=None):
    """Batched `AstarTrajectoryInitializer.initialize_trajectory`: -> (traj [B, N, D] fp32, status [B] int32), on the
    device.  status 0 = seeded along a shortest grid path; 1 = goal unreachable, 2 = start or goal outside the grid: those
    problems get the straight line of `init_trajectories`."""
    cells, count, status, _, starts, goals = _search(grid, starts, goals)
    traj = seed_trajectories(grid, cells, count, status, starts, goals, n_waypoints, init_angles_with_trajectory, out)
    return traj, status


class AstarTrajectoryInitializer(object):
    """Drop-in for nfop/astar/astar_trajectory_initializer.py (same constructor, same `initialize_trajectory`); the
    search runs on the device, and BatchPlanner / ConstrainedNERFOptPlanner seed whole batches through it."""

    def __init__(self, collision_checker, resolution=_MISSING, init_angles_with_trajectory=False):
        if not hasattr(collision_checker, "check_collision") and not hasattr(collision_checker, "labels"):
            raise NotImplementedError("AstarTrajectoryInitializer rasterises its collision checker: %r offers no "
                                      "check_collision, so there is no map to search" % (collision_checker,))
        if resolution is _MISSING:   # the reference's signature has no default: a usable checker without one is a TypeError
            raise TypeError("AstarTrajectoryInitializer.__init__() missing 1 required positional argument: 'resolution'")
        self._collision_checker = collision_checker
        self._resolution = resolution
        self._init_angles_with_trajectory = init_angles_with_trajectory
        self._grid = None
        self.status = None

    def grid(self, boundaries=None, device=None):
        """The rasterised map (built on first use; the reference rasterises on every call, the checker is static)."""
        if self._grid is None:
            self._grid = OccupancyGrid.from_checker(self._collision_checker, self._resolution, boundaries=boundaries,
                                                    device=device)
        return self._grid

    def initialize_batch(self, starts, goals, n_waypoints, out=None, boundaries=None):
        device = out.device if out is not None else None
        traj, self.status = grid_search_init(self.grid(boundaries, device), starts, goals, n_waypoints,
                                             self._init_angles_with_trajectory, out=out)
        return traj

    def initialize_trajectory(self, trajectory, start_point, goal_point):
        """Host protocol of the reference: `trajectory` [N, 3] is filled in place from start_point / goal_point [1, 3]."""
        _lib.require_gpu()
        grid = self.grid(device=trajectory.device if trajectory.is_cuda else None)
        traj = self.initialize_batch(start_point[:1].detach(), goal_point[:1].detach(), trajectory.shape[0])
        with torch.no_grad():
            trajectory.copy_(traj[0, :, :trajectory.shape[1]].to(trajectory.device))
        del grid
