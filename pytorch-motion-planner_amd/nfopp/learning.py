"""Continuous ONF learning for a batch of trajectories, entirely on the device: ground-truth checkers, training-pose
generation, retained-pool resampling (csrc/sampling.hip) and the data-parallel fitting step (batch.OnfFitter).

Reference semantics (one trajectory, host numpy): nfop/nerf_opt_planner.py:76-141.  Per step and per trajectory the
sample set is  N-1 "course" poses + the retained pool (<= 100 poses kept by weighted resampling) + `random_field_points`
uniform poses; labels come from the ground-truth checker; all trajectories of all ranks fit ONE shared field.
Differences to the reference, by construction of the batch: the pool holds min(100, N-1) poses and is full from the
first step (the reference grows it for N <= 100), and draws come from a counter-based Philox stream instead of
numpy's global generator (distributional parity, SURVEY.md "Hard parts").
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._grid import workspace


def _f4(values):
    return (ctypes.c_float * 4)(*[float(v) for v in values])


def _as_points(points, device):
    """`points` (numpy array or tensor, anything that reshapes to [n, 2]) as an fp32 [n, 2] tensor on `device`."""
    if isinstance(points, torch.Tensor):
        return points.detach().to(device=device, dtype=torch.float32).reshape(-1, 2).contiguous()
    return torch.tensor(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2), device=device)


class DeviceGridMap(object):
    """Occupancy grid on the device (nfop/ros/grid_map.py).  `data` [rows, cols] is the fp32 image of `GridMap` (a cell is
    occupied above `threshold`) or, through `from_occupancy_data`, the raw int8 image of a ROS OccupancyGrid; `origin` =
    (x, y, theta) of the map frame.  The point cloud is built by nfopp_grid_to_points in float64 like the reference's and
    handed to the checkers as fp32; reading its size back is the one host synchronisation per map."""

    def __init__(self, data, resolution, origin=(0.0, 0.0, 0.0), threshold=0.5, device="cuda"):
        if isinstance(data, torch.Tensor):
            raw = data.dtype == torch.int8
            self._map = data.detach().to(device=device, dtype=torch.int8 if raw else torch.float32).contiguous()
        else:
            data = np.asarray(data)
            raw = data.dtype == np.int8
            self._map = torch.tensor(np.ascontiguousarray(data, dtype=np.int8 if raw else np.float32), device=device)
        if self._map.dim() != 2:
            raise ValueError("the map is a [rows, cols] image")
        self._raw = raw
        self._resolution, self._threshold = float(resolution), float(threshold)
        self._origin = tuple(float(v) for v in origin)
        self._points = self._points64 = None

    @classmethod
    def from_occupancy_data(cls, int8_data, width, height, resolution, origin, device="cuda"):
        """`GridMap.from_ros_occupancy_grid` (grid_map.py:31-40) without the message: `int8_data` is OccupancyGrid.data
        (row-major, -1 unknown, 0..100 occupancy percent); the unpacking happens in the kernel."""
        if isinstance(int8_data, torch.Tensor):
            data = int8_data.to(torch.int8).reshape(int(height), int(width))
        else:
            data = np.asarray(int8_data).astype(np.int8).reshape(int(height), int(width))
        return cls(data, resolution, origin, device=device)

    def _build(self):
        rows, cols = self._map.shape
        x, y, theta = self._origin
        c, s = float(np.cos(theta)), float(np.sin(theta))   # the calls Position2.apply makes
        lib, grid = _lib.load(), _lib.ptr(self._map, self._map.dtype)
        count = torch.zeros(1, dtype=torch.int32, device=self._map.device)

        def run(max_points, p32, p64):
            _lib.check(lib.nfopp_grid_to_points(grid, int(self._raw), rows, cols, self._threshold, self._resolution, x, y,
                                                c, s, max_points, _lib.ptr(p32), _lib.ptr(p64, torch.float64),
                                                _lib.ptr(count, torch.int32), _lib.stream_ptr()))
        run(0, None, None)
        n = int(count.item())
        self._points = torch.empty(n, 2, dtype=torch.float32, device=self._map.device)
        self._points64 = torch.empty(n, 2, dtype=torch.float64, device=self._map.device)
        if n:
            run(n, self._points, self._points64)

    def as_point_cloud(self, dtype=torch.float32):
        """Device tensor [n, 2] of the occupied cells' centres in row-major cell order (cached); fp32 is the rounding of
        the float64 cloud (`dtype=torch.float64`), which equals the reference's."""
        if self._points is None:
            self._build()
        return self._points64 if dtype == torch.float64 else self._points

    @property
    def boundaries(self):
        rows, cols = self._map.shape   # grid_map.py:22-29
        left, bottom = self._origin[0], self._origin[1]
        return left, left + cols * self._resolution, bottom, bottom + rows * self._resolution


class _PointCloudChecker(object):
    """What the two point-cloud checkers share: the obstacle set, its cell index and the reference's update interface
    (nfop/collision_checker/collision_checker.py:21-28).  With INDEX_FROM points or more the points are sorted into a
    uniform cell index on the device (nfopp_build_cell_index; cell >= the robot's reach) and every pose tests the points
    of its 3 x 3 cells only: same predicate, same labels.  `cells` = (cell_start, nx, ny, x0, y0, size) or None."""

    def _setup(self, obstacle_points, boundaries, device):
        self.device, self.boundaries = device, boundaries
        self.update_obstacle_points(obstacle_points)

    def update_obstacle_points(self, points):
        """Replaces the obstacle set by `points` [n, 2] (numpy array or device tensor) and rebuilds the index."""
        pts = _as_points(points, self.device)
        n, reach = pts.shape[0], self._reach()
        self.cells, self.obstacles = None, pts
        if n < self.INDEX_FROM or n == 0 or not reach > 0:
            return
        lo, hi = (v.cpu().numpy() for v in torch.aminmax(pts, dim=0))   # fp32; the geometry is fixed on the host
        # a little more than the reach: fp32 rounding of the cell arithmetic must not move a point two cells away
        size = np.float32(max(reach * 1.001, float((hi - lo).max()) / 64.0))
        nx, ny = (int(np.floor((hi[k] - lo[k]) / size)) + 1 for k in (0, 1))
        lib = _lib.load()
        ws = workspace(lib.nfopp_cell_index_workspace_bytes(n), pts.device)
        ordered = torch.empty_like(pts)
        start = torch.empty(nx * ny + 1, dtype=torch.int32, device=pts.device)
        _lib.check(lib.nfopp_build_cell_index(_lib.ptr(pts), n, float(lo[0]), float(lo[1]), float(size), nx, ny,
                                              _lib.ptr(ordered), _lib.ptr(start, torch.int32), ws.ptr, ws.nbytes,
                                              _lib.stream_ptr()))
        self.obstacles = ordered
        self.cells = (start, nx, ny, float(lo[0]), float(lo[1]), float(size))

    def update_boundaries(self, boundaries):
        self.boundaries = boundaries

    def get_boundaries(self):
        return self.boundaries

    def _cloud_args(self):
        """What every C entry over the obstacle set takes after the poses: points, count and, with an index, its six
        parameters (CellIndex of csrc/point_cloud.h)."""
        index = () if self.cells is None else (_lib.ptr(self.cells[0], torch.int32),) + tuple(self.cells[1:])
        return (_lib.ptr(self.obstacles), self.obstacles.shape[0]) + index

    _box = None   # the rectangle checker's (x0, x1, y0, y1); None = disc robot

    def nearest(self, poses, out=None, index_out=None):
        """(dist [n] fp32, index [n] int32) of the nearest obstacle point per pose (nfopp_nearest_obstacle[_cells]): for the
        disc the distance to the robot's origin, the very number `labels` compares with the radius; for the box the
        distance to the closed box, 0 inside it.  `index` points into `self.obstacles` (cell-sorted once an index exists),
        the smallest index among equidistant points; +inf / -1 without obstacles.  The bounds play no part."""
        n, d = poses.shape
        dist = torch.empty(n, dtype=torch.float32, device=poses.device) if out is None else out
        index = torch.empty(n, dtype=torch.int32, device=poses.device) if index_out is None else index_out
        box = _f4(self._box) if self._box is not None else None
        lib = _lib.load()
        entry = lib.nfopp_nearest_obstacle if self.cells is None else lib.nfopp_nearest_obstacle_cells
        _lib.check(entry(_lib.ptr(poses), n, d, *self._cloud_args(), box, _lib.ptr(dist), _lib.ptr(index, torch.int32),
                         _lib.stream_ptr()))
        return dist, index

    def clearance(self, poses, out=None):
        """Free space around the robot's footprint at each pose [n] fp32: max(dist - radius, 0) for the disc (fp32 torch ops
        on the device), the distance to the box itself for the rectangle.  0 where `labels` reports an obstacle."""
        dist, _ = self.nearest(poses, out=out)
        if self._box is None:
            torch.sub(dist, self.radius, out=dist).clamp_(min=0)
        return dist

    swept_slack = 0.0   # the rectangle checker's rounding allowance (nfopp_swept_slack); the disc's test is exact

    def swept(self, poses_a, poses_b, horizon=None, out=None, index_out=None):
        """(value [n] fp32, index [n] int32) per segment poses_a[p] -> poses_b[p] (nfopp_swept_segments[_cells]; x, y linear,
        theta along the wrapped difference).  Disc: the exact distance from the nearest obstacle point to the segment, so
        `value < radius` is the swept collision test.  Box: min (d_a + d_b) - delta, a certificate -- `value > swept_slack`
        proves the whole segment free, anything else with free end poses is undecided (-inf: the poses are too far apart to
        certify at all).  A value above `horizon` comes back as +inf / -1; the default, the radius for the disc and
        `swept_slack` for the box, is the smallest that decides the verdicts: every value the comparison can reject is
        kept.  `index_out=False` skips the index (None is returned for it).  Leading dimensions are flattened; views
        are copied."""
        d = poses_a.shape[-1]
        a, b = poses_a.reshape(-1, d).contiguous(), poses_b.reshape(-1, d).contiguous()
        if a.shape != b.shape:
            raise ValueError("swept() needs as many start poses as end poses")
        n = a.shape[0]
        if horizon is None:
            horizon = self.radius if self._box is None else self.swept_slack
        value = torch.empty(n, dtype=torch.float32, device=a.device) if out is None else out
        if index_out is False:
            index = None
        else:
            index = torch.empty(n, dtype=torch.int32, device=a.device) if index_out is None else index_out
        box = _f4(self._box) if self._box is not None else None
        lib = _lib.load()
        entry = lib.nfopp_swept_segments if self.cells is None else lib.nfopp_swept_segments_cells
        _lib.check(entry(_lib.ptr(a), _lib.ptr(b), n, d, *self._cloud_args(), box, float(horizon), _lib.ptr(value),
                         _lib.ptr(index, torch.int32), _lib.stream_ptr()))
        return value, index

    def swept_labels(self, poses, values, labels, status=None, worst=None):
        """nfopp_path_swept_labels for `poses` [B, m, D], `values` [B, m - 1] of `swept` and the `labels` [B * m] this
        checker wrote: marks, in place, the first pose of every segment that is not certified."""
        B, m, d = poses.shape
        threshold = self.radius if self._box is None else self.swept_slack
        _lib.check(_lib.load().nfopp_path_swept_labels(_lib.ptr(poses), _lib.ptr(values), _lib.ptr(labels), B, m, d,
                                                       float(threshold), int(self._box is not None),
                                                       _lib.ptr(status, torch.uint8), _lib.ptr(worst), _lib.stream_ptr()))
        return labels

    def update_from_map(self, grid_map, extra_points=None):
        """One sensor message (`CollisionCheckerAdapter._callback`, nfop/ros/collision_checker_adapter.py:17-27): the
        sensor's points first, then the map's, and the boundaries from the map."""
        pts = grid_map.as_point_cloud()
        if extra_points is not None:
            pts = torch.cat([_as_points(extra_points, pts.device), pts], 0)
        self.update_obstacle_points(pts)
        self.update_boundaries(grid_map.boundaries)


class DeviceCircleChecker(_PointCloudChecker):
    """Disc robot against a point cloud + bounds (nfop/collision_checker/circle_collision_checker.py)."""

    INDEX_FROM = 32   # obstacle points from which the cell index pays

    def __init__(self, obstacle_points, robot_radius, boundaries=None, device="cuda"):
        self.radius = float(robot_radius)
        self._setup(obstacle_points, boundaries, device)

    def _reach(self):
        return self.radius

    def labels(self, poses, out=None):
        n, d = poses.shape
        out = torch.empty(n, dtype=torch.float32, device=poses.device) if out is None else out
        b = _f4(self.boundaries) if self.boundaries is not None else None
        lib = _lib.load()
        entry = lib.nfopp_check_collision_circle if self.cells is None else lib.nfopp_check_collision_circle_cells
        _lib.check(entry(_lib.ptr(poses), n, d, *self._cloud_args(), self.radius, b, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def swept_refine(self, poses_a, poses_b, max_depth=8, node_budget=1024, status_out=None, s_out=None, depth_out=None):
        raise NotImplementedError("the disc's swept() is already exact (value < radius is the swept collision test): "
                                  "there is nothing to refine; swept_refine is DeviceRectangleChecker's")


class DeviceRectangleChecker(_PointCloudChecker):
    """Box robot (x0, x1, y0, y1 in its own frame) against a point cloud (rectangle_collision_checker.py)."""

    INDEX_FROM = 48   # obstacle points from which the cell index pays: the measured crossover (profiles/obstacle_map.txt)

    def __init__(self, obstacle_points, box, boundaries=None, device="cuda"):
        self.box = self._box = tuple(float(v) for v in box)
        self.swept_slack = float(_lib.load().nfopp_swept_slack(_f4(self.box)))
        self._setup(obstacle_points, boundaries, device)

    def _reach(self):
        """Largest distance from the robot origin to a corner of the box (the box need not contain the origin); `box_reach`
        of csrc/point_cloud.h is its C counterpart (fp32, rounded up)."""
        x0, x1, y0, y1 = self.box
        return float(np.hypot(max(abs(x0), abs(x1)), max(abs(y0), abs(y1))))

    def labels(self, poses, out=None):
        n = poses.shape[0]
        out = torch.empty(n, dtype=torch.float32, device=poses.device) if out is None else out
        b = _f4(self.boundaries) if self.boundaries is not None else None
        lib = _lib.load()
        if self.cells is None:
            _lib.check(lib.nfopp_check_collision_rectangle(_lib.ptr(poses), n, *self._cloud_args(), _f4(self.box), b,
                                                           _lib.ptr(out), _lib.stream_ptr()))
        else:
            _lib.check(lib.nfopp_check_collision_rectangle_cells(_lib.ptr(poses), n, *self._cloud_args(), _f4(self.box),
                                                                 self._reach(), b, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def swept_refine(self, poses_a, poses_b, max_depth=8, node_budget=1024, status_out=None, s_out=None, depth_out=None):
        """(status [n] uint8, s [n] fp32, depth [n] uint8) per segment poses_a[p] -> poses_b[p] (nfopp_swept_refine[_cells]):
        the certificate of `swept` on dyadic pieces of the segment and `labels`' predicate at their midpoints, in pre-order,
        down to `max_depth` (0 .. 20) and for at most `node_budget` (>= 1) piece and midpoint tests per segment.  status 0 =
        proven free, 1 = a pose of the motion has an obstacle point inside the box, at parameter `s` (0 and 1: the end
        poses; the first hit in pre-order, -1 without one), 2 = undecided; `depth` = the deepest level tested.
        `s_out=False` / `depth_out=False` skip that output (None is returned for it).  Leading dimensions are flattened;
        views are copied.  Nothing synchronises."""
        d = poses_a.shape[-1]
        a, b = poses_a.reshape(-1, d).contiguous(), poses_b.reshape(-1, d).contiguous()
        if a.shape != b.shape:
            raise ValueError("swept_refine() needs as many start poses as end poses")
        n = a.shape[0]

        def output(given, dtype, what):
            """A fresh [n] tensor, or the caller's once it is known to hold n elements of `dtype` on the poses' device."""
            if given is None:
                return torch.empty(n, dtype=dtype, device=a.device)
            if not (isinstance(given, torch.Tensor) and given.dtype == dtype and given.device == a.device
                    and given.numel() == n and given.is_contiguous()):
                raise ValueError("%s must be a contiguous %s tensor of %d elements on %s, got %s"
                                 % (what, dtype, n, a.device, _lib._describe(given)))
            return given
        status = output(status_out, torch.uint8, "status_out")
        s = None if s_out is False else output(s_out, torch.float32, "s_out")
        depth = None if depth_out is False else output(depth_out, torch.uint8, "depth_out")
        lib = _lib.load()
        entry = lib.nfopp_swept_refine if self.cells is None else lib.nfopp_swept_refine_cells
        _lib.check(entry(_lib.ptr(a), _lib.ptr(b), n, d, *self._cloud_args(), _f4(self.box), int(max_depth), int(node_budget),
                         _lib.ptr(status, torch.uint8), _lib.ptr(s), _lib.ptr(depth, torch.uint8), _lib.stream_ptr()))
        return status, s, depth

    def refined_labels(self, seg_status, seg_s, labels, status=None, first=None):
        """nfopp_path_refined_labels for `seg_status`, `seg_s` [B, m - 1] of `swept_refine` and the `labels` [B * m] this
        checker wrote: marks, in place, the first pose of every segment that is not proven free."""
        B, m = seg_status.shape[0], seg_status.shape[1] + 1
        if seg_s.shape != seg_status.shape or labels.numel() != B * m:
            raise ValueError("refined_labels() needs seg_s of seg_status' shape [B, m - 1] and B * m labels")
        if (status is not None and status.numel() != B) or (first is not None and first.numel() != 2 * B):
            raise ValueError("refined_labels() writes B path statuses and [B, 2] first segments")
        _lib.check(_lib.load().nfopp_path_refined_labels(_lib.ptr(seg_status, torch.uint8), _lib.ptr(seg_s), _lib.ptr(labels),
                                                         B, m, _lib.ptr(status, torch.uint8), _lib.ptr(first),
                                                         _lib.stream_ptr()))
        return labels


class DeviceGridChecker(object):
    """uint8 occupancy image (MapCollisionChecker of notebooks/onf_planner_image_map.ipynb cell 2)."""

    def __init__(self, grid, origin_x, origin_y, cell_size, device="cuda"):
        self.grid = torch.tensor(np.ascontiguousarray(grid, dtype=np.uint8), device=device)
        self.origin_x, self.origin_y, self.cell_size = float(origin_x), float(origin_y), float(cell_size)

    def labels(self, poses, out=None):
        n, d = poses.shape
        out = torch.empty(n, dtype=torch.float32, device=poses.device) if out is None else out
        _lib.check(_lib.load().nfopp_check_collision_grid(_lib.ptr(poses), n, d, _lib.ptr(self.grid, torch.uint8),
                                                          self.grid.shape[0], self.grid.shape[1], self.origin_x,
                                                          self.origin_y, self.cell_size, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def clearance(self, poses, out=None):
        raise NotImplementedError("clearance needs a point cloud: use DeviceCircleChecker or DeviceRectangleChecker "
                                  "(the occupancy image has no nearest-obstacle query)")

    def swept(self, poses_a, poses_b, horizon=None, out=None, index_out=None):
        raise NotImplementedError("the swept check needs a point cloud: use DeviceCircleChecker or DeviceRectangleChecker "
                                  "(DeviceGridMap.as_point_cloud gives the occupancy image's)")

    def swept_refine(self, poses_a, poses_b, max_depth=8, node_budget=1024, status_out=None, s_out=None, depth_out=None):
        raise NotImplementedError("the swept check needs a point cloud: use DeviceRectangleChecker "
                                  "(DeviceGridMap.as_point_cloud gives the occupancy image's)")


class BatchSampler(object):
    """Per-trajectory training-pose generation with a retained pool, for B trajectories on one GPU."""

    def __init__(self, onf, batch, n_waypoints, course_sigma=1.5, fine_sigma=0.02, angle_sigma=0.0, n_field=10,
                 pool_cap=100, device="cuda", seed=0, traj_index_offset=0):
        self.onf, self.B, self.N, self.D = onf, int(batch), int(n_waypoints), onf.point_dim
        self.cap = min(int(pool_cap), self.N - 1)
        self.n_field = int(n_field)
        self.sigmas = (float(course_sigma), float(fine_sigma), float(angle_sigma))
        self.seed, self.offset, self.traj_index_offset = int(seed), 0, int(traj_index_offset)
        f32 = dict(dtype=torch.float32, device=device)
        B, N, D = self.B, self.N, self.D
        self.C = self.cap + N - 1
        self.S = (N - 1) + self.cap + self.n_field
        self.pool = torch.zeros(B, self.cap, D, **f32)
        self.pool_age = torch.zeros(B, self.cap, **f32)
        self.pool_full = False
        self.cand = torch.zeros(B, self.C, D, **f32)
        self.cand_age = torch.zeros(B, self.C, **f32)
        self.cand_out = torch.zeros(B, self.C, 4, **f32)
        self.samples = torch.zeros(B, self.S, D, **f32)
        self.labels = torch.zeros(B * self.S, **f32)

    def draw(self, prev_traj, bounds):
        """Fills `self.samples` [B, S, D] from the previous trajectories [B, N, D]; returns it flattened [B*S, D]."""
        lib = _lib.load()
        pool_n = self.cap if self.pool_full else 0
        n_cand = pool_n + self.N - 1
        course, fine, angle = self.sigmas
        _lib.check(lib.nfopp_sample_candidates(_lib.ptr(prev_traj), self.B, self.N, self.D, self.cap, pool_n, self.n_field,
                                               course, fine, angle, _f4(bounds), self.seed, self.offset,
                                               self.traj_index_offset, _lib.ptr(self.pool), _lib.ptr(self.pool_age),
                                               _lib.ptr(self.cand), _lib.ptr(self.cand_age), _lib.ptr(self.samples),
                                               _lib.stream_ptr()))
        if self.cap:
            cfg = self.onf.config_c()   # weights of the pool candidates: sigmoid(ONF) * exp(-0.03 age)  (nerf:124-126)
            _lib.check(lib.nfopp_onf_eval_logits(cfg, _lib.ptr(self.onf.flat_parameters), _lib.ptr(self.cand),
                                                 self.B * self.C, _lib.ptr(self.cand_out), _lib.stream_ptr()))
            _lib.check(lib.nfopp_resample_pool(self.B, n_cand, self.C, self.cap, self.D, self.S, self.N - 1, self.seed, self.offset,
                                               self.traj_index_offset, _lib.ptr(self.cand), _lib.ptr(self.cand_age),
                                               _lib.ptr(self.cand_out), _lib.ptr(self.pool), _lib.ptr(self.pool_age),
                                               _lib.ptr(self.samples), _lib.stream_ptr()))
            self.pool_full = True
        self.offset += 1
        return self.samples.view(self.B * self.S, self.D)
