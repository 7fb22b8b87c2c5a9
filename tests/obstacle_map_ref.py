"""numpy restatement of the obstacle-map path (csrc/obstacle_map.hip, the *_cells checkers of csrc/sampling.hip): the
point cloud of an occupancy grid, the cell index over a point set and the two point-cloud predicates.  Pinned to the
reference by tests/golden/g21_obstacle_map.npz (tests/test_obstacle_map_cpu.py); the GPU tests compare the device with it.
"""
import numpy as np

F32 = np.float32


def grid_points(data, resolution, origin, threshold=0.5):
    """float64 [n, 2]: centres of the occupied cells in row-major order, moved by the origin pose (x, y, theta).  `data`
    is the fp32 image or, as int8, the raw ROS image (-1 unknown -> 0, then percent / 100 in fp32)."""
    data = np.asarray(data)
    if data.dtype == np.int8:
        data = np.where(data < 0, 0, data).astype(F32) / F32(100)
    occupied = data.astype(F32) > F32(threshold)
    rows, cols = np.nonzero(occupied)
    res = float(resolution)
    x, y = cols * res + res / 2.0, rows * res + res / 2.0
    c, s = np.cos(origin[2]), np.sin(origin[2])
    return np.stack([x * c - y * s + origin[0], x * s + y * c + origin[1]], 1).reshape(-1, 2)


def grid_boundaries(shape, resolution, origin):
    rows, cols = shape
    return origin[0], origin[0] + cols * resolution, origin[1], origin[1] + rows * resolution


def rectangle_reach(box):
    return float(np.hypot(max(abs(box[0]), abs(box[1])), max(abs(box[2]), abs(box[3]))))


def index_geometry(points, reach):
    """(x0, y0, size, nx, ny) of the checkers' cell index over fp32 points: min / max of the points, cell =
    max(1.001 reach, extent / 64)."""
    pts = np.asarray(points, F32).reshape(-1, 2)
    lo, hi = pts.min(0), pts.max(0)
    size = F32(max(reach * 1.001, float((hi - lo).max()) / 64.0))
    nx, ny = (int(np.floor((hi[k] - lo[k]) / size)) + 1 for k in (0, 1))
    return F32(lo[0]), F32(lo[1]), size, nx, ny


def cell_ids(points, x0, y0, size, nx, ny):
    """The kernels' cell arithmetic: fp32 subtract, divide, floor, clamp."""
    pts = np.asarray(points, F32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((pts[:, 0] - F32(x0)) / F32(size))
        fy = np.floor((pts[:, 1] - F32(y0)) / F32(size))
    cx = np.clip(fx, 0, nx - 1).astype(np.int64)
    cy = np.clip(fy, 0, ny - 1).astype(np.int64)
    return cy * nx + cx


def cell_index(points, x0, y0, size, nx, ny):
    """(points sorted stably by cell, cell_start [nx * ny + 1] int32)."""
    pts = np.asarray(points, F32).reshape(-1, 2)
    cell = cell_ids(pts, x0, y0, size, nx, ny)
    order = np.argsort(cell, kind="stable")
    start = np.searchsorted(cell[order], np.arange(nx * ny + 1)).astype(np.int32)
    return pts[order], start


def out_of_bounds(xy, bounds):
    if bounds is None:
        return np.zeros(len(xy), bool)
    return (xy[:, 0] > bounds[1]) | (xy[:, 0] < bounds[0]) | (xy[:, 1] > bounds[3]) | (xy[:, 1] < bounds[2])


def circle_labels(poses, points, radius, bounds=None, dtype=np.float64):
    """Disc robot: any |pose.xy - point| < radius, or out of bounds."""
    xy = np.asarray(poses, dtype)[:, :2]
    pts = np.asarray(points, dtype).reshape(-1, 2)
    hit = np.zeros(len(xy), bool)
    for k in range(0, len(xy), 1024):
        d = np.linalg.norm(xy[k:k + 1024, None] - pts[None], axis=2)
        hit[k:k + 1024] = (d < radius).any(1)
    return hit | out_of_bounds(xy, bounds)


def robot_frame(poses, points, dtype=np.float64):
    """Obstacle points in each pose's frame: [n_poses, n_points] x and y."""
    p = np.asarray(poses, dtype)
    pts = np.asarray(points, dtype).reshape(-1, 2)
    dx, dy = pts[None, :, 0] - p[:, None, 0], pts[None, :, 1] - p[:, None, 1]
    c, s = np.cos(p[:, 2])[:, None], np.sin(p[:, 2])[:, None]
    return c * dx + s * dy, c * dy - s * dx


def rectangle_labels(poses, points, box, bounds=None, dtype=np.float64):
    """Box robot (x0, x1, y0, y1 in its frame): any point strictly inside the box, or out of bounds."""
    p = np.asarray(poses, dtype)
    hit = np.zeros(len(p), bool)
    for k in range(0, len(p), 1024):
        rx, ry = robot_frame(p[k:k + 1024], points, dtype)
        hit[k:k + 1024] = ((rx > box[0]) & (rx < box[1]) & (ry > box[2]) & (ry < box[3])).any(1)
    return hit | out_of_bounds(p[:, :2], bounds)
