"""numpy restatement of csrc/clearance.hip: the nearest-obstacle distance of both robot shapes in float64 (from the fp32
inputs) and the per-path statistics of nfopp_path_stats in float64 with the operation order of include/nfopp_hip.h.
Checked by hand-computed cases in tests/test_clearance_cpu.py; the GPU tests compare the device with it."""
import numpy as np

F32 = np.float32
NUM_PATH_STATS = 8
(LENGTH, MAX_CURVATURE, CURVATURE_AT, CUSPS, REVERSALS, MIN_CLEARANCE, CLEARANCE_AT, MEAN_CLEARANCE) = range(NUM_PATH_STATS)
# the longest path nfopp_path_stats serves: ps_lds_bytes(N) = 64 + 16 * ceil((N + 1) / 16) <= 160 KiB (csrc/clearance.hip)
LONGEST_PATH = 163775


def offsets(poses, points):
    """float64 (dx, dy) [n_poses, n_points] = obstacle - pose, from the fp32 values."""
    p = np.asarray(poses, F32).astype(np.float64)
    q = np.asarray(points, F32).astype(np.float64).reshape(-1, 2)
    return q[None, :, 0] - p[:, None, 0], q[None, :, 1] - p[:, None, 1]


def distances(poses, points, box=None):
    """float64 [n_poses, n_points]: |obstacle - pose| for the disc robot (box None), else the distance from the obstacle to
    the closed box (x0, x1, y0, y1; an fp32 box, widened) of a robot at pose (x, y, theta)."""
    dx, dy = offsets(poses, points)
    if box is None:
        return np.sqrt(dx * dx + dy * dy)
    th = np.asarray(poses, F32).astype(np.float64)[:, 2]
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    rx, ry = c * dx + s * dy, c * dy - s * dx
    b = np.asarray(box, F32).astype(np.float64)
    ex = np.maximum(np.maximum(b[0] - rx, rx - b[1]), 0.0)
    ey = np.maximum(np.maximum(b[2] - ry, ry - b[3]), 0.0)
    return np.sqrt(ex * ex + ey * ey)


def nearest(poses, points, box=None):
    """(min distance [n] float64, first index attaining it [n]); (+inf, -1) without points."""
    n = len(poses)
    if len(np.asarray(points).reshape(-1, 2)) == 0:
        return np.full(n, np.inf), np.full(n, -1)
    d = distances(poses, points, box)
    k = d.argmin(1)
    return d[np.arange(n), k], k


def path_stats(path, cos_cusp, pose_dist=None):
    """The 8 statistics of one path [N + 2, D] (start, waypoints, goal; fp32 values) as float64; pose_dist [M] or None.
    Every operation is a separate float64 numpy operation, in the order nfopp_path_stats states; the two sums run
    sequentially here (np.cumsum), the device sums a tree."""
    p = np.asarray(path, F32).astype(np.float64)
    out = np.zeros(NUM_PATH_STATS)
    ex, ey = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
    n = np.sqrt(ex * ex + ey * ey)
    out[LENGTH] = np.cumsum(n)[-1]
    ex0, ey0, ex1, ey1, n0, n1 = ex[:-1], ey[:-1], ex[1:], ey[1:], n[:-1], n[1:]
    cx, cy = p[2:, 0] - p[:-2, 0], p[2:, 1] - p[:-2, 1]
    chord = np.sqrt(cx * cx + cy * cy)
    both = (n0 > 0) & (n1 > 0)
    cand = both & (chord > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = (2.0 * np.abs(ex0 * ey1 - ey0 * ex1)) / ((n0 * n1) * chord)
    out[MAX_CURVATURE], out[CURVATURE_AT] = 0.0, -1
    if cand.any():
        k = np.where(cand, k, -np.inf)
        out[MAX_CURVATURE], out[CURVATURE_AT] = k.max(), int(k.argmax()) + 1      # argmax: the first maximum
    out[CUSPS] = int((both & (ex0 * ex1 + ey0 * ey1 < cos_cusp * (n0 * n1))).sum())
    if p.shape[1] == 3:
        fwd = np.cos(p[:-1, 2]) * ex + np.sin(p[:-1, 2]) * ey
        sign = np.sign(fwd[fwd != 0])
        out[REVERSALS] = int((sign[1:] != sign[:-1]).sum())
    out[MIN_CLEARANCE], out[CLEARANCE_AT], out[MEAN_CLEARANCE] = np.inf, -1, np.inf
    if pose_dist is not None:
        d = np.asarray(pose_dist, F32).astype(np.float64)
        out[MIN_CLEARANCE], out[CLEARANCE_AT] = d.min(), int(d.argmin())
        out[MEAN_CLEARANCE] = np.cumsum(d)[-1] / float(len(d))
    return out


def forward_components(path):
    """s_i of the reversal count (float64), for building fixtures that keep every |s_i| away from zero."""
    p = np.asarray(path, F32).astype(np.float64)
    ex, ey = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
    return np.cos(p[:-1, 2]) * ex + np.sin(p[:-1, 2]) * ey
