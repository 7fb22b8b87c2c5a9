"""numpy restatement of csrc/swept.hip in float64, computed from the fp32 inputs: the distance from obstacle points to a
segment with the interior / endpoint case split of include/nfopp_hip.h, the box robot's travel bound delta and its
certificate value (through clearance_ref.distances), the path reduction of nfopp_path_swept_labels, and a brute-force
sampler of the moving box for soundness.  Checked by hand-computed cases in tests/test_swept_cpu.py; the GPU tests compare
the device with it."""
import numpy as np

import clearance_ref as cr

F32 = np.float32
SAMPLES = 65              # interpolation parameters per segment of the brute-force sampler
MAX_TURN = F32(25.1327419)   # 8 pi: SW_MAX_TURN of csrc/swept.hip


def _w(a):
    return np.asarray(a, F32).astype(np.float64)


def wrap(a):
    """(a + pi) mod 2 pi - pi, remainder with the divisor's sign (wrap_angle of csrc/common.h), float64."""
    return np.mod(np.asarray(a, np.float64) + np.pi, 2 * np.pi) - np.pi


def box_reach(box):
    """box_reach of csrc/point_cloud.h in float64: the largest corner distance, scaled up by 1.000001."""
    b = np.abs(_w(box))
    return float(np.hypot(max(b[0], b[1]), max(b[2], b[3])) * float(F32(1.000001)))


def segment_distances(a, b, points):
    """float64 [n_segments, n_points]: distance from each obstacle point to each segment [a, b] (xy of the poses):
    min(|o - a|, |o - b|, and |cross(e, o - a)| / |e| where 0 < (o - a) . e < |e|^2 strictly)."""
    a, b, o = _w(a)[:, None, :2], _w(b)[:, None, :2], _w(points).reshape(-1, 2)[None]
    e, d = b - a, o - a
    da, db = np.sqrt((d ** 2).sum(-1)), np.sqrt(((o - b) ** 2).sum(-1))
    len2 = (e ** 2).sum(-1)
    t = (d * e).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        perp = np.abs(e[..., 0] * d[..., 1] - e[..., 1] * d[..., 0]) / np.sqrt(len2)
    interior = (t > 0) & (t < len2)
    return np.minimum(np.minimum(da, db), np.where(interior, perp, np.inf))


def finite_segments(a, b, box=None):
    used = 3 if box is not None else 2
    return np.isfinite(np.asarray(a)[:, :used]).all(1) & np.isfinite(np.asarray(b)[:, :used]).all(1)


def disc_values(a, b, points, horizon=np.inf):
    """(value [n] float64, index [n]) of nfopp_swept_segments for the disc; (+inf, -1) without points, for a non-finite
    segment and above the horizon."""
    n = len(a)
    if len(np.asarray(points).reshape(-1, 2)) == 0:
        return np.full(n, np.inf), np.full(n, -1)
    ok = finite_segments(a, b)
    d = segment_distances(np.where(ok[:, None], a, 0), np.where(ok[:, None], b, 0), points)
    k = d.argmin(1)
    v = d[np.arange(n), k]
    drop = ~ok | ~(v <= horizon)
    return np.where(drop, np.inf, v), np.where(drop, -1, k)


def delta(a, b, reach):
    """|delta xy| + reach * |wrapped delta theta| per segment, float64."""
    a, b = _w(a), _w(b)
    return np.sqrt(((b[:, :2] - a[:, :2]) ** 2).sum(1)) + reach * np.abs(wrap(b[:, 2] - a[:, 2]))


def box_values(a, b, points, box, horizon=np.inf):
    """(value, index) for the box: min over points of (d_a + d_b), minus delta; -inf where delta > 4 reach or the raw fp32
    heading difference exceeds 8 pi; +inf / -1 without points, for a non-finite segment and above the horizon."""
    n = len(a)
    if len(np.asarray(points).reshape(-1, 2)) == 0:
        return np.full(n, np.inf), np.full(n, -1)
    ok = finite_segments(a, b, box)
    a0, b0 = np.where(ok[:, None], a, 0).astype(F32), np.where(ok[:, None], b, 0).astype(F32)
    reach = box_reach(box)
    s = cr.distances(a0, points, box) + cr.distances(b0, points, box)
    k = s.argmin(1)
    dl = delta(a0, b0, reach)
    v = s[np.arange(n), k] - dl
    outside = (dl > 4 * reach) | (np.abs(b0[:, 2] - a0[:, 2]) > MAX_TURN)
    v, k = np.where(outside, -np.inf, v), np.where(outside, -1, k)
    drop = ~ok | ~(v <= horizon)
    return np.where(drop, np.inf, v), np.where(drop, -1, k)


def path_reduction(poses, values, labels, threshold, box):
    """nfopp_path_swept_labels for one path: poses [m, D], values [m - 1], labels [m] -> (labels [m], status, worst value,
    worst segment)."""
    poses, values = np.asarray(poses), np.asarray(values, F32)
    labels = np.array(labels, F32)
    used = 3 if box else 2
    finite = np.isfinite(poses[:-1, :used]).all(1) & np.isfinite(poses[1:, :used]).all(1)
    certified = finite & ((values > F32(threshold)) if box else (values >= F32(threshold)))
    pose_hit = bool((labels != 0).any())
    labels[:-1][~certified] = 1.0
    if pose_hit or (not box and not certified.all()):
        status = 1
    else:
        status = 0 if certified.all() else 2
    j = int(values.argmin())
    return labels, status, values[j], j


def box_hits_along(a, b, points, box, tol):
    """bool [n_segments]: at one of SAMPLES evenly spaced interpolation parameters (theta along the wrapped difference) an
    obstacle point lies inside the box shrunk by `tol` on every edge.  float64."""
    a, b, o = _w(a), _w(b), _w(points).reshape(-1, 2)
    bx = _w(box)
    dth = wrap(b[:, 2] - a[:, 2])
    hit = np.zeros(len(a), bool)
    for s in np.linspace(0.0, 1.0, SAMPLES):
        x, y, th = a[:, 0] + s * (b[:, 0] - a[:, 0]), a[:, 1] + s * (b[:, 1] - a[:, 1]), a[:, 2] + s * dth
        dx, dy = o[None, :, 0] - x[:, None], o[None, :, 1] - y[:, None]
        c, sn = np.cos(th)[:, None], np.sin(th)[:, None]
        rx, ry = c * dx + sn * dy, c * dy - sn * dx
        inside = (rx > bx[0] + tol) & (rx < bx[1] - tol) & (ry > bx[2] + tol) & (ry < bx[3] - tol)
        hit |= inside.any(1)
    return hit
