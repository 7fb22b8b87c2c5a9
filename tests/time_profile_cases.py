"""Paths for the time-parametrisation tests (tests/test_time_profile_cpu.py on the restatement, tests/test_gpu_time_profile.py
on the device): the hand cases and seeded random wiggly paths with folds, gear changes and repeated poses.  Every non-zero
segment keeps its forward component at least 0.5 of its length away from zero (the headings stay within 1 rad of the travel
direction or its opposite), so the device's cos / sin cannot flip a gear; a zero-length segment has an exactly zero one."""
import numpy as np

import time_profile_ref as tr

F32 = np.float32
LIMITS = tr.Limits(v_max=2.0, a_max=1.0, d_max=1.5, a_lat=1.0, w_max=1.5, cos_cusp=float(np.cos(np.pi - np.pi / 3)))
SIZES = ((1, 1), (3, 2), (2, 62), (2, 63), (2, 64), (3, 255), (1, 600))    # B x N of the device comparison
PROPERTY_N = (1, 2, 5, 62, 63, 64, 255, 600)
# (dim, N) of the longest path nfopp_path_time_profile serves: the largest m = N + 2 whose LDS image (lds_bytes below, the
# `tp_lds_bytes` of csrc/time_profile.hip restated) fits 160 KiB -- 3032 at dim 3, 3275 at dim 2
LONGEST = ((3, 3030), (2, 3273))
LONGEST_B, LONGEST_SEED = 2, 77


def lds_bytes(m, dim):
    """TP_WAVES * 16 + m * 40 + ((m * dim * 4 + 7) & ~7) + ((2 * m + 15) & ~15) with TP_WAVES = 4."""
    return 4 * 16 + m * 40 + ((m * dim * 4 + 7) & ~7) + ((2 * m + 15) & ~15)


def straight(xs, dim=2):
    """A path along the x axis through the abscissae `xs`, heading 0."""
    p = np.zeros((len(xs), dim), F32)
    p[:, 0] = xs
    return p


def wiggly(rng, n, dim, folds=True, repeats=True):
    """[n + 2, dim] fp32: a heading random walk with straight stretches and tight turns; with `folds` the travel direction
    now and then reverses at once (a cusp), with dim 3 the gear now and then changes (the heading keeps to the travel
    direction or to its opposite), with `repeats` some poses are repeated (zero-length segments)."""
    m = n + 2
    pts, heads = np.zeros((m, 2)), np.zeros(m)
    direction, gear, rate, step = rng.uniform(-np.pi, np.pi), 1, 0.0, 0.3
    for i in range(1, m):
        r = rng.uniform()
        if r < 0.15:
            rate, step = rng.choice([0.0, 0.0, 0.15, -0.15, 0.6, -0.6]), rng.choice([0.05, 0.3, 1.0])
        if folds and rng.uniform() < 0.04:
            direction += np.pi + rng.uniform(-0.3, 0.3)
        elif dim == 3 and rng.uniform() < 0.04:
            gear = -gear
        else:
            direction += rate + rng.uniform(-0.02, 0.02)
        heads[i - 1] = direction + (np.pi if gear < 0 else 0.0) + rng.uniform(-0.5, 0.5)
        length = 0.0 if (repeats and rng.uniform() < 0.05) else step * rng.uniform(0.5, 1.5)
        pts[i] = pts[i - 1] + length * np.array([np.cos(direction), np.sin(direction)])
    heads[-1] = heads[-2]
    if dim == 2:
        return pts.astype(F32)
    heads = (heads + np.pi) % (2 * np.pi) - np.pi
    return np.concatenate([pts, heads[:, None]], 1).astype(F32)


def batch(seed, b, n, dim):
    """(paths [b, n + 2, dim], v_start [b], v_goal [b]): wiggly paths; odd rows start and end moving."""
    rng = np.random.default_rng(seed)
    paths = np.stack([wiggly(rng, n, dim) for _ in range(b)])
    moving = (np.arange(b) % 2 == 1)
    return paths, np.where(moving, 0.75, 0.0).astype(F32), np.where(moving, 0.5, 0.0).astype(F32)


def forward_margin(path):
    """min over the non-zero segments of |forward component| / length (dim 3)."""
    p = np.asarray(path, F32).astype(np.float64)
    ex, ey = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
    n = np.sqrt(ex * ex + ey * ey)
    fwd = np.cos(p[:-1, 2]) * ex + np.sin(p[:-1, 2]) * ey
    return float(np.min(np.abs(fwd[n > 0]) / n[n > 0])) if (n > 0).any() else 1.0


def status_cases(dim=3):
    """[(path, v_start, v_goal, expected status)]: each status bit, and the ways a row goes out of range."""
    line = straight([0.0, 0.5, 1.0, 1.5], dim)
    nan_xy, inf_xy, far, huge = line.copy(), line.copy(), line.copy(), straight(np.arange(4) * 9.0e5, dim)
    nan_xy[2, 1], inf_xy[1, 0], far[3, 0] = np.nan, np.inf, 2.0 ** 20 + 1.5
    out = [(line, 0.0, 0.0, 0), (line, 3.0, 0.0, 1), (line, 0.0, 3.0, 2), (line, 3.0, 3.0, 3), (nan_xy, 0.0, 0.0, 4),
           (inf_xy, 0.0, 0.0, 4), (far, 0.0, 0.0, 4), (huge, 0.0, 0.0, 4), (line, np.nan, 0.0, 4), (line, 0.0, np.inf, 4),
           (line, -1.0, 0.0, 4)]
    if dim == 3:
        nan_th = line.copy()
        nan_th[1, 2] = np.nan
        out.append((nan_th, 0.0, 0.0, 4))
    return out
