"""The inputs the GPU tests of nfopp_swept_refine run on, and the float64 restatement's answers for them, computed once per
process: the eight clouds of tests/test_gpu_clearance.py, the 4099 segments of tests/test_gpu_swept.py per cloud ("short":
0 .. 4 radii long) and a second set per cloud whose lengths are 4 .. 16 radii ("long": beyond 4 reaches for most, so the
certificate's domain rule bites).  No GPU is needed to build them: tests/test_swept_refine_cpu.py asserts on these very
inputs that few segments are ambiguous and that enough of them are decided below the root."""
import numpy as np

import swept_ref as sr
import swept_refine_ref as rr
import test_gpu_clearance as tgc
import test_gpu_swept as tgs

F32 = np.float32
NAMES = tgs.NAMES
KINDS = ("short", "long")
DENSE = ("all_in_one_cell", "lattice")   # clouds whose points are closer together than the box is wide (below)
_CACHE = {}


def corner_clipping(name, kind, count, rng):
    """`count` segments that pass a corner of a DENSE cloud's bounding rectangle tangentially: closest to the corner point,
    at 0.3 .. 1.6 radii from it, at a parameter uniform in [0.1, 0.9], 3 .. 4 (short) or 4 .. 16 (long) radii long, heading
    along the travel direction +- 0.3 rad.  On a dense cloud a box anywhere over the points holds one of them, so random
    segments are free or hit at an end pose or at the root's midpoint and next to none is decided below the root (0.2 %
    and 0.6 % of make_segments' and of the plain long set); past a corner the box covers points for a short window only."""
    pts = tgc.CLOUDS[name][0].astype(np.float64)
    scale = tgc.scale_of(name)
    signs = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], np.float64)
    which = rng.integers(0, 4, count)
    normal = signs[which] / np.sqrt(2.0)
    corner = pts[(pts @ signs.T).argmax(0)][which]
    tangent = np.stack([-normal[:, 1], normal[:, 0]], 1) * rng.choice([-1.0, 1.0], (count, 1))
    lo, hi = (3, 4) if kind == "short" else (4, 16)
    length, at = rng.uniform(lo * scale, hi * scale, count), rng.uniform(0.1, 0.9, count)
    near = corner + normal * rng.uniform(0.3, 1.6, (count, 1)) * scale
    heading = np.arctan2(tangent[:, 1], tangent[:, 0])
    a = np.concatenate([near - tangent * (length * at)[:, None], sr.wrap(heading + rng.uniform(-0.3, 0.3, count))[:, None]], 1)
    b = np.concatenate([near + tangent * (length * (1 - at))[:, None], sr.wrap(heading + rng.uniform(-0.3, 0.3, count))[:, None]], 1)
    return a.astype(F32), b.astype(F32)


def segments(name, kind):
    """(a, b) fp32 [4099, 3].  "long": a as in the short set, b 4 .. 16 radii away in a random direction, the heading up to
    half a radian away and wrapped; the short set's zero-length and non-finite segments are not repeated.  On the two DENSE
    clouds every 8th segment of the long set (3, 11, ...) and every 4th of the short one (3, 7, 11, ...) is replaced by one of
    `corner_clipping`; the zero-length (0, 8, ...) and the non-finite (5, 69, ...) ones stay."""
    key = (name, kind, "segments")
    if key not in _CACHE:
        a, b = tgs.make_segments(name)
        if kind == "long":
            scale = tgc.scale_of(name)
            n = len(a)
            a = tgc.make_poses(name, scale)
            rng = np.random.default_rng(7 * n + len(tgc.CLOUDS[name][0]))
            length, phi = rng.uniform(4 * scale, 16 * scale, n), rng.uniform(0, 2 * np.pi, n)
            b = a.astype(np.float64)
            b[:, 0] += length * np.cos(phi)
            b[:, 1] += length * np.sin(phi)
            b[:, 2] = sr.wrap(b[:, 2] + rng.uniform(-0.5, 0.5, n))
            b = b.astype(F32)
        if name in DENSE:
            a, b = a.copy(), b.copy()
            step = 4 if kind == "short" else 8
            a[3::step], b[3::step] = corner_clipping(name, kind, len(a[3::step]), np.random.default_rng(len(a) + step))
        _CACHE[key] = (a, b)
    return _CACHE[key]


def sorted_points(name):
    """The cloud in the order of its cell index: what both entries are given."""
    key = (name, "points")
    if key not in _CACHE:
        pts, geom = tgc.CLOUDS[name]
        _CACHE[key] = tgc.omr.cell_index(pts, *geom)[0]
    return _CACHE[key]


def reference(name, kind, max_depth=8, node_budget=1024):
    """(status, s, depth, ambiguous) of the restatement, computed once and left unchanged."""
    key = (name, kind, max_depth, node_budget)
    if key not in _CACHE:
        a, b = segments(name, kind)
        _CACHE[key] = rr.refine(a, b, sorted_points(name), tgc.box_of(name), max_depth, node_budget)
    return _CACHE[key]
