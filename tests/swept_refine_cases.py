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


STAGE = 1024                                              # RF_STAGE of csrc/swept.hip: candidates a wave keeps in LDS
BEYOND = ((512, 512, 512), (500, 500, 536), (1100, 200, 200))   # points per row of cells, below


def beyond_the_stage(rows):
    """A cloud over a 3 x 3 index of unit cells from (0, 0) with rows[r] points in row r of cells, and 320 segments with both
    ends in the centre cell: with one further cell per side every segment's window is the whole index and every point is a
    candidate, in sorted order, so candidate 1024 -- the first a wave does not keep in LDS -- lies between two rows, inside
    the last row and inside the first one.  Rows 0 and 1 lie below y = 1.5 and the top row's filler in its first cell beyond
    y = 2.6, all out of the box's reach (reach + delta <= 5 reach = 0.31) of the segments, which run under the top of the
    centre cell with a turn, y in [1.88, 2); the 120 points that decide them lie over them in [1, 2) x [2, 2.3], the last 32
    segments slide 1e-4 under one of those.  The cloud is dense enough for test_gpu_clearance.scale_of to give its floor.
    -> (name the cloud is registered under while in use, points, geometry, box, a, b, {max_depth: restatement}), computed
    once.  Asserted here, without a GPU: the cloud exceeds the stage; every deciding point is a candidate beyond it; the
    restatement over the first 1024 sorted points alone answers at least 20 segments differently, none of them ambiguous, so
    a walk that dropped the unstaged candidates is caught; free, hit and undecided occur; 20 segments are decided below the
    root."""
    key = ("beyond", rows)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(sum(rows))
    decide = np.stack([rng.uniform(1.0, 1.999, 120), rng.uniform(2.0, 2.3, 120)], 1)
    filler = np.stack([rng.uniform(0.0, 0.6, rows[2] - 120), rng.uniform(2.6, 2.95, rows[2] - 120)], 1)
    low = [np.stack([rng.uniform(0.0, 2.999, n), rng.uniform(r + 0.05, r + 0.5, n)], 1) for r, n in enumerate(rows[:2])]
    points = rng.permutation(np.concatenate(low + [filler, decide])).astype(F32)
    geom = (F32(0), F32(0), F32(1), 3, 3)
    name = "beyond_%d_%d_%d" % rows
    tgc.CLOUDS[name] = (points, geom)          # scale_of and box_of read the cloud by name, as tgc.Device does
    try:
        box = tgc.box_of(name)
    finally:
        del tgc.CLOUDS[name]
    assert box == tgc.box_of("all_in_one_cell")            # the floor: 0.05
    n, graze = 320, 32
    a = np.stack([rng.uniform(1.05, 1.7, n), rng.uniform(1.88, 1.995, n), rng.uniform(-0.4, 0.4, n)], 1)
    length, phi = rng.uniform(0.05, 0.23, n), rng.uniform(-0.3, 0.3, n)
    b = np.stack([a[:, 0] + length * np.cos(phi), np.minimum(a[:, 1] + length * np.sin(phi), 1.998),
                  a[:, 2] + rng.uniform(-0.5, 0.5, n)], 1)
    under = decide[(decide[:, 1] < 2.03) & (decide[:, 0] > 1.1) & (decide[:, 0] < 1.9)]
    under = under[rng.integers(0, len(under), graze)].astype(F32).astype(np.float64)
    a[-graze:] = np.stack([under[:, 0] - 0.08, under[:, 1] - box[3] - 1e-4, np.zeros(graze)], 1)
    b[-graze:] = a[-graze:] + np.array([0.16, 0.0, 0.0])
    a, b = a.astype(F32), b.astype(F32)
    pts = tgc.omr.cell_index(points, *geom)[0]
    deciding = np.flatnonzero((pts[:, 1] >= 2.0) & (pts[:, 1] <= F32(2.3)))
    assert len(pts) > STAGE and len(deciding) == 120 and deciding.min() >= STAGE
    assert (np.floor(a[:, :2]) == 1).all() and (np.floor(b[:, :2]) == 1).all()
    idle = np.delete(pts, deciding, 0)
    assert sr.segment_distances(a, b, idle).min() > 5.01 * sr.box_reach(box)
    refs = {d: rr.refine(a, b, pts, box, d) for d in (0, 3, 8)}
    status, _, depth, ambiguous = refs[8]
    staged_only = rr.refine(a, b, pts[:STAGE], box, 8)[0]
    assert ((staged_only != status) & ~ambiguous).sum() >= 20
    assert set(status[~ambiguous]) == {rr.FREE, rr.HIT, rr.UNDECIDED}
    assert ((depth >= 1) & (status != rr.UNDECIDED) & ~ambiguous).sum() >= 20
    _CACHE[key] = (name, points, geom, box, a, b, refs)
    return _CACHE[key]


def reference(name, kind, max_depth=8, node_budget=1024):
    """(status, s, depth, ambiguous) of the restatement, computed once and left unchanged."""
    key = (name, kind, max_depth, node_budget)
    if key not in _CACHE:
        a, b = segments(name, kind)
        _CACHE[key] = rr.refine(a, b, sorted_points(name), tgc.box_of(name), max_depth, node_budget)
    return _CACHE[key]
