"""GPU tests of csrc/swept.hip (swept check between consecutive poses, its path reduction) and of the Python layer over it:
bit identity between the all-pairs and the indexed entry, exact agreement with the nearest-obstacle query and the circle
checker, derived bounds against the float64 restatement of tests/swept_ref.py, soundness of the box certificate against a
brute-force sampler, and the planner-level wall that `evaluate()` alone drives through."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
import swept_ref as sr  # noqa: E402
import test_gpu_clearance as tgc  # noqa: E402  (its clouds, indices and poses are this file's too)
from nfopp import _lib  # noqa: E402

F32 = np.float32
EPS = 2.0 ** -24
COUNTS = tgc.COUNTS                       # 1, 255, 257, 4099: around the 256-thread workgroup
NAMES = ["one_point", "n33", "n2049_empty_quarter", "all_in_one_cell", "index_1x1", "index_64x3", "lattice", "g21_d"]
SHAPES = ("disc", "box")
INF = float("inf")
bits, dev = tgc.bits, tgc.dev


def make_segments(name):
    """4099 fp32 segments (a, b) for a cloud.  a: the poses of test_gpu_clearance (0.2 .. 1.8 radii from an obstacle point,
    inside the index region, on its border, far outside it).  b: 0 .. 4 radii from a in a random direction, the heading up to
    half a radian away and wrapped into [-pi, pi] (pairs that straddle +-pi).  Every 8th segment has zero length
    (b == a, bit for bit), every 64th -- shifted, so they are others -- a non-finite component in one of its poses."""
    scale = tgc.scale_of(name)
    a = tgc.make_poses(name, scale)
    n = len(a)
    rng = np.random.default_rng(n + 3 * len(tgc.CLOUDS[name][0]))
    length, phi = rng.uniform(0, 4 * scale, n), rng.uniform(0, 2 * np.pi, n)
    b = a.astype(np.float64)
    b[:, 0] += length * np.cos(phi)
    b[:, 1] += length * np.sin(phi)
    b[:, 2] = sr.wrap(b[:, 2] + rng.uniform(-0.5, 0.5, n))
    b = b.astype(F32)
    b[::8] = a[::8]
    bad = np.arange(5, n, 64)
    values = np.array([np.nan, np.inf, -np.inf], F32)
    for j, p in enumerate(bad):
        (a if j % 2 else b)[p, j % 3] = values[(j // 3) % 3]
    return a, b


class Entries(object):
    """Both C entries over one of test_gpu_clearance's clouds and its index."""

    def __init__(self, name):
        self.cloud = tgc.Device(name)
        self.n = self.cloud.n

    @staticmethod
    def _out(n):
        return (torch.full((n,), -5.0, device="cuda"), torch.full((n,), -5, dtype=torch.int32, device="cuda"))

    @staticmethod
    def _box(box):
        return None if box is None else (ctypes.c_float * 4)(*box)

    def brute(self, a, b, box, horizon, dim=3, check=True):
        value, index = self._out(a.shape[0])
        rc = _lib.load().nfopp_swept_segments(_lib.ptr(a), _lib.ptr(b), a.shape[0], dim, _lib.ptr(self.cloud.sorted), self.n,
                                              self._box(box), horizon, _lib.ptr(value), _lib.ptr(index, torch.int32),
                                              _lib.stream_ptr())
        if not check:
            return rc
        _lib.check(rc)
        return value.cpu().numpy(), index.cpu().numpy()

    def cells(self, a, b, box, horizon, dim=3, check=True):
        x0, y0, size, nx, ny = self.cloud.geom
        value, index = self._out(a.shape[0])
        rc = _lib.load().nfopp_swept_segments_cells(_lib.ptr(a), _lib.ptr(b), a.shape[0], dim, _lib.ptr(self.cloud.sorted),
                                                    self.n, _lib.ptr(self.cloud.start, torch.int32), nx, ny, float(x0),
                                                    float(y0), float(size), self._box(box), horizon, _lib.ptr(value),
                                                    _lib.ptr(index, torch.int32), _lib.stream_ptr())
        if not check:
            return rc
        _lib.check(rc)
        return value.cpu().numpy(), index.cpu().numpy()


_CACHE = {}


def slack_of(name):
    return float(_lib.load().nfopp_swept_slack((ctypes.c_float * 4)(*tgc.box_of(name))))


def default_horizon(name, shape):
    """What `checker.swept` uses: the smallest horizon that keeps every value the verdict can reject."""
    return tgc.scale_of(name) if shape == "disc" else slack_of(name)


def results(name, shape):
    """(entries, a, b, box, {horizon: (all-pairs (value, index), indexed (value, index))}) for the horizons +inf, the
    default (the radius / the slack) and 3 radii; computed once, shared by the tests and left unchanged."""
    key = (name, shape)
    if key not in _CACHE:
        if name not in _CACHE:
            _CACHE[name] = (Entries(name), make_segments(name))
        entries, (a, b) = _CACHE[name]
        box = tgc.box_of(name) if shape == "box" else None
        da, db = dev(a), dev(b)
        runs = {h: (entries.brute(da, db, box, h), entries.cells(da, db, box, h))
                for h in (INF, default_horizon(name, shape), 3 * tgc.scale_of(name))}
        _CACHE[key] = (entries, a, b, box, runs)
    return _CACHE[key]


def reference(name, shape):
    """The float64 restatement for the case's segments at horizon +inf, computed once."""
    key = (name, shape, "ref")
    if key not in _CACHE:
        entries, a, b, box, _ = results(name, shape)
        pts = entries.cloud.sorted_np
        _CACHE[key] = sr.disc_values(a, b, pts) if box is None else sr.box_values(a, b, pts, box)
    return _CACHE[key]


# ---- 1: the two entries, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_indexed_and_all_pairs_entries_are_bit_identical(name, shape):
    entries, a, b, box, runs = results(name, shape)
    full = runs[INF][0]
    broken = ~sr.finite_segments(a, b, box)
    spoiled = len(np.arange(5, len(a), 64))           # a third of them in the heading, which the disc does not read
    assert broken.sum() == (spoiled if shape == "box" else spoiled - len(range(2, spoiled, 3)))
    for horizon, ((bv, bi), (cv, ci)) in runs.items():
        assert np.array_equal(bits(bv), bits(cv)) and np.array_equal(bi, ci), horizon
        # the horizon only removes: what it keeps is what the uncapped run holds
        keep = full[0] <= F32(horizon)
        assert np.array_equal(bits(bv), bits(np.where(keep, full[0], F32(np.inf))))
        assert np.array_equal(bi, np.where(keep, full[1], -1))
        assert np.isposinf(bv[broken]).all() and (bi[broken] == -1).all()
        assert ((bi >= 0) == (np.isfinite(bv))).all() and (bi < max(entries.n, 1)).all()
    if entries.n == 0:
        assert np.isposinf(full[0]).all() and (full[1] == -1).all()
    elif shape == "disc":
        assert np.isfinite(full[0][~broken]).all() and full[0].min() >= 0
    else:
        assert not np.isnan(full[0]).any() and (np.isneginf(full[0]) == ((full[1] == -1) & ~broken)).all()
    horizon = default_horizon(name, shape)
    (bv, bi), _ = runs[horizon]
    for count in COUNTS[:-1]:          # every count is a launch of its own: the prefixes give the prefixes' results
        pa, pb = dev(a[:count]), dev(b[:count])
        for value, index in (entries.brute(pa, pb, box, horizon), entries.cells(pa, pb, box, horizon)):
            assert np.array_equal(bits(value), bits(bv[:count])) and np.array_equal(index, bi[:count])
    again = entries.cells(dev(a), dev(b), box, horizon)     # run to run
    assert again[0].tobytes() == bv.tobytes() and again[1].tobytes() == bi.tobytes()
    if shape == "disc":                                     # pose_dim 2: the disc needs no heading
        for value, index in (entries.brute(dev(a[:, :2]), dev(b[:, :2]), None, horizon, dim=2),
                             entries.cells(dev(a[:, :2]), dev(b[:, :2]), None, horizon, dim=2)):
            assert np.array_equal(bits(value), bits(bv)) and np.array_equal(index, bi)


# ---- 2, 3: agreement with the nearest-obstacle query and the circle checker ----------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_zero_length_segments_are_the_nearest_obstacle_query(name, shape):
    """Through the checkers (their own index, the entry `swept` picks).  Disc: distance and index of `nearest`, bit for bit.
    Box: d_a + d_a - 0 is exactly twice `nearest`'s distance, and doubling keeps the order, so the index is the same."""
    _, a, b, box, _ = results(name, shape)
    pts = tgc.CLOUDS[name][0]
    checker = nfopp.DeviceCircleChecker(pts, tgc.scale_of(name)) if box is None else nfopp.DeviceRectangleChecker(pts, box)
    assert (checker.cells is None) == (len(pts) < checker.INDEX_FROM)
    zero = (bits(a) == bits(b)).all(1) & sr.finite_segments(a, b, box)
    assert zero.sum() >= len(a) // 8 - 70
    value, index = (t.cpu().numpy() for t in checker.swept(dev(a), dev(b), horizon=INF))
    dist, near = (t.cpu().numpy() for t in checker.nearest(dev(a)))
    want = dist if box is None else F32(2) * dist
    assert np.array_equal(bits(value[zero]), bits(want[zero])) and np.array_equal(index[zero], near[zero])
    # the default horizon is the smallest that decides: the radius, and the slack for the box -- what the verdict
    # rejects (value < radius; value <= slack) is kept, so the cap never turns an uncertified segment into +inf
    capped, none = checker.swept(dev(a), dev(b), index_out=False)
    capped = capped.cpu().numpy()
    threshold = F32(checker.radius if box is None else checker.swept_slack)
    assert none is None and (box is None or checker.swept_slack == slack_of(name) > 0)
    keep = value <= threshold
    assert np.array_equal(bits(capped), bits(np.where(keep, value, F32(np.inf))))
    certified = (capped >= threshold) if box is None else (capped > threshold)
    assert np.array_equal(certified, (value >= threshold) if box is None else (value > threshold))
    assert not certified[value <= threshold].any() if box is not None else not certified[value < threshold].any()


@pytest.mark.parametrize("name", NAMES)
def test_disc_value_is_at_most_the_nearest_distance_of_either_end(name):
    entries, a, b, _, runs = results(name, "disc")
    value = runs[INF][0][0]
    ok = sr.finite_segments(a, b)
    na, nb = entries.cloud.brute(dev(a), None)[0], entries.cloud.brute(dev(b), None)[0]
    assert (value[ok] <= np.minimum(na, nb)[ok]).all()
    radius = tgc.scale_of(name)
    checker = nfopp.DeviceCircleChecker(tgc.CLOUDS[name][0], radius, None)
    hit = (checker.labels(dev(a)).cpu().numpy() != 0) | (checker.labels(dev(b)).cpu().numpy() != 0)
    assert (value[hit & ok] < F32(radius)).all()
    if entries.n:
        assert hit[ok].mean() >= 0.1 and (~hit[ok]).mean() >= 0.1, hit[ok].mean()


# ---- 4: the disc against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_disc_value_against_float64(name):
    """|value - ref| <= 32 eps (|o* - a| + |e|), eps = 2^-24, o* the reference's nearest point.  Count, for a point at d = o - a
    of a segment e: the end terms are within 3 eps relative (test_gpu_clearance).  cross = fma(ex, dy, -(ey dx)): ex, ey,
    dx, dy are rounded differences, eps relative each, so either product carries 2 eps and their difference 2 eps |e| |d|
    (Cauchy-Schwarz); the product's and the fma's own roundings add eps |e| |d| each: 4 eps |e| |d|.  |e| = sqrt(fma(ex, ex,
    ey ey)): 4 eps relative on the square, so 2 eps, and the root's rounding: 3 eps.  The quotient: 4 eps |d| + 3 eps perp +
    eps perp <= 8 eps |d|.  The case split: fp32 and float64 may disagree on `interior` when the projection is within
    4 eps (|d| + |e|) of an end, and there the perpendicular and the end term differ by no more than that.  Together
    12 eps (|d| + |e|) for one point.  The device's nearest point kf need not be o*: min_f <= f(o*) <= ref + err(o*) and
    min_f = f(kf) >= ref(kf) - err(kf) >= ref - err(kf), with |kf - a| <= |o* - a| + |e| (up to the error itself), so
    err(kf) <= 12 eps (|o* - a| + 2 |e|) <= 24 eps (|o* - a| + |e|).  24 counted, 32 asserted.
    The label `value < radius` must equal the reference's wherever the reference is farther than that bound from the
    radius; at most 0.5 % of the segments may be that close, and swept-only hits -- an obstacle inside the swept disc,
    both end poses free -- must be present: both sides of the new predicate are populated."""
    entries, a, b, _, runs = results(name, "disc")
    if entries.n == 0:
        return
    value = runs[INF][0][0].astype(np.float64)
    ref, k = reference(name, "disc")
    ok = sr.finite_segments(a, b)
    pts = entries.cloud.sorted_np.astype(np.float64)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    size = np.zeros(len(a))
    size[ok] = np.sqrt(((pts[k[ok]] - a64[ok, :2]) ** 2).sum(1)) + np.sqrt(((b64[ok, :2] - a64[ok, :2]) ** 2).sum(1))
    err = np.abs(value[ok] - ref[ok])
    print("disc %s: max |value - ref| / (eps (|o* - a| + |e|)) = %.3f" % (name, float((err / (EPS * size[ok])).max())))
    assert (err <= 32 * EPS * size[ok]).all()
    radius = tgc.scale_of(name)
    decided = ok & (np.abs(ref - float(F32(radius))) > 32 * EPS * size)
    excluded = 1.0 - decided[ok].mean()
    assert np.array_equal(value[decided] < float(F32(radius)), ref[decided] < float(F32(radius)))
    ends = np.minimum(sr.disc_values(a, a, pts)[0], sr.disc_values(b, b, pts)[0])
    swept_only = ok & (ref < radius) & (ends >= radius)
    print("disc %s: excluded %.5f, swept-only hits %.4f, hits %.4f" % (name, excluded, swept_only[ok].mean(), (ref[ok] < radius).mean()))
    assert excluded <= 0.005
    # populated on every cloud; a share of a hundredth at least on the three whose points are a few radii apart
    assert swept_only.sum() >= 3 and (ref[ok] >= radius).mean() >= 0.1
    assert swept_only[ok].mean() >= 0.01 or name not in ("n33", "n2049_empty_quarter", "index_64x3")


# ---- 5, 6, 7: the box certificate ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_box_certificate_is_two_sided_and_sound(name):
    """Against the reference value with a margin of 2 slack either way (the header's count bounds the device's rounding by
    189 / 256 slack while delta <= 4 reach; the reference forms the reach in float64, 13 / 256 slack more), then against
    the brute-force sampler: nothing the device certifies has an obstacle inside the box (shrunk by 2^-20 reach) at any of
    65 poses along the segment.  The inputs must populate both sides, by the reference alone."""
    entries, a, b, box, runs = results(name, "box")
    if entries.n == 0:
        return
    slack = float(_lib.load().nfopp_swept_slack((ctypes.c_float * 4)(*box)))
    reach = sr.box_reach(box)
    assert abs(slack - reach * 2.0 ** -16) <= 2.0 ** -22 * slack
    ok = sr.finite_segments(a, b, box)
    ref, _ = reference(name, "box")
    assert (sr.delta(a[ok], b[ok], reach) < 3.95 * reach).all() and not np.isneginf(ref).any()
    for horizon, ((value, _), _) in runs.items():
        certified = ok & (value > F32(slack))
        assert certified[ok & (ref > 2 * slack)].all(), horizon
        assert not certified[ok & (ref < -2 * slack)].any(), horizon
    default = runs[default_horizon(name, "box")][0][0]
    certified = ok & (default > F32(slack))
    # at the default horizon the verdict is the uncapped one: nothing with a value <= slack comes back certified
    full = runs[INF][0][0]
    assert np.array_equal(certified, ok & (full > F32(slack))) and (default[ok & (full <= F32(slack))] <= F32(slack)).all()
    pts = entries.cloud.sorted_np
    assert not sr.box_hits_along(a[certified], b[certified], pts, box, 2.0 ** -20 * reach).any()
    share = (ref[ok] > 2 * slack).mean()
    print("box %s: certified by the reference %.4f, swept through by the sampler %.4f"
          % (name, share, sr.box_hits_along(a[ok], b[ok], pts, box, 0.0).mean()))
    assert share >= 0.1 and (ref[ok] <= 0).mean() >= 0.1


def test_a_box_value_inside_the_slack_is_undecided_at_the_default_horizon():
    """The unit box driven 0.5 along x towards a point g = slack / 4 beyond where its front ends up: d_a = 0.5 + g, d_b = g,
    delta = 0.5, value = 2 g -- positive, and within the rounding allowance.  The default horizon must keep it, or the
    reduction would read +inf and certify a segment that the header calls undecided."""
    box = (-1.0, 1.0, -1.0, 1.0)
    checker = nfopp.DeviceRectangleChecker(np.array([[0.0, 9.0]], F32), box)
    slack = checker.swept_slack
    assert 0 < slack < 1e-4
    checker.update_obstacle_points(np.array([[1.5 + slack / 4, 0.0]], F32))
    poses = dev(np.array([[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.5, 0.0, 0.0]]], F32))
    assert not checker.labels(poses.view(3, 3)).cpu().numpy().any()
    value, index = checker.swept(poses[0, :-1], poses[0, 1:])
    value = value.cpu().numpy()
    # the second segment has zero length: 2 d_b, the same 2 g; coordinates near 1.5 carry 2^-23, a few of them add up
    assert (0 < value).all() and (value <= F32(slack)).all() and index.cpu().tolist() == [0, 0]
    assert (np.abs(value - slack / 2) <= 2.0 ** -21).all()
    labels = torch.zeros(3, device="cuda")
    status, worst = torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(1, 2, device="cuda")
    checker.swept_labels(poses, dev(value.reshape(1, 2)), labels, status, worst)
    assert status.cpu().tolist() == [2] and labels.cpu().tolist() == [1.0, 1.0, 0.0] and 0 < worst.cpu().numpy()[0, 0] <= F32(slack)
    # a horizon of 0 would have hidden it
    assert np.isposinf(checker.swept(poses[0, :-1], poses[0, 1:], horizon=0.0)[0].cpu().numpy()[0])


# ---- 8: edge cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_edge_cases(shape):
    entries, a, b, box, runs = results("n33", shape)
    (bv, bi), _ = runs[INF]
    lib = _lib.load()
    cloud = entries.cloud
    # n = 0: a no-op that touches nothing
    assert lib.nfopp_swept_segments(None, None, 0, 3, _lib.ptr(cloud.sorted), cloud.n, None, 1.0, None, None, _lib.stream_ptr()) == 0
    # n_obstacles = 0 through both entries
    empty = Entries("g21_d")
    pa, pb = dev(a[:300]), dev(b[:300])
    for value, index in (empty.brute(pa, pb, box, INF), empty.cells(pa, pb, box, INF)):
        assert np.isposinf(value).all() and (index == -1).all()
    # index_dev may be null
    value = torch.empty(300, device="cuda")
    _lib.check(lib.nfopp_swept_segments(_lib.ptr(pa), _lib.ptr(pb), 300, 3, _lib.ptr(cloud.sorted), cloud.n, Entries._box(box),
                                        INF, _lib.ptr(value), None, _lib.stream_ptr()))
    assert np.array_equal(bits(value.cpu().numpy()), bits(bv[:300]))
    # bad arguments
    for horizon in (-1.0, float("nan")):
        assert entries.brute(pa, pb, box, horizon, check=False) == -1 and entries.cells(pa, pb, box, horizon, check=False) == -1
    unit = (-1.0, 1.0, -1.0, 1.0)
    assert entries.brute(dev(a[:300, :2]), dev(b[:300, :2]), unit, 1.0, dim=2, check=False) == -1
    assert entries.cells(dev(a[:300, :2]), dev(b[:300, :2]), unit, 1.0, dim=2, check=False) == -1
    if shape == "box":   # a turn of more than 8 pi between two poses, and poses more than 4 reaches apart: no certificate
        wide = b[:300].copy()
        wide[0, 2] = a[0, 2] + 26.0
        wide[1, :2] = a[1, :2] + 5 * sr.box_reach(box)
        ok = sr.finite_segments(a[:2], wide[:2], box)
        assert ok.all()
        for value, index in (entries.brute(pa, dev(wide), box, INF), entries.cells(pa, dev(wide), box, INF)):
            assert np.isneginf(value[:2]).all() and (index[:2] == -1).all()
            assert np.array_equal(bits(value[2:]), bits(bv[2:300]))


@pytest.mark.parametrize("box", [False, True])
def test_path_reduction_equals_the_restatement(box):
    """B = 5 paths of m = 259 poses (two strides of the workgroup and a remainder): every status, a tie for the worst value,
    a non-finite pose, +inf everywhere."""
    rng = np.random.default_rng(41 + box)
    B, m, D = 5, 259, 3 if box else 2
    threshold = 0.25
    poses = rng.uniform(-1, 1, (B, m, D)).astype(F32)
    values = rng.uniform(0.3, 2.0, (B, m - 1)).astype(F32)
    labels = np.zeros((B, m), F32)
    values[1, 200], values[1, 77] = 0.1, 0.1          # not certified, twice: the first index wins
    values[2, 257] = threshold                        # on the threshold: certified for the disc, not for the box
    labels[3, m - 1] = 1.0                            # only the last pose collides
    values[4] = np.inf
    poses[4, 100, D - 1] = np.nan
    lib = _lib.load()
    d_poses, d_values = dev(poses), dev(values)       # held: a temporary's memory is handed to the next allocation
    got = dev(labels.reshape(-1))
    status = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    worst = torch.full((B, 2), -7.0, device="cuda")
    _lib.check(lib.nfopp_path_swept_labels(_lib.ptr(d_poses), _lib.ptr(d_values), _lib.ptr(got), B, m, D, threshold,
                                           int(box), _lib.ptr(status, torch.uint8), _lib.ptr(worst), _lib.stream_ptr()))
    got, status, worst = got.cpu().numpy().reshape(B, m), status.cpu().numpy(), worst.cpu().numpy()
    for p in range(B):
        want, st, wv, wj = sr.path_reduction(poses[p], values[p], labels[p], threshold, box)
        assert np.array_equal(got[p], want) and status[p] == st and worst[p, 1] == wj, p
        assert np.array_equal(bits(worst[p, :1]), bits(np.array([wv], F32)))
    assert list(status) == ([0, 2, 2, 1, 2] if box else [0, 1, 0, 1, 1])
    assert worst[1, 1] == 77 and worst[4, 1] == 0 and np.isposinf(worst[4, 0])
    # status and worst may be null: the labels are the same
    again = dev(labels.reshape(-1))
    _lib.check(lib.nfopp_path_swept_labels(_lib.ptr(d_poses), _lib.ptr(d_values), _lib.ptr(again), B, m, D, threshold,
                                           int(box), None, None, _lib.stream_ptr()))
    assert np.array_equal(again.cpu().numpy().reshape(B, m), got)
    assert lib.nfopp_path_swept_labels(_lib.ptr(d_poses), _lib.ptr(d_values), _lib.ptr(again), B, m, 2,
                                       threshold, 1, None, None, _lib.stream_ptr()) == -1


@pytest.mark.parametrize("m", [2, 65, 257, 600])
@pytest.mark.parametrize("box", [False, True])
def test_path_reduction_across_wave_and_stride_boundaries(box, m):
    """The same reduction with fewer poses than one wave, a count that ends inside the second wave, one pose beyond a stride
    of the workgroup and more than two strides: the worst value tied in the middle and in the last segment, the only segment
    that is not certified at the far end, only the last pose in collision."""
    rng = np.random.default_rng(47 + m)
    B, D = 4, 3 if box else 2
    threshold = 0.25
    poses = rng.uniform(-1, 1, (B, m, D)).astype(F32)
    values = rng.uniform(0.3, 2.0, (B, m - 1)).astype(F32)
    labels = np.zeros((B, m), F32)
    values[1, m - 2], values[1, (m - 2) // 2] = 0.1, 0.1
    values[2, m - 2] = 0.2
    labels[3, m - 1] = 1.0
    lib = _lib.load()
    d_poses, d_values = dev(poses), dev(values)
    got = dev(labels.reshape(-1))
    status = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    worst = torch.full((B, 2), -7.0, device="cuda")
    _lib.check(lib.nfopp_path_swept_labels(_lib.ptr(d_poses), _lib.ptr(d_values), _lib.ptr(got), B, m, D, threshold,
                                           int(box), _lib.ptr(status, torch.uint8), _lib.ptr(worst), _lib.stream_ptr()))
    got, status, worst = got.cpu().numpy().reshape(B, m), status.cpu().numpy(), worst.cpu().numpy()
    for p in range(B):
        want, st, wv, wj = sr.path_reduction(poses[p], values[p], labels[p], threshold, box)
        assert np.array_equal(got[p], want) and status[p] == st and worst[p, 1] == wj, p
        assert np.array_equal(bits(worst[p, :1]), bits(np.array([wv], F32)))
    assert list(status) == ([0, 2, 2, 1] if box else [0, 1, 1, 1])
    assert worst[1, 1] == (m - 2) // 2 and worst[2, 1] == m - 2


# ---- 9 - 12: the planner and the wall ------------------------------------------------------------------------------------
RADIUS = 0.3
SMALL_BOX = (-0.25, 0.25, -0.15, 0.15)            # reach 0.292: the poses, 1 apart, are inside the certificate's domain
WALL = np.stack([np.zeros(61), np.linspace(-3.0, 3.0, 61)], 1)   # a one-cell wall along x = 0, points 0.1 apart


def wall_planner(D):
    """B = 3 straight paths of N = 8 waypoints, 10 poses 1 apart along x from -4.5 to 4.5 (sub = 1: the dense poses are the
    waypoints).  Trajectory 0 crosses the wall at y = 0 with its nearest poses 0.5 either side of it (1.67 radii; 1.7
    reaches of the box), trajectory 1 runs 2 beyond the wall's end, trajectory 2 is trajectory 0 at y = 1 with one waypoint
    pushed into the wall."""
    torch.random.manual_seed(5)
    onf = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=D == 3).to("cuda")
    x = -4.5 + np.arange(10.0)
    paths = np.zeros((3, 10, D), F32)
    paths[:, :, 0] = x
    paths[1, :, 1], paths[2, :, 1] = 5.0, 1.0
    paths[2, 5, 0] = 0.05
    bounds = (-6.0, 6.0, -6.0, 6.0)
    planner = nfopp.BatchPlanner(onf, 3, 8, nfopp.TrajectoryHyper(bounds=bounds))
    planner.init(paths[:, 0], paths[:, -1], bounds, trajectories=paths[:, 1:-1])
    checker = nfopp.DeviceCircleChecker(WALL, RADIUS, bounds) if D == 2 else nfopp.DeviceRectangleChecker(WALL, SMALL_BOX, bounds)
    assert checker.cells is not None                  # 61 points: the indexed entries
    return planner, checker, paths


def state(planner, result):
    return [t.clone().cpu().numpy().tobytes() for t in (planner.best_traj, planner.best_length) + tuple(result)]


@pytest.mark.parametrize("D", [2, 3])
def test_a_path_through_a_one_cell_wall(D):
    planner, checker, paths = wall_planner(D)
    dist = np.abs(paths[0, :, 0])
    assert dist.min() >= 1.5 * (RADIUS if D == 2 else sr.box_reach(SMALL_BOX))
    # 9: the sampled poses see nothing
    plain = planner.evaluate(checker, sub=1)
    assert plain[0].cpu().tolist() == [0, 0, 1]
    assert np.isfinite(planner.best_length.cpu().numpy()).tolist() == [True, True, False]
    # 12: swept=False is the call without the argument, byte for byte
    before = state(planner, plain)
    assert state(planner, planner.evaluate(checker, sub=1)) == before
    assert state(planner, planner.evaluate(checker, sub=1, swept=False)) == before
    # 11: certify() leaves the bookkeeping alone
    status, worst = planner.certify(checker, sub=1)
    assert state(planner, plain) == before
    status, worst = status.cpu().numpy(), worst.cpu().numpy()
    assert status.tolist() == ([1, 0, 1] if D == 2 else [2, 0, 1])
    assert worst[0, 1] == 4                            # poses 4 and 5, at x = -0.5 and 0.5
    if D == 2:
        assert worst[0, 0] == 0.0 and worst[2, 0] < RADIUS and np.isposinf(worst[1, 0])
    else:
        assert worst[0, 0] <= checker.swept_slack and np.isposinf(worst[1, 0])
    # 10: with swept=True trajectory 0 is no longer free, its best length stays inf and the early stop leaves it running
    planner, checker, _ = wall_planner(D)
    for _ in range(2):
        collides, length = planner.evaluate(checker, sub=1, early_stop=True, swept=True)
        assert collides.cpu().tolist() == [1, 0, 1]
    assert np.isfinite(planner.best_length.cpu().numpy()).tolist() == [False, True, False]
    assert planner.engine.active.cpu().tolist() == [1, 0, 1]
    assert np.array_equal(planner.best_traj.cpu().numpy()[1], paths[1, 1:-1])
    # the early stop without it retires the path that crosses the wall
    planner, checker, _ = wall_planner(D)
    for _ in range(2):
        planner.evaluate(checker, sub=1, early_stop=True)
    assert planner.engine.active.cpu().tolist() == [0, 0, 1]
    # it composes with a clearance margin: 4 is more than trajectory 1 keeps from the wall's end
    collides, _ = planner.evaluate(checker, sub=1, swept=True, min_clearance=4.0)
    assert collides.cpu().tolist() == [1, 1, 1]


def test_the_grid_checker_has_no_swept_check():
    grid = nfopp.DeviceGridChecker(np.zeros((8, 8), np.uint8), 0.0, 0.0, 0.5)
    with pytest.raises(NotImplementedError, match="DeviceCircleChecker"):
        grid.swept(torch.zeros(4, 3, device="cuda"), torch.zeros(4, 3, device="cuda"))
    planner, _, _ = wall_planner(2)
    with pytest.raises(NotImplementedError):
        planner.evaluate(grid, sub=1, swept=True)
    with pytest.raises(NotImplementedError):
        planner.certify(grid, sub=1)
