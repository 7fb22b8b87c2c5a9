"""GPU tests of csrc/clearance.hip (nearest-obstacle query, per-path statistics) and of the Python layer over it, against
the numpy restatement in tests/clearance_ref.py, the ground-truth checkers and each other.  Bit identity between the
all-pairs and the indexed entry, exact agreement with the checkers' labels, derived bounds against float64.

Measured on an MI355X: the whole file takes 3.5 s; the four cases at the longest path nfopp_path_stats serves take at most
0.04 s each, their paths (built once per dimension) included."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import clearance_ref as cr  # noqa: E402
import nfopp  # noqa: E402
import obstacle_map_ref as omr  # noqa: E402
from nfopp import _lib  # noqa: E402

F32 = np.float32
EPS = 2.0 ** -24
WORKGROUP = 256                                    # NR_THREADS of csrc/clearance.hip
COUNTS = (1, WORKGROUP - 1, WORKGROUP + 1, 4099)
UNIT_BOX = np.array([-0.85, 1.0, -0.675, 0.675])   # scaled per cloud; the robot's origin is off-centre


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def dev(a, dtype=F32):
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


# ---- clouds, indices, poses ------------------------------------------------------------------------------------------
def make_clouds():
    """name -> (points fp32 [n, 2], (x0, y0, size, nx, ny)).  Built once (CLOUDS)."""
    rng = np.random.default_rng(2024)
    g21 = load_golden("g21_obstacle_map.npz")
    out = {}

    def own_geometry(pts, reach=0.3):
        return omr.index_geometry(pts, reach) if len(pts) else (F32(0), F32(0), F32(1), 1, 1)
    one = rng.uniform(2, 3, (1, 2)).astype(F32)
    out["one_point"] = (one, own_geometry(one))
    p33 = rng.uniform(0, 10, (nfopp.DeviceCircleChecker.INDEX_FROM + 1, 2)).astype(F32)
    out["n33"] = (p33, own_geometry(p33))
    # 2049 points (one over a workgroup's share of the index build) on an L: the quarter [15, 30]^2 is empty
    ell = rng.uniform(0, 30, (6000, 2))
    ell = ell[~((ell[:, 0] > 15) & (ell[:, 1] > 15))][:2049].astype(F32)
    out["n2049_empty_quarter"] = (ell, own_geometry(ell))
    out["all_in_one_cell"] = (rng.uniform(4.01, 4.99, (500, 2)).astype(F32), (F32(0), F32(0), F32(1), 9, 7))
    out["index_1x1"] = (rng.uniform(0, 5, (200, 2)).astype(F32), (F32(0), F32(0), F32(10), 1, 1))
    out["index_64x3"] = (rng.uniform([0, 0], [64, 3], (700, 2)).astype(F32), (F32(0), F32(0), F32(1), 64, 3))
    lattice = np.stack(np.meshgrid(np.arange(12.0), np.arange(9.0)), -1).reshape(-1, 2)
    out["lattice"] = (rng.permutation(lattice).astype(F32), (F32(-0.25), F32(-0.25), F32(1.5), 8, 6))
    dup = rng.uniform(0, 8, (150, 2)).astype(F32)
    out["duplicated"] = (np.concatenate([dup, dup[::-1]]), own_geometry(dup))
    for m in "abcde":
        pts = g21[m + "_cloud"].astype(F32)
        out["g21_" + m] = (pts, own_geometry(pts))
    return out


CLOUDS = make_clouds()
assert len(CLOUDS["n2049_empty_quarter"][0]) == 2049 and len(CLOUDS["g21_d"][0]) == 0


def region_of(name):
    pts, (x0, y0, size, nx, ny) = CLOUDS[name]
    lo = np.array([x0, y0], np.float64)
    return lo, lo + np.array([nx, ny]) * float(size)


def make_poses(name, scale):
    """4099 fp32 poses [x, y, theta] for a cloud, shuffled so that every prefix mixes the kinds: inside the index region, on
    its border, 100 extents outside it (the search must reach the last ring), over twice the region (empty cells, the
    L's empty quarter) and -- so that both sides of the checkers' predicates are well populated -- within 0.2 .. 1.8
    `scale` of an obstacle point."""
    pts = CLOUDS[name][0]
    rng = np.random.default_rng(len(pts) + 17)
    lo, hi = region_of(name)
    ext = hi - lo
    inside = rng.uniform(lo, hi, (700, 2))
    border = rng.uniform(lo, hi, (400, 2))
    side = rng.integers(0, 4, 400)
    border[side == 0, 0], border[side == 1, 0] = lo[0], hi[0]
    border[side == 2, 1], border[side == 3, 1] = lo[1], hi[1]
    far = (lo + hi) / 2 + rng.choice([-100.0, 0.0, 100.0], (300, 2)) * ext + rng.uniform(-1, 1, (300, 2)) * ext
    far[0] = (lo + hi) / 2 + 100 * ext
    wide = rng.uniform(lo - ext / 2, hi + ext / 2, (699, 2))
    if name == "n2049_empty_quarter":
        wide[:300] = rng.uniform(16.5, 29.5, (300, 2))
    n_near = 4099 - 700 - 400 - 300 - 699
    if len(pts):
        ang, rad = rng.uniform(0, 2 * np.pi, n_near), rng.uniform(0.2, 1.8, n_near) * scale
        near = pts[rng.integers(0, len(pts), n_near)] + np.stack([np.cos(ang), np.sin(ang)], 1) * rad[:, None]
    else:
        near = rng.uniform(lo, hi, (n_near, 2))
    xy = np.concatenate([inside, border, far, wide, near])
    if name == "lattice":   # midpoints of lattice edges and of lattice squares: 2 and 4 points at exactly the same distance
        xy[:300] = rng.integers(0, 8, (300, 2)) + 0.5
        xy[300:500] = rng.integers(0, 8, (200, 2)) + np.array([0.5, 0.0])
    poses = np.concatenate([xy, rng.uniform(-np.pi, np.pi, (4099, 1))], 1)
    if name == "lattice":
        poses[:500, 2] = 0.0
    return rng.permutation(poses).astype(F32)


def scale_of(name):
    """The robot's size for a cloud: the typical distance between neighbouring points, from the cloud alone."""
    pts = CLOUDS[name][0].astype(np.float64)
    if len(pts) < 2:
        return 0.3
    sub = pts[:: max(1, len(pts) // 200)]
    d = np.sqrt(((sub[:, None] - pts[None]) ** 2).sum(-1))
    d[d == 0] = np.inf
    return float(max(np.median(d.min(1)), 0.05))


def box_of(name):
    return tuple(float(v) for v in (UNIT_BOX * scale_of(name)).astype(F32))


class Device(object):
    """A cloud on the device with its index, and both entries over it."""

    def __init__(self, name):
        pts, geom = CLOUDS[name]
        self.name, self.geom, self.n = name, geom, len(pts)
        self.points = dev(pts.reshape(-1, 2))
        self.sorted_np, self.start_np = omr.cell_index(pts, *geom)
        lib = _lib.load()
        x0, y0, size, nx, ny = geom
        self.sorted = torch.empty_like(self.points)
        self.start = torch.empty(nx * ny + 1, dtype=torch.int32, device="cuda")
        nbytes = lib.nfopp_cell_index_workspace_bytes(self.n)
        work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        _lib.check(lib.nfopp_build_cell_index(_lib.ptr(self.points), self.n, float(x0), float(y0), float(size), nx, ny,
                                              _lib.ptr(self.sorted), _lib.ptr(self.start, torch.int32),
                                              _lib.ptr(work, torch.uint8), nbytes, _lib.stream_ptr()))

    @staticmethod
    def _out(n):
        return (torch.full((n,), -5.0, device="cuda"), torch.full((n,), -5, dtype=torch.int32, device="cuda"))

    def brute(self, poses, box=None, points=None, dim=3):
        points = self.sorted if points is None else points
        dist, index = self._out(poses.shape[0])
        _lib.check(_lib.load().nfopp_nearest_obstacle(_lib.ptr(poses), poses.shape[0], dim, _lib.ptr(points), points.shape[0],
                                                      None if box is None else (ctypes.c_float * 4)(*box),
                                                      _lib.ptr(dist), _lib.ptr(index, torch.int32), _lib.stream_ptr()))
        return dist.cpu().numpy(), index.cpu().numpy()

    def cells(self, poses, box=None, probe=None, dim=3):
        x0, y0, size, nx, ny = self.geom
        dist, index = self._out(poses.shape[0])
        lib = _lib.load()
        args = (_lib.ptr(poses), poses.shape[0], dim, _lib.ptr(self.sorted), self.n, _lib.ptr(self.start, torch.int32), nx, ny,
                float(x0), float(y0), float(size), None if box is None else (ctypes.c_float * 4)(*box), _lib.ptr(dist),
                _lib.ptr(index, torch.int32), _lib.stream_ptr())
        _lib.check(lib.nfopp_nearest_obstacle_cells(*args) if probe is None
                   else lib.nfopp_nearest_obstacle_cells_probe(probe, *args))
        return dist.cpu().numpy(), index.cpu().numpy()


_CACHE = {}


def results(name, shape):
    """(poses fp32, box or None, brute-force (dist, index) over the SORTED points, indexed (dist, index)), computed once
    and shared by the tests of (a) to (e)."""
    key = (name, shape)
    if key not in _CACHE:
        if name not in _CACHE:
            _CACHE[name] = (Device(name), make_poses(name, scale_of(name)))
        device, poses = _CACHE[name]
        box = box_of(name) if shape == "box" else None
        p = dev(poses)
        _CACHE[key] = (device, poses, box, device.brute(p, box), device.cells(p, box))
    return _CACHE[key]


NAMES = sorted(CLOUDS)
SHAPES = ("disc", "box")


# ---- (a) the two entries, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_indexed_and_all_pairs_entries_are_bit_identical(name, shape):
    device, poses, box, (bd, bi), (cd, ci) = results(name, shape)
    assert np.array_equal(device.sorted.cpu().numpy(), device.sorted_np) and np.array_equal(device.start.cpu().numpy(), device.start_np)
    assert np.array_equal(bits(bd), bits(cd)) and np.array_equal(bi, ci)
    if device.n == 0:
        assert np.isinf(bd).all() and (bi == -1).all()
    else:
        assert np.isfinite(bd).all() and (bi >= 0).all() and (bi < device.n).all() and bd.min() >= 0
    for count in COUNTS[:-1]:          # every pose count is a launch of its own: the prefixes give the prefixes' results
        p = dev(poses[:count])
        for dist, index in (device.brute(p, box), device.cells(p, box)):
            assert np.array_equal(bits(dist), bits(bd[:count])) and np.array_equal(index, bi[:count])
    # the other work distribution (one wave per group of poses), at a count that ends inside a group
    wd, wi = device.cells(dev(poses[:1023]), box, probe=0)
    assert np.array_equal(bits(wd), bits(bd[:1023])) and np.array_equal(wi, bi[:1023])
    # the poses the file's docstring promises
    lo, hi = region_of(name)
    xy = poses[:, :2].astype(np.float64)
    on_border = ((xy == lo.astype(F32)) | (xy == hi.astype(F32))).any(1)
    outside = (np.abs(xy - (lo + hi) / 2) > 50 * (hi - lo)).any(1)
    assert on_border.sum() >= 300 and outside.sum() >= 150 and ((xy > lo) & (xy < hi)).all(1).sum() >= 700
    if device.n:   # a pose 100 extents away has to search every ring to the border
        rings = device.cells(dev(poses), box, probe=1)[1]
        x0, y0, size, nx, ny = device.geom
        assert rings.max() == max(nx, ny) and rings.min() >= min(2, max(nx, ny)) and (rings[outside] >= max(nx, ny) // 2).all()
    if name == "n2049_empty_quarter":
        quarter = ((xy > 16.5) & (xy < 29.5)).all(1)
        assert quarter.sum() >= 300 and np.median(rings[quarter]) >= 4 and bd[quarter].min() > 0.9


def test_the_index_refers_to_the_array_passed_in():
    """The all-pairs entry over the UNSORTED cloud: the same distances, indices that name the same points."""
    device, poses, box, (bd, bi), _ = results("n2049_empty_quarter", "disc")
    ud, ui = device.brute(dev(poses), None, points=device.points)
    assert np.array_equal(bits(ud), bits(bd))
    pts = CLOUDS["n2049_empty_quarter"][0]
    # near the cloud no two points are at the same fp32 distance (100 extents away many are, and the smallest index of
    # each array wins): the two indices name the same point
    near = (np.abs(poses[:, :2].astype(np.float64) - 15) < 30).all(1)
    assert near.sum() > 3000 and np.array_equal(bits(pts[ui[near]]), bits(device.sorted_np[bi[near]]))
    assert (ui >= 0).all() and (ui < device.n).all()
    d2, i2 = device.brute(dev(poses[:, :2]), None, dim=2)               # pose_dim 2: the disc needs no heading
    c2, j2 = device.cells(dev(poses[:, :2]), None, dim=2)
    assert np.array_equal(bits(d2), bits(bd)) and np.array_equal(i2, bi) and np.array_equal(bits(c2), bits(bd)) and np.array_equal(j2, bi)


# ---- (b) ties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["lattice", "duplicated"])
def test_ties_go_to_the_smallest_index(name, shape):
    device, poses, box, (bd, bi), (cd, ci) = results(name, shape)
    d64 = cr.distances(poses, device.sorted_np, box)
    if name == "lattice":
        # heading 0 at lattice midpoints: every offset, and (c, s) = (1, 0), are exact, so fp32 and float64 tie alike
        mid = (poses[:, 2] == 0) & (np.abs(poses[:, :2] % 1 - 0.5) < 1e-6).any(1)
        assert mid.sum() == 500
        tied = (d64[mid] == d64[mid].min(1, keepdims=True)).sum(1)
        assert set(tied) == {2, 4}
        assert np.array_equal(bi[mid], d64[mid].argmin(1)) and np.array_equal(ci[mid], bi[mid])
    if name == "duplicated":
        # every point occurs twice in the sorted array: the answer must be the first of each pair
        pts = device.sorted_np
        first = np.array([np.flatnonzero((pts == pts[k]).all(1))[0] for k in range(device.n)])
        assert (first != np.arange(device.n)).sum() == device.n // 2
        assert np.array_equal(first[bi], bi) and np.array_equal(ci, bi)
        assert (d64[np.arange(len(poses)), bi] <= d64.min(1) * (1 + 1e-5) + 1e-6).all()


# ---- (c) consistency with the ground-truth checkers --------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_disc_distance_below_the_radius_is_the_circle_checkers_label(name):
    device, poses, _, (bd, bi), _ = results(name, "disc")
    radius = scale_of(name)
    lo, hi = region_of(name)
    pad = (hi - lo) / 2 + 2 * radius                # the far-away poses are out of bounds, the others are not
    bounds = (float(lo[0] - pad[0]), float(hi[0] + pad[0]), float(lo[1] - pad[1]), float(hi[1] + pad[1]))
    checker = nfopp.DeviceCircleChecker(CLOUDS[name][0], radius, bounds)
    labels = checker.labels(dev(poses)).cpu().numpy()
    oob = omr.out_of_bounds(poses[:, :2], np.array(bounds, F32))
    hit = bd < F32(radius)
    assert np.array_equal(hit | oob, labels.astype(bool))
    got, index = checker.nearest(dev(poses))
    assert np.array_equal(bits(got.cpu().numpy()), bits(bd))
    if device.n:   # the checker's own index has another geometry: its indices name points at the same distance
        named = checker.obstacles.cpu().numpy()[index.cpu().numpy()].astype(np.float64) - poses[:, :2]
        assert (np.abs(np.sqrt((named ** 2).sum(1)) - bd) <= 4 * EPS * bd).all()
    clearance = checker.clearance(dev(poses)).cpu().numpy()
    assert np.array_equal(bits(clearance), bits(np.maximum(bd - F32(radius), F32(0))))
    if device.n:
        assert 0.2 <= hit.mean() <= 0.8, hit.mean()
        assert oob.any() and oob.mean() < 0.2
    else:
        assert not hit.any() and np.isinf(clearance).all()


@pytest.mark.parametrize("name", NAMES)
def test_box_distance_is_zero_wherever_the_rectangle_checker_finds_an_obstacle(name):
    device, poses, box, (bd, bi), _ = results(name, "box")
    checker = nfopp.DeviceRectangleChecker(CLOUDS[name][0], box, None)
    labels = checker.labels(dev(poses)).cpu().numpy().astype(bool)          # no bounds: the obstacle term alone
    assert (bd[labels] == 0).all() and not labels[bd > 0].any()
    got = checker.clearance(dev(poses)).cpu().numpy()
    assert np.array_equal(bits(got), bits(bd))
    if device.n:
        assert 0.2 <= labels.mean() <= 0.8 and 0.2 <= (bd > 0).mean() <= 0.8, (labels.mean(), (bd > 0).mean())
        # d == 0 without a collision happens on the rim only: rare, and the float64 distance is tiny there
        rim = (bd == 0) & ~labels
        assert rim.mean() < 0.01


# ---- (d), (e) against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_disc_distance_against_float64(name):
    """|dist - min d64| <= 4 eps min d64, eps = 2^-24: dx and dy are rounded once each (2 eps relative on d^2), dy * dy and the
    fma once each (eps each), the square root halves the relative error and adds its own rounding: at most 3 eps; 4 is
    asserted.  The point the index names must be within the same margin of the float64 minimum."""
    device, poses, _, (bd, bi), _ = results(name, "disc")
    if device.n == 0:
        return
    d64 = cr.distances(poses, device.sorted_np)
    m = d64.min(1)
    err = np.abs(bd.astype(np.float64) - m)
    print("disc %s: max |dist - d64| / (eps d64) = %.3f" % (name, float((err / (EPS * np.maximum(m, 1e-300))).max())))
    assert (err <= 4 * EPS * m).all()
    assert (np.abs(d64[np.arange(len(poses)), bi] - m) <= 4 * EPS * m).all()


@pytest.mark.parametrize("name", NAMES)
def test_box_distance_against_float64(name):
    """Absolute bound per point k, with a = |dx|, b = |dy| of that point and eps = 2^-24:  err(k) = 9.5 eps (a + b).
    rx = fma(c, dx, s * dy): c and s are the device's cosf / sinf, documented to 2 ulp of a value <= 1, i.e. 2 eps absolute
    -> 2 eps (a + b); dx, dy rounded -> eps (a + b); s * dy rounded -> eps b; the fma's rounding -> eps |rx| <= eps (a + b)
    ... together |rx - rx64| <= 4 eps a + 5 eps b, and |ry - ry64| <= 5 eps a + 4 eps b.  The distance to the box is
    1-Lipschitz in (rx, ry): sqrt((4a + 5b)^2 + (5a + 4b)^2) <= sqrt(41) (a + b) = 6.41 (a + b) eps.  Forming ex, ey (one
    subtraction each), ey * ey, the fma and the square root add at most 3 eps d <= 3 eps (a + b).  9.41 -> 9.5.
    Both the device's nearest point kf and float64's k64 enter: min_f <= d_f(k64) <= min64 + err(k64) and
    min_f = d_f(kf) >= d64(kf) - err(kf) >= min64 - err(kf)."""
    device, poses, box, (bd, bi), _ = results(name, "box")
    if device.n == 0:
        return
    d64 = cr.distances(poses, device.sorted_np, box)
    k64 = d64.argmin(1)
    rows = np.arange(len(poses))
    dx, dy = cr.offsets(poses, device.sorted_np)
    size = np.abs(dx) + np.abs(dy)
    got = bd.astype(np.float64)
    print("box %s: max (dist - min64) / (eps (|dx| + |dy|)) above %.3f below %.3f"
          % (name, float(((got - d64[rows, k64]) / (EPS * np.maximum(size[rows, k64], 1e-300))).max()),
             float(((d64[rows, k64] - got) / (EPS * np.maximum(size[rows, bi], 1e-300))).max())))
    assert (got - d64[rows, k64] <= 9.5 * EPS * size[rows, k64]).all()
    assert (d64[rows, k64] - got <= 9.5 * EPS * size[rows, bi]).all()
    assert (d64[rows, bi] - d64[rows, k64] <= 9.5 * EPS * (size[rows, bi] + size[rows, k64])).all()


# ---- (f) edge cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_edge_cases(shape):
    device, poses, box, (bd, bi), (cd, ci) = results("n33", shape)
    lib = _lib.load()
    # n = 0: a no-op that touches nothing
    assert lib.nfopp_nearest_obstacle(None, 0, 3, _lib.ptr(device.sorted), device.n, None, None, None, _lib.stream_ptr()) == 0
    # n_obstacles = 0 through both entries, with and without an index array
    empty = Device("g21_d")
    p = dev(poses[:300])
    for dist, index in (empty.brute(p, box), empty.cells(p, box)):
        assert np.isposinf(dist).all() and (index == -1).all()
    # non-finite poses among finite ones
    bad = poses[:300].copy()
    bad[7, 0], bad[100, 1], bad[255, 0], bad[256, 1] = np.nan, np.inf, -np.inf, np.nan
    if shape == "box":
        bad[31, 2], bad[32, 2] = np.nan, np.inf
    broken = ~np.isfinite(bad).all(1)
    assert broken.sum() == (6 if shape == "box" else 4)
    for dist, index in (device.brute(dev(bad), box), device.cells(dev(bad), box), device.cells(dev(bad), box, probe=0)):
        assert np.isposinf(dist[broken]).all() and (index[broken] == -1).all()
        assert np.array_equal(bits(dist[~broken]), bits(bd[:300][~broken])) and np.array_equal(index[~broken], bi[:300][~broken])
    # index_dev may be null
    dist = torch.empty(300, device="cuda")
    x0, y0, size, nx, ny = device.geom
    _lib.check(lib.nfopp_nearest_obstacle_cells(_lib.ptr(p), 300, 3, _lib.ptr(device.sorted), device.n,
                                                _lib.ptr(device.start, torch.int32), nx, ny, float(x0), float(y0), float(size),
                                                None if box is None else (ctypes.c_float * 4)(*box), _lib.ptr(dist), None,
                                                _lib.stream_ptr()))
    assert np.array_equal(bits(dist.cpu().numpy()), bits(bd[:300]))
    # run to run
    again = device.cells(dev(poses), box)
    assert again[0].tobytes() == cd.tobytes() and again[1].tobytes() == ci.tobytes()


# ---- (g) nfopp_path_stats --------------------------------------------------------------------------------------------
def run_stats(traj, start, goal, cos_cusp, pose_dist=None, active=None):
    B, N, D = traj.shape
    out = torch.full((B, 8), -77.0, dtype=torch.float64, device="cuda")
    t, s, g = dev(traj), dev(start), dev(goal)
    pd = None if pose_dist is None else dev(pose_dist)
    act = None if active is None else dev(active, np.uint8)
    _lib.check(_lib.load().nfopp_path_stats(_lib.ptr(t), _lib.ptr(s), _lib.ptr(g), B, N, D, _lib.ptr(pd),
                                            0 if pose_dist is None else pose_dist.shape[1], float(cos_cusp),
                                            _lib.ptr(out, torch.float64), _lib.ptr(act, torch.uint8), _lib.stream_ptr()))
    return out.cpu().numpy()


def check_stats(got, paths, cos_cusp, pose_dist=None, by_terms=False):
    """Slots 1-6 as bit patterns; the two sums (0, 7) to a relative 1e-12: a tree and a sequential float64 sum of at most
    2054 non-negative terms differ by at most n 2^-53 = 2.3e-13 relative.  `by_terms`: that bound itself, from the number of
    terms of each sum (N + 1 segments, the poses of a path), for paths so long that it exceeds 1e-12."""
    for b in range(len(paths)):
        ref = cr.path_stats(paths[b], cos_cusp, None if pose_dist is None else pose_dist[b])
        assert np.array_equal(bits(got[b, 1:7]), bits(ref[1:7])), (b, got[b], ref)
        terms = {cr.LENGTH: len(paths[b]) - 1, cr.MEAN_CLEARANCE: 0 if pose_dist is None else len(pose_dist[b])}
        for k in (cr.LENGTH, cr.MEAN_CLEARANCE):
            rel = terms[k] * 2.0 ** -53 if by_terms else 1e-12
            if by_terms and np.isfinite(ref[k]):
                print("path %d slot %d: |got - ref| / ref = %.3g, bound %.3g" % (b, k, abs(got[b, k] - ref[k]) / abs(ref[k]), rel))
            assert got[b, k] == ref[k] or abs(got[b, k] - ref[k]) <= rel * abs(ref[k]), (b, k, got[b, k], ref[k])


def wiggly_paths(rng, B, N, D):
    """Random walks with headings along the travel direction, so every forward component is far from zero; path 0 gets two
    coincident waypoints, a 180 degree cusp and a stretch driven backwards (where N allows)."""
    course = np.cumsum(rng.normal(0, 0.5, (B, N + 2)), 1)
    step = rng.uniform(0.05, 0.3, (B, N + 2, 1)) * np.stack([np.cos(course), np.sin(course)], -1)
    xy = np.cumsum(step, 1)
    paths = np.concatenate([xy, np.zeros((B, N + 2, 1))], 2)
    if N >= 12:
        paths[0, 3, :2] = paths[0, 2, :2]                                   # a zero segment
        paths[0, 7, :2] = paths[0, 5, :2] + 0.25 * (paths[0, 6, :2] - paths[0, 5, :2])   # 5 -> 6 -> 7 folds back exactly
    d = np.diff(paths[:, :, :2], axis=1)
    d = np.concatenate([d, d[:, -1:]], 1)
    paths[:, :, 2] = np.arctan2(d[:, :, 1], d[:, :, 0]) + rng.uniform(-0.3, 0.3, (B, N + 2))
    if N >= 12:
        paths[0, 9:12, 2] += np.pi                                          # segments 9, 10, 11 are driven backwards
    return paths[:, :, :D].astype(F32)


@pytest.mark.parametrize("sub", [1, 4])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("B,N", [(1, 1), (3, 2), (5, 255), (2, 257)])
def test_path_stats_equal_the_restatement(B, N, D, sub):
    rng = np.random.default_rng(1000 * N + 10 * D + sub)
    paths = wiggly_paths(rng, B, N, D)
    m = (N + 1) * sub + 1
    pose_dist = rng.uniform(0, 3, (B, m)).astype(F32)
    pose_dist[:, m // 2] = pose_dist.min(1) if m > 2 else pose_dist[:, m // 2]       # a tied minimum: the first index wins
    cos_cusp = float(np.cos(np.pi - np.pi / 3))
    if D == 3:
        fwd = np.concatenate([cr.forward_components(p) for p in paths])
        assert (np.abs(fwd[fwd != 0]) > 1e-9).all()
    active = np.ones(B, np.uint8)
    active[0] = 0                                                             # a retired path is written all the same
    got = run_stats(paths[:, 1:-1].copy(), paths[:, 0].copy(), paths[:, -1].copy(), cos_cusp, pose_dist, active)
    check_stats(got, paths, cos_cusp, pose_dist)
    assert np.array_equal(bits(got), bits(run_stats(paths[:, 1:-1].copy(), paths[:, 0].copy(), paths[:, -1].copy(), cos_cusp,
                                                    pose_dist, None)))
    if N >= 12:
        ref = cr.path_stats(paths[0], cos_cusp)
        assert ref[cr.CUSPS] >= 1 and ref[cr.REVERSALS] == (2 if D == 3 else 0) and ref[cr.CURVATURE_AT] >= 1
        assert got[0, cr.CUSPS] == ref[cr.CUSPS] and got[0, cr.REVERSALS] == ref[cr.REVERSALS]
    # without distances the clearance slots take their null values, the others stay
    bare = run_stats(paths[:, 1:-1].copy(), paths[:, 0].copy(), paths[:, -1].copy(), cos_cusp)
    check_stats(bare, paths, cos_cusp)
    assert np.isposinf(bare[:, cr.MIN_CLEARANCE]).all() and (bare[:, cr.CLEARANCE_AT] == -1).all()
    assert np.array_equal(bits(bare[:, :5]), bits(got[:, :5]))


def test_path_stats_of_hand_made_paths():
    """One 180 degree cusp on an otherwise straight path; two coincident waypoints; exactly two reversals."""
    x = np.array([0, 1, 2, 3, 2.5, 2.5, 1, 0, -1], np.float64)
    path = np.stack([x, 0.5 * np.ones_like(x), np.zeros_like(x)], 1)[None].astype(F32)
    path[0, 5:8, 2] = np.pi     # forward to x = 3, backwards (heading 0) to 2.5, a pause, then forward again, facing -x
    ref = cr.path_stats(path[0], -0.5)
    assert ref[cr.CUSPS] == 1 and ref[cr.REVERSALS] == 2 and ref[cr.MAX_CURVATURE] == 0 and ref[cr.LENGTH] == 7.0
    got = run_stats(path[:, 1:-1].copy(), path[:, 0].copy(), path[:, -1].copy(), -0.5)
    check_stats(got, path, -0.5)
    assert got[0, cr.LENGTH] == 7.0 and got[0, cr.CURVATURE_AT] == 1


@functools.lru_cache(maxsize=None)
def longest_paths(D):
    """Two wiggly paths of cr.LONGEST_PATH waypoints and a distance per pose at sub = 1, built once per D."""
    B, N = 2, cr.LONGEST_PATH
    rng = np.random.default_rng(40 + D)
    paths = wiggly_paths(rng, B, N, D)
    pose_dist = rng.uniform(0, 3, (B, N + 2)).astype(F32)
    pose_dist[:, (N + 2) // 2] = pose_dist.min(1)                            # a tied minimum: the first index wins
    return paths, pose_dist


@pytest.mark.parametrize("with_dist", [False, True])
@pytest.mark.parametrize("D", [2, 3])
def test_path_stats_at_the_longest_path_served(D, with_dist):
    """N = cr.LONGEST_PATH: the head and the sign array are exactly the 160 KiB of one workgroup's LDS, and every thread strides
    640 times over the path.  Slots 1-6 as bit patterns; the sums within n 2^-53 relative, n = N + 1 segments / N + 2 poses
    (1.8e-11: here the constant 1e-12 of the short paths would be tighter than the bound it stands for)."""
    paths, pose_dist = longest_paths(D)
    N = paths.shape[1] - 2
    assert N == cr.LONGEST_PATH and 64 + (N + 1 + 15) // 16 * 16 == 160 * 1024
    if D == 3:
        fwd = np.concatenate([cr.forward_components(p) for p in paths])
        assert (np.abs(fwd[fwd != 0]) > 1e-9).all() and (fwd == 0).sum() >= 1
    cos_cusp = float(np.cos(np.pi - np.pi / 3))
    dist = pose_dist if with_dist else None
    got = run_stats(paths[:, 1:-1].copy(), paths[:, 0].copy(), paths[:, -1].copy(), cos_cusp, dist)
    check_stats(got, paths, cos_cusp, dist, by_terms=True)
    assert np.array_equal(bits(got), bits(run_stats(paths[:, 1:-1].copy(), paths[:, 0].copy(), paths[:, -1].copy(), cos_cusp, dist)))
    ref = cr.path_stats(paths[0], cos_cusp)
    assert ref[cr.CUSPS] >= 1 and ref[cr.REVERSALS] >= (2 if D == 3 else 0) and ref[cr.CURVATURE_AT] >= 1
    assert got[0, cr.CUSPS] == ref[cr.CUSPS] and got[0, cr.REVERSALS] == ref[cr.REVERSALS]
    if not with_dist:
        assert np.isposinf(got[:, cr.MIN_CLEARANCE]).all() and (got[:, cr.CLEARANCE_AT] == -1).all()


# ---- (h) BatchPlanner ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner_case():
    torch.random.manual_seed(5)
    onf = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=True).to("cuda")
    rng = np.random.default_rng(8)
    B, N = 8, 32
    cloud = rng.uniform(0.5, 2.5, (40, 2))
    starts = np.concatenate([rng.uniform(0.1, 0.6, (B, 2)), rng.uniform(-3, 3, (B, 1))], 1).astype(F32)
    goals = np.concatenate([rng.uniform(2.4, 2.9, (B, 2)), rng.uniform(-3, 3, (B, 1))], 1).astype(F32)
    bounds = (0.0, 3.0, 0.0, 3.0)
    hyper = nfopp.TrajectoryHyper(collision_weight=3, direction_delta_weight=7, collision_beta=2, bounds=bounds)
    planner = nfopp.BatchPlanner(onf, B, N, hyper)              # no checker: the field stays frozen
    planner.init(starts, goals, bounds)
    planner.step(n=5)
    return planner, cloud, bounds


@pytest.mark.parametrize("kind", ["circle", "rectangle"])
def test_evaluate_with_a_clearance_margin(planner_case, kind):
    planner, cloud, bounds = planner_case
    checker = nfopp.DeviceCircleChecker(cloud, 0.05, bounds) if kind == "circle" \
        else nfopp.DeviceRectangleChecker(cloud, (-0.05, 0.08, -0.04, 0.04), bounds)
    plain = [t.clone() for t in planner.evaluate(checker)]
    zero = [t.clone() for t in planner.evaluate(checker, min_clearance=0.0)]
    assert torch.equal(plain[0], zero[0]) and np.array_equal(bits(plain[1].cpu().numpy()), bits(zero[1].cpu().numpy()))
    huge = planner.evaluate(checker, min_clearance=100.0)[0]
    assert huge.cpu().numpy().all()
    # a margin in between flags exactly the paths whose smallest clearance is below it
    stats = planner.path_stats(checker).cpu().numpy()
    margin = float(np.median(stats[:, nfopp.PATH_STAT_MIN_CLEARANCE])) + 1e-4
    flagged = planner.evaluate(checker, min_clearance=margin)[0].cpu().numpy().astype(bool)
    assert np.array_equal(flagged, plain[0].cpu().numpy().astype(bool) | (stats[:, nfopp.PATH_STAT_MIN_CLEARANCE] < F32(margin)))
    assert 0 < flagged.sum() < 8 or plain[0].all()


@pytest.mark.parametrize("sub", [1, 4])
def test_planner_path_stats_equal_the_restatement(planner_case, sub):
    planner, cloud, bounds = planner_case
    checker = nfopp.DeviceCircleChecker(cloud, 0.05, bounds)
    got = planner.path_stats(checker, sub=sub).cpu().numpy()
    paths = planner.get_paths()
    assert got.shape == (8, nfopp.NUM_PATH_STATS) and got.dtype == np.float64
    # the clearance the statistics were taken from is the checker's, at the poses evaluate() tests
    clearance = planner._stat_clearance.cpu().numpy()
    assert clearance.shape == (8, 33 * sub + 1)
    again = checker.clearance(planner._stat_poses.view(-1, 3)).cpu().numpy().reshape(clearance.shape)
    assert np.array_equal(bits(again), bits(clearance))
    d64, _ = cr.nearest(planner._stat_poses.view(-1, 3).cpu().numpy(), checker.obstacles.cpu().numpy())
    assert np.abs(np.maximum(d64 - 0.05, 0) - clearance.reshape(-1)).max() < 1e-6
    cos_cusp = float(np.cos(np.pi - np.pi / 3))
    check_stats(got, paths, cos_cusp, clearance)
    assert np.isfinite(got).all() and (got[:, nfopp.PATH_STAT_LENGTH] > 2.0).all()
    # without a point cloud: the path's own statistics only
    bare = planner.path_stats(None, sub=sub).cpu().numpy()
    check_stats(bare, paths, cos_cusp)
    grid = nfopp.DeviceGridChecker(np.zeros((8, 8), np.uint8), 0.0, 0.0, 0.5)
    assert np.array_equal(bits(planner.path_stats(grid, sub=sub).cpu().numpy()), bits(bare))


def test_the_grid_checker_has_no_clearance(planner_case):
    planner = planner_case[0]
    grid = nfopp.DeviceGridChecker(np.zeros((8, 8), np.uint8), 0.0, 0.0, 0.5)
    with pytest.raises(NotImplementedError, match="DeviceCircleChecker"):
        grid.clearance(torch.zeros(4, 3, device="cuda"))
    with pytest.raises(NotImplementedError):
        planner.evaluate(grid, min_clearance=0.1)
    assert not hasattr(grid, "nearest")
