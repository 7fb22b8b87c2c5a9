"""CPU-only tests of the clearance feature: the numpy restatement (tests/clearance_ref.py) against hand-computed cases,
the argument checks of the three C-ABI entries without a device, and the slot constants."""
import ctypes
import os

import numpy as np

import clearance_ref as cr
import nfopp
from nfopp import _lib

F32 = np.float32


def test_disc_distance_is_the_3_4_5_triangle():
    poses = np.array([[1.0, 2.0, 0.7], [0.0, 0.0, 0.0]], F32)
    points = np.array([[4.0, 6.0], [1.0, 2.0], [4.0, 6.0]], F32)
    d = cr.distances(poses, points)
    assert np.array_equal(d[0], [5.0, 0.0, 5.0]) and d[1, 1] == np.sqrt(5.0)
    dist, index = cr.nearest(poses, points)
    assert np.array_equal(dist, [0.0, np.sqrt(5.0)]) and np.array_equal(index, [1, 1])
    dist, index = cr.nearest(poses[:1], points[[0, 2]])          # a tie: the first index
    assert dist[0] == 5.0 and index[0] == 0
    dist, index = cr.nearest(poses, np.zeros((0, 2)))
    assert np.isinf(dist).all() and (index == -1).all()


def test_box_distance_inside_rim_and_outside():
    box = (-1.0, 2.0, -0.5, 0.5)
    poses = np.array([[10.0, 20.0, 0.0], [10.0, 20.0, np.pi / 2]], F32)
    # in the frame of pose 0: inside, on the front rim, 3 ahead of the front rim, off the front-left corner by (3, 4)
    points = np.array([[10.5, 20.25], [12.0, 20.0], [15.0, 20.0], [15.0, 24.5]], F32)
    d = cr.distances(poses[:1], points, box)[0]
    assert np.array_equal(d, [0.0, 0.0, 3.0, 5.0])
    # pose 1 looks along +y: the point 1.5 above it is inside, the one 0.75 to its right is 0.25 off the right side
    turned = np.array([[10.0, 21.5], [10.75, 20.0]], F32)
    d = cr.distances(poses[1:], turned, box)[0]
    assert d[0] == 0.0 and abs(d[1] - 0.25) < 1e-7           # cos(fp32(pi / 2)) is -4.4e-8, not 0
    dist, index = cr.nearest(poses[:1], points, box)
    assert dist[0] == 0.0 and index[0] == 0                      # inside and rim tie at 0: the first


def test_path_stats_of_a_right_angle():
    path = np.array([[0, 0], [3, 0], [3, 4]], F32)
    s = cr.path_stats(path, cos_cusp=-0.5)
    assert s[cr.LENGTH] == 7.0
    # Menger curvature of the triangle (0,0), (3,0), (3,4): 4 * area / (abc) = 2 * 12 / (3 * 4 * 5) = 0.4 = 1 / circumradius
    assert s[cr.MAX_CURVATURE] == 2.0 * 12.0 / (12.0 * 5.0) and s[cr.CURVATURE_AT] == 1
    assert s[cr.CUSPS] == 0 and s[cr.REVERSALS] == 0
    assert s[cr.MIN_CLEARANCE] == np.inf and s[cr.CLEARANCE_AT] == -1 and s[cr.MEAN_CLEARANCE] == np.inf
    assert cr.path_stats(path, cos_cusp=0.5)[cr.CUSPS] == 1     # a quarter turn is sharper than a 60 degree one
    s = cr.path_stats(path, -0.5, pose_dist=np.array([2.0, 0.5, 1.0, 0.5], F32))
    assert s[cr.MIN_CLEARANCE] == 0.5 and s[cr.CLEARANCE_AT] == 1 and s[cr.MEAN_CLEARANCE] == 1.0


def test_path_stats_of_a_cusp_and_of_a_zero_segment():
    path = np.array([[0, 0], [2, 0], [2, 0], [1, 0], [1, 1]], F32)     # out, a repeated waypoint, straight back, a turn
    s = cr.path_stats(path, cos_cusp=-0.5)
    assert s[cr.LENGTH] == 4.0
    # the vertices next to the zero segment are no candidates and no cusps; the 180 degree fold (2,0) is split by it
    assert s[cr.CUSPS] == 0 and s[cr.CURVATURE_AT] == 3 and s[cr.MAX_CURVATURE] == 2.0 * 1.0 / (1.0 * np.sqrt(2.0))
    fold = np.array([[0, 0], [2, 0], [1, 0]], F32)
    s = cr.path_stats(fold, cos_cusp=-0.5)
    assert s[cr.CUSPS] == 1 and s[cr.MAX_CURVATURE] == 0.0 and s[cr.CURVATURE_AT] == 1      # zero area, finite denominator
    there_and_back = np.array([[0, 0], [2, 0], [0, 0]], F32)            # the chord is zero: no candidate at all
    s = cr.path_stats(there_and_back, cos_cusp=-0.5)
    assert s[cr.CUSPS] == 1 and s[cr.MAX_CURVATURE] == 0.0 and s[cr.CURVATURE_AT] == -1


def test_path_stats_of_one_reversal():
    # heading +x all along; the path drives forward twice, then backs up twice
    path = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 0.1, 0], [0, 0.2, 0]], F32)
    assert np.all(np.abs(cr.forward_components(path)) > 0.5)
    s = cr.path_stats(path, cos_cusp=-0.5)
    assert s[cr.REVERSALS] == 1 and s[cr.CUSPS] == 1
    # a segment driven exactly sideways (s = 0) is skipped: forward, sideways, backward is still one reversal
    side = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F32)
    assert cr.forward_components(side)[1] == 0.0 and cr.path_stats(side, -0.5)[cr.REVERSALS] == 1
    assert cr.path_stats(path[:, :2], -0.5)[cr.REVERSALS] == 0   # no headings, no reversals


def test_slot_constants():
    names = ("LENGTH", "MAX_CURVATURE", "CURVATURE_AT", "CUSPS", "REVERSALS", "MIN_CLEARANCE", "CLEARANCE_AT", "MEAN_CLEARANCE")
    assert [getattr(nfopp, "PATH_STAT_" + n) for n in names] == list(range(8)) == [getattr(cr, n) for n in names]
    assert nfopp.NUM_PATH_STATS == cr.NUM_PATH_STATS == 8 and len(nfopp.PATH_STAT_NAMES) == 8
    assert [n.upper() for n in nfopp.PATH_STAT_NAMES] == list(names)
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nfopp_hip.h")).read()
    assert "#define NFOPP_NUM_PATH_STATS 8" in header
    for k, n in enumerate(names):
        assert "#define NFOPP_PATH_STAT_%s %d\n" % (n, k) in header


def test_c_abi_argument_checks():
    lib = _lib.load()
    one = ctypes.c_void_p(256)            # a non-null pointer that no rejected call may touch
    box = (ctypes.c_float * 4)(-0.34, 0.4, -0.27, 0.27)

    def err():
        return lib.nfopp_last_error()

    def brute(poses=one, n=10, dim=3, pts=one, n_pts=50, bx=None, dist=one, index=one):
        return lib.nfopp_nearest_obstacle(poses, n, dim, pts, n_pts, bx, dist, index, None)

    def cells(poses=one, n=10, dim=3, pts=one, n_pts=50, start=one, nx=4, ny=4, size=0.6, bx=None, dist=one, index=one):
        return lib.nfopp_nearest_obstacle_cells(poses, n, dim, pts, n_pts, start, nx, ny, 0.0, 0.0, size, bx, dist, index, None)

    for fn in (brute, cells):
        assert fn(n=0, poses=None, dist=None, index=None) == 0          # no pose: nothing to do, nothing is launched
        assert fn(poses=None) == -1 and b"null" in err()
        assert fn(dist=None) == -1 and b"null" in err()
        assert fn(pts=None) == -1 and b"obstacle" in err()
        assert fn(n=-1) == -1 and fn(n_pts=-1) == -1 and fn(dim=4) == -1 and fn(dim=1) == -1
        assert fn(dim=2, bx=box) == -1 and b"pose_dim 3" in err()
        assert fn(n=0, dim=2, bx=box) == -1                              # bad sizes are bad without poses too
    assert cells(start=None) == -1 and b"index" in err()
    assert cells(nx=0) == -1 and cells(ny=-3) == -1
    assert cells(nx=257, ny=256) == -1 and b"65536" in err()
    assert cells(size=0.0) == -1 and cells(size=float("nan")) == -1 and b"cell size" in err()

    def stats(traj=one, start=one, goal=one, batch=4, n=16, dim=3, dist=one, poses=69, cos_cusp=-0.5, out=one):
        return lib.nfopp_path_stats(traj, start, goal, batch, n, dim, dist, poses, cos_cusp, out, None, None)
    assert stats(batch=0, traj=None, start=None, goal=None, out=None) == 0
    assert stats(traj=None) == -1 and b"null" in err()
    assert stats(start=None) == -1 and stats(goal=None) == -1 and stats(out=None) == -1
    assert stats(batch=-1) == -1 and stats(n=0) == -1 and stats(dim=4) == -1
    assert stats(poses=0) == -1 and stats(poses=-1, dist=None) == -1 and b"pose count" in err()
    assert stats(cos_cusp=float("nan")) == -1
    assert stats(n=200000) == -1 and b"too long" in err()              # the sign array must fit one workgroup's LDS
    # with the reductions' 64-byte head in front of it, all of it dynamic: 64 + 16 * ceil((N + 1) / 16) bytes in 160 KiB.  The
    # last N served (cr.LONGEST_PATH, run on the device in tests/test_gpu_clearance.py) asks for exactly 163840 bytes, the first
    # one refused for 16 more -- the message carries the request.  N = 163792 .. 163839 fit while the head was static LDS
    # that the check did not count
    assert 64 + (cr.LONGEST_PATH + 1 + 15) // 16 * 16 == 160 * 1024 == 163840
    for dim in (2, 3):
        assert stats(n=cr.LONGEST_PATH + 1, dim=dim) == -1 and b"too long" in err() and b"(163856 bytes)" in err()
        assert stats(n=163792, dim=dim) == -1 and stats(n=163839, dim=dim) == -1 and b"too long" in err()
    kernel = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-motion-planner_amd", "csrc",
                               "clearance.hip")).read()
    stats_kernel = kernel[kernel.index("void path_stats_kernel("):kernel.index("static void launch_nearest(")]
    assert "extern __shared__" in stats_kernel and stats_kernel.count("__shared__") == 1      # no static array beside the dynamic block
    assert "constexpr int PS_HEAD = 64;" in kernel and "N = %d" % cr.LONGEST_PATH in kernel
