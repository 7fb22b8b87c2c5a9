"""Hand-computed cases that pin tests/swept_ref.py, the float64 restatement the GPU tests of csrc/swept.hip compare the
device with.  No GPU."""
import ctypes

import numpy as np

import swept_ref as sr
from nfopp import _lib

F32 = np.float32
BOX = (-1.0, 3.0, -0.5, 0.5)          # largest corner distance hypot(3, 0.5)


def seg(ax, ay, bx, by, tha=0.0, thb=0.0):
    return np.array([[ax, ay, tha]], F32), np.array([[bx, by, thb]], F32)


def test_point_beside_the_middle_of_a_segment():
    a, b = seg(0, 0, 4, 0)
    d = sr.segment_distances(a, b, [[2.0, 1.5]])
    assert d.shape == (1, 1) and d[0, 0] == 1.5
    # a slanted segment: (0, 0) -> (3, 4), the point (4, -3) + (1.5, 2) projects onto its middle at distance 5
    a, b = seg(0, 0, 3, 4)
    assert abs(sr.segment_distances(a, b, [[5.5, -1.0]])[0, 0] - 5.0) < 1e-12


def test_point_beyond_each_end():
    a, b = seg(0, 0, 4, 0)
    d = sr.segment_distances(a, b, [[-3.0, 4.0], [7.0, -4.0]])
    assert d[0, 0] == 5.0 and d[0, 1] == 5.0          # |o - a| and |o - b|, not the distance 4 to the line


def test_point_on_the_line_outside_the_segment():
    a, b = seg(1, 1, 3, 3)
    d = sr.segment_distances(a, b, [[5.0, 5.0], [0.0, 0.0], [2.0, 2.0], [3.0, 3.0]])
    assert np.allclose(d[0], [2 * np.sqrt(2), np.sqrt(2), 0.0, 0.0], atol=1e-15)
    assert d[0, 3] == 0.0                                # the end point itself: the endpoint term, exactly


def test_zero_length_segment_is_the_point_distance():
    a, b = seg(2, 1, 2, 1)
    pts = np.array([[5.0, 5.0], [2.0, 3.5], [-1.0, 1.0]], F32)
    d = sr.segment_distances(a, b, pts)
    assert np.array_equal(d[0], [5.0, 2.5, 3.0])
    v, k = sr.disc_values(a, b, pts)
    assert v[0] == 2.5 and k[0] == 1
    assert np.array_equal(sr.disc_values(a, b, pts, horizon=2.0), (np.array([np.inf]), np.array([-1])))
    assert np.array_equal(sr.disc_values(a, b, np.zeros((0, 2))), (np.array([np.inf]), np.array([-1])))


def test_ties_go_to_the_first_point_and_non_finite_segments_have_no_value():
    a, b = seg(0, 0, 2, 0)
    v, k = sr.disc_values(a, b, [[1.0, 1.0], [1.0, -1.0], [3.0, 0.0]])
    assert v[0] == 1.0 and k[0] == 0
    a[0, 1] = np.nan
    assert np.array_equal(sr.disc_values(a, b, [[1.0, 1.0]]), (np.array([np.inf]), np.array([-1])))


def test_pure_rotation_of_a_box():
    reach = sr.box_reach(BOX)
    assert abs(reach - np.hypot(3.0, 0.5) * 1.000001) < 1e-6 and reach > np.hypot(3.0, 0.5)
    a, b = seg(1, 2, 1, 2, 0.25, 0.75)
    assert abs(sr.delta(a, b, reach)[0] - reach * 0.5) < 1e-7 * reach
    a, b = seg(0, 0, 0, 0, 0.0, np.pi / 2)
    # at heading 0 the point (0, 4) is 3.5 above the box; at pi / 2 the box covers y in [-1, 3]: 1 beyond its front
    v, k = sr.box_values(a, b, [[0.0, 4.0]], BOX)
    assert abs(v[0] - (3.5 + 1.0 - reach * np.pi / 2)) < 1e-6 and k[0] == 0


def test_heading_pair_straddling_pi():
    reach = sr.box_reach(BOX)
    a, b = seg(0, 0, 0, 0, 3.1, -3.1)
    turn = 2 * np.pi - float(F32(3.1)) * 2
    assert 0.08 < turn < 0.09
    assert abs(sr.delta(a, b, reach)[0] - reach * turn) < 1e-12
    a, b = seg(0, 0, 3, 4, -3.0, 3.0)
    assert abs(sr.delta(a, b, reach)[0] - (5.0 + reach * (2 * np.pi - 6.0))) < 1e-6
    # the sampler turns the short way too: the box keeps pointing along -x, a point behind it is never touched,
    # a point the long way round would sweep over stays free as well
    a, b = seg(0, 0, 0, 0, 3.1, -3.1)
    assert not sr.box_hits_along(a, b, [[2.0, 0.0], [0.0, 2.0]], BOX, 0.0)[0]
    assert sr.box_hits_along(a, b, [[-2.0, 0.0]], BOX, 0.0)[0]


def test_box_value_domain_and_translation():
    reach = sr.box_reach(BOX)
    a, b = seg(0, 0, 2, 0)
    # the point (1, 3): 2.5 above the box at either end (x inside [-1, 3] and [1, 5])
    v, k = sr.box_values(a, b, [[1.0, 3.0]], BOX)
    assert v[0] == 2.5 + 2.5 - 2.0 and k[0] == 0
    assert np.array_equal(sr.box_values(a, b, [[1.0, 3.0]], BOX, horizon=2.0)[0], [np.inf])
    # a wall point the box drives through, 1 in front of it at the start and 1 behind it at the end: no certificate
    a, b = seg(0, 0, 6, 0)
    v, _ = sr.box_values(a, b, [[4.0, 0.0]], BOX)
    assert v[0] == 1.0 + 1.0 - 6.0 and sr.box_hits_along(a, b, [[4.0, 0.0]], BOX, 0.0)[0]
    # poses more than 4 reaches apart are outside the certificate's domain
    a, b = seg(0, 0, 4.1 * reach, 0)
    assert sr.box_values(a, b, [[0.0, 50.0]], BOX)[0][0] == -np.inf


def test_the_three_statuses_of_the_reduction():
    poses = np.zeros((5, 3), F32)
    free = np.zeros(5, F32)
    # disc, radius 0.5
    labels, status, worst, at = sr.path_reduction(poses, [0.9, np.inf, 0.5, 0.7], free, 0.5, box=False)
    assert status == 0 and np.array_equal(labels, free) and worst == F32(0.5) and at == 2
    labels, status, worst, at = sr.path_reduction(poses, [0.9, 0.4, 0.6, 0.4], free, 0.5, box=False)
    assert status == 1 and np.array_equal(labels, [0, 1, 0, 1, 0]) and at == 1
    # box, slack 0.01: an uncertified segment between free poses is undecided, a pose in collision is a collision
    labels, status, worst, at = sr.path_reduction(poses, [0.9, 0.01, 0.6, -np.inf], free, 0.01, box=True)
    assert status == 2 and np.array_equal(labels, [0, 1, 0, 1, 0]) and worst == -np.inf and at == 3
    hit = np.array([0, 0, 0, 0, 1], F32)
    labels, status, _, _ = sr.path_reduction(poses, [0.9, 0.02, 0.6, 0.5], hit, 0.01, box=True)
    assert status == 1 and np.array_equal(labels, hit)
    assert sr.path_reduction(poses, [0.9, 0.02, 0.6, 0.5], free, 0.01, box=True)[1] == 0
    # a non-finite pose spoils both of its segments, whatever their values say
    bad = poses.copy()
    bad[2, 0] = np.nan
    labels, status, _, _ = sr.path_reduction(bad, [np.inf] * 4, free, 0.5, box=False)
    assert status == 1 and np.array_equal(labels, [0, 1, 1, 0, 0])


def test_the_library_states_the_slack_the_header_defines():
    lib = _lib.load()
    box = (ctypes.c_float * 4)(*BOX)
    slack = lib.nfopp_swept_slack(box)
    assert abs(slack - sr.box_reach(BOX) * 2.0 ** -16) <= 2.0 ** -23 * slack
    assert lib.nfopp_swept_slack(None) == 0.0
    for name in ("nfopp_swept_segments", "nfopp_swept_segments_cells", "nfopp_path_swept_labels", "nfopp_swept_slack"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_argument_checks_need_no_device():
    lib = _lib.load()
    box = (ctypes.c_float * 4)(*BOX)
    fake = ctypes.c_void_p(64)      # never dereferenced: every call below returns before a launch
    assert lib.nfopp_swept_segments(None, None, 0, 3, None, 0, None, 1.0, None, None, None) == 0
    assert lib.nfopp_swept_segments_cells(None, None, 0, 2, None, 0, None, 4, 4, 0.0, 0.0, 1.0, None, 0.0, None, None, None) == 0
    for horizon in (-1.0, float("nan")):
        assert lib.nfopp_swept_segments(fake, fake, 5, 3, fake, 7, None, horizon, fake, None, None) == -1
        assert lib.nfopp_swept_segments_cells(fake, fake, 5, 3, fake, 7, fake, 4, 4, 0.0, 0.0, 1.0, box, horizon, fake, None,
                                              None) == -1
    assert lib.nfopp_swept_segments(fake, fake, 5, 2, fake, 7, box, 1.0, fake, None, None) == -1      # a box without headings
    assert lib.nfopp_swept_segments(fake, fake, 5, 4, fake, 7, None, 1.0, fake, None, None) == -1
    assert lib.nfopp_swept_segments_cells(fake, fake, 5, 3, fake, 7, fake, 0, 4, 0.0, 0.0, 1.0, None, 1.0, fake, None, None) == -1
    assert lib.nfopp_swept_segments_cells(fake, fake, 5, 3, fake, 7, fake, 4, 4, 0.0, 0.0, 0.0, None, 1.0, fake, None, None) == -1
    assert lib.nfopp_swept_segments(None, fake, 5, 3, fake, 7, None, 1.0, fake, None, None) == -1
    assert lib.nfopp_path_swept_labels(None, None, None, 0, 5, 2, 0.3, 0, None, None, None) == 0
    assert lib.nfopp_path_swept_labels(fake, fake, fake, 3, 1, 2, 0.3, 0, None, None, None) == -1    # a path needs two poses
    assert lib.nfopp_path_swept_labels(fake, fake, fake, 3, 5, 2, 0.3, 1, None, None, None) == -1    # a box without headings
    assert lib.nfopp_path_swept_labels(fake, fake, fake, 3, 5, 3, -0.1, 1, None, None, None) == -1
    assert b"horizon" in lib.nfopp_last_error() or b"slack" in lib.nfopp_last_error()
