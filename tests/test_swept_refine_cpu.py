"""Hand-computed cases that pin tests/swept_refine_ref.py, the float64 restatement of nfopp_swept_refine the GPU tests
compare the device with; the stackless pre-order step against a recursive walk; the path reduction; and, on the very inputs
of tests/test_gpu_swept_refine.py, that the comparison there is neither blunted by ambiguous segments nor confined to the
root.  No GPU."""
import ctypes

import numpy as np
import pytest

import swept_refine_cases as cases
import swept_refine_ref as rr
from nfopp import _lib

F32 = np.float32
SQUARE = (-0.5, 0.5, -0.5, 0.5)       # reach 0.7071: 4 reaches = 2.83
LONG = (-1.0, 1.0, -0.5, 0.5)         # reach 1.118: 4 reaches = 4.47
FREE, HIT, UNDECIDED = rr.FREE, rr.HIT, rr.UNDECIDED


def one(ax, bx, points, box, tha=0.0, thb=0.0, **kw):
    a, b = np.array([[ax, 0.0, tha]], F32), np.array([[bx, 0.0, thb]], F32)
    status, s, depth, _ = rr.refine(a, b, np.asarray(points, F32).reshape(-1, 2), box, **kw)
    return int(status[0]), float(s[0]), int(depth[0])


def test_a_certified_root_is_free_at_depth_0():
    # the point is 4.5 above the box at either end, delta = 1: value 8
    assert one(0, 1, [[0.5, 5.0]], LONG) == (FREE, -1.0, 0)


def test_an_end_pose_that_hits():
    assert one(0, 1, [[0.5, 0.0]], LONG) == (HIT, 0.0, 0)          # inside the box at a (x in (-1, 1)) and at b
    assert one(0, 1, [[1.8, 0.0]], LONG) == (HIT, 1.0, 0)          # inside the box at b (x in (0, 2)) only
    assert one(0, 1, [[1.8, 0.0], [-0.5, 0.2]], LONG) == (HIT, 0.0, 0)   # a is asked first


def test_a_box_passing_over_a_point_between_free_end_poses():
    # the box covers x in (4 s - 1, 4 s + 1): (-1, 1) at a, (3, 5) at b, (1, 3) at the midpoint
    assert one(0, 4, [[2.0, 0.2]], LONG) == (HIT, 0.5, 0)
    assert one(0, 4, [[2.0, 0.2]], LONG, max_depth=0) == (UNDECIDED, -1.0, 0)      # no midpoint is asked at the limit
    assert one(0, 1, [[0.5, 5.0]], LONG, max_depth=0) == (FREE, -1.0, 0)


def test_the_first_hit_in_pre_order():
    # the square covers x in (2 s - 0.5, 2 s + 0.5): x = 0.5 is on the rim at s = 0 and 0.5 (not a hit: strictly inside) and
    # inside at 0.25; x = 1.5 is inside at 0.75 only
    assert one(0, 2, [[0.5, 0.0]], SQUARE) == (HIT, 0.25, 1)
    status, s, _ = one(0, 2, [[1.5, 0.0]], SQUARE)
    assert (status, s) == (HIT, 0.75)
    status, s, depth = one(0, 2, [[1.5, 0.0], [0.5, 0.0]], SQUARE)
    assert (status, s, depth) == (HIT, 0.25, 1)                  # the left half is walked first, and the walk stops there


def test_a_long_segment_in_a_free_corridor_is_split_until_the_domain_rule_lets_it_pass():
    # delta = 8 > 4 reaches, and 4 still is; the four pieces of 2 are certified: the point keeps 2.5 from the box
    assert one(0, 8, [[4.0, 3.0]], SQUARE) == (FREE, -1.0, 2)
    assert one(0, 8, [[4.0, 3.0]], SQUARE, max_depth=1) == (UNDECIDED, -1.0, 1)
    # 10 evaluations: 7 pieces and 3 midpoints.  9 stop it in front of the last piece
    assert one(0, 8, [[4.0, 3.0]], SQUARE, node_budget=10) == (FREE, -1.0, 2)
    assert one(0, 8, [[4.0, 3.0]], SQUARE, node_budget=9) == (UNDECIDED, -1.0, 2)


def test_a_raw_turn_above_8_pi():
    """theta_b = 26 is 0.867 beyond 8 pi.  The walk turns the short way (0.867), but the last piece ends on b's raw heading, so
    its raw difference stays above 8 pi at every depth: undecided at the limit, 1 + 2 max_depth pieces tested.  With the
    heading wrapped the same motion is certified at the root."""
    far = [[0.0, 50.0]]
    assert one(0, 0, far, SQUARE, thb=26.0, max_depth=3) == (UNDECIDED, -1.0, 3)
    assert one(0, 0, far, SQUARE, thb=26.0, max_depth=3, node_budget=10) == (UNDECIDED, -1.0, 3)
    assert one(0, 0, far, SQUARE, thb=float(rr.wrap_f32(F32(26.0))), max_depth=3) == (FREE, -1.0, 0)
    assert abs(float(rr.wrap_f32(F32(26.0))) - (26.0 - 8 * np.pi)) < 1e-5


def test_sliding_beside_a_row_of_points():
    # 1e-4 of clearance: a piece is certified once its delta is below 2e-4 - slack, depth 14 for a delta of 2
    row = np.stack([np.arange(-1.0, 3.0, 0.05), np.full(80, 0.5 + 1e-4)], 1)
    assert one(0, 2, row, SQUARE) == (UNDECIDED, -1.0, 8)
    assert one(0, 2, row, SQUARE, max_depth=14, node_budget=64) == (UNDECIDED, -1.0, 14)   # the budget, 28 levels down the left
    status, s, depth = one(0, 2, row, SQUARE, node_budget=3)      # the root, its midpoint, its left half
    assert (status, s) == (UNDECIDED, -1.0) and depth <= 1 and depth == 1
    assert one(0, 2, row, SQUARE, node_budget=1) == (UNDECIDED, -1.0, 0)
    assert one(0, 2, row, SQUARE, node_budget=2) == (UNDECIDED, -1.0, 0)


def test_non_finite_poses_and_the_empty_cloud():
    for bad in (np.nan, np.inf, -np.inf):
        assert one(bad, 1, [[0.5, 0.0]], LONG) == (UNDECIDED, -1.0, 0)          # though the point is inside the box at b
        assert one(0, 1, [[0.5, 5.0]], LONG, thb=bad) == (UNDECIDED, -1.0, 0)
    none = np.zeros((0, 2), F32)
    assert one(0, 1, none, LONG) == (FREE, -1.0, 0)
    assert one(0, 800, none, LONG, thb=30.0) == (FREE, -1.0, 0)                 # an empty cloud certifies everything
    assert one(np.nan, 1, none, LONG) == (UNDECIDED, -1.0, 0)


def test_sub_poses():
    a, b = np.array([[1.0, 2.0, 3.0]], F32), np.array([[3.0, -2.0, -3.0]], F32)
    turn = 2 * np.pi - 6.0                                        # the short way from 3 to -3 goes up through pi
    assert np.array_equal(rr.sub_poses(a, b, [0], [3]), a) and np.array_equal(rr.sub_poses(a, b, [8], [3]), b)
    got = rr.sub_poses(a, b, [3], [2])[0]
    assert got[0] == 2.5 and got[1] == -1.0 and abs(got[2] - (3.0 + 0.75 * turn)) < 1e-6


def test_the_stackless_successor_rule_walks_in_pre_order():
    for depth_limit in range(6):
        for pattern in range(8):
            def leaf(d, i):
                return d == depth_limit or (pattern and (d * 7 + i * 13 + pattern * 5) % (pattern + 1) == 0 and d > 0)
            want = []

            def visit(d, i):
                want.append((d, i))
                if not leaf(d, i):
                    visit(d + 1, 2 * i)
                    visit(d + 1, 2 * i + 1)
            visit(0, 0)
            got, d, i = [], 0, 0
            while True:
                got.append((d, i))
                if not leaf(d, i):
                    d, i = d + 1, 2 * i
                    continue
                nd, ni, done = rr.successor([d], [i])
                if done[0]:
                    break
                d, i = int(nd[0]), int(ni[0])
            assert got == want, (depth_limit, pattern)
    assert len(want) >= 3       # the last pattern at depth 5 is a tree, not a root


def test_the_three_statuses_of_the_reduction_and_first():
    free = np.zeros(5, F32)
    labels, status, first = rr.path_reduction([0, 0, 0, 0], [-1, -1, -1, -1], free)
    assert status == 0 and np.array_equal(labels, free) and first == (-1.0, -1.0)
    labels, status, first = rr.path_reduction([0, 2, 0, 2], [-1, -1, -1, -1], free)
    assert status == 2 and np.array_equal(labels, [0, 1, 0, 1, 0]) and first == (1.0, -1.0)
    labels, status, first = rr.path_reduction([0, 2, 1, 0], [-1, -1, 0.375, -1], free)
    assert status == 1 and np.array_equal(labels, [0, 1, 1, 0, 0]) and first == (1.0, -1.0)
    labels, status, first = rr.path_reduction([0, 0, 1, 0], [-1, -1, 0.375, -1], free)
    assert status == 1 and first == (2.0, 0.375)
    hit = np.array([0, 0, 0, 0, 1], F32)                           # the last pose keeps its label, and it is a collision
    labels, status, first = rr.path_reduction([0, 0, 0, 2], [-1] * 4, hit)
    assert status == 1 and np.array_equal(labels, [0, 0, 0, 1, 1]) and first == (3.0, -1.0)
    assert rr.path_reduction([0, 0, 0, 0], [-1] * 4, hit)[1:] == (1, (-1.0, -1.0))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_the_gpu_inputs_are_decisive_and_reach_below_the_root(name, kind):
    """At most 2 % of a set's segments may be ambiguous (they are left out of the GPU comparison), and at least 1 % must end
    UNDECIDED or HIT with a piece tested at depth >= 1, or the comparison would exercise the root alone.  The empty cloud
    cannot do the second: every finite segment is certified at its root.  The two dense clouds met it only after a share of
    their segments was replaced by ones that clip a corner of the cloud (swept_refine_cases.corner_clipping)."""
    status, s, depth, ambiguous = cases.reference(name, kind)
    below = (status != FREE) & (depth >= 1)
    print("%s %s: ambiguous %.4f, not free at depth >= 1 %.4f, free / hit / undecided %s, deepest %d"
          % (name, kind, ambiguous.mean(), below.mean(), np.bincount(status, minlength=3).tolist(), depth.max()))
    assert ambiguous.mean() <= 0.02
    if len(cases.sorted_points(name)) == 0:
        assert (depth == 0).all() and not (status == HIT).any()
        return
    assert below.mean() >= 0.01
    assert ((s >= 0) == (status == HIT)).all() and (s[status != HIT] == -1).all()


def test_the_library_exports_the_entries():
    lib = _lib.load()
    for name in ("nfopp_swept_refine", "nfopp_swept_refine_cells", "nfopp_path_refined_labels"):
        assert name in _lib._SIGNATURES and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.nfopp_abi_version() == 6


def test_argument_checks_need_no_device():
    lib = _lib.load()
    box = (ctypes.c_float * 4)(*LONG)
    fake = ctypes.c_void_p(64)      # never dereferenced: every call below returns before a launch

    def brute(a=fake, b=fake, n=5, dim=3, box4=box, depth=8, budget=1024, status=fake):
        return lib.nfopp_swept_refine(a, b, n, dim, fake, 7, box4, depth, budget, status, None, None, None)

    def cells(a=fake, b=fake, n=5, dim=3, box4=box, depth=8, budget=1024, status=fake, nx=4, size=1.0):
        return lib.nfopp_swept_refine_cells(a, b, n, dim, fake, 7, fake, nx, 4, 0.0, 0.0, size, box4, depth, budget, status, None,
                                            None, None)
    for entry in (brute, cells):
        assert entry(n=0, a=None, b=None, status=None) == 0                      # n = 0 is a no-op
        assert entry(a=None) == -1 and entry(b=None) == -1 and entry(status=None) == -1
        assert entry(box4=None) == -1 and entry(dim=2) == -1 and entry(n=-1) == -1
        assert entry(depth=-1) == -1 and entry(depth=21) == -1
        assert entry(budget=0) == -1 and entry(budget=-5) == -1
    assert b"node_budget" in lib.nfopp_last_error()
    assert cells(nx=0) == -1 and cells(size=0.0) == -1
    assert lib.nfopp_path_refined_labels(None, None, None, 0, 5, None, None, None) == 0
    assert lib.nfopp_path_refined_labels(fake, fake, fake, 3, 1, None, None, None) == -1     # a path needs two poses
    assert lib.nfopp_path_refined_labels(None, fake, fake, 3, 5, None, None, None) == -1
    assert lib.nfopp_path_refined_labels(fake, None, fake, 3, 5, None, fake, None) == -1     # first needs the s values
