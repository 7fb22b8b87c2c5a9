"""GPU tests of nfopp_swept_refine / nfopp_swept_refine_cells / nfopp_path_refined_labels (csrc/swept.hip) and of the Python
layer over them: bit identity between the all-pairs and the indexed entry, the max_depth = 0 answer against the existing
certificate on the device, equality with the float64 restatement of tests/swept_refine_ref.py on every segment it does not
call ambiguous, soundness of FREE and HIT against a float64 brute-force sampler without a tolerance, decisiveness at the
depth the header's termination bound names, the evaluation budget, and the planner-level wall."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
import swept_ref as sr  # noqa: E402
import swept_refine_cases as cases  # noqa: E402
import swept_refine_ref as rr  # noqa: E402
import test_gpu_clearance as tgc  # noqa: E402
import test_gpu_swept as tgs  # noqa: E402
from nfopp import _lib  # noqa: E402

F32 = np.float32
NAMES, KINDS = cases.NAMES, cases.KINDS
DEPTHS = (0, 3, 8)
COUNTS = (1, 255, 257)
SAMPLES = 1025
FREE, HIT, UNDECIDED = rr.FREE, rr.HIT, rr.UNDECIDED
dev = tgc.dev


class Entries(object):
    """Both C entries over one of test_gpu_clearance's clouds and its index."""

    def __init__(self, name):
        self.cloud = tgc.Device(name)
        self.box = tgc.box_of(name)

    def run(self, cells, a, b, max_depth=8, node_budget=1024, with_s=True, with_depth=True, check=True, box=True, dim=3,
            outputs=None):
        n = a.shape[0]
        status = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
        s = torch.full((n,), -5.0, device="cuda") if with_s else None
        depth = torch.full((n,), 77, dtype=torch.uint8, device="cuda") if with_depth else None
        if outputs is not None:
            status, s, depth = outputs
        x0, y0, size, nx, ny = self.cloud.geom
        index = (_lib.ptr(self.cloud.start, torch.int32), nx, ny, float(x0), float(y0), float(size)) if cells else ()
        entry = _lib.load().nfopp_swept_refine_cells if cells else _lib.load().nfopp_swept_refine
        rc = entry(_lib.ptr(a), _lib.ptr(b), n, dim, _lib.ptr(self.cloud.sorted), self.cloud.n, *index,
                   (ctypes.c_float * 4)(*self.box) if box else None, max_depth, node_budget, _lib.ptr(status, torch.uint8),
                   _lib.ptr(s), _lib.ptr(depth, torch.uint8), _lib.stream_ptr())
        if not check:
            return rc
        _lib.check(rc)
        return tuple(None if t is None else t.cpu().numpy() for t in (status, s, depth))


_CACHE = {}


def results(name, kind):
    """(entries, a, b, device a, device b, {max_depth: (all-pairs outputs, indexed outputs)}), computed once, left unchanged."""
    key = (name, kind)
    if key not in _CACHE:
        if name not in _CACHE:
            _CACHE[name] = Entries(name)
        entries = _CACHE[name]
        a, b = cases.segments(name, kind)
        da, db = dev(a), dev(b)
        runs = {d: (entries.run(False, da, db, d), entries.run(True, da, db, d)) for d in DEPTHS}
        _CACHE[key] = (entries, a, b, da, db, runs)
    return _CACHE[key]


def same(x, y):
    return all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


def motion(a, b, s):
    """float64 poses [..., 3] of the motion at parameters s (broadcast against the segments), from the fp32 inputs."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    dth = sr.wrap(b[..., 2] - a[..., 2])
    return a[..., 0] + s * (b[..., 0] - a[..., 0]), a[..., 1] + s * (b[..., 1] - a[..., 1]), a[..., 2] + s * dth


def robot_frame(x, y, th, o):
    dx, dy = o[..., 0] - x, o[..., 1] - y
    c, sn = np.cos(th), np.sin(th)
    return c * dx + sn * dy, c * dy - sn * dx


def sampled(a, b, points, box, grow, reach, margin):
    """The loop of swept_ref.box_hits_along with 1025 parameters, float64, over the (segment, point) pairs that can matter:
    a point farther than reach + margin from the segment of the robot's origins is never within `margin` of the box.
    -> (hit [n]: a point strictly inside the box grown by `grow` on every edge at one of the parameters,
        clearance [n]: the smallest distance from a point to the box over the parameters, +inf without a pair)."""
    n = len(a)
    hit, clearance = np.zeros(n, bool), np.full(n, np.inf)
    pts = points.astype(np.float64).reshape(-1, 2)
    if len(pts) == 0 or n == 0:
        return hit, clearance
    si, pi = [], []
    for k in range(0, n, 512):
        close = sr.segment_distances(a[k:k + 512], b[k:k + 512], pts) <= 1.01 * reach + margin
        u, v = np.nonzero(close)
        si.append(u + k)
        pi.append(v)
    si, pi = np.concatenate(si), np.concatenate(pi)
    bx = np.asarray(box, F32).astype(np.float64)
    s = np.linspace(0.0, 1.0, SAMPLES)[None, :]
    for k in range(0, len(si), 4096):
        u, v = si[k:k + 4096], pi[k:k + 4096]
        x, y, th = motion(a[u][:, None, :], b[u][:, None, :], s)
        rx, ry = robot_frame(x, y, th, pts[v][:, None, :])
        inside = (rx > bx[0] - grow) & (rx < bx[1] + grow) & (ry > bx[2] - grow) & (ry < bx[3] + grow)
        ex = np.maximum(np.maximum(bx[0] - rx, rx - bx[1]), 0.0)
        ey = np.maximum(np.maximum(bx[2] - ry, ry - bx[3]), 0.0)
        np.logical_or.at(hit, u, inside.any(1))
        np.minimum.at(clearance, u, np.sqrt(ex * ex + ey * ey).min(1))
    return hit, clearance


# ---- the two entries, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_indexed_and_all_pairs_entries_are_bit_identical(name, kind):
    entries, a, b, da, db, runs = results(name, kind)
    for max_depth, (brute, cells) in runs.items():
        assert same(brute, cells), max_depth
        status, s, depth = brute
        assert status.max() <= 2 and depth.max() <= max_depth
        assert ((s >= 0) == (status == HIT)).all() and (s[status != HIT] == -1).all() and (s <= 1).all()
    brute = runs[8][0]
    assert same(entries.run(True, da, db, 8), brute) and same(entries.run(False, da, db, 8), brute)      # run to run
    for count in COUNTS:               # every count is a launch of its own: the prefixes give the prefixes' results
        pa, pb = dev(a[:count]), dev(b[:count])
        for cells in (False, True):
            assert same(entries.run(cells, pa, pb, 8), [t[:count] for t in brute]), count
    for cells in (False, True):        # null s or depth changes nothing else
        status, s, depth = entries.run(cells, da, db, 8, with_s=False)
        assert s is None and same((status, depth), (brute[0], brute[2]))
        status, s, depth = entries.run(cells, da, db, 8, with_depth=False)
        assert depth is None and same((status, s), brute[:2])
        status, s, depth = entries.run(cells, da, db, 8, with_s=False, with_depth=False)
        assert same((status,), brute[:1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_max_depth_0_is_the_existing_certificate(name, kind):
    """status == 0 <=> nfopp_swept_segments_cells' value > slack, wherever no end pose hits; and an evaluation budget of 1
    pays for the root piece alone, so it gives the max_depth = 0 answer at any depth."""
    entries, a, b, da, db, runs = results(name, kind)
    status, s, depth = runs[0][0]
    slack = tgs.slack_of(name)
    value, _ = tgs.Entries(name).cells(da, db, entries.box, slack)
    ends = status == HIT
    assert np.isin(s[ends], (0.0, 1.0)).all() and (depth == 0).all()
    ok = sr.finite_segments(a, b, entries.box)
    # a non-finite segment's value is +inf today, and nfopp_path_swept_labels reads it as not certified: UNDECIDED here
    assert np.array_equal(status[ok & ~ends] == FREE, value[ok & ~ends] > F32(slack))
    assert (status[~ok] == UNDECIDED).all() and np.isposinf(value[~ok]).all()
    labels = nfopp.DeviceRectangleChecker(tgc.CLOUDS[name][0], entries.box)
    hit_a, hit_b = (labels.labels(t).cpu().numpy() != 0 for t in (da, db))
    assert np.array_equal(ends[ok], (hit_a | hit_b)[ok]) and np.array_equal(s[ok & ends] == 0.0, hit_a[ok & ends])
    for cells in (False, True):
        assert same(entries.run(cells, da, db, 8, node_budget=1), runs[0][0])
    # what depth 0 decides, every depth decides the same way
    for max_depth in (3, 8):
        deeper = runs[max_depth][0]
        decided = status != UNDECIDED
        assert same([t[decided] for t in deeper], [t[decided] for t in runs[0][0]])


@pytest.mark.parametrize("rows", cases.BEYOND, ids=lambda rows: "%d_%d_%d" % rows)
def test_indexed_walk_beyond_the_staged_candidates(rows):
    """Every segment's window is the whole 3 x 3 index, which holds more than the 1024 candidates a wave keeps in LDS, and
    the points that decide the segments are candidates beyond them: the indexed walk reads them from global memory, row by
    row, from where the staged ones end -- between two rows, inside the last row, inside the first (the preconditions are
    swept_refine_cases.beyond_the_stage's)."""
    name, points, geom, box, a, b, refs = cases.beyond_the_stage(rows)
    tgc.CLOUDS[name] = (points, geom)          # Entries reads the cloud by name
    try:
        entries = Entries(name)
    finally:
        del tgc.CLOUDS[name]
    assert entries.box == box and entries.cloud.n == sum(rows)
    da, db = dev(a), dev(b)
    for max_depth in DEPTHS:
        brute, cells = entries.run(False, da, db, max_depth), entries.run(True, da, db, max_depth)
        assert same(brute, cells), max_depth
        status, s, depth = brute
        want_status, want_s, want_depth, ambiguous = refs[max_depth]
        differ = ~ambiguous & ((status != want_status) | (s != want_s) | (depth != want_depth))
        print("%s depth %d: ambiguous %d, device free / hit / undecided %s, differing %d"
              % (name, max_depth, ambiguous.sum(), np.bincount(status, minlength=3).tolist(), differ.sum()))
        assert not differ.any(), (max_depth, np.flatnonzero(differ)[:8])


# ---- against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_equal_to_the_float64_restatement_wherever_it_is_not_ambiguous(name, kind):
    _, a, b, _, _, runs = results(name, kind)
    status, s, depth = runs[8][0]
    want_status, want_s, want_depth, ambiguous = cases.reference(name, kind)
    clear = ~ambiguous
    differ = clear & ((status != want_status) | (s != want_s) | (depth != want_depth))
    print("%s %s: ambiguous %.4f; device free / hit / undecided %s, decided below the root %.4f, differing %d"
          % (name, kind, ambiguous.mean(), np.bincount(status, minlength=3).tolist(), (depth >= 1).mean(), differ.sum()))
    assert not differ.any(), np.flatnonzero(differ)[:8]


@pytest.mark.parametrize("budget", [2, 3, 10])
@pytest.mark.parametrize("name", NAMES)
def test_the_evaluation_budget_stops_the_walk_where_the_restatement_stops(name, budget):
    """The long set at max_depth = 8 with 2, 3 and 10 evaluations: the walk of pass 2 ends on its budget, in front of a
    midpoint (2), of a piece (3) and several levels down (10).  A full walk at depth 8 costs at most 511 + 255 = 766, so the
    default budget never ends one."""
    entries, a, b, da, db, runs = results(name, "long")
    brute, cells = entries.run(False, da, db, 8, budget), entries.run(True, da, db, 8, budget)
    assert same(brute, cells)
    status, s, depth = brute
    want_status, want_s, want_depth, ambiguous = cases.reference(name, "long", 8, budget)
    clear = ~ambiguous
    differ = clear & ((status != want_status) | (s != want_s) | (depth != want_depth))
    assert not differ.any(), np.flatnonzero(differ)[:8]
    full = runs[8][0]
    cut = (status == UNDECIDED) & (full[0] != UNDECIDED)
    print("%s budget %d: stopped by the budget %.4f, deepest %d" % (name, budget, cut.mean(), depth.max()))
    assert depth.max() <= (budget - 1) // 2            # a piece at depth d is the (2 d + 1)th evaluation at the earliest
    if entries.cloud.n:
        assert cut.mean() >= 0.01
    # what the budget leaves decided is what the full walk decides
    decided = status != UNDECIDED
    assert same([t[decided] for t in brute], [t[decided] for t in full])


# ---- soundness, no tolerance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_free_and_hit_are_proofs(name, kind):
    """Every FREE segment has no obstacle inside the box shrunk by 4 slack at any of 1025 parameters; every HIT has one inside
    the float64 box grown by 4 slack at its s."""
    entries, a, b, _, _, runs = results(name, kind)
    pts, box = entries.cloud.sorted_np, entries.box
    reach = sr.box_reach(box)
    slack = reach * 2.0 ** -16
    for max_depth in (3, 8):
        status, s, _ = runs[max_depth][0]
        free = status == FREE
        swept_through, _ = sampled(a[free], b[free], pts, box, -4 * slack, reach, 0.0)
        assert not swept_through.any(), (max_depth, np.flatnonzero(free)[swept_through][:8])
        hit = np.flatnonzero(status == HIT)
        if len(hit) == 0:
            continue
        assert len(pts)
        x, y, th = motion(a[hit], b[hit], s[hit].astype(np.float64))
        inside = np.zeros(len(hit), bool)
        bx = np.asarray(box, F32).astype(np.float64)
        for k in range(0, len(hit), 256):
            rx, ry = robot_frame(x[k:k + 256, None], y[k:k + 256, None], th[k:k + 256, None], pts.astype(np.float64)[None])
            inside[k:k + 256] = ((rx > bx[0] - 4 * slack) & (rx < bx[1] + 4 * slack) & (ry > bx[2] - 4 * slack)
                                 & (ry < bx[3] + 4 * slack)).any(1)
        assert inside.all(), (max_depth, hit[~inside][:8])


# ---- decisiveness ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_segments_with_clearance_are_decided_by_the_depth_of_the_termination_bound(name, kind):
    """A segment whose sampled float64 clearance is at least c = 0.05 reach is not UNDECIDED at
    max_depth = ceil(log2(delta / (2 c - slack))) + 1.  The evaluation budget is lifted out of the way: the bound speaks of
    the depth.  (The sampler sees the clearance every delta / 1024; the + 1 halves the pieces once more than the argument
    needs, which covers that as it covers the rounding.)"""
    entries, a, b, _, _, _ = results(name, kind)
    pts, box = entries.cloud.sorted_np, entries.box
    reach = sr.box_reach(box)
    slack, c = reach * 2.0 ** -16, 0.05 * reach
    ok = sr.finite_segments(a, b, box)
    _, clearance = sampled(a[ok], b[ok], pts, box, 0.0, reach, c)
    roomy = np.flatnonzero(ok)[clearance >= c]
    delta = sr.delta(a[roomy], b[roomy], reach)
    need = np.where(delta > 0, np.ceil(np.log2(np.maximum(delta, 1e-300) / (2 * c - slack))) + 1, 0).clip(0, None).astype(int)
    assert len(roomy) >= 400 and need.max() <= 20 and (need >= 2).sum() >= 40, (len(roomy), need.max())
    for max_depth in np.unique(need):
        pick = roomy[need == max_depth]
        for cells in (False, True):
            status, _, depth = entries.run(cells, dev(a[pick]), dev(b[pick]), int(max_depth), node_budget=1 << 24)
            assert (status != UNDECIDED).all() and depth.max() <= max_depth, (max_depth, pick[status == UNDECIDED][:8])


# ---- the path reduction ------------------------------------------------------------------------------------------------
def test_path_reduction_equals_the_restatement():
    """B = 6 paths of m = 259 poses (two strides of the workgroup and a remainder): every status, a hit behind an undecided
    segment, only the last pose in collision, nothing to report."""
    rng = np.random.default_rng(43)
    B, m = 6, 259
    seg = np.zeros((B, m - 1), np.uint8)
    s = np.full((B, m - 1), -1.0, F32)
    labels = np.zeros((B, m), F32)
    seg[1, 200], seg[1, 77] = UNDECIDED, UNDECIDED
    seg[2, 257], seg[2, 256], s[2, 257] = HIT, UNDECIDED, 0.375
    labels[3, m - 1] = 1.0
    seg[4] = rng.integers(0, 3, m - 1)
    s[4][seg[4] == HIT] = rng.integers(0, 257, (seg[4] == HIT).sum()) / F32(256)
    seg[5, 0], s[5, 0] = HIT, 1.0
    lib = _lib.load()
    d_seg, d_s = dev(seg, np.uint8), dev(s)
    got = dev(labels.reshape(-1))
    status = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    first = torch.full((B, 2), -7.0, device="cuda")
    _lib.check(lib.nfopp_path_refined_labels(_lib.ptr(d_seg, torch.uint8), _lib.ptr(d_s), _lib.ptr(got), B, m,
                                             _lib.ptr(status, torch.uint8), _lib.ptr(first), _lib.stream_ptr()))
    got, status, first = got.cpu().numpy().reshape(B, m), status.cpu().numpy(), first.cpu().numpy()
    for p in range(B):
        want, st, fs = rr.path_reduction(seg[p], s[p], labels[p])
        assert np.array_equal(got[p], want) and status[p] == st and tuple(first[p]) == fs, p
    assert status.tolist()[:4] == [0, 2, 1, 1] and status[5] == 1
    assert first[0].tolist() == [-1, -1] and first[1].tolist() == [77, -1] and first[2].tolist() == [256, -1]
    assert first[3].tolist() == [-1, -1] and first[5].tolist() == [0, 1]
    again = dev(labels.reshape(-1))       # status and first may be null, and then the s values too: the labels are the same
    _lib.check(lib.nfopp_path_refined_labels(_lib.ptr(d_seg, torch.uint8), None, _lib.ptr(again), B, m, None, None,
                                             _lib.stream_ptr()))
    assert np.array_equal(again.cpu().numpy().reshape(B, m), got)


@pytest.mark.parametrize("m", [2, 65, 257, 600])
def test_path_reduction_across_wave_and_stride_boundaries(m):
    """The same reduction with fewer poses than one wave, a count that ends inside the second wave, one pose beyond a stride
    of the workgroup and more than two strides: the only segment that is not free at the far end, a hit there behind an
    undecided segment in the middle, only the last pose in collision, a random mix."""
    rng = np.random.default_rng(53 + m)
    B = 5
    seg = np.zeros((B, m - 1), np.uint8)
    s = np.full((B, m - 1), -1.0, F32)
    labels = np.zeros((B, m), F32)
    seg[1, m - 2] = UNDECIDED
    seg[2, (m - 2) // 2] = UNDECIDED
    seg[2, m - 2], s[2, m - 2] = HIT, 0.375
    labels[3, m - 1] = 1.0
    seg[4] = rng.integers(0, 3, m - 1)
    s[4][seg[4] == HIT] = rng.integers(0, 257, (seg[4] == HIT).sum()) / F32(256)
    lib = _lib.load()
    d_seg, d_s = dev(seg, np.uint8), dev(s)
    got = dev(labels.reshape(-1))
    status = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    first = torch.full((B, 2), -7.0, device="cuda")
    _lib.check(lib.nfopp_path_refined_labels(_lib.ptr(d_seg, torch.uint8), _lib.ptr(d_s), _lib.ptr(got), B, m,
                                             _lib.ptr(status, torch.uint8), _lib.ptr(first), _lib.stream_ptr()))
    got, status, first = got.cpu().numpy().reshape(B, m), status.cpu().numpy(), first.cpu().numpy()
    for p in range(B):
        want, st, fs = rr.path_reduction(seg[p], s[p], labels[p])
        assert np.array_equal(got[p], want) and status[p] == st and tuple(first[p]) == fs, p
    assert status.tolist()[:4] == [0, 2, 1, 1]
    assert first[0].tolist() == [-1, -1] and first[1].tolist() == [m - 2, -1] and first[3].tolist() == [-1, -1]
    assert first[2].tolist() == ([0, 0.375] if m == 2 else [(m - 2) // 2, -1])


# ---- the planner and the wall ------------------------------------------------------------------------------------------
def wall_planner():
    """DESIGN 14's wall with the box robot: B = 4 straight paths of N = 8 waypoints, 10 poses 1 apart along x from -4.5 to 4.5
    (sub = 1: the dense poses are the waypoints).  Path 0 crosses the wall at y = 0 with its nearest poses 0.5 either side
    of it; path 1 runs 2 beyond the wall's end; path 2 is path 0 at y = 1 with one waypoint pushed into the wall; path 3
    passes the wall's end at y = 3.45, the box's side 0.3 from the last point: d_a + d_b = 0.78 for the segment of length 1
    that passes it, no certificate, and free -- its halves have 2 * 0.3 > 0.5."""
    torch.random.manual_seed(5)
    onf = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=True).to("cuda")
    paths = np.zeros((4, 10, 3), F32)
    paths[:, :, 0] = -4.5 + np.arange(10.0)
    paths[1, :, 1], paths[2, :, 1], paths[3, :, 1] = 5.0, 1.0, 3.45
    paths[2, 5, 0] = 0.05
    bounds = (-6.0, 6.0, -6.0, 6.0)
    planner = nfopp.BatchPlanner(onf, 4, 8, nfopp.TrajectoryHyper(bounds=bounds))
    planner.init(paths[:, 0], paths[:, -1], bounds, trajectories=paths[:, 1:-1])
    checker = nfopp.DeviceRectangleChecker(tgs.WALL, tgs.SMALL_BOX, bounds)
    assert checker.cells is not None
    return planner, checker, paths


def test_a_box_through_a_one_cell_wall_is_a_hit_and_a_box_past_its_end_is_free():
    planner, checker, paths = wall_planner()
    status, worst = planner.certify(checker, sub=1)
    assert status.cpu().tolist() == [2, 0, 1, 2]                   # today's answer, and it stays
    assert worst.cpu().numpy()[0, 1] == 4 and worst.cpu().numpy()[3, 1] == 4
    before = tgs.state(planner, planner.evaluate(checker, sub=1))
    status, first = planner.certify(checker, sub=1, refine=8)
    assert status.dtype == torch.uint8 and first.shape == (4, 2)
    assert status.cpu().tolist() == [1, 0, 1, 0]
    first = first.cpu().numpy()
    assert first[0].tolist() == [4.0, 0.5] and first[1].tolist() == [-1.0, -1.0] and first[3].tolist() == [-1.0, -1.0]
    assert first[2, 0] in (4.0, 5.0) and first[2, 1] in (0.0, 1.0)     # the pose in the wall ends segment 4, starts 5
    assert planner.certify(checker, sub=1, refine=0)[0].cpu().tolist() == [2, 0, 1, 2]
    assert tgs.state(planner, planner.evaluate(checker, sub=1)) == before          # certify leaves the bookkeeping alone
    # evaluate: without refine the path past the wall's end is never the best one, with it it is
    planner, checker, _ = wall_planner()
    collides, _ = planner.evaluate(checker, sub=1, swept=True)
    assert collides.cpu().tolist() == [1, 0, 1, 1]
    assert np.isfinite(planner.best_length.cpu().numpy()).tolist() == [False, True, False, False]
    plain = tgs.state(planner, (collides,))
    assert tgs.state(planner, (planner.evaluate(checker, sub=1, swept=True, refine=None)[0],)) == plain
    collides, _ = planner.evaluate(checker, sub=1, swept=True, refine=8)
    assert collides.cpu().tolist() == [1, 0, 1, 0]
    assert np.isfinite(planner.best_length.cpu().numpy()).tolist() == [False, True, False, True]
    assert np.array_equal(planner.best_traj.cpu().numpy()[3], paths[3, 1:-1])
    segments = planner._segments
    planner.evaluate(checker, sub=1, swept=True, refine=8)
    assert all(x is y for x, y in zip(segments, planner._segments))               # the cached buffers are reused


def test_who_refines():
    planner, checker, _ = wall_planner()
    poses = torch.zeros(4, 3, device="cuda")
    status, s, depth = checker.swept_refine(poses, poses + 0.25)
    assert status.dtype == torch.uint8 and s.dtype == torch.float32 and depth.dtype == torch.uint8 and status.shape == (4,)
    out = (torch.empty(4, dtype=torch.uint8, device="cuda"), torch.empty(4, device="cuda"),
           torch.empty(4, dtype=torch.uint8, device="cuda"))
    got = checker.swept_refine(poses, poses + 0.25, 3, 64, *out)
    assert all(x is y for x, y in zip(got, out)) and torch.equal(got[0], status)
    disc = nfopp.DeviceCircleChecker(tgs.WALL, 0.3)
    with pytest.raises(NotImplementedError, match="exact"):
        disc.swept_refine(poses, poses)
    grid = nfopp.DeviceGridChecker(np.zeros((8, 8), np.uint8), 0.0, 0.0, 0.5)
    with pytest.raises(NotImplementedError, match="DeviceRectangleChecker"):
        grid.swept_refine(poses, poses)
    with pytest.raises(ValueError):
        planner.certify(disc, sub=1, refine=8)
    with pytest.raises(ValueError):
        planner.evaluate(checker, sub=1, refine=8)                 # refine belongs to swept=True
    with pytest.raises(_lib.NfoppError, match="max_depth"):
        checker.swept_refine(poses, poses, max_depth=21)
    with pytest.raises(ValueError):
        planner.certify(grid, sub=1, refine=8)                     # not the box robot's checker: before anything is launched
    with pytest.raises(ValueError):
        planner.certify(checker, sub=1, refine=21)
    # a refused call launches nothing and overwrites nothing
    planner.evaluate(checker, sub=1)
    before = planner._pose_labels.clone()
    planner._pose_labels.fill_(7.0)
    with pytest.raises(ValueError):
        planner.evaluate(checker, sub=1, refine=8)
    with pytest.raises(ValueError):
        planner.evaluate(disc, sub=1, swept=True, refine=8)
    assert (planner._pose_labels == 7.0).all() and before.numel() == planner._pose_labels.numel()
    # outputs of the caller's are checked before the kernel sees them
    for bad in (dict(status_out=torch.empty(3, dtype=torch.uint8, device="cuda")), dict(s_out=torch.empty(4, dtype=torch.float64, device="cuda")),
                dict(depth_out=torch.empty(4, dtype=torch.float32, device="cuda")), dict(s_out=torch.empty(8, device="cuda")[::2]),
                dict(status_out=torch.empty(4, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="_out must be"):
            checker.swept_refine(poses, poses + 0.25, **bad)


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    entries, a, b, da, db, _ = results("n33", "short")
    pa, pb = da[:300].contiguous(), db[:300].contiguous()
    for cells in (False, True):
        outputs = (torch.full((300,), 77, dtype=torch.uint8, device="cuda"), torch.full((300,), -5.0, device="cuda"),
                   torch.full((300,), 77, dtype=torch.uint8, device="cuda"))
        kw = dict(check=False, outputs=outputs)
        assert entries.run(cells, pa, pb, box=False, **kw) != 0
        assert entries.run(cells, pa[:, :2].contiguous(), pb[:, :2].contiguous(), dim=2, **kw) != 0
        for max_depth in (-1, 21):
            assert entries.run(cells, pa, pb, max_depth, **kw) != 0
        for budget in (0, -3):
            assert entries.run(cells, pa, pb, 8, budget, **kw) != 0
        lib = _lib.load()
        box = (ctypes.c_float * 4)(*entries.box)
        x0, y0, size, nx, ny = entries.cloud.geom
        index = (_lib.ptr(entries.cloud.start, torch.int32), nx, ny, float(x0), float(y0), float(size)) if cells else ()
        entry = lib.nfopp_swept_refine_cells if cells else lib.nfopp_swept_refine
        for nulled in range(3):
            ptrs = [_lib.ptr(pa), _lib.ptr(pb), _lib.ptr(outputs[0], torch.uint8)]
            ptrs[nulled] = None
            assert entry(ptrs[0], ptrs[1], 300, 3, _lib.ptr(entries.cloud.sorted), entries.cloud.n, *index, box, 8, 1024,
                         ptrs[2], None, None, _lib.stream_ptr()) != 0
        assert entry(None, None, 0, 3, _lib.ptr(entries.cloud.sorted), entries.cloud.n, *index, box, 8, 1024, None, None, None,
                     _lib.stream_ptr()) == 0                       # n = 0 is a no-op
        torch.cuda.synchronize()
        assert (outputs[0] == 77).all() and (outputs[1] == -5.0).all() and (outputs[2] == 77).all()
