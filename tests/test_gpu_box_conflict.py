"""GPU: nfopp_track_headings against numpy's float64 cos / sin, and nfopp_box_track_conflicts (csrc/box_conflict.hip) against
the numpy restatement (tests/box_conflict_ref.py) run on the device's own unit vectors, bit for bit: pair status, both pair
times and the summaries of both sides, in self and A-against-B mode, at the sizes where the kernel takes another path (one
pair, a tile edge, several tiles, one and several chunks of instants); then the Python interface and the torch ops against
the raw calls."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
from nfopp import _lib, torch_ops  # noqa: E402

import box_conflict_cases as bc  # noqa: E402
import box_conflict_ref as br  # noqa: E402

F32, F64 = np.float32, np.float64
INF = np.inf
SIZES = ((1, 1, 1), (2, 2, 2), (31, 33, 33), (33, 65, 65), (67, 67, 130))
REFINES = (0, 3, 8)
OUTPUTS = ("summary", "summary_b", "pair_status", "pair_first", "pair_undecided")
# The largest |device - numpy| over both components of the unit vectors of 2^20 headings in +-8 pi, measured on an MI355X
# (DESIGN section 23); the test allows 4 times that, and never more than 1e-14.
HEADING_ERR_MEASURED = 1.1102230246251565e-16
HEADING_TOL = min(4.0 * HEADING_ERR_MEASURED, 1e-14)


def _dev(x, dtype=F32):
    return None if x is None else torch.tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda")


def _headings(t):
    """The raw headings pass on a [B, K, S] device tensor."""
    b, k, s = t.shape
    out = torch.full((b, k, 2), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().nfopp_track_headings(_lib.ptr(t), b, s, k, _lib.ptr(out, torch.float64), _lib.stream_ptr()))
    return out


def _raw(c, refine, pairs=True, side_b=True):
    """The C entries on case `c` with preallocated outputs -> (dict of device tensors (None where not asked for), the case with
    the device's unit vectors in place of numpy's)."""
    lib, L = _lib.load(), _lib
    a, b = _dev(c["a"]), _dev(c["b"])
    self_mode = b is None
    ba, k, sa = a.shape
    bb, sb = (0, 3) if self_mode else (b.shape[0], b.shape[2])
    ua, ub = _headings(a), None if self_mode or bb == 0 else _headings(b)
    box_a, box_b = _dev(c["box_a"]), _dev(c["box_b"])
    ra, rb = _dev(c["radius_a"]), _dev(c["radius_b"])
    f64 = dict(dtype=torch.float64, device="cuda")
    cols = ba if self_mode else bb
    out = dict(summary=torch.full((ba, 7), -7.0, **f64), summary_b=None, pair_status=None, pair_first=None, pair_undecided=None)
    if not self_mode and side_b:
        out["summary_b"] = torch.full((bb, 7), -7.0, **f64)
    if pairs:
        out["pair_status"] = torch.full((ba, cols), -7, dtype=torch.int32, device="cuda")
        out["pair_first"], out["pair_undecided"] = (torch.full((ba, cols), -7.0, **f64) for _ in range(2))
    nbytes = lib.nfopp_box_track_conflicts_workspace_bytes(ba, bb, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b_ptr = None if self_mode else (L.ptr(b) or L.ptr(a))
    L.check(lib.nfopp_box_track_conflicts(
        L.ptr(a), L.ptr(ua, torch.float64), ba, sa, b_ptr, L.ptr(ub, torch.float64), bb, sb, k, c["t0"], c["dt"], L.ptr(box_a),
        L.ptr(box_b), L.ptr(ra), L.ptr(rb), c["margin"], refine, L.ptr(out["summary"], torch.float64),
        L.ptr(out["summary_b"], torch.float64), L.ptr(out["pair_status"], torch.int32), L.ptr(out["pair_first"], torch.float64),
        L.ptr(out["pair_undecided"], torch.float64), L.ptr(ws, torch.uint8), nbytes, L.stream_ptr()))
    return out, dict(c, ua=ua.cpu().numpy(), ub=None if ub is None else ub.cpu().numpy())


def _bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _check(c, refine, label):
    got, on_device_units = _raw(c, refine)
    want = br.conflicts(on_device_units["a"], on_device_units["ua"], on_device_units["b"], on_device_units["ub"], **bc.kwargs(c, refine))
    for name in OUTPUTS:
        if want[name] is None:
            assert got[name] is None
            continue
        g, w = got[name].cpu().numpy(), want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (label, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(_bits(g), _bits(w)), (label, name, np.argwhere(_bits(g) != _bits(w))[:6], g.ravel()[:8], w.ravel()[:8])
    return got, want


def _equal(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and bool(np.array_equal(_bits(x), _bits(y)))


def test_unit_vectors_against_numpy():
    rng = np.random.default_rng(0)
    th = rng.uniform(-8 * np.pi, 8 * np.pi, (1024, 1024)).astype(F32)
    th.ravel()[:9] = [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 8 * np.pi, -8 * np.pi, 1e-30, -0.0]
    tracks = np.zeros((1024, 1024, 3), F32)
    tracks[:, :, 2] = th
    got = _headings(_dev(tracks)).cpu().numpy()
    want = np.stack([np.cos(th.astype(F64)), np.sin(th.astype(F64))], -1)
    err = float(np.abs(got - want).max())
    print("track_headings: max |device - numpy| over %d headings in +-8 pi = %.17g" % (th.size, err))
    assert err <= HEADING_TOL, err
    assert got[0, 0, 0] == 1.0 and got[0, 0, 1] == 0.0                      # theta = 0 is exact: the hand cases rest on it
    assert np.abs(np.hypot(got[..., 0], got[..., 1]) - 1.0).max() < 4e-16
    bad = np.zeros((2, 3, 4), F32)
    bad[0, 1, 2], bad[1, 2, 2] = np.nan, -np.inf
    u = _headings(_dev(bad)).cpu().numpy()
    assert np.isnan(u[0, 1]).all() and np.isnan(u[1, 2]).all() and np.isfinite(u).sum() == 2 * (6 - 2)
    assert _equal(nfopp.track_headings(_dev(tracks[:7])), torch.tensor(got[:7]))
    assert _equal(torch_ops.load().track_headings(_dev(tracks[:7])), torch.tensor(got[:7]))
    view = _dev(np.concatenate([tracks[:3], tracks[:3]], -1))[:, :, :3]            # rows keep their stride of 6
    assert _equal(nfopp.track_headings(view), torch.tensor(got[:3]))


@pytest.mark.parametrize("mode", ("ab", "self"))
@pytest.mark.parametrize("index,size", list(enumerate(SIZES)))
def test_equals_the_restatement_bit_for_bit(index, size, mode):
    ba, bb, k = size
    # every stride, one box for all or per-track boxes, radii on and off: each appears at a small and at a large size
    stride = (3, 4, 5)[(index + (mode == "self")) % 3]
    per_track, radii = bool((index + (mode == "self")) % 2), bool(index % 2) or index == 4
    c = bc.random_case(100 * index + (mode == "self"), ba, None if mode == "self" else bb, k, stride=stride, bad=True,
                       per_track_boxes=per_track, radii=radii, extent=max(8.0, 2.0 * np.sqrt(ba + bb)))
    seen = set()
    for refine in REFINES:
        got, want = _check(c, refine, (size, mode, refine))
        seen |= set(np.unique(want["pair_status"]))
        if mode == "self":
            for name in ("pair_status", "pair_first", "pair_undecided"):
                m = torch.as_tensor(_bits(got[name]))
                assert torch.equal(m, m.t()), name
        if refine == 3:
            again, _ = _raw(c, refine)                                       # the same bytes on a second run
            for name in OUTPUTS:
                assert got[name] is None or _equal(again[name], got[name]), name
            slim, _ = _raw(c, refine, pairs=False, side_b=False)             # null optional outputs
            assert _equal(slim["summary"], got["summary"])
    if ba > 2:
        assert seen >= {br.BAD_PAIR, br.FREE, br.CONFLICT, br.UNDECIDED}, seen
        bad = want["pairs"]["bad_a"]
        assert bad.sum() >= 1 and (got["summary"][torch.tensor(bad, device="cuda"), 6] == nfopp.BoxTrackConflicts.BAD_TRACK).all()


@pytest.mark.parametrize("stride", (3, 4, 5))
def test_strided_rows_with_junk_past_theta(stride):
    plain = bc.random_case(31, 33, 34, 18)
    c = bc.with_stride(plain, stride, seed=stride)
    got, _ = _check(c, 3, ("ab", stride))
    base, _ = _raw(plain, 3)
    for name in OUTPUTS:
        assert _equal(got[name], base[name]), name


def test_hand_cases_and_bad_tracks():
    for name, c in bc.hand_cases().items():
        all_east = all(np.array_equal(u[..., 0], np.ones_like(u[..., 0])) for u in (c["ua"], c["ub"]))
        for refine, expect in c["expect"].items():
            got, want = _check(c, refine, (name, refine))                   # the restatement on the device's unit vectors
            pair = (int(got["pair_status"][0, 0]), float(got["pair_first"][0, 0]), float(got["pair_undecided"][0, 0]))
            if all_east:
                assert pair == expect, (name, refine, pair)                  # theta = 0: the exact hand values
            elif name not in ("half_turn", "single_instant_miss"):           # those two rest on an exact pi and an exact touch
                assert pair[0] == expect[0], (name, refine, pair)
    for self_mode in (True, False):
        c = bc.bad_tracks(self_mode)
        got, want = _check(c, 2, ("bad", self_mode))
        assert (got["summary"][:, 6].cpu().numpy() == [0, 1, 0, 1, 1, 0]).all()


def test_python_interface_and_torch_ops_equal_the_raw_calls():
    ops = torch_ops.load()
    for c in (bc.random_case(41, 9, 6, 21, stride=4), bc.random_case(42, 9, None, 21)):
        raw, _ = _raw(c, 3)
        a, b = _dev(c["a"]), _dev(c["b"])
        res = nfopp.box_track_conflicts(a, b, dt=c["dt"], t0=c["t0"], box_a=c["box_a"], box_b=c["box_b"], radius_a=c["radius_a"],
                                        radius_b=c["radius_b"], margin=c["margin"], refine=3, want_pairs=True)
        assert isinstance(res, nfopp.BoxTrackConflicts)
        for name in OUTPUTS:
            assert (getattr(res, name) is None and raw[name] is None) or _equal(getattr(res, name), raw[name]), name
        lean = nfopp.box_track_conflicts(a, b, dt=c["dt"], t0=c["t0"], box_a=_dev(c["box_a"]), box_b=_dev(c["box_b"]),
                                         radius_a=_dev(c["radius_a"]), radius_b=_dev(c["radius_b"]), margin=c["margin"], refine=3)
        assert lean.pair_status is None and lean.pair_first is None and lean.pair_undecided is None   # no matrix is written
        assert _equal(lean.summary, raw["summary"])
        assert torch.equal(res.in_conflict, raw["summary"][:, 2] > 0) and torch.equal(res.undecided, raw["summary"][:, 5] > 0)
        o = ops.box_track_conflicts(a, b, c["dt"], c["t0"], _dev(c["box_a"]), _dev(c["box_b"]), _dev(c["radius_a"]),
                                    _dev(c["radius_b"]), c["margin"], 3, True)
        assert _equal(o[0], raw["summary"]) and all(_equal(o[q], raw[OUTPUTS[q]]) for q in (2, 3, 4))
        assert o[1].shape[0] == 0 if c["b"] is None else _equal(o[1], raw["summary_b"])
        o = ops.box_track_conflicts(a, b, c["dt"], c["t0"], _dev(c["box_a"]), _dev(c["box_b"]), None, None, 0.0, 0, False)
        assert o[2].numel() == 0 and o[3].numel() == 0 and o[0].shape == (9, 7)
    # one box and one radius for all tracks
    c = bc.random_case(43, 9, 6, 21, per_track_boxes=False)
    one = nfopp.box_track_conflicts(_dev(c["a"]), _dev(c["b"]), dt=0.25, box_a=bc.SWEPT_BOX, box_b=bc.SWEPT_BOX, radius_a=0.0625,
                                    radius_b=0.125, refine=2, want_pairs=True)
    raw, _ = _raw(dict(c, radius_a=np.full(9, 0.0625, F32), radius_b=np.full(6, 0.125, F32), t0=0.0, margin=0.0), 2)
    assert all(_equal(getattr(one, n), raw[n]) for n in OUTPUTS)
    # an empty set A: the entry writes nothing, the Python forms give every obstacle the "no partner" row
    empty = nfopp.box_track_conflicts(_dev(c["a"][:0]), _dev(c["b"]), dt=0.25, box_a=bc.SWEPT_BOX, box_b=bc.SWEPT_BOX, want_pairs=True)
    op_empty = ops.box_track_conflicts(_dev(c["a"][:0]), _dev(c["b"]), 0.25, 0.0, _dev(c["box_a"][:0]), _dev(c["box_b"]), None, None,
                                       0.0, 0, True)
    for sb in (empty.summary_b, op_empty[1]):
        assert sb.shape == (6, 7) and (sb[:, 6] == nfopp.BoxTrackConflicts.NO_PARTNER).all() and (sb[:, 1] == -1).all()
    assert empty.summary.shape == (0, 7) and empty.pair_status.shape == (0, 6)
    with pytest.raises(RuntimeError, match="must"):
        ops.box_track_conflicts(_dev(c["a"]), _dev(c["b"][:, :5]), 0.1, 0.0, _dev(c["box_a"]), _dev(c["box_b"]), None, None, 0.0, 0, False)
    with pytest.raises(nfopp.NfoppError, match="refine"):
        _raw(c, 9)


def test_neighbouring_lanes_through_the_time_parametrisation():
    """Two straight SE(2) paths in lanes 0.75 m apart, the car of profiles/swept.txt (0.54 m wide, circumscribed radius 0.48),
    timed under the same limits and sampled: free as boxes, in conflict as the circumscribed discs."""
    n = 8
    xs = np.linspace(0.0, 10.0, n + 2).astype(F32)
    paths = np.zeros((2, n + 2, 3), F32)
    paths[:, :, 0] = xs
    paths[1, :, 1] = 0.75
    lim = nfopp.MotionLimits(1.0, 1.0, w_max=1.0, cusp_angle=None)
    timed = nfopp.time_parametrize(_dev(paths[:, 1:-1]), _dev(paths[:, 0]), _dev(paths[:, -1]), lim)
    dt, count = 0.25, 48
    boxes = timed.conflicts(dt, count, box=bc.SWEPT_BOX, want_pairs=True)
    assert isinstance(boxes, nfopp.BoxTrackConflicts)
    assert boxes.pair_status.cpu().tolist() == [[0, 0], [0, 0]] and not bool(boxes.in_conflict.any()) and not bool(boxes.undecided.any())
    reach = float(np.hypot(0.4, 0.27))
    discs = timed.conflicts(dt, count, radius=reach, want_pairs=True)
    assert isinstance(discs, nfopp.TrackConflicts) and bool(discs.in_conflict.all()) and float(discs.pair_first[0, 1]) == 0.0
    # the keyword forms equal the direct call on the sampled states; the chord margin has its rotation term
    states = timed.sample(dt, count)
    chord = ((1.0 + 1.0) * dt / 2.0 + reach * 1.0 * dt / 2.0) + reach * 1.0 * dt / 2.0
    got = timed.conflicts(dt, count, box=bc.SWEPT_BOX, radius=0.03125, margin="chord", refine=2, want_pairs=True)
    want = nfopp.box_track_conflicts(states, dt=dt, box_a=bc.SWEPT_BOX, radius_a=0.03125, margin=chord, refine=2, want_pairs=True)
    assert all(_equal(getattr(got, name), getattr(want, name)) for name in OUTPUTS if name != "summary_b")
    assert bool(got.in_conflict.all())                                      # 0.75 - 0.54 < 0.0625 + 0.25 + 0.12
    with pytest.raises(ValueError, match="turn-rate"):
        nfopp.time_parametrize(_dev(paths[:, 1:-1]), _dev(paths[:, 0]), _dev(paths[:, -1]), nfopp.MotionLimits(1.0, 1.0)).conflicts(
            dt, count, box=bc.SWEPT_BOX, margin="chord")
    with pytest.raises(ValueError, match="give box"):
        timed.conflicts(dt, count, refine=2)
