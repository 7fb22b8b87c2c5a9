"""GPU: nfopp_fleet_shift_masks and nfopp_fleet_assign_delays (csrc/fleet_schedule.hip) against the numpy restatement
(tests/fleet_schedule_ref.py), bit for bit: pair and base masks, bad flags, delays, statuses and forbidden words, at the sizes
where the kernels take another path (one robot, tile edges of 8 x 8 pairs, 64 and 65 shifts -- one mask word and the word
boundary --, the full 127 bits, several chunks of instants, more robots than the assignment pass has threads); then the device's
own end-to-end check through nfopp.track_conflicts, the Python interface and the torch ops against the raw calls.

The restatement of the 67 x 65 x 63 case walks 67^2 x 127 x 97 intervals in numpy, which is most of that case's time; it is
computed once."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
from nfopp import _lib, torch_ops  # noqa: E402

import fleet_schedule_cases as fc  # noqa: E402
import fleet_schedule_ref as fr  # noqa: E402

F32 = np.float32
# obstacles and row strides rotate over the sizes; the largest case goes without obstacles (its restatement is the slow one)
OBSTACLES = (0, 1, 33, 0, 33, 0, 1)
STRIDES = (2, 3, 4, 3, 2, 4, 3)


def _dev(x, dtype=F32):
    return None if x is None else torch.tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _raw_masks(c):
    """The C entry on case `c` with preallocated, poisoned outputs -> (pair, base, bad) device tensors."""
    lib, L = _lib.load(), _lib
    t, o = _dev(c["tracks"]), _dev(c["obstacles"])
    radius, obstacle_radius = _dev(c["radius"]), _dev(c["obstacle_radius"])       # alive until the launch
    b, k, stride = t.shape
    m, so = (0, 2) if o is None else (o.shape[0], o.shape[2])
    pair = torch.full((b, b, 2), -7, dtype=torch.int64, device="cuda")
    base = torch.full((b,), -7, dtype=torch.int64, device="cuda")
    bad = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    nbytes = lib.nfopp_fleet_shift_masks_workspace_bytes(b, m)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    L.check(lib.nfopp_fleet_shift_masks(L.ptr(t), b, stride, k, L.ptr(radius), c["margin"], c["max_delay"], L.ptr(o), m, so,
                                        L.ptr(obstacle_radius), L.ptr(pair, torch.int64), L.ptr(base, torch.int64),
                                        L.ptr(bad, torch.int32), L.ptr(ws, torch.uint8), nbytes, L.stream_ptr()))
    return pair, base, bad


def _raw_assign(masks, max_delay, order=None, forbidden=True):
    lib, L = _lib.load(), _lib
    pair, base, bad = masks
    b = pair.shape[0]
    delay = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    forb = torch.full((b,), -7, dtype=torch.int64, device="cuda") if forbidden else None
    order = _dev(order, np.int32)
    L.check(lib.nfopp_fleet_assign_delays(L.ptr(pair, torch.int64), L.ptr(base, torch.int64), L.ptr(bad, torch.int32),
                                          L.ptr(order, torch.int32), b, max_delay, L.ptr(delay, torch.int32),
                                          L.ptr(status, torch.int32), L.ptr(forb, torch.int64), L.stream_ptr()))
    return delay, status, forb


def _check_masks(c, label):
    want = fr.shift_masks(c["tracks"], **fc.kwargs(c))
    got = _raw_masks(c)
    pair, base, bad = _u64(got[0]), _u64(got[1]), got[2].cpu().numpy()
    assert np.array_equal(bad, want["bad"]), (label, "bad", bad, want["bad"])
    assert np.array_equal(pair, want["pair"]), (label, "pair", np.argwhere(pair != want["pair"])[:6])
    assert np.array_equal(base, want["base"]), (label, "base", np.argwhere(base != want["base"])[:6])
    return got, want


def _check_assign(got_masks, want_masks, max_delay, order, label):
    want = fr.assign(want_masks, order)
    delay, status, forb = _raw_assign(got_masks, max_delay, order)
    assert np.array_equal(delay.cpu().numpy(), want["delay"]), (label, "delay", delay.tolist(), want["delay"].tolist())
    assert np.array_equal(status.cpu().numpy(), want["status"]), (label, "status")
    assert np.array_equal(_u64(forb), want["forbidden"]), (label, "forbidden")
    return (delay, status, forb), want


@pytest.mark.parametrize("n", range(len(fc.SIZES)), ids=["%dx%dx%d" % s for s in fc.SIZES])
def test_masks_and_delays_equal_the_restatement_bit_for_bit(n):
    b, k, md = fc.SIZES[n]
    c = fc.sized_case(b, k, md, m=OBSTACLES[n], stride=STRIDES[n])
    got, want = _check_masks(c, fc.SIZES[n])
    again = _raw_masks(c)                                            # the same bits on a second run
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    seen = set()
    for name, order in sorted(fc.orders(b, seed=n).items()):
        (delay, status, forb), ws = _check_assign(got, want, md, order, (fc.SIZES[n], name))
        seen |= set(ws["status"].tolist())
        d2, s2, _ = _raw_assign(got, md, order, forbidden=False)     # a null optional output; a second run
        assert torch.equal(d2, delay) and torch.equal(s2, status)
    if b >= 32:
        assert seen >= {0, fr.STATUS_BAD_TRACK, fr.STATUS_NOT_ORDERED} and want["bad"].sum() == 3
    if b >= 33:
        assert fr.STATUS_UNRESOLVED in seen
    if OBSTACLES[n] == 33:
        assert (want["base"] != 0).any()
    if md >= 32:
        assert (want["pair"][:, :, 1] != 0).any() and (want["pair"][:, :, 0] != 0).any()      # bits in both words


def test_several_chunks_of_instants():
    """K = 150: three trips of 64 instants; d0 of a trip's first interval is read again from the staged window."""
    c = fc.sized_case(11, 150, 9, m=3, stride=3)
    got, want = _check_masks(c, "chunks")
    assert want["pair"].any() and (want["base"] != 0).any()
    _check_assign(got, want, 9, None, "chunks")


@pytest.mark.parametrize("name", sorted(fc.hand_cases()))
def test_hand_cases(name):
    c = fc.hand_cases()[name]
    got, want = _check_masks(c, name)
    (delay, status, forb), _ = _check_assign(got, want, c["max_delay"], c["order"], name)
    e = c["expect"]
    assert delay.tolist() == e["delay"] and status.tolist() == e["status"] and [int(x) for x in _u64(forb)] == e["forbidden"]
    if "base" in e:
        assert [int(x) for x in _u64(got[1])] == e["base"]


def test_lanes_at_exactly_r_and_one_fp32_step_closer():
    pair, _, _ = _raw_masks(fc.lanes(False))
    assert not pair.any()
    pair, _, _ = _raw_masks(fc.lanes(True))
    p = _u64(pair)
    assert [int(x) for x in p[0, 1]] == [2 ** 64 - 1, 2 ** 63 - 1] == [int(x) for x in p[1, 0]] and not p[0, 0].any() and not p[1, 1].any()
    _check_masks(fc.lanes(True), "lanes")


def test_the_schedule_is_clear_by_the_conflict_check_and_orders_reuse_the_masks():
    c = fc.crossing_obstacles(fc.circle(16, 18, 31), 5, seed=2)
    tracks, obstacles = _dev(c["tracks"]), _dev(c["obstacles"])
    masks = nfopp.fleet_shift_masks(tracks, max_delay=31, radius=_dev(c["radius"]), margin=c["margin"], obstacles=obstacles,
                                    obstacle_radius=_dev(c["obstacle_radius"]))
    raw = _raw_masks(c)
    assert isinstance(masks, nfopp.FleetMasks) and all(torch.equal(x, y) for x, y in zip((masks.pair, masks.base, masks.bad), raw))
    want_m = fr.shift_masks(c["tracks"], **fc.kwargs(c))
    perm = fc.orders(16)["permutation"]
    first, second = masks.assign(), masks.assign(torch.tensor(perm, device="cuda"))
    for sched, order in ((first, None), (second, perm)):
        want = fr.assign(want_m, order)
        assert isinstance(sched, nfopp.FleetSchedule) and np.array_equal(sched.delay.cpu().numpy(), want["delay"])
        assert np.array_equal(sched.status.cpu().numpy(), want["status"]) and np.array_equal(_u64(sched.forbidden), want["forbidden"])
        assert torch.equal(sched.scheduled, sched.status == 0) and sched.max_delay == 31
        # the device's own end-to-end check: the delayed tracks through the conflict kernel
        on = sched.scheduled
        assert on.sum() >= 8 and (sched.delay[on] > 0).any()
        moved = nfopp.delay_tracks(tracks, sched.delay, 18 + 31)
        fleet = nfopp.track_conflicts(moved[on], dt=1.0, radius_a=_dev(c["radius"])[on], margin=c["margin"])
        assert not fleet.in_conflict.any()
        floor = nfopp.track_conflicts(moved[on], obstacles, dt=1.0, radius_a=_dev(c["radius"])[on], radius_b=_dev(c["obstacle_radius"]),
                                      margin=c["margin"])
        assert not floor.in_conflict.any()
    assert not torch.equal(first.delay, second.delay)
    both = nfopp.schedule_delays(tracks, max_delay=31, radius=_dev(c["radius"]), margin=c["margin"], obstacles=obstacles,
                                 obstacle_radius=_dev(c["obstacle_radius"]), order=perm)
    assert torch.equal(both.delay, second.delay) and torch.equal(both.status, second.status)
    lean = masks.assign(want_forbidden=False)
    assert lean.forbidden is None and torch.equal(lean.delay, first.delay)
    # a number for a radius, and a view of the x, y columns of wider rows
    wide = _dev(fc.with_stride(c, 4, seed=5)["tracks"])
    one = nfopp.fleet_shift_masks(wide[:, :, :2], max_delay=31, radius=0.0625, margin=c["margin"])
    want = fr.shift_masks(c["tracks"], 31, radius=0.0625, margin=c["margin"])
    assert np.array_equal(_u64(one.pair), want["pair"]) and not one.base.any()


def one_predicate_case(b, k):
    """B straight drives across a square floor that take all K instants, radii and floor sized so that some pairs conflict
    and some do not, and (B > 1) a NaN coordinate in track B // 2 -> (tracks [B, K, 2], radius [B], margin)."""
    rng = np.random.default_rng(100 * b + k)
    ends = rng.uniform(0.0, 0.5 * np.sqrt(b), (2, b, 1, 2))
    lam = (np.arange(k) / max(k - 1, 1))[None, :, None]
    tracks = (ends[0] * (1 - lam) + ends[1] * lam).astype(F32)
    if b > 1:
        tracks[b // 2, k // 2, 1] = np.nan
    return tracks, rng.uniform(0.05, 0.2, b).astype(F32), 0.03125


# (1, 1): one pair; (9, 5): two 8-tiles of the scheduler; (33, 5): across a 32-tile of the conflict kernel; (9, 70) with
# max_delay 3: K + max_delay across the 64-instant chunk of one kernel and the 32-instant chunk of the other
@pytest.mark.parametrize("b,k,md", ((1, 1, 0), (9, 5, 2), (33, 5, 2), (9, 70, 3)), ids=lambda v: str(v))
def test_one_predicate_on_the_device(b, k, md):
    """Bit max_delay (r = 0) of every pair mask is `pair_first < inf` of the conflict check in self mode: device against
    device over the whole matrix, the diagonal and the bad track's row and column included (there pair_first is +inf or NaN
    and the mask is 0).  Both kernels take the predicate from csrc/track_pairs.h."""
    tracks, radius, margin = one_predicate_case(b, k)
    t, r = _dev(tracks), _dev(radius)
    masks = nfopp.fleet_shift_masks(t, max_delay=md, radius=r, margin=margin)
    found = nfopp.track_conflicts(t, dt=1.0, radius_a=r, margin=margin, want_pairs=True)
    bit = ((masks.pair[:, :, md // 64] >> (md % 64)) & 1).bool()
    want = found.pair_first < float("inf")
    assert torch.equal(bit, want), torch.nonzero(bit != want)[:6].tolist()
    bad = masks.bad.bool()
    assert bad.tolist() == [b > 1 and i == b // 2 for i in range(b)]
    assert torch.isnan(found.pair_first[bad]).all() and torch.isnan(found.pair_first[:, bad]).all()
    assert not masks.pair[bad].any() and not masks.pair[:, bad].any() and not masks.pair.diagonal().any()
    if b > 1:
        good = ~(bad[:, None] | bad[None, :] | torch.eye(b, dtype=torch.bool, device="cuda"))
        assert want[good].any() and (~want)[good].any()
    if k > 64:      # a first contact in the last chunk of instants of either kernel
        assert (found.pair_first[want] > 64.0).any()


def test_the_torch_ops_equal_the_raw_calls():
    ops = torch_ops.load()
    for c in (fc.sized_case(9, 7, 5, m=3, stride=3), fc.sized_case(10, 6, 40, m=0, stride=2)):
        raw = _raw_masks(c)
        o = ops.fleet_shift_masks(_dev(c["tracks"]), c["max_delay"], _dev(c["radius"]), c["margin"], _dev(c["obstacles"]),
                                  _dev(c["obstacle_radius"]))
        assert all(torch.equal(x, y) for x, y in zip(o, raw))
        order = fc.orders(len(c["tracks"]))["odd"]
        want = _raw_assign(raw, c["max_delay"], order)
        got = ops.fleet_assign_delays(o[0], o[1], o[2], _dev(order, np.int32), c["max_delay"])
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        got = ops.fleet_assign_delays(o[0], o[1], o[2], None, c["max_delay"])
        assert all(torch.equal(x, y) for x, y in zip(got, _raw_assign(raw, c["max_delay"])))
    with pytest.raises(RuntimeError, match="K \\+ max_delay"):
        ops.fleet_shift_masks(_dev(c["tracks"]), 5, None, 0.0, _dev(c["tracks"]), None)
    with pytest.raises(RuntimeError, match="max_delay"):
        ops.fleet_shift_masks(_dev(c["tracks"]), 64, None, 0.0, None, None)
    empty = ops.fleet_shift_masks(_dev(c["tracks"][:0]), 5, None, 0.0, None, None)
    assert empty[0].shape == (0, 0, 2) and ops.fleet_assign_delays(*empty, None, 5)[0].shape == (0,)


def _planner(b, n, seed=3):
    z = load_golden("g1_onf.npz")
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    rng = np.random.default_rng(seed)
    starts = np.concatenate([rng.uniform(0.2, 0.8, (b, 2)), rng.uniform(-3, 3, (b, 1))], 1).astype(F32)
    goals = np.concatenate([rng.uniform(2.2, 2.8, (b, 2)), rng.uniform(-3, 3, (b, 1))], 1).astype(F32)
    bp = nfopp.BatchPlanner(onf, b, n, nfopp.TrajectoryHyper(collision_weight=3, direction_delta_weight=7, collision_beta=2))
    bp.init(starts, goals, (-0.1, 3.1, -0.1, 3.1))
    bp.step(n=3)
    return bp


def test_timed_paths_and_fleet_schedule_equal_the_raw_calls():
    bp = _planner(6, 24)
    lim = nfopp.MotionLimits(1.0, 0.5)
    dt, count, md = 0.125, 48, 20
    timed = bp.timed_paths(lim)
    states = timed.sample(dt, count)
    radius = torch.linspace(0.05, 0.15, 6, device="cuda")
    chord = (lim.v_max + lim.v_max) * dt / 2.0
    order = torch.argsort(timed.summary[:, nfopp.TIME_SUMMARY_TIME], descending=True, stable=True)
    want = nfopp.schedule_delays(states, max_delay=md, radius=radius, margin=chord, order=order)
    got = timed.schedule(dt, count, md, radius, order="longest_first")
    assert torch.equal(got.delay, want.delay) and torch.equal(got.status, want.status) and torch.equal(got.forbidden, want.forbidden)
    host_m, host = fr.schedule(states.cpu().numpy(), md, radius=radius.cpu().numpy(), margin=chord, order=order.cpu().numpy())
    assert np.array_equal(got.delay.cpu().numpy(), host["delay"]) and np.array_equal(_u64(got.forbidden), host["forbidden"])
    sec = got.delay_seconds.cpu().numpy()
    assert got.delay_seconds.dtype == torch.float64 and np.array_equal(np.isnan(sec), host["delay"] < 0)
    assert np.array_equal(sec[host["delay"] >= 0], host["delay"][host["delay"] >= 0] * dt)
    assert torch.equal(got.complete, timed.summary[:, nfopp.TIME_SUMMARY_TIME] <= (count - 1) * dt) and got.complete.dtype == torch.bool
    fleet = bp.fleet_schedule(lim, dt, count, radius, md, order="longest_first")
    assert torch.equal(fleet.delay, got.delay) and torch.equal(fleet.status, got.status)
    # predicted obstacle tracks, count + max_delay instants; one chord margin from the larger top speed
    obstacles = nfopp.constant_velocity_tracks(torch.tensor([[0.5, 2.5], [2.5, 0.5], [1.5, 1.5]], device="cuda"),
                                               torch.tensor([[0.4, -0.4], [-0.3, 0.3], [0.0, 0.0]], device="cuda"), dt, count + md)
    margin = (lim.v_max + 1.25) * dt / 2.0
    want = nfopp.schedule_delays(states, max_delay=md, radius=radius, margin=margin, obstacles=obstacles, obstacle_radius=0.2)
    got = timed.schedule(dt, count, md, radius, other=obstacles, other_radius=0.2, other_v_max=1.25)
    assert torch.equal(got.delay, want.delay) and torch.equal(got.forbidden, want.forbidden)
    fleet = bp.fleet_schedule(lim, dt, count, radius, md, obstacles=obstacles, obstacle_radius=0.2, obstacle_v_max=1.25)
    assert torch.equal(fleet.delay, want.delay) and torch.equal(fleet.status, want.status)
    with pytest.raises(ValueError, match="other_v_max"):
        bp.fleet_schedule(lim, dt, count, radius, md, obstacles=obstacles)
    # another TimedPaths as the obstacles, sampled at count + max_delay instants on the same grid
    other = nfopp.time_parametrize(timed.traj.flip(0), timed.start.flip(0), timed.goal.flip(0), nfopp.MotionLimits(0.5, 0.5))
    got = timed.schedule(dt, count, md, 0.1, other=other, other_radius=0.1)
    want = nfopp.schedule_delays(states, max_delay=md, radius=0.1, margin=(1.0 + 1.0) * dt / 2.0, obstacles=other.sample(dt, count + md),
                                 obstacle_radius=0.1)
    assert torch.equal(got.delay, want.delay) and torch.equal(got.status, want.status)


def test_head_on_at_a_junction_through_the_time_parametrisation():
    """Two L-shaped paths that meet head-on at a junction under MotionLimits(v_max=1, a_max=1): timed, sampled, scheduled --
    the device against the restatement run on the sampled states; robot 1 waits, and the delayed fleet is clear."""
    n = 15
    a = np.concatenate([np.stack([np.linspace(0, 4, 9), np.zeros(9)], -1), np.stack([np.full(8, 4.0), np.linspace(0.5, 4, 8)], -1)])
    b = np.concatenate([np.stack([np.linspace(8, 4, 9), np.zeros(9)], -1), np.stack([np.full(8, 4.0), -np.linspace(0.5, 4, 8)], -1)])
    paths = np.stack([a, b]).astype(F32)
    assert paths.shape == (2, n + 2, 2)
    lim = nfopp.MotionLimits(1.0, 1.0, cusp_angle=None)
    timed = nfopp.time_parametrize(_dev(paths[:, 1:-1]), _dev(paths[:, 0]), _dev(paths[:, -1]), lim)
    dt, md = 0.25, 24
    count = int(np.ceil(float(timed.summary[:, nfopp.TIME_SUMMARY_TIME].max()) / dt)) + 2
    got = timed.schedule(dt, count, md, 0.5, margin=0.0)
    assert got.complete.all()
    states = timed.sample(dt, count)
    _, want = fr.schedule(states.cpu().numpy(), md, radius=0.5)
    assert np.array_equal(got.delay.cpu().numpy(), want["delay"]) and np.array_equal(_u64(got.forbidden), want["forbidden"])
    delay = got.delay.tolist()
    assert delay[0] == 0 and 0 < delay[1] <= md and got.status.tolist() == [0, 0]
    assert abs(float(got.delay_seconds[1]) - delay[1] * dt) == 0.0
    before = nfopp.track_conflicts(states, dt=dt, radius_a=0.5)
    after = nfopp.track_conflicts(nfopp.delay_tracks(states, got.delay, count + md), dt=dt, radius_a=0.5)
    assert before.in_conflict.all() and not after.in_conflict.any()
