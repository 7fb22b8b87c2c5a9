"""GPU: nfopp_fleet_box_shift_masks (csrc/fleet_box_schedule.hip) against the numpy restatement
(tests/fleet_box_schedule_ref.py) run on the device's own unit vectors, bit for bit: pair and base masks and bad flags at the
sizes where the kernel takes another path (one robot, one pair, tile edges at 8 and 32, 65 bits -- the word boundary --, the full
127 bits, K = 1 and 2, and 9 and 17 on either side of the 16-instant chunk), refine 0, 1 and 3, row strides 3 and 5, with and
without obstacles, with bad robots and bad obstacles; outputs inside guard bytes pre-filled with 0x00 and 0xFF; the same bits
run after run; delays and statuses of the unchanged assignment pass; the schedule FREE by the box check on the delayed tracks;
the hand cases through the Python interface; `TimedPaths.schedule_boxes` and `BatchPlanner.fleet_schedule(box=)` against
`schedule_box_delays`; `fleet_schedule(box=, replan=)` to completion, with the radii that reach the space-time search; and the
disc path as before.

The restatement of every size is computed once (a module fixture) and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
from nfopp import _lib  # noqa: E402

import box_conflict_ref as br  # noqa: E402
import fleet_box_schedule_cases as xc  # noqa: E402
import fleet_box_schedule_ref as xr  # noqa: E402
import fleet_schedule_cases as fc  # noqa: E402
import fleet_schedule_ref as fr  # noqa: E402
import guarded  # noqa: E402

F32 = np.float32
IDS = ["%dx%dx%d" % s for s in xc.SIZES]


def _dev(x, dtype=F32):
    return None if x is None else torch.tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _headings(t):
    b, k, s = t.shape
    out = torch.full((b, k, 2), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().nfopp_track_headings(_lib.ptr(t), b, s, k, _lib.ptr(out, torch.float64), _lib.stream_ptr()))
    return out


def _raw_masks(c, refine, fill=0x00):
    """The C entry on case `c`, outputs inside guard bytes filled with `fill` -> ((pair, base, bad) device tensors, their parent
    allocations, the case with the device's unit vectors in place of numpy's)."""
    lib, L = _lib.load(), _lib
    t, o = _dev(c["tracks"]), _dev(c["obstacles"])
    b, k, stride = t.shape
    m, so = (0, 3) if o is None else (o.shape[0], o.shape[2])
    u, uo = _headings(t), None if o is None else _headings(o)
    box, radius = _dev(c["box"]), _dev(c["radius"])
    obox, oradius = _dev(c["obstacle_box"]), _dev(c["obstacle_radius"])
    pair, p_pair = guarded.guarded((b, b, 2), torch.int64, "cuda", fill)
    base, p_base = guarded.guarded((b,), torch.int64, "cuda", fill)
    bad, p_bad = guarded.guarded((b,), torch.int32, "cuda", fill)
    nbytes = lib.nfopp_fleet_box_shift_masks_workspace_bytes(b, m, k, c["max_delay"])
    ws, p_ws = guarded.guarded((nbytes,), torch.uint8, "cuda", fill)
    L.check(lib.nfopp_fleet_box_shift_masks(
        L.ptr(t), L.ptr(u, torch.float64), b, stride, k, L.ptr(box), L.ptr(radius), c["margin"], refine, c["max_delay"], L.ptr(o),
        L.ptr(uo, torch.float64), m, so, L.ptr(obox), L.ptr(oradius), L.ptr(pair, torch.int64), L.ptr(base, torch.int64),
        L.ptr(bad, torch.int32), L.ptr(ws, torch.uint8), nbytes, L.stream_ptr()))
    torch.cuda.synchronize()
    on_device = dict(c, units=u.cpu().numpy(), obstacle_units=None if uo is None else uo.cpu().numpy())
    return (pair, base, bad), (p_pair, p_base, p_bad, p_ws), on_device


@pytest.fixture(scope="module")
def device_runs():
    """Per size: the device's masks and the restatement on the device's unit vectors, computed once."""
    out = []
    for n in range(len(xc.SIZES)):
        c = xc.sized_case(n)
        got, parents, on_device = _raw_masks(c, xc.REFINES[n])
        want = xr.shift_masks(on_device["tracks"], on_device["units"], c["max_delay"], **xc.kwargs(on_device, xc.REFINES[n]))
        out.append((c, got, parents, on_device, want))
    return out


@pytest.mark.parametrize("n", range(len(xc.SIZES)), ids=IDS)
def test_masks_equal_the_restatement_bit_for_bit_inside_their_guards(device_runs, n):
    c, got, parents, on_device, want = device_runs[n]
    pair, base, bad = _u64(got[0]), _u64(got[1]), got[2].cpu().numpy()
    assert np.array_equal(bad, want["bad"]), (xc.SIZES[n], "bad", bad, want["bad"])
    assert np.array_equal(pair, want["pair"]), (xc.SIZES[n], "pair", np.argwhere(pair != want["pair"])[:6])
    assert np.array_equal(base, want["base"]), (xc.SIZES[n], "base", np.argwhere(base != want["base"])[:6])
    assert all(guarded.guards_intact(p) for p in parents), xc.SIZES[n]
    # the other fill: nothing is read before it is written, every output element is written, the same bits on a second run
    again, parents2, _ = _raw_masks(c, xc.REFINES[n], fill=0xFF)
    assert all(torch.equal(x, y) for x, y in zip(got, again)) and all(guarded.guards_intact(p) for p in parents2)
    if (want["bad"] == 0).sum() >= 2:
        assert 0.1 <= xc.density(want) <= 0.9, xc.density(want)
    if c["max_delay"] >= 32:
        assert (want["pair"][:, :, 1] != 0).any() and (want["pair"][:, :, 0] != 0).any()      # bits in both words


@pytest.mark.parametrize("n", range(len(xc.SIZES)), ids=IDS)
def test_the_assignment_pass_gives_the_restatements_delays_and_statuses(device_runs, n):
    c, got, _, _, want = device_runs[n]
    b = len(c["tracks"])
    masks = nfopp.FleetMasks(got[0], got[1], got[2], c["max_delay"])
    for name, order in sorted(fc.orders(b, seed=n).items()):
        w = xr.assign(want, order)
        s = masks.assign(None if order is None else torch.tensor(order, device="cuda"))
        assert np.array_equal(s.delay.cpu().numpy(), w["delay"]), (xc.SIZES[n], name)
        assert np.array_equal(s.status.cpu().numpy(), w["status"]) and np.array_equal(_u64(s.forbidden), w["forbidden"]), (xc.SIZES[n], name)


@pytest.mark.parametrize("n", (5, 6), ids=[IDS[n] for n in (5, 6)])      # the sizes whose schedule places ten robots and more
def test_the_schedule_is_free_by_the_box_check(n):
    """By construction: box_track_conflicts on the delayed tracks, the same box, radius, margin and refine, reports FREE for
    every pair of scheduled robots and against every good obstacle.  Through the Python interface, which must equal the raw
    call."""
    c = xc.sized_case(n)
    refine, md = xc.REFINES[n], c["max_delay"]
    t, o = _dev(c["tracks"]), _dev(c["obstacles"])
    box, radius = _dev(c["box"]), _dev(c["radius"])
    masks = nfopp.fleet_box_shift_masks(t, max_delay=md, box=box, radius=radius, margin=c["margin"], refine=refine, obstacles=o,
                                        obstacle_box=_dev(c["obstacle_box"]), obstacle_radius=_dev(c["obstacle_radius"]))
    raw, _, _ = _raw_masks(c, refine)
    assert all(torch.equal(x, y) for x, y in zip((masks.pair, masks.base, masks.bad), raw))
    assert masks.refine == refine and torch.equal(masks.box, box)
    sched = masks.assign()
    both = nfopp.schedule_box_delays(t, max_delay=md, box=box, radius=radius, margin=c["margin"], refine=refine, obstacles=o,
                                     obstacle_box=_dev(c["obstacle_box"]), obstacle_radius=_dev(c["obstacle_radius"]))
    assert torch.equal(both.delay, sched.delay) and torch.equal(both.status, sched.status)
    on = sched.scheduled
    assert on.sum() >= 2
    moved = nfopp.delay_tracks(t, sched.delay, t.shape[1] + md)
    fleet = nfopp.box_track_conflicts(moved[on], dt=1.0, box_a=box[on], radius_a=radius[on], margin=c["margin"], refine=refine,
                                      want_pairs=True)
    off = ~torch.eye(int(on.sum()), dtype=torch.bool, device="cuda")
    assert (fleet.pair_status[off] == nfopp.BoxTrackConflicts.FREE).all()
    if o is not None:
        floor = nfopp.box_track_conflicts(moved[on], o, dt=1.0, box_a=box[on], box_b=_dev(c["obstacle_box"]), radius_a=radius[on],
                                          radius_b=_dev(c["obstacle_radius"]), margin=c["margin"], refine=refine, want_pairs=True)
        st = floor.pair_status
        assert ((st == nfopp.BoxTrackConflicts.FREE) | (st == nfopp.BoxTrackConflicts.BAD)).all()
        assert (st == nfopp.BoxTrackConflicts.FREE).any()


@pytest.mark.parametrize("name", sorted(xc.hand_cases()))
def test_hand_cases_through_the_python_interface(name):
    c = xc.hand_cases()[name]
    e = c["expect"]
    t = _dev(c["tracks"])
    md = c["max_delay"]
    for refine, (want_bits, delay, status) in sorted(e["refines"].items()):
        masks = nfopp.fleet_box_shift_masks(t, max_delay=md, box=xc.CAR, refine=refine)
        got = fr.unpack(_u64(masks.pair), 2 * md + 1)
        assert "".join("1" if x else "0" for x in got[0, 1]) == want_bits, (name, refine)
        assert "".join("1" if x else "0" for x in got[1, 0]) == want_bits[::-1] and not got[0, 0].any() and not got[1, 1].any()
        s = nfopp.schedule_box_delays(t, max_delay=md, box=xc.CAR, refine=refine)
        assert s.delay.tolist() == delay and s.status.tolist() == status, (name, refine)
    disc = nfopp.schedule_delays(t, max_delay=md, radius=xc.DISC)
    assert disc.delay.tolist() == e["disc"][1] and disc.status.tolist() == e["disc"][2]


def test_the_disc_path_returns_the_same_bits_as_before():
    """`fleet_shift_masks` on the disc scheduler's own case: the restatement's bits, with box None and refine 0."""
    c = fc.sized_case(9, 17, 31, m=9, stride=3)
    masks = nfopp.fleet_shift_masks(_dev(c["tracks"]), max_delay=31, radius=_dev(c["radius"]), margin=c["margin"],
                                    obstacles=_dev(c["obstacles"]), obstacle_radius=_dev(c["obstacle_radius"]))
    want = fr.shift_masks(c["tracks"], **fc.kwargs(c))
    assert masks.box is None and masks.refine == 0
    assert np.array_equal(_u64(masks.pair), want["pair"]) and np.array_equal(_u64(masks.base), want["base"])
    assert np.array_equal(masks.bad.cpu().numpy(), want["bad"]) and want["pair"].any() and (want["base"] != 0).any()


def test_timed_paths_and_fleet_schedule_with_boxes_equal_schedule_box_delays():
    """`TimedPaths.schedule_boxes` and `BatchPlanner.fleet_schedule(box=)` are `schedule_box_delays` on the sampled states with
    the box chord margin of `TimedPaths.conflicts(box=)`; without `box` the call is the disc schedule, as before.  (The six
    paths of this planner end within 0.6 m of each other, so few of them can be placed: that a placed fleet is FREE is
    `test_the_schedule_is_free_by_the_box_check`'s.)"""
    from conftest import load_golden
    z = load_golden("g1_onf.npz")
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    rng = np.random.default_rng(3)
    b, n = 6, 24
    starts = np.concatenate([rng.uniform(0.2, 0.8, (b, 2)), rng.uniform(-3, 3, (b, 1))], 1).astype(F32)
    goals = np.concatenate([rng.uniform(2.2, 2.8, (b, 2)), rng.uniform(-3, 3, (b, 1))], 1).astype(F32)
    bp = nfopp.BatchPlanner(onf, b, n, nfopp.TrajectoryHyper(collision_weight=3, direction_delta_weight=7, collision_beta=2))
    bp.init(starts, goals, (-0.1, 3.1, -0.1, 3.1))
    bp.step(n=3)
    lim = nfopp.MotionLimits(1.0, 0.5, w_max=2.0)
    dt, count, md, box, r = 0.125, 48, 20, (-0.17, 0.2, -0.135, 0.135), 0.02
    timed = bp.timed_paths(lim)
    states = timed.sample(dt, count)
    reach = nfopp.conflicts.box_reach(box)
    turn = reach * lim.w_max * dt / 2.0      # per side, added one after the other as `TimedPaths.conflicts(box=)` does
    chord = nfopp.conflicts.chord_margin(lim.v_max, lim.v_max, dt) + turn + turn
    assert abs(chord - nfopp.conflicts.box_chord_margin(lim.v_max, lim.v_max, dt, reach, lim.w_max, reach, lim.w_max)) < 1e-15
    want = nfopp.schedule_box_delays(states, max_delay=md, box=box, radius=r, margin=chord, refine=2)
    got = timed.schedule_boxes(dt, count, md, box, radius=r, refine=2)
    assert torch.equal(got.delay, want.delay) and torch.equal(got.status, want.status) and torch.equal(got.forbidden, want.forbidden)
    assert got.delay_seconds.dtype == torch.float64 and got.complete.dtype == torch.bool and got.margin == chord
    fleet = bp.fleet_schedule(lim, dt, count, r, md, box=box, refine=2)
    assert torch.equal(fleet.delay, want.delay) and torch.equal(fleet.status, want.status)
    # obstacles as a tracks tensor with theta: one margin for robot pairs and obstacle pairs, the larger of the two
    other = torch.zeros(2, count + md, 3, device="cuda")
    other[0, :, :2] = torch.tensor([1.5, 1.5], device="cuda")
    other[1, :, 0] = torch.linspace(0.0, 3.0, count + md, device="cuda")
    other[1, :, 1] = 2.9
    big = (-0.3, 0.3, -0.2, 0.2)
    reach_o = nfopp.conflicts.box_reach(big)
    both = nfopp.conflicts.chord_margin(lim.v_max, max(lim.v_max, 0.5), dt) + reach * lim.w_max * dt / 2.0 + \
        max(reach * lim.w_max, reach_o * 0.25) * dt / 2.0
    want = nfopp.schedule_box_delays(states, max_delay=md, box=box, radius=r, margin=both, refine=1, obstacles=other, obstacle_box=big,
                                     obstacle_radius=0.05)
    got = bp.fleet_schedule(lim, dt, count, r, md, obstacles=other, obstacle_radius=0.05, obstacle_v_max=0.5, box=box, refine=1,
                            obstacle_box=big, obstacle_w_max=0.25)
    assert torch.equal(got.delay, want.delay) and torch.equal(got.status, want.status) and got.margin == both
    with pytest.raises(ValueError, match="replan_radius"):
        bp.fleet_schedule(lim, dt, count, r, md, box=box, replan=object())
    with pytest.raises(ValueError, match="give box"):
        bp.fleet_schedule(lim, dt, count, r, md, refine=2)
    plain = bp.fleet_schedule(lim, dt, count, 0.1, md)
    disc = nfopp.schedule_delays(states, max_delay=md, radius=0.1, margin=nfopp.conflicts.chord_margin(lim.v_max, lim.v_max, dt))
    assert torch.equal(plain.delay, disc.delay) and torch.equal(plain.status, disc.status)


@pytest.mark.parametrize("with_obstacles", (False, True), ids=("fleet_alone", "with_obstacles"))
def test_fleet_schedule_with_boxes_replans_against_discs_that_cover_the_boxes(monkeypatch, with_obstacles):
    """`fleet_schedule(box=, replan=grid, replan_radius=)` to completion.  The space-time search reserves discs: every robot
    goes in with `replan_radius`, every obstacle with the disc that covers its box at every heading -- the farthest corner
    (times 1.000001, as the box check's reach) plus its rounding radius -- and never with the rounding radius alone.  The radii
    are read where they reach `spacetime_plan`; what comes back is free of conflicts by `track_conflicts` at those radii."""
    from conftest import load_golden
    import nfopp.spacetime as spacetime
    z = load_golden("g1_onf.npz")
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    rng = np.random.default_rng(3)
    b, n = 6, 24
    starts = np.concatenate([rng.uniform(0.2, 0.8, (b, 2)), rng.uniform(-3, 3, (b, 1))], 1).astype(F32)
    goals = np.concatenate([rng.uniform(2.2, 2.8, (b, 2)), rng.uniform(-3, 3, (b, 1))], 1).astype(F32)
    bp = nfopp.BatchPlanner(onf, b, n, nfopp.TrajectoryHyper(collision_weight=3, direction_delta_weight=7, collision_beta=2))
    bp.init(starts, goals, (-0.1, 3.1, -0.1, 3.1))
    bp.step(n=3)
    lim = nfopp.MotionLimits(1.0, 0.5, w_max=2.0)
    dt, count, md, box, r, disc = 0.125, 48, 2, (-0.085, 0.1, -0.0675, 0.0675), 0.01, 0.125
    grid = nfopp.OccupancyGrid(np.zeros((32, 32), np.uint8), (-0.1, 3.1, -0.1, 3.1), 0.1, device="cuda")
    kw, m = {}, 0
    if with_obstacles:
        m = 2
        other = torch.zeros(m, count + md, 3, device="cuda")
        other[0, :, 0], other[0, :, 1] = 1.5, 0.3
        other[1, :, 0] = torch.linspace(0.2, 2.9, count + md, device="cuda")
        other[1, :, 1] = 2.95
        big = np.array([(-0.3, 0.3, -0.2, 0.2), (-0.1, 0.2, -0.05, 0.05)], F32)
        kw = dict(obstacles=other, obstacle_radius=torch.tensor([0.05, 0.0], device="cuda"), obstacle_v_max=0.5, obstacle_box=big,
                  obstacle_w_max=0.25)
    seen = []
    real = spacetime.spacetime_plan

    def recording(*args, **kwargs):
        seen.append(kwargs)
        return real(*args, **kwargs)
    monkeypatch.setattr(spacetime, "spacetime_plan", recording)
    plain = bp.fleet_schedule(lim, dt, count, r, md, box=box, refine=1, **kw)
    got = bp.fleet_schedule(lim, dt, count, r, md, box=box, refine=1, replan=grid, replan_radius=disc, **kw)
    assert not hasattr(plain, "plan") and len(seen) == 1
    assert torch.equal(got.delay, plain.delay) and torch.equal(got.status, plain.status)
    assert (got.status == nfopp.SCHEDULE_UNRESOLVED).any()
    sent = seen[0]
    assert sent["robot_radius"] == disc
    want_radius = [float(F32(disc))] * b
    if with_obstacles:
        reach = np.hypot(np.abs(big[:, :2]).max(1), np.abs(big[:, 2:]).max(1)).astype(F32) * F32(1.000001)
        cover = reach + np.array([0.05, 0.0], F32)
        assert (cover >= np.hypot(0.3, 0.2) + 0.05 - 1e-6)[0] and cover[1] >= np.hypot(0.2, 0.05) - 1e-6      # never the rounding radius alone
        want_radius += cover.tolist()
        assert np.allclose(got.obstacle_radius.cpu().numpy(), cover, rtol=0, atol=1e-7)
    assert sent["track_radius"].shape == (b + m,) and np.allclose(sent["track_radius"].cpu().numpy(), want_radius, rtol=0, atol=1e-7)
    assert sent["tracks"].shape == (b + m, count + md, 2) and sent["visible"].shape == (b + m,)
    assert sent["visible"][b:].all() and torch.equal(sent["visible"][:b], got.scheduled)
    assert got.merged.shape == (b, count + md, 2)
    assert torch.equal(got.plan.status != nfopp.SPACETIME_NOT_ORDERED, got.status == nfopp.SCHEDULE_UNRESOLVED)
    on = ~torch.isnan(got.merged[:, 0, 0])
    assert torch.equal(on, got.scheduled | got.plan.planned)
    # what was planned is clear of everything it was planned against, by the disc check at the radii that were reserved
    snap = got.margin + grid.resolution / np.sqrt(2.0)
    planned = got.plan.planned
    if with_obstacles:
        floor = nfopp.track_conflicts(got.merged[planned], other[:, :, :2].contiguous(), dt=dt, radius_a=disc,
                                      radius_b=got.obstacle_radius, margin=snap)
        assert not floor.in_conflict.any()
    if on.sum() >= 2 and planned.any():
        fleet = nfopp.track_conflicts(got.merged[on], dt=dt, radius_a=disc, margin=snap, want_pairs=True)
        rows = planned[on]
        assert not (fleet.pair_first[rows] < float("inf")).any()
