"""GPU: nfopp_spacetime_reservation_init, nfopp_spacetime_reserve and nfopp_spacetime_plan_fleet (csrc/spacetime_search.hip)
against the numpy restatement (tests/spacetime_ref.py), bit for bit: the blocked and last bitmaps, cells, arrivals, statuses and
tracks (NaN rows as bits), at the sizes where the kernels take another path (one cell, a row of 63 / 64 / 65 cells -- one word
and the word boundary --, three words a row, more movers than the reserve kernel stages per trip); at the sizes past one trip
of the plan kernels' strided loops (spacetime_cases.EDGES: more than 1024 words, with one and with two words a row; more than
1024 instants on either side of the trip boundary; more robots x instants than the init kernel has threads) and at the largest
frontier one workgroup's LDS holds; then the device's own end-to-end check through nfopp.track_conflicts and the Python
interface.  The 40 x 130 case has more cells than the search kernel has threads but only 120 words, which is what its loops
run over: it never took them past one trip.

Measured on an MI355X: the whole file takes 8.4 s; about 4 s of it are the numpy restatement of the movers of the 40 x 130 x 33
case, which is computed once and shared, never written to.  The eight EDGES cases and the refusal take 0.6 s together, none
more than 0.2 s."""
import functools

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
import spacetime_cases as sc  # noqa: E402
import spacetime_ref as sr  # noqa: E402

F32 = np.float32


def _dev(x, dtype=F32):
    return None if x is None else torch.tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)



def _geometry(c):
    g = c["geo"]
    return g.rows, g.cols, c["T"], g.b0, g.b2, g.res, c["robot_radius"], c["margin"]


def _raw_init(c):
    """The C entry on case `c` -> the reservation words [n] int64 (poisoned first)."""
    lib, L = _lib.load(), _lib
    g = c["geo"]
    nbytes = lib.nfopp_spacetime_reservation_bytes(g.rows, g.cols, c["T"])
    assert nbytes == ((c["T"] - 1) * 9 + 1) * g.rows * g.words * 8
    words = torch.full((nbytes // 8,), -7, dtype=torch.int64, device="cuda")
    occ = _dev(c["occ"], np.uint8)
    L.check(lib.nfopp_spacetime_reservation_init(L.ptr(occ, torch.uint8), g.rows, g.cols, c["T"], L.ptr(words, torch.int64), nbytes,
                                                 L.stream_ptr()))
    return words


def _raw_reserve(c, words, lo=0, hi=None):
    """ORs the movers lo .. hi of case `c` into `words`."""
    if c["tracks"] is None:
        return words
    lib, L = _lib.load(), _lib
    t = _dev(c["tracks"][lo:hi])
    radius = _dev(c["radius"][lo:hi])
    visible = None if c["visible"] is None else _dev(c["visible"][lo:hi], np.uint8)
    m, _, stride = t.shape
    nbytes = lib.nfopp_spacetime_reserve_workspace_bytes(m)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    L.check(lib.nfopp_spacetime_reserve(*_geometry(c), L.ptr(t), m, stride, L.ptr(radius), L.ptr(visible, torch.uint8),
                                        L.ptr(words, torch.int64), words.numel() * 8, L.ptr(ws, torch.uint8), nbytes, L.stream_ptr()))
    return words


def _raw_plan(c, words, order="case"):
    rc, out = _plan_call(c, words, order)
    _lib.check(rc)
    return out


def _plan_call(c, words, order="case"):
    """-> (the entry's return value, (cells, arrival, status, tracks) poisoned with -7 / 7.0 before the call)."""
    lib, L = _lib.load(), _lib
    g, T = c["geo"], c["T"]
    r = len(c["starts"])
    occ, starts, goals = _dev(c["occ"], np.uint8), _dev(c["starts"], np.int32), _dev(c["goals"], np.int32)
    order = _dev(c["order"] if isinstance(order, str) else order, np.int32)
    cells = torch.full((r, T), -7, dtype=torch.int32, device="cuda")
    arrival = torch.full((r,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((r,), -7, dtype=torch.int32, device="cuda")
    tracks = torch.full((r, T, 2), 7.0, dtype=torch.float32, device="cuda")
    nbytes = lib.nfopp_spacetime_plan_workspace_bytes(g.rows, g.cols, T, r)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.nfopp_spacetime_plan_fleet(L.ptr(occ, torch.uint8), *_geometry(c), L.ptr(starts, torch.int32), L.ptr(goals, torch.int32),
                                        L.ptr(order, torch.int32), r, L.ptr(words, torch.int64), words.numel() * 8,
                                        L.ptr(cells, torch.int32), L.ptr(arrival, torch.int32), L.ptr(status, torch.int32),
                                        L.ptr(tracks), L.ptr(ws, torch.uint8), nbytes, L.stream_ptr())
    return rc, (cells, arrival, status, tracks)


def _split(c, words):
    g, T = c["geo"], c["T"]
    n = (T - 1) * 9 * g.rows * g.words
    w = _u64(words)
    return w[:n].reshape(T - 1, 9, g.rows, g.words), w[n:].reshape(g.rows, g.words)


def _check_reservation(c, words, want, label):
    blocked, last = _split(c, words)
    wb, wl = want.words()
    assert np.array_equal(last, wl), (label, "last", np.argwhere(last != wl)[:6])
    assert np.array_equal(blocked, wb), (label, "blocked", np.argwhere(blocked != wb)[:6])


def _check_plan(got, want, label):
    cells, arrival, status, tracks = got
    assert np.array_equal(status.cpu().numpy(), want["status"]), (label, "status", status.tolist(), want["status"].tolist())
    assert np.array_equal(arrival.cpu().numpy(), want["arrival"]), (label, "arrival", arrival.tolist(), want["arrival"].tolist())
    assert np.array_equal(cells.cpu().numpy(), want["cells"]), (label, "cells", np.argwhere(cells.cpu().numpy() != want["cells"])[:6])
    off = (want["status"] != 0)
    got_t = tracks.cpu().numpy()
    assert np.array_equal(got_t[~off].view(np.uint32), want["tracks"][~off].view(np.uint32)), (label, "tracks")
    assert np.isnan(got_t[off]).all(), (label, "NaN rows")


def _run(c, label, before=None):
    """init, reserve, plan on the device against the restatement -> (device outputs, words after, restated plan)."""
    before = sc.reservation(c) if before is None else before
    after = before.copy()
    want = sr.plan_fleet(after, c["starts"], c["goals"], c["order"])
    words = _raw_init(c)
    _check_reservation(c, words, sr.Reservation(c["occ"], c["geo"], c["T"], c["robot_radius"], c["margin"]), (label, "static"))
    _raw_reserve(c, words)
    _check_reservation(c, words, before, (label, "movers"))
    got = _raw_plan(c, words)
    _check_plan(got, want, label)
    _check_reservation(c, words, after, (label, "after the fleet"))
    return got, words, want, after


@functools.lru_cache(maxsize=None)
def _sized(n):
    """Case n and the restatement of its movers' reservation: computed once, never written to."""
    c = sc.sized_case(n)
    return c, sc.reservation(c)


@pytest.mark.parametrize("n", range(len(sc.SIZES)), ids=["%dx%dx%dx%dx%d" % s for s in sc.SIZES])
def test_bitmaps_and_plans_equal_the_restatement_bit_for_bit(n):
    c, before = _sized(n)
    rows, cols, T, m, r = sc.SIZES[n]
    seen = set()
    for name, order in sorted(sc.orders(r, seed=n).items()):
        co = dict(c, order=order)
        got, words, want, _ = _run(co, (n, name), before)
        seen |= set(want["status"].tolist())
        again = _raw_plan(co, _raw_reserve(co, _raw_init(co)))                # a second run gives the same bits
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(got, again))
    if m >= 2:                                                                # reserve in two halves equals one call
        halves = _raw_reserve(c, _raw_reserve(c, _raw_init(c), 0, m // 2), m // 2, None)
        whole = _raw_reserve(c, _raw_init(c))
        assert torch.equal(halves, whole)
    if r >= 3:
        assert seen >= {0, sr.STATUS_BAD_CELL, sr.STATUS_NOT_ORDERED}


def test_hand_cases():
    for label, c, status, arrival in (("corridor", sc.corridor(), [0, 0], [6, 6]), ("no bay", sc.corridor(bay=False), [0, 2], [6, -1]),
                                      ("reversed", sc.corridor(order=[1, 0]), [0, 0], [6, 6]), ("gate", sc.gate(), [0], [10]),
                                      ("parked", sc.parked_on_goal(), [2], [-1]), ("leaves", sc.parked_on_goal(leaves=6), [0], [6]),
                                      ("T = 1", sc.single_instant((0, 0), False), [0], [0]),
                                      ("T = 1, last", sc.single_instant((0, 0), True), [2], [-1]),
                                      ("T = 1, elsewhere", sc.single_instant((0, 1), False), [2], [-1]),
                                      ("exactly R", sc.strict(False), [0], [0]), ("one step closer", sc.strict(True), [2], [-1])):
        (cells, arr, st, _), _, _, _ = _run(c, label)
        assert st.tolist() == status and arr.tolist() == arrival, (label, st.tolist(), arr.tolist())
        if label == "corridor":
            assert 3 in cells[1].tolist() and 3 not in cells[0].tolist()      # robot 1 takes the bay (0, 3)
        if label == "reversed":
            assert 3 in cells[0].tolist() and 3 not in cells[1].tolist()
        if label == "gate":
            assert cells[0].tolist() == [0, 0, 1, 0, 1, 2, 3, 4, 5, 6, 7, 7]


@pytest.mark.parametrize("name", list(sc.EDGES))
def test_sizes_past_one_trip_and_the_largest_frontier_equal_the_restatement_bit_for_bit(name):
    """spacetime_cases.EDGES through init, reserve, plan, the reservation after the fleet, and a second run on fresh poisoned
    buffers; what each case reaches is computed in tests/test_spacetime_cpu.py."""
    c = sc.edge_case(name)
    _, status, arrival = sc.EDGES[name]
    (cells, arr, st, tracks), words, want, _ = _run(c, name)
    visited = np.flatnonzero(want["status"] != sr.STATUS_NOT_ORDERED)
    assert st.cpu().numpy()[visited].tolist() == status and arr.cpu().numpy()[visited].tolist() == arrival, (name, visited)
    again = _raw_plan(c, _raw_reserve(c, _raw_init(c)))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((cells, arr, st, tracks), again))
    if name == "R=513":       # everyone `order` leaves out holds what the init kernel wrote, past its grid's one trip too
        off = torch.tensor(want["status"] == sr.STATUS_NOT_ORDERED, device="cuda")
        assert int(off.sum()) == len(c["starts"]) - 3 and len(c["starts"]) * c["T"] > sc.INIT_GRID * sc.INIT_THREADS
        assert (cells[off] == -1).all() and (arr[off] == -1).all() and torch.isnan(tracks[off]).all()


def test_a_frontier_one_row_past_the_largest_is_refused_and_nothing_is_written():
    c = sc.largest_frontier(sc.LARGEST_RW + 1)
    words = _raw_init(c)
    before = words.clone()
    rc, (cells, arrival, status, tracks) = _plan_call(c, words)
    assert rc == -1 and "frontier too large" in _lib.load().nfopp_last_error().decode()
    torch.cuda.synchronize()
    assert (cells == -7).all() and (arrival == -7).all() and (status == -7).all() and (tracks == 7.0).all()
    assert torch.equal(words, before)


def _grid(c):
    g = c["geo"]
    return nfopp.OccupancyGrid(c["occ"], (g.b0, g.b0 + g.cols * g.res, g.b2, g.b2 + g.rows * g.res), g.res, device="cuda")


def test_nobody_planned_is_in_conflict_by_the_conflict_kernel_and_the_python_interface_equals_the_raw_calls():
    for n in (6, 7):
        c = _sized(n)[0]
        grid = _grid(c)
        tracks = _dev(c["tracks"])
        plan = nfopp.spacetime_plan(grid, _dev(c["starts"], np.int32), _dev(c["goals"], np.int32), c["T"], robot_radius=c["robot_radius"],
                                    margin=c["margin"], tracks=tracks, track_radius=_dev(c["radius"]), visible=_dev(c["visible"], np.uint8))
        raw = _raw_plan(c, _raw_reserve(c, _raw_init(c)))
        assert isinstance(plan, nfopp.SpaceTimePlan)
        for x, y in zip((plan.cells, plan.arrival, plan.status, plan.tracks), raw):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        want_after = _sized(n)[1].copy()
        sr.plan_fleet(want_after, c["starts"], c["goals"], None)
        _check_reservation(c, plan.reservation.words, want_after, (n, "python"))
        assert plan.reservation.blocked.shape == (c["T"] - 1, 9, c["geo"].rows, c["geo"].words) and plan.reservation.last.shape == (c["geo"].rows, c["geo"].words)
        on = plan.planned
        assert torch.equal(on, plan.status == 0) and on.sum() >= 4
        fleet = nfopp.track_conflicts(plan.tracks[on], dt=1.0, radius_a=c["robot_radius"], margin=c["margin"])
        assert not fleet.in_conflict.any()
        good = torch.tensor(sr.good_tracks(c["tracks"], c["radius"], c["visible"]), device="cuda")
        floor = nfopp.track_conflicts(plan.tracks[on], tracks[good][:, :, :2].contiguous(), dt=1.0, radius_a=c["robot_radius"],
                                      radius_b=_dev(c["radius"])[good], margin=c["margin"])
        assert not floor.in_conflict.any()
        # points for cells, a reservation to go on from, an order
        pts = _dev(np.stack([sr.Geometry.centre_of(c["geo"], r, q) for r, q in c["starts"]]))
        res = nfopp.SpaceTimeReservation(grid, c["T"], c["robot_radius"], c["margin"]).add(tracks, _dev(c["radius"]), _dev(c["visible"], np.uint8))
        _check_reservation(c, res.words, _sized(n)[1], (n, "add"))
        again = nfopp.spacetime_plan(grid, pts, _dev(c["goals"], np.int32), c["T"], robot_radius=c["robot_radius"], margin=c["margin"],
                                     reservation=res.clone())
        assert torch.equal(again.cells, plan.cells) and torch.equal(again.reservation.words, plan.reservation.words)
        assert not torch.equal(res.words, plan.reservation.words)


def test_the_circle_fleet_from_schedule_through_replan_is_on_the_floor_and_clear():
    """fleet_schedule_cases.circle(16, 18, 7): the schedule leaves 8 of 16 unresolved; re-planned on a wall-free 24 x 24 grid of
    0.25 m over 41 instants everyone is on the floor, and the 16 merged tracks are clear by the conflict kernel."""
    case, geo, count = sc.circle_replan()
    tracks = _dev(case["tracks"])
    radius = float(case["radius"][0])
    sched = nfopp.schedule_delays(tracks, max_delay=case["max_delay"], radius=radius, margin=case["margin"])
    _, want_s = fc.solve(case)
    assert np.array_equal(sched.status.cpu().numpy(), want_s["status"]) and (want_s["status"] == fr.STATUS_UNRESOLVED).sum() == 8
    grid = nfopp.OccupancyGrid(np.zeros((geo.rows, geo.cols), np.uint8), (geo.b0, geo.b0 + geo.cols * geo.res, geo.b2, geo.b2 + geo.rows * geo.res),
                               geo.res, device="cuda")
    plan, merged = sched.replan(tracks, grid, count, robot_radius=radius, base_margin=case["margin"])
    c, want, want_merged = sc.replan_ref(case, want_s, geo, count)
    _check_plan((plan.cells, plan.arrival, plan.status, plan.tracks), want, "replan")
    assert np.array_equal(merged.cpu().numpy().view(np.uint32), want_merged.view(np.uint32))
    assert torch.equal(plan.planned, sched.status == nfopp.SCHEDULE_UNRESOLVED) and not torch.isnan(merged).any()
    found = nfopp.track_conflicts(merged, dt=1.0, radius_a=radius, margin=case["margin"])
    assert not found.in_conflict.any()


def test_replan_searches_the_unresolved_robots_only():
    """The circle fleet with a NaN planted in robot 5 and an odd schedule order: the bad robot and the ones the schedule never
    visited are not searched -- NOT_ORDERED from the plan, NaN rows in the merged tracks --, the unresolved ones are."""
    case, geo, count = sc.circle_replan_odd()
    tracks = _dev(case["tracks"])
    radius = float(case["radius"][0])
    sched = nfopp.schedule_delays(tracks, max_delay=case["max_delay"], radius=radius, margin=case["margin"], order=case["order"])
    _, want_s = fc.solve(case)
    st = want_s["status"]
    assert np.array_equal(sched.status.cpu().numpy(), st) and st[5] == fr.STATUS_BAD_TRACK
    assert set(st.tolist()) == {0, fr.STATUS_BAD_TRACK, fr.STATUS_UNRESOLVED, fr.STATUS_NOT_ORDERED}
    grid = nfopp.OccupancyGrid(np.zeros((geo.rows, geo.cols), np.uint8), (geo.b0, geo.b0 + geo.cols * geo.res, geo.b2, geo.b2 + geo.rows * geo.res),
                               geo.res, device="cuda")
    plan, merged = sched.replan(tracks, grid, count, robot_radius=radius, base_margin=case["margin"])
    c, want, want_merged = sc.replan_ref(case, want_s, geo, count)
    _check_plan((plan.cells, plan.arrival, plan.status, plan.tracks), want, "replan, odd")
    assert np.array_equal(merged.cpu().numpy().view(np.uint32), want_merged.view(np.uint32))
    skipped = torch.tensor((st == fr.STATUS_BAD_TRACK) | (st == fr.STATUS_NOT_ORDERED), device="cuda")
    assert skipped.sum() >= 3 and (plan.status[skipped] == nfopp.SPACETIME_NOT_ORDERED).all() and torch.isnan(merged[skipped]).all()
    assert torch.equal(plan.status != nfopp.SPACETIME_NOT_ORDERED, sched.status == nfopp.SCHEDULE_UNRESOLVED) and plan.planned.any()
    on = ~torch.isnan(merged[:, 0, 0])
    assert torch.equal(on, sched.scheduled | plan.planned)
    found = nfopp.track_conflicts(merged[on], dt=1.0, radius_a=radius, margin=case["margin"])
    assert not found.in_conflict.any()


def test_batch_planner_fleet_schedule_with_replan_equals_the_steps():
    z = load_golden("g1_onf.npz")
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    b, n = 6, 24
    rng = np.random.default_rng(3)
    starts = np.concatenate([rng.uniform(0.2, 0.8, (b, 2)), rng.uniform(-3, 3, (b, 1))], 1).astype(F32)
    goals = np.concatenate([rng.uniform(2.2, 2.8, (b, 2)), rng.uniform(-3, 3, (b, 1))], 1).astype(F32)
    bp = nfopp.BatchPlanner(onf, b, n, nfopp.TrajectoryHyper(collision_weight=3, direction_delta_weight=7, collision_beta=2))
    bp.init(starts, goals, (-0.1, 3.1, -0.1, 3.1))
    bp.step(n=3)
    lim = nfopp.MotionLimits(1.0, 0.5)
    dt, count, md, radius = 0.125, 48, 2, 0.1
    grid = nfopp.OccupancyGrid(np.zeros((32, 32), np.uint8), (-0.1, 3.1, -0.1, 3.1), 0.1, device="cuda")
    plain = bp.fleet_schedule(lim, dt, count, radius, md)
    got = bp.fleet_schedule(lim, dt, count, radius, md, replan=grid)
    assert torch.equal(got.delay, plain.delay) and torch.equal(got.status, plain.status) and not hasattr(plain, "plan")
    assert (got.status == nfopp.SCHEDULE_UNRESOLVED).any()
    states = bp.timed_paths(lim).sample(dt, count)
    plan, merged = plain.replan(states, grid, count + md, robot_radius=radius, base_margin=plain.margin)
    assert torch.equal(got.plan.cells, plan.cells) and torch.equal(got.plan.status, plan.status)
    assert torch.equal(got.merged.view(torch.int32), merged.view(torch.int32)) and merged.shape == (b, count + md, 2)
    assert torch.equal(plan.status != nfopp.SPACETIME_NOT_ORDERED, plain.status == nfopp.SCHEDULE_UNRESOLVED)
    on = ~torch.isnan(merged[:, 0, 0])
    assert on.sum() >= plain.scheduled.sum()
    found = nfopp.track_conflicts(merged[on], dt=dt, radius_a=radius, margin=plain.margin)
    assert not found.in_conflict.any()


def test_the_torch_ops_equal_the_raw_calls():
    ops = torch_ops.load()
    for n in (5, 6):
        c = _sized(n)[0]
        g = c["geo"]
        args = (_dev(c["occ"], np.uint8), c["T"], g.b0, g.b2, g.res, c["robot_radius"], c["margin"])
        static = ops.spacetime_reserve(*args, None, None, None, None)
        assert torch.equal(static, _raw_init(c))
        m = len(c["tracks"])
        half = ops.spacetime_reserve(*args, None, _dev(c["tracks"][:m // 2]), _dev(c["radius"][:m // 2]), _dev(c["visible"][:m // 2], np.uint8))
        words = ops.spacetime_reserve(*args, half, _dev(c["tracks"][m // 2:]), _dev(c["radius"][m // 2:]), _dev(c["visible"][m // 2:], np.uint8))
        raw = _raw_reserve(c, _raw_init(c))
        assert torch.equal(words, raw) and not torch.equal(half, words)
        assert n == 5 or not torch.equal(static, half)                        # case 5: the first half is the one invisible mover
        order = sc.orders(len(c["starts"]), seed=n)["odd"]
        want = _raw_plan(dict(c, order=order), raw)
        got = ops.spacetime_plan_fleet(*args, _dev(c["starts"], np.int32), _dev(c["goals"], np.int32), _dev(order, np.int32), words)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(got, want)) and torch.equal(words, raw)
    with pytest.raises(RuntimeError, match="count"):
        ops.spacetime_reserve(*args, None, _dev(c["tracks"][:, :-1]), None, None)
    with pytest.raises(RuntimeError, match="reservation"):
        ops.spacetime_plan_fleet(*args, _dev(c["starts"], np.int32), _dev(c["goals"], np.int32), None, words[:-1])
    empty = ops.spacetime_plan_fleet(*args, _dev(c["starts"][:0], np.int32), _dev(c["goals"][:0], np.int32), None, words)
    assert empty[0].shape == (0, c["T"]) and empty[3].shape == (0, c["T"], 2)
