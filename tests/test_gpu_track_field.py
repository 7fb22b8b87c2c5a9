"""GPU: the moving-obstacle collision term (csrc/track_field.hip, nfopp/moving.py) against its restatement
(tests/track_field_ref.py): the overlay at explicit poses and times (bit for bit where no sine is taken, within 16 x the spread
of the float32 and float64 restatements where one is), trajectory mode behind each of the three collision entries, the engine
and the batch planner with `moving`, `moving=None` against the entries it took before, and yielding to a crossing vehicle."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import guarded as gd  # noqa: E402
import heading_field_cases as hc  # noqa: E402
import nfopp  # noqa: E402
import sdf_cases as sc  # noqa: E402
import track_field_cases as tc  # noqa: E402
import track_field_ref as ref  # noqa: E402
from nfopp import _lib  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402

F32 = np.float32
DEV = "cuda"
FILLS = (0x00, 0xFF)


def _moving(tracks, radius, discs, margin=0.05, gain=10.0, dim=3, t0=tc.T0, dt=tc.DT):
    return nfopp.MovingObstacles(torch.tensor(tracks, device=DEV), dt, t0=t0, radius=torch.tensor(radius, device=DEV),
                                 discs=discs, margin=margin, gain=gain, dim=dim)


def _same_bits(got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    if not np.array_equal(a, b):
        rows = np.unique(np.argwhere(a != b)[:, 0])[:5]
        raise AssertionError("rows %s differ: got %s, want %s" % (rows, np.asarray(got)[rows].tolist(), np.asarray(want)[rows].tolist()))


# The spread of the two restatements over each float64 case, per output column: computed here, on the CPU, at import.
SPREAD = {name: ref.spread(tc.f64_field(name), *tc.F64_CASES[name][5:]) for name in tc.F64_CASES}


# ---- explicit poses and times, no trigonometry ---------------------------------------------------------------------------------
def _overlay_guarded(moving, poses, times, base, fill):
    """nfopp_track_field_eval_points with out4 inside guard bytes, pre-filled with `fill` and then with the rows of `base`
    (None: left at the fill) -> the [P, 4] result (numpy)."""
    pts, pts_parent = gd.from_array(poses, DEV)
    tm, tm_parent = gd.from_array(times, DEV)
    snaps = gd.snapshot(pts_parent), gd.snapshot(tm_parent)
    out, parent = gd.guarded((len(poses), 4), torch.float32, DEV, fill)
    if base is not None:
        out.copy_(torch.tensor(base))
    _lib.check(_lib.load().nfopp_track_field_eval_points(moving.config_c(), _lib.ptr(pts), _lib.ptr(tm), len(poses), poses.shape[1],
                                                         _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert gd.guards_intact(parent) and gd.unchanged(pts_parent, snaps[0]) and gd.unchanged(tm_parent, snaps[1])
    return out.cpu().numpy()


@pytest.mark.parametrize("stride", tc.STRIDES)
@pytest.mark.parametrize("k", tc.INSTANT_COUNTS)
@pytest.mark.parametrize("m", tc.TRACK_COUNTS)
def test_explicit_mode_bits(m, k, stride):
    """Every count of poses and both pose dimensions on one set of tracks: rows of logit -inf, +inf, NaN, below, above and equal
    to the track row's; only rows the track row beats change, the others keep their bits; poses and times that are not finite
    and a track with a NaN coordinate are among them."""
    for dim in (2, 3):
        for count in tc.POINT_COUNTS:
            field, tracks, radius, poses, times = tc.explicit_case(m, k, stride, count, dim)
            moving = _moving(tracks, radius, tc.CENTRED, dim=dim)
            assert (moving.config_c().stride, moving.config_c().k, moving.config_c().m) == (stride, k, m)
            rows, _, _ = ref.track_rows(field, poses, times, F32)
            base = tc.base_rows(rows, count)
            want, won = ref.overlay(field, poses, times, base)
            for fill in FILLS:
                got = _overlay_guarded(moving, poses, times, base, fill)
                _same_bits(got, want)
                _same_bits(got[~won], base[~won])
            if count >= 64:
                assert won.any() and not won.all()
        # the Python entry, base=None: the pure track row, and -inf rows where there is none
        pure = moving.eval(poses, times).cpu().numpy()
        want, won = ref.overlay(field, poses, times, np.tile(np.asarray([-np.inf, 0, 0, 0], F32), (len(poses), 1)))
        _same_bits(pure, want)
        assert (pure[~won] == np.asarray([-np.inf, 0, 0, 0], F32)).all()


def test_rows_that_are_not_beaten_are_not_written():
    """out4 left at its fill (0xFF: a NaN logit) keeps every byte; at 0x00 (logit 0) only the winning rows change."""
    field, tracks, radius, poses, times = tc.coverage_case()
    moving = _moving(tracks, radius, tc.CENTRED)
    got = _overlay_guarded(moving, poses, times, None, 0xFF)
    assert (got.view(np.uint8) == 0xFF).all()
    got = _overlay_guarded(moving, poses, times, None, 0x00)
    want, won = ref.overlay(field, poses, times, np.zeros((len(poses), 4), F32))
    _same_bits(got, want)
    assert won.any() and (got[~won].view(np.uint32) == 0).all()


def test_hand_cases():
    field, pose, time, R = tc.standing_case()
    moving = nfopp.MovingObstacles(torch.tensor(field.tracks, device=DEV), tc.DT, t0=tc.T0, radius=0.25, robot_radius=0.5,
                                   margin=0.125, gain=2.0)
    got = moving.eval(pose, time).cpu().numpy()
    _same_bits(got, ref.track_rows(field, pose, time, F32)[0])
    assert got[0, 0] == F32(2.0 * (R - 1.25)) and abs(got[0, 1] + 1.2) < 1e-6 and abs(got[0, 2] + 1.6) < 1e-6
    on_it = np.concatenate([field.tracks[0, 0, :2], [0.3]])[None].astype(F32)
    assert moving.eval(on_it, time).cpu().numpy()[0].tolist() == [2.0 * R, 0, 0, 0]
    # the first of two equal penetrations wins
    tracks, pose, time = tc.tie_case()
    for order, sign in ((tracks, 1.0), (tracks[::-1].copy(), -1.0)):
        got = nfopp.MovingObstacles(torch.tensor(order, device=DEV), tc.DT, t0=tc.T0, robot_radius=0.0, gain=2.0).eval(pose, time)
        assert got.cpu().numpy()[0].tolist() == [-2.0, 2.0 * sign, 0, 0]
    # no obstacles: every row stays
    none = nfopp.MovingObstacles(torch.zeros(0, 4, 2, device=DEV), tc.DT, robot_radius=0.1)
    base = np.arange(8, dtype=F32).reshape(2, 4)
    _same_bits(none.eval(np.zeros((2, 3), F32), np.zeros(2, F32), base=base).cpu().numpy(), base)


# ---- offset discs: a sine is taken ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.F64_CASES))
def test_offset_discs_against_float64(name):
    """The device may differ from the float32 restatement only through sinf / cosf; it is held to 16 x the spread of the two
    restatements per output column, over the poses at which they take the same disc, track and interval.
    Measured on MI355X: see the table there."""
    tracks, radius, discs, margin, gain, poses, times = tc.F64_CASES[name]
    spread, kept = SPREAD[name]
    got = _moving(tracks, radius, discs, margin, gain).eval(poses, times).cpu().numpy()
    want, _, _ = ref.track_rows(tc.f64_field(name), poses, times, np.float64)
    dist = np.abs(got.astype(np.float64) - want)[kept].max(0)
    print("%s: SPREAD %s, device distance %s, excluded %d of %d" % (name, spread, dist, (~kept).sum(), len(kept)))
    assert np.isfinite(got).all()
    assert (dist <= 16 * spread).all(), (dist, spread)


# ---- trajectory mode behind each collision entry -----------------------------------------------------------------------------------
KINDS = (("onf", 2), ("onf", 3), ("sdf", 2), ("sdf", 3), ("hdf", 3))


@functools.lru_cache(maxsize=None)
def _model(kind, dim):
    if kind == "onf":
        torch.random.manual_seed(3)
        return nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=dim == 3).to(DEV)
    if kind == "sdf":
        g = tc.TRAJ_GRID
        return nfopp.DistanceField(nfopp.OccupancyGrid(g.occupancy, g.boundaries, g.resolution, device=DEV),
                                   discs=tc.CENTRED if dim == 2 else tc.THREE_DISCS, margin=0.05, gain=10.0, dim=dim)
    lay = hc.FIELD_LAYERS["16x37x53"]
    return nfopp.HeadingDistanceField(lay.occupancy, lay.boundaries, lay.resolution, margin=0.05, gain=10.0, device=DEV)


@functools.lru_cache(maxsize=None)
def _traj_moving(dim):
    tracks = tc.traj_tracks()
    return _moving(tracks, tc.random_radii(len(tracks), 43), tc.CENTRED if dim == 2 else tc.THREE_DISCS, dim=dim)


@functools.lru_cache(maxsize=None)
def _planner_moving(dim):
    """The same tracks with 0.5 m more radius and margin: deep enough to beat rows of a sample inside a wall, so the overlay
    has a say in every planner test whatever the seeds."""
    tracks = tc.traj_tracks()
    return _moving(tracks, tc.random_radii(len(tracks), 43) + F32(0.5), tc.CENTRED if dim == 2 else tc.THREE_DISCS, margin=0.5, dim=dim)


def _base_entry(kind, model, traj, B, N, dim, t, mode, seed, offset, index_offset, out, active):
    """The collision entry of `kind` on device tensors."""
    lib, P, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    act = P(active, torch.uint8)
    if kind == "onf":
        live = torch.zeros(B + 1, dtype=torch.int32, device=DEV) if active is not None else None
        rc = lib.nfopp_traj_collision_eval(model.config_c(), P(model.flat_parameters), P(traj), B, N, dim, P(t), mode, seed, offset,
                                           index_offset, P(out), act, P(live, torch.int32), st)
    elif kind == "sdf":
        rc = lib.nfopp_traj_sdf_collision_eval(model.config_c(), P(traj), B, N, dim, P(t), mode, seed, offset, index_offset, P(out),
                                               act, st)
    else:
        rc = lib.nfopp_traj_hdf_collision_eval(model.config_c(), P(traj), B, N, P(t), mode, seed, offset, index_offset, P(out), act, st)
    _lib.check(rc)


@pytest.mark.parametrize("kind,dim", KINDS)
@pytest.mark.parametrize("B,N", tc.TRAJ_SHAPES)
def test_trajectory_mode(kind, dim, B, N):
    model, moving = _model(kind, dim), _traj_moving(dim)
    traj = sc.random_trajectories(tc.TRAJ_GRID, B, N, dim)
    wp = tc.waypoint_times(B, N)
    seed, offset, index_offset = 1234, 5, 7
    lib, P = _lib.load(), _lib.ptr
    for fill in FILLS:
        results = []
        for active in (None, torch.tensor(np.arange(B) % 2 == 0, device=DEV).to(torch.uint8)):
            tr, tr_parent = gd.from_array(traj, DEV)
            wt, wt_parent = gd.from_array(wp, DEV)
            t, t_parent = gd.guarded((B, N - 1), torch.float32, DEV, fill)
            out, out_parent = gd.guarded((B, N - 1, 4), torch.float32, DEV, fill)
            _base_entry(kind, model, tr, B, N, dim, t, 1, seed, offset, index_offset, out, active)
            base = out.clone()
            snaps = [gd.snapshot(p) for p in (tr_parent, wt_parent, t_parent)]
            _lib.check(lib.nfopp_traj_track_overlay(moving.config_c(), P(tr), P(wt), B, N, dim, P(t), P(out), P(active, torch.uint8),
                                                    _lib.stream_ptr()))
            torch.cuda.synchronize()
            assert gd.guards_intact(out_parent)
            assert all(gd.unchanged(p, s) for p, s in zip((tr_parent, wt_parent, t_parent), snaps))      # t is not written
            results.append((t.cpu().numpy(), base.cpu().numpy(), out.cpu().numpy()))
        (t_np, base_np, out_np), (_, basem, outm) = results
        # the base entry's rows overlaid by the explicit entry at the oracle's samples and times
        pts = (orc.sample_collision_points if dim == 3 else orc.sample_collision_points_2d)(traj, t_np)
        tau = ref.sample_times(wp, t_np)
        want = moving.eval(pts.reshape(-1, dim), tau.reshape(-1), base=base_np.reshape(-1, 4)).cpu().numpy().reshape(B, N - 1, 4)
        _same_bits(out_np, want)
        changed = (out_np.view(np.uint32) != base_np.view(np.uint32)).any(-1)
        if B * (N - 1) >= 100:
            assert changed.any() and not changed.all()
        # with a mask: retired rows keep their bytes, live rows are those of the unmasked launch
        live = np.arange(B) % 2 == 0
        _same_bits(outm[live], out_np[live])
        assert (outm[~live].view(np.uint8) == fill).all() and (basem[~live].view(np.uint8) == fill).all()


# ---- engine and planner ----------------------------------------------------------------------------------------------------------------
def _planner(kind, dim, B, N, moving="default", freq=3, seed=5, times=True):
    g = tc.TRAJ_GRID
    rng = np.random.default_rng(11)
    b = g.boundaries
    ends = [np.stack([rng.uniform(b[0] + 0.3, b[1] - 0.3, B), rng.uniform(b[2] + 0.3, b[3] - 0.3, B), rng.uniform(-3, 3, B)], 1)
            [:, :dim].astype(F32) for _ in range(2)]
    hp = nfopp.TrajectoryHyper(collision_weight=5, collision_beta=2, direction_delta_weight=1, bounds=b)
    kw = {} if moving == "absent" else dict(moving=_planner_moving(dim) if moving == "default" else moving)
    p = nfopp.BatchPlanner(_model(kind, dim), B, N, hp, device=DEV, seed=seed, reparametrize_trajectory_freq=freq, **kw)
    p.init(ends[0], ends[1], b)
    if times:
        p.set_waypoint_times(tc.waypoint_times(B, N))
    return p


def _state(p):
    e = p.engine
    torch.cuda.synchronize()
    bufs = [x for x in (e.traj, e.lam, e.cm, e.adam_m, e.adam_v, e.terms, e.t, e.onf_out) if x is not None]
    return [x.cpu().numpy().copy() for x in bufs] + [e.adam_step, e.rng_offset, p.step_count]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint32) if isinstance(x, np.ndarray) else x,
                              np.asarray(y).view(np.uint32) if isinstance(y, np.ndarray) else y)


@pytest.mark.parametrize("kind,dim", KINDS)
def test_engine_step_is_collision_entry_overlay_then_update(kind, dim):
    p = _planner(kind, dim, 3, 20)
    e = p.engine
    lib, P = _lib.load(), _lib.ptr
    c = {k: (None if getattr(e, k) is None else getattr(e, k).clone()) for k in ("traj", "lam", "cm", "adam_m", "adam_v", "t", "onf_out", "terms")}
    _base_entry(kind, e.onf, c["traj"], e.B, e.N, e.D, c["t"], 1, e.seed, e.rng_offset, e.traj_index_offset, c["onf_out"], None)
    static = c["onf_out"].clone()
    _lib.check(lib.nfopp_traj_track_overlay(e.moving.config_c(), P(c["traj"]), P(e.wp_time), e.B, e.N, e.D, P(c["t"]), P(c["onf_out"]),
                                            None, _lib.stream_ptr()))
    assert not torch.equal(static.view(torch.int32), c["onf_out"].view(torch.int32))        # the overlay had a say
    _lib.check(lib.nfopp_traj_update(e.hyper.to_c(e.adam_step + 1), e.B, e.N, e.D, P(c["traj"]), P(e.start), P(e.goal), P(c["lam"]),
                                     P(c["cm"]), P(c["adam_m"]), P(c["adam_v"]), P(c["t"]), P(c["onf_out"]), P(e.hinv_band),
                                     e.half_width, e.interior[0], e.interior[1], P(c["terms"]), None, _lib.stream_ptr()))
    seed = e.traj.clone()
    e.optimize_trajectory(want_terms=True)
    torch.cuda.synchronize()
    for k, v in c.items():
        if v is not None:
            assert np.array_equal(gd.bits(v), gd.bits(getattr(e, k))), k
    assert not torch.equal(e.traj, seed)


@pytest.mark.parametrize("kind,dim", (("onf", 3), ("sdf", 3), ("hdf", 3), ("sdf", 2)))
@pytest.mark.parametrize("injected", [False, True])
def test_step_n_equals_n_steps(kind, dim, injected):
    B, N, n = 4, 33, 7
    one, many = (_planner(kind, dim, B, N, freq=3) for _ in range(2))
    for p in (one, many):
        p.engine.active = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device=DEV)
    t = np.random.default_rng(2).uniform(0, 1, (n, B, N - 1)).astype(F32) if injected else None
    seed = many.engine.traj.clone()
    for k in range(n):
        one.step(None if t is None else t[k], want_terms=True)
    many.step(t, want_terms=True, n=n)
    a, b = _state(one), _state(many)
    if injected:      # the single steps copy the draws into the engine's t; step(n) reads them where they are
        a.pop(6 if dim == 3 else 4), b.pop(6 if dim == 3 else 4)
    _same(a, b)
    assert one.step_count == n and np.isfinite(many.get_paths()).all()
    moved = [not torch.equal(many.engine.traj[r], seed[r]) for r in range(B)]
    assert moved == [True, False, True, True]      # a retired row never moves


@pytest.mark.parametrize("kind,dim", KINDS)
def test_without_moving_obstacles_nothing_changes(kind, dim):
    """moving=None takes the calls it took before this term existed: seven steps equal the model's own step-loop entry called
    directly, single steps equal it too, and a set of no obstacles gives the same bits through the new entries."""
    B, N, n = 3, 20, 7
    absent, none, single = (_planner(kind, dim, B, N, moving=m, times=False) for m in ("absent", None, None))
    empty_set = nfopp.MovingObstacles(torch.zeros(0, 4, 2, device=DEV), tc.DT, discs=tc.CENTRED, dim=dim)
    empty = _planner(kind, dim, B, N, moving=empty_set)
    direct = _planner(kind, dim, B, N, moving=None, times=False)
    e = direct.engine
    P = _lib.ptr
    buf = _lib.TrajBuffersC(P(e.traj), P(e.start), P(e.goal), P(e.lam), P(e.cm), P(e.adam_m), P(e.adam_v), P(e.t), P(e.onf_out),
                            P(e.hinv_band), P(e.u), None, None, e.B, e.N, e.D, e.half_width, e.interior[0], e.interior[1])
    sched = _lib.StepScheduleC(float(e.hyper.lr), 0.9, 0.9, 0, 0, e.traj_index_offset, e.seed, 0, 3, 1)
    lib, hp, terms, st = _lib.load(), e.hyper.to_c(1), P(e.terms), _lib.stream_ptr()
    if kind == "onf":
        _lib.check(lib.nfopp_traj_steps(e.onf.config_c(), P(e.onf.flat_parameters), hp, buf, sched, n, None, terms, st))
    else:
        entry = lib.nfopp_traj_steps_sdf if kind == "sdf" else lib.nfopp_traj_steps_hdf
        _lib.check(entry(e.onf.config_c(), hp, buf, sched, n, None, terms, st))
    e.adam_step, e.rng_offset, direct.step_count = n, n, n
    for p in (absent, none, empty):
        p.step(n=n, want_terms=True)
    for _ in range(n):
        single.step(want_terms=True)
    want = _state(direct)
    for p in (absent, none, single, empty):
        _same(_state(p), want)


def test_moving_needs_waypoint_times_and_a_matching_robot():
    p = _planner("sdf", 3, 2, 8, times=False)
    before = _state(p)
    with pytest.raises(ValueError):
        p.step()
    with pytest.raises(ValueError):
        p.step(n=3)
    _same(_state(p), before)
    with pytest.raises(ValueError):
        p.set_waypoint_times(np.zeros((3, 8), F32))
    p.set_waypoint_times(np.linspace(0, 5, 8))            # [N]: every trajectory alike
    assert torch.equal(p.engine.wp_time[0], p.engine.wp_time[1])
    p.step(n=2)
    with pytest.raises(ValueError):
        _planner("sdf", 3, 2, 8, moving=_traj_moving(2))   # a robot without a heading behind SE(2) trajectories
    times = p.uniform_waypoint_times(1.0, 9.0)
    assert np.array_equal(times.numpy(), (1.0 + 9.0 * np.arange(1, 9) / 9.0).astype(F32))
    assert np.array_equal(p.engine.wp_time.cpu().numpy(), np.tile(times.numpy(), (2, 1)))


def test_update_keeps_the_buffer_and_gives_fresh_bits():
    tracks = tc.traj_tracks()
    radius = tc.random_radii(len(tracks), 43)
    moving = _moving(tracks, radius, tc.THREE_DISCS)
    ptr = moving.tracks.data_ptr()
    new = tc.traj_tracks(seed=77)
    moving.update(torch.tensor(new, device=DEV), t0=tc.T0 + 0.5)
    assert moving.tracks.data_ptr() == ptr == moving.config_c().tracks_dev and moving.config_c().t0 == F32(tc.T0 + 0.5)
    fresh = _moving(new, radius, tc.THREE_DISCS, t0=tc.T0 + 0.5)
    poses, times = tc.random_points(300, 3, tracks.shape[1], 5)
    _same_bits(moving.eval(poses, times).cpu().numpy(), fresh.eval(poses, times).cpu().numpy())
    # another horizon length is taken over as it is
    longer = torch.tensor(tc.traj_tracks(k=30, seed=78), device=DEV)
    moving.update(longer)
    assert moving.tracks.data_ptr() == longer.data_ptr() and moving.config_c().k == 30
    with pytest.raises(ValueError):
        moving.update(longer[:3])


# ---- behaviour -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_moving", [True, False])
def test_yields_to_a_crossing_vehicle(with_moving):
    """Straight seeds that meet a crossing vehicle head-on: in conflict before; after BEHAVIOUR_STEPS steps conflict-free with
    `moving` and still in conflict without, by the project's own predicate (nfopp.track_conflicts on the waypoint grid).  The
    restated pipeline (tests/test_track_field_cpu.py) is conflict-free from step BEHAVIOUR_FIRST_PASS = 24 on with the same
    injected draws."""
    case = tc.behaviour_case()
    g = case["grid"]
    grid = nfopp.OccupancyGrid(g.occupancy, g.boundaries, g.resolution, device=DEV)
    field = nfopp.DistanceField(grid, discs=case["discs"], margin=case["margin"], gain=case["gain"])
    tracks = torch.tensor(case["tracks"], device=DEV)
    moving = nfopp.MovingObstacles(tracks, case["dt"], t0=case["t0"], radius=case["obstacle_radius"], robot_radius=case["robot_radius"],
                                   margin=case["track_margin"], gain=case["track_gain"])
    B, N = len(case["starts"]), case["n_waypoints"]
    p = nfopp.BatchPlanner(field, B, N, gc.hyper_from(orc.Hyper(**case["hyper"])), device=DEV,
                           reparametrize_trajectory_freq=case["reparam_freq"], moving=moving if with_moving else None)
    p.init(case["starts"], case["goals"], g.boundaries, trajectories=nfopp.straight_line_init(case["starts"], case["goals"], N))
    if with_moving:
        times = p.uniform_waypoint_times(case["t0"], case["dt"] * (N + 1))
        assert np.array_equal(times.numpy(), case["wp_time"][0])

    def in_conflict():
        robots = p.engine.full_trajectory()[:, :, :2].contiguous()
        found = nfopp.track_conflicts(robots, tracks, dt=case["dt"], t0=case["t0"], radius_a=case["robot_radius"],
                                      radius_b=case["obstacle_radius"])
        return found.in_conflict.cpu().numpy()

    assert in_conflict().all()
    p.step(case["draws"], n=tc.BEHAVIOUR_STEPS)
    assert np.isfinite(p.get_paths()).all()
    assert not in_conflict().any() if with_moving else in_conflict().all()


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_leave_the_outputs_untouched():
    good = _traj_moving(3)
    lib, P, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    B, N = 2, 6
    traj = torch.tensor(sc.random_trajectories(tc.TRAJ_GRID, B, N, 3), device=DEV)
    wp = torch.tensor(tc.waypoint_times(B, N), device=DEV)
    pts = torch.tensor(sc.random_poses(tc.TRAJ_GRID, 10, 1), device=DEV)
    tm = torch.zeros(10, device=DEV)
    t = torch.full((B, N - 1), 0.5, device=DEV)

    def field(**changes):
        f = _lib.TrackFieldC.from_buffer_copy(good.config_c())
        for key, value in changes.items():
            setattr(f, key, value)
        return f

    out, parent = gd.guarded((10, 4), torch.float32, DEV, 0x5A)
    for f, dim in ((field(k=0), 3), (field(stride=1), 3), (field(m=-1), 3), (field(n_discs=0), 3), (field(n_discs=9), 3),
                   (field(tracks_dev=None), 3), (field(), 2), (field(inv_dt=0.0), 3), (field(gain=np.inf), 3), (field(t0=np.nan), 3)):
        assert lib.nfopp_track_field_eval_points(f, P(pts), P(tm), 10, dim, P(out), st) == -1 and lib.nfopp_last_error()
        assert lib.nfopp_traj_track_overlay(f, P(traj), P(wp), B, N, dim, P(t), P(out), None, st) == -1
    ok = good.config_c()
    assert lib.nfopp_track_field_eval_points(ok, P(pts), None, 10, 3, P(out), st) == -1
    assert lib.nfopp_traj_track_overlay(ok, P(traj), None, B, N, 3, P(t), P(out), None, st) == -1
    assert lib.nfopp_traj_track_overlay(ok, P(traj), P(wp), B, N, 3, None, P(out), None, st) == -1
    assert lib.nfopp_traj_track_overlay(ok, P(traj), P(wp), B, 1, 3, P(t), P(out), None, st) == -1
    torch.cuda.synchronize()
    off, n = gd.span(parent)
    assert gd.guards_intact(parent) and bool((parent[off:off + n] == 0x5A).all())
    # the step loop: a bad kind, track field or missing times is refused before the first launch
    p = _planner("sdf", 3, B, N)
    e = p.engine
    before = _state(p)
    buf = _lib.TrajBuffersC(P(e.traj), P(e.start), P(e.goal), P(e.lam), P(e.cm), P(e.adam_m), P(e.adam_v), P(e.t), P(e.onf_out),
                            P(e.hinv_band), P(e.u), None, None, e.B, e.N, e.D, e.half_width, e.interior[0], e.interior[1])
    hp = e.hyper.to_c(1)
    sched = _lib.StepScheduleC(1e-2, 0.9, 0.9, 0, 0, 0, 0, 0, 3, 1)
    model = ctypes.addressof(e.onf.config_c())
    for kind, fld, times in ((7, ok, P(e.wp_time)), (_lib.MODEL_SDF, field(k=0), P(e.wp_time)), (_lib.MODEL_SDF, ok, None),
                             (_lib.MODEL_SDF, None, P(e.wp_time)), (_lib.MODEL_ONF, ok, P(e.wp_time))):
        assert lib.nfopp_traj_steps_moving(kind, model, None, fld, times, hp, buf, sched, 2, None, None, st) == -1
    bad_sched = _lib.StepScheduleC(1e-2, 0.9, 0.9, 0, 0, 0, 0, 0, 0, 1)
    assert lib.nfopp_traj_steps_moving(_lib.MODEL_SDF, model, None, ok, P(e.wp_time), hp, buf, bad_sched, 2, None, None, st) == -1
    _same(before, _state(p))
