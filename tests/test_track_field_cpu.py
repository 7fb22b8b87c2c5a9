"""CPU: the restatement of the moving-obstacle collision term (tests/track_field_ref.py) has the properties the model is
defined by, the committed cases reach every branch and meet the condition under which the GPU tests compare against float64,
the restated planner step clears the behaviour scenario, and the built library exports the three entries and refuses what
it must without a device."""
import ctypes

import numpy as np
import pytest

import track_conflict_ref as tcr
import track_field_cases as tc
import track_field_ref as ref
from oracle import nfopp_oracle as orc

F32 = np.float32


# ---- hand cases ------------------------------------------------------------------------------------------------------------------
def test_standing_track():
    field, pose, time, R = tc.standing_case()
    rows, choice, valid = ref.track_rows(field, pose, time, F32)
    assert valid.all() and tuple(choice[0]) == (0, 0, 0)
    gain = F32(field.gain)
    assert rows[0, 0] == gain * F32(R - 1.25)                              # every term exact in fp32
    assert rows[0, 1] == gain * -(F32(0.75) / F32(1.25)) and rows[0, 2] == gain * -(F32(1.0) / F32(1.25))
    assert abs(rows[0, 1] / gain + 0.6) < 1e-7 and abs(rows[0, 2] / gain + 0.8) < 1e-7
    assert rows[0, 3] == 0
    # a standing track is the same at every time
    for t in (-1e9, tc.T0, 1e9):
        again, _, _ = ref.track_rows(field, pose, np.asarray([t], F32), F32)
        assert np.array_equal(again, rows)


def test_zero_distance_gives_a_zero_gradient():
    field, pose, time, R = tc.standing_case()
    on_it = np.concatenate([field.tracks[0, 0, :2], [0.3]])[None].astype(F32)
    rows, _, _ = ref.track_rows(field, on_it, time, F32)
    assert rows[0, 0] == F32(field.gain) * F32(R) and (rows[0, 1:] == 0).all()


def test_time_index_at_the_edges():
    tracks = np.zeros((1, 5, 2), F32)
    tracks[0, :, 0] = [0, 1, 3, 6, 10]
    field = ref.make_field(tracks, tc.DT, tc.T0)
    times = np.asarray([tc.T0 - 0.6, tc.T0, tc.T0 + 2 * tc.DT, tc.T0 + 2.5 * tc.DT, tc.T0 + 4 * tc.DT, tc.T0 + 9.0, np.nan], F32)
    n, n1, s, below, above = ref.time_index(field, times)
    assert n.tolist() == [0, 0, 2, 2, 3, 3, 0] and n1.tolist() == [1, 1, 3, 3, 4, 4, 1]
    assert s.tolist() == [0, 0, 0, 0.5, 1, 1, 0]
    assert below.tolist() == [True, True, False, False, False, False, True] and above.tolist() == [False] * 4 + [True, True, False]
    # the obstacle's x at those times, read off the row of a robot at the origin: logit = -dist
    far = ref.make_field(tracks, tc.DT, tc.T0, gain=1.0)
    rows, _, _ = ref.track_rows(far, np.zeros((6, 2), F32), times[:6], F32)
    assert (-rows[:, 0]).tolist() == [0, 0, 3, 4.5, 10, 10]
    # K = 1: one interval of no length
    n, n1, s, _, _ = ref.time_index(ref.make_field(tracks[:, :1], tc.DT, tc.T0), times)
    assert not n.any() and not n1.any() and not s.any()


def test_first_of_the_largest_wins_and_a_nan_never_does():
    tracks, pose, time = tc.tie_case()
    for order, sign in ((tracks, 1.0), (tracks[::-1], -1.0)):
        rows, choice, _ = ref.track_rows(ref.make_field(order, tc.DT, tc.T0, gain=2.0), pose, time, F32)
        assert choice[0, 1] == 0 and rows[0, 1] == F32(2.0 * sign) and rows[0, 2] == 0      # -(e / dist), e = c - q
    bad = np.concatenate([np.full((1, 1, 2), np.nan, F32), tracks])
    rows, choice, _ = ref.track_rows(ref.make_field(bad, tc.DT, tc.T0, gain=2.0), pose, time, F32)
    assert choice[0, 1] == 1 and rows[0, 1] == F32(2.0)
    rows, choice, _ = ref.track_rows(ref.make_field(bad[:1], tc.DT, tc.T0), pose, time, F32)
    assert choice[0, 1] == -1 and np.isnan(rows[0, 0])
    out, won = ref.overlay(ref.make_field(bad[:1], tc.DT, tc.T0), pose, time, np.asarray([[-np.inf, 1, 2, 3]], F32))
    assert not won.any() and out[0].tolist() == [-np.inf, 1, 2, 3]


# ---- the gradient ----------------------------------------------------------------------------------------------------------------
def test_float64_gradient_against_central_differences():
    """Away from ties (the same disc, track and interval at x - h, x and x + h) the float64 row's gradient is the derivative of
    its logit in x, y and theta at a fixed time.  The logit is gain * (R - |c - q|): its third derivative along any direction is
    at most 3 gain / dist^2 (times the lever cubed, <= 0.26^3, in theta), so with dist >= 0.1 m, gain 10 and h = 1e-4 the
    central difference is off by at most h^2 / 6 * 3000 = 5e-6."""
    tracks, radius, discs, margin, gain, poses, times = tc.F64_CASES["three_discs"]
    field = tc.f64_field("three_discs")
    h = 1e-4
    f64 = dict(dtype=np.float64, pose_dtype=np.float64)
    base, choice, valid = ref.track_rows(field, poses, times, **f64)
    keep = valid & ((field.discs[choice[:, 0], 2] + field.radius[choice[:, 1]] + field.margin) - base[:, 0] / gain >= 0.1)
    slope = []
    for comp in range(3):
        side = []
        for sign in (-1.0, 1.0):
            p = poses.astype(np.float64)
            p[:, comp] += sign * h
            out, ch, _ = ref.track_rows(field, p, times, **f64)
            keep &= ref.same_branch(ch, choice)
            side.append(out[:, 0])
        slope.append((side[1] - side[0]) / (2 * h))
    assert keep.sum() > len(poses) // 2
    for comp in range(3):
        assert np.abs(slope[comp] - base[:, 1 + comp])[keep].max() < 1e-4
    assert (np.abs(base[keep, 3]) > 1e-3).any()        # the heading column is a real one


# ---- what the committed cases reach ------------------------------------------------------------------------------------------------
def test_cases_reach_every_branch():
    field, tracks, radius, poses, times = tc.coverage_case()
    n, n1, s, below, above = ref.time_index(field, times)
    rows, choice, valid = ref.track_rows(field, poses, times, F32)
    assert below[valid].any() and above[valid].any() and (~below & ~above)[valid].any()     # both clamps and the inside
    assert (s[valid] == 0).any() and (s[valid] == 1).any() and ((s > 0) & (s < 1))[valid].any()
    assert (~valid).sum() == 12 and np.isnan(rows[~valid]).all()
    assert np.isnan(tracks[1, :, 0]).any() and (choice[valid, 1] != 1).any()                  # the NaN track is met
    at_nan = valid & (n == tracks.shape[1] // 2)
    assert at_nan.any() and (choice[at_nan, 1] != 1).all()
    base = tc.base_rows(rows, 3)
    out, won = ref.overlay(field, poses, times, base)
    assert won.any() and (~won & valid).any()
    for kind, wins in ((0, True), (1, False), (2, False), (3, True), (4, False), (5, False)):
        rows_of = valid & (np.arange(len(poses)) % 6 == kind) & np.isfinite(rows[:, 0])
        assert rows_of.any() and (won[rows_of] == wins).all(), kind
    assert np.array_equal(out[~won].view(np.uint32), base[~won].view(np.uint32))
    # K = 1 and the tie rule have cases of their own
    assert 1 in tc.INSTANT_COUNTS and tc.tie_case()[0].shape == (2, 1, 2)


@pytest.mark.parametrize("name", sorted(tc.F64_CASES))
def test_excluded_share(name):
    poses, times = tc.F64_CASES[name][5:]
    spread, kept = ref.spread(tc.f64_field(name), poses, times)
    print("%s: excluded %d of %d, SPREAD %s" % (name, (~kept).sum(), len(kept), spread))
    assert 1.0 - kept.mean() <= tc.MAX_EXCLUDED_SHARE
    assert np.isfinite(spread).all() and (spread > 0).all()


# ---- behaviour: the restated pipeline --------------------------------------------------------------------------------------------
def _conflicts(case, traj):
    r = tcr.conflicts(tc.behaviour_robot_tracks(case, traj), case["tracks"], dt=case["dt"], t0=case["t0"],
                      radius_a=case["robot_radius"], radius_b=case["obstacle_radius"])
    return r["summary"][:, tcr.SLOT_CONFLICTS] > 0


@pytest.mark.parametrize("with_moving", [True, False])
def test_restated_pipeline_yields_to_the_crossing_vehicle(with_moving):
    """track_field_ref.planner_step from the straight seeds: every seed is in conflict with the obstacle's track; with the
    overlay every path is conflict-free from BEHAVIOUR_FIRST_PASS on and still after the BEHAVIOUR_STEPS steps the GPU test
    runs; without it every path is still in conflict then."""
    import nfopp
    case = tc.behaviour_case()
    static, moving = tc.behaviour_fields(case)
    hp = orc.Hyper(**case["hyper"])
    B, N = len(case["starts"]), case["n_waypoints"]
    s = dict(traj=nfopp.straight_line_init(case["starts"], case["goals"], N), start=case["starts"], goal=case["goals"],
             lam=np.zeros((B, N + 1), F32), cm=np.zeros((B, N), F32), adam_m=np.zeros((B, N, 3), F32),
             adam_v=np.zeros((B, N, 3), F32), adam_step=0, step_count=0)
    hinv = orc.calculate_inv_hessian(N, 0.5)
    assert _conflicts(case, s["traj"]).all()
    for k in range(tc.BEHAVIOUR_STEPS):
        ref.planner_step(static, moving if with_moving else None, case["wp_time"], s, case["draws"][k], hp, hinv, case["reparam_freq"])
        if with_moving and k + 1 >= tc.BEHAVIOUR_FIRST_PASS:
            assert not _conflicts(case, s["traj"]).any(), k + 1
        if with_moving and k + 1 == tc.BEHAVIOUR_FIRST_PASS - 1:
            assert _conflicts(case, s["traj"]).any()
    if not with_moving:
        assert _conflicts(case, s["traj"]).all()


# ---- the library -----------------------------------------------------------------------------------------------------------------
ENTRIES = ("nfopp_track_field_eval_points", "nfopp_traj_track_overlay", "nfopp_traj_steps_moving")


def test_library_exports_the_entries():
    from nfopp import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.nfopp_abi_version() == 6 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.TrackFieldC) == 144     # 2 * 8 + 3 * 4 + 2 * 4 + 4 + 8 * 3 * 4 + 2 * 4, no padding
    assert (_lib.MODEL_ONF, _lib.MODEL_SDF, _lib.MODEL_HDF) == (0, 1, 2)


def _good_field(_lib):
    good = _lib.TrackFieldC()
    good.tracks_dev, good.m, good.k, good.stride, good.inv_dt, good.n_discs, good.gain = 4096, 2, 3, 2, 4.0, 1, 1.0
    return good


def _bad_fields(_lib):
    """[(field, dim)]: every field the entries refuse."""
    good = _good_field(_lib)

    def field(**changes):
        f = _lib.TrackFieldC.from_buffer_copy(good)
        for key, value in changes.items():
            setattr(f, key, value)
        return f

    offset = field()
    offset.disc[0][1] = 0.1
    bad = [(field(tracks_dev=None), 3), (field(m=-1), 3), (field(k=0), 3), (field(stride=1), 3), (field(n_discs=0), 3),
           (field(n_discs=9), 3), (offset, 2), (field(n_discs=2), 2), (field(), 4), (field(), 1),
           (field(m=1 << 15, k=1 << 15, stride=2), 3), (field(inv_dt=0.0), 3), (field(inv_dt=-1.0), 3)]
    for name in ("t0", "inv_dt", "margin", "gain"):
        bad += [(field(**{name: v}), 3) for v in (np.nan, np.inf, -np.inf)]
    return bad


def test_library_rejects_bad_arguments_without_a_device():
    """The argument checks come before any launch: they answer on a machine without a GPU too."""
    from nfopp import _lib
    lib = _lib.load()
    good = _good_field(_lib)
    A = 4096        # a dummy, 16-byte aligned address: a refused call reads and writes nothing
    for f, dim in _bad_fields(_lib):
        assert lib.nfopp_track_field_eval_points(f, A, A, 1, dim, A, None) == -1 and lib.nfopp_last_error()
        assert lib.nfopp_traj_track_overlay(f, A, A, 1, 4, dim, A, A, None, None) == -1
    assert lib.nfopp_track_field_eval_points(None, A, A, 1, 3, A, None) == -1
    assert lib.nfopp_track_field_eval_points(good, None, A, 1, 3, A, None) == -1
    assert lib.nfopp_track_field_eval_points(good, A, None, 1, 3, A, None) == -1       # null times
    assert lib.nfopp_track_field_eval_points(good, A, A, 1, 3, None, None) == -1
    assert lib.nfopp_track_field_eval_points(good, A, A, 1, 3, A + 4, None) == -1      # out4 not 16-byte aligned
    assert lib.nfopp_track_field_eval_points(good, A, A, -1, 3, A, None) == -1
    assert lib.nfopp_track_field_eval_points(good, A, A, 0x7fffffff * 256 + 1, 3, A, None) == -1
    assert lib.nfopp_traj_track_overlay(None, A, A, 1, 4, 3, A, A, None, None) == -1
    assert lib.nfopp_traj_track_overlay(good, None, A, 1, 4, 3, A, A, None, None) == -1
    assert lib.nfopp_traj_track_overlay(good, A, None, 1, 4, 3, A, A, None, None) == -1    # null waypoint times
    assert lib.nfopp_traj_track_overlay(good, A, A, 1, 4, 3, None, A, None, None) == -1
    assert lib.nfopp_traj_track_overlay(good, A, A, 1, 4, 3, A, None, None, None) == -1
    assert lib.nfopp_traj_track_overlay(good, A, A, 1, 4, 3, A, A + 8, None, None) == -1
    assert lib.nfopp_traj_track_overlay(good, A, A, 1, 1, 3, A, A, None, None) == -1       # fewer than 2 waypoints
    assert lib.nfopp_traj_track_overlay(good, A, A, -1, 4, 3, A, A, None, None) == -1
    assert lib.nfopp_traj_track_overlay(good, A, A, 1 << 31, 4, 3, A, A, None, None) == -1
    assert lib.nfopp_traj_track_overlay(good, A, A, 0x7fffffff, 258, 3, A, A, None, None) == -1   # beyond one launch
    # a set of no obstacles, n = 0 and batch = 0 launch nothing and succeed
    none = _lib.TrackFieldC.from_buffer_copy(good)
    none.m, none.tracks_dev = 0, None
    assert lib.nfopp_track_field_eval_points(none, A, A, 5, 3, A, None) == 0
    assert lib.nfopp_traj_track_overlay(none, A, A, 2, 4, 3, A, A, None, None) == 0
    assert lib.nfopp_track_field_eval_points(good, None, None, 0, 3, None, None) == 0
    assert lib.nfopp_traj_track_overlay(good, None, None, 0, 4, 3, None, None, None, None) == 0


def test_step_loop_rejects_bad_arguments_without_a_device():
    from nfopp import _lib
    lib = _lib.load()
    good = _good_field(_lib)
    A = 4096
    sdf = _lib.SdfFieldC()
    sdf.sd_dev, sdf.rows, sdf.cols, sdf.n_discs, sdf.inv_res, sdf.gain = A, 4, 4, 1, 1.0, 1.0
    hdf = _lib.HeadingFieldC()
    hp = _lib.TrajHyperC()
    sched = _lib.StepScheduleC(1e-2, 0.9, 0.9, 0, 0, 0, 0, 0, 3, 1)

    def buffers(dim=3, n=4, batch=1, out=A):
        return _lib.TrajBuffersC(A, A, A, A if dim == 3 else None, A if dim == 3 else None, A, A, A, out, A, A, None, None, batch, n,
                                 dim, 1, 0, 0)

    def call(kind=_lib.MODEL_SDF, model=ctypes.addressof(sdf), params=None, field=good, times=A, hyper=hp, buf=None, schedule=sched):
        return lib.nfopp_traj_steps_moving(kind, model, params, field, times, hyper, buf or buffers(), schedule, 2, None, None, None)

    for kind in (-1, 3):
        assert call(kind=kind) == -1
    assert call(model=None) == -1 and call(field=None) == -1 and call(times=None) == -1 and call(hyper=None) == -1
    assert lib.nfopp_traj_steps_moving(_lib.MODEL_SDF, ctypes.addressof(sdf), None, good, A, hp, None, sched, 2, None, None, None) == -1
    assert call(schedule=None) == -1
    assert call(kind=_lib.MODEL_ONF, model=ctypes.addressof(_lib.OnfConfigC()), params=None) == -1     # an ONF without parameters
    assert call(kind=_lib.MODEL_HDF, model=ctypes.addressof(hdf), buf=buffers(dim=2)) == -1              # a heading field with dim 2
    assert call(buf=buffers(n=1)) == -1 and call(buf=buffers(out=A + 4)) == -1 and call(buf=buffers(batch=1 << 31)) == -1
    for f, dim in _bad_fields(_lib):
        if dim in (2, 3):
            assert call(field=f, buf=buffers(dim=dim)) == -1
    # the schedule's own refusals still come before any launch
    assert call(schedule=_lib.StepScheduleC(1e-2, 0.9, 0.9, 0, 0, 0, 0, 0, 0, 1)) == -1
    assert call(schedule=_lib.StepScheduleC(1e-2, 0.9, 0.9, 0, 0, 0, 0, 0, 3, 0)) == -1       # injected draws without draws


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_checks_come_before_the_device():
    import torch

    import nfopp
    tracks = torch.zeros(3, 5, 2)
    ok = dict(dt=0.25, robot_radius=0.2)
    for kw in (dict(dt=0.25), dict(ok, discs=[(0, 0, 0.1)]), dict(dt=0.25, discs=[(0, 0, 0.1)] * 9), dict(dt=0.25, discs=[(0, 0, -1.0)]),
               dict(dt=0.25, discs=[(0.1, 0, 0.1)], dim=2), dict(dt=0.25, discs=[(0, 0, 0.1)] * 2, dim=2), dict(ok, dim=4),
               dict(ok, dt=0.0), dict(ok, dt=-1.0), dict(ok, dt=np.inf), dict(ok, dt=np.nan), dict(ok, t0=np.inf), dict(ok, margin=np.nan),
               dict(ok, gain=np.inf)):
        with pytest.raises((ValueError, TypeError)):
            nfopp.MovingObstacles(tracks, **kw)
    for bad in (torch.zeros(3, 5), torch.zeros(3, 0, 2), torch.zeros(3, 5, 1), torch.zeros(3, 5, 2, dtype=torch.float64),
                torch.zeros(5, 3, 2).transpose(0, 1)):
        with pytest.raises(ValueError):
            nfopp.MovingObstacles(bad, **ok)
    with pytest.raises(TypeError):
        nfopp.MovingObstacles(np.zeros((3, 5, 2), F32), **ok)
    with pytest.raises(ValueError):
        nfopp.MovingObstacles(tracks, radius=[0.1, 0.2], **ok)       # two radii for three tracks
    with pytest.raises(nfopp.NfoppError):
        nfopp.MovingObstacles(tracks, **ok)                          # everything in order but the device: there is no CPU path
