"""GPU: nfopp_path_time_profile / nfopp_path_time_sample (csrc/time_profile.hip) against the numpy restatement
(tests/time_profile_ref.py), bit for bit: profile, gear, summary, states and segment, at the sizes where the kernel takes
another path (one interior vertex, the wave boundary at N + 2 = 64 / 65 / 66, the 256-thread stride, several trips, the
longest path whose image fits one workgroup's LDS and the refusal one waypoint past it); then the Python interface and the
torch ops against the raw calls.

Measured on an MI355X: the whole file takes 4.0 s; the two longest-path cases take 0.06 s each."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
from nfopp import _lib, torch_ops  # noqa: E402

import time_profile_cases as tc  # noqa: E402
import time_profile_ref as tr  # noqa: E402

F32 = np.float32
LIMITS = nfopp.MotionLimits(tc.LIMITS.v_max, tc.LIMITS.a_max, tc.LIMITS.d_max, tc.LIMITS.a_lat, tc.LIMITS.w_max, np.pi / 3)
assert LIMITS.cos_cusp == tc.LIMITS.cos_cusp


def _dev(x, dtype=F32):
    return torch.tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda")


def _same_bits(got, want):
    got, want = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return np.array_equal(got.view(np.uint8), want.view(np.uint8)) or np.array_equal(got, want, equal_nan=True) and \
        np.array_equal(np.signbit(got), np.signbit(want))


def _timed(paths, limits=LIMITS, vs=None, vg=None):
    return nfopp.time_parametrize(_dev(paths[:, 1:-1]), _dev(paths[:, 0]), _dev(paths[:, -1]), limits,
                                  None if vs is None else _dev(vs), None if vg is None else _dev(vg))


def _instants(prof, count=61):
    """(t0, dt, count) from before the start to past the end of the slowest path."""
    total = np.nanmax(prof[:, -1, tr.SLOT_T])
    return -0.25, (total + 0.75) / (count - 1), count


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("b,n", tc.SIZES)
def test_profile_and_samples_equal_the_restatement_bit_for_bit(b, n, dim):
    paths, vs, vg = tc.batch(1000 * n + 10 * b + dim, b, n, dim)
    if dim == 3:
        assert min(tc.forward_margin(p) for p in paths) >= 1e-6
    prof, gear, summary = tr.profile_batch(paths, tc.LIMITS, vs, vg)
    got = _timed(paths, vs=vs, vg=vg)
    assert _same_bits(got.gear, gear)
    assert _same_bits(got.summary, summary), (got.summary.cpu().numpy(), summary)
    assert _same_bits(got.profile, prof), np.argwhere(got.profile.cpu().numpy() != prof)[:8]
    again = _timed(paths, vs=vs, vg=vg)                     # the same bits on a second run
    assert torch.equal(again.profile, got.profile) and torch.equal(again.gear, got.gear) and torch.equal(again.summary, got.summary)
    t0, dt, count = _instants(prof)
    states, segment = tr.sample_batch(paths, prof, gear, tc.LIMITS, t0, dt, count)
    got_states, got_segment = got.sample(dt, count, t0=t0, want_segment=True)
    assert _same_bits(got_segment, segment)
    assert _same_bits(got_states, states), np.argwhere(got_states.cpu().numpy() != states)[:8]
    assert torch.equal(got.sample(dt, count, t0=t0), got_states)
    # exactly at a vertex time of path 0: the segment that STARTS there
    t_mid = float(prof[0, (n + 1) // 2, tr.SLOT_T])
    states, segment = tr.sample_batch(paths, prof, gear, tc.LIMITS, t_mid, 1.0, 1)
    got_states, got_segment = got.sample(1.0, 1, t0=t_mid, want_segment=True)
    assert segment[0, 0] >= (n + 1) // 2 and _same_bits(got_segment, segment) and _same_bits(got_states, states)
    # more instants than one workgroup takes, on a fine grid
    if n == 62:
        states, segment = tr.sample_batch(paths, prof, gear, tc.LIMITS, 0.0, 0.01, 700)
        got_states, got_segment = got.sample(0.01, 700, want_segment=True)
        assert _same_bits(got_segment, segment) and _same_bits(got_states, states)


@pytest.mark.parametrize("dim,n", tc.LONGEST)
def test_the_longest_path_served_equals_the_restatement_and_one_waypoint_more_is_refused(dim, n):
    """N + 2 = 3032 (dim 3) / 3275 (dim 2): the largest LDS image the entry accepts, every thread 12 or 13 trips over the
    vertices.  Profile, gear, summary and samples bit for bit; at N + 1 the call answers "path too long" and writes nothing."""
    b = tc.LONGEST_B
    paths, vs, vg = tc.batch(tc.LONGEST_SEED, b, n, dim)
    assert tc.lds_bytes(n + 2, dim) <= 160 * 1024 < tc.lds_bytes(n + 3, dim)
    if dim == 3:
        assert min(tc.forward_margin(p) for p in paths) >= 1e-6
    prof, gear, summary = tr.profile_batch(paths, tc.LIMITS, vs, vg)
    assert (summary[:, tr.SUM_STATUS] != 4).all()
    got = _timed(paths, vs=vs, vg=vg)
    assert _same_bits(got.gear, gear)
    assert _same_bits(got.summary, summary), (got.summary.cpu().numpy(), summary)
    assert _same_bits(got.profile, prof), np.argwhere(got.profile.cpu().numpy() != prof)[:8]
    again = _timed(paths, vs=vs, vg=vg)
    assert torch.equal(again.profile, got.profile) and torch.equal(again.gear, got.gear) and torch.equal(again.summary, got.summary)
    # 61 instants from before the start to past the end, and 700 on a finer grid that ends past the slowest path's goal
    total = float(np.nanmax(prof[:, -1, tr.SLOT_T]))
    for t0, dt, count in (_instants(prof), (0.0, total / 650, 700)):
        states, segment = tr.sample_batch(paths, prof, gear, tc.LIMITS, t0, dt, count)
        got_states, got_segment = got.sample(dt, count, t0=t0, want_segment=True)
        assert segment.max() == n + 1 and len(np.unique(segment)) > count // 2      # all along the path, and past its end
        assert _same_bits(got_segment, segment)
        assert _same_bits(got_states, states), np.argwhere(got_states.cpu().numpy() != states)[:8]
    # one waypoint more: refused before anything is launched, the poisoned outputs stay as they were
    lib, L = _lib.load(), _lib
    traj = torch.zeros(1, n + 1, dim, device="cuda")
    start, goal = torch.zeros(1, dim, device="cuda"), torch.ones(1, dim, device="cuda")
    profile_dev = torch.full((1, n + 3, 4), -7.0, dtype=torch.float64, device="cuda")
    gear_dev = torch.full((1, n + 2), -7, dtype=torch.int8, device="cuda")
    summary_dev = torch.full((1, 4), -7.0, dtype=torch.float64, device="cuda")
    rc = lib.nfopp_path_time_profile(L.ptr(traj), L.ptr(start), L.ptr(goal), 1, n + 1, dim, LIMITS.to_c(), None, None,
                                     L.ptr(profile_dev, torch.float64), L.ptr(gear_dev, torch.int8), L.ptr(summary_dev, torch.float64),
                                     L.stream_ptr())
    assert rc == -1 and "path too long" in lib.nfopp_last_error().decode()
    torch.cuda.synchronize()
    assert (profile_dev == -7.0).all() and (gear_dev == -7).all() and (summary_dev == -7.0).all()


def test_out_of_range_rows_are_nan_and_the_others_untouched():
    for dim in (2, 3):
        cases = tc.status_cases(dim)
        paths = np.stack([c[0] for c in cases])
        vs, vg = np.array([c[1] for c in cases], F32), np.array([c[2] for c in cases], F32)
        rest = tr.Limits(2.0, 1.0, 1.0)
        prof, gear, summary = tr.profile_batch(paths, rest, vs, vg)
        assert summary[:, tr.SUM_STATUS].tolist() == [c[3] for c in cases]
        got = _timed(paths, nfopp.MotionLimits(2.0, 1.0, cusp_angle=None), vs, vg)
        assert _same_bits(got.profile, prof) and _same_bits(got.gear, gear) and _same_bits(got.summary, summary)
        bad = summary[:, tr.SUM_STATUS] == 4
        assert bad.any() and np.isnan(got.profile.cpu().numpy()[bad]).all() and np.isfinite(got.profile.cpu().numpy()[~bad]).all()
        states, segment = got.sample(0.1, 8, t0=-0.1, want_segment=True)
        want_states, want_segment = tr.sample_batch(paths, prof, gear, rest, -0.1, 0.1, 8)
        assert _same_bits(states, want_states) and _same_bits(segment, want_segment)
        assert np.isnan(states.cpu().numpy()[bad]).all() and (segment.cpu().numpy()[bad] == -1).all()


def test_null_gear_and_null_segment_and_the_instants_at_the_edges():
    path = tc.straight([0.0, 1.0, 1.0, 2.0], dim=3)[None]      # segment 1 has zero duration
    path[0, :, 2] = np.pi                                       # driven backwards
    rest = tr.Limits(2.0, 1.0, 1.0)
    lim = nfopp.MotionLimits(2.0, 1.0, cusp_angle=None)
    prof, gear, summary = tr.profile_batch(path, rest)
    assert prof[0, 1, tr.SLOT_T] == prof[0, 2, tr.SLOT_T] and gear[0].tolist() == [-1, -1, -1]
    traj, start, goal = _dev(path[:, 1:-1]), _dev(path[:, 0]), _dev(path[:, -1])
    lib, L = _lib.load(), _lib
    profile_dev, summary_dev = torch.empty(1, 4, 4, dtype=torch.float64, device="cuda"), torch.empty(1, 4, dtype=torch.float64, device="cuda")
    L.check(lib.nfopp_path_time_profile(L.ptr(traj), L.ptr(start), L.ptr(goal), 1, 2, 3, lim.to_c(), None, None,
                                        L.ptr(profile_dev, torch.float64), None, L.ptr(summary_dev, torch.float64), L.stream_ptr()))
    assert _same_bits(profile_dev, prof) and _same_bits(summary_dev, summary)
    t_mid, total = float(prof[0, 1, tr.SLOT_T]), float(prof[0, -1, tr.SLOT_T])
    for t0, dt, want_seg in ((-1.0, 0.5, [-1, -1]), (total, 1.0, [3, 3]), (t_mid, total - t_mid, [2, 3]),
                             (t_mid - 2.0 ** -32, 2.0 ** -32, [0, 2])):
        states = torch.empty(1, 2, 4, dtype=torch.float32, device="cuda")
        L.check(lib.nfopp_path_time_sample(L.ptr(traj), L.ptr(start), L.ptr(goal), 1, 2, 3, lim.to_c(),
                                           L.ptr(profile_dev, torch.float64), None, t0, dt, 2, L.ptr(states), None, L.stream_ptr()))
        want, seg = tr.sample_batch(path, prof, None, rest, t0, dt, 2)            # null gear: forward
        assert seg[0].tolist() == want_seg and _same_bits(states, want), (t0, states.cpu().numpy(), want)
        segment = torch.empty(1, 2, dtype=torch.int32, device="cuda")
        L.check(lib.nfopp_path_time_sample(L.ptr(traj), L.ptr(start), L.ptr(goal), 1, 2, 3, lim.to_c(),
                                           L.ptr(profile_dev, torch.float64), None, t0, dt, 2, L.ptr(states),
                                           L.ptr(segment, torch.int32), L.stream_ptr()))
        assert segment[0].tolist() == want_seg and _same_bits(states, want), (t0, segment)
        assert (want[..., 3] >= 0).all()
    before = tr.sample_batch(path, prof, gear, rest, -1.0, 0.5, 2)[0]
    assert np.array_equal(before[0, 0], path[0, 0].tolist() + [0.0])             # the start pose, at rest
    timed = nfopp.TimedPaths(traj, start, goal, lim, profile_dev, _dev(gear, np.int8), summary_dev)
    assert _same_bits(timed.sample(0.25, 12), tr.sample_batch(path, prof, gear, rest, 0.0, 0.25, 12)[0])
    assert (timed.sample(0.25, 12).cpu().numpy()[..., 3] <= 0).all()              # signed speed: reverse gear
    assert timed.sample(0.25, 0).shape == (1, 0, 4)


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


def test_batch_planner_and_torch_ops_equal_the_raw_calls():
    bp = _planner(5, 40)
    eng = bp.engine
    vs = torch.full((5,), 0.25, device="cuda")
    timed = bp.timed_paths(LIMITS, v_start=vs)
    raw = nfopp.time_parametrize(eng.traj.view(5, 40, 3), eng.start, eng.goal, LIMITS, v_start=vs)
    for name in ("profile", "gear", "summary"):
        assert torch.equal(getattr(timed, name), getattr(raw, name)), name
    assert timed.profile.shape == (5, 42, 4) and timed.gear.shape == (5, 41) and timed.summary.shape == (5, 4)
    # a TimedPaths holds its own copy of the poses: it stays what it was when the planner moves on
    before = timed.sample(0.05, 60)
    bp.step(n=2)
    assert not torch.equal(timed.traj, eng.traj.view(5, 40, 3)) and torch.equal(timed.sample(0.05, 60), before)
    timed = bp.timed_paths(LIMITS, v_start=vs)
    raw = nfopp.time_parametrize(eng.traj.view(5, 40, 3), eng.start, eng.goal, LIMITS, v_start=vs)
    assert torch.equal(timed.profile, raw.profile)
    with pytest.raises(ValueError, match="speed"):
        bp.timed_paths(LIMITS, v_start=vs[:4])
    assert torch.equal(bp.timed_paths(LIMITS, v_start=0.25).profile, raw.profile)
    paths = bp.get_paths()
    prof, gear, summary = tr.profile_batch(paths, tc.LIMITS, np.full(5, 0.25, F32), None)
    assert np.array_equal(timed.summary.cpu().numpy()[:, tr.SUM_LENGTH], summary[:, tr.SUM_LENGTH])     # integer arc length
    ops = torch_ops.load()
    lim = torch_ops.limits_list(LIMITS)
    o_prof, o_gear, o_sum = ops.path_time_profile(eng.traj.view(5, 40, 3), eng.start, eng.goal, lim, vs, None)
    assert torch.equal(o_prof, raw.profile) and torch.equal(o_gear, raw.gear) and torch.equal(o_sum, raw.summary)
    states, segment = raw.sample(0.05, 90, t0=-0.1, want_segment=True)
    o_states, o_segment = ops.path_time_sample(eng.traj.view(5, 40, 3), eng.start, eng.goal, lim, o_prof, o_gear, -0.1, 0.05, 90)
    assert torch.equal(o_states, states) and torch.equal(o_segment, segment)
    with pytest.raises(RuntimeError, match="must be"):
        ops.path_time_sample(eng.traj.view(5, 40, 3), eng.start, eng.goal, lim, o_prof.float(), o_gear, 0.0, 0.05, 4)
    with pytest.raises(RuntimeError, match="6 doubles"):
        ops.path_time_profile(eng.traj.view(5, 40, 3), eng.start, eng.goal, lim[:5], None, None)


def test_best_times_the_best_paths():
    bp = _planner(4, 24, seed=4)
    rng = np.random.default_rng(0)
    obstacles = rng.uniform(5.0, 6.0, (16, 2)).astype(F32)          # far from every path: all collision-free
    bp.evaluate(nfopp.DeviceCircleChecker(obstacles, 0.1))
    bp.step(n=2)                                                    # the current paths move on, the best stay
    best = bp.best_paths()
    assert not np.array_equal(best, bp.get_paths())
    timed = bp.timed_paths(LIMITS, best=True)
    prof, gear, summary = tr.profile_batch(best, tc.LIMITS)
    assert np.array_equal(timed.profile.cpu().numpy()[..., tr.SLOT_S], prof[..., tr.SLOT_S])
    raw = _timed(best)
    assert torch.equal(timed.profile, raw.profile) and torch.equal(timed.summary, raw.summary)
    assert not torch.equal(timed.profile, bp.timed_paths(LIMITS).profile)


def test_drop_in_planner_returns_monotone_stamps_that_end_at_the_total():
    A = nfopp.AttributeDict
    z = load_golden("g9_full_steps.npz")
    params = A(device="cuda", trajectory_length=100,
               collision_model=A(mean=0, sigma=1, use_cos=True, bias=True, use_normal_init=True, angle_encoding=True, name="ONF"),
               trajectory_initializer=A(name="TrajectoryInitializer", resolution=0.05),
               collision_optimizer=A(lr=5e-2, betas=(0.9, 0.9)), trajectory_optimizer=A(lr=1e-2, betas=(0.9, 0.9)),
               planner=A(name="ConstrainedNERFOptPlanner", trajectory_random_offset=0.02, collision_weight=1,
                         velocity_hessian_weight=0.5, random_field_points=10, init_collision_iteration=0,
                         constraint_deltas_weight=20, multipliers_lr=0.1, init_collision_points=100,
                         reparametrize_trajectory_freq=10, optimize_collision_model_freq=1, angle_weight=0.5,
                         angle_offset=0.3, boundary_weight=1, collision_multipliers_lr=1e-3))
    torch.random.manual_seed(100)
    np.random.seed(400)
    cc = nfopp.CircleDirectedCollisionChecker(0.3, (0, 3, 0, 3))
    cc.update_obstacle_points(z["obstacles"])
    cc.update_boundaries(tuple(z["bounds"]))
    planner = nfopp.PlannerFactory.make_constrained_onf_planner(cc, params)
    planner.init(z["start"], z["goal"], tuple(z["bounds"]))
    planner.step(3)
    rows = planner.get_timed_path(LIMITS, 0.1)
    eng = planner._engine
    total = float(nfopp.time_parametrize(eng.traj.view(1, eng.N, eng.D), eng.start, eng.goal, LIMITS).summary[0, 0])
    assert rows.shape[1] == 1 + eng.D + 1 and (np.diff(rows[:, 0]) > 0).all()
    assert rows[0, 0] == 0.0 and rows[-1, 0] == total
    path = planner.get_path()
    assert np.array_equal(rows[0, 1:1 + eng.D], path[0].astype(np.float64)) and np.array_equal(rows[-1, 1:1 + eng.D], path[-1].astype(np.float64))
    assert rows[0, -1] == 0.0 and rows[-1, -1] == 0.0 and (np.abs(rows[:, -1]) <= LIMITS.v_max).all()
    # a step that divides the total exactly: the last grid stamp stays below the total, which is not repeated
    rows = planner.get_timed_path(LIMITS, total / 8)
    assert len(rows) == 9 and (np.diff(rows[:, 0]) > 0).all() and rows[-1, 0] == total
    moving = planner.get_timed_path(LIMITS, 0.1, v_start=0.05)
    assert abs(moving[0, -1]) == np.float32(0.05)
    with pytest.raises(ValueError, match="too fast"):
        planner.get_timed_path(LIMITS, 0.1, v_start=50.0)
