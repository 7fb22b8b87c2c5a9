"""The tracks, robots, poses and times of the moving-obstacle tests (tests/test_track_field_cpu.py,
tests/test_gpu_track_field.py).  Everything is generated from fixed seeds; nothing here needs a device."""
import numpy as np

import sdf_cases as sc
import track_field_ref as ref

F32 = np.float32

# The frame of every case: a floor of 6 m x 4 m; the time grid starts at T0 with step DT, both exact in fp32, so an instant
# written as T0 + n * DT is that instant to the bit.
FLOOR = (0.0, 6.0, 0.0, 4.0)
T0, DT = 1.0, 0.25

CENTRED = [(0.0, 0.0, 0.2)]
THREE_DISCS = sc.THREE_DISCS


def random_tracks(m, k, stride, seed, nan_track=None):
    """fp32 [m, k, stride]: constant-velocity tracks over the floor with a little noise on every instant; the columns past y
    hold NaN (they are never read).  `nan_track`: that track gets a NaN x at its middle instant."""
    rng = np.random.default_rng(seed)
    p0 = np.stack([rng.uniform(FLOOR[0], FLOOR[1], m), rng.uniform(FLOOR[2], FLOOR[3], m)], 1)
    v = rng.uniform(-1.0, 1.0, (m, 2))
    t = np.arange(k) * DT
    xy = p0[:, None, :] + v[:, None, :] * t[None, :, None] + rng.normal(0, 0.02, (m, k, 2))
    tracks = np.full((m, k, stride), np.nan, F32)
    tracks[:, :, :2] = xy
    if nan_track is not None:
        tracks[nan_track, k // 2, 0] = np.nan
    return tracks


def random_radii(m, seed):
    return np.random.default_rng(seed).uniform(0.05, 0.4, m).astype(F32)


def t_end(k):
    return T0 + (k - 1) * DT


def special_times(k):
    """Times at which the index is delicate: before T0, at T0, exactly at an inner instant, at the last instant, after it, far
    on either side, and one float32 step to either side of the first and of the last instant."""
    last = F32(t_end(k))
    fixed = [T0 - 0.6, T0, T0 + (k // 2) * DT, last, last + 0.4, -1e30, 1e30, np.nextafter(F32(T0), F32(-np.inf)),
             np.nextafter(F32(T0), F32(np.inf)), np.nextafter(last, F32(-np.inf)), np.nextafter(last, F32(np.inf))]
    return np.asarray(fixed, F32)


def random_points(count, dim, k, seed):
    """(poses fp32 [count, dim], times fp32 [count]): poses over the floor grown by 0.5 m, times over the track grid grown by
    two steps on either side, the special times first (as many as fit)."""
    rng = np.random.default_rng(seed)
    cols = [rng.uniform(FLOOR[0] - 0.5, FLOOR[1] + 0.5, count), rng.uniform(FLOOR[2] - 0.5, FLOOR[3] + 0.5, count),
            rng.uniform(-np.pi, np.pi, count)]
    times = rng.uniform(T0 - 2 * DT, t_end(k) + 2 * DT, count).astype(F32)
    sp = special_times(k)[:count]
    times[:len(sp)] = sp
    return np.stack(cols[:dim], 1).astype(F32), times


def bad_points(dim):
    """(poses, times): every pose component and the time set in turn to NaN, +inf and -inf -- samples that read no track."""
    poses, times = [], []
    for bad in (np.nan, np.inf, -np.inf):
        for comp in range(dim + 1):
            p = [2.9, 2.1, 0.4, T0 + 0.3]
            p[comp if comp < dim else 3] = bad
            poses.append(p[:dim])
            times.append(p[3])
    return np.asarray(poses, F32), np.asarray(times, F32)


def base_rows(track_rows, seed):
    """Rows to beat for the given track rows [P, 4], cycling through: logit -inf, +inf, NaN, a finite logit below the track
    row's, one above it, and the track row's own logit (a tie: the row stays).  The other three columns hold recognisable
    finite numbers."""
    rng = np.random.default_rng(seed)
    P = len(track_rows)
    base = rng.uniform(-3.0, 3.0, (P, 4)).astype(F32)
    logit = np.where(np.isfinite(track_rows[:, 0]), track_rows[:, 0], F32(0)).astype(F32)
    kinds = np.arange(P) % 6
    base[:, 0] = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3, kinds == 4],
                           [-np.inf, np.inf, np.nan, logit - F32(1.5), logit + F32(1.5)], logit).astype(F32)
    return base


# ---- explicit mode ------------------------------------------------------------------------------------------------------------------
POINT_COUNTS = (1, 63, 64, 65, 257)
TRACK_COUNTS = (1, 2, 65)
INSTANT_COUNTS = (1, 2, 3, 130)
STRIDES = (2, 4, 3)      # 3: x and y cannot come in one 8-byte load, the kernel's other fetch


def explicit_case(m, k, stride, count, dim):
    """-> (field, tracks fp32 [m, k, stride], radius fp32 [m], poses, times): one explicit-mode case; with two tracks or more
    the second has a NaN coordinate, and from 64 poses on the last ones are the non-finite samples."""
    seed = 1000 * m + 10 * k + stride
    tracks = random_tracks(m, k, stride, seed, nan_track=1 if m >= 2 else None)
    radius = random_radii(m, seed + 1)
    poses, times = random_points(count, dim, k, seed + count)
    if count >= 64:
        bp, bt = bad_points(dim)
        poses[-len(bp):], times[-len(bt):] = bp, bt
    discs = CENTRED
    return ref.make_field(tracks, DT, T0, radius, discs, margin=0.05, gain=10.0), tracks, radius, poses, times


def coverage_case():
    """The explicit case the CPU test counts branches on: M = 65, K = 130, 257 poses."""
    return explicit_case(65, 130, 2, 257, 3)


# ---- the hand cases -------------------------------------------------------------------------------------------------------------------
def standing_case():
    """A standing track (K = 1) (0.75, 1.0) from a centred disc: dist = 1.25 exactly.  -> (field, pose [1, 3], time [1], R)."""
    tracks = np.asarray([[[2.0 - 0.75, 1.5 - 1.0]]], F32)
    field = ref.make_field(tracks, DT, T0, 0.25, [(0.0, 0.0, 0.5)], margin=0.125, gain=2.0)
    return field, np.asarray([[2.0, 1.5, 0.3]], F32), np.asarray([7.0], F32), 0.875


def tie_case():
    """Two standing tracks mirrored about a centred disc at the origin: equal penetrations, opposite normals.  The first wins."""
    tracks = np.asarray([[[1.0, 0.0]], [[-1.0, 0.0]]], F32)
    return tracks, np.zeros((1, 3), F32), np.asarray([T0], F32)


# ---- offset discs: held against float64 -----------------------------------------------------------------------------------------
# name -> (tracks, radius, discs, margin, gain, poses, times).  The share of poses at which the float32 and the float64
# restatement take a different disc, track or interval may be at most 2 % (tests/test_track_field_cpu.py asserts it).
def _f64_case(m, k, discs, margin, gain, count, seed):
    tracks = random_tracks(m, k, 2, seed)
    poses, times = random_points(count, 3, k, seed + 1)
    times[:len(special_times(k))] = np.random.default_rng(seed + 2).uniform(T0, t_end(k), len(special_times(k))).astype(F32)
    return tracks, random_radii(m, seed + 3), discs, margin, gain, poses, times


F64_CASES = {
    "three_discs": _f64_case(8, 16, THREE_DISCS, 0.05, 10.0, 2048, 31),
    "box_robot": _f64_case(33, 40, sc._box_robot(), 0.0, 4.0, 1000, 32),
}
MAX_EXCLUDED_SHARE = 0.02


def f64_field(name):
    tracks, radius, discs, margin, gain, _, _ = F64_CASES[name]
    return ref.make_field(tracks, DT, T0, radius, discs, margin, gain)


# ---- trajectory mode --------------------------------------------------------------------------------------------------------------
TRAJ_SHAPES = sc.TRAJ_SHAPES
TRAJ_GRID = sc.FIELD_GRIDS["37x53"]      # the static map behind the overlay: x in -1.3 .. 4.0, y in 0.7 .. 4.4


def traj_tracks(m=9, k=24, seed=41):
    """Tracks over the static map's box, so that the overlay wins a good share of the rows."""
    rng = np.random.default_rng(seed)
    b = TRAJ_GRID.boundaries
    p0 = np.stack([rng.uniform(b[0], b[1], m), rng.uniform(b[2], b[3], m)], 1)
    v = rng.uniform(-0.5, 0.5, (m, 2))
    t = np.arange(k) * DT
    return (p0[:, None, :] + v[:, None, :] * t[None, :, None]).astype(F32)


def waypoint_times(batch, n, k=24, seed=42):
    """fp32 [batch, n]: increasing times per trajectory that start before the track grid and end behind it."""
    rng = np.random.default_rng(seed)
    steps = rng.uniform(0.5, 1.5, (batch, n))
    span = t_end(k) - T0 + 4 * DT
    return (T0 - 2 * DT + span * np.cumsum(steps, 1) / steps.sum(1, keepdims=True)).astype(F32)


# ---- behaviour: a crossing vehicle ---------------------------------------------------------------------------------------------
BEHAVIOUR_STEPS = 100       # what the GPU test runs
BEHAVIOUR_FIRST_PASS = 24   # the first step from which every path is conflict-free at every later step the restated pipeline
                            # runs: found with the first choice of radii, margin (0.1), gain (10) and sdf_cases.behaviour_case's weights


def behaviour_case():
    """An obstacle-free 13 m x 4 m map at 0.25 m; eight SE(2) robots drive +x at 0.3 m/s along straight seeds of 32 waypoints,
    staggered in x and 0.15 m apart in y; waypoint i is reached at T0 + (i + 1) * dt with dt = 0.5 s, so the paths' vertices
    (start, waypoints, goal) lie on the track grid of 34 instants.  One disc obstacle drives (-0.3, +0.1) m/s and meets robot
    b head-on at t = 3 + 1.5 b seconds, 0.1 m to the left of the robot's line: every seed is in conflict.
    -> dict(grid, discs, margin, gain, hyper, starts, goals, n_waypoints, reparam_freq, draws, dt, t0, wp_time, tracks,
            robot_radius, obstacle_radius, track_margin, track_gain)."""
    grid = sc.make_grid(np.zeros((16, 52), np.uint8), (0.0, 0.0), 0.25)
    n, dt, t0, speed = 32, 0.5, 0.0, 0.3
    b = np.arange(8)
    meet = 3.0 + 1.5 * b
    origin = np.asarray([9.0, 1.0])
    velocity = np.asarray([-0.3, 0.1])
    ys = origin[1] + velocity[1] * meet - 0.1
    xs = origin[0] + velocity[0] * meet - speed * meet
    length = speed * dt * (n + 1)
    zeros = np.zeros(8)
    starts = np.stack([xs, ys, zeros], 1).astype(F32)
    goals = np.stack([xs + length, ys, zeros], 1).astype(F32)
    instants = t0 + dt * np.arange(n + 2)
    tracks = (origin[None, None, :] + velocity[None, None, :] * instants[None, :, None]).astype(F32)
    wp_time = np.broadcast_to(instants[1:-1].astype(F32), (8, n)).copy()
    hyper = dict(collision_weight=20.0, collision_beta=2.0, direction_delta_weight=1.0, lr=1e-2, bounds=grid.boundaries)
    draws = np.random.default_rng(9).uniform(0, 1, (BEHAVIOUR_STEPS, 8, n - 1)).astype(F32)
    return dict(grid=grid, discs=[(0.0, 0.0, 0.15)], margin=0.0, gain=10.0, hyper=hyper, starts=starts, goals=goals, n_waypoints=n,
                reparam_freq=10, draws=draws, dt=dt, t0=t0, wp_time=wp_time, tracks=tracks, robot_radius=0.15,
                obstacle_radius=0.15, track_margin=0.1, track_gain=10.0)


def behaviour_fields(case):
    """-> (sdf_ref field of the static map, track_field_ref field of the obstacle) of a behaviour case."""
    static = sc.field_of(case["grid"], case["discs"], case["margin"], case["gain"])
    moving = ref.make_field(case["tracks"], case["dt"], case["t0"], case["obstacle_radius"], [(0.0, 0.0, case["robot_radius"])],
                            case["track_margin"], case["track_gain"])
    return static, moving


def behaviour_robot_tracks(case, traj):
    """traj fp32 [8, n, 3] -> fp32 [8, n + 2, 2]: the robots' positions at the instants of the track grid."""
    return np.concatenate([case["starts"][:, None, :2], np.asarray(traj, F32)[:, :, :2], case["goals"][:, None, :2]], 1)
