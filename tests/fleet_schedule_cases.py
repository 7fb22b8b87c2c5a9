"""Fleets for the start-delay scheduling tests (tests/test_fleet_schedule_cpu.py on the restatement,
tests/test_gpu_fleet_schedule.py on the device).  A case is a dict(tracks [B, K, S], max_delay, radius [B], margin, obstacles
[M, K + max_delay, S] or None, obstacle_radius [M] or None, order [B] int32 or None); hand cases are on dyadic coordinates and
carry `expect`: exact delays and statuses.

Families: "circle" -- B robots evenly spaced on a circle drive straight through the centre region to the point opposite,
rotated by half a spacing so that no goal is anyone's start; every robot conflicts at delay 0 and delays resolve most of it.
"crowded" -- random starts and goals on a small square; more than half of such a fleet stays unresolved, which makes it the
family for the unresolved status, not the main one."""
import numpy as np

import fleet_schedule_ref as fr

F32 = np.float32


def case(tracks, max_delay, radius=0.5, margin=0.0, obstacles=None, obstacle_radius=None, order=None, **expect):
    tracks = np.asarray(tracks, F32)
    radius = np.broadcast_to(np.asarray(radius, F32), (len(tracks),)).copy()
    if obstacles is not None:
        obstacles = np.asarray(obstacles, F32)
        obstacle_radius = np.broadcast_to(np.asarray(0.0 if obstacle_radius is None else obstacle_radius, F32), (len(obstacles),)).copy()
    if order is not None:
        order = np.asarray(order, np.int32)
    return dict(tracks=tracks, max_delay=int(max_delay), radius=radius, margin=float(margin), obstacles=obstacles,
                obstacle_radius=obstacle_radius, order=order, expect=expect)


def kwargs(c):
    """The arguments of fleet_schedule_ref.shift_masks for case `c`."""
    return dict(max_delay=c["max_delay"], radius=c["radius"], margin=c["margin"], obstacles=c["obstacles"],
                obstacle_radius=c["obstacle_radius"])


def solve(c):
    """-> (masks, schedule) of the restatement."""
    m = fr.shift_masks(c["tracks"], **kwargs(c))
    return m, fr.assign(m, c["order"])


def polyline_track(points, k, step=1.0):
    """[k, 2] fp32: from points[0] along the polyline at `step` metres per grid step, then parked at its end."""
    pts = np.asarray(points, np.float64)
    seg = np.linalg.norm(np.diff(pts, axis=0), axis=1)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    s = np.minimum(np.arange(k) * step, cum[-1])
    out = np.zeros((k, 2))
    for d in range(2):
        out[:, d] = np.interp(s, cum, pts[:, d])
    return out.astype(F32)


def hand_cases():
    out = {}
    # head-on along y = 0 towards the junction (4, 0), where each turns off to its own side.  R = 1.  Together they meet at
    # the junction; one step late, robot 1 cuts the corner robot 0 is leaving (closest 1 / sqrt 2); two steps late it is clear
    out["head_on_junction"] = case([polyline_track([(0, 0), (4, 0), (4, 4)], 12), polyline_track([(8, 0), (4, 0), (4, -4)], 12)], 7,
                                   delay=[0, 2], status=[0, 0], forbidden=[0, 3])
    # a crossing at (5, 0), R = 1: delayed by q the closest approach is q / sqrt 2 -- 1 is not enough, 2 is
    k = np.arange(12.0)
    cross = [np.stack([k, 0 * k], -1), np.stack([5 + 0 * k, k - 5], -1)]
    out["right_angle"] = case(cross, 3, delay=[0, 2], status=[0, 0], forbidden=[0, 3])
    # the same fleet with the crossing robot first: now the other one waits
    out["right_angle_reordered"] = case(cross, 3, order=[1, 0], delay=[2, 0], status=[0, 0], forbidden=[3, 0])
    # robot 0 parks on robot 1's start at instant 4; robot 1 crawls away at 1/8 m per step and is still inside R = 1 then, for
    # every delay: unresolved whatever D is
    slow = np.stack([4 + 0 * k, k / 8], -1)
    for md in (0, 5, 63):
        out["parked_on_start_%d" % md] = case([polyline_track([(0, 0), (4, 0)], 12), slow], md, delay=[0, -1],
                                              status=[0, fr.STATUS_UNRESOLVED], forbidden=[0, (1 << (md + 1)) - 1])
    # K = 1: a robot is a point.  0 and 1 overlap (for every shift: only the last-instant term can say so at r = 0), 2 is clear
    out["single_instant"] = case([[(0, 0)], [(0.5, 0)], [(3, 0)]], 3, delay=[0, -1, 0], status=[0, fr.STATUS_UNRESOLVED, 0],
                                 forbidden=[0, 15, 0])
    # an obstacle walks down x = 0 at 1 m per step and is within R = 1.25 of the robot's start (0, 0) during instants 3 .. 5
    # only.  The robot leaves along y = 0 at 1 m per step: delayed by 0 .. 2 it is gone in time, from 3 on it is still there
    kk = np.arange(8.0)
    ko = np.arange(8.0 + 5)
    out["obstacle_at_start"] = case([np.stack([kk, 0 * kk], -1)], 5, obstacles=[np.stack([0 * ko, ko - 4], -1)], obstacle_radius=0.75,
                                    delay=[0], status=[0], forbidden=[0b111000], base=[0b111000])
    # a second obstacle stands 1 m off the lane at x = 2 until instant 2 and then jumps away: only the undelayed robot meets it
    gate = np.stack([2 + 0 * ko, np.where(ko <= 2, 1.0, 4.0)], -1)
    out["obstacle_gate"] = case([np.stack([kk, 0 * kk], -1)], 5, obstacles=[np.stack([0 * ko, ko - 4], -1), gate], obstacle_radius=0.75,
                                delay=[1], status=[0], forbidden=[0b111001], base=[0b111001])
    return out


def lanes(closer):
    """Two robots side by side on parallel lanes, R = 1 apart exactly (no bit of the pair mask may be set: the test is strict)
    or one fp32 step closer (every bit is set: whatever the shift, they end parked side by side)."""
    k = np.arange(11.0)
    y = float(np.nextafter(F32(1.0), F32(0.0))) if closer else 1.0
    return case([np.stack([k, 0 * k], -1), np.stack([k, y + 0 * k], -1)], 63)


def circle(b, k, max_delay, rho=None, step=0.25, radius=0.0625, margin=0.0625, seed=0, jitter=2.0 ** -10):
    """B robots evenly spaced on a circle of radius rho, starts jittered in fp32; each drives straight at `step` metres per
    grid step to the point opposite its start, rotated by half a spacing, then parks.  rho None: b / 8, which keeps the
    spacing of 16 robots on a 2 m circle (the drive then takes b grid steps at the default step)."""
    rho = b / 8.0 if rho is None else rho
    rng = np.random.default_rng(seed)
    th = 2.0 * np.pi * np.arange(b) / b
    starts = (rho * np.stack([np.cos(th), np.sin(th)], -1) + rng.uniform(-jitter, jitter, (b, 2))).astype(F32)
    tg = th + np.pi + np.pi / b
    goals = (rho * np.stack([np.cos(tg), np.sin(tg)], -1)).astype(F32)
    tracks = np.stack([polyline_track([s, g], k, step) for s, g in zip(starts.astype(np.float64), goals.astype(np.float64))])
    return case(tracks, max_delay, radius=radius, margin=margin)


def crowded(b, k, max_delay, side=2.0, step=0.25, radius=0.125, seed=0):
    """Random starts and goals on a square of `side` metres."""
    rng = np.random.default_rng(seed)
    starts, goals = rng.uniform(0, side, (b, 2)), rng.uniform(0, side, (b, 2))
    tracks = np.stack([polyline_track([s, g], k, step) for s, g in zip(starts, goals)])
    return case(tracks, max_delay, radius=radius)


def crossing_obstacles(c, m, seed=0, radius=0.125, extent=2.5):
    """The case with M obstacles that cross the floor on straight lines at constant speed, over K + max_delay instants."""
    rng = np.random.default_rng(seed + 1000)
    n = c["tracks"].shape[1] + c["max_delay"]
    p0 = rng.uniform(-extent, extent, (m, 2))
    p1 = rng.uniform(-extent, extent, (m, 2))
    lam = (np.arange(n) / max(n - 1, 1))[None, :, None]
    obstacles = (p0[:, None] * (1 - lam) + p1[:, None] * lam).astype(F32)
    return dict(c, obstacles=obstacles, obstacle_radius=np.full(m, radius, F32))


def with_stride(c, stride, seed=0):
    """The case with rows of `stride` floats: columns 2.. hold junk (NaN among it) that must not be read."""
    rng = np.random.default_rng(seed)

    def widen(t):
        if t is None or stride == 2:
            return t
        junk = rng.uniform(-1e6, 1e6, t.shape[:2] + (stride - 2,)).astype(F32)
        junk[..., 0][rng.uniform(size=junk.shape[:2]) < 0.2] = np.nan
        return np.concatenate([t[:, :, :2], junk], -1)
    return dict(c, tracks=widen(c["tracks"]), obstacles=widen(c["obstacles"]))


def with_bad(c, robots=(), obstacles=(), radius_robot=None):
    """The case with a NaN / inf planted in the given robots and obstacles (and a NaN radius for robot `radius_robot`)."""
    c = dict(c, tracks=c["tracks"].copy(), radius=c["radius"].copy())
    for n, i in enumerate(robots):
        c["tracks"][i, (n * 7) % c["tracks"].shape[1], n % 2] = np.nan if n % 2 == 0 else np.inf
    if radius_robot is not None:
        c["radius"][radius_robot] = np.nan
    if len(obstacles):
        c["obstacles"] = c["obstacles"].copy()
        for n, j in enumerate(obstacles):
            c["obstacles"][j, -1 - n, 1] = -np.inf
    return c


def orders(b, seed=0):
    """identity (None), a random permutation, and an order holding a repeat, a -1 and a value >= B."""
    rng = np.random.default_rng(seed + 7)
    perm = rng.permutation(b).astype(np.int32)
    odd = perm.copy()
    if b >= 1:
        odd[0] = -1
    if b >= 2:
        odd[1] = b + 3
    if b >= 4:
        odd[3] = odd[2]
    return dict(identity=None, permutation=perm, odd=odd)


# B x K x max_delay of the device comparison: the smallest case, tile edges (8 x 8 pairs a tile; 64 and 65 shifts: one word and
# the word boundary), the full 127 bits, and more robots than the assignment pass has threads
SIZES = ((1, 1, 0), (2, 2, 1), (3, 5, 3), (32, 32, 31), (33, 33, 32), (67, 65, 63), (300, 4, 7))


def sized_case(b, k, max_delay, m=0, stride=2, bad=True, seed=0):
    """The circle family at the given size, the step chosen so that the drive takes about 3/4 of the K instants (300 robots
    and 4 instants: a tight ring on which neighbours touch), with M crossing obstacles, rows of `stride` floats, and (b >= 3)
    bad robots, a robot with a NaN radius and a bad obstacle."""
    rho = b / 8.0
    c = circle(b, k, max_delay, rho=rho, step=2.0 * rho / max(0.75 * (k - 1), 1.0), seed=seed + b)
    if b >= 256:
        rho = b / 34.0
        c = circle(b, k, max_delay, rho=rho, step=0.0625, seed=seed + b, jitter=2.0 ** -6)
    if m:
        c = crossing_obstacles(c, m, seed=seed + b, radius=0.0625, extent=1.25 * rho)
    if bad and b >= 3:
        c = with_bad(c, robots=(b // 2, b - 1) if b > 4 else (1,), obstacles=(m // 2,) if m > 1 else (), radius_robot=2 if b > 4 else None)
    return with_stride(c, stride, seed=seed)
