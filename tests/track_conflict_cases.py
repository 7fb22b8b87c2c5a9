"""Tracks for the conflict-detection tests (tests/test_track_conflict_cpu.py on the restatement, tests/test_gpu_track_conflict.py
on the device): hand cases on integer or dyadic coordinates, whose expected values are exact, and a seeded random set of wiggly
tracks with stops.  A case is a dict(a=[Ba, K, S], b=[Bb, K, S] or None, dt, t0, radius_a, radius_b, margin) -- the keyword
arguments of track_conflict_ref.conflicts -- and hand cases carry `expect`, a dict of exact values for the pair (0, 0) (self
mode: the pair (0, 1))."""
import numpy as np

F32 = np.float32


def track(xs, ys):
    """[K, 2] fp32 from two coordinate lists (a number = constant)."""
    xs, ys = np.broadcast_arrays(np.asarray(xs, np.float64), np.asarray(ys, np.float64))
    return np.stack([xs, ys], -1).astype(F32)


def case(a, b, dt=1.0, t0=0.0, radius_a=0.5, radius_b=0.5, margin=0.0, **expect):
    a = np.asarray(a, F32)
    a = a[None] if a.ndim == 2 else a
    if b is not None:
        b = np.asarray(b, F32)
        b = b[None] if b.ndim == 2 else b
    ra = np.broadcast_to(np.asarray(radius_a, F32), (len(a),)).copy()
    rb = None if b is None else np.broadcast_to(np.asarray(0.0 if radius_b is None else radius_b, F32), (len(b),)).copy()
    return dict(a=a, b=b, dt=dt, t0=t0, radius_a=ra, radius_b=rb, margin=margin, expect=expect)


def kwargs(c):
    """The keyword arguments of track_conflict_ref.conflicts / pairs for case `c`."""
    return dict(dt=c["dt"], t0=c["t0"], radius_a=c["radius_a"], radius_b=c["radius_b"], margin=c["margin"])


def hand_cases():
    k = np.arange(11.0)
    one_step_closer = float(np.nextafter(F32(1.0), F32(0.0)))
    out = {}
    # (0,0)->(10,0) against (10,0)->(0,0): they meet at t = 5; R = 1 is reached half-way through interval 4
    out["head_on"] = case(track(k, 0.0), track(10.0 - k, 0.0), M=0.0, tstar=5.0, tc=4.5, gap=-1.0)
    # a crossing at (5, 0): A passes at t = 5, B waits 2 s and passes at t = 7; closest sqrt(2) at the end of interval 5
    out["right_angle_late"] = case(track(k, 0.0), track(5.0, -5.0 + np.maximum(k - 2.0, 0.0)), M=2.0, tstar=6.0, tc=np.inf,
                                   gap=float(np.sqrt(2.0) - 1.0))
    # without the wait they collide
    out["right_angle_on_time"] = case(track(k, 0.0), track(5.0, -5.0 + k), M=0.0, tstar=5.0, tc=4.0 + (2.0 - np.sqrt(2.0)) / 2.0, gap=-1.0)
    # side by side at exactly R: a == 0 in every interval, the test is strict
    out["parallel_at_R"] = case(track(k, 0.0), track(k, 1.0), t0=2.0, M=1.0, tstar=2.0, tc=np.inf, gap=0.0)
    # one fp32 step closer: in conflict from t0 on
    out["parallel_inside_R"] = case(track(k, 0.0), track(k, one_step_closer), t0=2.0, M=one_step_closer * one_step_closer, tstar=2.0, tc=2.0,
                                    gap=one_step_closer - 1.0)
    # moving apart from 1 m: b >= 0 in every interval
    out["moving_apart"] = case(track(-k, 0.0), track(1.0 + k, 0.0), radius_a=0.25, radius_b=0.25, M=1.0, tstar=0.0, tc=np.inf, gap=0.5)
    # one interval, still approaching at its end: -b >= a
    out["closest_at_end"] = case(track([0.0, 1.0], 0.0), track([3.0, 3.0], 0.0), dt=0.5, M=4.0, tstar=0.5, tc=np.inf, gap=1.0)
    # A parks at (2, 0.5) from k = 2 on; B passes along y = -0.5 and is abreast at t = 8.  R = 1.25: entry where |d|^2 = 1.5625
    out["parked_passed"] = case(track(np.minimum(k, 2.0), 0.5), track(10.0 - k, -0.5), radius_a=0.75, M=1.0, tstar=8.0, tc=7.25, gap=-0.25)
    # a glancing pass inside one interval: the interior branch and the root; d = (-1 + 2 s, 0.5), R = 0.625
    out["interior_root"] = case(track([0.0, 2.0], 0.5), track([1.0, 1.0], 0.0), radius_a=0.125, M=0.25, tstar=0.5, tc=0.3125, gap=-0.125)
    # a single instant
    out["single_instant_hit"] = case(track([0.0], 0.0), track([0.5], 0.0), t0=3.0, M=0.25, tstar=3.0, tc=3.0, gap=-0.5)
    out["single_instant_miss"] = case(track([0.0], 0.0), track([1.5], 0.0), t0=3.0, M=2.25, tstar=3.0, tc=np.inf, gap=0.5)
    # a conflict that only the last-instant term reports needs K = 1: with K = 2 a meeting at the end of the interval is found
    # by the interval itself (s = 1), entered three quarters of the way
    out["end_touch"] = case(track([0.0, 0.0], 0.0), track([4.0, 0.0], 0.0), M=0.0, tstar=1.0, tc=0.75, gap=-1.0)
    return out


def mirrored_self():
    """Self mode, 4 tracks: track 0 parked at the origin, tracks 1 and 2 mirrored about it (equal gaps and equal first
    times: the smaller partner wins both ties), track 3 far away."""
    k = np.arange(9.0)
    a = np.stack([track(0.0 * k, 0.0), track(k - 4.0, 0.5), track(4.0 - k, -0.5), track(100.0 + k, 100.0)])
    return case(a, None, radius_a=0.5)


def alone():
    """Self mode, one track: no partner."""
    return case(track(np.arange(4.0), 0.0), None)


def bad_tracks(self_mode):
    """Tracks 1 (NaN y at one instant) and 3 (inf x) are bad; with set B, B's track 2 is bad and B's track 0 has a NaN radius."""
    k = np.arange(6.0)
    a = np.stack([track(k, 0.0), track(k, 0.5), track(5.0 - k, 0.25), track(k, 3.0), track(2.0, k - 2.0)])
    a[1, 3, 1] = np.nan
    a[3, 0, 0] = np.inf
    if self_mode:
        return case(a, None, radius_a=0.25)
    b = np.stack([track(k, 1.0), track(5.0 - k, 0.0), track(k, k), track(3.0 + 0.0 * k, 0.125)])
    b[2, 5, 0] = -np.inf
    rb = np.array([np.nan, 0.25, 0.25, 0.5], F32)
    return case(a, b, radius_a=0.25, radius_b=rb)


def with_stride(c, stride, seed=0):
    """The case with rows of `stride` floats: columns 2.. hold junk (NaN among it) that must not be read."""
    rng = np.random.default_rng(seed)

    def widen(t):
        if t is None or stride == 2:
            return t
        junk = rng.uniform(-1e6, 1e6, t.shape[:2] + (stride - 2,)).astype(F32)
        junk[..., 0][rng.uniform(size=junk.shape[:2]) < 0.2] = np.nan
        return np.concatenate([t[:, :, :2], junk], -1)
    return dict(c, a=widen(c["a"]), b=widen(c["b"]))


def wiggly_tracks(rng, n, k, extent=8.0, step=0.35):
    """[n, k, 2] fp32: heading random walks inside a square of `extent` metres, with stops (stretches of repeated positions)
    and changes of pace."""
    out = np.zeros((n, k, 2))
    for i in range(n):
        p = rng.uniform(0.0, extent, 2)
        heading, pace, wait = rng.uniform(-np.pi, np.pi), 1.0, 0
        for j in range(k):
            out[i, j] = p
            if wait > 0:
                wait -= 1
                continue
            if rng.uniform() < 0.08:
                wait = int(rng.integers(1, 5))
                continue
            if rng.uniform() < 0.2:
                pace = rng.choice([0.3, 1.0, 1.6])
            heading += rng.uniform(-0.5, 0.5)
            q = p + step * pace * np.array([np.cos(heading), np.sin(heading)])
            if not (0.0 <= q[0] <= extent and 0.0 <= q[1] <= extent):
                heading += np.pi
                q = p + step * pace * np.array([np.cos(heading), np.sin(heading)])
            p = q
    return out.astype(F32)


RANDOM_MARGIN = 0.25  # with radii of 0.15 .. 0.45 m on an 8 m floor: roughly a third of the pairs conflict (asserted in the CPU test)


def random_case(seed, ba, bb, k, stride=2, dt=0.25, t0=-1.0, bad=False):
    """Wiggly tracks with radii drawn per track; bb None = self mode.  `bad` plants a NaN in one track of each side."""
    rng = np.random.default_rng(seed)
    a = wiggly_tracks(rng, ba, k)
    b = None if bb is None else wiggly_tracks(rng, bb, k)
    ra = rng.uniform(0.15, 0.45, ba).astype(F32)
    rb = None if bb is None else rng.uniform(0.15, 0.45, bb).astype(F32)
    if bad and ba > 1:
        a[ba // 2, k // 2, 0] = np.nan
    if bad and bb:
        b[bb - 1, 0, 1] = np.inf
    c = dict(a=a, b=b, dt=dt, t0=t0, radius_a=ra, radius_b=rb, margin=RANDOM_MARGIN, expect={})
    return with_stride(c, stride, seed)
