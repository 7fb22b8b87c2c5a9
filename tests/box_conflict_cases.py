"""Tracks for the box conflict tests (tests/test_box_conflict_cpu.py on the restatement, tests/test_gpu_box_conflict.py on the
device): hand cases on dyadic coordinates with unit vectors given directly as (+-1, 0) and (0, +-1), whose expected values are
exact, and a seeded random family of cars that drive along their headings.  A case is a dict(a=[Ba, K, 3] fp32 (x, y, theta),
ua=[Ba, K, 2] float64, b, ub (None: self mode), box_a, box_b [B, 4] fp32, radius_a, radius_b, dt, t0, margin); hand cases
carry `expect`: {refine: (status, first_conflict, first_undecided)} of the pair (0, 0) (self mode: the pair (0, 1))."""
import numpy as np

import box_conflict_ref as br
import track_conflict_cases as tc

F32, F64 = np.float32, np.float64
INF = np.inf
CAR = (-1.0, 1.0, -0.5, 0.5)                 # the 2 x 1 box of the hand cases
SWEPT_BOX = (-0.34, 0.4, -0.27, 0.27)        # the car of profiles/swept.txt
EAST, NORTH, WEST, SOUTH = (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)
_THETA = {EAST: 0.0, NORTH: np.pi / 2, WEST: np.pi, SOUTH: -np.pi / 2}


def track(xs, ys, units):
    """([K, 3] fp32, [K, 2] float64) from coordinate lists (a number = constant) and one unit vector or a list of K."""
    xs, ys = np.broadcast_arrays(np.asarray(xs, F64), np.asarray(ys, F64))
    units = [units] * len(xs) if isinstance(units[0], float) else list(units)
    assert len(units) == len(xs)
    th = np.array([_THETA[tuple(u)] for u in units])
    return np.stack([xs, ys, th], -1).astype(F32), np.array(units, F64)


def case(a, b, dt=1.0, t0=0.0, box_a=CAR, box_b=CAR, radius_a=0.0, radius_b=0.0, margin=0.0, expect=None):
    def side(t):
        if t is None:
            return None, None
        if isinstance(t, tuple):
            t = [t]
        return np.stack([x[0] for x in t]), np.stack([x[1] for x in t])
    ta, ua = side(a)
    tb, ub = side(b)

    def boxes(bx, n):
        return np.broadcast_to(np.asarray(bx, F32).reshape(-1, 4), (n, 4)).copy()
    return dict(a=ta, ua=ua, b=tb, ub=ub, dt=dt, t0=t0, box_a=boxes(box_a, len(ta)), box_b=None if tb is None else boxes(box_b, len(tb)),
                radius_a=np.broadcast_to(np.asarray(radius_a, F32), (len(ta),)).copy(),
                radius_b=None if tb is None else np.broadcast_to(np.asarray(radius_b, F32), (len(tb),)).copy(),
                margin=margin, expect=expect or {})


def kwargs(c, refine=0):
    """The keyword arguments of box_conflict_ref.conflicts / pairs for case `c`."""
    return dict(dt=c["dt"], t0=c["t0"], box_a=c["box_a"], box_b=c["box_b"], radius_a=c["radius_a"], radius_b=c["radius_b"],
                margin=c["margin"], refine=refine)


FREE, CONFLICT, UNDECIDED = br.FREE, br.CONFLICT, br.UNDECIDED
TURN_GAP_FREE = 2.1875       # a parked car this far east of a car that turns in place: never touched (2.1875 - 1 > sqrt(1.25))
TURN_GAP_HIT = 2.0625        # touched while the corner swings past: sqrt(1.25) cos(theta - 26.57 deg) > 1.0625 for 8.4 .. 44.7 deg


def hand_cases():
    k = np.arange(9.0)
    out = {}
    # two 2 x 1 cars side by side in lanes 1.25 apart, same speed: the bodies are 0.25 apart, the circumscribed discs overlap
    out["parallel_lanes"] = case(track(0.5 * k, 0.0, EAST), track(0.5 * k, 1.25, EAST), expect={0: (FREE, INF, INF)})
    # head-on in one lane: the noses meet at t = 4 (sep == 0: no conflict), the bodies coincide at t = 5.  refine 0: interval 4
    # is UNDECIDED at 4, the instant 5 is in conflict; refine 3: [4, 4.125] stays undecided, 4.125 is the first node inside
    k11 = np.arange(11.0)
    out["head_on"] = case(track(k11, 0.0, EAST), track(10.0 - k11, 0.0, WEST),
                          expect={0: (CONFLICT, 5.0, 4.0), 3: (CONFLICT, 4.125, 4.0), 8: (CONFLICT, 4.0 + 2.0 ** -8, 4.0)})
    # a right-angle crossing at (5, 0): sep(t) = max(3.5 - t, t - 6.5)
    out["right_angle"] = case(track(k11, 0.0, EAST), track(5.0, -5.0 + k11, NORTH),
                              expect={0: (CONFLICT, 4.0, 3.0), 2: (CONFLICT, 3.75, 3.25)})
    # parked side by side, the rounded bodies exactly touching: sep == R is no conflict, and nothing moves
    out["touching"] = case(track([0.0] * 3, 0.0, EAST), track([0.0] * 3, 1.25, EAST), radius_a=0.25, expect={0: (FREE, INF, INF)})
    # one float64 step closer than touching
    out["one_step_closer"] = case(track([0.0] * 3, 0.0, EAST), track([0.0] * 3, 1.25, EAST), t0=2.0,
                                  margin=float(np.nextafter(0.25, 1.0)), expect={0: (CONFLICT, 2.0, INF)})
    # a single instant
    out["single_instant_hit"] = case(track([0.0], 0.0, EAST), track([1.25], 0.75, NORTH), t0=3.0, expect={0: (CONFLICT, 3.0, INF)})
    out["single_instant_miss"] = case(track([0.0], 0.0, EAST), track([1.5], 1.0, NORTH), t0=3.0, expect={0: (FREE, INF, INF)})
    # corner to corner: the discs are clear of each other by more than R, the face axes see only 0.75 (the separating-axis gap
    # is short of the corner distance): the discs speak first, at the last instant too
    out["single_instant_corners"] = case(track([0.0], 0.0, EAST), track([2.5], 1.75, EAST), margin=0.78125, expect={0: (FREE, INF, INF)})
    out["parked_corners"] = case(track([0.0] * 3, 0.0, EAST), track([2.5] * 3, 1.75, EAST), margin=0.78125, expect={0: (FREE, INF, INF)})
    # a quarter turn in place beside a parked car: the certificate cannot decide the whole turn, its parts it can
    turn = track([0.0, 0.0], 0.0, [EAST, NORTH])
    out["quarter_turn_free"] = case(turn, track([TURN_GAP_FREE] * 2, 0.0, EAST), expect={0: (UNDECIDED, INF, 0.0), 8: (FREE, INF, INF)})
    # the same turn closer: free at both ends, the corner touches in between.  refine 2: [0, 1/4] undecided, 22.5 degrees is
    # inside; refine 3: [0, 1/8] undecided, 11.25 degrees is inside
    out["quarter_turn_hit"] = case(turn, track([TURN_GAP_HIT] * 2, 0.0, EAST), dt=2.0, t0=1.0,
                                   expect={0: (UNDECIDED, INF, 1.0), 2: (CONFLICT, 1.5, 1.0), 3: (CONFLICT, 1.25, 1.0)})
    # a half turn: the mid heading is not defined
    out["half_turn"] = case(track([0.0, 0.0], 0.0, [EAST, WEST]), track([TURN_GAP_FREE] * 2, 0.0, EAST),
                            expect={0: (UNDECIDED, INF, 0.0), 8: (UNDECIDED, INF, 0.0)})
    # the lanes again with rounded bodies: 0.125 each touches exactly, 0.25 each is a conflict from the start
    out["rounded_touching"] = case(track(0.5 * k, 0.0, EAST), track(0.5 * k, 1.25, EAST), radius_a=0.125, radius_b=0.125,
                                   expect={0: (FREE, INF, INF)})
    out["rounded_hit"] = case(track(0.5 * k, 0.0, EAST), track(0.5 * k, 1.25, EAST), radius_a=0.25, radius_b=0.25,
                              expect={0: (CONFLICT, 0.0, INF)})
    return out


def bad_tracks(self_mode):
    """Set A: track 1 has a NaN y, track 3 an infinite heading, track 4 a box with x0 > x1; with set B: B's track 0 has a NaN
    radius, B's track 2 a NaN box entry."""
    k = np.arange(6.0)
    a = [track(k, 0.0, EAST), track(k, 0.75, EAST), track(5.0 - k, 0.5, WEST), track(k, 3.0, EAST), track(2.0, k - 2.0, NORTH),
         track(2.5, 4.0 - k, SOUTH)]
    box_a = np.tile(np.asarray(CAR, F32), (6, 1))
    box_a[4] = (1.0, -1.0, -0.5, 0.5)
    if self_mode:
        c = case(a, None, box_a=box_a)
    else:
        b = [track(k, 1.0, EAST), track(5.0 - k, 0.0, WEST), track(k, k, NORTH), track(3.0, 0.125 * k, NORTH)]
        box_b = np.tile(np.asarray(CAR, F32), (4, 1))
        box_b[2, 3] = np.nan
        c = case(a, b, box_a=box_a, box_b=box_b, radius_b=np.array([np.nan, 0.0, 0.0, 0.25], F32))
    c["a"][1, 3, 1] = np.nan
    c["a"][3, 2, 2] = np.inf
    c["ua"][3, 2] = np.nan
    return c


def car_tracks(rng, n, k, extent=8.0, step=0.35):
    """[n, k, 3] fp32: track_conflict_cases' wiggly walks with the heading along the motion (kept while the car waits)."""
    xy = tc.wiggly_tracks(rng, n, k, extent=extent, step=step).astype(F64)
    out = np.zeros((n, k, 3))
    out[:, :, :2] = xy
    for i in range(n):
        th = rng.uniform(-np.pi, np.pi)
        moves = [(j, xy[i, j + 1] - xy[i, j]) for j in range(k - 1) if (xy[i, j + 1] != xy[i, j]).any()]
        if moves:
            th = np.arctan2(moves[0][1][1], moves[0][1][0])
        for j in range(k):
            if j < k - 1 and (xy[i, j + 1] != xy[i, j]).any():
                d = xy[i, j + 1] - xy[i, j]
                th = np.arctan2(d[1], d[0])
            out[i, j, 2] = th
    return out.astype(F32)


RANDOM_MARGIN = 0.0625


def random_case(seed, ba, bb, k, stride=3, dt=0.25, t0=-1.0, bad=False, per_track_boxes=True, radii=True, extent=8.0):
    """Cars on an `extent`-metre floor; bb None = self mode.  `bad` plants a NaN position in one track of A and a bad box in
    one of the other side (self mode: of A).  The unit vectors are numpy's: the GPU test replaces them with the device's."""
    rng = np.random.default_rng(seed)

    def boxes(n):
        bx = np.tile(np.asarray(SWEPT_BOX, F32), (n, 1))
        if per_track_boxes:
            bx = (bx * rng.uniform(0.6, 1.4, (n, 1))).astype(F32)
            bx[:, 1] += rng.uniform(0.0, 0.2, n).astype(F32)
        return bx
    a = car_tracks(rng, ba, k, extent)
    b = None if bb is None else car_tracks(rng, bb, k, extent)
    box_a, box_b = boxes(ba), None if bb is None else boxes(bb)
    ra = (rng.uniform(0.0, 0.1, ba) if radii else np.zeros(ba)).astype(F32)
    rb = None if bb is None else (rng.uniform(0.0, 0.1, bb) if radii else np.zeros(bb)).astype(F32)
    if bad and ba > 2:
        a[ba // 2, k // 2, 0] = np.nan
        if bb is None:
            box_a[ba - 1, 2] = box_a[ba - 1, 3]
    if bad and bb and bb > 1:
        box_b[bb - 1, 0] = np.inf
    c = dict(a=a, b=b, dt=dt, t0=t0, box_a=box_a, box_b=box_b, radius_a=ra, radius_b=rb, margin=RANDOM_MARGIN, expect={})
    c = with_stride(c, stride, seed)
    c["ua"], c["ub"] = br.unit_vectors(c["a"]), None if b is None else br.unit_vectors(c["b"])
    return c


def with_stride(c, stride, seed=0):
    """The case with rows of `stride` floats: columns 3.. hold junk (NaN among it) that must not be read."""
    rng = np.random.default_rng(seed)

    def widen(t):
        if t is None or stride == 3:
            return t
        junk = rng.uniform(-1e6, 1e6, t.shape[:2] + (stride - 3,)).astype(F32)
        junk[..., 0][rng.uniform(size=junk.shape[:2]) < 0.2] = np.nan
        return np.concatenate([t[:, :, :3], junk], -1)
    return dict(c, a=widen(c["a"]), b=widen(c["b"]))
