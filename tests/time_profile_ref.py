"""numpy restatement of csrc/time_profile.hip: the velocity profile of nfopp_path_time_profile and the timed states of
nfopp_path_time_sample, float64 with every operation a separate numpy operation in the order include/nfopp_hip.h states,
the two prefix sums in integers.  `profile` also returns what the device does not store (caps, closed-form terms, phases)
for the property tests, and `sweeps` is the sequential formulation the closed form replaces.
Checked by hand-computed cases in tests/test_time_profile_cpu.py; the GPU tests compare the device with it bit for bit."""
import collections

import numpy as np

from swept_refine_ref import wrap_f32

F32 = np.float32
TWO32 = 4294967296.0
INV32 = 1.0 / TWO32
SEG_LIMIT, TOTAL_LIMIT, TIME_LIMIT = 2.0 ** 20, 2.0 ** 21, 2.0 ** 20
SLOT_S, SLOT_T, SLOT_V, SLOT_VP = range(4)
SUM_TIME, SUM_LENGTH, SUM_STOPS, SUM_STATUS = range(4)
STATUS_START_TOO_FAST, STATUS_GOAL_UNREACHABLE, STATUS_OUT_OF_RANGE = 1, 2, 4
LIMIT_CAP, LIMIT_ACCEL, LIMIT_DECEL = 0, 1, 2          # what holds a vertex (detail["limiter"])

Limits = collections.namedtuple("Limits", "v_max a_max d_max a_lat w_max cos_cusp")
Limits.__new__.__defaults__ = (np.inf, np.inf, -1.0)


def gears(path):
    """int8 [N + 1]: the sign of each segment's forward component as nfopp_path_stats forms it, a zero taking the last
    non-zero sign before it, else the first after it, else +1; all +1 for dim 2."""
    p = np.asarray(path, F32).astype(np.float64)
    ex, ey = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
    if p.shape[1] != 3:
        return np.ones(len(ex), np.int8)
    with np.errstate(invalid="ignore"):
        fwd = np.cos(p[:-1, 2]) * ex + np.sin(p[:-1, 2]) * ey
    sg = np.where(fwd > 0, 1, np.where(fwd < 0, -1, 0)).astype(np.int8)
    out = sg.copy()
    for i in np.flatnonzero(sg == 0):
        before, after = np.flatnonzero(sg[:i]), np.flatnonzero(sg[i + 1:])
        out[i] = sg[before[-1]] if len(before) else (sg[i + 1 + after[0]] if len(after) else 1)
    return out


def _nan_row(m):
    return dict(profile=np.full((m, 4), np.nan), gear=np.zeros(m - 1, np.int8),
                summary=np.array([np.nan, np.nan, np.nan, float(STATUS_OUT_OF_RANGE)]))


def profile(path, lim, v_start=0.0, v_goal=0.0):
    """One path [N + 2, D] (fp32 values) -> dict(profile [N + 2, 4], gear int8 [N + 1], summary [4]) and, for rows in
    range, the intermediate arrays c, k, u, fwd, bwd, stop_cusp, stop_gear, limiter, cruise, duration, ds."""
    p32 = np.asarray(path, F32)
    p = p32.astype(np.float64)
    m = len(p)
    vs, vg = float(F32(v_start)), float(F32(v_goal))
    A, Dd = 2.0 * lim.a_max, 2.0 * lim.d_max
    ex, ey = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.sqrt(ex * ex + ey * ey)
    if not (np.isfinite(p).all() and 0.0 <= vs < np.inf and 0.0 <= vg < np.inf and (n < SEG_LIMIT).all()):
        return _nan_row(m)
    L = np.rint(n * TWO32).astype(np.uint64)
    S = np.concatenate([[0], np.cumsum(L, dtype=np.uint64)]).astype(np.uint64)
    if float(S[-1]) >= TOTAL_LIMIT * TWO32:
        return _nan_row(m)
    s = S.astype(np.float64) * INV32
    gear = gears(p32)
    # vertex caps
    ex0, ey0, ex1, ey1, n0, n1 = ex[:-1], ey[:-1], ex[1:], ey[1:], n[:-1], n[1:]
    cx, cy = p[2:, 0] - p[:-2, 0], p[2:, 1] - p[:-2, 1]
    chord = np.sqrt(cx * cx + cy * cy)
    both = (n0 > 0) & (n1 > 0)
    k = np.full(m, np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        kappa = (2.0 * np.abs(ex0 * ey1 - ey0 * ex1)) / ((n0 * n1) * chord)
        turning = both & (chord > 0) & (kappa > 0)
        q = lim.w_max / kappa
        k[1:-1] = np.where(turning, np.minimum(lim.a_lat / kappa, q * q), np.inf)
    stop_cusp = both & (ex0 * ex1 + ey0 * ey1 < lim.cos_cusp * (n0 * n1)) if lim.cos_cusp > -1.0 else np.zeros(m - 2, bool)
    stop_gear = gear[:-1] != gear[1:]
    stop = stop_cusp | stop_gear
    c = np.minimum(lim.v_max * lim.v_max, k)
    c[1:-1][stop] = 0.0
    c[0], c[-1] = vs * vs, vg * vg
    # speeds: the closed form of the two sweeps
    As, Ds = A * s, Dd * s
    fwd = np.minimum.accumulate(c - As) + As
    bwd = np.minimum.accumulate((c + Ds)[::-1])[::-1] - Ds
    u = np.maximum(0.0, np.minimum(np.minimum(c, fwd), bwd))
    v = np.sqrt(u)
    limiter = np.where(u == c, LIMIT_CAP, np.where(fwd <= bwd, LIMIT_ACCEL, LIMIT_DECEL))
    # segments
    ds = L.astype(np.float64) * INV32
    g = np.minimum(lim.v_max * lim.v_max, np.maximum(k[:-1], k[1:]))
    u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
    reach = ((((A * lim.d_max) * ds + lim.d_max * u0) + lim.a_max * u1) / (lim.a_max + lim.d_max))
    u_p = np.maximum(np.minimum(g, reach), np.maximum(u0, u1))
    v_p = np.sqrt(u_p)
    t_acc, t_dec = (v_p - v0) / lim.a_max, (v_p - v1) / lim.d_max
    l_cruise = np.maximum(0.0, (ds - (u_p - u0) / A) - (u_p - u1) / Dd)
    with np.errstate(invalid="ignore", divide="ignore"):
        t_cruise = np.where(l_cruise > 0, l_cruise / v_p, 0.0)
    duration = (t_acc + t_cruise) + t_dec
    if not (duration < TIME_LIMIT).all():
        return _nan_row(m)
    Q = np.rint(duration * TWO32).astype(np.uint64)
    T = np.concatenate([[0], np.cumsum(Q, dtype=np.uint64)]).astype(np.uint64)
    t = T.astype(np.float64) * INV32
    prof = np.stack([s, t, v, np.concatenate([v_p, v[-1:]])], 1)
    status = (STATUS_START_TOO_FAST if u[0] < vs * vs else 0) | (STATUS_GOAL_UNREACHABLE if u[-1] < vg * vg else 0)
    summary = np.array([t[-1], s[-1], float(stop.sum()), float(status)])
    return dict(profile=prof, gear=gear, summary=summary, c=c, k=k, u=u, fwd=fwd, bwd=bwd, stop_cusp=stop_cusp,
                stop_gear=stop_gear, limiter=limiter, cruise=l_cruise > 0, duration=duration, ds=ds, s=s)


def profile_batch(paths, lim, v_start=None, v_goal=None):
    """(profile [B, N + 2, 4], gear [B, N + 1], summary [B, 4]) of paths [B, N + 2, D]."""
    rows = [profile(p, lim, 0.0 if v_start is None else v_start[b], 0.0 if v_goal is None else v_goal[b])
            for b, p in enumerate(paths)]
    return (np.stack([r["profile"] for r in rows]), np.stack([r["gear"] for r in rows]),
            np.stack([r["summary"] for r in rows]))


def sweeps(c, ds, a_max, d_max):
    """u by the two sequential sweeps in float64: forward u_i = min(c_i, u_{i-1} + 2 a ds_{i-1}), then backward
    u_i = min(u_i, u_{i+1} + 2 d ds_i)."""
    u = np.array(c, np.float64)
    for i in range(1, len(u)):
        u[i] = min(u[i], u[i - 1] + (2.0 * a_max) * ds[i - 1])
    for i in range(len(u) - 2, -1, -1):
        u[i] = min(u[i], u[i + 1] + (2.0 * d_max) * ds[i])
    return u


def sample(path, prof, gear, lim, t0, dt, count):
    """(states fp32 [count, D + 1], segment int32 [count], dist float64 [count]) of one path at t0 + k * dt; `dist` is the
    distance run inside the segment before the rounding to fp32 (NaN outside a segment)."""
    p32 = np.asarray(path, F32)
    p = p32.astype(np.float64)
    m, d = p.shape
    n = m - 2
    gear = np.ones(m - 1, np.int8) if gear is None else np.asarray(gear, np.int8)
    t = np.float64(t0) + np.arange(count, dtype=np.float64) * np.float64(dt)
    states, seg, dist_out = np.full((count, d + 1), np.nan, F32), np.full(count, -1, np.int32), np.full(count, np.nan)
    tc = prof[:, SLOT_T]
    if count == 0 or np.isnan(tc[-1]):
        return states, seg, dist_out
    before, after = t < tc[0], t >= tc[-1]
    states[before, :d], states[before, d] = p32[0], 0.0
    states[after, :d], states[after, d] = p32[-1], F32(float(gear[-1]) * prof[-1, SLOT_V])
    seg[after] = n + 1
    mid = ~(before | after)
    i = np.minimum(np.searchsorted(tc, t[mid], side="right") - 1, n)        # the largest i <= N with t_i <= t
    tau = t[mid] - tc[i]
    dur, ds = tc[i + 1] - tc[i], prof[i + 1, SLOT_S] - prof[i, SLOT_S]
    v0, v1, vp = prof[i, SLOT_V], prof[i + 1, SLOT_V], prof[i, SLOT_VP]
    t_acc, t_dec = (vp - v0) / lim.a_max, (vp - v1) / lim.d_max
    rem = dur - tau
    ha, hd = 0.5 * lim.a_max, 0.5 * lim.d_max
    run_acc = v0 * tau + (ha * tau) * tau
    run_dec = ds - (v1 * rem + (hd * rem) * rem)
    run_cruise = (v0 * t_acc + (ha * t_acc) * t_acc) + vp * (tau - t_acc)
    accel, decel = tau < t_acc, rem < t_dec
    dist = np.where(accel, run_acc, np.where(decel, run_dec, run_cruise))
    speed = np.where(accel, v0 + lim.a_max * tau, np.where(decel, v1 + lim.d_max * rem, vp))
    dist, speed = np.minimum(np.maximum(dist, 0.0), ds), np.minimum(speed, vp)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(ds > 0, dist / ds, 0.0)
    out = np.empty((len(i), d + 1), F32)
    out[:, 0] = (p[i, 0] + frac * (p[i + 1, 0] - p[i, 0])).astype(F32)
    out[:, 1] = (p[i, 1] + frac * (p[i + 1, 1] - p[i, 1])).astype(F32)
    if d == 3:
        dth = wrap_f32((p32[i + 1, 2] - p32[i, 2]).astype(F32)).astype(np.float64)
        out[:, 2] = (p[i, 2] + frac * dth).astype(F32)
    out[:, d] = (gear[i].astype(np.float64) * speed).astype(F32)
    states[mid], seg[mid], dist_out[mid] = out, i, dist
    return states, seg, dist_out


def sample_batch(paths, prof, gear, lim, t0, dt, count):
    rows = [sample(p, prof[b], None if gear is None else gear[b], lim, t0, dt, count)[:2] for b, p in enumerate(paths)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
