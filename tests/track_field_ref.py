"""CPU restatement of the moving-obstacle collision term (csrc/track_field.hip, include/nfopp_hip.h: nfopp_track_field), for
the tests.

`track_rows(field, points, times, dtype)` restates the kernel's track row per pose and time.  With dtype float32 every
operation is one numpy float32 operation in the kernel's order, so the result equals the device's bit for bit wherever no sine
or cosine is taken (robots of centred discs); with float64 the same formulas run on the same fp32 inputs widened, and serve as
the reference the device is held against where numpy's float32 sine and the device's may differ in the last place.
`overlay` is the combination with the rows of a static collision model, `planner_step` the oracle's step with a distance
field and the overlay in the ONF's place."""
import collections

import numpy as np

import sdf_ref
from oracle import nfopp_oracle as orc

F32 = np.float32

# tracks fp32 [M, K, >= 2]; radius fp32 [M]; t0, inv_dt, margin, gain fp32 scalars; discs fp32 [n, 3]
Field = collections.namedtuple("Field", "tracks radius t0 inv_dt discs margin gain")


def make_field(tracks, dt, t0=0.0, radius=0.0, discs=((0.0, 0.0, 0.0),), margin=0.0, gain=10.0):
    """The nfopp_track_field block as the host forms it: t0, 1 / dt, the discs, margin and gain each rounded to fp32 once
    from double."""
    tracks = np.asarray(tracks, F32)
    radius = np.broadcast_to(np.asarray(radius, F32), (tracks.shape[0],)).copy()
    return Field(tracks, radius, F32(t0), F32(1.0 / float(dt)), np.asarray(discs, np.float64).reshape(-1, 3).astype(F32),
                 F32(margin), F32(gain))


def sample_times(wp_time, t, dtype=F32):
    """wp_time [B, N], t [B, N-1] -> [B, N-1]: tau = T[j+1] + t (T[j] - T[j+1]), one subtraction, one product, one sum."""
    T, tt = np.asarray(wp_time, dtype), np.asarray(t, dtype)
    return (T[:, 1:] + tt * (T[:, :-1] - T[:, 1:])).astype(dtype)


def time_index(field, times, dtype=F32):
    """times [P] -> (n, n1 int64 [P], s [P] of `dtype`, below bool [P], above bool [P]): the interval of the track grid, the
    weight in it, and whether the time was clamped at the first / last instant."""
    T = dtype
    K = field.tracks.shape[1]
    tau = np.asarray(times, T)
    with np.errstate(invalid="ignore", over="ignore"):
        w = (tau - T(field.t0)) * T(field.inv_dt)
        below, above = ~(w > 0), ~(w < T(K - 1))
        w = np.where(w > 0, w, T(0))
        w = np.where(w < T(K - 1), w, T(K - 1))
    n = np.maximum(np.minimum(np.floor(w).astype(np.int64), K - 2), 0)
    return n, np.minimum(n + 1, K - 1), (w - n.astype(T)).astype(T), below, above & ~below


def track_rows(field, points, times, dtype=F32, pose_dtype=F32):
    """points [P, 2 or 3] and times [P], rounded to `pose_dtype` (fp32: what the device is handed) -> (rows [P, 4] of `dtype`,
    choice int64 [P, 3], valid bool [P]): the track row per pose, what it was taken from -- the disc and the track that count
    (-1: no candidate counts) and the interval n -- and whether the pose and the time are finite (the others read no track;
    their rows are NaN here).  A row with no candidate that counts has a NaN logit."""
    T = dtype
    pts = np.asarray(points, pose_dtype)
    P, D = pts.shape
    x, y = pts[:, 0].astype(T), pts[:, 1].astype(T)
    th = pts[:, 2].astype(T) if D == 3 else np.zeros(P, T)
    tau = np.asarray(times, pose_dtype).astype(T)
    valid = np.isfinite(x) & np.isfinite(y) & np.isfinite(th) & np.isfinite(tau)
    x, y, th, tau = (np.where(valid, a, T(0)) for a in (x, y, th, tau))
    n, n1, s, _, _ = time_index(field, tau, T)
    discs, tracks, radius = field.discs.astype(T), field.tracks.astype(T), field.radius.astype(T)
    margin, gain = T(field.margin), T(field.gain)
    if (discs[:, :2] != 0).any():
        c, sn = np.cos(th).astype(T), np.sin(th).astype(T)
    else:   # a robot of centred discs takes no sine
        c, sn = np.ones(P, T), np.zeros(P, T)
    pen = np.full(P, np.nan, T)
    ex, ey, dist, lx, ly = (np.zeros(P, T) for _ in range(5))
    choice = np.full((P, 3), -1, np.int64)
    choice[:, 2] = n
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for d, (ox, oy, r) in enumerate(discs):
            if ox == 0 and oy == 0:
                cx, cy = x, y
            else:
                cx, cy = (x + ox * c) - oy * sn, (y + ox * sn) + oy * c
            lxd, lyd = (-ox) * sn - oy * c, ox * c - oy * sn
            for m in range(tracks.shape[0]):
                a, b = tracks[m, n], tracks[m, n1]
                qx, qy = a[:, 0] + s * (b[:, 0] - a[:, 0]), a[:, 1] + s * (b[:, 1] - a[:, 1])
                dx, dy = cx - qx, cy - qy
                dk = np.sqrt(dx * dx + dy * dy).astype(T)
                pk = ((r + radius[m]) + margin) - dk
                take = (pk > pen) | (np.isnan(pen) & ~np.isnan(pk))
                pen, ex, ey, dist, lx, ly = (np.where(take, new, old) for new, old in
                                             ((pk, pen), (dx, ex), (dy, ey), (dk, dist), (lxd, lx), (lyd, ly)))
                choice[take, 0], choice[take, 1] = d, m
        zero = dist == 0
        nx, ny = np.where(zero, T(0), ex / np.where(zero, T(1), dist)), np.where(zero, T(0), ey / np.where(zero, T(1), dist))
        nnx, nny = -nx, -ny
        dth = gain * (nnx * lx + nny * ly) if D == 3 else np.zeros(P, T)
        rows = np.stack([gain * pen, gain * nnx, gain * nny, dth], 1).astype(T)
    rows[~valid] = np.nan
    return rows, choice, valid


def overlay(field, points, times, base, dtype=F32):
    """base [P, 4] -> (out [P, 4] of `dtype`, won bool [P]): the rows with the track row in the place of every row whose logit
    the track row's exceeds (strict; NaN compares false on either side), and where that happened."""
    rows, _, valid = track_rows(field, points, times, dtype)
    base = np.asarray(base, dtype)
    with np.errstate(invalid="ignore"):
        won = valid & (rows[:, 0] > base[:, 0])
    return np.where(won[:, None], rows, base), won


def same_branch(choice_a, choice_b):
    """bool [P]: the poses at which two evaluations took the same disc, track and interval."""
    return (choice_a == choice_b).all(1)


def spread(field, points, times):
    """(SPREAD [4], kept bool [P]): the largest |float32 restatement - float64 restatement| of the track row per output column
    over the poses at which both took the same branch, and those poses."""
    r32, c32, _ = track_rows(field, points, times, F32)
    r64, c64, _ = track_rows(field, points, times, np.float64)
    kept = same_branch(c32, c64) & np.isfinite(r64).all(1)
    return np.abs(r32.astype(np.float64) - r64)[kept].max(0), kept


# ---- the planner step on a distance field with moving obstacles ------------------------------------------------------------------
def optimize_trajectory(sdf, field, wp_time, traj, start, goal, lam, cm, adam_m, adam_v, adam_step, t, hp, hinv):
    """sdf_ref.optimize_trajectory with the overlay behind the distance field's rows; `field` None: without it."""
    B, N, _ = traj.shape
    pts = orc.sample_collision_points(np.asarray(traj, F32), np.asarray(t, F32)).reshape(-1, 3)
    out, _ = sdf_ref.eval_points(sdf, pts, F32)
    if field is not None:
        out, _ = overlay(field, pts, sample_times(wp_time, t).reshape(-1), out)
    out = out.reshape(B, N - 1, 4)
    terms = orc.trajectory_loss_terms(traj, start, goal, lam, cm, t, out[..., 0], out[..., 1:], hp)
    g = np.einsum("ij,bjd->bid", hinv, terms["g_traj"]).astype(F32)
    new_traj, m, v = orc.adam_update(traj, g, adam_m, adam_v, adam_step + 1, hp.lr, hp.beta1, hp.beta2, hp.eps)
    new_lam = (np.asarray(lam, F32) + F32(hp.multipliers_lr) * terms["g_lam"]).astype(F32)
    new_cm = (np.asarray(cm, F32) + F32(hp.collision_multipliers_lr) * terms["g_cm"]).astype(F32)
    new_cm = np.where(new_cm > 0, new_cm, F32(0)).astype(F32)
    return new_traj, new_lam, new_cm, m, v, terms


def planner_step(sdf, field, wp_time, state, t, hp, hinv, reparam_freq=10):
    """sdf_ref.planner_step with moving obstacles; `state` is updated in place."""
    tr, lam, cm, m, v, terms = optimize_trajectory(sdf, field, wp_time, state["traj"], state["start"], state["goal"], state["lam"],
                                                   state["cm"], state["adam_m"], state["adam_v"], state["adam_step"], t, hp, hinv)
    state.update(traj=tr, lam=lam, cm=cm, adam_m=m, adam_v=v, adam_step=state["adam_step"] + 1)
    if state["step_count"] % reparam_freq == 0:
        tr, lam, cm = orc.reparametrize(state["traj"], state["start"], state["goal"], state["lam"], state["cm"])
        state.update(traj=tr, lam=lam, cm=cm)
    state["step_count"] += 1
    return terms
