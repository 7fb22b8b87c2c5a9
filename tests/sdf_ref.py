"""CPU restatement of the distance-field collision model (OccupancyGrid.signed_distance_field, csrc/sdf_field.hip,
include/nfopp_hip.h: nfopp_sdf_field), for the tests.

`eval_points(field, points, dtype)` restates the kernel's row per pose.  With dtype float32 every operation is one numpy
float32 operation in the kernel's order, so the result equals the device's bit for bit wherever no sine or cosine is taken
(robots of centred discs); with float64 the same formulas run on the same fp32 inputs widened, and serve as the reference
the device is held against where numpy's float32 sine and the device's may differ in the last place."""
import collections

import numpy as np

import edt_ref
from oracle import nfopp_oracle as orc

F32 = np.float32

Field = collections.namedtuple("Field", "sd x0 y0 inv_res discs margin gain")


def signed_distance(occupancy, resolution, border=False):
    """-> fp32 [rows, cols]: resolution * (sqrt(dist2 to the nearest wall) - sqrt(dist2 to the nearest free cell)), formed in
    float64 and rounded once; a missing distance (no wall / no free cell at all) counts as rows + cols cells."""
    occ = np.asarray(occupancy) != 0
    far = float(occ.shape[0] + occ.shape[1])
    cells = [np.where(d2 == edt_ref.NONE, far, np.sqrt(d2.astype(np.float64)))
             for d2 in (edt_ref.edt(occ, border)[0], edt_ref.edt(~occ, False)[0])]
    return ((cells[0] - cells[1]) * float(resolution)).astype(F32)


def make_field(sd, boundaries, resolution, discs, margin, gain):
    """The nfopp_sdf_field block as the host forms it: x0, y0, 1 / resolution, the discs, margin and gain each rounded to fp32
    once from double."""
    return Field(np.asarray(sd, F32), F32(boundaries[0]), F32(boundaries[2]), F32(1.0 / float(resolution)),
                 np.asarray(discs, np.float64).reshape(-1, 3).astype(F32), F32(margin), F32(gain))


def _axis(u, count, T):
    last = T(count - 1)
    inside = (u > 0) & (u < last)
    c = np.where(u > 0, u, T(0))
    c = np.where(c < last, c, last)
    cell = np.minimum(np.floor(c).astype(np.int64), count - 2)
    return cell, (c - cell.astype(T)).astype(T), inside


def eval_points(field, points, dtype=F32, pose_dtype=F32):
    """points [P, 2 or 3], rounded to `pose_dtype` (fp32: what the device is handed) -> (out [P, 4] of `dtype`, choice int64
    [P, 5]): the row per pose and what it was taken from -- the disc that counts, its cell (i, j) and its two inside flags.
    Two evaluations that agree on `choice` took the same branch of the (piecewise bilinear, piecewise per disc) function."""
    T = dtype
    pts = np.asarray(points, pose_dtype)
    P, D = pts.shape
    x, y = pts[:, 0].astype(T), pts[:, 1].astype(T)
    th = pts[:, 2].astype(T) if D == 3 else np.zeros(P, T)
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(th)
    x, y, th = (np.where(finite, a, T(0)) for a in (x, y, th))
    discs = field.discs.astype(T)
    sd = field.sd.astype(T)
    rows, cols = sd.shape
    x0, y0, inv_res, margin, gain, half = T(field.x0), T(field.y0), T(field.inv_res), T(field.margin), T(field.gain), T(0.5)
    if (discs[:, :2] != 0).any():
        c, s = np.cos(th).astype(T), np.sin(th).astype(T)
    else:   # a robot of centred discs takes no sine
        c, s = np.ones(P, T), np.zeros(P, T)
    pen = gx = gy = lx = ly = None
    choice = np.zeros((P, 5), np.int64)
    for k, (ox, oy, r) in enumerate(discs):
        if ox == 0 and oy == 0:
            cx, cy = x, y
        else:
            cx, cy = (x + ox * c) - oy * s, (y + ox * s) + oy * c
        u = (cx - x0) * inv_res - half
        v = (cy - y0) * inv_res - half
        i, fu, in_x = _axis(u, cols, T)
        j, fv, in_y = _axis(v, rows, T)
        s00, s01, s10, s11 = sd[j, i], sd[j, i + 1], sd[j + 1, i], sd[j + 1, i + 1]
        a, b = s01 - s00, s11 - s10
        top, bot = s00 + fu * a, s10 + fu * b
        d = top + fv * (bot - top)
        pk = (r + margin) - d
        gxk = np.where(in_x, (a + fv * (b - a)) * inv_res, T(0))
        gyk = np.where(in_y, (bot - top) * inv_res, T(0))
        lxk, lyk = (-ox) * s - oy * c, ox * c - oy * s
        if k == 0:
            pen, gx, gy, lx, ly = pk, gxk, gyk, lxk, lyk
            take = np.ones(P, bool)
        else:
            take = pk > pen
            pen, gx, gy, lx, ly = (np.where(take, new, old) for new, old in ((pk, pen), (gxk, gx), (gyk, gy), (lxk, lx), (lyk, ly)))
        choice[take] = np.stack([np.full(P, k), i, j, in_x, in_y], 1)[take]
    ngx, ngy = -gx, -gy
    dth = gain * (ngx * lx + ngy * ly) if D == 3 else np.zeros(P, T)
    out = np.stack([gain * pen, gain * ngx, gain * ngy, dth], 1).astype(T)
    out[~finite] = np.nan
    return out, choice


def same_branch(choice_a, choice_b):
    """bool [P]: the poses at which two evaluations took the same disc, cell and inside flags."""
    return (choice_a == choice_b).all(1)


def spread(field, points):
    """(SPREAD [4], kept bool [P]): the largest |float32 restatement - float64 restatement| per output column over the poses
    at which both took the same branch, and those poses."""
    o32, c32 = eval_points(field, points, F32)
    o64, c64 = eval_points(field, points, np.float64)
    kept = same_branch(c32, c64) & np.isfinite(o64).all(1)
    return np.abs(o32.astype(np.float64) - o64)[kept].max(0), kept


# ---- the planner step on a distance field: the oracle's step with this model in the ONF's place ----------------------------
def optimize_trajectory(field, traj, start, goal, lam, cm, adam_m, adam_v, adam_step, t, hp, hinv):
    """orc.optimize_trajectory (SE(2)) with eval_points where the oracle evaluates the ONF."""
    B, N, _ = traj.shape
    pts = orc.sample_collision_points(np.asarray(traj, F32), np.asarray(t, F32))
    out, _ = eval_points(field, pts.reshape(-1, 3), F32)
    out = out.reshape(B, N - 1, 4)
    terms = orc.trajectory_loss_terms(traj, start, goal, lam, cm, t, out[..., 0], out[..., 1:], hp)
    g = np.einsum("ij,bjd->bid", hinv, terms["g_traj"]).astype(F32)
    new_traj, m, v = orc.adam_update(traj, g, adam_m, adam_v, adam_step + 1, hp.lr, hp.beta1, hp.beta2, hp.eps)
    new_lam = (np.asarray(lam, F32) + F32(hp.multipliers_lr) * terms["g_lam"]).astype(F32)
    new_cm = (np.asarray(cm, F32) + F32(hp.collision_multipliers_lr) * terms["g_cm"]).astype(F32)
    new_cm = np.where(new_cm > 0, new_cm, F32(0)).astype(F32)
    return new_traj, new_lam, new_cm, m, v, terms


def planner_step(field, state, t, hp, hinv, reparam_freq=10):
    """orc.planner_step on a distance field; `state` is updated in place."""
    tr, lam, cm, m, v, terms = optimize_trajectory(field, state["traj"], state["start"], state["goal"], state["lam"],
                                                   state["cm"], state["adam_m"], state["adam_v"], state["adam_step"], t, hp, hinv)
    state.update(traj=tr, lam=lam, cm=cm, adam_m=m, adam_v=v, adam_step=state["adam_step"] + 1)
    if state["step_count"] % reparam_freq == 0:
        tr, lam, cm = orc.reparametrize(state["traj"], state["start"], state["goal"], state["lam"], state["cm"])
        state.update(traj=tr, lam=lam, cm=cm)
    state["step_count"] += 1
    return terms
