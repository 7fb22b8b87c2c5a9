"""CPU restatement of the heading-layered distance field (csrc/heading_field.hip, nfopp/heading_field.py,
include/nfopp_hip.h: nfopp_heading_field), for the tests.

`eval_points(field, points, dtype)` restates the kernel's row per pose.  With dtype float32 every operation is one numpy
float32 operation in the kernel's order (np.floor and np.fmod are exact, as floorf and fmodf are), so the result equals the
device's bit for bit; with float64 the same formulas run on the same fp32 inputs widened."""
import collections

import numpy as np

import sdf_ref
from oracle import nfopp_oracle as orc

F32 = np.float32

Field = collections.namedtuple("Field", "sd x0 y0 inv_res layers_per_rad margin gain")


def slice_headings(n_layers):
    """float32 [L]: the heading of slice k, float32(k * 2 pi / L) formed in double."""
    return np.asarray([F32(k * (2 * np.pi) / n_layers) for k in range(n_layers)], F32)


def signed_distance_stack(layers, resolution, border=False):
    """uint8 [L, rows, cols] -> fp32 [L, rows, cols]: sdf_ref.signed_distance of every slice."""
    return np.stack([sdf_ref.signed_distance(occ, resolution, border) for occ in np.asarray(layers)])


def make_field(layers, boundaries, resolution, margin, gain, border=False):
    """The nfopp_heading_field block as the host forms it: the stacked image, and x0, y0, 1 / resolution, L / (2 pi), margin
    and gain each rounded to fp32 once from double."""
    sd = signed_distance_stack(layers, resolution, border)
    return Field(sd, F32(boundaries[0]), F32(boundaries[2]), F32(1.0 / float(resolution)), F32(len(sd) / (2 * np.pi)),
                 F32(margin), F32(gain))


def heading_index(field, theta, dtype=F32):
    """theta [P] -> (k0 int64, k1 int64, fw `dtype`, ok bool): the two slices and the weight of the second; ok is False where
    w = theta * layers_per_rad is not finite (k0 = k1 = 0 and fw = 0 stand in there)."""
    T = dtype
    n_layers = field.sd.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.asarray(theta, T) * T(field.layers_per_rad)
    ok = np.isfinite(w)
    w = np.where(ok, w, T(0))
    kf = np.floor(w)
    fw = (w - kf).astype(T)
    r = np.fmod(kf, T(n_layers))
    k0 = r.astype(np.int64)
    k0 = np.where(k0 < 0, k0 + n_layers, k0)
    k1 = np.where(k0 + 1 == n_layers, 0, k0 + 1)
    return k0, k1, fw, ok


def eval_points(field, points, dtype=F32, pose_dtype=F32):
    """points [P, 3], rounded to `pose_dtype` (fp32: what the device is handed) -> (out [P, 4] of `dtype`, choice int64 [P, 7]):
    the row per pose and the branch it took -- k0, k1, cell (i, j), in_x, in_y, and whether the row is the NaN row.  Two
    evaluations that agree on `choice` took the same piece of the (piecewise trilinear) function."""
    T = dtype
    pts = np.asarray(points, pose_dtype)
    x, y, th = (pts[:, c].astype(T) for c in range(3))
    k0, k1, fw, w_ok = heading_index(field, np.where(np.isfinite(th), th, T(0)), T)
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(th) & w_ok
    x, y = (np.where(finite, a, T(0)) for a in (x, y))
    sd = field.sd.astype(T)
    _, rows, cols = sd.shape
    x0, y0, inv_res, lpr, margin, gain, half = (T(v) for v in (field.x0, field.y0, field.inv_res, field.layers_per_rad,
                                                               field.margin, field.gain, 0.5))
    u = (x - x0) * inv_res - half
    v = (y - y0) * inv_res - half
    i, fu, in_x = sdf_ref._axis(u, cols, T)
    j, fv, in_y = sdf_ref._axis(v, rows, T)
    tap = []
    for k in (k0, k1):
        s00, s01, s10, s11 = sd[k, j, i], sd[k, j, i + 1], sd[k, j + 1, i], sd[k, j + 1, i + 1]
        a, b = s01 - s00, s11 - s10
        top, bot = s00 + fu * a, s10 + fu * b
        dv = bot - top
        tap.append((top + fv * dv, (a + fv * (b - a)) * inv_res, dv * inv_res))
    (d0, gx0, gy0), (d1, gx1, gy1) = tap
    dd = d1 - d0
    d = d0 + fw * dd
    gx = np.where(in_x, gx0 + fw * (gx1 - gx0), T(0))
    gy = np.where(in_y, gy0 + fw * (gy1 - gy0), T(0))
    gth = dd * lpr
    pen = margin - d
    out = np.stack([gain * pen, gain * (-gx), gain * (-gy), gain * (-gth)], 1).astype(T)
    out[~finite] = np.nan
    choice = np.stack([k0, k1, i, j, in_x, in_y, ~finite], 1).astype(np.int64)
    return out, choice


def same_branch(choice_a, choice_b):
    return (choice_a == choice_b).all(1)


# ---- the planner step on a layered field: the oracle's step with this model in the ONF's place -----------------------------
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
    """orc.planner_step on a layered field; `state` is updated in place."""
    tr, lam, cm, m, v, terms = optimize_trajectory(field, state["traj"], state["start"], state["goal"], state["lam"],
                                                   state["cm"], state["adam_m"], state["adam_v"], state["adam_step"], t, hp, hinv)
    state.update(traj=tr, lam=lam, cm=cm, adam_m=m, adam_v=v, adam_step=state["adam_step"] + 1)
    if state["step_count"] % reparam_freq == 0:
        tr, lam, cm = orc.reparametrize(state["traj"], state["start"], state["goal"], state["lam"], state["cm"])
        state.update(traj=tr, lam=lam, cm=cm)
    state["step_count"] += 1
    return terms
