"""Float64 restatements of the two core kernels' operations, from the model's definition, in plain numpy.

  K1  the occupancy network (nfop/onf_model.py:33-50, nfop/angle_encoder.py:15-18): logit, input gradient, the fit's pass-1
      intermediates and summed parameter gradient (nfop/nerf_opt_planner.py:83-89)
  K2  one trajectory update (nfop/constrained_nerf_opt_planner.py:63-130, nfop/nerf_opt_planner.py:143-176): the eight loss
      terms, their gradient, the banded H^-1 product, Adam, the multiplier ascent and the collision-multiplier clamp; D = 3 and
      the 2-D planner's D = 2 form

Every input is cast to float64 once and nothing is rounded to fp32 on the way: these are the values a correct fp32
evaluation approximates, whatever its summation order.  oracle/nfopp_oracle.py stays the fp32 yardstick and is not used here
(only an OnfConfig-like object with layout() / mean / sigma / ... is taken as an argument).  The optional arguments that
plant an error (`drop_unit`, `swap_grad_rows`) exist for the tests that show the float64 gate has teeth."""
import numpy as np

F64 = np.float64
HIDDEN = 100
# order of a row of the kernel's `terms` buffer (include/nfopp_hip.h)
TERMS = ("total", "l_dist", "l_col", "l_lin", "l_c2", "l_bnd", "l_cm", "l_dir")
KINK = 1e-5      # |pre-activation| below which a row counts as sitting on a ReLU kink


# ----------------------------------------------------------------------------------------------------------
# K1: occupancy network
def unpack64(params, cfg):
    flat = np.asarray(params, F64).reshape(-1)
    out, o = {}, 0
    for name, shape in cfg.layout():
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    assert o == flat.size, (o, flat.size)
    if "be" not in out:
        out["be"] = np.zeros(cfg.n_enc)
    return out


def onf_eval64(params, cfg, x, drop_unit=None):
    """-> dict of the forward and the input backward of every row of x [P, 2 | 3]:
      logit [P], grad [P, point_dim], kink [P] = min |pre-activation| over both hidden layers, and the intermediates
      u, e, z, inp, a1, h1, a2, h2, dh2, dh1, din, darg [P, feature_dim] (d logit / d encoding argument: what pass 1 of the fit
      calls `de`, positional then angle features).
    drop_unit = (row, j): PLANTED ERROR, hidden unit j of the second layer is left out of that row."""
    p = unpack64(params, cfg)
    x = np.asarray(x, F64)
    u = (x[:, :2] - cfg.mean) / cfg.sigma
    e = u @ p["we"].T + p["be"]
    feats = [np.sin(e[:, :100])]
    dfeat = [np.cos(e[:, :100])]
    if cfg.use_cos:
        feats.append(np.cos(e[:, 100:]))
        dfeat.append(-np.sin(e[:, 100:]))
    z = None
    if cfg.angle_encoding:
        k = cfg.angle_dim
        z = (x[:, 2:3] + p["ang_b"][None]) * p["ang_f"][None]
        feats += [np.sin(z[:, :k]), np.cos(z[:, k:])]
        dfeat += [np.cos(z[:, :k]), -np.sin(z[:, k:])]
    inp = np.concatenate(feats, 1)
    a1 = inp @ p["w1"].T + p["b1"]
    on1 = a1 > 0
    h1 = a1 * on1
    a2 = h1 @ p["w2"].T + p["b2"]
    on2 = a2 > 0
    if drop_unit is not None:
        on2[drop_unit] = False
    h2 = a2 * on2
    w3 = p["w3"].reshape(-1)
    logit = h2 @ w3[:HIDDEN] + inp @ w3[HIDDEN:] + p["b3"].reshape(-1)[0]
    dh2 = w3[None, :HIDDEN] * on2
    dh1 = (dh2 @ p["w2"]) * on1
    din = dh1 @ p["w1"] + w3[None, HIDDEN:]
    darg = din * np.concatenate(dfeat, 1)
    grad = darg[:, :cfg.n_enc] @ p["we"] / cfg.sigma
    if cfg.angle_encoding:
        grad = np.concatenate([grad, (darg[:, cfg.n_enc:] * p["ang_f"][None]).sum(1, keepdims=True)], 1)
    kink = np.minimum(np.abs(a1).min(1), np.abs(a2).min(1))
    return dict(logit=logit, grad=grad, kink=kink, u=u, e=e, z=z, inp=inp, a1=a1, h1=h1, a2=a2, h2=h2, dh2=dh2, dh1=dh1,
                din=din, darg=darg, p=p, x=x)


def onf_forward64(params, cfg, x):
    """float64 logit of the network whose weights are the fp32 parameters"""
    return onf_eval64(params, cfg, x)["logit"]


def fit_sums64(c, cfg, rho, rows=None, mag=False):
    """The summed parameter gradient of the fit from the per-sample values `c` of onf_eval64 and the upstream rho [P] -> flat
    gradient in cfg.layout() order.
      rows   the samples that are summed (default: all): the contribution of those samples alone
      mag    every factor of every product replaced by its absolute value (|dh1|^T |in|, sum |rho|, ...): the magnitude that
             the rounding error of an fp32 evaluation of the same sums scales with, whatever cancels in the sums themselves"""
    p = c["p"]
    f = np.abs if mag else (lambda a: a)
    sel = slice(None) if rows is None else rows
    rho = np.asarray(rho, F64)[sel]
    r = rho[:, None]
    h1, h2, inp, u = (f(c[k][sel]) for k in ("h1", "h2", "inp", "u"))
    dh2, dh1, de = f(r * c["dh2"][sel]), f(r * c["dh1"][sel]), r * c["darg"][sel]
    den = f(de[:, :cfg.n_enc])
    rho = f(rho)
    g = dict(w3=rho @ np.concatenate([h2, inp], 1), b3=rho.sum(keepdims=True), w2=dh2.T @ h1, b2=dh2.sum(0),
             w1=dh1.T @ inp, b1=dh1.sum(0), we=den.T @ u, be=den.sum(0))
    if cfg.angle_encoding:
        dz = f(de[:, cfg.n_enc:])
        g["ang_b"] = (dz * f(p["ang_f"])[None]).sum(0)
        g["ang_f"] = (dz * f(c["x"][sel, 2:3] + p["ang_b"][None])).sum(0)
    return np.concatenate([np.asarray(g[name]).reshape(-1) for name, _ in cfg.layout()])


def onf_fit64(params, cfg, x, labels, keep_eval=False):
    """The fit's step on P samples (mean BCE with logits) -> dict:
      loss, rho [P] = (sigmoid(logit) - y) / P, the pass-1 factors h1 [P, 100], rho_dh1 [P, 100], rho_de [P, feature_dim],
      grad = the flat parameter gradient in cfg.layout() order, and kink / a2 / u of onf_eval64.
    keep_eval: also `eval` = the dict of onf_eval64 and `loss_p` [P], the per-sample losses (what fit_sums64 takes)."""
    c = onf_eval64(params, cfg, x)
    y = np.asarray(labels, F64)
    P = len(y)
    logit = c["logit"]
    loss_p = np.maximum(logit, 0) - logit * y + np.log1p(np.exp(-np.abs(logit)))
    loss = np.mean(loss_p)
    rho = (1.0 / (1.0 + np.exp(-logit)) - y) / P
    r = rho[:, None]
    out = dict(loss=loss, rho=rho, h1=c["h1"], rho_dh1=r * c["dh1"], rho_de=r * c["darg"], grad=fit_sums64(c, cfg, rho),
               kink=c["kink"], a2=c["a2"], u=c["u"], logit=logit)
    if keep_eval:
        out.update(eval=c, loss_p=loss_p)
    return out


# ----------------------------------------------------------------------------------------------------------
# K2: one trajectory update
def wrap64(a):
    return np.remainder(a + np.pi, 2 * np.pi) - np.pi


def _softplus(logit, beta):
    """torch softplus with its threshold of 20 and its derivative"""
    bl = logit * beta
    lin = bl > 20
    z = np.exp(np.where(lin, 0.0, bl))
    return np.where(lin, logit, np.log1p(z) / beta), np.where(lin, 1.0, z / (z + 1.0))


def traj_loss64(s, hp):
    """Loss terms and their gradient for the state s (arrays traj [B, N, D], start, goal, t [B, N-1], onf [B, N-1, 4] = logit and
    d logit / d pose of the collision samples, and for D = 3 lam [B, N+1], cm [B, N]); hp has the fields of TrajectoryHyper.
    -> (terms {name: [B]}, g_traj [B, N, D], g_lam [B, N+1] | None, g_cm [B, N] | None)"""
    traj, start, goal, t, onf = (np.asarray(s[k], F64) for k in ("traj", "start", "goal", "t", "onf"))
    B, N, D = traj.shape
    logit, dlogit = onf[..., 0], onf[..., 1:1 + D]
    q = np.concatenate([start[:, None], traj, goal[:, None]], 1)
    G = np.zeros_like(q)
    zero = np.zeros(B)
    sp, dsp = _softplus(logit, hp.collision_beta)
    l_col = sp.sum(1)
    if D == 2:
        delta = q[:, 1:] - q[:, :-1]
        l_dist = (delta ** 2).sum((1, 2))
        G[:, 1:] += 2 * delta
        G[:, :-1] -= 2 * delta
        gg = (hp.collision_weight * dsp)[..., None] * dlogit
        G[:, 1:-2] += t[..., None] * gg
        G[:, 2:-1] += (1 - t)[..., None] * gg
        terms = dict(total=l_dist + hp.collision_weight * l_col, l_dist=l_dist, l_col=l_col, l_lin=zero, l_c2=zero, l_bnd=zero,
                     l_cm=zero, l_dir=zero)
        return terms, G[:, 1:-1], None, None
    lam, cm = np.asarray(s["lam"], F64), np.asarray(s["cm"], F64)
    aw = hp.angle_weight
    # distance: raw heading differences, the winding constant on the last segment, headings scaled by angle_weight
    delta = q[:, 1:] - q[:, :-1]
    delta[:, -1, 2] += wrap64(delta[..., 2]).sum(1) - q[:, -1, 2] + q[:, 0, 2]
    delta[..., 2] *= aw
    l_dist = (delta ** 2).sum((1, 2))
    gd = 2 * delta
    gd[..., 2] *= aw
    G[:, 1:] += gd
    G[:, :-1] -= gd
    # non-holonomic constraint with its multipliers
    dx, dy, th = q[:, 1:, 0] - q[:, :-1, 0], q[:, 1:, 1] - q[:, :-1, 1], q[..., 2]
    m = th[:, :-1] + wrap64(th[:, 1:] - th[:, :-1]) / 2
    sm, cmm = np.sin(m), np.cos(m)
    c = dx * sm - dy * cmm
    e = dx * cmm + dy * sm
    g = lam + 2 * hp.constraint_deltas_weight * c
    G[:, 1:, 0] += g * sm
    G[:, :-1, 0] -= g * sm
    G[:, 1:, 1] -= g * cmm
    G[:, :-1, 1] += g * cmm
    G[:, :-1, 2] += g * e / 2
    G[:, 1:, 2] += g * e / 2
    # forward-only direction term
    mp = th[:, :-1] + wrap64(th[:, :-1] - th[:, 1:]) / 2
    smp, cmp_ = np.sin(mp), np.cos(mp)
    r = np.maximum(-(cmp_ * dx + smp * dy), 0)
    hh = 2 * hp.direction_delta_weight * r
    k = smp * dx - cmp_ * dy
    G[:, 1:, 0] -= hh * cmp_
    G[:, :-1, 0] += hh * cmp_
    G[:, 1:, 1] -= hh * smp
    G[:, :-1, 1] += hh * smp
    G[:, :-1, 2] += 1.5 * hh * k
    G[:, 1:, 2] -= 0.5 * hh * k
    # boundary, interior waypoints only
    lo_x, hi_x, lo_y, hi_y = hp.bounds
    x, y = traj[..., 0], traj[..., 1]
    bx0, bx1, by0, by1 = np.maximum(lo_x - x, 0), np.maximum(x - hi_x, 0), np.maximum(lo_y - y, 0), np.maximum(y - hi_y, 0)
    l_bnd = (bx0 ** 2 + bx1 ** 2 + by0 ** 2 + by1 ** 2).sum(1)
    G[:, 1:-1, 0] += 2 * hp.boundary_weight * (bx1 - bx0)
    G[:, 1:-1, 1] += 2 * hp.boundary_weight * (by1 - by0)
    # collision: softplus of the logits and the multiplier term on tanh
    th_l = np.tanh(logit)
    cm_i = cm[:, 1:] * (1 - t) + cm[:, :-1] * t
    gg = (hp.collision_weight * dsp + cm_i * (1 - th_l * th_l))[..., None] * dlogit
    G[:, 1:-2] += t[..., None] * gg
    G[:, 2:-1] += (1 - t)[..., None] * gg
    g_cm = np.zeros_like(cm)
    g_cm[:, 1:] += (1 - t) * th_l
    g_cm[:, :-1] += t * th_l
    terms = dict(l_dist=l_dist, l_col=l_col, l_lin=(lam * c).sum(1), l_c2=(c * c).sum(1), l_bnd=l_bnd, l_cm=(cm_i * th_l).sum(1),
                 l_dir=(r * r).sum(1))
    terms["total"] = (terms["l_dist"] + hp.collision_weight * l_col + terms["l_lin"] + hp.constraint_deltas_weight * terms["l_c2"]
                      + hp.boundary_weight * l_bnd + terms["l_cm"] + hp.direction_delta_weight * terms["l_dir"])
    return terms, G[:, 1:-1], c, g_cm


def band_product64(band, half_width, g):
    """out[b, i] = sum_k band[k, i] * g[b, i + k - W]: the product with the band as it is stored (fp32 values of the band of the
    fp32 inverse), not with the full inverse"""
    band = np.asarray(band, F64)
    W, (B, N, D) = half_width, g.shape
    assert band.shape == (2 * W + 1, N)
    gp = np.zeros((B, N + 2 * W, D))
    gp[:, W:W + N] = g
    out = np.zeros_like(g)
    for k in range(2 * W + 1):
        out += band[k][None, :, None] * gp[:, k:k + N]
    return out


def traj_update64(s, band, half_width, hp, adam_step, swap_grad_rows=None):
    """One nfopp_traj_update call on the state s (see traj_loss64; plus adam_m, adam_v [B, N, D]) -> {traj, adam_m, adam_v,
    lam, cm (D = 3), terms [B, 8]} after it.  adam_step is the 1-based count of the step being taken, as
    TrajectoryHyper.to_c takes it.
    swap_grad_rows = (b, w): PLANTED ERROR, the gradient rows of waypoints w and w + 1 of trajectory b change places."""
    terms, g, g_lam, g_cm = traj_loss64(s, hp)
    if swap_grad_rows is not None:
        b, w = swap_grad_rows
        g = g.copy()
        g[b, [w, w + 1]] = g[b, [w + 1, w]]
    g = band_product64(band, half_width, g)
    traj, m, v = (np.asarray(s[k], F64) for k in ("traj", "adam_m", "adam_v"))
    b1, b2 = hp.betas
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** adam_step) + hp.eps
    out = dict(traj=traj - hp.lr / (1 - b1 ** adam_step) * (m / denom), adam_m=m, adam_v=v,
               terms=np.stack([terms[k] for k in TERMS], 1))
    if g_lam is not None:
        out["lam"] = np.asarray(s["lam"], F64) + hp.multipliers_lr * g_lam
        out["cm"] = np.maximum(np.asarray(s["cm"], F64) + hp.collision_multipliers_lr * g_cm, 0)
    return out
