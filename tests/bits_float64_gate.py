"""The float64 gate of the K1 / K2 bit fixtures: the inputs of every recorded case rebuilt on the CPU, their float64 values
(tests/float64_ref.py), the fp32 oracle's values on the same inputs, and the comparer that tests/test_bits_float64_cpu.py
applies to the recorded arrays and tests/test_gpu_bits_float64.py to live device output.

The gate of an array:   max |got - float64|  <=  8 x max(max |oracle32 - float64|, one fp32 ulp of the array's scale)

  the yardstick is the project's fp32 oracle on the same case and the same array, measured, not chosen: two correct fp32
  evaluations differ by the summation order over at most 220 inputs (K1) or 185 band taps (K2), which the factor 8 covers
  (the recorded fixtures are within 3.6 x the oracle's own error, profiles/bits_float64.txt); a wrong tap, hidden unit or
  step count is two or more orders above the fp32 error
  K1 scale   the largest |float64 value| of that quantity over all cases of the network in the fixture (a P = 1 case is not
             scaled by its single value)
  K2 scale   the array's own largest |float64 value|; errors are absolute, the scale only sets the floor
  caps       a gate is never looser than the one tests/test_gpu_parity.py holds the same quantity to: PARITY

ReLU kinks: a row whose float64 |pre-activation| minimum is below float64_ref.KINK may differ by one hidden unit's whole
gradient contribution between two correct fp32 evaluations; it may be left out of the gradient and factor comparisons (its
logit stays gated).  That is a condition on the cases, not a measurement: at most KINK_ROWS of a case's rows, none of an edge
case.  With 200 hidden units about 1 row in 100 is that near a kink -- more than the cap admits -- so kink_free() leaves out
the rows nearest a kink up to the cap (none of a case below 200 rows) and every other row stays gated."""
import collections

import numpy as np
import torch

import nfopp
from oracle import nfopp_oracle as orc

import float64_ref as f64
import k1_bits_cases as kc
import k1_kind_bits_cases as kk
import k2_bits_cases as k2

F32 = np.float32
FACTOR = 8.0
KINK_ROWS = 0.005
# tests/test_gpu_parity.py: logit 1e-5 and gradient 5e-5 of the output scale; one step moves traj by 2e-6 at most, adam_m by
# 1e-5 and adam_v by 2e-5 of their scale (default hyper block: lr = 1e-2, coordinates within 3.1)
PARITY = dict(logit=1e-5, grad=5e-5, traj=2e-6, adam_m=1e-5, adam_v=2e-5)
PARITY_TRAJ_SCALE, PARITY_LR = 3.1, 1e-2

Row = collections.namedtuple("Row", "family case array scale orc_err got_err bound ok")


def ratio(row):
    """the device's (or fixture's) error in units of the oracle's, the floor of one ulp included"""
    return row.got_err / max(row.orc_err, float(np.spacing(F32(row.scale))), 1e-300)


def gate(rows, family, case, array, got, want, orc32, scale, cap=None, keep=None):
    """appends the measured pair of one array to `rows`; `keep` = the rows that are compared, `cap` = absolute upper limit of
    the bound"""
    got, want, orc32 = (np.asarray(a, np.float64) for a in (got, want, orc32))
    assert got.shape == want.shape == orc32.shape, (case, array, got.shape, want.shape, orc32.shape)
    if keep is not None:
        got, want, orc32 = got[keep], want[keep], orc32[keep]
    got_err = float(np.abs(got - want).max()) if got.size else 0.0
    orc_err = float(np.abs(orc32 - want).max()) if got.size else 0.0
    bound = FACTOR * max(orc_err, float(np.spacing(F32(scale))))
    if cap is not None:
        bound = min(bound, cap)
    rows.append(Row(family, case, array, float(scale), orc_err, got_err, bound, bool(np.isfinite(got).all() and got_err <= bound)))


def fact(rows, family, case, what, holds):
    """a structural fact of a recorded array (exact: no tolerance)"""
    rows.append(Row(family, case, what, 0.0, 0.0, 0.0 if holds else np.inf, 0.0, bool(holds)))


def failures(rows):
    return ["%s %s: |err| %.3g > %.3g (oracle32 %.3g, scale %.3g)" % (r.case, r.array, r.got_err, r.bound, r.orc_err, r.scale)
            for r in rows if not r.ok]


def summary(rows):
    """per case family and array: the largest oracle32 and fixture / device error (of scale) and the worst ratio"""
    groups = collections.OrderedDict()
    for r in rows:
        if r.scale > 0:
            groups.setdefault((r.family, r.array), []).append(r)
    lines = ["%-28s %-8s %5s %12s %12s %7s" % ("family", "array", "cases", "oracle32", "got", "ratio")]
    for (family, array), rs in groups.items():
        lines.append("%-28s %-8s %5d %12.3g %12.3g %7.2f" % (family, array, len(rs), max(r.orc_err / r.scale for r in rs),
                                                          max(r.got_err / r.scale for r in rs), max(ratio(r) for r in rs)))
    return lines


def worst_ratio(rows):
    return max([ratio(r) for r in rows if r.scale > 0] or [0.0])


# ----------------------------------------------------------------------------------------------------------
# K1
def cpu_network(fin):
    """the network of kc.make_onf(fin), built on the CPU under the same seed -> (flat fp32 parameters, oracle config)"""
    use_cos, angle, bias = kc.DIMS[fin]
    torch.random.manual_seed(1000 + fin)
    onf = nfopp.ONF(0.4, 2.5, use_cos=use_cos, use_normal_init=True, bias=bias, angle_encoding=angle)
    return onf.flat_parameters.detach().cpu().numpy().astype(F32), orc.OnfConfig(0.4, 2.5, use_cos, bias, angle)


def _traj_poses(fin, seed, B, N):
    """the sample poses of a module's _traj(): its draws restated, the poses formed in fp32 as the oracle forms them (that
    rounding is pinned bit for bit by tests/test_gpu_parity.py)"""
    D = 3 if kc.DIMS[fin][1] else 2
    rng = np.random.default_rng(seed)
    traj = rng.uniform(-4, 6, (B, N, D)).astype(F32)
    if D == 3:
        traj[:, :, 2] = rng.uniform(-3.3, 3.3, (B, N)).astype(F32)
    t = rng.uniform(0, 1, (B, N - 1)).astype(F32)
    return (orc.sample_collision_points(traj, t) if D == 3 else orc.sample_collision_points_2d(traj, t)).reshape(-1, D)


def big_rows(n):
    return np.concatenate([np.arange(0, n, kc.BIG_STRIDE), np.arange(n - kc.BIG_TAIL, n)])


def k1_inputs(mod, big_count=None):
    """{case name: (kind, fin, poses [P, 2 | 3] fp32, labels | None)} of every value-holding case of a case module, in the
    order of its run_cases(); kind is pose / edge / traj / logits / big / fit"""
    out = collections.OrderedDict()
    own = mod is kc
    for fin in mod.DIMS:
        for P in mod.POSE_P:
            out["pose_F%d_P%d" % (fin, P)] = ("pose", fin, kc.points(fin, P, (100 if own else 1100) + fin + P), None)
        if not own:
            out["edge_F%d" % fin] = ("edge", fin, kk.edge_poses(fin), None)
        if own or fin in kk.TRAJ_DIMS:
            out["traj_F%d" % fin] = ("traj", fin, _traj_poses(fin, 300 + fin, 3, 9) if own else _traj_poses(fin, 600 + fin, 2, 5), None)
        if own:
            out["logits_F%d" % fin] = ("logits", fin, kc.points(fin, 257, 200 + fin), None)
        if fin in mod.FIT_DIMS:
            for P in (kc.FIT_P if own else (kk.FIT_P,)):
                y = (np.random.default_rng(700 + fin + P).uniform(size=P) < 0.35).astype(F32)
                out["fit_F%d_P%d" % (fin, P)] = ("fit", fin, kc.points(fin, P, 500 + fin + P), y)
        if own and fin == 220 and big_count is not None:
            out["big_rows"] = ("big", fin, kc.points(fin, int(big_count), 900)[big_rows(int(big_count))], None)
    return out


def _oracle_fit32(flat, cfg, x, y):
    """the oracle's pass-1 intermediates in fp32 (nfop/nerf_opt_planner.py:83-89 unrolled, as orc.onf_train_grads forms them)"""
    p = orc.unpack_params(flat, cfg)
    logit, c = orc._onf_forward_cache(p, cfg, x)
    rho = ((orc.sigmoid(logit) - y) / F32(len(y))).astype(F32)
    w3, e = p["w3"][0], c["e"]
    dh2 = (rho[:, None] * w3[None, :100] * (c["a2"] > 0)).astype(F32)
    dh1 = ((dh2 @ p["w2"]) * (c["a1"] > 0)).astype(F32)
    din = (dh1 @ p["w1"] + rho[:, None] * w3[None, 100:]).astype(F32)
    de = [din[:, :100] * np.cos(e[:, :100])] + ([-din[:, 100:200] * np.sin(e[:, 100:])] if cfg.use_cos else [])
    if cfg.angle_encoding:
        z, k, n = c["z"], cfg.angle_dim, cfg.n_enc
        de += [din[:, n:n + k] * np.cos(z[:, :k]), -din[:, n + k:] * np.sin(z[:, k:])]
    return dict(h1=c["h1"], rho=rho, rho_dh1=dh1, rho_de=np.concatenate(de, 1).astype(F32), u=c["u"])


def k1_reference(mod, big_count=None, plant=None, only=None):
    """float64 and oracle32 values of every case of k1_inputs(mod), or of the cases named in `only` -> {name: dict}.
    plant = (case name, keyword arguments of f64.onf_eval64) | (case name, "theta", row): a PLANTED ERROR in that case's
    float64 values"""
    nets = {fin: cpu_network(fin) for fin in mod.DIMS}
    ref = collections.OrderedDict()
    for name, (kind, fin, x, y) in k1_inputs(mod, big_count).items():
        if only is not None and name not in only:
            continue
        flat, cfg = nets[fin]
        r = dict(kind=kind, fin=fin, x=x, y=y)
        if kind == "fit":
            r["f64"] = f64.onf_fit64(flat, cfg, x, y)
            r["o32"] = _oracle_fit32(flat, cfg, x, y)
            r["o32_loss"], _, r["o32_grad"] = orc.onf_train_grads(flat, cfg, x, y)
            r["kink"] = r["f64"]["kink"]
        else:
            kw, xe = {}, x
            if plant is not None and plant[0] == name:
                if plant[1] == "theta":
                    xe = x.copy()
                    xe[plant[2], 2] = -xe[plant[2], 2]
                else:
                    kw = plant[1]
            c = f64.onf_eval64(flat, cfg, xe, **kw)
            r["logit"], r["grad"], r["kink"], r["c"] = c["logit"], c["grad"], c["kink"], c
            r["o32_logit"], r["o32_grad"] = orc.onf_forward_grad(flat, cfg, x)
        ref[name] = r
    return ref


def kink_free(r):
    """rows of a case that are compared in gradients and factors; the caps on the others are part of the gate"""
    kink = r["kink"]
    cap = 0 if r["kind"] == "edge" else int(KINK_ROWS * len(kink))
    keep = np.ones(len(kink), bool)
    nearest = np.argsort(kink, kind="stable")[:cap]        # about 1 row in 100 is below KINK: more than the cap admits, so
    keep[nearest[kink[nearest] < f64.KINK]] = False        # the rows nearest a kink go first and the others stay gated
    return keep


def k1_scales(ref):
    """{fin: (logit scale, gradient scale)} over all output cases of the network"""
    s = {}
    for r in ref.values():
        if r["kind"] != "fit":
            a, b = s.get(r["fin"], (0.0, 0.0))
            s[r["fin"]] = (max(a, float(np.abs(r["logit"]).max())), max(b, float(np.abs(r["grad"]).max())))
    return s


def _own_scale(a):
    return max(float(np.abs(a).max()), 1e-30)


def compare_k1(tag, arrays, ref, only=None):
    """every value-holding array of `arrays` (fixture or run_cases() output, {name: array}) against `ref` -> [Row]"""
    rows = []
    scales = k1_scales(ref)
    for name, r in ref.items():
        if only is not None and name not in only:
            continue
        fin, kind = r["fin"], r["kind"]
        family = "%s %s_F%d" % (tag, kind, fin)
        d = 3 if kc.DIMS[fin][1] else 2
        keep = kink_free(r)
        if kind == "fit":
            _compare_fit(rows, family, name, arrays, r, keep)
            continue
        out = np.asarray(arrays[name]).reshape(-1, 4)
        sl, sg = scales[fin]
        gate(rows, family, name, "logit", out[:, 0], r["logit"], r["o32_logit"], sl, cap=PARITY["logit"] * sl)
        if kind == "logits":       # the forward-only kernel writes the logit alone
            fact(rows, family, name, "columns 1..3 are zero", np.all(out[:, 1:] == 0))
            continue
        gate(rows, family, name, "grad", out[:, 1:1 + d], r["grad"], r["o32_grad"], sg, cap=PARITY["grad"] * sg, keep=keep)
        if d == 2:
            fact(rows, family, name, "column 3 is zero (2-D network)", np.all(out[:, 3] == 0))
    return rows


def _compare_fit(rows, family, name, arrays, r, keep):
    """pass 1 of the fit: h1 [P,112] | rho dh1 [P,112] | rho de [P,16*NKB] | record [P,12] (layout: tests/test_gpu_split_path.py,
    test_fit_pass1_factors_on_the_32x32_kernel_vs_oracle); P = 257 is recorded for the rows kc.BIG_FIT_ROWS"""
    fin, x = r["fin"], r["x"]
    P = len(x)
    sel = np.arange(P) if P == 33 else kc.BIG_FIT_ROWS
    suffix = "" if P == 33 else "_rows"
    h1, dh1, de, rec = (np.asarray(arrays["%s_%s%s" % (name, k, suffix)]) for k in ("h1", "dh1", "de", "rec"))
    want, o32, keep = r["f64"], r["o32"], keep[sel]
    gate(rows, family, name, "h1", h1[:, :100], want["h1"][sel], o32["h1"][sel], _own_scale(want["h1"]))
    gate(rows, family, name, "rho", dh1[:, 100], want["rho"][sel], o32["rho"][sel], _own_scale(want["rho"]))
    gate(rows, family, name, "rec.rho", rec[:, 4], want["rho"][sel], o32["rho"][sel], _own_scale(want["rho"]))
    gate(rows, family, name, "rho_dh1", dh1[:, :100], want["rho_dh1"][sel], o32["rho_dh1"][sel], _own_scale(want["rho_dh1"]), keep=keep)
    gate(rows, family, name, "rho_de", de[:, :fin], want["rho_de"][sel], o32["rho_de"][sel], _own_scale(want["rho_de"]), keep=keep)
    fact(rows, family, name, "h1[:, 101] == 1", np.all(h1[:, 101] == 1.0))
    fact(rows, family, name, "pad positions of de are zero", np.all(de[:, fin + 1:] == 0.0))
    u = o32["u"][sel]       # u = (x - mean) / sigma formed in fp32: the record holds it exactly
    fact(rows, family, name, "record u is exact", np.array_equal(rec[:, 0], u[:, 0]) and np.array_equal(rec[:, 1], u[:, 1]))
    fact(rows, family, name, "record ones column", np.all(rec[:, 2] == 1.0))
    theta = x[sel, 2] if kc.DIMS[fin][1] else np.zeros(len(sel), F32)
    fact(rows, family, name, "record theta is exact", np.array_equal(rec[:, 3].view(np.uint32), theta.view(np.uint32)))
    words = np.ascontiguousarray(rec[:, 8:12]).view(np.uint32)
    s = np.arange(100)
    bits = ((words[:, (s >> 2) & 3] >> (4 * (s >> 4) + (s & 3))) & 1).astype(bool)
    fact(rows, family, name, "record sign bits of a2", np.array_equal(bits[keep], (want["a2"][sel] > 0)[keep]))
    fact(rows, family, name, "record words end at bit 28", not (words >> 28).any())


def compare_fit_grad(tag, name, g, r):
    """the fit's summed gradient g [n_params + 2] (gradient | loss | count) against the float64 gradient -> [Row]"""
    rows = []
    family = "%s fitgrad_F%d" % (tag, r["fin"])
    want = r["f64"]
    gate(rows, family, name, "grad", g[:-2], want["grad"], r["o32_grad"], _own_scale(want["grad"]))
    gate(rows, family, name, "loss", g[-2:-1], [want["loss"]], [r["o32_loss"]], abs(float(want["loss"])))
    fact(rows, family, name, "sample count", g[-1] == len(r["x"]))
    return rows


# ----------------------------------------------------------------------------------------------------------
# K2
def _band_product32(band, W, g):
    g = np.asarray(g, F32)
    B, N, D = g.shape
    gp = np.zeros((B, N + 2 * W, D), F32)
    gp[:, W:W + N] = g
    acc = np.zeros_like(g)
    for k in range(2 * W + 1):
        acc = (acc + band[k][None, :, None] * gp[:, k:k + N]).astype(F32)
    return acc


def k2_oracle32(case):
    """one update of the case by the fp32 oracle: orc.trajectory_loss_terms (D = 2: orc.trajectory_loss_2d, whose softplus has
    beta = 1, on beta * logit), the product with the same band, orc.adam_update, the ascent of orc.optimize_trajectory"""
    n, weight, d = case
    s, hp = k2.inputs(case), k2.HYPER
    band, W, _ = k2.band(n, weight)
    if d == 3:
        oh = orc.Hyper(hp.collision_weight, hp.angle_weight, hp.constraint_deltas_weight, hp.multipliers_lr, hp.collision_multipliers_lr,
                       hp.boundary_weight, hp.collision_beta, hp.direction_delta_weight, hp.lr, hp.betas[0], hp.betas[1], hp.eps, hp.bounds)
        tm = orc.trajectory_loss_terms(s["traj"], s["start"], s["goal"], s["lam"], s["cm"], s["t"], s["onf"][..., 0], s["onf"][..., 1:], oh)
        terms = np.stack([tm[k] for k in f64.TERMS], 1)
    else:
        beta = F32(hp.collision_beta)
        tm = orc.trajectory_loss_2d(s["traj"], s["start"], s["goal"], s["t"], (s["onf"][..., 0] * beta).astype(F32), s["onf"][..., 1:3],
                                    hp.collision_weight)
        l_col = (tm["l_col"] / beta).astype(F32)
        zero = np.zeros(k2.B, F32)
        terms = np.stack([(tm["l_dist"] + F32(hp.collision_weight) * l_col).astype(F32), tm["l_dist"], l_col] + [zero] * 5, 1)
    g = _band_product32(band, W, tm["g_traj"])
    traj, m, v = orc.adam_update(s["traj"], g, s["adam_m"], s["adam_v"], k2.ADAM_STEP, hp.lr, hp.betas[0], hp.betas[1], hp.eps)
    out = dict(traj=traj, adam_m=m, adam_v=v, terms=terms)
    if d == 3:
        out["lam"] = (s["lam"] + F32(hp.multipliers_lr) * tm["g_lam"]).astype(F32)
        cm = (s["cm"] + F32(hp.collision_multipliers_lr) * tm["g_cm"]).astype(F32)
        out["cm"] = np.where(cm > 0, cm, F32(0)).astype(F32)
    return out


def k2_reference(case, band=None, adam_step=k2.ADAM_STEP, **plant):
    """float64 values of the case after one update; `band`, `adam_step` and `plant` differ from the case's own only where a
    test plants an error"""
    n, weight, _ = case
    own, W, _ = k2.band(n, weight)
    return f64.traj_update64(k2.inputs(case), own if band is None else band, W, k2.HYPER, adam_step, **plant)


def k2_cap(name, scale):
    """the parity gate of the quantity carried to the case's conditions: traj moves by lr x (a quotient of order one) and is
    stored at the coordinates' magnitude, so the 2e-6 measured at lr = 1e-2 within 3.1 scales with both; the moments' gates
    are relative already"""
    if name == "traj":
        return PARITY["traj"] * max(1.0, scale / PARITY_TRAJ_SCALE) * max(1.0, k2.HYPER.lr / PARITY_LR)
    return PARITY[name] * scale if name in PARITY else None


def compare_k2(tag, case, arrays, want, o32, names=None, rows_of=None):
    """the arrays of one case ({name: array}) against float64 -> [Row]; rows_of = the trajectories that are compared"""
    rows = []
    family = "%s D%d" % (tag, case[2])
    sel = slice(None) if rows_of is None else rows_of
    for k in (k2.arrays_of(case) if names is None else names):
        got, w, o = np.asarray(arrays[k])[sel], want[k][sel], o32[k][sel]
        if k == "terms":
            for j, term in enumerate(f64.TERMS):
                scale = float(np.abs(want[k][:, j]).max())
                if scale == 0:
                    fact(rows, family, k2.tag(case), "%s is zero" % term, np.all(got[:, j] == 0))
                else:
                    gate(rows, family, k2.tag(case), term, got[:, j], w[:, j], o[:, j], scale)
        else:
            scale = _own_scale(want[k])
            gate(rows, family, k2.tag(case), k, got, w, o, scale, cap=k2_cap(k, scale))
    return rows


def fixture_rows():
    """the measured pairs of the three committed fixtures (what profiles/bits_float64.txt lists)"""
    from conftest import load_golden
    out = collections.OrderedDict()
    z = load_golden("k1_bits.npz")
    out["k1_bits.npz"] = compare_k1("k1_bits", z, k1_reference(kc, int(z["big_count"])))
    out["k1_kind_bits.npz"] = compare_k1("k1_kind", load_golden("k1_kind_bits.npz"), k1_reference(kk))
    z = load_golden("k2_bits.npz")
    rows = []
    for case in k2.CASES:
        got = {k: z["%s_%s" % (k2.tag(case), k)] for k in k2.arrays_of(case)}
        rows += compare_k2("k2_bits", case, got, k2_reference(case), k2_oracle32(case))
    out["k2_bits.npz"] = rows
    return out


if __name__ == "__main__":
    for name, rows in fixture_rows().items():
        print("%s: %d arrays, worst ratio %.2f, %d outside the gate" % (name, len(rows), worst_ratio(rows), len(failures(rows))))
        print("\n".join(summary(rows)))
        for r in sorted((r for r in rows if r.scale > 0), key=ratio)[-3:]:
            print("   worst: %s %s  oracle32 %.3g  fixture %.3g  ratio %.2f" % (r.case, r.array, r.orc_err, r.got_err, ratio(r)))
        print("\n".join(failures(rows)))
