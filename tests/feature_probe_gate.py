"""The gate of the feature probes (tests/feature_probe_cases.py): fp32 emulations of the two device sines in numpy, a model of
what a probe reads out of a network through its skip weights, and the comparer that tests/test_feature_probe_cpu.py applies
to planted errors and tests/test_gpu_feature_probe.py to device output.

  hw_revolutions  the hardware chain in the order of csrc/common.h sin_halfturns_hw (the same chain is written out in
                  eval_item / eval_angle_item / eval_any_item of csrc/onf_x32_impl.h, twice in csrc/onf_split.hip and in pass 2
                  of csrc/onf_wgrad.hip): every fma a float64 product and sum rounded once to fp32.  Its result is the
                  revolutions f handed to v_sin_f32; hw_sine = sin(2 pi f) in float64 stands for a perfect v_sin_f32
  sin_quadrant    the polynomial form of csrc/common.h, what the per-sample fit (csrc/onf_train.hip) evaluates

The gate of a probed value with float64 reference r and emulation e, u = 2^-24:

  MFMA paths        |dev - r| <= |e - r| + 2 V + 2 u     V = 1.25e-7: max |v_sin_f32(f) - sin(2 pi f)| as recorded for gfx950
                                                         (tools/micro/vsin_accuracy.hip); the factor 2
                                                         covers inputs that tool's 4 M-point grid did not visit
  per-sample path   |dev - r| <= |e - r| + 2 u           no hardware sine
  2 u               one rounding each in the readout's product and sum (values of magnitude <= 1)

A value read out through an operand of weight w (d logit / d pose = s' w) is held to the same gate in units of w:
|dev - w r| <= |w| (|e - r| + 2 V) + 2 u max(1, |w|): the one product s' w rounds relative to its own magnitude.

Condition on the cases, asserted on the CPU: |e - r| <= CAP = 1e-6 for every probe argument, so the yardstick cannot grow to
hide a failure.  PLANTS are the errors the CPU test puts into the model to show that the comparer rejects them."""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
V = 1.25e-7
U = 2.0 ** -24
CAP = 1e-6
MFMA, PER_SAMPLE = "mfma", "per-sample"
DECADES = ("[0, 1)", "[1, 10)", "[10, 1e2)", "[1e2, 1e3)", "[1e3, 1e4)", "[1e4, 1e5)")
OFFSETS = ("0", "1/4", "1/2")          # turns added to the argument: sine kinds, cosine kinds = derivative of sine, derivative of cosine

# the planted errors of tests/test_feature_probe_cpu.py
DROP_LO = "a: the second reduction constant is dropped"
HI_ULP = "b: the first 2 pi constant is one fp32 ulp high"
COS_AS_SIN = "c: the first position of the cosine block is evaluated as a sine"
SWAP = "d: the table entries of two neighbouring positions are swapped"
ANGLE_FORM = "e: the angle argument is formed as theta * fr + b"
DERIV_BACK = "f: the derivative is taken a quarter turn backward"
PLANTS = (DROP_LO, HI_ULP, COS_AS_SIN, SWAP, ANGLE_FORM, DERIV_BACK)

INV_2PI = F32(0.159154943)
MAGIC = F32(12582912.0)
TWO_PI_HI = F32(6.28318548202514648)
TWO_PI_LO = F32(1.74845553e-07)


def fma32(a, b, c):
    """fma in fp32: the float64 product of two fp32 values is exact, the sum is rounded once to float64 (far below an fp32 ulp)
    and once to fp32"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def hw_revolutions(x, qq, plant=None):
    """sin_halfturns_hw up to the v_sin_f32: fp32 argument x, offset qq in revolutions -> the fp32 revolutions"""
    x = np.asarray(x, F32)
    jm = fma32(x, INV_2PI, MAGIC)
    j = (jm - MAGIC).astype(F32)
    hi = np.nextafter(TWO_PI_HI, F32(np.inf)) if plant == HI_ULP else TWO_PI_HI
    r = fma32(j, -hi, x)
    if plant != DROP_LO:
        r = fma32(j, TWO_PI_LO, r)
    return fma32(r, INV_2PI, np.asarray(qq, F32))


def hw_sine(x, q, plant=None):
    """the hardware chain with a perfect v_sin_f32: float64 sin(2 pi f); q = quarter turns added to the argument"""
    f = hw_revolutions(x, (np.asarray(q, F64) * 0.25).astype(F32), plant)
    return np.sin(2.0 * np.pi * f.astype(F64))


def sin_quadrant(x, q):
    """fp32 emulation of csrc/common.h sin_quadrant(x, q) = sin(x + q pi/2), q integer"""
    x = np.asarray(x, F32)
    j = np.rint((x * F32(0.636619772)).astype(F32)).astype(F32)
    r = fma32(j, F32(-1.57079601e+00), x)
    r = fma32(j, F32(-3.13916473e-07), r)
    r = fma32(j, F32(-5.39030253e-15), r)
    n = j.astype(np.int64) + q
    s = (r * r).astype(F32)
    ps = fma32(fma32(fma32(np.full_like(x, F32(2.86567956e-6)), s, F32(-1.98559923e-4)), s, F32(8.33338592e-3)), s, F32(-1.66666672e-1))
    sv = fma32(ps, (r * s).astype(F32), r)
    pc = fma32(fma32(fma32(np.full_like(x, F32(2.44677067e-5)), s, F32(-1.38877297e-3)), s, F32(4.16666567e-2)), s, F32(-0.5))
    cv = fma32(pc, s, F32(1))
    res = np.where(n & 1, cv, sv)
    return np.where(n & 2, -res, res).astype(F32)


def poly_sine(x, q, plant=None):
    """the per-sample path's sine, as float64 values (it has no reduction constants of the hardware chain to plant into)"""
    q = np.broadcast_to(np.asarray(q, np.int64), np.shape(x))
    return sin_quadrant(x, q).astype(F64)


def ref_sine(a, q):
    """the reference: plain float64 sin(a + q pi/2)"""
    return np.sin(np.asarray(a, F64) + np.asarray(q, F64) * (np.pi / 2))


SINES = {MFMA: hw_sine, PER_SAMPLE: poly_sine}


# ----------------------------------------------------------------------------------------------------------
# what a probe reads: the feature table of a network and its evaluation at poses
Table = collections.namedtuple("Table", "c0 c1 b isa q")      # by input position: (wx | fr, wy, b, angle feature?, kind 0 sin / 1 cos)


def table(cfg, p, plant=None, where=None):
    """the feature table of the parameters p ({name: fp32 array} in cfg.layout() names), as decode_feature (csrc/onf_layout.h)
    forms it.  plant COS_AS_SIN: the first position of every cosine block is a sine; SWAP: the entries of positions
    where = (i, j) change places"""
    n, k = cfg.n_enc, cfg.angle_dim
    we = np.asarray(p["we"], F32)
    be = np.asarray(p["be"], F32) if "be" in p else np.zeros(n, F32)
    c0, c1, b = we[:, 0], we[:, 1], be
    q = (np.arange(n) >= 100).astype(np.int64)
    isa = np.zeros(n, bool)
    if k:
        c0 = np.concatenate([c0, np.asarray(p["ang_f"], F32)])
        c1 = np.concatenate([c1, np.zeros(2 * k, F32)])
        b = np.concatenate([b, np.asarray(p["ang_b"], F32)])
        q = np.concatenate([q, (np.arange(2 * k) >= k).astype(np.int64)])
        isa = np.concatenate([isa, np.ones(2 * k, bool)])
    c0, c1, b, q = c0.copy(), c1.copy(), b.copy(), q.copy()
    if plant == COS_AS_SIN:
        for first in cosine_block_starts(cfg):
            q[first] = 0
    if plant == SWAP:
        i, j = where
        for a in (c0, c1, b, q):
            a[[i, j]] = a[[j, i]]
    return Table(c0, c1, b, isa, q)


def cosine_block_starts(cfg):
    return ([100] if cfg.use_cos else []) + ([cfg.n_enc + cfg.angle_dim] if cfg.angle_dim else [])


def evaluate(tab, x, cols, sine=None, plant=None):
    """features `cols` of the table at the fp32 poses x [P, 2 | 3] -> (value, derivative by the argument, argument), each
    [P, len(cols)].  sine = None: the float64 reference on the float64 argument; else an emulation on the argument formed in
    fp32 as the kernels form it: fma(wx, ux, fma(wy, uy, b)), (theta + b) * fr"""
    x = np.asarray(x, F32)
    ux, uy = x[:, 0:1], x[:, 1:2]
    th = x[:, 2:3] if x.shape[1] == 3 else np.zeros_like(ux)
    c0, c1, b, isa, q = (a[cols][None] for a in tab)
    if sine is None:
        ux, uy, th, c0, c1, b = (a.astype(F64) for a in (ux, uy, th, c0, c1, b))
        arg = np.where(isa, (th + b) * c0, c0 * ux + (c1 * uy + b))
        return ref_sine(arg, q), ref_sine(arg, q + 1), arg
    pos = fma32(c0, ux, fma32(c1, uy, b))
    if plant == ANGLE_FORM:
        ang = ((th * c0).astype(F32) + b).astype(F32)
    else:
        ang = ((th + b).astype(F32) * c0).astype(F32)
    arg = np.where(isa, ang, pos)
    kw = dict(plant=plant) if plant in (DROP_LO, HI_ULP) else {}
    dq = q - 1 if plant == DERIV_BACK else q + 1
    return sine(arg, q, **kw), sine(arg, dq, **kw), arg


# ----------------------------------------------------------------------------------------------------------
# the comparer
class Stats(object):
    """worst |dev - r|, |dev - e|, |e - r| per (decade of |argument|, offset in quarter turns), and what is outside the gate"""

    def __init__(self, path):
        self.path = path
        self.worst = np.zeros((len(DECADES), len(OFFSETS), 3))
        self.count = np.zeros((len(DECADES), len(OFFSETS)), np.int64)
        self.failures = []
        self.cap_worst = 0.0

    def gate(self, what, dev, r, e, arg, offset, weight=1.0):
        """holds the probed values dev to the gate; r, e = reference and emulation of the sine itself, arg = its argument,
        offset = its quarter turns (0, 1, 2), weight = the exact factor the readout multiplies it by"""
        shape = np.shape(dev)
        assert np.shape(r) == np.shape(e) == np.shape(arg) == shape, (what, shape, np.shape(r), np.shape(e), np.shape(arg))
        offset = np.broadcast_to(np.asarray(offset, np.int64), shape).reshape(-1)
        dev, r, e, arg = (np.asarray(a, F64).reshape(-1) for a in (dev, r, e, arg))
        w = abs(float(weight))
        assert w > 0
        extra = 2 * V if self.path == MFMA else 0.0
        bound = w * (np.abs(e - r) + extra) + 2 * U * max(1.0, w)
        err = np.abs(dev - weight * r)
        bad = ~(np.isfinite(dev) & (err <= bound))
        for i in np.nonzero(bad)[0][:4]:
            self.failures.append("%s: arg %.9g offset %s/4: |dev - r| = %.3g > %.3g (|e - r| = %.3g, weight %g)"
                                 % (what, arg[i], offset[i], err[i] / w, bound[i] / w, abs(e[i] - r[i]), weight))
        if bad.sum() > 4:
            self.failures.append("%s: ... and %d more" % (what, int(bad.sum()) - 4))
        dec = decade(arg)
        fig = np.stack([err / w, np.abs(dev / weight - e), np.abs(e - r)], 1)
        fig = np.where(np.isfinite(fig), fig, np.inf)
        for d in range(len(DECADES)):
            for o in range(len(OFFSETS)):
                m = (dec == d) & (offset == o)
                if m.any():
                    self.worst[d, o] = np.maximum(self.worst[d, o], fig[m].max(0))
                    self.count[d, o] += int(m.sum())
        self.cap_worst = max(self.cap_worst, float(np.abs(e - r).max()) if e.size else 0.0)

    def exact_zero(self, what, dev):
        """values that are products with an exact zero: == 0, the sign of the zero is free"""
        dev = np.asarray(dev)
        if not np.all(dev == 0):
            bad = np.nonzero(dev.reshape(-1) != 0)[0]
            self.failures.append("%s: %d of %d values are not zero (first: index %d = %r)"
                                 % (what, bad.size, dev.size, bad[0], dev.reshape(-1)[bad[0]]))

    def fact(self, what, holds):
        if not holds:
            self.failures.append(what)

    def merge(self, other):
        assert other.path == self.path
        self.worst = np.maximum(self.worst, other.worst)
        self.count += other.count
        self.failures += other.failures
        self.cap_worst = max(self.cap_worst, other.cap_worst)
        return self

    def lines(self, tag):
        out = ["%-22s %-11s %-6s %8s %12s %12s %12s" % ("launch", "decade", "offset", "values", "|dev - r|", "|dev - e|", "|e - r|")]
        for d, dn in enumerate(DECADES):
            for o, on in enumerate(OFFSETS):
                if self.count[d, o]:
                    out.append("%-22s %-11s %-6s %8d %12.3g %12.3g %12.3g" % ((tag, dn, on, self.count[d, o]) + tuple(self.worst[d, o])))
        out.append("%-22s %-11s %-6s %8d %12.3g %12.3g %12.3g" % ((tag, "all", "all", self.count.sum()) + tuple(self.worst.max((0, 1)))))
        return out


def decade(arg):
    a = np.abs(np.asarray(arg, F64))
    return np.clip(np.floor(np.log10(np.maximum(a, 1e-300))).astype(np.int64) + 1, 0, len(DECADES) - 1)


# ----------------------------------------------------------------------------------------------------------
# Probe A: one position of one network, read through eval_points / eval_logits
def expect_a(case, path):
    """reference and emulation of the probed feature and its derivative at the case's poses -> dict of [P] arrays"""
    import feature_probe_cases as pc
    tab = table(pc.config(case.fin), pc.probe_a_params(case))
    cols = [case.f]
    r_val, r_d, arg = evaluate(tab, case.x, cols)
    e_val, e_d, arg32 = evaluate(tab, case.x, cols, SINES[path])
    return dict(arg=arg[:, 0], arg32=arg32[:, 0], q=int(tab.q[case.f]), r_val=r_val[:, 0], r_d=r_d[:, 0], e_val=e_val[:, 0],
                e_d=e_d[:, 0], weights=case.weights)


def simulate_a(case, path, plant=None, neighbour=None):
    """what a device with the planted error would return for the case: (logit [P], grad [P, 3]) in float64.  Only position f
    is read out (every other skip weight is an exact zero); under SWAP it is evaluated from its neighbour's table entry"""
    import feature_probe_cases as pc
    tab = table(pc.config(case.fin), pc.probe_a_params(case), plant, (case.f, neighbour) if plant == SWAP else None)
    val, d, _ = evaluate(tab, case.x, [case.f], SINES[path], plant)
    w = (0.0, 0.0, float(tab.c0[case.f])) if tab.isa[case.f] else (float(tab.c0[case.f]), float(tab.c1[case.f]), 0.0)
    return val[:, 0], d * np.array(w)[None]


def select_rows(case, exp, keep):
    """the case and its expectation on a subset of the poses"""
    return case._replace(x=case.x[keep]), {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in exp.items()}


def check_a(stats, case, exp, logit, grad=None):
    """holds a launch of the case to the gate: logit [P] and, with grad [P, 3], the gradient (operands that carry the
    argument: s' x weight; every other component an exact zero)"""
    tag = "A F%d f%d %s" % (case.fin, case.f, case.variant)
    stats.gate(tag + " logit", logit, exp["r_val"], exp["e_val"], exp["arg"], exp["q"])
    if grad is None:
        return
    for c, w in enumerate(exp["weights"]):
        if w != 0:
            stats.gate(tag + " grad[%d]" % c, grad[:, c], exp["r_d"], exp["e_d"], exp["arg"], exp["q"] + 1, weight=w)
        else:
            stats.exact_zero(tag + " grad[%d]" % c, grad[:, c])


# ----------------------------------------------------------------------------------------------------------
# Probe B: every position at once, read through the gradient of the fit
ZERO_BLOCKS = ("w1", "b1", "w2", "b2")


def expect_b(fin, c, path):
    """-> dict of [F] arrays for call c"""
    import feature_probe_cases as pc
    cfg = pc.config(fin)
    tab = table(cfg, pc.probe_b_params(fin, c))
    cols, x = np.arange(cfg.feature_dim), pc.probe_b_pose(fin)
    r_val, r_d, arg = evaluate(tab, x, cols)
    e_val, e_d, _ = evaluate(tab, x, cols, SINES[path])
    return dict(arg=arg[0], q=tab.q, r_val=r_val[0], r_d=r_d[0], e_val=e_val[0], e_d=e_d[0])


def simulate_b(fin, c, path, plant=None, where=None):
    """the gradient blocks {name: float64 array} a device with the planted error would return for call c (rho = -1)"""
    import feature_probe_cases as pc
    cfg = pc.config(fin)
    n = cfg.n_enc
    tab = table(cfg, pc.probe_b_params(fin, c), plant, where)
    val, d, _ = evaluate(tab, pc.probe_b_pose(fin), np.arange(cfg.feature_dim), SINES[path], plant)
    g = {name: np.zeros(shape) for name, shape in cfg.layout()}
    g["w3"][0, 100:] = -val[0]
    g["b3"][0] = -1
    g["we"][:, 0] = -d[0, :n]
    if cfg.bias:
        g["be"][:] = -d[0, :n]
    if cfg.angle_dim:
        g["ang_f"][:] = -d[0, n:]
        g["ang_b"][:] = -d[0, n:] * tab.c0[n:]
    return g


def unpack(cfg, flat_grad):
    out, o = {}, 0
    for name, shape in cfg.layout():
        k = int(np.prod(shape))
        out[name] = np.asarray(flat_grad[o:o + k]).reshape(shape)
        o += k
    return out


def check_b(stats, fin, c, exp, g):
    """holds the gradient blocks g of call c to the gate.  Precondition, bit for bit: grad[b3] == -1 (the sigmoid saturated to
    exactly 0, rho = -1, every product below is exact)"""
    import feature_probe_cases as pc
    cfg = pc.config(fin)
    n = cfg.n_enc
    tag = "B F%d call %d" % (fin, c)
    stats.fact(tag + ": grad[b3] = %r, not -1" % float(g["b3"][0]), float(g["b3"][0]) == -1.0)
    stats.gate(tag + " w3 skip", -g["w3"][0, 100:], exp["r_val"], exp["e_val"], exp["arg"], exp["q"])
    read = [("we[:, 0]", g["we"][:, 0], slice(0, n))]
    if cfg.bias:
        read.append(("be", g["be"], slice(0, n)))
    if cfg.angle_dim:
        read.append(("ang_f", g["ang_f"], slice(n, None)))
    for name, block, s in read:
        stats.gate("%s %s" % (tag, name), -block, exp["r_d"][s], exp["e_d"][s], exp["arg"][s], exp["q"][s] + 1)
    stats.exact_zero(tag + " we[:, 1]", g["we"][:, 1])
    for name in ZERO_BLOCKS:
        stats.exact_zero("%s %s" % (tag, name), g[name])
    stats.exact_zero(tag + " w3[:100]", g["w3"][0, :100])
