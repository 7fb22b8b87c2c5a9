"""The probe networks and arguments of the feature probes: shared by tests/test_feature_probe_cpu.py and
tests/test_gpu_feature_probe.py (the gate: tests/feature_probe_gate.py).

The network has a skip connection, logit = w3 . [h2, in] + b3.  With mean = 0, sigma = 1 and w1, b1, w2, b2, w3[:100] all
zero the hidden layers contribute exactly 0 and every ReLU mask is off, so the skip weights read single input features out
through the public entries, exactly: a feature sin(arg + q pi/2) and its derivative by the argument, per input position.

Every argument is exact: the fp32 operations that form it -- fma(wx, ux, fma(wy, uy, b)) for a positional feature,
(theta + b) * fr for an angle feature -- round nothing, because one operand carries the argument and the others are 1 or 0, or
because all values lie on a grid of 2^-6 (times weights that keep the products on it) so that the sums are exact.
argument_steps() restates each operation in float64 and exact() checks fl32(result) == result for every one.

Probe A (inference: nfopp_onf_eval_points, nfopp_onf_eval_logits): one network per probed position f and operand variant,
  w3[100 + f] = 1, every other skip weight 0, b3 = 0; every other feature row holds random frequencies and biases N(0, 1) x 30,
  so a kernel that reads a neighbour's table entry errs by O(1).  The poses carry the argument list of probe_a_arguments().
    x / y     we[f] = (1, 0) / (0, 1), the argument in x / y       angle positions: `unit` b = 0, fr = 1, the argument in theta
    grid      we[f] = (0.75, -0.5), b = 105/64 where the configuration has an encoding bias; ux on the 2^-4 grid, uy on
              2^-5: every product and sum on the 2^-6 grid      angle positions: fr = 2, b = -49/64, theta on the 2^-6 grid
  logit = s_f(arg), d logit / d pose = s_f'(arg) x (wx, wy, fr); the components of the other operands are exactly 0.
Probe B (the fit: nfopp_onf_train_grad_ex): one sample (1, 0[, 0]), label 1, b3 = -1000, every skip weight 1; position f's
  argument is its own frequency, we[f] = (a_f, 0), be = 0; angle positions ang_b = 1, ang_f = a_k.  The sigmoid saturates to
  exactly 0, rho = -1: grad[w3 skip][f] = -s_f(a_f), grad[be][f] = grad[we][f, 0] = -s_f'(a_f), grad[ang_f][k] = -s_k'(a_k),
  grad[b3] = -1 and grad[w1 | b1 | w2 | b2 | w3[:100]] = 0.  Call c gives position f the argument number (c + 7 f) mod n of
  probe_b_arguments(): over the n calls every position meets every argument of the list."""
import collections
import functools

import numpy as np

from oracle import nfopp_oracle as orc

F32, F64 = np.float32, np.float64
# (use_cos, angle, bias) of the four feature dimensions: tests/k1_bits_cases.py DIMS (not imported: that module needs torch)
DIMS = {220: (True, True, True), 200: (True, False, True), 120: (False, True, False), 100: (False, False, True)}
LIMIT = 1e5                      # csrc/common.h states the accuracy of the hardware chain for |x| < 1e5
FILL_SCALE = 30.0
GRID_W = (F32(0.75), F32(-0.5))
GRID_B, GRID_ANG_B, GRID_FR = F32(105 / 64), F32(-49 / 64), F32(2)
B_STEP = 7
VARIANTS = {False: ("x", "y", "grid"), True: ("unit", "grid")}     # by `angle position?`


def config(fin):
    use_cos, angle, bias = DIMS[fin]
    return orc.OnfConfig(0.0, 1.0, use_cos, bias, angle)


def is_angle(fin, f):
    return f >= config(fin).n_enc


def blocks(fin):
    """[(first, end)] of the kind blocks: positional sine, positional cosine, angle sine, angle cosine"""
    cfg = config(fin)
    out = [(0, 100)] + ([(100, 200)] if cfg.use_cos else [])
    if cfg.angle_dim:
        out += [(cfg.n_enc, cfg.n_enc + cfg.angle_dim), (cfg.n_enc + cfg.angle_dim, cfg.feature_dim)]
    return out


# ----------------------------------------------------------------------------------------------------------
# arguments
def edge_arguments():
    """+-0; the fp32 value nearest k pi/2 and both its neighbours; the fp32 value nearest (n + 1/2) 2 pi, where the turn count
    is a tie; +-2^k; 99 999.99 -- nothing at or beyond 1e5, nothing non-finite"""
    out = [F32(0.0), F32(-0.0)]
    for k in (1, 2, 3, 4, 100, 1001, 10007, 63660):
        c = F32(k * np.pi / 2)
        out += [np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf)), -c]
    for n in (0, 1, 159, 15914):
        c = F32((n + 0.5) * 2 * np.pi)
        out += [c, -c]
    for k in range(-20, 17):
        out += [F32(2.0 ** k), F32(-2.0 ** k)]
    out += [F32(99999.99), -F32(99999.99)]
    out = np.array(out, F32)
    assert np.all(np.abs(out) < LIMIT) and np.isfinite(out).all()
    return out


def decade_arguments(per_decade, seed):
    """per_decade arguments in each of [0, 1), [1, 10), ... [1e4, 1e5), signs alternating; log-uniform from [1, 10) up"""
    rng = np.random.default_rng(seed)
    out = []
    for d in range(6):
        a = rng.uniform(0.02, 0.98, per_decade) if d == 0 else 10.0 ** (d - 1 + rng.uniform(0.01, 0.99, per_decade))
        out.append(a * np.where(np.arange(per_decade) % 2, -1.0, 1.0))
    return np.concatenate(out).astype(F32)


@functools.lru_cache(None)
def probe_a_arguments():
    a = np.concatenate([decade_arguments(36, 11), edge_arguments()])
    assert 257 <= len(a) <= 600 and len(a) % 32
    return a


@functools.lru_cache(None)
def probe_b_arguments():
    return np.concatenate([decade_arguments(8, 12), edge_arguments()])


def grid_targets():
    """where the grid variant's arguments are aimed: the decades, +-2^k from the grid's step up, and small arguments"""
    rng = np.random.default_rng(13)
    pw = [s * 2.0 ** k for k in range(-6, 17) for s in (1, -1)]
    t = np.concatenate([decade_arguments(36, 14).astype(F64), pw, rng.uniform(-12, 12, 72)])
    assert len(t) == len(probe_a_arguments())
    return t


# ----------------------------------------------------------------------------------------------------------
# Probe A
ProbeA = collections.namedtuple("ProbeA", "fin f variant row x weights")    # row = the table words of position f: (c0, c1, b)


def positions(fin):
    """both ends of every kind block; both sides of every multiple of 16 from position 96 up; every angle position; for 120
    inputs every position from 96 on (the group with mixed kinds)"""
    cfg = config(fin)
    s = set()
    for lo, hi in blocks(fin):
        s |= {lo, hi - 1}
    for m in range(96, cfg.feature_dim, 16):
        s |= {m - 1, m}
    s |= set(range(cfg.n_enc, cfg.feature_dim))
    if fin == 120:
        s |= set(range(96, 120))
    return sorted(s)


def _other_coordinates(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4, 6, (n, 3)).astype(F32)
    x[:, 2] = rng.uniform(-3.3, 3.3, n).astype(F32)
    return x


def probe_a_case(fin, f, variant):
    cfg = config(fin)
    D = cfg.point_dim
    args = probe_a_arguments()
    x = _other_coordinates(len(args), 1000 * fin + 10 * f + len(variant))
    if not is_angle(fin, f):
        if variant in ("x", "y"):
            c = "xy".index(variant)
            row = (F32(c == 0), F32(c == 1), F32(0))
            x[:, c] = args
        else:
            wx, wy = GRID_W
            b = GRID_B if cfg.bias else F32(0)
            t = grid_targets()
            uy = np.round(x[:, 1].astype(F64) * 32) / 32
            ux = np.round((t - float(wy) * uy - float(b)) / float(wx) * 16) / 16
            x[:, 0], x[:, 1] = ux.astype(F32), uy.astype(F32)
            row = (wx, wy, b)
        weights = (float(row[0]), float(row[1]), 0.0)
    else:
        if variant == "unit":
            row = (F32(1), F32(0), F32(0))
            x[:, 2] = args
        else:
            row = (GRID_FR, F32(0), GRID_ANG_B)
            x[:, 2] = (np.round((grid_targets() / float(GRID_FR) - float(GRID_ANG_B)) * 64) / 64).astype(F32)
        weights = (0.0, 0.0, float(row[0]))
    return ProbeA(fin, f, variant, row, np.ascontiguousarray(x[:, :D]), weights)


@functools.lru_cache(None)
def probe_a_cases(fin):
    return tuple(probe_a_case(fin, f, v) for f in positions(fin) for v in VARIANTS[is_angle(fin, f)])


@functools.lru_cache(None)
def _fill(fin):
    """{name: fp32 array} of the probe networks' common part: zero hidden layers and skip weights, every feature row random"""
    cfg = config(fin)
    rng = np.random.default_rng(2000 + fin)
    p = {name: np.zeros(shape, F32) for name, shape in cfg.layout()}
    for name in ("we", "be", "ang_b", "ang_f"):
        if name in p:
            p[name] = (rng.standard_normal(p[name].shape) * FILL_SCALE).astype(F32)
    return p


def probe_a_params(case):
    """{name: fp32 array} of the case's network"""
    cfg = config(case.fin)
    p = {k: v.copy() for k, v in _fill(case.fin).items()}
    c0, c1, b = case.row
    if not is_angle(case.fin, case.f):
        p["we"][case.f] = (c0, c1)
        if cfg.bias:
            p["be"][case.f] = b
        else:
            assert b == 0
    else:
        k = case.f - cfg.n_enc
        p["ang_f"][k], p["ang_b"][k] = c0, b
    p["w3"][0, 100 + case.f] = 1
    return p


def flat(fin, p):
    return orc.pack_params(p, config(fin))


def argument_steps(case):
    """the operations that form the case's argument, each restated in float64 on the fp32 operands -> [step results [P]]"""
    c0, c1, b = (float(v) for v in case.row)
    x = case.x.astype(F64)
    if not is_angle(case.fin, case.f):
        inner = c1 * x[:, 1] + b
        return [inner, c0 * x[:, 0] + inner]
    s = x[:, 2] + b
    return [s, s * c0]


def exact(steps):
    """fl32(exact) == exact for every step"""
    return all(bool(np.all(s.astype(F32).astype(F64) == s)) for s in steps)


# ----------------------------------------------------------------------------------------------------------
# Probe B
def probe_b_calls(fin):
    return len(probe_b_arguments())


def probe_b_args(fin, c):
    """the arguments of call c by input position [F]"""
    L = probe_b_arguments()
    return L[(c + B_STEP * np.arange(config(fin).feature_dim)) % len(L)]


def probe_b_params(fin, c):
    cfg = config(fin)
    a = probe_b_args(fin, c)
    p = {name: np.zeros(shape, F32) for name, shape in cfg.layout()}
    p["we"][:, 0] = a[:cfg.n_enc]
    if cfg.angle_dim:
        p["ang_b"][:] = 1
        p["ang_f"][:] = a[cfg.n_enc:]
    p["w3"][0, 100:] = 1
    p["b3"][0] = -1000
    return p


def probe_b_pose(fin):
    x = np.zeros((1, config(fin).point_dim), F32)
    x[0, 0] = 1
    return x
