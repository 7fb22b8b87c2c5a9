"""Every angle dimension the ONF entries accept, and what each must do with it on each matrix path: the table, networks, poses
and comparers shared by tests/test_onf_geometries_cpu.py (no GPU) and tests/test_gpu_onf_geometries.py.

make_geom (csrc/common.h) takes angle_dim 0 .. 16 for both encoder widths (n_enc = 100, or 200 with use_cos); the input width
is F = n_enc + 2 angle_dim.  nfopp.ONF builds four of these shapes (100/100/0, 100/120/10, 200/200/0, 200/220/10: "stock");
the C entries and the torch ops take all of them.  TABLE states, cell by cell, what must happen.  It is written out, not
computed: the route (csrc/onf_dispatch.hip: onf_route) is what it checks.

  columns    uc ad F     use_cos, angle_dim, input width
             tiles       input tiles of 16 the 16x16 kernels visit.  They hold the features in layout P (csrc/onf_layout.h:
                         slot_layout_p): of a block of 32, features 0..7 and 16..23 sit in the even tile, 8..15 and 24..31 in
                         the odd one, so F = 105..112 needs 8 tiles and F = 201..208 needs 14 (not 7 and 13)
             blocks      input blocks of the 32x32 kernel the geometry is routed to on matrix path 1 ('-': none)
             inf 0 1 2   nfopp_onf_eval_points / _logits / nfopp_traj_collision_eval on matrix path 0, 1, 2
             fit 0 1 2   nfopp_onf_train_grad_ex, fit path 2 (MFMA), on matrix path 0, 1, 2
             ps          nfopp_onf_train_grad_ex, fit path 1 (per-sample)
  outcomes   fp32 / x32 / s16    computed, by the fp32 kernel / the 32x32 split kernel / the 16x16 split kernel
             ok                  the fit is computed
             R32                 refused by the 32x32 family's launcher: its kernels are written for the stock shapes
             pad                 the fit is refused: "no pad feature available" (the last tile is full: F = 128, 224)
             U                   refused: "unsupported ONF feature dimension"

Networks are seeded and drawn with the initialisers of nfopp.ONF (nn.Linear's uniform bounds, a normal encoding layer), angle
frequencies 1 .. angle_dim twice, angle biases uniform in +-pi and at least 0.05 from zero.  Poses are drawn like
k1_bits_cases.points and kept where the float64 distance to a ReLU kink is at least KINK_MARGIN, the way fit_blocks_cases
draws them: no row is left out of any comparison."""
import collections
import functools

import numpy as np

from oracle import nfopp_oracle as orc

import bits_float64_gate as bg
import fit_blocks_gate as fg
import float64_ref as f64

F32, F64 = np.float32, np.float64
MEAN, SIGMA = 0.4, 2.5                   # of k1_bits_cases.make_onf
POSE_P = (33, 65)                        # k1_kind_bits_cases.POSE_P: one ragged tile; a full tile and a row
FIT_P = 65
KINK_MARGIN = 1e-4                       # = fit_blocks_cases.KINK_MARGIN
TRAJ_B, TRAJ_N = 2, 9
MATRIX_PATHS = (0, 1, 2)
CUS = 256                                # the yardstick of a 65-sample fit does not depend on it (at most 5 chunks)

TABLE_TEXT = """
# uc ad   F tiles blocks | inf0 inf1 inf2 | fit0 fit1 fit2 | ps
   0  0 100     7      7 | fp32 x32  s16  | ok   ok   ok   | ok
   0  1 102     7      7 | fp32 R32  s16  | ok   R32  ok   | ok
   0  2 104     7      7 | fp32 R32  s16  | ok   R32  ok   | ok
   0  3 106     8      7 | fp32 R32  s16  | ok   R32  ok   | ok
   0  4 108     8      7 | fp32 R32  s16  | ok   R32  ok   | ok
   0  5 110     8      7 | fp32 R32  s16  | ok   R32  ok   | ok
   0  6 112     8      8 | fp32 R32  s16  | ok   R32  ok   | ok
   0  7 114     8      8 | fp32 R32  s16  | ok   R32  ok   | ok
   0  8 116     8      8 | fp32 R32  s16  | ok   R32  ok   | ok
   0  9 118     8      8 | fp32 R32  s16  | ok   R32  ok   | ok
   0 10 120     8      8 | fp32 x32  s16  | ok   ok   ok   | ok
   0 11 122     8      8 | fp32 R32  s16  | ok   R32  ok   | ok
   0 12 124     8      8 | fp32 R32  s16  | ok   R32  ok   | ok
   0 13 126     8      8 | fp32 R32  s16  | ok   R32  ok   | ok
   0 14 128     8      - | fp32 s16  s16  | pad  pad  pad  | ok
   0 15 130     -      - | U    U    U    | U    U    U    | U
   0 16 132     -      - | U    U    U    | U    U    U    | U
   1  0 200    13     13 | fp32 x32  s16  | ok   ok   ok   | ok
   1  1 202    14     13 | fp32 R32  s16  | ok   R32  ok   | ok
   1  2 204    14     13 | fp32 R32  s16  | ok   R32  ok   | ok
   1  3 206    14     13 | fp32 R32  s16  | ok   R32  ok   | ok
   1  4 208    14     14 | fp32 R32  s16  | ok   R32  ok   | ok
   1  5 210    14     14 | fp32 R32  s16  | ok   R32  ok   | ok
   1  6 212    14     14 | fp32 R32  s16  | ok   R32  ok   | ok
   1  7 214    14     14 | fp32 R32  s16  | ok   R32  ok   | ok
   1  8 216    14     14 | fp32 R32  s16  | ok   R32  ok   | ok
   1  9 218    14     14 | fp32 R32  s16  | ok   R32  ok   | ok
   1 10 220    14     14 | fp32 x32  s16  | ok   ok   ok   | ok
   1 11 222    14     14 | fp32 R32  s16  | ok   R32  ok   | ok
   1 12 224    14      - | fp32 s16  s16  | pad  pad  pad  | ok
   1 13 226     -      - | U    U    U    | U    U    U    | U
   1 14 228     -      - | U    U    U    | U    U    U    | U
   1 15 230     -      - | U    U    U    | U    U    U    | U
   1 16 232     -      - | U    U    U    | U    U    U    | U
"""

COMPUTED = ("fp32", "x32", "s16", "ok")
MESSAGE = {"U": "unsupported ONF feature dimension", "pad": "no pad feature available"}
Entry = collections.namedtuple("Entry", "use_cos angle_dim fin tiles blocks inf fit per_sample")


def _parse(text):
    out = collections.OrderedDict()
    for line in text.strip().splitlines():
        if line.lstrip().startswith("#"):
            continue
        head, inf, fit, ps = (part.split() for part in line.split("|"))
        uc, ad, fin = (int(v) for v in head[:3])
        tiles, blocks = (None if v == "-" else int(v) for v in head[3:])
        out[(uc, ad)] = Entry(uc, ad, fin, tiles, blocks, tuple(inf), tuple(fit), ps[0])
    return out


TABLE = _parse(TABLE_TEXT)
ACCEPTED = tuple(k for k, e in TABLE.items() if e.per_sample == "ok")
UNSUPPORTED = tuple(k for k, e in TABLE.items() if e.per_sample == "U")
STOCK = ((0, 0), (0, 10), (1, 0), (1, 10))
# one geometry per tile count without an encoding bias; 13 tiles serve the stock 200/200/0 alone
NO_BIAS = ((0, 2), (0, 4), (1, 2))
# (use_cos, angle_dim, has_bias) of every network
NETWORKS = tuple(k + (1,) for k in ACCEPTED) + tuple(k + (0,) for k in NO_BIAS)


def name(geom):
    e = TABLE[geom[:2]]
    return "%d/%d/%d%s" % (200 if e.use_cos else 100, e.fin, e.angle_dim, "" if len(geom) < 3 or geom[2] else " nobias")


def refusal(entry, outcome):
    """the words the error message of a refused cell must contain"""
    if outcome == "R32":
        return ("%d input blocks" % entry.blocks, "fin %d" % entry.fin, "angle_dim %d" % entry.angle_dim)
    return (MESSAGE[outcome],)


# ----------------------------------------------------------------------------------------------------------
# networks, poses, trajectories
@functools.lru_cache(None)
def network(use_cos, angle_dim, has_bias=1):
    """-> (flat fp32 parameters, read-only; oracle config)"""
    cfg = orc.OnfConfig(MEAN, SIGMA, bool(use_cos), bool(has_bias), angle_dim > 0, angle_dim)
    assert cfg.feature_dim == TABLE[(use_cos, angle_dim)].fin
    rng = np.random.default_rng([1000, use_cos, angle_dim, has_bias])
    p = {}
    for key, shape in cfg.layout():
        if key == "ang_b":
            b = rng.uniform(0.05, np.pi, shape) * rng.choice([-1.0, 1.0], shape)
        elif key == "ang_f":
            b = np.tile(np.arange(1, angle_dim + 1), 2)
        elif key == "we":
            b = rng.standard_normal(shape)
        else:
            fan_in = {"w1": cfg.feature_dim, "b1": cfg.feature_dim, "w2": 100, "b2": 100, "w3": 100 + cfg.feature_dim,
                      "b3": 100 + cfg.feature_dim, "be": 2}[key]
            b = rng.uniform(-1, 1, shape) / np.sqrt(fan_in)
        p[key] = b.astype(F32)
    flat = orc.pack_params(p, cfg)
    flat.setflags(write=False)
    return flat, cfg


def _draw(rng, n, dim):
    x = rng.uniform(-4, 6, (n, dim)).astype(F32)
    if dim == 3:
        x[:, 2] = rng.uniform(-3.3, 3.3, n).astype(F32)
    return x


@functools.lru_cache(None)
def poses(use_cos, angle_dim, has_bias, P):
    """[P, 2 | 3] fp32, every row at least KINK_MARGIN from a ReLU kink in float64"""
    flat, cfg = network(use_cos, angle_dim, has_bias)
    drawn = _draw(np.random.default_rng([2000, use_cos, angle_dim, has_bias, P]), P + P // 4 + 64, cfg.point_dim)
    keep = np.flatnonzero(f64.onf_eval64(flat, cfg, drawn)["kink"] >= KINK_MARGIN)[:P]
    assert len(keep) == P, "too few kink-free rows drawn for %s, P = %d" % (name((use_cos, angle_dim, has_bias)), P)
    x = np.ascontiguousarray(drawn[keep])
    x.setflags(write=False)
    return x


@functools.lru_cache(None)
def trajectory(use_cos, angle_dim):
    """-> (traj [B, N, D], draws t [B, N - 1], the oracle's sample poses [B (N - 1), D])"""
    dim = 3 if angle_dim else 2
    rng = np.random.default_rng([3000, use_cos, angle_dim])
    traj = _draw(rng, TRAJ_B * TRAJ_N, dim).reshape(TRAJ_B, TRAJ_N, dim)
    t = rng.uniform(0, 1, (TRAJ_B, TRAJ_N - 1)).astype(F32)
    samples = orc.sample_collision_points(traj, t) if dim == 3 else orc.sample_collision_points_2d(traj, t)
    return traj, t, np.ascontiguousarray(samples.reshape(-1, dim).astype(F32))


# ----------------------------------------------------------------------------------------------------------
# inference: reference and comparer (the float64 gate of bits_float64_gate)
@functools.lru_cache(None)
def inference_reference(use_cos, angle_dim, has_bias=1):
    """{P: dict of x, float64 and oracle32 logit / gradient, kink} and the network's scales, computed once"""
    flat, cfg = network(use_cos, angle_dim, has_bias)
    ref = collections.OrderedDict()
    for P in POSE_P:
        x = poses(use_cos, angle_dim, has_bias, P)
        c = f64.onf_eval64(flat, cfg, x)
        o_logit, o_grad = orc.onf_forward_grad(flat, cfg, x)
        ref[P] = dict(x=x, logit=c["logit"], grad=c["grad"], kink=c["kink"], darg=c["darg"], o32_logit=o_logit, o32_grad=o_grad)
    ref["scale"] = (max(float(np.abs(ref[P]["logit"]).max()) for P in POSE_P), max(float(np.abs(ref[P]["grad"]).max()) for P in POSE_P))
    return ref


def compare_inference(tag, geom, P, ref, full=None, forward=None):
    """out4 [P, 4] of nfopp_onf_eval_points (`full`) and nfopp_onf_eval_logits (`forward`) against float64 -> [bg.Row].
    Every row is compared: the poses are kink-free."""
    rows, r = [], ref[P]
    sl, sg = ref["scale"]
    dim = r["x"].shape[1]
    case = "%s P%d" % (name(geom), P)
    if full is not None:
        full = np.asarray(full).reshape(-1, 4)
        bg.gate(rows, tag, case, "logit", full[:, 0], r["logit"], r["o32_logit"], sl, cap=bg.PARITY["logit"] * sl)
        bg.gate(rows, tag, case, "grad", full[:, 1:1 + dim], r["grad"], r["o32_grad"], sg, cap=bg.PARITY["grad"] * sg)
        if dim == 2:
            bg.fact(rows, tag, case, "column 3 is zero (2-D network)", np.all(full[:, 3] == 0))
    if forward is not None:
        forward = np.asarray(forward).reshape(-1, 4)
        bg.gate(rows, tag, case, "logit fwd", forward[:, 0], r["logit"], r["o32_logit"], sl, cap=bg.PARITY["logit"] * sl)
        bg.fact(rows, tag, case, "columns 1..3 are zero", np.all(forward[:, 1:] == 0))
    return rows


# ----------------------------------------------------------------------------------------------------------
# fit: reference and comparer (fit_blocks_gate)
def labels(use_cos, angle_dim, has_bias, logit64):
    """uniform < 0.35, the sentinels of fit_blocks_cases (last sample, first sample of the last 32-chunk) contradicted"""
    P = len(logit64)
    y = (np.random.default_rng([4000, use_cos, angle_dim, has_bias]).uniform(size=P) < 0.35).astype(F32)
    s = sorted({P - 1, 32 * ((P - 1) // 32)})
    y[s] = (logit64[s] < 0).astype(F32)
    return y


@functools.lru_cache(None)
def fit_reference(use_cos, angle_dim, has_bias=1):
    flat, cfg = network(use_cos, angle_dim, has_bias)
    x = poses(use_cos, angle_dim, has_bias, FIT_P)
    y = labels(use_cos, angle_dim, has_bias, f64.onf_eval64(flat, cfg, x)["logit"])
    return fg.reference_of(flat, cfg, x, y, CUS)


def compare_fit(tag, geom, ref, g, K):
    """the fit's output g [n_params + 2] block by block -> [bg.Row] (ten blocks or eight, the loss, the count)"""
    rows = fg.compare(tag, ref, g, K)
    return [r._replace(case=name(geom)) for r in rows]


# ----------------------------------------------------------------------------------------------------------
# single-feature read-out (the construction of feature_probe_cases): positions and networks
PROBE_P = 33
PROBE_WE, PROBE_BE = (F32(0.75), F32(-0.5)), F32(0.3125)
PROBE_FR, PROBE_ANG_B = F32(1.5), F32(-0.40625)


def probe_positions(use_cos, angle_dim):
    """n_enc, F - 1 and both sides of every multiple of 8 from 96 (192) up to F"""
    e = TABLE[(use_cos, angle_dim)]
    n_enc = 200 if use_cos else 100
    s = {n_enc, e.fin - 1}
    for m in range(n_enc - n_enc % 32, e.fin + 1, 8):
        s |= {m - 1, m}
    return sorted(f for f in s if 0 <= f < e.fin)


def probe_config(use_cos, angle_dim, has_bias=1):
    return orc.OnfConfig(0.0, 1.0, bool(use_cos), bool(has_bias), angle_dim > 0, angle_dim)


@functools.lru_cache(None)
def _probe_fill(use_cos, angle_dim, has_bias):
    cfg = probe_config(use_cos, angle_dim, has_bias)
    rng = np.random.default_rng([5000, use_cos, angle_dim, has_bias])
    p = {key: np.zeros(shape, F32) for key, shape in cfg.layout()}
    for key in ("we", "be", "ang_b", "ang_f"):
        if key in p:
            p[key] = (rng.standard_normal(p[key].shape) * 30.0).astype(F32)     # feature_probe_cases.FILL_SCALE
    return p


def probe_params(use_cos, angle_dim, has_bias, f):
    """{name: fp32 array}: both hidden layers zero, skip weight 1 at position f, every other feature row random at scale 30"""
    cfg = probe_config(use_cos, angle_dim, has_bias)
    p = {k: v.copy() for k, v in _probe_fill(use_cos, angle_dim, has_bias).items()}
    if f < cfg.n_enc:
        p["we"][f] = PROBE_WE
        if cfg.bias:
            p["be"][f] = PROBE_BE
    else:
        p["ang_f"][f - cfg.n_enc], p["ang_b"][f - cfg.n_enc] = PROBE_FR, PROBE_ANG_B
    p["w3"][0, 100 + f] = 1
    return p


@functools.lru_cache(None)
def probe_poses(use_cos, angle_dim):
    """arguments within a few radians: |0.75 x - 0.5 y + b| <= 2.9, |(theta - 0.41) 1.5| <= 3.6"""
    rng = np.random.default_rng([6000, use_cos, angle_dim])
    x = rng.uniform(-2, 2, (PROBE_P, 3 if angle_dim else 2)).astype(F32)
    x.setflags(write=False)
    return x
