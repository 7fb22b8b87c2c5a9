"""The block-by-block gate of the fit's summed gradient (nfopp_onf_train_grad[_ex]) against float64, at the cases of
tests/fit_blocks_cases.py.  tests/test_fit_blocks_cpu.py shows on the CPU that the gate passes two independent fp32
evaluations and rejects planted errors; tests/test_gpu_fit_blocks.py applies it to the device.

Per parameter block k of cfg.layout() (ang_b, ang_f, w1, b1, w2, b2, w3, b3, we, be):

  S        float64_ref.fit_sums64(mag=True): the float64 gradient formula with every factor replaced by its absolute value
  unit_k   2^-24 x max over the block of S: the fp32 rounding unit of the block's sums, whatever cancels in them
  e(g, k)  max over the block of |g - float64| / unit_k
  loss     unit = 2^-24 x mean |loss_p|

The yardstick is measured, not chosen: two fp32 evaluations that use none of the code under test,
  oracle32       orc.onf_train_grads on the whole case
  chunked32(K)   the oracle's fp32 per-sample arithmetic (rho with the whole case's 1 / P), summed as pass 2 sums: K-sample
                 chunks, the chunks w, w + C, ... of each virtual workgroup added in order in fp32, then the workgroup sums
                 added in order (K = 32; 16 for matrix path 0)
  Y_case = max(1, max over the ten blocks and both evaluations of e)
  bound of block k = FACTOR x Y_case x unit_k, FACTOR = 8 as everywhere in bits_float64_gate, and never looser than the gate
  of tests/test_gpu_split_path.py: 2e-5 x max(1, max |oracle32 gradient|) (loss: 5e-6 x max(1, |loss|)).

Y is pooled over the blocks of a case because in these units every block of a correct evaluation sits at the same few
units; pooling keeps a one-element block (b3) from being judged by its own luck (an earlier per-block yardstick was nearly
zero there), while each block is still judged at its OWN scale.  Rows reuse bits_float64_gate.Row with scale = unit_k and
orc_err = Y_case x unit_k, so its summary() prints Y and e in units and its ratio() the fraction e / Y (gate: FACTOR)."""
import collections
import functools

import numpy as np

from oracle import nfopp_oracle as orc

import bits_float64_gate as bg
import fit_blocks_cases as fc
import float64_ref as f64

F32 = np.float32
EPS = 2.0 ** -24
FACTOR = bg.FACTOR
OLD_GRAD, OLD_LOSS = 2e-5, 5e-6      # tests/test_gpu_split_path.py, tests/test_gpu_parity.py


@functools.lru_cache(maxsize=None)
def network(fin):
    return bg.cpu_network(fin)


def blocks(cfg):
    """{block name: slice of the flat gradient}"""
    out, o = collections.OrderedDict(), 0
    for name, shape in cfg.layout():
        n = int(np.prod(shape))
        out[name] = slice(o, o + n)
        o += n
    return out


def family_of(P, C):
    """the case family a count is listed under in profiles/fit_blocks.txt"""
    if P in fc.SMALL:
        return "small"
    for K in fc.KS:
        if P in fc.grid_edges(C, K):
            return "grid K=%d" % K
    return "cap 64"


# ----------------------------------------------------------------------------------------------------------
# the two fp32 evaluations
def factors32(flat, cfg, x, y):
    """the oracle's per-sample factors in fp32: orc.onf_train_grads restated up to, not including, its sums over samples"""
    p = orc.unpack_params(flat, cfg)
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    logit, c = orc._onf_forward_cache(p, cfg, x)
    inv = F32(len(y))
    rho = ((orc.sigmoid(logit) - y) / inv).astype(F32)
    loss_p = ((np.maximum(logit, 0) - logit * y + np.log1p(np.exp(-np.abs(logit)))) / inv).astype(F32)
    w3, e = p["w3"][0], c["e"]
    dh2 = (rho[:, None] * w3[None, :100] * (c["a2"] > 0)).astype(F32)
    dh1 = ((dh2 @ p["w2"]) * (c["a1"] > 0)).astype(F32)
    din = (dh1 @ p["w1"] + rho[:, None] * w3[None, 100:]).astype(F32)
    if cfg.use_cos:
        de = np.concatenate([din[:, :100] * np.cos(e[:, :100]), -din[:, 100:200] * np.sin(e[:, 100:])], 1).astype(F32)
    else:
        de = (din[:, :100] * np.cos(e)).astype(F32)
    f = dict(rho=rho[:, None], loss_p=loss_p[:, None], cat=np.concatenate([c["h2"], c["inp"]], 1), dh2=dh2, h1=c["h1"], dh1=dh1,
             inp=c["inp"], de=de, u=c["u"], on1=c["a1"] > 0, on2=c["a2"] > 0)
    if cfg.angle_encoding:
        d, z = cfg.angle_dim, c["z"]
        dz = np.concatenate([din[:, cfg.n_enc:cfg.n_enc + d] * np.cos(z[:, :d]), -din[:, cfg.n_enc + d:] * np.sin(z[:, d:])], 1).astype(F32)
        f["dzb"] = (dz * p["ang_f"][None]).astype(F32)
        f["dzf"] = (dz * (x[:, 2:3] + p["ang_b"][None])).astype(F32)
    return f


SUMMED = ("rho", "loss_p", "cat", "dh2", "h1", "dh1", "inp", "de", "u", "dzb", "dzf")


def _chunk_sums(ch, cfg):
    """fp32 sums of the chunks ch = {factor: [n, K, width]} -> [n, n_params + 1] (flat gradient | loss)"""
    t = lambda a: a.transpose(0, 2, 1)
    g = dict(w3=np.matmul(t(ch["rho"]), ch["cat"]), b3=ch["rho"].sum(1, dtype=F32), w2=np.matmul(t(ch["dh2"]), ch["h1"]),
             b2=ch["dh2"].sum(1, dtype=F32), w1=np.matmul(t(ch["dh1"]), ch["inp"]), b1=ch["dh1"].sum(1, dtype=F32),
             we=np.matmul(t(ch["de"]), ch["u"]), be=ch["de"].sum(1, dtype=F32))
    if cfg.angle_encoding:
        g["ang_b"], g["ang_f"] = ch["dzb"].sum(1, dtype=F32), ch["dzf"].sum(1, dtype=F32)
    n = len(ch["rho"])
    out = [g[name].reshape(n, -1) for name, _ in cfg.layout()] + [ch["loss_p"].sum(1, dtype=F32).reshape(n, 1)]
    assert all(a.dtype == F32 for a in out)
    return np.concatenate(out, 1)


def chunked32(f, cfg, K, C):
    """the summed gradient and loss from the fp32 factors f in the order of pass 2 on C compute units -> (grad, loss)"""
    P = len(f["rho"])
    n_chunks = -(-P // K)
    grid = min(C, n_chunks)
    pad = n_chunks * K - P        # zero rows: they add exact zeros to the last chunk
    ch = {k: np.concatenate([f[k], np.zeros((pad, f[k].shape[1]), F32)]).reshape(n_chunks, K, -1) for k in SUMMED if k in f}
    part = np.zeros((grid, cfg.n_params() + 1), F32)
    for lo in range(0, n_chunks, grid):          # round r: chunk r of every workgroup
        hi = min(lo + grid, n_chunks)
        part[:hi - lo] += _chunk_sums({k: a[lo:hi] for k, a in ch.items()}, cfg)
    total = part[0].copy()
    for w in range(1, grid):
        total += part[w]
    assert total.dtype == F32
    return total[:-1], total[-1]


# ----------------------------------------------------------------------------------------------------------
# reference and comparer
def errors(ref, g, loss):
    """{block: e(g, block)} and the loss's e, in units"""
    d = np.abs(np.asarray(g, np.float64) - ref["grad"])
    e = collections.OrderedDict((k, float(d[s].max()) / ref["unit"][k]) for k, s in ref["blocks"].items())
    return e, abs(float(loss) - ref["loss"]) / ref["loss_unit"]


def reference(fin, P, C, keep_eval=False):
    """everything the comparer needs of the case (F, P) on C compute units, computed once and shared by every launch"""
    flat, cfg = network(fin)
    x, y = fc.inputs(fin, P, flat, cfg)
    return reference_of(flat, cfg, x, y, C, keep_eval)


def reference_of(flat, cfg, x, y, C, keep_eval=False):
    """the same for any network (flat, cfg) and samples (x, y): what tests/onf_geometry_cases.py builds its fit cases with"""
    fin, P = cfg.feature_dim, len(y)
    r64 = f64.onf_fit64(flat, cfg, x, y, keep_eval=True)
    c = r64["eval"]
    S = f64.fit_sums64(c, cfg, r64["rho"], mag=True)
    bl = blocks(cfg)
    ref = dict(fin=fin, P=P, C=C, cfg=cfg, x=x, y=y, blocks=bl, grad=r64["grad"], loss=float(r64["loss"]), rho=r64["rho"],
               kink=r64["kink"], unit=collections.OrderedDict((k, EPS * float(S[s].max())) for k, s in bl.items()),
               loss_unit=EPS * float(np.abs(r64["loss_p"]).mean()))
    o_loss, _, o_grad = orc.onf_train_grads(flat, cfg, x, y)
    f = factors32(flat, cfg, x, y)
    ref["masks_agree"] = bool(np.array_equal(f["on1"], c["a1"] > 0) and np.array_equal(f["on2"], c["a2"] > 0))
    ref["o32"] = (o_grad, float(o_loss))
    ref["e_o32"] = errors(ref, *ref["o32"])
    ref["old_grad"] = OLD_GRAD * max(1.0, float(np.abs(o_grad).max()))
    ref["old_loss"] = OLD_LOSS * max(1.0, abs(float(o_loss)))
    ref["chunked"], ref["e_chunked"], ref["Y"] = {}, {}, {}
    for K in fc.KS:
        ref["chunked"][K] = chunked32(f, cfg, K, C)
        ref["e_chunked"][K] = errors(ref, *ref["chunked"][K])
        ref["Y"][K] = max([1.0] + list(ref["e_o32"][0].values()) + list(ref["e_chunked"][K][0].values()))
    if keep_eval:
        ref["eval"] = c
    return ref


def compare(tag, ref, g, K, count=True):
    """the fit's output g [n_params + 2] (gradient | loss | count) against the case's float64 values, with the yardstick of
    chunk length K -> [Row]: ten blocks, the loss and the count slot"""
    g = np.asarray(g)
    fin, P, Y = ref["fin"], ref["P"], ref["Y"][K]
    family, case = "%s %s" % (tag, family_of(P, ref["C"])), "F%d_P%d" % (fin, P)
    e, e_loss = errors(ref, g[:-2], g[-2])
    rows = []

    def row(name, unit, err, cap, finite):
        bound = min(FACTOR * Y * unit, cap)
        rows.append(bg.Row(family, case, name, unit, Y * unit, err * unit, bound, bool(finite and err * unit <= bound)))

    for k, s in ref["blocks"].items():
        row(k, ref["unit"][k], e[k], ref["old_grad"], np.isfinite(g[:-2][s]).all())
    row("loss", ref["loss_unit"], e_loss, ref["old_loss"], np.isfinite(g[-2]))
    if count:
        bg.fact(rows, family, case, "sample count", g[-1] == P)
    return rows


def old_gate_accepts(ref, g):
    """the gate this one replaces at these cases: one number for the whole gradient, at the scale of its largest entry"""
    return bool(np.abs(np.asarray(g, np.float64)[:-2] - ref["o32"][0]).max() < ref["old_grad"])


def output_of(grad, loss, P):
    return np.concatenate([np.asarray(grad, F32), [F32(loss), F32(P)]]).astype(F32)


def table(rows):
    """per family and block: cases, Y and worst e in units, worst e / bound -- the lines of profiles/fit_blocks.txt"""
    groups = collections.OrderedDict()
    for r in rows:
        if r.scale > 0:
            groups.setdefault((r.family, r.array), []).append(r)
    lines = ["%-24s %-6s %5s %8s %8s %8s  %s" % ("family", "block", "cases", "Y", "worst e", "e/bound", "worst at")]
    for (family, array), rs in groups.items():
        w = max(rs, key=lambda r: r.got_err / r.bound)
        lines.append("%-24s %-6s %5d %8.1f %8.1f %8.3f  %s" % (family, array, len(rs), max(r.orc_err / r.scale for r in rs),
                                                             max(r.got_err / r.scale for r in rs), w.got_err / w.bound, w.case))
    return lines
