"""GPU: every (geometry, matrix path) cell of the table in tests/onf_geometry_cases.py -- all 28 angle dimensions the ONF
entries accept, not only the four shapes nfopp.ONF builds.

  inference    nfopp_onf_eval_points and nfopp_onf_eval_logits at P = 33 and 65 against float64 (bits_float64_gate.gate:
               |dev - f64| <= 8 x max(|oracle32 - f64|, 1 ulp of the scale)); outputs NaN-filled between guards; a repeat of
               the call bit-equal
  read-out     both hidden layers zero and a skip weight of 1 at one position (the construction of feature_probe_cases): the
               logit is that feature, the gradient its derivative times (wx, wy, fr), at n_enc, F - 1 and both sides of every
               multiple of 8 from 96 (192) -- a dropped tile cannot hide behind dense weights
  trajectory   nfopp_traj_collision_eval with injected t == explicit-pose mode on the oracle's sample poses, bit for bit
  fit          nfopp_onf_train_grad_ex, fit path 2 on each matrix path and the per-sample path, P = 65, every block and the
               loss within fit_blocks_gate; workspace exactly nfopp_onf_train_workspace_bytes with guard words behind it
  refused      the return code, the message, and outputs that still hold their fill

`python tests/test_gpu_onf_geometries.py [file]` runs every cell and prints (or writes) the table kept in
profiles/onf_geometries.txt."""
import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("gpu_common")
from nfopp import _lib  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402

import bits_float64_gate as bg  # noqa: E402
import feature_probe_gate as fpg  # noqa: E402
import fit_blocks_gate as fg  # noqa: E402
import guarded  # noqa: E402
import onf_geometry_cases as gc  # noqa: E402

GUARD_BYTES = 4096           # 256 output rows behind (and in front of) every out4
GUARD_WORDS, FILL = 1024, 0x7FC12345        # tests/test_gpu_fit_blocks.py: a quiet NaN with a payload no kernel writes
# (tag, fit path, matrix path, chunk length of the yardstick, column of the table)
FITS = (("fit2 path0", 2, 0, 16, 0), ("fit2 path1", 2, 1, 32, 1), ("fit2 path2", 2, 2, 32, 2), ("per-sample", 1, 1, 32, None))
IDS = [gc.name(g).replace(" ", "-") for g in gc.NETWORKS]


class matrix_path(object):
    def __init__(self, path):
        self.path = path

    def __enter__(self):
        self.lib = _lib.load()
        self.before = self.lib.nfopp_get_matrix_path()
        _lib.check(self.lib.nfopp_set_matrix_path(self.path))
        return self.lib

    def __exit__(self, *exc):
        _lib.check(self.lib.nfopp_set_matrix_path(self.before))


def config_c(cfg):
    return _lib.OnfConfigC(cfg.mean, cfg.sigma, int(cfg.use_cos), int(cfg.bias), cfg.angle_dim)


def out4(P):
    """[P, 4] of NaN (bytes 0xFF) with guards on both sides"""
    return guarded.guarded((P, 4), torch.float32, "cuda", 0xFF, GUARD_BYTES)


def untouched(view, parent):
    return guarded.guards_intact(parent) and bool((guarded.bits(view) == 0xFFFFFFFF).all())


def refused(lib, rc, words):
    msg = lib.nfopp_last_error().decode()
    return rc == -1 and all(w in msg for w in words), (rc, msg)


def call_eval(lib, fn, c, params, xd, P):
    """-> (rc, out4 view, parent)"""
    view, parent = out4(P)
    rc = fn(c, _lib.ptr(params), _lib.ptr(xd), P, _lib.ptr(view), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, view, parent


# ----------------------------------------------------------------------------------------------------------
def run_inference(geom):
    """every matrix path of the geometry -> [bg.Row]"""
    e = gc.TABLE[geom[:2]]
    flat, cfg = gc.network(*geom)
    ref = gc.inference_reference(*geom)
    params, c = torch.tensor(flat, device="cuda"), config_c(cfg)
    rows = []
    for path in gc.MATRIX_PATHS:
        outcome = e.inf[path]
        tag = "path%d %s" % (path, outcome)
        with matrix_path(path) as lib:
            for P in gc.POSE_P:
                case = "%s P%d" % (gc.name(geom), P)
                xd = torch.tensor(ref[P]["x"], device="cuda")
                got = {}
                for key, fn in (("full", lib.nfopp_onf_eval_points), ("forward", lib.nfopp_onf_eval_logits)):
                    rc, view, parent = call_eval(lib, fn, c, params, xd, P)
                    if outcome not in gc.COMPUTED:
                        ok, why = refused(lib, rc, gc.refusal(e, outcome))
                        bg.fact(rows, tag, case, "%s is refused with its message: %r" % (key, why), ok)
                        bg.fact(rows, tag, case, "%s: the refused call writes nothing" % key, untouched(view, parent))
                        continue
                    _lib.check(rc)
                    bg.fact(rows, tag, case, "%s: guard rows intact" % key, guarded.guards_intact(parent))
                    rc2, again, parent2 = call_eval(lib, fn, c, params, xd, P)
                    _lib.check(rc2)
                    bg.fact(rows, tag, case, "%s: a repeat is bit-equal" % key, np.array_equal(guarded.bits(view), guarded.bits(again)))
                    got[key] = view.cpu().numpy()
                if got:
                    rows += gc.compare_inference(tag, geom, P, ref, **got)
    return rows


@pytest.mark.parametrize("geom", gc.NETWORKS, ids=IDS)
def test_inference_on_every_matrix_path(geom):
    rows = run_inference(geom)
    print("\n".join(bg.summary(rows)))
    assert len(rows) >= 3 * 2 * 4 and not bg.failures(rows), bg.failures(rows)


# ----------------------------------------------------------------------------------------------------------
def run_readout(geom):
    """-> fpg.Stats over every computed matrix path and probed position"""
    use_cos, angle_dim, has_bias = geom
    e = gc.TABLE[geom[:2]]
    cfg = gc.probe_config(*geom)
    positions = gc.probe_positions(use_cos, angle_dim)
    nets = [gc.probe_params(use_cos, angle_dim, has_bias, f) for f in positions]
    row = (cfg.n_params() + 63) // 64 * 64
    host = np.zeros((len(nets), row), np.float32)
    for i, p in enumerate(nets):
        host[i, :cfg.n_params()] = orc.pack_params(p, cfg)
    params, c = torch.tensor(host, device="cuda"), config_c(cfg)
    x = gc.probe_poses(use_cos, angle_dim)
    xd = torch.tensor(x, device="cuda")
    P, D = x.shape
    stats = fpg.Stats(fpg.MFMA)
    expected = []
    for f, p in zip(positions, nets):
        tab = fpg.table(cfg, p)
        r_val, r_d, arg = fpg.evaluate(tab, x, [f])
        e_val, e_d, _ = fpg.evaluate(tab, x, [f], fpg.hw_sine)
        w = (0.0, 0.0, float(tab.c0[f])) if tab.isa[f] else (float(tab.c0[f]), float(tab.c1[f]), 0.0)
        assert np.abs(arg).max() < 4.0
        expected.append((int(tab.q[f]), r_val[:, 0], r_d[:, 0], e_val[:, 0], e_d[:, 0], arg[:, 0], w))
    for path in gc.MATRIX_PATHS:
        if e.inf[path] not in gc.COMPUTED:
            continue
        with matrix_path(path) as lib:
            out = torch.full((len(nets), 2, P, 4), float("nan"), device="cuda")
            for i in range(len(nets)):
                for k, fn in enumerate((lib.nfopp_onf_eval_points, lib.nfopp_onf_eval_logits)):
                    _lib.check(fn(c, _lib.ptr(params[i]), _lib.ptr(xd), P, _lib.ptr(out[i, k]), _lib.stream_ptr()))
            host_out = out.cpu().numpy()
        for i, f in enumerate(positions):
            q, r_val, r_d, e_val, e_d, arg, w = expected[i]
            tag = "%s path %d f%d" % (gc.name(geom), path, f)
            full, fwd = host_out[i, 0], host_out[i, 1]
            stats.gate(tag + " logit", full[:, 0], r_val, e_val, arg, q)
            stats.gate(tag + " logit (forward only)", fwd[:, 0], r_val, e_val, arg, q)
            stats.exact_zero(tag + ": the zeros of the forward-only entry", fwd[:, 1:])
            for col in range(3):
                if w[col] != 0:
                    assert col < D
                    stats.gate(tag + " grad[%d]" % col, full[:, 1 + col], r_d, e_d, arg, q + 1, weight=w[col])
                else:
                    stats.exact_zero(tag + " grad[%d]" % col, full[:, 1 + col])
    return stats


@pytest.mark.parametrize("geom", gc.NETWORKS, ids=IDS)
def test_single_feature_readout(geom):
    stats = run_readout(geom)
    e = gc.TABLE[geom[:2]]
    computed = sum(o in gc.COMPUTED for o in e.inf)
    positions = gc.probe_positions(*geom[:2])
    n_enc = 200 if e.use_cos else 100
    assert stats.count.sum() == computed * gc.PROBE_P * sum(3 if f >= n_enc else 4 for f in positions)
    assert stats.cap_worst <= fpg.CAP
    assert not stats.failures, "%d outside the gate, first: %s" % (len(stats.failures), stats.failures[:6])


# ----------------------------------------------------------------------------------------------------------
def run_trajectory(geom):
    """-> [(path, refused or bit-equal?, detail)]"""
    e = gc.TABLE[geom[:2]]
    flat, cfg = gc.network(*geom)
    traj, t, samples = gc.trajectory(*geom[:2])
    B, N, D = traj.shape
    params, c = torch.tensor(flat, device="cuda"), config_c(cfg)
    td, sd = torch.tensor(traj, device="cuda"), torch.tensor(samples, device="cuda")
    res = []
    for path in gc.MATRIX_PATHS:
        with matrix_path(path) as lib:
            tt = torch.tensor(t, device="cuda")
            view, parent = out4(B * (N - 1))
            rc = lib.nfopp_traj_collision_eval(c, _lib.ptr(params), _lib.ptr(td), B, N, D, _lib.ptr(tt), 0, 0, 0, 0, _lib.ptr(view),
                                               None, None, _lib.stream_ptr())
            torch.cuda.synchronize()
            if e.inf[path] not in gc.COMPUTED:
                ok, why = refused(lib, rc, gc.refusal(e, e.inf[path]))
                res.append((path, ok and untouched(view, parent), why))
                continue
            _lib.check(rc)
            rc, poses_out, parent2 = call_eval(lib, lib.nfopp_onf_eval_points, c, params, sd, B * (N - 1))
            _lib.check(rc)
            same = np.array_equal(guarded.bits(view), guarded.bits(poses_out)) and not np.isnan(view.cpu().numpy()).any()
            res.append((path, same and guarded.guards_intact(parent) and np.array_equal(tt.cpu().numpy(), t), "bits differ"))
    return res


@pytest.mark.parametrize("geom", gc.NETWORKS, ids=IDS)
def test_trajectory_mode_equals_pose_mode_bit_for_bit(geom):
    res = run_trajectory(geom)
    assert len(res) == 3 and all(ok for _, ok, _ in res), res


# ----------------------------------------------------------------------------------------------------------
def launch_fit(lib, c, params, n_params, x, y, fit_path):
    """one nfopp_onf_train_grad_ex call on FILL-ed buffers, workspace exactly as large as asked -> (rc, grad words, guards ok)"""
    P = x.shape[0]
    need = lib.nfopp_onf_train_workspace_bytes(c, P)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4 + GUARD_WORDS,), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    grad = torch.full((n_params + 2 + GUARD_WORDS,), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    rc = lib.nfopp_onf_train_grad_ex(c, _lib.ptr(params), _lib.ptr(xd), _lib.ptr(yd), P, 1.0 / P, _lib.ptr(grad), _lib.ptr(ws), need,
                                     fit_path, _lib.stream_ptr())
    torch.cuda.synchronize()
    guards = bool((ws[need // 4:].view(torch.int32) == FILL).all()) and bool((grad[n_params + 2:].view(torch.int32) == FILL).all())
    return rc, grad[:n_params + 2].cpu().numpy(), guards


def run_fit(geom):
    e = gc.TABLE[geom[:2]]
    flat, cfg = gc.network(*geom)
    ref = gc.fit_reference(*geom)
    params, c = torch.tensor(flat, device="cuda"), config_c(cfg)
    rows = []
    for tag, fit_path, path, K, column in FITS:
        outcome = e.per_sample if column is None else e.fit[column]
        case = gc.name(geom)
        with matrix_path(path) as lib:
            rc, g, guards = launch_fit(lib, c, params, cfg.n_params(), ref["x"], ref["y"], fit_path)
            bg.fact(rows, tag, case, "guard words behind the workspace and the gradient", guards)
            if outcome not in gc.COMPUTED:
                ok, why = refused(lib, rc, gc.refusal(e, outcome))
                bg.fact(rows, tag, case, "refused with its message: %r" % (why,), ok)
                bg.fact(rows, tag, case, "the refused fit leaves grad alone", bool((g.view(np.uint32) == FILL).all()))
                continue
            _lib.check(rc)
            rows += gc.compare_fit(tag, geom, ref, g, K)
            bg.fact(rows, tag, case, "every word is finite", np.isfinite(g).all())
            rc, again, _ = launch_fit(lib, c, params, cfg.n_params(), ref["x"], ref["y"], fit_path)
            _lib.check(rc)
            bg.fact(rows, tag, case, "a second launch gives the same words", np.array_equal(g.view(np.uint32), again.view(np.uint32)))
    return rows


@pytest.mark.parametrize("geom", gc.NETWORKS, ids=IDS)
def test_fit_gradient_block_by_block(geom):
    rows = run_fit(geom)
    print("\n".join(fg.table(rows)))
    assert len(rows) >= 4 * 3 and not bg.failures(rows), bg.failures(rows)


@pytest.mark.parametrize("geom", gc.UNSUPPORTED, ids=gc.name)
def test_an_unsupported_geometry_writes_nothing(geom):
    e = gc.TABLE[geom]
    c = _lib.OnfConfigC(gc.MEAN, gc.SIGMA, e.use_cos, 1, e.angle_dim)
    n_params = _lib.load().nfopp_onf_param_count(c)
    params = torch.zeros(n_params, device="cuda")
    P = 33
    xd = torch.zeros(P, 3, device="cuda")
    words = gc.refusal(e, "U")
    for path in gc.MATRIX_PATHS:
        with matrix_path(path) as lib:
            for fn in (lib.nfopp_onf_eval_points, lib.nfopp_onf_eval_logits):
                rc, view, parent = call_eval(lib, fn, c, params, xd, P)
                ok, why = refused(lib, rc, words)
                assert ok and untouched(view, parent), why
            view, parent = out4(8)
            tt = torch.zeros(8, device="cuda")
            rc = lib.nfopp_traj_collision_eval(c, _lib.ptr(params), _lib.ptr(xd), 1, 9, 3, _lib.ptr(tt), 0, 0, 0, 0, _lib.ptr(view), None, None,
                                               _lib.stream_ptr())
            torch.cuda.synchronize()
            ok, why = refused(lib, rc, words)
            assert ok and untouched(view, parent), why
            for fit_path in (1, 2):
                rc, g, guards = launch_fit(lib, c, params, n_params, np.zeros((P, 3), np.float32), np.zeros(P, np.float32), fit_path)
                ok, why = refused(lib, rc, words)
                assert ok and guards and bool((g.view(np.uint32) == FILL).all()), why


# ----------------------------------------------------------------------------------------------------------
def main(out=None):
    """worst error in units of the yardstick per (geometry, matrix path, array): inference ratio = |dev - f64| over
    max(|oracle32 - f64|, 1 ulp of the scale), gate 8; fit = worst e / bound over the blocks and the loss, gate 1"""
    lines = ["%-18s %-11s %9s %9s %9s   %s" % ("geometry", "cell", "logit", "grad", "logit fwd", "fit: worst block e/bound")]
    failures = []
    for geom in gc.NETWORKS:
        e = gc.TABLE[geom[:2]]
        inf, fit = run_inference(geom), run_fit(geom)
        stats = run_readout(geom)
        traj = run_trajectory(geom)
        failures += bg.failures(inf) + bg.failures(fit) + stats.failures + ["%s trajectory path %d: %s" % (gc.name(geom), p, why)
                                                                          for p, ok, why in traj if not ok]
        for path in gc.MATRIX_PATHS:
            tag = "path%d %s" % (path, e.inf[path])
            worst = collections.OrderedDict((a, max([bg.ratio(r) for r in inf if r.family == tag and r.array == a] or [float("nan")]))
                                            for a in ("logit", "grad", "logit fwd"))
            fr = [r for r in fit if r.family.startswith("fit2 path%d" % path) and r.scale > 0]
            cell = "refused (%s)" % e.fit[path] if not fr else "%.3f at %s" % max((r.got_err / r.bound, r.array) for r in fr)
            lines.append("%-18s %-11s %9.2f %9.2f %9.2f   %s" % ((gc.name(geom), tag) + tuple(worst.values()) + (cell,)))
        fr = [r for r in fit if r.family.startswith("per-sample") and r.scale > 0]
        lines.append("%-18s %-11s %9s %9s %9s   %.3f at %s" % ((gc.name(geom), "per-sample", "", "", "") + max((r.got_err / r.bound, r.array) for r in fr)))
        lines.append("%-18s %-11s read-out: %d values, worst |dev - r| %.3g; trajectory mode == pose mode (refused: untouched) on %d paths"
                     % (gc.name(geom), "", stats.count.sum(), stats.worst[..., 0].max(), sum(ok for _, ok, _ in traj)))
    lines.append("%d outside the gate" % len(failures))
    lines += failures[:60]
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    import sys
    main(sys.argv[1] if len(sys.argv) > 1 else None)
