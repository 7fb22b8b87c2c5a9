"""GPU: every ONF input feature and its derivative, one by one, against float64 over the argument range the kernels promise
(|arg| < 1e5): the probes of tests/feature_probe_cases.py, held to the gate of tests/feature_probe_gate.py.

  Probe A   nfopp_onf_eval_points and nfopp_onf_eval_logits on matrix paths 1, 2 and 0: per probed position and operand
            variant, logit = s_f(arg) and d logit / d pose = s_f'(arg) x (wx, wy, fr); every other component == 0
  Probe B   nfopp_onf_train_grad_ex, fit path 2 on matrix paths 1, 2 and 0 (pass 1 = K1's chain in training mode, pass 2's
            re-evaluation) and fit path 1 (the per-sample kernels, sin_quadrant): all positions in one call, read out of
            grad[w3 skip], grad[be], grad[we][:, 0] and grad[ang_f]; grad[b3] == -1 bit for bit, the hidden blocks == 0

Every output buffer is filled with NaN before each call.  `python tests/test_gpu_feature_probe.py [file]` runs every probe
and prints (or writes) the table kept in profiles/feature_probe.txt."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
from nfopp import _lib  # noqa: E402

import feature_probe_cases as pc  # noqa: E402
import feature_probe_gate as fg  # noqa: E402

FINS = sorted(pc.DIMS)
MATRIX_PATHS = (1, 2, 0)
# (tag, fit path, matrix path, gate)
FITS = (("fit2 path1", 2, 1, fg.MFMA), ("fit2 path2", 2, 2, fg.MFMA), ("fit2 path0", 2, 0, fg.MFMA), ("per-sample", 1, 1, fg.PER_SAMPLE))
ROW_ALIGN = 64          # floats: every network of a stack starts on a 256-byte boundary, like a buffer of its own


def config_c(fin):
    cfg = pc.config(fin)
    return _lib.OnfConfigC(cfg.mean, cfg.sigma, int(cfg.use_cos), int(cfg.bias), cfg.angle_dim)


def stack(fin, networks):
    """the flat parameters of several networks in one device buffer [n, row]: one upload per test"""
    n_params = pc.config(fin).n_params()
    row = (n_params + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN
    host = np.zeros((len(networks), row), np.float32)
    for i, p in enumerate(networks):
        host[i, :n_params] = pc.flat(fin, p)
    return torch.tensor(host, device="cuda")


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


@functools.lru_cache(None)
def expected_a(fin):
    """computed once, shared by the matrix paths, never changed"""
    return tuple(fg.expect_a(case, fg.MFMA) for case in pc.probe_a_cases(fin))


@functools.lru_cache(None)
def expected_b(fin, gate):
    return tuple(fg.expect_b(fin, c, gate) for c in range(pc.probe_b_calls(fin)))


def run_probe_a(fin, path):
    cases = pc.probe_a_cases(fin)
    params = stack(fin, [pc.probe_a_params(case) for case in cases])
    c = config_c(fin)
    stats = fg.Stats(fg.MFMA)
    with matrix_path(path) as lib:
        for i, (case, exp) in enumerate(zip(cases, expected_a(fin))):
            P = case.x.shape[0]
            xd = torch.tensor(case.x, device="cuda")
            out = torch.full((2, P, 4), float("nan"), device="cuda")
            for k, fn in enumerate((lib.nfopp_onf_eval_points, lib.nfopp_onf_eval_logits)):
                _lib.check(fn(c, _lib.ptr(params[i]), _lib.ptr(xd), P, _lib.ptr(out[k]), _lib.stream_ptr()))
            both = out.cpu().numpy()
            full, fwd = both[0], both[1]
            D = case.x.shape[1]
            grad = np.zeros((P, 3), np.float32)
            grad[:, :D] = full[:, 1:1 + D]
            fg.check_a(stats, case, exp, full[:, 0], grad)
            stats.exact_zero("A F%d f%d %s: the slots past the pose dimension" % (fin, case.f, case.variant), full[:, 1 + D:])
            fg.check_a(stats, case._replace(variant=case.variant + " (forward only)"), exp, fwd[:, 0])
            stats.exact_zero("A F%d f%d %s: the zeros of the forward-only entry" % (fin, case.f, case.variant), fwd[:, 1:])
    return stats


def run_probe_b(fin, fit_path, path, gate):
    cfg = pc.config(fin)
    n = pc.probe_b_calls(fin)
    params = stack(fin, [pc.probe_b_params(fin, c) for c in range(n)])
    c = config_c(fin)
    xd, yd = torch.tensor(pc.probe_b_pose(fin), device="cuda"), torch.ones(1, device="cuda")
    stats = fg.Stats(gate)
    with matrix_path(path) as lib:
        need = lib.nfopp_onf_train_workspace_bytes(c, 1)
        assert need > 0 and need % 4 == 0
        ws = torch.empty(need // 4, device="cuda")
        grads = torch.empty((n, cfg.n_params() + 2), device="cuda")
        for i in range(n):
            ws.fill_(float("nan"))
            grads[i].fill_(float("nan"))
            _lib.check(lib.nfopp_onf_train_grad_ex(c, _lib.ptr(params[i]), _lib.ptr(xd), _lib.ptr(yd), 1, 1.0, _lib.ptr(grads[i]),
                                                   _lib.ptr(ws), need, fit_path, _lib.stream_ptr()))
        host = grads.cpu().numpy()
    for i, exp in enumerate(expected_b(fin, gate)):
        stats.fact("B F%d call %d: the count slot is not 1" % (fin, i), host[i, -1] == 1)
        fg.check_b(stats, fin, i, exp, fg.unpack(cfg, host[i, :-2]))
    return stats


def _report(tag, stats):
    print("\n".join(stats.lines(tag)))
    assert stats.cap_worst <= fg.CAP
    assert not stats.failures, "%d outside the gate, first: %s" % (len(stats.failures), stats.failures[:6])


@pytest.mark.parametrize("path", MATRIX_PATHS)
@pytest.mark.parametrize("fin", FINS)
def test_probe_a_inference(fin, path):
    stats = run_probe_a(fin, path)
    assert stats.count.sum() == len(pc.probe_a_cases(fin)) * len(pc.probe_a_arguments()) * 3 \
        + sum(c.variant == "grid" and not pc.is_angle(fin, c.f) for c in pc.probe_a_cases(fin)) * len(pc.probe_a_arguments())
    _report("A F%d matrix path %d" % (fin, path), stats)


@pytest.mark.parametrize("tag,fit_path,path,gate", FITS, ids=[f[0].replace(" ", "-") for f in FITS])
@pytest.mark.parametrize("fin", FINS)
def test_probe_b_fit(fin, tag, fit_path, path, gate):
    stats = run_probe_b(fin, fit_path, path, gate)
    _report("B F%d %s" % (fin, tag), stats)


def main(out=None):
    lines, failures = [], []
    for kind, launches in (("A", [("matrix path %d" % p, p) for p in MATRIX_PATHS]), ("B", FITS)):
        for launch in launches:
            total = None
            for fin in FINS:
                s = run_probe_a(fin, launch[1]) if kind == "A" else run_probe_b(fin, *launch[1:])
                failures += s.failures
                total = s if total is None else total.merge(s)
            lines += total.lines("%s %s" % (kind, launch[0])) + [""]
    lines.append("%d values outside the gate" % len(failures))
    lines += failures[:40]
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    import sys
    main(sys.argv[1] if len(sys.argv) > 1 else None)
