"""GPU: the bits of an ONF sample do not depend on where the sample sits in the launch.

include/nfopp_hip.h promises for matrix path 1 that "results do not depend on the batch size or on how a batch is sharded".
A lane-level slip in a tile -- a remainder row, a lane swap, the second point tile of a wave -- is a sample whose bits change
with its row, and no tolerance test sees that until it is large.  Everything here is compared with == on bits:

  * one pose repeated P times gives P identical rows, on every matrix path (every column of a tile runs the same instructions);
  * a slice of a batch evaluated on its own gives the rows of the whole batch: across both workgroup shapes on path 1 (the
    header's promise), and inside the one-tile-per-wave range (launches below 16384 points) on paths 2 and 0, for which the
    header promises nothing across their switch to two tiles per wave;
  * pass 1 of the fit on path 1 leaves the same workspace rows for a sample whether the fit started 7 samples earlier or not.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
from nfopp import _lib  # noqa: E402

F32 = np.float32
# (use_cos, angle, bias): F = 220, 200, 120, 100, and 200 without the encoding bias
CONFIGS = [(True, True, True), (True, False, True), (False, True, False), (False, False, True), (True, False, False)]
COUNTS = (1, 33, 300, 4099, 70001)
MEAN, SIGMA = 0.4, 2.5
# 8 poses: inside the range the field was normalised for, on its rim, far outside it, |theta| > pi, zeros, tiny values
POSES = np.array([[0.4, 0.4, 0.0], [1.7, -2.3, 3.0], [-4.0, 6.0, -3.3], [40.0, -35.0, 3.3], [-250.0, 300.0, 9.5],
                  [2.9, 2.9, -7.0], [0.0, 0.0, -0.0], [1e-6, -1e-6, 1e-3]], F32)

_ONFS = {}


def _onf(cfg):
    """one field per configuration for the whole module (the tests only read it)"""
    if cfg not in _ONFS:
        use_cos, angle, bias = cfg
        torch.random.manual_seed(11)
        _ONFS[cfg] = nfopp.ONF(MEAN, SIGMA, use_cos=use_cos, use_normal_init=True, bias=bias, angle_encoding=angle).to("cuda")
    return _ONFS[cfg]


def _eval(onf, x, entry):
    """raw C entry on the current matrix path: out4 [P, 4] as int32 bits"""
    lib = _lib.load()
    out = torch.empty(x.shape[0], 4, dtype=torch.float32, device="cuda")
    fn = getattr(lib, entry)
    _lib.check(fn(onf.config_c(), _lib.ptr(onf.flat_parameters), _lib.ptr(x), x.shape[0], _lib.ptr(out), _lib.stream_ptr()))
    return out.view(torch.int32)


def _set_path(path):
    _lib.check(_lib.load().nfopp_set_matrix_path(path))    # tests/conftest.py puts the switch back after every test


def _random_poses(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4, 6, (n, d)).astype(F32)
    if d == 3:
        x[:, 2] = rng.uniform(-3.3, 3.3, n)
    return x


@pytest.mark.parametrize("entry", ["nfopp_onf_eval_points", "nfopp_onf_eval_logits"])
@pytest.mark.parametrize("path", [1, 2, 0])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_one_pose_repeated_gives_identical_rows(cfg, path, entry):
    onf = _onf(cfg)
    d = onf.point_dim
    _set_path(path)
    for k, pose in enumerate(POSES):
        row = torch.tensor(pose[:d].copy(), device="cuda")
        first = None
        for P in COUNTS:
            out = _eval(onf, row.repeat(P, 1).contiguous(), entry)
            same = bool((out == out[:1]).all())
            assert same, (cfg, path, entry, k, P, int((out != out[:1]).any(1).sum()))
            if path == 1:       # the header's promise: the batch size does not enter either
                first = out[0].clone() if first is None else first
                assert torch.equal(out[0], first), (cfg, entry, k, P)


SLICES_FULL = [(0, 1), (1, 34), (31, 331), (5, 4104), (0, 4099), (65000, 70001)]
# paths 2 and 0: every launch below 16384 points; the last slice keeps its length and ends with the batch
N_SMALL = 16383
SLICES_SMALL = [(0, 1), (1, 34), (31, 331), (5, 4104), (0, 4099), (N_SMALL - 5001, N_SMALL)]


@pytest.mark.parametrize("entry", ["nfopp_onf_eval_points", "nfopp_onf_eval_logits"])
@pytest.mark.parametrize("path", [1, 2, 0])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_a_slice_evaluated_alone_equals_its_rows_of_the_batch(cfg, path, entry):
    onf = _onf(cfg)
    d = onf.point_dim
    _set_path(path)
    n, slices = (70001, SLICES_FULL) if path == 1 else (N_SMALL, SLICES_SMALL)
    x = torch.tensor(_random_poses(70001, d, 29)[:n], device="cuda")
    full = _eval(onf, x, entry)
    for a, b in slices:
        part = _eval(onf, x[a:b].contiguous(), entry)
        bad = (part != full[a:b]).any(1)
        assert not bool(bad.any()), (cfg, path, entry, (a, b), int(bad.sum()), bad.nonzero()[:8].flatten().tolist())
    for p in range(64):
        one = _eval(onf, x[p:p + 1].contiguous(), entry)
        assert torch.equal(one[0], full[p]), (cfg, path, entry, p)


def _fit_workspace(onf, x, y, inv_count):
    """pass 1 + weight-gradient GEMMs (fit path 2) on matrix path 1; the workspace as int32 bits, pre-filled with 0xFF"""
    lib = _lib.load()
    P = x.shape[0]
    c = onf.config_c()
    need = lib.nfopp_onf_train_workspace_bytes(c, P)
    ws = torch.full(((need + 3) // 4,), -1, dtype=torch.int32, device="cuda")
    grad = torch.full((onf.n_params + 2,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.nfopp_onf_train_grad_ex(c, _lib.ptr(onf.flat_parameters), _lib.ptr(x), _lib.ptr(y), P, inv_count,
                                           grad.data_ptr(), ws.data_ptr(), need, 2, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return ws


def _factor_rows(ws, P, fin):
    """h1 [P,112] | rho*dh1 [P,112] | rho*de [P,win] | record [P,12]: the layout test_gpu_split_path.py documents"""
    win = 16 * ((fin + 16) // 16)
    o1, o2, o3 = P * 112, 2 * P * 112, 2 * P * 112 + P * win
    return (ws[:o1].view(P, 112), ws[o1:o2].view(P, 112), ws[o2:o3].view(P, win), ws[o3:o3 + P * 12].view(P, 12))


@pytest.mark.parametrize("cfg", [(True, True, True), (False, False, True)])      # F = 220 / 100: even / odd input blocks
def test_fit_pass1_rows_do_not_depend_on_where_the_fit_starts(cfg):
    onf = _onf(cfg)
    d = onf.point_dim
    _set_path(1)
    P, shift = 4099, 7
    rng = np.random.default_rng(31)
    x = torch.tensor(_random_poses(P, d, 37), device="cuda")
    y = torch.tensor((rng.uniform(size=P) < 0.35).astype(F32), device="cuda")
    inv_count = 1.0 / P
    whole = _factor_rows(_fit_workspace(onf, x, y, inv_count), P, onf.feature_dim)
    tail = _factor_rows(_fit_workspace(onf, x[shift:].contiguous(), y[shift:].contiguous(), inv_count), P - shift, onf.feature_dim)
    for name, a, b in zip(("h1", "rho*dh1", "rho*de", "record"), whole, tail):
        bad = (a[shift:] != b).any(1)
        assert not bool(bad.any()), (cfg, name, int(bad.sum()), bad.nonzero()[:8].flatten().tolist())
