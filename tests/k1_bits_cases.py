"""The launches of the 32x32 ONF kernel (matrix path 1, csrc/onf_x32_impl.h) whose output bits are pinned by
tests/golden/k1_bits.npz: shared by the recorder (tools/x32/record_k1_bits.py) and tests/test_gpu_k1_bits.py.

Every case has a fixed seed and explicit draws `t`, goes through the C ABI, and returns plain arrays:
  pose_F<fin>_P<P>      out4 [P, 4] of nfopp_onf_eval_points, P = 1 (one padded tile), 33 (a tile and a bit), 255 / 257 (both
                        sides of a chunk edge; both lane halves form poses there)
  traj_F<fin>           out4 [3, 8, 4] of nfopp_traj_collision_eval, B = 3, N = 9, injected draws
  logits_F<fin>         out4 [257, 4] of nfopp_onf_eval_logits (forward-only kernel)
  big_rows / big_sum    one pose launch of CUs x 256 + 31 points (the smallest launch on the 512-thread shape, ragged last chunk):
                        a fixed strided row sample and the sum of all words as uint32, in uint64
  fit_F<fin>_P<P>_*     pass 1 of the fit (h1 | rho dh1 | rho de | record) for 220 and 100 inputs at P = 33 (full) and 257 (rows
                        BIG_FIT_ROWS in full, plus the per-row and per-column uint32 sums of every array)
  params_sum_F<fin>     uint32 sum of the parameter vector: tells a drifted initialiser from a changed kernel"""
import numpy as np
import torch

import nfopp
from nfopp import _lib

F32 = np.float32
# (use_cos, angle, bias) of the four feature dimensions, as tests/test_gpu_split_path.py has them
DIMS = {220: (True, True, True), 200: (True, False, True), 120: (False, True, False), 100: (False, False, True)}
POSE_P = (1, 33, 255, 257)
FIT_DIMS, FIT_P = (220, 100), (33, 257)
BIG_FIT_ROWS = np.array(sorted(set(range(0, 257, 8)) | set(range(124, 132)) | set(range(252, 257))))
BIG_STRIDE, BIG_TAIL = 257, 64


def wsum(a):
    """sum of the array's 32-bit words, exact in uint64"""
    return np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum(dtype=np.uint64)


def wsum_axis(a, axis):
    return np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum(axis=axis, dtype=np.uint64)


def make_onf(fin):
    use_cos, angle, bias = DIMS[fin]
    torch.random.manual_seed(1000 + fin)
    return nfopp.ONF(0.4, 2.5, use_cos=use_cos, use_normal_init=True, bias=bias, angle_encoding=angle).to("cuda")


def points(fin, n, seed):
    angle = DIMS[fin][1]
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4, 6, (n, 3 if angle else 2)).astype(F32)
    if angle:
        x[:, 2] = rng.uniform(-3.3, 3.3, n).astype(F32)
    return x


def big_count():
    return torch.cuda.get_device_properties(0).multi_processor_count * 256 + 31


def _eval(lib, fn, onf, x):
    xd = torch.tensor(x, device="cuda")
    out = torch.full((x.shape[0], 4), float("nan"), device="cuda")
    _lib.check(fn(onf.config_c(), _lib.ptr(onf.flat_parameters), _lib.ptr(xd), x.shape[0], _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _traj(lib, onf, fin):
    B, N, D = 3, 9, (3 if DIMS[fin][1] else 2)
    rng = np.random.default_rng(300 + fin)
    traj = rng.uniform(-4, 6, (B, N, D)).astype(F32)
    if D == 3:
        traj[:, :, 2] = rng.uniform(-3.3, 3.3, (B, N)).astype(F32)
    t = rng.uniform(0, 1, (B, N - 1)).astype(F32)
    td, tt = torch.tensor(traj, device="cuda"), torch.tensor(t, device="cuda")
    out = torch.full((B, N - 1, 4), float("nan"), device="cuda")
    _lib.check(lib.nfopp_traj_collision_eval(onf.config_c(), _lib.ptr(onf.flat_parameters), _lib.ptr(td), B, N, D, _lib.ptr(tt), 0,
                                             0, 0, 0, _lib.ptr(out), None, None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _fit(lib, onf, fin, P):
    """the four factor arrays pass 1 leaves at the front of the workspace (layout: tests/test_gpu_split_path.py)"""
    x = points(fin, P, 500 + fin + P)
    y = (np.random.default_rng(700 + fin + P).uniform(size=P) < 0.35).astype(F32)
    c = onf.config_c()
    need = lib.nfopp_onf_train_workspace_bytes(c, P)
    ws = torch.zeros((need + 3) // 4, dtype=torch.float32, device="cuda")
    grad = torch.zeros(onf.n_params + 2, device="cuda")
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    _lib.check(lib.nfopp_onf_train_grad_ex(c, _lib.ptr(onf.flat_parameters), _lib.ptr(xd), _lib.ptr(yd), P, 1.0 / P, _lib.ptr(grad),
                                           _lib.ptr(ws), ws.numel() * 4, 2, _lib.stream_ptr()))
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    win = 16 * ((fin + 16) // 16)
    o1, o2, o3 = P * 112, 2 * P * 112, 2 * P * 112 + P * win
    return dict(h1=w[:o1].reshape(P, 112), dh1=w[o1:o2].reshape(P, 112), de=w[o2:o3].reshape(P, win),
                rec=w[o3:o3 + P * 12].reshape(P, 12))


def run_cases():
    """every case on the current build, matrix path 1 -> {name: array}"""
    lib = _lib.load()
    before = lib.nfopp_get_matrix_path()
    _lib.check(lib.nfopp_set_matrix_path(1))
    res = {}
    try:
        for fin in DIMS:
            onf = make_onf(fin)
            res["params_sum_F%d" % fin] = wsum(onf.flat_parameters.cpu().numpy())
            for P in POSE_P:
                res["pose_F%d_P%d" % (fin, P)] = _eval(lib, lib.nfopp_onf_eval_points, onf, points(fin, P, 100 + fin + P))
            res["traj_F%d" % fin] = _traj(lib, onf, fin)
            res["logits_F%d" % fin] = _eval(lib, lib.nfopp_onf_eval_logits, onf, points(fin, 257, 200 + fin))
            if fin in FIT_DIMS:
                for P in FIT_P:
                    for k, v in _fit(lib, onf, fin, P).items():
                        name = "fit_F%d_P%d_%s" % (fin, P, k)
                        if P == 33:
                            res[name] = v.copy()
                        else:
                            res[name + "_rows"] = v[BIG_FIT_ROWS].copy()
                            res[name + "_rowsum"] = wsum_axis(v, 1)
                            res[name + "_colsum"] = wsum_axis(v, 0)
            if fin == 220:
                n = big_count()
                out = _eval(lib, lib.nfopp_onf_eval_points, onf, points(fin, n, 900))
                res["big_count"] = np.int64(n)
                res["big_rows"] = np.concatenate([out[::BIG_STRIDE], out[-BIG_TAIL:]])
                res["big_sum"] = wsum(out)
    finally:
        _lib.check(lib.nfopp_set_matrix_path(before))
    return res
