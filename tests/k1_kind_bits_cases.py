"""The launches of the 32x32 ONF kernel (matrix path 1, csrc/onf_x32_impl.h) that stress the input blocks whose feature
kinds are fixed at compile time (the blocks from Cfg::FS on: positional / angle / ones / pad positions) and the last
output tile's chain-rule epilogue; their output bits are pinned by tests/golden/k1_kind_bits.npz.  Shared by the recorder
(tools/x32/record_k1_kind_bits.py) and tests/test_gpu_k1_kind_bits.py; networks, random poses and the fit's read-back are
those of tests/k1_bits_cases.py.

  pose_F<fin>_P<P>    out4 [P, 4] of nfopp_onf_eval_points at P = 33 and 65 (one and two full tiles and a bit)
  edge_F<fin>         out4 of the poses of edge_poses(): theta < 0, -0, +0, > 0 and +-pi, each at a random place and at
                      u_x = u_y = 0 (x = y = the model's mean) -- the pad positions that share a four-slot group with angle
                      features then see (theta + 0) * 0 with both signs of zero
  traj_F<fin>         out4 [2, 4, 4] of nfopp_traj_collision_eval, B = 2, N = 5, injected draws (220 and 120 inputs)
  fit_F<fin>_P33_*    pass 1 of the fit (h1 | rho dh1 | rho de | record) for 220 inputs and for 120, the shape with a group
                      whose lane halves hold different kinds"""
import numpy as np
import torch

from nfopp import _lib

import k1_bits_cases as kc

F32 = np.float32
DIMS = kc.DIMS
POSE_P = (33, 65)
TRAJ_DIMS = (220, 120)
FIT_DIMS, FIT_P = (220, 120), 33
MEAN = 0.4          # of kc.make_onf: x = y = MEAN is u = 0 exactly
THETAS = (-1.3, -0.0, 0.0, 2.1, float(np.float32(np.pi)), -float(np.float32(np.pi)), float(np.pi), -float(np.pi))


def edge_poses(fin):
    """every theta of THETAS at a random place and at u = 0; without angle features: the random places and u = 0"""
    angle = DIMS[fin][1]
    rng = np.random.default_rng(400 + fin)
    rows = []
    for th in THETAS:
        xy = rng.uniform(-4, 6, 2)
        rows.append([xy[0], xy[1], th])
        rows.append([MEAN, MEAN, th])
    x = np.array(rows, F32)
    return x if angle else np.ascontiguousarray(x[:, :2])


def _traj(lib, onf, fin):
    B, N, D = 2, 5, (3 if DIMS[fin][1] else 2)
    rng = np.random.default_rng(600 + fin)
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


def run_cases():
    """every case on the current build, matrix path 1 -> {name: array}"""
    lib = _lib.load()
    before = lib.nfopp_get_matrix_path()
    _lib.check(lib.nfopp_set_matrix_path(1))
    res = {}
    try:
        for fin in DIMS:
            onf = kc.make_onf(fin)
            res["params_sum_F%d" % fin] = kc.wsum(onf.flat_parameters.cpu().numpy())
            for P in POSE_P:
                res["pose_F%d_P%d" % (fin, P)] = kc._eval(lib, lib.nfopp_onf_eval_points, onf, kc.points(fin, P, 1100 + fin + P))
            res["edge_F%d" % fin] = kc._eval(lib, lib.nfopp_onf_eval_points, onf, edge_poses(fin))
            if fin in TRAJ_DIMS:
                res["traj_F%d" % fin] = _traj(lib, onf, fin)
            if fin in FIT_DIMS:
                for k, v in kc._fit(lib, onf, fin, FIT_P).items():
                    res["fit_F%d_P%d_%s" % (fin, FIT_P, k)] = v.copy()
    finally:
        _lib.check(lib.nfopp_set_matrix_path(before))
    return res
