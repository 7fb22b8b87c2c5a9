"""The launches whose output bits tests/golden/k1_claim_bits.npz pins across the change from a fixed tile walk to tiles by
claim (csrc/onf_x32_impl.h, "Tiles by claim"): shared by tools/x32/record_k1_claim_bits.py (run on the build IN FRONT of the
change) and tests/test_gpu_k1_claim_bits.py.  Matrix path 1; parameters and poses from the seeded generators of
tests/k1_bits_cases.py.

With T = CUs x 256 samples, the launcher's threshold between the 256- and the 512-thread workgroup (csrc/onf_x32_impl.h:
launch_t), read from the library (nfopp_onf_wide_launch_threshold):
  points / logits, F = 220   P = 1, 33, 64, 65, 255, 257, 1023 (256 threads: pools of one or two tiles, odd numbers of
                             tiles with samples, a partial last tile) and T, T + 1, T + 256 + 33, 2 T - 31 (512 threads: one
                             chunk per workgroup; one workgroup with a second chunk holding a one-sample tile; a partial
                             pair; a nearly full second round)
  points / logits, F = 100   P = 65, T + 1
  traj                       nfopp_traj_collision_eval, F = 220, B = ceil(T / 255) + 40, N = 256, device draws, every third
                             trajectory retired through `active`
Every output buffer has GUARD rows behind the last one and is filled with a NaN payload pattern before each launch."""
import hashlib

import numpy as np
import torch

import k1_bits_cases as kc
from nfopp import _lib

GUARD = 64
PATTERN = 0x7FC5A5A5          # a quiet NaN no arithmetic produces
KEEP = 64                     # first and last rows kept in the fixture beside the hash
SMALL_P = (1, 33, 64, 65, 255, 257, 1023)
REPEATS = 8


def threshold():
    return int(_lib.load().nfopp_onf_wide_launch_threshold())


BIG_P = {"T": lambda T: T, "T+1": lambda T: T + 1, "T+256+33": lambda T: T + 256 + 33, "2T-31": lambda T: 2 * T - 31}


def pose_specs():
    """[(name, fin, entry point name, P or a key of BIG_P)]: names do not depend on the device"""
    specs = []
    for fn in ("points", "logits"):
        specs += [("%s_F220_P%d" % (fn, P), 220, fn, P) for P in SMALL_P]
        specs += [("%s_F220_P%s" % (fn, tag), 220, fn, tag) for tag in BIG_P]
        specs += [("%s_F100_P65" % fn, 100, fn, 65), ("%s_F100_PT+1" % fn, 100, fn, "T+1")]
    return specs


def pose_cases():
    """[(name, fin, entry point name, P)] on this device"""
    T = threshold()
    return [(name, fin, fn, BIG_P[P](T) if isinstance(P, str) else P) for name, fin, fn, P in pose_specs()]


def case_names():
    return [c[0] for c in pose_specs()] + ["traj_F220"]


def _filled(rows):
    return torch.full((rows, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)


class Runner:
    """holds the networks and inputs of the cases; run(name) launches once into a freshly filled buffer and returns it
    (device tensor of words, [rows + GUARD, 4] int32) with the number of rows the launch owns"""

    def __init__(self):
        self.lib = _lib.load()
        self.onf = {fin: kc.make_onf(fin) for fin in (220, 100)}
        self.cases = {c[0]: c for c in pose_cases()}
        self.inputs = {}
        self.last_draws = None

    def _traj_inputs(self):
        if "traj" not in self.inputs:
            B, N = (threshold() + 254) // 255 + 40, 256
            rng = np.random.default_rng(4242)
            traj = rng.uniform(-4, 6, (B, N, 3)).astype(np.float32)
            traj[:, :, 2] = rng.uniform(-3.3, 3.3, (B, N)).astype(np.float32)
            active = np.ones(B, np.uint8)
            active[::3] = 0
            self.inputs["traj"] = (B, N, torch.tensor(traj, device="cuda"), torch.tensor(active, device="cuda"), active,
                                   torch.zeros(B + 1, dtype=torch.int32, device="cuda"))
        return self.inputs["traj"]

    def retired_rows(self):
        B, N, _, _, active, _ = self._traj_inputs()
        return np.repeat(active == 0, N - 1)

    def run(self, name):
        lib = self.lib
        if name == "traj_F220":
            B, N, traj, active, _, live = self._traj_inputs()
            onf = self.onf[220]
            rows = B * (N - 1)
            out = _filled(rows + GUARD)
            t = _filled((rows + GUARD + 3) // 4).view(-1)       # the draws are written too: the same pattern and guard
            self.last_draws = t.view(torch.int32)                # (checked by the test: [rows] draws, then guard words)
            _lib.check(lib.nfopp_traj_collision_eval(onf.config_c(), _lib.ptr(onf.flat_parameters), _lib.ptr(traj), B, N, 3,
                                                     _lib.ptr(t), 1, 11, 5, 0, _lib.ptr(out), _lib.ptr(active, torch.uint8),
                                                     _lib.ptr(live, torch.int32),
                                                     _lib.stream_ptr()))
            return out.view(torch.int32), rows
        _, fin, fn, P = self.cases[name]
        if name not in self.inputs:
            self.inputs[name] = torch.tensor(kc.points(fin, P, 4000 + fin + P % 100003), device="cuda")
        x, onf = self.inputs[name], self.onf[fin]
        out = _filled(P + GUARD)
        entry = lib.nfopp_onf_eval_points if fn == "points" else lib.nfopp_onf_eval_logits
        _lib.check(entry(onf.config_c(), _lib.ptr(onf.flat_parameters), _lib.ptr(x), P, _lib.ptr(out), _lib.stream_ptr()))
        return out.view(torch.int32), P


def digest(words, rows):
    """what the fixture keeps of a launch: sha256 of the bytes of its rows (32 x uint8), the first and the last KEEP rows"""
    a = np.ascontiguousarray(words[:rows].cpu().numpy())
    sha = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()
    return sha, a[:KEEP].copy(), a[-KEEP:].copy()


def record():
    """every case on the current build -> {name_sha / name_head / name_tail: array, params_sum_F<fin>}"""
    lib = _lib.load()
    before = lib.nfopp_get_matrix_path()
    _lib.check(lib.nfopp_set_matrix_path(1))
    res = {"cus": np.int64(threshold() // 256)}
    try:
        r = Runner()
        for fin, onf in r.onf.items():
            res["params_sum_F%d" % fin] = kc.wsum(onf.flat_parameters.cpu().numpy())
        for name in case_names():
            words, rows = r.run(name)
            torch.cuda.synchronize()
            res[name + "_sha"], res[name + "_head"], res[name + "_tail"] = digest(words, rows)
    finally:
        _lib.check(lib.nfopp_set_matrix_path(before))
    return res
