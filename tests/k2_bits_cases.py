"""The launches of the trajectory-update kernel (csrc/traj_update.hip, K2) whose output bits are pinned by
tests/golden/k2_bits.npz: shared by the recorder (tools/record_k2_bits.py) and tests/test_gpu_k2_bits.py.

Every case calls nfopp_traj_update directly on B = 3 trajectories with seeded random state, random draws `t` and random ONF
records -- no ONF kernel runs, and every gradient row is non-zero, so every staged band coefficient reaches an output.
A case is (N, velocity-Hessian weight, D); its branch in the kernel follows from engine.band_of / engine.interior_range:

  no interior, NB <= 64      N = 2, 9, 64          every waypoint is a boundary column; one wave of columns at most
  no interior, NB > 64       N = 100, 121          a second trip over the columns (121: the largest N without an interior)
  interior, NB = 58          N = 122, 256, 257, 512  (122: the smallest with one; 257: second waypoint trip per thread)
  interior, not staged       N = 256, w = 2        NB = 116, 38 KB > the 32 KB budget: boundary taps from global memory
  no interior, not staged    N = 256, w = 10

run_case returns the five state arrays and `terms` after ONE call; `want_terms=False` passes a null terms pointer (the planner's
own step), `retired` passes an `active` mask with that trajectory switched off."""
import functools

import numpy as np
import torch

from nfopp import _lib
from nfopp.engine import TrajectoryHyper, band_of, interior_range, inverse_hessian

F32 = np.float32
B = 3
ADAM_STEP = 7
BND_BUDGET = 32 * 1024     # K2_BND_BUDGET of csrc/traj_update.hip
CASES = ((2, 0.5, 3), (2, 0.5, 2), (9, 0.5, 3), (64, 0.5, 3), (100, 0.5, 3), (100, 0.5, 2), (121, 0.5, 3), (122, 0.5, 3),
         (256, 0.5, 3), (256, 0.5, 2), (257, 0.5, 3), (512, 0.5, 3), (256, 2, 3), (256, 10, 3))
STATE = ("traj", "adam_m", "adam_v", "lam", "cm")
# the benchmark's hyper block (bench.py): every term of the loss is switched on
HYPER = TrajectoryHyper(100, 5, 100, 0.1, 1e-3, 1, 10, 100, 5e-2, (0.9, 0.9), 1e-8, (0, 100, 0, 100))
TERMS_FILL = F32(-7.25)    # what the terms buffer holds before the call: rows the kernel does not write keep it


def tag(case):
    return "N%d_w%g_D%d" % case


def arrays_of(case):
    """names of the arrays a case records (the 2-D planner has no multipliers)"""
    return tuple(k for k in STATE if case[2] == 3 or k not in ("lam", "cm")) + ("terms",)


@functools.lru_cache(maxsize=None)
def band(n, weight):
    """(band [2W+1, N], W, (interior_lo, interior_hi)) as the engine forms them"""
    bnd, w = band_of(inverse_hessian(n, weight))
    return bnd, w, interior_range(bnd)


def branch(case):
    """(has interior, boundary columns, staged in LDS) of a case, as nfopp_traj_update decides it"""
    n, weight, _ = case
    _, w, (lo, hi) = band(n, weight)
    nb = lo + (n - hi)
    return hi > lo, nb, nb * (2 * w + 1) * 4 <= BND_BUDGET


def inputs(case):
    n, weight, d = case
    rng = np.random.default_rng([n, d, int(round(100 * weight))])
    s = {}
    s["traj"] = rng.uniform(-5, 105, (B, n, d)).astype(F32)       # the bounds are 0 .. 100: some waypoints lie outside
    s["start"] = rng.uniform(0, 100, (B, d)).astype(F32)
    s["goal"] = rng.uniform(0, 100, (B, d)).astype(F32)
    if d == 3:
        for k in ("traj", "start", "goal"):
            s[k][..., 2] = rng.uniform(-3.3, 3.3, s[k].shape[:-1]).astype(F32)
        s["lam"] = rng.normal(0, 2, (B, n + 1)).astype(F32)
        s["cm"] = rng.uniform(0, 3, (B, n)).astype(F32)
    s["adam_m"] = rng.normal(0, 5, (B, n, d)).astype(F32)
    s["adam_v"] = rng.uniform(0.1, 40, (B, n, d)).astype(F32)
    s["t"] = rng.uniform(0, 1, (B, n - 1)).astype(F32)
    onf = rng.normal(0, 1, (B, n - 1, 4)).astype(F32)
    onf[..., 0] *= F32(1.5)                                       # logits: beta = 10 puts some beyond the softplus threshold
    s["onf"] = onf
    return s


def run_case(case, lib=None, want_terms=True, retired=None):
    """one nfopp_traj_update call on the case's inputs -> {name: array} of the state after it and the terms buffer"""
    lib = lib or _lib.load()
    n, weight, d = case
    bnd, w, (lo, hi) = band(n, weight)
    s = inputs(case)
    dev = {k: torch.tensor(v, device="cuda") for k, v in s.items()}
    dev["band"] = torch.tensor(bnd, device="cuda")
    dev["terms"] = torch.full((B, _lib.NUM_TERMS), float(TERMS_FILL), device="cuda")
    active = None
    if retired is not None:
        mask = np.ones(B, np.uint8)
        mask[retired] = 0
        active = torch.tensor(mask, device="cuda")
    P = _lib.ptr
    rc = lib.nfopp_traj_update(HYPER.to_c(ADAM_STEP), B, n, d, P(dev["traj"]), P(dev["start"]), P(dev["goal"]), P(dev.get("lam")),
                               P(dev.get("cm")), P(dev["adam_m"]), P(dev["adam_v"]), P(dev["t"]), P(dev["onf"]), P(dev["band"]),
                               w, lo, hi, P(dev["terms"]) if want_terms else None, P(active, torch.uint8), _lib.stream_ptr())
    assert rc == 0, lib.nfopp_last_error()
    torch.cuda.synchronize()
    return {k: dev[k].cpu().numpy() for k in arrays_of(case)}


def run_cases(lib=None):
    """every case with terms and without a mask: the arrays of the golden file, {"<tag>_<array>": array}"""
    return {"%s_%s" % (tag(c), k): v for c in CASES for k, v in run_case(c, lib).items()}
