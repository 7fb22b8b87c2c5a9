#!/usr/bin/env python3
"""Device-event timings of the box conflict check between timed SE(2) tracks (csrc/box_conflict.hip) on one GPU: the figures of
profiles/box_conflict.txt and DESIGN.md 23.  Self mode at 256 and 1024 robots x 256 instants, `refine` 0 and 4, the car of
profiles/swept.txt on the random walks of tools/track_conflict_timing.py with the heading along the motion; beside each, in
the same process and on the same tracks, one nfopp_track_conflicts call at the circumscribed radius.  Outputs preallocated,
medians of 20 event-timed calls.  The shares say which step of the rule settled a pair: the discs (the disc check finds the
pair free at the reach), the certificate at the instants (decided at refine 0), refinement (decided at refine 4 only).  Every
case runs in a child process of its own under a time limit; the first one that fails ends the run.

Usage:  python tools/box_conflict_timing.py            (all cases)
        python tools/box_conflict_timing.py --case self1024
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

K = 256
CASES = {"self256": 256, "self1024": 1024}
REFINES = (0, 4)
BOX = (-0.34, 0.4, -0.27, 0.27)
DT, MARGIN = 0.1, 0.1
LIMIT_S = 240


def random_car_tracks(rng, n, k, extent):
    """[n, k, 3] fp32: the heading random walks of tools/track_conflict_timing.py (0.1 .. 0.4 m steps, a tenth of them a stop)
    with theta the heading of the walk, wrapped to (-pi, pi]."""
    turn = rng.uniform(-0.4, 0.4, (n, k))
    heading = rng.uniform(-np.pi, np.pi, (n, 1)) + np.cumsum(turn, 1)
    step = rng.uniform(0.1, 0.4, (n, k)) * (rng.uniform(size=(n, k)) > 0.1)
    xy = rng.uniform(0.0, extent, (n, 1, 2)) + np.cumsum(step[..., None] * np.stack([np.cos(heading), np.sin(heading)], -1), 1)
    theta = np.arctan2(np.sin(heading), np.cos(heading))
    return np.concatenate([xy, theta[..., None]], -1).astype(np.float32)


def run_case(name):
    import torch
    from nfopp import _lib as L
    from obstacle_map_timing import timed
    torch.cuda.set_device(0)
    lib = L.load()
    n = CASES[name]
    rng = np.random.default_rng(97531)
    a = torch.tensor(random_car_tracks(rng, n, K, 2.0 * np.sqrt(n)), device="cuda")
    box = torch.tensor(np.tile(np.asarray(BOX, np.float32), (n, 1)), device="cuda")
    b32 = np.abs(np.asarray(BOX, np.float32))
    corner = np.float32(np.sqrt(np.float64(max(b32[0], b32[1])) ** 2 + np.float64(max(b32[2], b32[3])) ** 2))
    reach = torch.full((n,), float(corner * np.float32(1.000001)), dtype=torch.float32, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    units = torch.empty(n, K, 2, **f64)
    summary, first, und = torch.empty(n, 7, **f64), torch.empty(n, n, **f64), torch.empty(n, n, **f64)
    status = torch.empty(n, n, dtype=torch.int32, device="cuda")
    nbytes = lib.nfopp_box_track_conflicts_workspace_bytes(n, 0, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    pairs = n * (n - 1) // 2

    def headings():
        L.check(lib.nfopp_track_headings(L.ptr(a), n, 3, K, L.ptr(units, torch.float64), L.stream_ptr()))

    def boxes(refine, with_pairs=False):
        L.check(lib.nfopp_box_track_conflicts(
            L.ptr(a), L.ptr(units, torch.float64), n, 3, None, None, 0, 3, K, 0.0, DT, L.ptr(box), None, None, None, MARGIN, refine,
            L.ptr(summary, torch.float64), None, L.ptr(status, torch.int32) if with_pairs else None,
            L.ptr(first, torch.float64) if with_pairs else None, L.ptr(und, torch.float64) if with_pairs else None,
            L.ptr(ws, torch.uint8), nbytes, L.stream_ptr()))

    d_summary, d_gap, d_first = torch.empty(n, 7, **f64), torch.empty(n, n, **f64), torch.empty(n, n, **f64)
    d_bytes = lib.nfopp_track_conflicts_workspace_bytes(n, 0, K)
    d_ws = torch.empty(d_bytes, dtype=torch.uint8, device="cuda")

    def discs(with_pairs=False):
        L.check(lib.nfopp_track_conflicts(L.ptr(a), n, 3, None, 0, 2, K, 0.0, DT, L.ptr(reach), None, MARGIN,
                                          L.ptr(d_summary, torch.float64), None, L.ptr(d_gap, torch.float64) if with_pairs else None,
                                          L.ptr(d_first, torch.float64) if with_pairs else None, L.ptr(d_ws, torch.uint8), d_bytes,
                                          L.stream_ptr()))

    h_med, h_lo, h_hi = timed(headings, warmup=3, reps=20)
    d_med, d_lo, d_hi = timed(discs, warmup=3, reps=20)
    print("  %-9s headings pass            %9.4f / %9.4f / %9.4f ms" % (name, h_med, h_lo, h_hi), flush=True)
    print("  %-9s discs at the reach       %9.4f / %9.4f / %9.4f ms" % (name, d_med, d_lo, d_hi), flush=True)
    decided = {}
    for refine in REFINES:
        med, lo, hi = timed(lambda: boxes(refine), warmup=3, reps=20)
        print("  %-9s boxes, refine %d          %9.4f / %9.4f / %9.4f ms   %5.2f x the discs   %8.3e pair-intervals/s" %
              (name, refine, med, lo, hi, med / d_med, pairs * (K - 1) / (med * 1e-3)), flush=True)
        boxes(refine, with_pairs=True)
        decided[refine] = status.cpu().numpy()[np.triu_indices(n, 1)]
    discs(with_pairs=True)
    by_discs = ~(d_first.cpu().numpy()[np.triu_indices(n, 1)] < np.inf)
    s0, s4 = decided[0], decided[4]
    by_cert = ~by_discs & (s0 != 2)
    by_refinement = (s0 == 2) & (s4 != 2)
    left = s4 == 2
    print("    %d pairs: %.2f %% settled by the discs, %.2f %% by the certificate at the instants, %.2f %% by refinement, %.2f %% "
          "left undecided at refine 4" % (pairs, 100.0 * by_discs.mean(), 100.0 * by_cert.mean(), 100.0 * by_refinement.mean(),
                                           100.0 * left.mean()), flush=True)
    print("    in conflict: %.2f %% of the pairs as boxes (refine 4), %.2f %% as circumscribed discs; free at refine 4: %.2f %%; "
          "workspace %.1f MiB; device %s" % (100.0 * (s4 == 1).mean(), 100.0 * (~by_discs).mean(), 100.0 * (s4 == 0).mean(),
                                             nbytes / 2.0 ** 20, torch.cuda.get_device_name(0)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        return 0
    # the parent never opens the GPU: every case is a fresh process
    print("%d instants per track, self mode; median / min / max of 20 event-timed calls" % K, flush=True)
    for name in ("self256", "self1024"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print("case %s ran past %d s: stopping" % (name, LIMIT_S))
            return 124
        if rc != 0:
            print("case %s ended with status %d: stopping" % (name, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
