#!/usr/bin/env python3
"""Device-event timings of the conflict check between timed tracks (csrc/track_conflict.hip) on one GPU: the figures of
profiles/track_conflicts.txt and DESIGN.md 17.  Self mode at 256, 1024 and 4096 robots x 256 instants, 4096 paths against 64
obstacle tracks x 256 instants, each with and without the pair matrices, and -- for the triangle decision -- the full square
of the 4096-robot fleet (set B = set A).  Outputs preallocated, medians of 20 event-timed calls, milliseconds and
pair-intervals per second.  Every case runs in a child process of its own under a time limit; the first one that fails ends
the run.

Usage:  python tools/track_conflict_timing.py            (all cases)
        python tools/track_conflict_timing.py --case self4096
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
CASES = {"self256": (256, None), "self1024": (1024, None), "self4096": (4096, None), "square4096": (4096, "same"),
         "obstacles4096x64": (4096, 64)}
LIMIT_S = 240


def random_tracks(rng, n, k, extent):
    """[n, k, 2] fp32: heading random walks of 0.1 .. 0.4 m steps on a floor of `extent` metres, a tenth of the steps a stop."""
    turn = rng.uniform(-0.4, 0.4, (n, k))
    heading = rng.uniform(-np.pi, np.pi, (n, 1)) + np.cumsum(turn, 1)
    step = rng.uniform(0.1, 0.4, (n, k)) * (rng.uniform(size=(n, k)) > 0.1)
    xy = rng.uniform(0.0, extent, (n, 1, 2)) + np.cumsum(step[..., None] * np.stack([np.cos(heading), np.sin(heading)], -1), 1)
    return xy.astype(np.float32)


def run_case(name):
    import torch
    from nfopp import _lib as L
    from obstacle_map_timing import timed
    torch.cuda.set_device(0)
    lib = L.load()
    ba, other = CASES[name]
    rng = np.random.default_rng(97531)
    extent = 2.0 * np.sqrt(ba)
    a = torch.tensor(random_tracks(rng, ba, K, extent), device="cuda")
    ra = torch.tensor(rng.uniform(0.2, 0.4, ba).astype(np.float32), device="cuda")
    if other is None:
        b, rb, bb, pairs = None, None, 0, ba * (ba - 1) // 2
    elif other == "same":
        b, rb, bb, pairs = a, ra, ba, ba * ba
    else:
        bb = other
        b = torch.tensor(random_tracks(rng, bb, K, extent), device="cuda")
        rb = torch.tensor(rng.uniform(0.2, 0.4, bb).astype(np.float32), device="cuda")
        pairs = ba * bb
    cols = ba if b is None else bb
    f64 = dict(dtype=torch.float64, device="cuda")
    summary, summary_b = torch.empty(ba, 7, **f64), (None if b is None else torch.empty(bb, 7, **f64))
    gap, first = torch.empty(ba, cols, **f64), torch.empty(ba, cols, **f64)
    nbytes = lib.nfopp_track_conflicts_workspace_bytes(ba, bb, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for with_pairs in (False, True):
        def call():
            L.check(lib.nfopp_track_conflicts(L.ptr(a), ba, 2, L.ptr(b), bb, 2, K, 0.0, 0.1, L.ptr(ra), L.ptr(rb), 0.2,
                                              L.ptr(summary, torch.float64), L.ptr(summary_b, torch.float64),
                                              L.ptr(gap, torch.float64) if with_pairs else None,
                                              L.ptr(first, torch.float64) if with_pairs else None, L.ptr(ws, torch.uint8), nbytes,
                                              L.stream_ptr()))
        med, lo, hi = timed(call, warmup=3, reps=20)
        rate = pairs * (K - 1) / (med * 1e-3)
        print("  %-18s %-12s %9.4f / %9.4f / %9.4f ms   %8.3e pair-intervals/s" %
              (name, "with pairs" if with_pairs else "summary only", med, lo, hi, rate), flush=True)
    s = summary.cpu().numpy()
    print("    %d of %d tracks in conflict, %.1f partners each on average; workspace %.1f MiB; device %s" %
          (int((s[:, 5] > 0).sum()), ba, s[:, 5].mean(), nbytes / 2.0 ** 20, torch.cuda.get_device_name(0)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        return 0
    # the parent never opens the GPU: every case is a fresh process
    print("%d instants per track; median / min / max of 20 event-timed calls" % K, flush=True)
    print("(self: pairs = B (B - 1) / 2, the upper triangle of tiles; square: set B = set A, all B^2 pairs; rate = pairs x %d intervals / median)" % (K - 1), flush=True)
    for name in ("self256", "self1024", "self4096", "square4096", "obstacles4096x64"):
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
