#!/usr/bin/env python3
"""Device-event timings of the start-delay scheduling of a fleet (csrc/fleet_schedule.hip) on one GPU: the figures of
profiles/fleet_schedule.txt and DESIGN.md 18.  Self-mode fleets of 256 and 1024 robots x 256 instants at max_delay 15 and 63:
nfopp_fleet_shift_masks and nfopp_fleet_assign_delays separately, and beside each one nfopp_track_conflicts self-mode call on
the same tracks in the same run -- the shift masks do 2 D - 1 = 2 max_delay + 1 times the closest-approach work of that call
when nothing is pruned and no walk ends early, so their ratio is to be read against 2 D - 1.  Outputs preallocated, medians of
20 event-timed calls, milliseconds.  Every case runs in a child process of its own under a time limit; the first one that
fails ends the run.

Usage:  python tools/fleet_schedule_timing.py [--out profiles/fleet_schedule.txt]      (all cases)
        python tools/fleet_schedule_timing.py --case 1024x63
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
CASES = {"256x15": (256, 15), "256x63": (256, 63), "1024x15": (1024, 15), "1024x63": (1024, 63)}
LIMIT_S = 240


def run_case(name):
    import torch
    from nfopp import _lib as L
    from obstacle_map_timing import timed
    from track_conflict_timing import random_tracks
    torch.cuda.set_device(0)
    lib = L.load()
    b, md = CASES[name]
    rng = np.random.default_rng(97531)
    tracks = torch.tensor(random_tracks(rng, b, K, 2.0 * np.sqrt(b)), device="cuda")
    radius = torch.tensor(rng.uniform(0.2, 0.4, b).astype(np.float32), device="cuda")
    margin = 0.2
    i64, i32 = dict(dtype=torch.int64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    pair, base, bad = torch.empty(b, b, 2, **i64), torch.empty(b, **i64), torch.empty(b, **i32)
    delay, status, forbidden = torch.empty(b, **i32), torch.empty(b, **i32), torch.empty(b, **i64)
    summary = torch.empty(b, 7, dtype=torch.float64, device="cuda")
    nbytes = lib.nfopp_track_conflicts_workspace_bytes(b, 0, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def masks():
        L.check(lib.nfopp_fleet_shift_masks(L.ptr(tracks), b, 2, K, L.ptr(radius), margin, md, None, 0, 2, None, L.ptr(pair, torch.int64),
                                            L.ptr(base, torch.int64), L.ptr(bad, torch.int32), None, 0, L.stream_ptr()))

    def assign():
        L.check(lib.nfopp_fleet_assign_delays(L.ptr(pair, torch.int64), L.ptr(base, torch.int64), L.ptr(bad, torch.int32), None, b, md,
                                              L.ptr(delay, torch.int32), L.ptr(status, torch.int32), L.ptr(forbidden, torch.int64),
                                              L.stream_ptr()))

    def conflicts():
        L.check(lib.nfopp_track_conflicts(L.ptr(tracks), b, 2, None, 0, 2, K, 0.0, 0.1, L.ptr(radius), None, margin,
                                          L.ptr(summary, torch.float64), None, None, None, L.ptr(ws, torch.uint8), nbytes, L.stream_ptr()))

    t_masks = timed(masks, warmup=3, reps=20)
    t_assign = timed(assign, warmup=3, reps=20)
    t_conf = timed(conflicts, warmup=3, reps=20)
    for label, t in (("shift_masks", t_masks), ("assign_delays", t_assign), ("track_conflicts", t_conf)):
        print("  %-9s %-16s %9.4f / %9.4f / %9.4f ms" % (name, label, t[0], t[1], t[2]), flush=True)
    st = status.cpu().numpy()
    bits = int(sum(bin(int(x) & (2 ** 64 - 1)).count("1") for x in pair.cpu().numpy().ravel()))
    print("    shift_masks / track_conflicts = %.1f against 2 D - 1 = %d; %.1f %% of the %d pair-shift bits set; %d scheduled "
          "(%d delayed, largest delay %d), %d unresolved; %d of %d in conflict undelayed; device %s" %
          (t_masks[0] / t_conf[0], 2 * md + 1, 100.0 * bits / (b * (b - 1) * (2 * md + 1)), b * (b - 1) * (2 * md + 1),
           int((st == 0).sum()), int((delay > 0).sum()), int(delay.max()), int((st == 2).sum()), int((summary[:, 5] > 0).sum()), b,
           torch.cuda.get_device_name(0)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_schedule.txt"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        return 0
    # the parent never opens the GPU: every case is a fresh process
    lines = ["%d instants per track, self mode (no obstacles); median / min / max of 20 event-timed calls" % K]
    print(lines[0], flush=True)
    rc = 0
    for name in ("256x15", "256x63", "1024x15", "1024x63"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], timeout=LIMIT_S, stdout=subprocess.PIPE,
                               universal_newlines=True)
        except subprocess.TimeoutExpired:
            lines.append("case %s ran past %d s: stopping" % (name, LIMIT_S))
            rc = 124
            break
        sys.stdout.write(r.stdout)
        lines.extend(r.stdout.rstrip("\n").split("\n"))
        if r.returncode != 0:
            lines.append("case %s ended with status %d: stopping" % (name, r.returncode))
            rc = r.returncode
            break
    if rc:
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
