#!/usr/bin/env python3
"""Device-event timings of the space-time grid search (csrc/spacetime_search.hip) on one GPU: the figures of
profiles/spacetime_search.txt and DESIGN.md 19.  Wall-free images of 100 x 100 and 384 x 384 cells of 0.1 m over 128 and 256
instants, with 32 movers and 8 robots to plan, and with 256 movers and 64 robots.  Reported separately: nfopp_spacetime_reserve
of all movers (and its rate in (cell, direction, interval, track) predicates per second), of one track, the whole
nfopp_spacetime_plan_fleet call with its 2 R + 1 launches, and the same call for one robot -- one search and the reservation of
its track, so that the search is that minus the one-track reserve.  Beside them one nfopp_fleet_shift_masks call on the movers'
tracks as a fleet of that size at max_delay 15: the price of the step this one follows.  A fleet call writes to its reservation,
so every timed fleet call starts with a device copy of the saved words, timed on its own as well.  Outputs preallocated, medians
of 20 event-timed calls, milliseconds.  Every case runs in a child process of its own under a time limit; the first one that
fails ends the run.

Usage:  python tools/spacetime_timing.py [--out profiles/spacetime_search.txt]      (all cases)
        python tools/spacetime_timing.py --case 384x256x256x64
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

RES, RADIUS, MARGIN, MAX_DELAY = 0.1, 0.035, 0.01, 15
CASES = {"%dx%dx%dx%d" % c: c for c in ((100, 128, 32, 8), (100, 128, 256, 64), (100, 256, 32, 8), (100, 256, 256, 64),
                                         (384, 128, 32, 8), (384, 128, 256, 64), (384, 256, 32, 8), (384, 256, 256, 64))}
LIMIT_S = 240


def run_case(name):
    import torch
    from nfopp import _lib as L
    from obstacle_map_timing import timed
    torch.cuda.set_device(0)
    lib = L.load()
    side, T, m, r = CASES[name]
    rng = np.random.default_rng(24680)
    lam = (np.arange(T) / (T - 1))[None, :, None]
    p0, p1 = rng.uniform(0, side * RES, (m, 1, 2)), rng.uniform(0, side * RES, (m, 1, 2))
    tracks = torch.tensor((p0 * (1 - lam) + p1 * lam).astype(np.float32), device="cuda")
    radius = torch.tensor(rng.uniform(0.03, 0.09, m).astype(np.float32), device="cuda")
    starts = rng.integers(0, side, (r, 2))
    goals = np.clip(starts + rng.integers(-(T // 2), T // 2 + 1, (r, 2)), 0, side - 1)
    i32 = dict(dtype=torch.int32, device="cuda")
    occ = torch.zeros(side, side, dtype=torch.uint8, device="cuda")
    start_cells, goal_cells = torch.tensor(starts, **i32), torch.tensor(goals, **i32)
    nres = lib.nfopp_spacetime_reservation_bytes(side, side, T)
    words = torch.empty(nres // 8, dtype=torch.int64, device="cuda")
    nws_r = lib.nfopp_spacetime_reserve_workspace_bytes(m)
    ws_r = torch.empty(nws_r, dtype=torch.uint8, device="cuda")
    nws_p = lib.nfopp_spacetime_plan_workspace_bytes(side, side, T, r)
    ws_p = torch.empty(nws_p, dtype=torch.uint8, device="cuda")
    cells, arrival, status = torch.empty(r, T, **i32), torch.empty(r, **i32), torch.empty(r, **i32)
    out = torch.empty(r, T, 2, dtype=torch.float32, device="cuda")
    geometry = (side, side, T, 0.0, 0.0, RES, RADIUS, MARGIN)

    def init():
        L.check(lib.nfopp_spacetime_reservation_init(L.ptr(occ, torch.uint8), side, side, T, L.ptr(words, torch.int64), nres, L.stream_ptr()))

    def reserve(count=m):
        L.check(lib.nfopp_spacetime_reserve(*geometry, L.ptr(tracks), count, 2, L.ptr(radius), None, L.ptr(words, torch.int64), nres,
                                            L.ptr(ws_r, torch.uint8), nws_r, L.stream_ptr()))

    def plan(count=r):
        words.copy_(saved)
        L.check(lib.nfopp_spacetime_plan_fleet(L.ptr(occ, torch.uint8), *geometry, L.ptr(start_cells, torch.int32),
                                               L.ptr(goal_cells, torch.int32), None, count, L.ptr(words, torch.int64), nres,
                                               L.ptr(cells, torch.int32), L.ptr(arrival, torch.int32), L.ptr(status, torch.int32), L.ptr(out),
                                               L.ptr(ws_p, torch.uint8), nws_p, L.stream_ptr()))

    i64 = dict(dtype=torch.int64, device="cuda")
    pair, base, bad = torch.empty(m, m, 2, **i64), torch.empty(m, **i64), torch.empty(m, **i32)

    def masks():
        L.check(lib.nfopp_fleet_shift_masks(L.ptr(tracks), m, 2, T, L.ptr(radius), MARGIN, MAX_DELAY, None, 0, 2, None, L.ptr(pair, torch.int64),
                                            L.ptr(base, torch.int64), L.ptr(bad, torch.int32), None, 0, L.stream_ptr()))

    t_init = timed(init, warmup=2, reps=20)
    t_reserve = timed(reserve, warmup=2, reps=20)
    t_one = timed(lambda: reserve(1), warmup=2, reps=20)
    init()
    reserve()
    saved = words.clone()
    t_copy = timed(lambda: words.copy_(saved), warmup=2, reps=20)
    t_plan = timed(plan, warmup=2, reps=20)
    t_plan1 = timed(lambda: plan(1), warmup=2, reps=20)
    plan()
    t_masks = timed(masks, warmup=2, reps=20)
    rows = (("reservation_init", t_init), ("reserve %d tracks" % m, t_reserve), ("reserve 1 track", t_one), ("copy of the words", t_copy),
            ("plan_fleet %d robots" % r, t_plan), ("plan_fleet 1 robot", t_plan1), ("fleet_shift_masks %d" % m, t_masks))
    for label, t in rows:
        print("  %-16s %-22s %9.4f / %9.4f / %9.4f ms" % (name, label, t[0], t[1], t[2]), flush=True)
    predicates = float(side) * side * 9 * (T - 1) * m
    st = status.cpu().numpy()
    print("    reserve: %.3g predicates, %.3g per second (%.4f ms a track); search of one robot about %.4f ms; plan_fleet %.4f ms a robot "
          "without the copy; %d of %d planned, latest arrival %d; reservation %.1f MiB; device %s" %
          (predicates, predicates / (t_reserve[0] * 1e-3), t_reserve[0] / m, t_plan1[0] - t_copy[0] - t_one[0], (t_plan[0] - t_copy[0]) / r,
           int((st == 0).sum()), r, int(arrival.max()), nres / 2.0 ** 20, torch.cuda.get_device_name(0)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spacetime_search.txt"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        return 0
    # the parent never opens the GPU: every case is a fresh process
    lines = ["side x instants x movers x robots; wall-free images of %.1f m cells; median / min / max of 20 event-timed calls" % RES]
    print(lines[0], flush=True)
    rc = 0
    for name in CASES:
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
