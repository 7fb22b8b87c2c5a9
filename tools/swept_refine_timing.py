#!/usr/bin/env python3
"""Device-event timings of the box robot's swept refinement on one GPU (the figures of profiles/swept_refine.txt and
DESIGN.md 14): `BatchPlanner.evaluate(swept=True)` beside `evaluate(swept=True, refine=8)` on the workload of
tools/swept_timing.py (4096 paths x 256 waypoints, the cloud of the 384 x 384 map, the box of tools/obstacle_map_timing.py)
at sub = 4, the same pair at sub = 1 -- refine at sub = 1 against the plain check at sub = 4 is the trade the refinement
exists for -- and the shares of segments decided at the root, below it, and left undecided.  The forms are timed
alternately in one run (medians of 10 event-timed calls after 3 warm-up calls, three rounds; smallest and largest median).
Every step runs in a child process of its own under a time limit; a step that fails or runs out of time ends the run.

Usage:  python tools/swept_refine_timing.py [--batch 4096] [--waypoints 256] [--out profiles/swept_refine.txt]
        python tools/swept_refine_timing.py --step evaluate|shares|kernels --sub S     (one step, what the parent starts)
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEPTH = 8
STEP_SECONDS = 240


def workload(B, N):
    """The planner, checker and paths of tools/swept_timing.py for the box robot (the same draws)."""
    import nfopp
    from obstacle_map_timing import BOX, blob_map
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    blob_map(rng, 64, 30, 2, 7)
    img = blob_map(rng, 384, 420, 3, 8)
    cloud = nfopp.DeviceGridMap(torch.tensor(img, device="cuda"), 0.1, (0.0, 0.0, 0.3)).as_point_cloud()
    lo, hi = cloud.min(0).values.cpu().numpy(), cloud.max(0).values.cpu().numpy()
    starts, goals = rng.uniform(lo, hi, (B, 2)), rng.uniform(lo, hi, (B, 2))
    u = np.linspace(0, 1, N + 2)[None, :, None]
    wander = np.cumsum(rng.normal(0, 0.02, (B, N + 2, 2)), 1)
    wander -= u * wander[:, -1:]
    xy = starts[:, None] + u * (goals - starts)[:, None] + wander
    d = np.diff(xy, axis=1)
    th = np.arctan2(d[..., 1], d[..., 0])
    paths = np.concatenate([xy, np.concatenate([th, th[:, -1:]], 1)[..., None]], 2).astype(np.float32)
    bounds = (float(lo[0]) - 1, float(hi[0]) + 1, float(lo[1]) - 1, float(hi[1]) + 1)
    torch.random.manual_seed(0)
    onf = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=True).to("cuda")
    planner = nfopp.BatchPlanner(onf, B, N, nfopp.TrajectoryHyper(bounds=bounds))
    planner.init(np.ascontiguousarray(paths[:, 0]), np.ascontiguousarray(paths[:, -1]), bounds,
                 trajectories=np.ascontiguousarray(paths[:, 1:-1]))
    return planner, nfopp.DeviceRectangleChecker(cloud, BOX, bounds), cloud.shape[0]


def step_evaluate(args):
    from obstacle_map_timing import timed
    planner, checker, _ = workload(args.batch, args.waypoints)
    sub = args.sub
    forms = (("evaluate()", dict()), ("evaluate(swept=True)", dict(swept=True)),
             ("evaluate(swept=True, refine=%d)" % DEPTH, dict(swept=True, refine=DEPTH)))
    medians = {name: [] for name, _ in forms}
    for _ in range(3):                                       # alternating, so that all see the same machine
        for name, kw in forms:
            medians[name].append(timed(lambda: planner.evaluate(checker, sub=sub, **kw)))
    for name, kw in forms:
        best = min(medians[name])
        collides = float(planner.evaluate(checker, sub=sub, **kw)[0].float().mean())
        print("  sub = %d  %-34s %8.4f / %8.4f / %8.4f   medians of the 3 rounds %.4f .. %.4f   paths in collision %.4f"
              % ((sub, name) + best + (min(medians[name])[0], max(medians[name])[0], collides)))


def step_shares(args):
    planner, checker, _ = workload(args.batch, args.waypoints)
    sub = args.sub
    planner.evaluate(checker, sub=sub)
    poses = planner._poses
    seg_a, seg_b = poses[:, :-1].contiguous().view(-1, 3), poses[:, 1:].contiguous().view(-1, 3)
    spacing = float((seg_b[:, :2] - seg_a[:, :2]).norm(dim=1).median())
    status, s, depth = checker.swept_refine(seg_a, seg_b, max_depth=DEPTH)
    n = float(status.numel())
    root = depth == 0
    print("  sub = %d  %d segments, median distance between dense poses %.3f m, max_depth %d, node_budget 1024"
          % (sub, int(n), spacing, DEPTH))
    print("           decided at depth 0: free %.5f, hit at an end pose %.5f, hit at the root's midpoint %.5f"
          % (float((root & (status == 0)).sum()) / n, float((root & (status == 1) & (s != 0.5)).sum()) / n,
             float((root & (status == 1) & (s == 0.5)).sum()) / n))
    print("           decided at depth 1 .. %d: free %.5f, hit %.5f;  left undecided %.5f (of them non-finite or at depth 0: %.5f)"
          % (DEPTH, float((~root & (status == 0)).sum()) / n, float((~root & (status == 1)).sum()) / n,
             float((status == 2).sum()) / n, float((root & (status == 2)).sum()) / n))
    one_shot = planner.certify(checker, sub=sub)[0]
    refined = planner.certify(checker, sub=sub, refine=DEPTH)[0]
    print("           paths free / colliding / undecided: certify() %s, certify(refine=%d) %s"
          % (" ".join("%.4f" % float((one_shot == k).float().mean()) for k in range(3)), DEPTH,
             " ".join("%.4f" % float((refined == k).float().mean()) for k in range(3))))


def step_kernels(args):
    from obstacle_map_timing import timed
    planner, checker, _ = workload(args.batch, args.waypoints)
    sub = args.sub
    planner.evaluate(checker, sub=sub)
    poses = planner._poses
    seg_a, seg_b = poses[:, :-1].contiguous().view(-1, 3), poses[:, 1:].contiguous().view(-1, 3)
    n = seg_a.shape[0]
    value = torch.empty(n, device="cuda")
    status, depth = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    t_one = timed(lambda: checker.swept(seg_a, seg_b, out=value, index_out=False))
    t_root = timed(lambda: checker.swept_refine(seg_a, seg_b, 0, 1024, status, value, depth))
    t_full = timed(lambda: checker.swept_refine(seg_a, seg_b, DEPTH, 1024, status, value, depth))
    print("  sub = %d  segments, one-shot certificate (indexed)       %8.4f / %8.4f / %8.4f" % ((sub,) + t_one))
    print("           swept_refine, max_depth 0 (pass 1 alone)        %8.4f / %8.4f / %8.4f" % t_root)
    print("           swept_refine, max_depth %d (pass 1 + the walk)    %8.4f / %8.4f / %8.4f" % ((DEPTH,) + t_full))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--waypoints", type=int, default=256)
    ap.add_argument("--sub", type=int, default=4)
    ap.add_argument("--step", choices=("evaluate", "shares", "kernels"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        {"evaluate": step_evaluate, "shares": step_shares, "kernels": step_kernels}[args.step](args)
        return 0
    lines = ["4096 x 256 workload of tools/swept_timing.py, box robot: %d paths x %d waypoints against the cloud of the 384 x 384 "
             "map; ms, median / min / max of 10 event-timed calls after 3 warm-up calls" % (args.batch, args.waypoints)]
    for sub in (4, 1):
        for step in ("evaluate", "shares", "kernels"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--sub", str(sub), "--batch", str(args.batch),
                   "--waypoints", str(args.waypoints)]
            try:
                done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=STEP_SECONDS)
            except subprocess.TimeoutExpired:
                print("step %s at sub = %d ran out of its %d s: stopping" % (step, sub, STEP_SECONDS))
                return 1
            text = done.stdout.decode(errors="replace")
            print(text, end="", flush=True)
            if done.returncode != 0:
                print("step %s at sub = %d failed (%d): stopping" % (step, sub, done.returncode))
                return 1
            lines.append(text.rstrip("\n"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
