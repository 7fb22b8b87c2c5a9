#!/usr/bin/env python3
"""Device-event timings of the swept check on one GPU (the figures of profiles/swept.txt and DESIGN.md 14):
`BatchPlanner.evaluate(swept=True)` beside `evaluate()` at 4096 paths x 256 waypoints, sub = 4, against the cloud of the
384 x 384 occupancy grid of tools/obstacle_map_timing.py, both robot shapes, and the indexed segment entry
beside the all-pairs one on the same 4.2 M segments.  The two evaluate forms are timed alternately in one run.

Usage:  python tools/swept_timing.py [--batch 4096] [--waypoints 256] [--sub 4]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import nfopp  # noqa: E402
from nfopp import _lib  # noqa: E402
from obstacle_map_timing import BOX, blob_map, timed  # noqa: E402

RADIUS = 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--waypoints", type=int, default=256)
    ap.add_argument("--sub", type=int, default=4)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    blob_map(rng, 64, 30, 2, 7)                       # the draws tools/obstacle_map_timing.py makes before the large map
    img = blob_map(rng, 384, 420, 3, 8)
    cloud = nfopp.DeviceGridMap(torch.tensor(img, device="cuda"), 0.1, (0.0, 0.0, 0.3)).as_point_cloud()
    lo, hi = cloud.min(0).values.cpu().numpy(), cloud.max(0).values.cpu().numpy()
    B, N, sub = args.batch, args.waypoints, args.sub
    m = (N + 1) * sub + 1
    # paths as a planner holds them: start and goal uniform over the map, waypoints on the straight line plus a smooth
    # wander of a few cells, headings along the travel direction; consecutive dense poses end up a few centimetres apart
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
    print("device: %s, %d paths x %d waypoints, sub = %d: %d poses and %d segments per call, cloud of the 384 x 384 map: %d "
          "points (median / min / max of 10 event-timed calls after 3 warm-up calls, ms)"
          % (torch.cuda.get_device_name(0), B, N, sub, B * m, B * (m - 1), cloud.shape[0]))
    lib = _lib.load()
    for shape, D in (("disc r = %.1f" % RADIUS, 2), ("box %s" % (BOX,), 3)):
        onf = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=D == 3).to("cuda")
        planner = nfopp.BatchPlanner(onf, B, N, nfopp.TrajectoryHyper(bounds=bounds))
        planner.init(np.ascontiguousarray(paths[:, 0, :D]), np.ascontiguousarray(paths[:, -1, :D]), bounds,
                     trajectories=np.ascontiguousarray(paths[:, 1:-1, :D]))
        checker = nfopp.DeviceCircleChecker(cloud, RADIUS, bounds) if D == 2 else nfopp.DeviceRectangleChecker(cloud, BOX, bounds)
        start, nx, ny, x0, y0, size = checker.cells
        plain, swept = [], []
        for _ in range(3):                                   # alternating, so that both see the same machine
            plain.append(timed(lambda: planner.evaluate(checker, sub=sub)))
            swept.append(timed(lambda: planner.evaluate(checker, sub=sub, swept=True)))
        t_plain, t_swept = min(plain), min(swept)            # the run with the smallest median of each
        collides_plain = float(planner.evaluate(checker, sub=sub)[0].float().mean())
        collides_swept = float(planner.evaluate(checker, sub=sub, swept=True)[0].float().mean())
        status, _ = planner.certify(checker, sub=sub)
        poses = planner._poses
        seg_a, seg_b = poses[:, :-1].contiguous().view(-1, D), poses[:, 1:].contiguous().view(-1, D)
        spacing = float((seg_b[:, :2] - seg_a[:, :2]).norm(dim=1).median())
        n = seg_a.shape[0]
        value, index = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        horizon = RADIUS if D == 2 else checker.swept_slack     # the defaults of checker.swept
        t_cells = timed(lambda: checker.swept(seg_a, seg_b, out=value, index_out=index))
        v_cells, i_cells = value.clone(), index.clone()
        box = None if D == 2 else (ctypes.c_float * 4)(*checker.box)
        t_brute = timed(lambda: _lib.check(lib.nfopp_swept_segments(
            _lib.ptr(seg_a), _lib.ptr(seg_b), n, D, _lib.ptr(checker.obstacles), checker.obstacles.shape[0], box, horizon,
            _lib.ptr(value), _lib.ptr(index, torch.int32), _lib.stream_ptr())), warmup=1, reps=3)
        assert torch.equal(value, v_cells) and torch.equal(index, i_cells), "the two entries disagree"
        labels = torch.empty(B * m, device="cuda")
        t_label = timed(lambda: checker.labels(poses.view(B * m, D), out=labels))
        t_copy = timed(lambda: (planner._segments[0].copy_(poses[:, :-1]), planner._segments[1].copy_(poses[:, 1:])))
        t_reduce = timed(lambda: checker.swept_labels(poses, v_cells.view(B, m - 1), labels))
        print("%s, %d x %d cells of %.3f m, median distance between dense poses %.3f m" % (shape, nx, ny, size, spacing))
        print("  paths reported in collision: evaluate() %.3f, evaluate(swept=True) %.3f; certify status 0 / 1 / 2: %s"
              % (collides_plain, collides_swept, " ".join("%.3f" % float((status == k).float().mean()) for k in range(3))))
        print("  evaluate()                                 %8.4f / %8.4f / %8.4f" % t_plain)
        print("  evaluate(swept=True)                       %8.4f / %8.4f / %8.4f   %.2f x evaluate()" % (t_swept + (t_swept[0] / t_plain[0],)))
        print("  spread of the medians over 3 alternating runs: evaluate() %.4f .. %.4f, swept %.4f .. %.4f"
              % (min(plain)[0], max(plain)[0], min(swept)[0], max(swept)[0]))
        print("  of which: copies of the two pose views     %8.4f / %8.4f / %8.4f" % t_copy)
        print("            segments, indexed                %8.4f / %8.4f / %8.4f   %.2f x the indexed label kernel (%.4f)"
              % (t_cells + (t_cells[0] / t_label[0], t_label[0])))
        print("            nfopp_path_swept_labels          %8.4f / %8.4f / %8.4f" % t_reduce)
        print("  segments, all pairs (3 calls)              %8.4f / %8.4f / %8.4f   %.1f x the indexed entry" % (t_brute + (t_brute[0] / t_cells[0],)))


if __name__ == "__main__":
    main()
