#!/usr/bin/env python3
"""Device-event timings of the nearest-obstacle query and the per-path statistics on one GPU (the figures of
profiles/clearance.txt and DESIGN.md 12): cfg5's 2.54 M poses per fit against the cloud of the 384 x 384 occupancy grid of
tools/obstacle_map_timing.py, both robot shapes, the all-pairs and the indexed entry, and the two work distributions of the
indexed one (one thread per pose; one wave per group of poses).  The yardstick is the indexed LABEL kernel of the
ground-truth checkers on the same poses: a nearest query looks at least as far, so it cannot be faster.  Also the rings
each pose's search takes, and nfopp_path_stats at 4096 paths x 256 waypoints, sub = 4.

Usage:  python tools/clearance_timing.py [--poses 2540000]
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
    ap.add_argument("--poses", type=int, default=2540000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    blob_map(rng, 64, 30, 2, 7)                       # the draws tools/obstacle_map_timing.py makes before the large map
    img = blob_map(rng, 384, 420, 3, 8)
    cloud = nfopp.DeviceGridMap(torch.tensor(img, device="cuda"), 0.1, (0.0, 0.0, 0.3)).as_point_cloud()
    lo, hi = cloud.min(0).values.cpu().numpy() - 0.5, cloud.max(0).values.cpu().numpy() + 0.5
    xy = rng.uniform(lo, hi, (args.poses, 2))
    poses = torch.tensor(np.concatenate([xy, rng.uniform(-np.pi, np.pi, (args.poses, 1))], 1).astype(np.float32), device="cuda")
    n = poses.shape[0]
    print("device: %s, poses per call: %d, cloud of the 384 x 384 map: %d points (median / min / max of 10 event-timed "
          "calls, ms)" % (torch.cuda.get_device_name(0), n, cloud.shape[0]))
    lib = _lib.load()
    dist, index = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    for shape, checker, box in (("disc r = %.1f" % RADIUS, nfopp.DeviceCircleChecker(cloud, RADIUS), None),
                                ("box %s" % (BOX,), nfopp.DeviceRectangleChecker(cloud, BOX), (ctypes.c_float * 4)(*BOX))):
        start, nx, ny, x0, y0, size = checker.cells
        pts = checker.obstacles

        def cells_args():
            return (_lib.ptr(poses), n, 3, _lib.ptr(pts), pts.shape[0], _lib.ptr(start, torch.int32), nx, ny, x0, y0, size, box,
                    _lib.ptr(dist), _lib.ptr(index, torch.int32), _lib.stream_ptr())
        labels = torch.empty(n, device="cuda")
        t_label = timed(lambda: checker.labels(poses, out=labels))
        t_thread = timed(lambda: _lib.check(lib.nfopp_nearest_obstacle_cells(*cells_args())))
        d_thread, i_thread = dist.clone(), index.clone()
        t_wave = timed(lambda: _lib.check(lib.nfopp_nearest_obstacle_cells_probe(0, *cells_args())))
        assert torch.equal(dist, d_thread) and torch.equal(index, i_thread), "the two work distributions disagree"
        t_brute = timed(lambda: _lib.check(lib.nfopp_nearest_obstacle(_lib.ptr(poses), n, 3, _lib.ptr(pts), pts.shape[0], box,
                                                                    _lib.ptr(dist), _lib.ptr(index, torch.int32),
                                                                    _lib.stream_ptr())), warmup=1, reps=3)
        assert torch.equal(dist, d_thread) and torch.equal(index, i_thread), "the two entries disagree"
        t_clear = timed(lambda: checker.clearance(poses, out=dist))
        _lib.check(lib.nfopp_nearest_obstacle_cells_probe(1, *cells_args()))
        rings = index.cpu().numpy()
        hit = float(labels.mean())
        print("%s, %d x %d cells of %.3f m, in collision %.3f" % (shape, nx, ny, size, hit))
        print("  indexed label kernel (yardstick)          %8.4f / %8.4f / %8.4f" % t_label)
        print("  nearest, indexed, one thread per pose     %8.4f / %8.4f / %8.4f   %.2f x the label kernel" % (t_thread + (t_thread[0] / t_label[0],)))
        print("  nearest, indexed, one wave per 4 poses    %8.4f / %8.4f / %8.4f   %.2f x" % (t_wave + (t_wave[0] / t_label[0],)))
        print("  nearest, all pairs (3 calls)              %8.4f / %8.4f / %8.4f   %.2f x" % (t_brute + (t_brute[0] / t_label[0],)))
        print("  checker.clearance (nearest + torch ops)   %8.4f / %8.4f / %8.4f" % t_clear)
        print("  rings per pose: mean %.2f, median %d, 99th percentile %d, max %d; share of poses by rings 2..6+: %s"
              % (rings.mean(), np.median(rings), np.percentile(rings, 99), rings.max(),
                 " ".join("%.3f" % (np.mean(rings == k) if k < 6 else np.mean(rings >= 6)) for k in range(2, 7))))

    B, N, sub = 4096, 256, 4
    m = (N + 1) * sub + 1
    traj = torch.tensor(np.cumsum(rng.normal(0, 0.1, (B, N + 2, 3)), 1).astype(np.float32), device="cuda")
    inner, first, last = traj[:, 1:-1].contiguous(), traj[:, 0].contiguous(), traj[:, -1].contiguous()
    pose_dist = torch.rand(B, m, device="cuda")
    stats = torch.empty(B, 8, dtype=torch.float64, device="cuda")
    t = timed(lambda: _lib.check(lib.nfopp_path_stats(_lib.ptr(inner), _lib.ptr(first), _lib.ptr(last), B, N, 3,
                                                      _lib.ptr(pose_dist), m, -0.5, _lib.ptr(stats, torch.float64), None,
                                                      _lib.stream_ptr())))
    print("nfopp_path_stats %d paths x %d waypoints, %d poses per path (sub = %d): %8.4f / %8.4f / %8.4f" % ((B, N, m, sub) + t))


if __name__ == "__main__":
    main()
