#!/usr/bin/env python3
"""Device-event timings of the time parametrisation (csrc/time_profile.hip) on one GPU: the figures of
profiles/time_profile.txt and DESIGN.md 16.  4096 paths x 256 waypoints (SE(2) and 2-D), random-walk headings with
stretches, bends, folds and gear changes: nfopp_path_time_profile, then nfopp_path_time_sample at 256 and 2048 instants per
path, into preallocated outputs.  Medians of event-timed calls.

Usage:  python tools/time_profile_timing.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import nfopp  # noqa: E402
from nfopp import _lib as L  # noqa: E402
from obstacle_map_timing import timed  # noqa: E402


def random_paths(rng, b, n, dim):
    """[b, n + 2, dim] fp32: heading random walks, 4 % folds, 4 % gear changes (dim 3), steps of 0.05 .. 0.45 m."""
    m = n + 2
    turn = rng.choice([0.0, 0.0, 0.15, -0.15, 0.6, -0.6], (b, m - 1)) + rng.uniform(-0.02, 0.02, (b, m - 1))
    turn = np.where(rng.uniform(size=(b, m - 1)) < 0.04, np.pi, turn)
    direction = rng.uniform(-np.pi, np.pi, (b, 1)) + np.cumsum(turn, 1)
    step = rng.uniform(0.05, 0.45, (b, m - 1))
    xy = np.concatenate([np.zeros((b, 1, 2)), np.cumsum(step[..., None] * np.stack([np.cos(direction), np.sin(direction)], -1), 1)], 1)
    if dim == 2:
        return xy.astype(np.float32)
    gear = np.cumprod(np.where(rng.uniform(size=(b, m - 1)) < 0.04, -1.0, 1.0), 1)
    heading = direction + np.where(gear < 0, np.pi, 0.0) + rng.uniform(-0.5, 0.5, (b, m - 1))
    heading = np.concatenate([heading, heading[:, -1:]], 1)
    return np.concatenate([xy, ((heading + np.pi) % (2 * np.pi) - np.pi)[..., None]], -1).astype(np.float32)


def main():
    torch.cuda.set_device(0)
    lib = L.load()
    rng = np.random.default_rng(2468)
    B, N = 4096, 256
    limits = nfopp.MotionLimits(2.0, 1.0, 1.5, a_lat=1.0, w_max=1.5)
    lim = limits.to_c()
    print("device: %s; %d paths x %d waypoints, median / min / max of event-timed calls, ms" % (torch.cuda.get_device_name(0), B, N))
    for dim in (3, 2):
        paths = torch.tensor(random_paths(rng, B, N, dim), device="cuda")
        traj, start, goal = paths[:, 1:-1].contiguous(), paths[:, 0].contiguous(), paths[:, -1].contiguous()
        f64 = dict(dtype=torch.float64, device="cuda")
        profile, summary = torch.empty(B, N + 2, 4, **f64), torch.empty(B, 4, **f64)
        gear = torch.empty(B, N + 1, dtype=torch.int8, device="cuda")

        def run_profile():
            L.check(lib.nfopp_path_time_profile(L.ptr(traj), L.ptr(start), L.ptr(goal), B, N, dim, lim, None, None,
                                                L.ptr(profile, torch.float64), L.ptr(gear, torch.int8),
                                                L.ptr(summary, torch.float64), L.stream_ptr()))

        print("dim %d" % dim)
        print("  nfopp_path_time_profile                  %8.4f / %8.4f / %8.4f" % timed(run_profile, warmup=3, reps=20))
        s = summary.cpu().numpy()
        print("    status 0 on %d of %d rows; mean time %.2f s, length %.2f m, stops %.1f" %
              (int((s[:, 3] == 0).sum()), B, s[:, 0].mean(), s[:, 1].mean(), s[:, 2].mean()))
        for count in (256, 2048):
            states = torch.empty(B, count, dim + 1, dtype=torch.float32, device="cuda")
            segment = torch.empty(B, count, dtype=torch.int32, device="cuda")
            dt = float(s[:, 0].max()) / (count - 1)

            def run_sample():
                L.check(lib.nfopp_path_time_sample(L.ptr(traj), L.ptr(start), L.ptr(goal), B, N, dim, lim,
                                                   L.ptr(profile, torch.float64), L.ptr(gear, torch.int8), 0.0, dt, count,
                                                   L.ptr(states), L.ptr(segment, torch.int32), L.stream_ptr()))

            print("  nfopp_path_time_sample, %4d instants     %8.4f / %8.4f / %8.4f" % ((count,) + timed(run_sample, warmup=3, reps=20)))
        t = timed(lambda: nfopp.time_parametrize(traj, start, goal, limits).sample(dt, 256), warmup=3, reps=20)
        print("  time_parametrize(...).sample(dt, 256)    %8.4f / %8.4f / %8.4f   (with allocation and host work)" % t)


if __name__ == "__main__":
    main()
