#!/usr/bin/env python3
"""Device-event timings of the any-angle stages (csrc/grid_any_angle.hip, nfopp_grid_seed_polylines) on one GPU: the
figures of profiles/grid_any_angle.txt and DESIGN.md 15.  4096 problems x 256 waypoints on the cfg4 100 x 100 map, as the
stage timings of DESIGN.md 9 (fields 3.75 ms, trace 0.68 ms, seeding 0.18 ms): nfopp_grid_shorten_paths alone for a few
lookahead values and clearance levels, nfopp_grid_seed_polylines alone beside nfopp_grid_seed_trajectories on the same
paths, then the whole grid_search_init with and without the flag.  Medians of event-timed calls; the grid_search_init
calls include their host work.

Usage:  python tools/grid_any_angle_timing.py
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
from nfopp import grid_search as gs  # noqa: E402
import bench  # noqa: E402
from obstacle_map_timing import timed  # noqa: E402


def main():
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    env = bench.GridMap()
    truth = env.device_checker(device)
    grid = nfopp.OccupancyGrid.from_checker(truth, 1.0, boundaries=(0.5, 100.0, 0.5, 100.0))
    rng = np.random.default_rng(4321)
    B, N = 4096, 256
    starts = torch.tensor(env.free_poses(rng, B), dtype=torch.float32, device="cuda")
    goals = torch.tensor(env.free_poses(rng, B), dtype=torch.float32, device="cuda")
    grid.distance_transform(False)
    print("device: %s; %d problems x %d waypoints on the cfg4 map, median / min / max of event-timed calls, ms" %
          (torch.cuda.get_device_name(0), B, N))
    for name, clearance in (("plain grid", None), ("clearance 1 m", 1.0), ("clearance (2 m, 1 m)", (2.0, 1.0))):
        if clearance is None:
            cells, count, status, _, s, g = gs._search(grid, starts, goals)
            cells2 = None
        else:
            cells, count, status, _, s, g, _, cells2 = gs._search_with_clearance(grid, starts, goals, clearance)
        ok = status == 0
        print("%s: %d of %d paths, %d cells at most, %.1f on average" %
              (name, int(ok.sum()), B, int(cells.shape[1]), float(count[ok].float().mean())))
        for lookahead in (16, 64, 256, 2 ** 30):
            t = timed(lambda: gs._shorten_paths(grid, cells, count, status, cells2, lookahead), warmup=2, reps=10)
            points, point_counts, _, anchor_counts = gs._shorten_paths(grid, cells, count, status, cells2, lookahead)
            print("  nfopp_grid_shorten_paths, lookahead %-10d %8.4f / %8.4f / %8.4f   anchors per path %.1f" %
                  ((lookahead,) + t + (float(anchor_counts[ok].float().mean()),)))
        points, point_counts = gs._shorten_paths(grid, cells, count, status, cells2, 256)[:2]
        out = torch.empty(B, N, 3, dtype=torch.float32, device="cuda")
        print("  nfopp_grid_seed_polylines                 %8.4f / %8.4f / %8.4f" %
              timed(lambda: gs.seed_polylines(grid, points, point_counts, status, s, g, N, out=out), warmup=2, reps=10))
        print("  nfopp_grid_seed_trajectories (cell path)  %8.4f / %8.4f / %8.4f" %
              timed(lambda: gs.seed_trajectories(grid, cells, count, status, s, g, N, out=out), warmup=2, reps=10))
        for any_angle in (False, True):
            t = timed(lambda: nfopp.grid_search_init(grid, starts, goals, N, clearance=clearance, any_angle=any_angle), warmup=1, reps=5)
            print("  grid_search_init, any_angle=%-5s         %8.3f / %8.3f / %8.3f" % ((any_angle,) + t))


if __name__ == "__main__":
    main()
