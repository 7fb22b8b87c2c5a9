#!/usr/bin/env python3
"""Straight-line seed against grid-search seed on the cfg4 map (the committed 100 x 100 occupancy grid of corridors).

The same problems (bench.py's generator) are planned twice for the same number of steps with the frozen pre-fitted field:
once from the stock straight line, once from the grid-search seed (nfopp/grid_search.py).  Prints the collision-free rate
from BatchPlanner.evaluate for both, and the seeding time split into its three stages by events.  With --clearance the
grid-search seed is planned once more per margin (metres; the cfg4 cell is 1 m), seeded off the walls by that margin
(grid_search_init's `clearance`).  With --any-angle every grid-search row is planned once more from the any-angle seed
(grid_search_init's `any_angle`).  Information, not a gate.

Usage:  python tools/grid_seed_quality.py [--problems 256] [--steps 500] [--time-batch 4096] [--clearance 1 2] [--any-angle]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import nfopp  # noqa: E402
from nfopp import _grid, grid_search as gs  # noqa: E402
import bench  # noqa: E402


def stage_times(grid, starts, goals, n, repeats=5):
    """Median ms of (fields, trace, seeding) by events; the goal-cell bookkeeping in torch is outside the three."""
    starts, goals = _grid.as_device_points(grid, starts), _grid.as_device_points(grid, goals)
    rows, cols = grid.shape
    goal_cells = grid.cells_of(goals)
    uniq = torch.unique(goal_cells[:, 0].long() * cols + goal_cells[:, 1].long())
    unique_cells = torch.stack([uniq // cols, uniq % cols], 1).to(torch.int32).contiguous()
    out = {"fields": [], "trace": [], "seed": []}
    for _ in range(repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        gs.distance_fields(grid, unique_cells)
        ev[1].record()
        torch.cuda.synchronize()
        ev[2].record()
        cells, count, status, _, s, g = gs._search(grid, starts, goals)      # fields again + two traces
        ev[3].record()
        torch.cuda.synchronize()
        ev[4].record()
        gs.seed_trajectories(grid, cells, count, status, s, g, n)
        ev[5].record()
        torch.cuda.synchronize()
        out["fields"].append(ev[0].elapsed_time(ev[1]))
        out["trace"].append(max(ev[2].elapsed_time(ev[3]) - out["fields"][-1], 0.0))
        out["seed"].append(ev[4].elapsed_time(ev[5]))
    res = {k: float(np.median(v[1:])) for k, v in out.items()}
    res["unique_goal_cells"] = int(uniq.numel())
    res["max_path_cells"] = int(cells.shape[1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--time-batch", type=int, default=4096)
    ap.add_argument("--fit-iters", type=int, default=300)
    ap.add_argument("--clearance", type=float, nargs="*", default=[],
                    help="margins in metres: one more grid-search row per margin")
    ap.add_argument("--any-angle", action="store_true",
                    help="one more row per grid-search row: the seed shortened by line of sight")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    env = bench.GridMap()
    onf, fit_loss = bench.make_onf(device, env, args.fit_iters, 4096)
    rng = np.random.default_rng(4321)
    big = max(args.problems, args.time_batch)
    starts, goals = env.free_poses(rng, big), env.free_poses(rng, big)
    truth = env.device_checker(device)
    # the planner's map: DeviceGridChecker cells are centred half a cell off the origin (bench.GridMap.in_collision)
    grid = nfopp.OccupancyGrid.from_checker(truth, 1.0, boundaries=(0.5, 100.0, 0.5, 100.0))
    N, B = 256, args.problems
    result = {"map": env.name, "problems": B, "steps": args.steps, "waypoints": N, "onf_fit_loss": fit_loss}
    rows = [("straight_line", None, None, False), ("grid_search", grid, None, False)]
    rows += [("grid_search_clearance_%g" % m, grid, m, False) for m in args.clearance]
    if args.any_angle:
        rows += [(name + "_any_angle", ini, margin, True) for name, ini, margin, _ in rows[1:]]
    for name, ini, margin, any_angle in rows:
        planner = nfopp.BatchPlanner(onf, B, N, bench.bench_hyper(), velocity_hessian_weight=0.5, device=device, seed=bench.SEED)
        planner.init(starts[:B], goals[:B], bench.BOUNDS, initializer=ini, seed_clearance=margin, seed_any_angle=any_angle)
        collides0, _ = planner.evaluate(truth)
        free0 = 1.0 - float(collides0.float().mean())
        planner.step(n=args.steps)
        collides, length = planner.evaluate(truth)
        free = collides == 0
        result[name] = {"collision_free_at_seed": free0, "collision_free_after_steps": float(free.float().mean()),
                        "mean_length_of_free_paths": float(length[free].mean()) if bool(free.any()) else None}
        if ini is not None:
            result[name]["seed_status_counts"] = np.bincount(planner.seed_status.cpu().numpy(), minlength=3).tolist()
        if margin is not None:
            result[name]["seeded_at_the_margin"] = int((planner.seed_margin > 0).sum())
    result["seeding_ms_%dx%d" % (args.time_batch, N)] = stage_times(grid, starts[:args.time_batch], goals[:args.time_batch], N)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
