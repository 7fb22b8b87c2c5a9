#!/usr/bin/env python3
"""8-connected seed against lattice seed on the cfg4 map, on the problems of tools/grid_seed_quality.py.

The same 256 problems (bench.py's generator, the same random stream) are planned from the straight line, from the
8-connected grid-search seed and from the lattice seed with turn_cost 0 and 2, for the same number of steps with the
frozen pre-fitted field.  Per row: the collision-free share at the seed and after the steps (BatchPlanner.evaluate), the
cusps per path at the seed and after the steps (BatchPlanner.path_stats), and the angle between the start heading and the
seed's first segment (start -> first waypoint), and the same angle to the first waypoint two cells away, mean and 90th
percentile in degrees.  With --gears the lattice search with reverse moves (nfopp.GearLattice) adds a row per gear setting,
with the gear changes and reversals of its seeds and how many of the problems the forward-only lattice leaves unseeded
(status 1) it seeds.  Information, not a gate.

Usage:  python tools/lattice_seed_quality.py [--problems 256] [--steps 500] [--gears] [--out profiles/lattice_search.txt]
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
import bench  # noqa: E402


def departure_angles(planner, reach=2.0):
    """Per problem, degrees (float64 on the host): |wrap(direction - start heading)| for the direction start -> first
    waypoint (the seed's first segment: it runs from the start to the centre of the start's own cell, wherever in the
    cell the start lies) and for the direction start -> the first waypoint at least `reach` metres away (two cells on
    cfg4), which is where the path the search chose shows."""
    eng = planner.engine
    start = eng.start.double().cpu().numpy()
    xy = eng.traj.view(eng.B, eng.N, eng.D)[:, :, :2].double().cpu().numpy()
    rel = xy - start[:, None, :2]
    far = np.argmax(np.hypot(rel[..., 0], rel[..., 1]) >= reach, axis=1)       # 0 where no waypoint is that far
    out = []
    for v in (rel[:, 0], rel[np.arange(len(rel)), far]):
        d = np.arctan2(v[:, 1], v[:, 0]) - start[:, 2]
        out.append(np.degrees(np.abs((d + np.pi) % (2 * np.pi) - np.pi)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--fit-iters", type=int, default=300)
    ap.add_argument("--gears", action="store_true", help="add the rows of the search with reverse moves")
    ap.add_argument("--out", default=None, help="append the result line to this file as well")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    env = bench.GridMap()
    onf, fit_loss = bench.make_onf(device, env, args.fit_iters, 4096)
    rng = np.random.default_rng(4321)
    big = max(args.problems, 4096)                      # tools/grid_seed_quality.py draws 4096 and plans the first 256
    starts, goals = env.free_poses(rng, big), env.free_poses(rng, big)
    truth = env.device_checker(device)
    grid = nfopp.OccupancyGrid.from_checker(truth, 1.0, boundaries=(0.5, 100.0, 0.5, 100.0))
    lgrid = nfopp.LatticeGrid.from_grid(grid)
    N, B = 256, args.problems
    result = {"map": env.name, "problems": B, "steps": args.steps, "waypoints": N, "onf_fit_loss": fit_loss}
    rows = [("straight_line", None, 0), ("grid_search", grid, 0), ("lattice_turn_cost_0", lgrid, 0), ("lattice_turn_cost_2", lgrid, 2)]
    if args.gears:   # (turn, reverse, cusp)
        rows += [("lattice_gears_%d_%d_%d" % (tc, rc, cc), nfopp.GearLattice(lgrid, rc, cc), tc)
                 for tc, rc, cc in ((0, 0, 0), (0, 1, 3), (2, 1, 3), (2, 2, 6))]   # 16 * 100 * 100 * (1 + costs) < 2^21: a cost sum of at most 12
    unseeded = None
    for name, ini, tc in rows:
        planner = nfopp.BatchPlanner(onf, B, N, bench.bench_hyper(), velocity_hessian_weight=0.5, device=device, seed=bench.SEED)
        planner.init(starts[:B], goals[:B], bench.BOUNDS, initializer=ini, seed_turn_cost=tc)
        angle, angle_far = departure_angles(planner)
        collides0, _ = planner.evaluate(truth)
        free0 = 1.0 - float(collides0.float().mean())      # read now: evaluate() returns the planner's own buffer
        stats0 = planner.path_stats().clone()
        cusps0 = stats0[:, nfopp.PATH_STAT_CUSPS]
        planner.step(n=args.steps)
        collides, length = planner.evaluate(truth)
        stats = planner.path_stats()
        cusps = stats[:, nfopp.PATH_STAT_CUSPS]
        free = collides == 0
        result[name] = {"collision_free_at_seed": free0,
                        "collision_free_after_steps": float(free.float().mean()),
                        "cusps_per_path_at_seed": float(cusps0.mean()), "cusps_per_path_after_steps": float(cusps.mean()),
                        "first_segment_angle_deg_mean": float(angle.mean()), "first_segment_angle_deg_p90": float(np.percentile(angle, 90)),
                        "angle_at_two_cells_deg_mean": float(angle_far.mean()), "angle_at_two_cells_deg_p90": float(np.percentile(angle_far, 90)),
                        "mean_length_of_free_paths": float(length[free].mean()) if bool(free.any()) else None}
        if ini is not None:
            result[name]["seed_status_counts"] = np.bincount(planner.seed_status.cpu().numpy(), minlength=3).tolist()
        if name == "lattice_turn_cost_0":
            unseeded = planner.seed_status == 1
        if isinstance(ini, nfopp.GearLattice):
            ok = planner.seed_status == 0
            result[name].update(
                gear_changes_per_seeded_path=float(planner.seed_gear_changes[ok].float().mean()),
                seeds_with_a_gear_change=int((planner.seed_gear_changes[ok] > 0).sum()),
                reversals_per_path_at_seed=float(stats0[:, nfopp.PATH_STAT_REVERSALS].mean()),
                reversals_per_path_after_steps=float(stats[:, nfopp.PATH_STAT_REVERSALS].mean()),
                seeded_of_the_forward_lattice_unreachable="%d of %d" % (int((ok & unseeded).sum()), int(unseeded.sum())))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
