#!/usr/bin/env python3
"""Device-event timings of the moving-obstacle overlay (csrc/track_field.hip) on one GPU: the figures of
profiles/track_field.txt and DESIGN.md 27.  BatchPlanner.step(n=100) at 4096 trajectories x 256 waypoints, D = 3, on the cfg4
100 x 100 map with a DistanceField of one disc, without moving obstacles and with M = 0, 8, 64, 256 constant-velocity tracks of
K = 256 instants, the configurations alternating round by round in one process; then the launches alone -- the distance
field's collision entry, nfopp_traj_track_overlay per M, nfopp_traj_update -- on the state the steps have left.  With
tools/micro/track_layouts built (see its header) the fetch layouts are timed by it, before this process touches the GPU, and
its lines are appended.  Medians of event-timed calls after a spin-up; a call that is timed is 100 steps or 50 launches.

Usage:  python tools/track_field_timing.py
"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from sdf_field_timing import alternating  # noqa: E402

B, N, K, STEPS, ROUNDS = 4096, 256, 256, 100, 7
TRACK_COUNTS = (0, 8, 64, 256)
DT = 0.5


def main():
    # the stand-alone layout program runs first, as a child of a process that has not touched the GPU yet
    micro = os.path.join(ROOT, "tools", "micro", "track_layouts")
    layouts = subprocess.run([micro], check=True, capture_output=True, text=True).stdout if os.path.exists(micro) else None
    import nfopp
    import bench
    from nfopp import _lib
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    env = bench.GridMap()
    grid = nfopp.OccupancyGrid(env.grid, bench.BOUNDS, 1.0, device=device)
    field = nfopp.DistanceField(grid, radius=0.5, margin=0.5, gain=2.0)
    rng = np.random.default_rng(4321)
    starts, goals = env.free_poses(rng, B), env.free_poses(rng, B)
    x0, x1, y0, y1 = bench.BOUNDS
    planners = {}
    for m in (None,) + TRACK_COUNTS:
        moving = None
        if m is not None:
            p0 = torch.tensor(np.stack([rng.uniform(x0, x1, m), rng.uniform(y0, y1, m)], 1).reshape(m, 2), device=device)
            v = torch.tensor(rng.uniform(-0.5, 0.5, (m, 2)), device=device)
            tracks = nfopp.constant_velocity_tracks(p0, v, DT, K)
            moving = nfopp.MovingObstacles(tracks, DT, radius=0.5, robot_radius=0.5, margin=0.5, gain=2.0)
        p = nfopp.BatchPlanner(field, B, N, bench.bench_hyper(), velocity_hessian_weight=0.5, device=device, seed=bench.SEED,
                               moving=moving)
        p.init(starts, goals, bench.BOUNDS)
        if moving is not None:
            p.uniform_waypoint_times(0.0, DT * (K - 1))
        planners["no moving obstacles" if m is None else "M = %d" % m] = p
    print("device: %s; %d trajectories x %d waypoints, D = 3, cfg4 map, DistanceField of one disc, K = %d" %
          (torch.cuda.get_device_name(0), B, N, K))
    for p in planners.values():     # spin-up: code objects, clocks
        p.step(n=STEPS)
    torch.cuda.synchronize()
    res = alternating({k: (lambda p=p: p.step(n=STEPS)) for k, p in planners.items()}, ROUNDS, STEPS)
    print("BatchPlanner.step(n=%d), ms per step: median / min / max of %d alternating rounds" % (STEPS, ROUNDS))
    base = res["no moving obstacles"][0]
    for k, t in res.items():
        print("  %-22s %8.4f / %8.4f / %8.4f   (+%.1f us over no moving obstacles)" % ((k,) + t + ((t[0] - base) * 1e3,)))
    assert all(np.isfinite(p.get_paths()).all() for p in planners.values())

    # the launches alone, on the state the steps have left
    reps = 50
    lib = _lib.load()

    def overlay(e):
        for _ in range(reps):
            _lib.check(lib.nfopp_traj_track_overlay(e.moving.config_c(), _lib.ptr(e.traj), _lib.ptr(e.wp_time), e.B, e.N, e.D,
                                                    _lib.ptr(e.t), _lib.ptr(e.onf_out), None, _lib.stream_ptr()))

    e0 = planners["no moving obstacles"].engine
    calls = {"nfopp_traj_sdf_collision_eval": (lambda: [e0.collision_eval() for _ in range(reps)]),
             "nfopp_traj_update (K2)": (lambda: [e0.update(False) for _ in range(reps)])}
    for m in TRACK_COUNTS:
        calls["nfopp_traj_track_overlay, M = %d" % m] = (lambda e=planners["M = %d" % m].engine: overlay(e))
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    res = alternating(calls, ROUNDS, reps)
    print("one launch, microseconds: median / min / max of %d alternating rounds of %d launches" % (ROUNDS, reps))
    for k, t in res.items():
        print("  %-40s %8.2f / %8.2f / %8.2f" % (k, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3))
    samples = B * (N - 1)
    for m in TRACK_COUNTS[1:]:
        t = res["nfopp_traj_track_overlay, M = %d" % m][0] * 1e-3
        print("  M = %d: %.0f M disc-track candidates per launch -> %.1f G candidates/s" % (m, samples * m / 1e6, samples * m / t / 1e9))

    if layouts is not None:
        print("fetch layouts (tools/micro/track_layouts: the kernel's arithmetic on 4096 x 255 samples along straight lines):")
        print(layouts.rstrip())
    else:
        print("fetch layouts: tools/micro/track_layouts is not built (its header has the command)")


if __name__ == "__main__":
    main()
