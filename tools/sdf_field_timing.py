#!/usr/bin/env python3
"""Device-event timings of planning on a distance field (csrc/sdf_field.hip) on one GPU: the figures of
profiles/sdf_field.txt and DESIGN.md 24.  BatchPlanner.step(n=100) at 4096 trajectories x 256 waypoints, D = 3, on the cfg4
100 x 100 map, for three collision models in one process -- the frozen ONF (bench.py's, fitted for 300 iterations), a
DistanceField of one disc and one of three discs -- with the three alternating round by round; then the collision kernels
alone (nfopp_traj_collision_eval and nfopp_traj_sdf_collision_eval with 1 and 3 discs), nfopp_traj_update alone, and the
bytes the distance-field kernel moves over its time.  With tools/micro/sdf_taps built (see its header) the two tap layouts
are timed by it, before this process touches the GPU, and its lines are appended.  Medians of event-timed calls after a
spin-up; a call that is timed is 100 steps (the ONF's: 70 ms) or 50 launches of one kernel.

Usage:  python tools/sdf_field_timing.py
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
B, N, STEPS, ROUNDS = 4096, 256, 100, 7


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(calls, rounds, per_call):
    """calls: name -> fn.  Each round times every call once, in an order that rotates -> name -> (median, min, max) / per_call."""
    names = list(calls)
    times = {k: [] for k in names}
    for r in range(rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            times[k].append(event_ms(calls[k]) / per_call)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def main():
    # the stand-alone tap-layout program runs first, as a child of a process that has not touched the GPU yet
    micro = os.path.join(ROOT, "tools", "micro", "sdf_taps")
    taps = subprocess.run([micro], check=True, capture_output=True, text=True).stdout if os.path.exists(micro) else None
    import nfopp
    import bench
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    env = bench.GridMap()
    # the checker's nodes (origin 0, cell 1 m: node i at i + 0.5) are the centres of this grid's cells
    grid = nfopp.OccupancyGrid(env.grid, bench.BOUNDS, 1.0, device=device)
    onf, fit_loss = bench.make_onf(device, env, 300, 4096)
    fields = {"ONF (frozen, F = 220)": onf,
              "DistanceField, 1 disc": nfopp.DistanceField(grid, radius=0.5, margin=0.5, gain=2.0),
              "DistanceField, 3 discs": nfopp.DistanceField(grid, discs=nfopp.DistanceField.discs_for_box((-0.5, 1.5, -0.4, 0.4), 3),
                                                            margin=0.5, gain=2.0)}
    rng = np.random.default_rng(4321)
    starts, goals = env.free_poses(rng, B), env.free_poses(rng, B)
    planners = {}
    for name, field in fields.items():
        p = nfopp.BatchPlanner(field, B, N, bench.bench_hyper(), velocity_hessian_weight=0.5, device=device, seed=bench.SEED)
        p.init(starts, goals, bench.BOUNDS)
        planners[name] = p
    print("device: %s; %d trajectories x %d waypoints, D = 3, cfg4 map (ONF fit loss %.3f)" % (torch.cuda.get_device_name(0), B, N, fit_loss))
    for p in planners.values():     # spin-up: code objects, clocks
        p.step(n=STEPS)
    torch.cuda.synchronize()
    res = alternating({k: (lambda p=p: p.step(n=STEPS)) for k, p in planners.items()}, ROUNDS, STEPS)
    print("BatchPlanner.step(n=%d), ms per step: median / min / max of %d alternating rounds" % (STEPS, ROUNDS))
    for k, t in res.items():
        print("  %-24s %8.4f / %8.4f / %8.4f" % ((k,) + t))
    base = res["ONF (frozen, F = 220)"][0]
    for k in list(res)[1:]:
        print("  ONF step / %s step: %.1f x" % (k, base / res[k][0]))

    assert all(np.isfinite(p.get_paths()).all() for p in planners.values())

    # the kernels alone, on the state the steps have left
    reps = 50
    calls = {}
    for name, p in planners.items():
        e = p.engine
        calls["collision entry, " + name] = (lambda e=e: [e.collision_eval() for _ in range(reps)])
    e = planners["DistanceField, 1 disc"].engine
    calls["nfopp_traj_update (K2)"] = (lambda e=e: [e.update(False) for _ in range(reps)])
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    res = alternating(calls, ROUNDS, reps)
    print("one launch, microseconds: median / min / max of %d alternating rounds of %d launches" % (ROUNDS, reps))
    for k, t in res.items():
        print("  %-44s %8.2f / %8.2f / %8.2f" % (k, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3))
    moved = B * N * 12 + B * (N - 1) * (4 + 16)      # the waypoints read once, t and the rows written
    for k in ("DistanceField, 1 disc", "DistanceField, 3 discs"):
        t = res["collision entry, " + k][0] * 1e-3
        print("  %s: %.1f MB of trajectories in, t and rows out -> %.2f TB/s (the image, %d KB, is served by the caches)" %
              (k, moved / 1e6, moved / t / 1e12, grid.shape[0] * grid.shape[1] * 4 // 1024))

    if taps is not None:
        print("tap layouts (tools/micro/sdf_taps: the kernel's arithmetic on 4096 x 255 samples along straight lines):")
        print(taps.rstrip())
    else:
        print("tap layouts: tools/micro/sdf_taps is not built (its header has the command)")


if __name__ == "__main__":
    main()
