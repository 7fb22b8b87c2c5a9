#!/usr/bin/env python3
"""Device-event timings of planning on a heading-layered distance field (csrc/heading_field.hip) on one GPU: the figures of
profiles/heading_field.txt and DESIGN.md 26.  BatchPlanner.step(n=100) at 4096 trajectories x 256 waypoints, D = 3, on the cfg4
100 x 100 map, for seven collision models in one process -- HeadingDistanceField with 8, 16, 32 and 64 slices of the box
(-0.5, 1.5, -0.4, 0.4) from a DeviceRectangleChecker, and DistanceField with 1, 3 and 8 discs covering the same box -- the
seven alternating round by round; then the collision entries alone, the bytes they stream over their time, how long
from_checker and update take, and the collision entry on a 384 x 384 image with 8 and with 64 slices (4.7 and 37.7 MB).
Medians of event-timed calls after a spin-up; a call that is timed is 100 steps or 50 launches of one kernel.

Usage:  python tools/heading_field_timing.py
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from sdf_field_timing import alternating  # noqa: E402

B, N, STEPS, ROUNDS = 4096, 256, 100, 7
BOX = (-0.5, 1.5, -0.4, 0.4)
LAYER_COUNTS = (8, 16, 32, 64)
DISC_COUNTS = (1, 3, 8)
FRAME = (0.0, 99.5, 0.0, 99.5)     # the raster rule (cells = extent // resolution + 1) gives the map's 100 x 100 cells from it


def wall_ms(fn, repeats=5):
    """Median wall-clock milliseconds of fn() with the device drained before and after: host work included."""
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    import nfopp
    import bench
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    env = bench.GridMap()
    occ = np.asarray(env.grid) != 0
    grid = nfopp.OccupancyGrid(occ, bench.BOUNDS, 1.0, device=device)
    rows, cols = np.nonzero(occ)
    points = np.stack([cols + 0.5, rows + 0.5], 1)        # the centres of the occupied cells
    checker = nfopp.DeviceRectangleChecker(points, BOX, bench.BOUNDS, device=device)
    fields = {}
    for n_layers in LAYER_COUNTS:
        fields["HeadingDistanceField, L = %d" % n_layers] = nfopp.HeadingDistanceField.from_checker(
            checker, 1.0, layers=n_layers, boundaries=FRAME, margin=0.5, gain=2.0)
    for n_discs in DISC_COUNTS:
        fields["DistanceField, %d disc%s" % (n_discs, "" if n_discs == 1 else "s")] = nfopp.DistanceField(
            grid, discs=nfopp.DistanceField.discs_for_box(BOX, n_discs), margin=0.5, gain=2.0)
    rng = np.random.default_rng(4321)
    starts, goals = env.free_poses(rng, B), env.free_poses(rng, B)
    planners = {}
    for name, field in fields.items():
        p = nfopp.BatchPlanner(field, B, N, bench.bench_hyper(), velocity_hessian_weight=0.5, device=device, seed=bench.SEED)
        p.init(starts, goals, bench.BOUNDS)
        planners[name] = p
    print("device: %s; %d trajectories x %d waypoints, D = 3, cfg4 map, box %s" % (torch.cuda.get_device_name(0), B, N, BOX))
    for p in planners.values():     # spin-up: code objects, clocks
        p.step(n=STEPS)
    torch.cuda.synchronize()
    res = alternating({k: (lambda p=p: p.step(n=STEPS)) for k, p in planners.items()}, ROUNDS, STEPS)
    print("BatchPlanner.step(n=%d), ms per step: median / min / max of %d alternating rounds" % (STEPS, ROUNDS))
    for k, t in res.items():
        print("  %-32s %8.4f / %8.4f / %8.4f" % ((k,) + t))
    assert all(np.isfinite(p.get_paths()).all() for p in planners.values())

    # the collision entries alone, on the state the steps have left
    reps = 50
    calls = {"collision entry, " + name: (lambda e=p.engine: [e.collision_eval() for _ in range(reps)]) for name, p in planners.items()}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    res = alternating(calls, ROUNDS, reps)
    moved = B * N * 12 + B * (N - 1) * (4 + 16)      # the waypoints read once, t and the rows written
    print("one launch, microseconds: median / min / max of %d alternating rounds of %d launches; %.1f MB streamed per launch "
          "(waypoints in, t and rows out) over the median" % (ROUNDS, reps, moved / 1e6))
    for k, t in res.items():
        f = fields[k[len("collision entry, "):]]
        print("  %-50s %8.2f / %8.2f / %8.2f   %.2f TB/s   image %d KB" %
              (k, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, moved / (t[0] * 1e-3) / 1e12, f.field.numel() * 4 // 1024))

    # field construction: one labels call and 2 L distance transforms, host work included
    print("field construction on the 100 x 100 map, wall-clock ms with the device drained (median of 5):")
    for n_layers in LAYER_COUNTS:
        f = fields["HeadingDistanceField, L = %d" % n_layers]
        make = wall_ms(lambda: nfopp.HeadingDistanceField.from_checker(checker, 1.0, layers=n_layers, boundaries=FRAME))
        occ_dev = (f.field < 0).to(torch.uint8)
        print("  L = %2d: from_checker %8.2f   update(layers) %8.2f   update_from_checker %8.2f" %
              (n_layers, make, wall_ms(lambda: f.update(occ_dev)), wall_ms(lambda: f.update_from_checker(checker))))

    # a 384 x 384 image: does the collision entry still tap at cache speed when the image is 37.7 MB?
    big = np.kron(occ, np.ones((4, 4), bool))[:384, :384]
    bounds = (0.0, 96.0, 0.0, 96.0)
    calls, sizes = {}, {}
    keep = []

    def inside(poses):     # xy into the smaller map, headings as they are
        return np.concatenate([np.clip(poses[:, :2], 0.5, 95.5), poses[:, 2:]], 1).astype(np.float32)

    for n_layers in (8, 64):
        layers = np.stack([np.roll(big, (k, 2 * k), (0, 1)) for k in range(n_layers)]).astype(np.uint8)
        f = nfopp.HeadingDistanceField(layers, bounds, 0.25, margin=0.5, gain=2.0, device=device)
        p = nfopp.BatchPlanner(f, B, N, bench.bench_hyper(), velocity_hessian_weight=0.5, device=device, seed=bench.SEED)
        p.init(inside(starts), inside(goals), bounds)
        keep.append(p)
        name = "384 x 384, L = %d" % n_layers
        calls[name] = (lambda e=p.engine: [e.collision_eval() for _ in range(reps)])
        sizes[name] = f.field.numel() * 4 / 1e6
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    res = alternating(calls, ROUNDS, reps)
    print("collision entry on a 384 x 384 image at 0.25 m (straight seeds across the whole map), microseconds: median / min / max")
    for k, t in res.items():
        print("  %-24s %8.2f / %8.2f / %8.2f   %.2f TB/s   image %.1f MB" %
              (k, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, moved / (t[0] * 1e-3) / 1e12, sizes[k]))


if __name__ == "__main__":
    main()
