#!/usr/bin/env python3
"""Device-event timings of the grid distance transform (csrc/grid_edt.hip) on one GPU: the figures of
profiles/grid_edt.txt and DESIGN.md 13.  nfopp_grid_edt alone (both outputs) on the cfg4 100 x 100 map, that map tiled to
400 x 400, a 4096 x 4096 grid with ONE occupied cell (the row pass's worst case: every cell scans until its offset exceeds
its distance to that cell) and a 4096 x 4096 tiling of the map; then OccupancyGrid.inflated without its cache, and the
whole grid_search_init with and without a clearance at 4096 problems x 256 waypoints on the cfg4 map.  Medians of
event-timed calls; the seeding calls include their host work (two host reads per level).

Usage:  python tools/grid_edt_timing.py
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
from nfopp import _lib  # noqa: E402
import bench  # noqa: E402
from obstacle_map_timing import timed  # noqa: E402


def edt_call(occ, border=0):
    lib = _lib.load()
    rows, cols = occ.shape
    dist2 = torch.empty(rows, cols, dtype=torch.int32, device="cuda")
    nearest = torch.empty(rows, cols, dtype=torch.int32, device="cuda")
    ws_bytes = lib.nfopp_grid_edt_workspace_bytes(rows, cols)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device="cuda")
    args = (_lib.ptr(occ, torch.uint8), rows, cols, border, _lib.ptr(dist2, torch.int32), _lib.ptr(nearest, torch.int32),
            _lib.ptr(ws, torch.int32), ws_bytes)
    return (lambda: _lib.check(lib.nfopp_grid_edt(*(args + (_lib.stream_ptr(),))))), dist2


def main():
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    env = bench.GridMap()
    truth = env.device_checker(device)
    grid = nfopp.OccupancyGrid.from_checker(truth, 1.0, boundaries=(0.5, 100.0, 0.5, 100.0))
    base = grid.occupancy_host
    one = np.zeros((4096, 4096), np.uint8)
    one[1234, 2345] = 1
    cases = (("cfg4 map 100 x 100", base, 20), ("cfg4 map tiled 400 x 400", np.tile(base, (4, 4)), 20),
             ("4096 x 4096, one occupied cell", one, 3), ("cfg4 map tiled 4096 x 4096", np.tile(base, (41, 41))[:4096, :4096], 5))
    print("device: %s; nfopp_grid_edt with both outputs, median / min / max of event-timed calls, ms" % torch.cuda.get_device_name(0))
    for name, img, reps in cases:
        occ = torch.tensor(np.ascontiguousarray(img), device="cuda")
        call, dist2 = edt_call(occ)
        t = timed(call, warmup=1, reps=reps)
        finite = dist2[dist2 < 2 ** 31 - 1]
        print("  %-34s %9.4f / %9.4f / %9.4f   occupied %.3f, largest dist2 %d" %
              ((name,) + t + (float((occ != 0).float().mean()), int(finite.max()) if finite.numel() else -1)))

    def inflate_uncached():
        grid._edt.clear()
        grid._inflated.clear()
        grid.inflated(1.0)
    print("OccupancyGrid.inflated(1.0) on the cfg4 map, nothing cached (transform + threshold): %.4f / %.4f / %.4f" % timed(inflate_uncached))
    rng = np.random.default_rng(4321)
    B, N = 4096, 256
    starts = torch.tensor(env.free_poses(rng, B), dtype=torch.float32, device="cuda")
    goals = torch.tensor(env.free_poses(rng, B), dtype=torch.float32, device="cuda")
    for name, clearance in (("no clearance", None), ("clearance 1 m", 1.0), ("clearance (2 m, 1 m)", (2.0, 1.0))):
        t = timed(lambda: nfopp.grid_search_init(grid, starts, goals, N, clearance=clearance), warmup=1, reps=5)
        line = "grid_search_init %d x %d, %-22s %9.3f / %9.3f / %9.3f" % ((B, N, name) + t)
        if clearance is not None:
            margin = nfopp.grid_search_init(grid, starts, goals, N, clearance=clearance)[2]
            line += "   seeded at a margin: %d of %d" % (int((margin > 0).sum()), B)
        print(line)


if __name__ == "__main__":
    main()
