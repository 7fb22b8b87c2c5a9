#!/usr/bin/env python3
"""Device-event timings of the lattice search with reverse moves (csrc/lattice_gears.hip) beside the forward-only lattice
search on the same problems, in the same process: the figures of profiles/lattice_gears.txt and DESIGN.md 21.

Fields and trace are timed on their own through the C entries, outputs and workspaces preallocated, median of 20 calls by
HIP events: the 4096-problem batch on the cfg4 100 x 100 corridor map (16 * 100 * 100 * (1 + costs) < 2^21 admits a cost sum
of 12), and the largest square map the bound admits at zero costs, 362 x 362 random blocks (16 * 362 * 362 = 2 096 704 <
2^21; 384 x 384 is refused).  Information, not a gate.

Usage:  python tools/lattice_gears_timing.py [--reps 20] [--out profiles/lattice_gears.txt]
"""
import argparse
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
from lattice_timing import _unique, lattice_calls  # noqa: E402
from obstacle_map_timing import blob_map, timed  # noqa: E402

I32 = torch.int32


def gear_calls(lg, starts, goals, costs):
    """-> (fields call, trace call, facts) over preallocated buffers."""
    lib = _lib.load()
    rows, cols = lg.shape
    dev = starts.device
    s_states, g_states = lg.states_of(starts), lg.states_of(goals)
    uniq, fidx = _unique((g_states[:, 0].long() * cols + g_states[:, 1].long()) * 9 + g_states[:, 2].long() + 1)
    cell = uniq // 9
    u_states = torch.stack([cell // cols, cell % cols, uniq % 9 - 1], 1).to(I32).contiguous()
    g, b = u_states.shape[0], starts.shape[0]
    fields = torch.empty(g, 2, 8, rows, cols, 2, dtype=I32, device=dev)
    ws_bytes = lib.nfopp_lattice_gear_fields_workspace_bytes(rows, cols, costs[0], costs[1], costs[2], g)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    count, status, cost = (torch.empty(n, dtype=I32, device=dev) for n in (b, b, 2 * b))

    def run_fields():
        _lib.check(lib.nfopp_lattice_gear_distance_fields(
            _lib.ptr(lg.layers, torch.uint8), lg.n_layers, rows, cols, _lib.ptr(u_states, I32), g, costs[0], costs[1], costs[2],
            _lib.ptr(fields, I32), _lib.ptr(ws, torch.int64) if ws_bytes else None, ws_bytes, _lib.stream_ptr()))

    def trace(max_len, cells, heads, gears):
        _lib.check(lib.nfopp_lattice_gear_trace_paths(
            _lib.ptr(fields, I32), 0, g, g, rows, cols, costs[0], costs[1], costs[2], _lib.ptr(s_states, I32),
            _lib.ptr(g_states, I32), _lib.ptr(fidx, I32), b, max_len, _lib.ptr(cells, I32) if max_len else None,
            _lib.ptr(heads, I32) if max_len else None, _lib.ptr(gears, I32) if max_len else None, _lib.ptr(count, I32),
            _lib.ptr(status, I32), _lib.ptr(cost, I32), _lib.stream_ptr()))

    run_fields()
    trace(0, None, None, None)
    max_len = max(int(count.max()), 1)
    cells = torch.empty(b, max_len, 2, dtype=I32, device=dev)
    heads = torch.empty(b, max_len, dtype=I32, device=dev)
    gears = torch.zeros(b, max_len, dtype=I32, device=dev)

    def run_trace():   # the sizing pass and the writing pass, as lattice_gear_search_paths makes them
        trace(0, None, None, None)
        trace(max_len, cells, heads, gears)

    run_trace()
    changes = nfopp.lattice.gear_changes(gears, count, status)
    facts = dict(goals=g, max_len=max_len, ok=int((status == 0).sum()), form="workspace" if ws_bytes else "LDS",
                 reversing=int(((gears * (torch.arange(max_len, device=dev)[None] < count[:, None])).sum(1) > 0).sum()),
                 changes=float(changes.float().mean()))
    return run_fields, run_trace, facts


def report(title, grid, starts, goals, reps, cost_sets, lines):
    lines.append(title)
    lg = nfopp.LatticeGrid.from_grid(grid)
    f, t, facts = lattice_calls(lg, starts, goals, 0, "fixed")
    base_f, base_t = timed(f, warmup=2, reps=reps), timed(t, warmup=2, reps=reps)
    lines.append("  forward lattice, turn_cost 0        fields %9.3f  trace %8.3f   (%d goal states, %s form, longest path %d states, "
                 "%d of %d reached)" % (base_f[0], base_t[0], facts["goals"], facts["form"], facts["max_len"], facts["ok"], len(starts)))
    for costs in cost_sets:
        if 16 * grid.shape[0] * grid.shape[1] * (1 + sum(costs)) >= 2 ** 21:
            lines.append("  gears %s: refused, 16 * rows * cols * (1 + costs) reaches 2^21" % (costs,))
            continue
        f, t, facts = gear_calls(lg, starts, goals, costs)
        tf, tt = timed(f, warmup=2, reps=reps), timed(t, warmup=2, reps=reps)
        lines.append("  gears (turn, reverse, cusp) %-9s fields %9.3f  trace %8.3f   (%d goal states, %s form, longest path %d states, "
                     "%d of %d reached, %d paths reverse, %.2f gear changes a path)   fields x %.1f, trace x %.1f of the forward lattice"
                     % (costs, tf[0], tt[0], facts["goals"], facts["form"], facts["max_len"], facts["ok"], len(starts),
                        facts["reversing"], facts["changes"], tf[0] / base_f[0], tt[0] / base_t[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big-batch", type=int, default=256)
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    lines = ["device: %s; median of %d event-timed calls, ms; outputs and workspaces preallocated" %
             (torch.cuda.get_device_name(0), args.reps)]
    env = bench.GridMap()
    grid = nfopp.OccupancyGrid.from_checker(env.device_checker(device), 1.0, boundaries=(0.5, 100.0, 0.5, 100.0))
    rng = np.random.default_rng(4321)
    starts = torch.tensor(env.free_poses(rng, 4096), device=device)
    goals = torch.tensor(env.free_poses(rng, 4096), device=device)
    report("cfg4 map %d x %d, 4096 problems" % grid.shape, grid, starts, goals, args.reps, ((0, 0, 0), (2, 1, 3), (0, 4, 8)), lines)
    side = 362
    occ = blob_map(np.random.default_rng(384), side, 160, 8, 40) > 0
    big = nfopp.OccupancyGrid(occ, (0.0, float(side), 0.0, float(side)), 1.0, device=device)
    free = np.argwhere(~occ)
    pick = free[rng.integers(0, len(free), (2, args.big_batch))]
    poses = [np.concatenate([p[:, ::-1] + 0.5, rng.uniform(-np.pi, np.pi, (len(p), 1))], 1).astype(np.float32) for p in pick]
    report("random blocks %d x %d (%.0f %% walls), %d problems" % (side, side, 100.0 * occ.mean(), args.big_batch), big,
           torch.tensor(poses[0], device=device), torch.tensor(poses[1], device=device), args.reps, ((0, 0, 0), (0, 0, 1)), lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
