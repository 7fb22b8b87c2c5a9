#!/usr/bin/env python3
"""Device-event timings of the lattice search (csrc/lattice_search.hip) beside the 8-connected search on the same problems,
in the same process: the figures of profiles/lattice_search.txt and DESIGN.md 20.

Fields and trace are timed on their own through the C entries, outputs and workspaces preallocated, median of 20 calls by
HIP events: the 4096 x 256 batch of DESIGN.md 9 on the cfg4 100 x 100 corridor map, and a 384 x 384 map of random blocks
(8 * 384 * 384 = 1 179 648 < 2^21, so turn_cost 0 is admitted) with a smaller batch.  Information, not a gate.

Usage:  python tools/lattice_timing.py [--reps 20] [--out profiles/lattice_search.txt]
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
from obstacle_map_timing import blob_map, timed  # noqa: E402

I32 = torch.int32


def _unique(key):
    uniq, inverse = torch.unique(key, return_inverse=True)
    return uniq, inverse.to(I32).contiguous()


def lattice_calls(lg, starts, goals, turn_cost, goal_heading):
    """-> (fields call, trace call, facts) over preallocated buffers."""
    lib = _lib.load()
    rows, cols = lg.shape
    dev = starts.device
    s_states = lg.states_of(starts)
    g_states = lg.states_of(goals, free_heading=goal_heading == "free")
    uniq, fidx = _unique((g_states[:, 0].long() * cols + g_states[:, 1].long()) * 9 + g_states[:, 2].long() + 1)
    cell = uniq // 9
    u_states = torch.stack([cell // cols, cell % cols, uniq % 9 - 1], 1).to(I32).contiguous()
    g, b = u_states.shape[0], starts.shape[0]
    fields = torch.empty(g, 8, rows, cols, 2, dtype=I32, device=dev)
    ws_bytes = lib.nfopp_lattice_fields_workspace_bytes(rows, cols, turn_cost, g)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    count, status, cost = (torch.empty(n, dtype=I32, device=dev) for n in (b, b, 2 * b))

    def run_fields():
        _lib.check(lib.nfopp_lattice_distance_fields(_lib.ptr(lg.layers, torch.uint8), lg.n_layers, rows, cols, _lib.ptr(u_states, I32),
                                                     g, turn_cost, _lib.ptr(fields, I32), _lib.ptr(ws, torch.int64) if ws_bytes else None,
                                                     ws_bytes, _lib.stream_ptr()))

    def trace(max_len, cells, heads):
        _lib.check(lib.nfopp_lattice_trace_paths(_lib.ptr(fields, I32), 0, g, g, rows, cols, turn_cost, _lib.ptr(s_states, I32),
                                                 _lib.ptr(g_states, I32), _lib.ptr(fidx, I32), b, max_len, _lib.ptr(cells, I32) if max_len else None,
                                                 _lib.ptr(heads, I32) if max_len else None, _lib.ptr(count, I32), _lib.ptr(status, I32),
                                                 _lib.ptr(cost, I32), _lib.stream_ptr()))

    run_fields()
    trace(0, None, None)
    max_len = max(int(count.max()), 1)
    cells = torch.empty(b, max_len, 2, dtype=I32, device=dev)
    heads = torch.empty(b, max_len, dtype=I32, device=dev)

    def run_trace():   # the sizing pass and the writing pass, as lattice_search_paths makes them
        trace(0, None, None)
        trace(max_len, cells, heads)

    run_trace()
    facts = dict(goals=g, max_len=max_len, ok=int((status == 0).sum()), form="workspace" if ws_bytes else "LDS")
    return run_fields, run_trace, facts


def grid_calls(grid, starts, goals):
    lib = _lib.load()
    rows, cols = grid.shape
    dev = starts.device
    s_cells, g_cells = grid.cells_of(starts), grid.cells_of(goals)
    uniq, fidx = _unique(g_cells[:, 0].long() * cols + g_cells[:, 1].long())
    u_cells = torch.stack([uniq // cols, uniq % cols], 1).to(I32).contiguous()
    g, b = u_cells.shape[0], starts.shape[0]
    fields = torch.empty(g, rows, cols, 2, dtype=I32, device=dev)
    ws_bytes = lib.nfopp_grid_fields_workspace_bytes(rows, cols, g)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    count, status, cost = (torch.empty(n, dtype=I32, device=dev) for n in (b, b, 2 * b))

    def run_fields():
        _lib.check(lib.nfopp_grid_distance_fields(_lib.ptr(grid.occupancy, torch.uint8), rows, cols, _lib.ptr(u_cells, I32), g,
                                                  _lib.ptr(fields, I32), _lib.ptr(ws, torch.int64) if ws_bytes else None, ws_bytes,
                                                  _lib.stream_ptr()))

    def trace(max_len, cells):
        _lib.check(lib.nfopp_grid_trace_paths(_lib.ptr(fields, I32), g, rows, cols, _lib.ptr(s_cells, I32), _lib.ptr(g_cells, I32),
                                              _lib.ptr(fidx, I32), b, max_len, _lib.ptr(cells, I32) if max_len else None,
                                              _lib.ptr(count, I32), _lib.ptr(status, I32), _lib.ptr(cost, I32), _lib.stream_ptr()))

    run_fields()
    trace(0, None)
    max_len = max(int(count.max()), 1)
    cells = torch.empty(b, max_len, 2, dtype=I32, device=dev)

    def run_trace():
        trace(0, None)
        trace(max_len, cells)

    run_trace()
    facts = dict(goals=g, max_len=max_len, ok=int((status == 0).sum()), form="workspace" if ws_bytes else "LDS")
    return run_fields, run_trace, facts


def report(title, grid, starts, goals, reps, lines):
    lines.append(title)
    lg = nfopp.LatticeGrid.from_grid(grid)
    f, t, facts = grid_calls(grid, starts, goals)
    base_f, base_t = timed(f, warmup=2, reps=reps), timed(t, warmup=2, reps=reps)
    lines.append("  8-connected                        fields %9.3f  trace %8.3f   (%d goal cells, %s form, longest path %d cells, "
                 "%d of %d reached)" % (base_f[0], base_t[0], facts["goals"], facts["form"], facts["max_len"], facts["ok"], len(starts)))
    for tc, mode in ((0, "fixed"), (2, "fixed"), (0, "free")):
        if 8 * grid.shape[0] * grid.shape[1] * (1 + tc) >= 2 ** 21:
            lines.append("  lattice turn_cost %d: refused, 8 * rows * cols * (1 + turn_cost) reaches 2^21" % tc)
            continue
        f, t, facts = lattice_calls(lg, starts, goals, tc, mode)
        tf, tt = timed(f, warmup=2, reps=reps), timed(t, warmup=2, reps=reps)
        lines.append("  lattice turn_cost %d, %-5s heading  fields %9.3f  trace %8.3f   (%d goal states, %s form, longest path %d "
                     "states, %d of %d reached)   fields x %.1f, trace x %.1f of the 8-connected"
                     % (tc, mode, tf[0], tt[0], facts["goals"], facts["form"], facts["max_len"], facts["ok"], len(starts),
                        tf[0] / base_f[0], tt[0] / base_t[0]))


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
    report("cfg4 map %d x %d, 4096 problems" % grid.shape, grid, starts, goals, args.reps, lines)
    side = 384
    occ = blob_map(np.random.default_rng(384), side, 160, 8, 40) > 0
    big = nfopp.OccupancyGrid(occ, (0.0, float(side), 0.0, float(side)), 1.0, device=device)
    free = np.argwhere(~occ)
    pick = free[rng.integers(0, len(free), (2, args.big_batch))]
    poses = [np.concatenate([p[:, ::-1] + 0.5, rng.uniform(-np.pi, np.pi, (len(p), 1))], 1).astype(np.float32) for p in pick]
    report("random blocks %d x %d (%.0f %% walls), %d problems" % (side, side, 100.0 * occ.mean(), args.big_batch), big,
           torch.tensor(poses[0], device=device), torch.tensor(poses[1], device=device), args.reps, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
