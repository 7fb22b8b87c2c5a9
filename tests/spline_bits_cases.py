"""The launches of the two kernels that fit the quadratic spline of csrc/spline2.h -- the path post-processor
(csrc/path_post.hip) and the seeding stage (csrc/grid_search.hip: seed_body, behind nfopp_grid_seed_trajectories,
nfopp_grid_seed_polylines and nfopp_lattice_seed_trajectories) -- whose output bits are pinned by tests/golden/spline_bits.npz:
shared by the recorder (tools/record_spline_bits.py), tests/test_gpu_spline_bits.py and tests/test_spline_bits_cpu.py.

Every input comes from a numpy generator seeded by the case's name; nothing but the outputs is stored.

Post-processor cases (POST_CASES): name -> (paths fp32 [B, n, 3], minimal_distance, distance_step, max_out).  The output buffer
is pre-filled with SENTINEL; a case records `count` int32 [B] and `out` float64 [B, max_out, 3] as the call leaves them.

  m3_unfiltered   n = 3, nothing filtered: no interior knot          m2          n = 3, middle pose filtered: count -1
  m3_filtered     n = 4, one pose filtered                           m4          n = 4, nothing filtered
  n5                                                                 n130        129 segments: second block of the pairwise sum
  n1026           the longest path; more than 64 KiB of LDS          duplicate   two equal sites (see duplicate_sites_path)
  mixed           B = 3, m = 12, 10 and 6 in one launch

Seeder cases (SEED_CASES): (entry, size, dim, directed) with entry in cells / points / lattice and size a key of SEED_SIZES:

  base      max_len 40, rows with count 1 (m = 3), 2, 40 (a full buffer), status 1 and count 43 > max_len (both the straight line)
  lds, ws   max_len 1167 (dynamic LDS) and 1168 (global workspace), a row of full length and a short one each
  n1, n2, n257   n_waypoints 1, 2 and 257 (one past the 256 threads)

The base size runs through every entry and every heading rule (dim 2, dim 3, dim 3 with angles_with_direction; the lattice
entry has its own); each other size through all three entries.  No seeder row has two equal sites: seed_sites_distinct
restates the parameter, and the CPU test asserts it, so the fixture holds no NaN."""
import zlib

import numpy as np

F32 = np.float32
I32 = np.int32
SENTINEL = -12345.678
LDS_LIMIT = 64 * 1024
RES, OX, OY = 0.1, -1.5, 2.25           # the seeder's grid frame: resolution and origin in metres


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- the parameter, restated ------------------------------------------------------------------------------------------
def chord_parameter(xy):
    """xy fp32 [m, 2] -> (par float64 [m], dist fp32 [m - 1]): fp32 segment lengths + 1e-6, their fp32 running sum widened
    to float64 and divided by its last value -- what both kernels compute (utils/math.py:58-61 on an fp32 path)"""
    xy = np.asarray(xy, F32)
    d = (xy[1:] - xy[:-1]).astype(F32)
    dist = (np.sqrt((d[:, 0] * d[:, 0]).astype(F32) + (d[:, 1] * d[:, 1]).astype(F32)).astype(F32) + F32(1e-6)).astype(F32)
    cum = np.zeros(len(xy), F32)
    acc = F32(0)
    for i, v in enumerate(dist):
        acc = F32(acc + v)
        cum[i + 1] = acc
    return cum.astype(np.float64) / np.float64(cum[-1]), dist


def cell_centres(cells):
    """fp32 xy [k, 2] of (row, col) cells: (u * res + res / 2) + origin in float64, rounded once (csrc/grid_frame.h)"""
    cells = np.asarray(cells, np.float64)
    return np.stack([(cells[:, 1] * RES + RES / 2) + OX, (cells[:, 0] * RES + RES / 2) + OY], 1).astype(F32)


def stalled_seed_polyline():
    """start | 400 cell centres in a row | goal, the goal exactly on its cell's centre: after 40 m of fp32 running sum the
    last segment, 0 + 1e-6, rounds away (the open case of DESIGN.md section 9)"""
    cells = np.stack([np.full(400, 7), np.arange(400)], 1)
    c = cell_centres(cells)
    start = (c[0] + F32([-0.03, 0.02])).astype(F32)
    return np.concatenate([start[None], c, c[-1:]])


# ---- post-processor ---------------------------------------------------------------------------------------------------
def _curve(rng, n, step=0.1):
    d = rng.uniform(0.6 * step, 1.4 * step, n)
    head = np.cumsum(rng.normal(0, 0.15, n))
    return np.stack([np.cumsum(d * np.cos(head)), np.cumsum(d * np.sin(head)), head + rng.normal(0, 0.05, n)], 1).astype(F32)


def _drop(path, idx):
    """move the poses `idx` to within minimal_distance of the goal: the filter, walking from the goal, drops them"""
    path[idx, :2] = path[-1, :2] + F32(4e-4)
    return path


def duplicate_sites_path():
    """g22's `degenerate` construction: a pose 1e-7 m beside its neighbour after 39 m; with minimal_distance 0 the filter keeps
    it, and its segment 1e-7 + 1e-6 rounds away in the fp32 running sum"""
    p = np.zeros((61, 3), F32)
    p[:60, 1], p[60, 1], p[:, 2] = np.linspace(0, 40, 60), 41.0, np.pi / 2
    p = np.insert(p, 59, p[58], axis=0)
    p[59, 0] = 1e-7
    return p


def _post_cases():
    c = {}
    md, step = 0.001, 0.05
    for name, n, drop in (("m3_unfiltered", 3, []), ("m2", 3, [1]), ("m3_filtered", 4, [2]), ("m4", 4, []), ("n5", 5, [])):
        c[name] = (_drop(_curve(_rng(name), n), drop)[None], md, step, 16)
    c["n130"] = (_curve(_rng("n130"), 130)[None], md, step, 280)
    c["n1026"] = (_curve(_rng("n1026"), 1026)[None], md, 0.25, 430)
    c["duplicate"] = (duplicate_sites_path()[None], 0.0, 1.0, 48)
    rng = _rng("mixed")
    c["mixed"] = (np.stack([_drop(_curve(rng, 12), idx) for idx in ([], [9, 10], [5, 6, 7, 8, 9, 10])]), md, step, 32)
    return c


POST_CASES = _post_cases()


def post_lds_bytes(n):
    """dynamic LDS of one nfopp_path_postprocess workgroup: 7 n + 3 doubles of spline, 4 n floats of poses and lengths"""
    return (7 * n + 3) * 8 + 4 * n * 4


def run_post(name, lib=None):
    import torch
    from nfopp import _lib
    lib = lib or _lib.load()
    paths, md, step, max_out = POST_CASES[name]
    b, n, _ = paths.shape
    dev = torch.tensor(paths, device="cuda")
    count = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((b, max_out, 3), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.nfopp_path_postprocess(_lib.ptr(dev), b, n, float(md), float(step), max_out, _lib.ptr(out, torch.float64),
                                    _lib.ptr(count, torch.int32), _lib.stream_ptr())
    assert rc == 0, lib.nfopp_last_error()
    torch.cuda.synchronize()
    return {"count": count.cpu().numpy(), "out": out.cpu().numpy()}


# ---- seeder -----------------------------------------------------------------------------------------------------------
# size -> (max_len, n_waypoints, counts, status)
SEED_SIZES = {
    "base": (40, 9, (1, 2, 40, 17, 43), (0, 0, 0, 1, 0)),
    "lds": (1167, 9, (1167, 5), (0, 0)),
    "ws": (1168, 9, (1168, 5), (0, 0)),
    "n1": (40, 1, (40, 7), (0, 0)),
    "n2": (40, 2, (40, 7), (0, 0)),
    "n257": (40, 257, (40, 7), (0, 0)),
}
SEED_CASES = tuple([(e, "base", d, w) for e in ("cells", "points") for d, w in ((2, 0), (3, 0), (3, 1))] + [("lattice", "base", 3, 0)] +
                   [c for s in ("lds", "ws", "n1", "n2", "n257") for c in (("cells", s, 3, 1), ("points", s, 2 if s in ("lds", "ws") else 3, 0),
                                                                          ("lattice", s, 3, 0))])


def seed_tag(case):
    return "%s_%s_d%d%s" % (case[0], case[1], case[2], "w" if case[3] else "")


def seed_workspace_doubles(max_len):
    """doubles one seeding problem needs (nfopp_grid_seed_workspace_bytes / 8 per problem once it exceeds LDS_LIMIT)"""
    return 7 * (max_len + 2) + 3


def seed_inputs(case):
    entry, size, dim, _ = case
    max_len, n, counts, status = SEED_SIZES[size]
    rng = _rng(seed_tag(case))
    b = len(counts)
    moves = np.asarray([(0, 1), (1, 1), (1, 0)])
    cells = np.zeros((b, max_len, 2), I32)
    heads = np.zeros((b, max_len), I32)
    points = np.zeros((b, max_len, 2), F32)
    start, goal = np.zeros((b, dim), F32), np.zeros((b, dim), F32)
    for r, cnt in enumerate(counts):
        k = min(cnt, max_len)
        walk = np.concatenate([rng.integers(2, 9, (1, 2)), moves[rng.integers(0, 3, k - 1)]]).cumsum(0)
        cells[r, :k] = walk
        steps = rng.integers(-1, 2, k)
        steps[:3] = (-1, 0, 1)[:k]                          # every row of 3 or more cells turns both ways and holds
        heads[r, :k] = np.cumsum(steps) % 8
        points[r, :k] = cell_centres(walk) + rng.uniform(-0.03, 0.03, (k, 2)).astype(F32)
        ends = cell_centres(walk[[0, -1]]) + F32(RES) * rng.uniform(0.1, 0.4, (2, 2)).astype(F32) * rng.choice(F32([-1, 1]), (2, 2))
        start[r, :2], goal[r, :2] = ends.astype(F32)
    if dim == 3:
        start[:, 2], goal[:, 2] = rng.uniform(-3.3, 3.3, (2, b)).astype(F32)
    return {"cells": cells, "headings": heads, "points": points, "start": start, "goal": goal,
            "count": np.asarray(counts, I32), "status": np.asarray(status, I32)}


def seed_polylines(case):
    """the fp32 polyline start | interior | goal of every row the spline is fitted on (status 0, 1 <= count <= max_len)"""
    s = seed_inputs(case)
    max_len = SEED_SIZES[case[1]][0]
    rows = [r for r in range(len(s["count"])) if s["status"][r] == 0 and 1 <= s["count"][r] <= max_len]
    mid = (lambda r: s["points"][r, :s["count"][r]]) if case[0] == "points" else (lambda r: cell_centres(s["cells"][r, :s["count"][r]]))
    return [np.concatenate([s["start"][r:r + 1, :2], mid(r), s["goal"][r:r + 1, :2]]) for r in rows]


def seed_sites_distinct(case):
    return all(bool(np.all(np.diff(chord_parameter(p)[0]) > 0)) for p in seed_polylines(case))


def run_seed(case, lib=None):
    import torch
    from nfopp import _lib
    lib = lib or _lib.load()
    entry, size, dim, directed = case
    max_len, n, counts, _ = SEED_SIZES[size]
    b = len(counts)
    d = {k: torch.tensor(v, device="cuda") for k, v in seed_inputs(case).items()}
    traj = torch.full((b, n, dim), SENTINEL, dtype=torch.float32, device="cuda")
    ws_bytes = lib.nfopp_grid_seed_workspace_bytes(b, max_len)
    ws = torch.zeros(max(ws_bytes, 8), dtype=torch.uint8, device="cuda")
    P, i32 = _lib.ptr, torch.int32
    tail = (P(traj), P(ws, torch.uint8) if ws_bytes else None, ws_bytes, _lib.stream_ptr())
    head = (P(d["count"], i32), P(d["status"], i32), b, max_len, P(d["start"]), P(d["goal"]), n)
    if entry == "cells":
        rc = lib.nfopp_grid_seed_trajectories(P(d["cells"], i32), *head, dim, directed, OX, OY, RES, *tail)
    elif entry == "points":
        rc = lib.nfopp_grid_seed_polylines(P(d["points"]), *head, dim, directed, *tail)
    else:
        rc = lib.nfopp_lattice_seed_trajectories(P(d["cells"], i32), P(d["headings"], i32), *head, OX, OY, RES, *tail)
    assert rc == 0, lib.nfopp_last_error()
    torch.cuda.synchronize()
    return {"traj": traj.cpu().numpy()}


# ---- the golden file --------------------------------------------------------------------------------------------------
def words(a):
    """the integer view the comparisons are made on: uint32 of fp32, uint64 of float64, int32 as it is"""
    a = np.ascontiguousarray(a)
    return a.view({np.dtype(F32): np.uint32, np.dtype(np.float64): np.uint64, np.dtype(I32): I32}[a.dtype])


def run_cases(lib=None):
    """{"post_<name>_<array>" / "seed_<tag>_<array>": array}: the arrays of tests/golden/spline_bits.npz"""
    res = {"post_%s_%s" % (name, k): v for name in POST_CASES for k, v in run_post(name, lib).items()}
    res.update({"seed_%s_%s" % (seed_tag(c), k): v for c in SEED_CASES for k, v in run_seed(c, lib).items()})
    return res
