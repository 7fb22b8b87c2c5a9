#!/usr/bin/env python3
"""Device-event timings of the obstacle update on one GPU (the figures of profiles/obstacle_map.txt and DESIGN.md 11):
the brute-force rectangle kernel against the cell-indexed one at cfg5's 2.54 M poses per fit, on the cloud of a 64 x 64
and of a 384 x 384 occupancy grid; the two build steps (grid -> points, cell index); and the obstacle count from which
the indexed rectangle kernel wins (DeviceRectangleChecker.INDEX_FROM).

Usage:  python tools/obstacle_map_timing.py [--poses 2540000] [--parent-lib path/to/an/older/libnfopp_hip.so]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import nfopp  # noqa: E402
from nfopp import _lib  # noqa: E402

BOX = (-0.34, 0.4, -0.27, 0.27)


def timed(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def blob_map(rng, side, blobs, lo, hi):
    img = np.zeros((side, side), np.float32)
    for _ in range(blobs):
        h, w = rng.integers(lo, hi, 2)
        r, c = rng.integers(0, side - h), rng.integers(0, side - w)
        img[r:r + h, c:c + w] = 1.0
    return img


def parent_rectangle(path):
    lib = ctypes.CDLL(path)
    fn = lib.nfopp_check_collision_rectangle
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_float),
                   ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=2540000)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    print("device: %s, poses per call: %d, box %s (median / min / max of 10 event-timed calls, ms)"
          % (torch.cuda.get_device_name(0), args.poses, BOX))
    parent = parent_rectangle(args.parent_lib) if args.parent_lib else None
    maps = {"64x64": blob_map(rng, 64, 30, 2, 7), "384x384": blob_map(rng, 384, 420, 3, 8)}
    clouds = {}
    for name, img in maps.items():
        side = img.shape[0]
        data = torch.tensor(img, device="cuda")

        def to_points():
            grid = nfopp.DeviceGridMap(data, 0.1, (0.0, 0.0, 0.3))
            return grid.as_point_cloud()
        cloud = to_points()
        clouds[name] = cloud
        n = cloud.shape[0]
        # the two launches of the map -> points step without the host read of the count in between
        lib = _lib.load()
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        p32, p64 = torch.empty(n, 2, device="cuda"), torch.empty(n, 2, dtype=torch.float64, device="cuda")
        t = timed(lambda: _lib.check(lib.nfopp_grid_to_points(_lib.ptr(data), 0, side, side, 0.5, 0.1, 0.0, 0.0, float(np.cos(0.3)),
                                                              float(np.sin(0.3)), n, _lib.ptr(p32), _lib.ptr(p64, torch.float64),
                                                              _lib.ptr(count, torch.int32), _lib.stream_ptr())))
        print("grid_to_points      %-8s %6d occupied of %6d cells: %8.4f / %8.4f / %8.4f" % ((name, n, side * side) + t))
        checker = nfopp.DeviceRectangleChecker(np.zeros((0, 2)), BOX)
        checker.INDEX_FROM = 1
        t = timed(lambda: checker.update_obstacle_points(cloud))
        print("update_obstacle_points (min/max, build_cell_index, one host sync) %-8s n = %6d: %8.4f / %8.4f / %8.4f"
              % ((name, n) + t))
        start, nx, ny, x0, y0, size = checker.cells
        nbytes = lib.nfopp_cell_index_workspace_bytes(n)
        work, ordered = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty_like(cloud)
        t = timed(lambda: _lib.check(lib.nfopp_build_cell_index(_lib.ptr(cloud), n, x0, y0, size, nx, ny, _lib.ptr(ordered),
                                                                _lib.ptr(start, torch.int32), _lib.ptr(work, torch.uint8),
                                                                nbytes, _lib.stream_ptr())))
        print("build_cell_index    %-8s n = %6d, %d x %d cells of %.3f m: %8.4f / %8.4f / %8.4f" % ((name, n, nx, ny, size) + t))

    def poses_over(cloud):
        lo, hi = cloud.min(0).values.cpu().numpy() - 0.5, cloud.max(0).values.cpu().numpy() + 0.5
        xy = rng.uniform(lo, hi, (args.poses, 2))
        return torch.tensor(np.concatenate([xy, rng.uniform(-np.pi, np.pi, (args.poses, 1))], 1).astype(np.float32), device="cuda")

    def compare(tag, points, poses):
        out = torch.empty(poses.shape[0], device="cuda")
        fast = nfopp.DeviceRectangleChecker(np.zeros((0, 2)), BOX)
        fast.INDEX_FROM = 1
        fast.update_obstacle_points(points)
        slow = nfopp.DeviceRectangleChecker(np.zeros((0, 2)), BOX)
        slow.INDEX_FROM = 1 << 30
        slow.update_obstacle_points(points)
        assert fast.cells is not None and slow.cells is None
        a = fast.labels(poses).clone()
        assert torch.equal(a, slow.labels(poses)), "the two kernels disagree"
        tf, ts = timed(lambda: fast.labels(poses, out=out)), timed(lambda: slow.labels(poses, out=out))
        line = "%-22s n = %6d  in collision %.3f  brute force %9.4f / %9.4f / %9.4f   indexed %8.4f / %8.4f / %8.4f" \
            % ((tag, points.shape[0], float(a.mean())) + ts + tf)
        if parent is not None:
            box = (ctypes.c_float * 4)(*BOX)
            tp = timed(lambda: parent(poses.data_ptr(), poses.shape[0], slow.obstacles.data_ptr(), points.shape[0], box, None,
                                      out.data_ptr(), _lib.stream_ptr()))
            assert torch.equal(out, a), "the parent's brute-force kernel disagrees"
            line += "   parent brute force %9.4f / %9.4f / %9.4f" % tp
        print(line)
        return tf[0], ts[0]

    for name, cloud in clouds.items():
        compare("rectangle " + name, cloud, poses_over(cloud))
    cloud = clouds["64x64"]
    poses = poses_over(cloud)
    print("crossover on subsets of the 64x64 cloud (same poses):")
    first = None
    for n in (1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 128, 256):
        pick = torch.tensor(rng.choice(cloud.shape[0], n, replace=False), device="cuda")
        tf, ts = compare("  subset", cloud[pick].contiguous(), poses)
        if first is None and tf < ts:
            first = n
    print("the indexed kernel is first faster at n = %s" % first)


if __name__ == "__main__":
    main()
