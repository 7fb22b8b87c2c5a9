#!/usr/bin/env python3
"""Generate tests/golden/g21_obstacle_map.npz from the reference's GridMap (ros/grid_map.py), CircleDirectedCollisionChecker
and RectangleCollisionChecker (collision_checker/*.py), all float64 numpy.

Needs the reference checkout (NFOPP_REFERENCE), imported unmodified through make_golden.py's shims (Position2 needs
scipy).  Only inputs and the numbers the reference computed from them are written.

Maps (`<m>_data`, `<m>_resolution`, `<m>_origin` = x, y, theta; `<m>_cloud` float64 = GridMap.as_point_cloud(),
`<m>_bounds` = GridMap.boundaries):
    a  37 x 53 fp32, origin (-1.25, 0.5, 0), resolution 0.1; cells at exactly 0.5 (free) and one fp32 step above it
    b  the same image, origin angle 0.3
    c  64 x 64 raw int8 ROS image holding -1, 0, 50, 51 and 100 (unpacked as from_ros_occupancy_grid does)
    d  an empty 37 x 53 map            e  a full 5 x 7 map of resolution 0.25
Labels, per map and checker k in circle (radius 0.3), recta (box -0.34, 0.4, -0.27, 0.27), rectb (0.1, 0.5, -0.2, 0.2):
    <m>_poses [4000, 3] fp32 (evaluated by the reference as float64), uniform over the map's bounds grown by 0.3 m (map e: 0.5 m)
    <m>_<k>_before   labels of a checker without boundaries that was given the map's cloud
    <m>_<k>_after    labels after one sensor message (CollisionCheckerAdapter._callback): points = [<m>_extra (25 sensor
                     points), cloud], boundaries = the map's
    <m>_<k>_keep     poses whose float64 margin to every decision boundary of BOTH states is at least 1e-4 m: |d - r| to
                     every point (circle), the distance of every robot-frame point to every edge of the box (rectangle),
                     |x - bound| to the four boundaries.  fp32 evaluation at these coordinates errs by about 1e-5 m, so
                     a device checker must reproduce the kept labels with no exception.
The generator asserts that the filter drops under 1 % of the poses and that each label class holds at least 20 % of the
kept ones -- except where the map leaves one class empty by construction: `d` before the message (no obstacle, no
boundary: every pose free) and `e` after it (every pose inside the boundaries is within reach of an occupied cell and
every pose outside them collides).

Usage:  MPLBACKEND=Agg python tests/golden/make_golden_obstacles.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (installs the shims and the reference's path)
from make_golden import CircleDirectedCollisionChecker, F32, Position2, RectangleCollisionChecker  # noqa: E402
from neural_field_optimal_planner.ros.grid_map import GridMap  # noqa: E402

MARGIN = 1e-4
N_POSES = 4000
CHECKERS = (("circle", 0.3), ("recta", (-0.34, 0.4, -0.27, 0.27)), ("rectb", (0.1, 0.5, -0.2, 0.2)))
DEGENERATE = {("d", "before"), ("e", "after")}


def blobs(rng, rows, cols, count, lo, hi):
    mask = np.zeros((rows, cols), bool)
    for _ in range(count):
        h, w = rng.integers(lo, hi, 2)
        r, c = rng.integers(0, rows - h), rng.integers(0, cols - w)
        mask[r:r + h, c:c + w] = True
    return mask


def fp32_image(rng):
    mask = blobs(rng, 37, 53, 20, 2, 6)
    img = np.where(mask, rng.uniform(0.5, 1.0, mask.shape), rng.uniform(0.0, 0.5, mask.shape)).astype(F32)
    img[mask & (img <= 0.5)] = F32(0.75)
    img[~mask & (img >= 0.5)] = F32(0.25)
    occupied = np.argwhere(mask)
    img[tuple(occupied[0])] = np.nextafter(F32(0.5), F32(1))      # just above the threshold: occupied
    free = np.argwhere(~mask)
    img[tuple(free[0])] = F32(0.5)                                 # exactly the threshold: free
    img[36, 52] = F32(0.9)                                         # the last cell
    return img


def ros_image(rng):
    img = np.zeros((64, 64), np.int8)
    img[blobs(rng, 64, 64, 6, 3, 9)] = -1
    img[blobs(rng, 64, 64, 24, 2, 7)] = 100
    img[blobs(rng, 64, 64, 10, 2, 6)] = 51
    img[blobs(rng, 64, 64, 5, 2, 6)] = 50                          # 0.5: not above the threshold
    assert set(np.unique(img)) == {-1, 0, 50, 51, 100}
    return img


def unpack_ros(img):
    """The array from_ros_occupancy_grid (grid_map.py:31-40) hands to GridMap, from message.data's values."""
    data = np.array([int(v) for v in img.reshape(-1)]).reshape(img.shape)
    data = np.where(data == -1, 0, data)
    return data.astype(np.float32) / 100


def circle_margin(poses, points, radius):
    if len(points) == 0:
        return np.full(len(poses), np.inf)
    d = np.linalg.norm(poses[:, None, :2] - points[None], axis=2)
    return np.abs(d - radius).min(1)


def rectangle_margin(poses, points, box):
    """Smallest distance of a robot-frame obstacle point to an edge (segment) of the box."""
    if len(points) == 0:
        return np.full(len(poses), np.inf)
    dx, dy = points[None, :, 0] - poses[:, None, 0], points[None, :, 1] - poses[:, None, 1]
    c, s = np.cos(poses[:, 2])[:, None], np.sin(poses[:, 2])[:, None]
    rx, ry = c * dx + s * dy, c * dy - s * dx
    x0, x1, y0, y1 = box
    ox, oy = np.maximum(np.maximum(x0 - rx, rx - x1), 0), np.maximum(np.maximum(y0 - ry, ry - y1), 0)
    outside = np.hypot(ox, oy)
    inside = np.minimum(np.minimum(rx - x0, x1 - rx), np.minimum(ry - y0, y1 - ry))
    return np.where(inside > 0, inside, outside).min(1)


def bounds_margin(poses, bounds):
    return np.minimum(np.abs(poses[:, 0:1] - np.asarray(bounds[:2])[None]).min(1),
                      np.abs(poses[:, 1:2] - np.asarray(bounds[2:])[None]).min(1))


def labels_of(checker, poses):
    return np.asarray(checker.check_collision(Position2.from_vec(poses))).astype(np.uint8)


def main():
    rng = np.random.default_rng(2100)
    image = fp32_image(rng)
    ros = ros_image(rng)
    # image, resolution, origin, metres the pose region extends beyond the map's boundaries
    maps = dict(a=(image, 0.1, (-1.25, 0.5, 0.0), 0.3), b=(image, 0.1, (-1.25, 0.5, 0.3), 0.3),
                c=(ros, 0.1, (0.4, -2.0, 0.0), 0.3), d=(np.zeros((37, 53), F32), 0.1, (-1.25, 0.5, 0.0), 0.3),
                e=(np.ones((5, 7), F32), 0.25, (2.0, 1.0, 0.0), 0.5))
    out = {}
    for m, (data, resolution, origin, grow) in maps.items():
        grid = GridMap(unpack_ros(data) if data.dtype == np.int8 else data, resolution, Position2(*origin))
        cloud = np.asarray(grid.as_point_cloud(), np.float64).reshape(-1, 2)
        bounds = tuple(float(v) for v in grid.boundaries)
        out[m + "_data"], out[m + "_resolution"], out[m + "_origin"] = data, np.float64(resolution), np.asarray(origin, np.float64)
        out[m + "_cloud"], out[m + "_bounds"] = cloud, np.asarray(bounds, np.float64)
        lo, hi = np.array([bounds[0], bounds[2]]) - grow, np.array([bounds[1], bounds[3]]) + grow
        extra = rng.uniform(lo + grow, hi - grow, (25, 2))
        poses = np.concatenate([rng.uniform(lo, hi, (N_POSES, 2)), rng.uniform(-np.pi, np.pi, (N_POSES, 1))], 1).astype(F32)
        out[m + "_extra"], out[m + "_poses"] = extra, poses
        p64 = poses.astype(np.float64)
        updated = np.concatenate([extra, cloud], axis=0)
        print("map %s: %d x %d, %d occupied cells" % ((m,) + data.shape + (len(cloud),)))
        for name, shape in CHECKERS:
            if name == "circle":
                checker = CircleDirectedCollisionChecker(shape, None)
                margin = np.minimum(circle_margin(p64, cloud, shape), circle_margin(p64, updated, shape))
            else:
                checker = RectangleCollisionChecker(shape, None)
                margin = np.minimum(rectangle_margin(p64, cloud, shape), rectangle_margin(p64, updated, shape))
            checker.update_obstacle_points(cloud)
            before = labels_of(checker, p64)
            checker.update_obstacle_points(updated)
            checker.update_boundaries(bounds)
            assert checker.get_boundaries() == bounds
            after = labels_of(checker, p64)
            keep = np.minimum(margin, bounds_margin(p64, bounds)) >= MARGIN
            assert (~keep).mean() < 0.01, (m, name, (~keep).mean())
            for phase, lab in (("before", before), ("after", after)):
                hit = lab[keep].mean()
                print("  %-6s %-6s kept %4d  in collision %.3f" % (name, phase, keep.sum(), hit))
                if (m, phase) in DEGENERATE:
                    assert hit in (0.0, 1.0) or m == "e", (m, name, phase, hit)
                else:
                    assert 0.2 <= hit <= 0.8, (m, name, phase, hit)
                out["%s_%s_%s" % (m, name, phase)] = lab
            assert (before[keep] != after[keep]).any()
            out["%s_%s_keep" % (m, name)] = keep
    for k, v in out.items():
        assert v.dtype != object, k
    path = os.path.join(HERE, "g21_obstacle_map.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
