"""The slices, frames and poses of the heading-layered distance field tests (tests/test_heading_field_cpu.py,
tests/test_gpu_heading_field.py).  Everything is made on the CPU from fixed seeds and handed to the device as explicit
`layers`: no device sine stands between the restatement and the kernel."""
import collections

import numpy as np

import heading_field_ref as ref
import obstacle_map_ref as omr
import sdf_cases as sc

F32 = np.float32

Layers = collections.namedtuple("Layers", "occupancy boundaries resolution")    # occupancy uint8 [L, rows, cols]


def make_layers(occupancy, origin, resolution):
    occ = np.ascontiguousarray(np.asarray(occupancy) != 0, dtype=np.uint8)
    _, rows, cols = occ.shape
    x0, y0 = origin
    return Layers(occ, (x0, x0 + cols * resolution, y0, y0 + rows * resolution), resolution)


def random_layers(n_layers, rows, cols, seed, empty=None, full=None):
    """Random wall blocks per slice (sdf_cases.random_blocks); slice `empty` has no blocked cell and slice `full` no free one."""
    occ = np.stack([sc.random_blocks(rows, cols, 5, seed * 100 + k) for k in range(n_layers)])
    if empty is not None:
        occ[empty] = 0
    if full is not None:
        occ[full] = 1
    return occ


def box_layers(occupancy, resolution, box, n_layers, origin=(0.0, 0.0)):
    """The footprint slices of a box robot on one occupancy image: obstacle_map_ref.rectangle_labels at every cell centre and
    every slice heading float32(k * 2 pi / L), the obstacle points being the centres of the occupied cells."""
    occ = np.asarray(occupancy) != 0
    rows, cols = occ.shape
    points = omr.grid_points(occ.astype(F32), resolution, (origin[0], origin[1], 0.0))
    j, i = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    x = (i.reshape(-1) * resolution + resolution / 2 + origin[0]).astype(F32)
    y = (j.reshape(-1) * resolution + resolution / 2 + origin[1]).astype(F32)
    out = np.empty((n_layers, rows, cols), np.uint8)
    for k, th in enumerate(ref.slice_headings(n_layers)):
        poses = np.stack([x, y, np.full(len(x), th, F32)], 1)
        out[k] = omr.rectangle_labels(poses, points, box).reshape(rows, cols)
    return out


# ---- the images pinned bit for bit: (L, rows, cols) with one slice without a blocked cell and one fully blocked --------------
FIELD_LAYERS = {
    "2x2x2": make_layers(random_layers(2, 2, 2, 1, empty=0, full=1), (0.0, 0.0), 0.5),
    "3x2x9": make_layers(random_layers(3, 2, 9, 2, empty=2, full=0), (-1.0, 2.0), 0.3),
    "16x37x53": make_layers(random_layers(16, 37, 53, 3, empty=5, full=11), (-1.3, 0.7), 0.1),
    "64x9x12": make_layers(random_layers(64, 9, 12, 4, empty=63, full=0), (1.0, -2.0), 0.25),     # sdf_cases.exact_frame_grid's frame
}
EXACT_FRAME = "64x9x12"    # resolution 0.25, origin (1, -2): x0 + (i + 0.5) * res lies on node i to the bit


def field_of(layers, margin=0.05, gain=10.0, border=False):
    return ref.make_field(layers.occupancy, layers.boundaries, layers.resolution, margin, gain, border)


# ---- headings ------------------------------------------------------------------------------------------------------------------
HEADING_LAYER_COUNTS = (2, 3, 16, 64)


def heading_list(n_layers):
    """fp32 headings at which the slice index is delicate: zeros, half and whole turns, large and huge arguments, the largest
    finite float, denormals, and every slice heading float32(k * 2 pi / L) with both of its float32 neighbours."""
    big = np.finfo(F32).max
    fixed = [0.0, -0.0, np.pi, -np.pi, -2 * np.pi, 7.5 * np.pi, 1e6, 3e7, big, -big, 1e-45, -1e-45, 1e-39, -1e-39]
    out = [F32(v) for v in fixed]
    for h in ref.slice_headings(n_layers):
        out += [np.nextafter(h, F32(-np.inf)), h, np.nextafter(h, F32(np.inf))]
    return np.asarray(out, F32)


def heading_poses(layers, seed=21):
    """The heading list of the field's own L at random positions inside the grid."""
    th = heading_list(layers.occupancy.shape[0])
    xy = sc.random_poses(sc.Grid(layers.occupancy[0], layers.boundaries, layers.resolution), len(th), seed, outside=0.0)[:, :2]
    return np.concatenate([xy, th[:, None]], 1).astype(F32)


def edge_poses(layers):
    """sdf_cases.edge_poses on the layered grid's frame (SE(2))."""
    return sc.edge_poses(sc.Grid(layers.occupancy[0], layers.boundaries, layers.resolution), 3)


def random_poses(layers, count, seed, outside=0.5):
    """fp32 [count, 3] over the grid's box grown by `outside` metres, headings over (-3 pi, 3 pi): negative and wrapped ones."""
    p = sc.random_poses(sc.Grid(layers.occupancy[0], layers.boundaries, layers.resolution), count, seed, outside)
    p[:, 2] *= F32(3)
    return p


POINT_COUNTS = (1, 63, 64, 65, 257)


def point_poses(layers, count, seed=6):
    """`count` poses from the pool (edge poses, the heading list, random ones), a non-finite one always among them."""
    edge, heads = edge_poses(layers)[0], heading_poses(layers)
    pool = np.concatenate([edge[-9:], heads[:14], edge[:-9], heads[14:], random_poses(layers, count, seed)])
    return pool[:count]


def coverage_poses():
    """(layers, poses): every explicit pose the GPU tests evaluate on the exact frame."""
    layers = FIELD_LAYERS[EXACT_FRAME]
    return layers, np.concatenate([edge_poses(layers)[0], heading_poses(layers), random_poses(layers, 257, 6)])


# ---- the hand case: a box in a gap the disc cover does not fit ----------------------------------------------------------------
HAND_BOX = (-1.0, 1.0, -0.25, 0.25)
HAND_LAYERS = 16
HAND_FREE = (2.0, 1.95, 0.0)                                  # in the gap's centre, heading along the passage
HAND_BLOCKED = ((2.0, 1.95, np.pi / 2), (2.0, 2.05, 0.0))     # across the passage; one cell off the centre line
HAND_BETWEEN = (2.0, 1.95, 0.2)                               # the model's limit: free by the checker, d < 0 by interpolation


def hand_map():
    """40 x 40 cells at 0.1 m: a wall 0.4 m thick across x = 2 with a gap of five cells around y = 1.95."""
    occ = np.zeros((40, 40), np.uint8)
    occ[:, 18:22] = 1
    occ[17:22, 18:22] = 0
    return sc.make_grid(occ, (0.0, 0.0), 0.1)


def hand_case():
    """-> (grid, layers): the map and the 16 footprint slices of the 2 m x 0.5 m box on it."""
    g = hand_map()
    return g, make_layers(box_layers(g.occupancy, g.resolution, HAND_BOX, HAND_LAYERS), (0.0, 0.0), g.resolution)


# ---- behaviour: straight seeds through a wall end up in its gap, for a box ---------------------------------------------------
BEHAVIOUR_BOX = (-0.5, 0.5, -0.25, 0.25)
BEHAVIOUR_LAYERS = 32
BEHAVIOUR_STEPS = 200       # what the GPU test runs
BEHAVIOUR_FIRST_PASS = 37   # the first step from which every path is free by rectangle_labels at every later step up to 200:
                            # found with the first choice of margin (0.1), gain (10) and sdf_cases.behaviour_case's weights


def behaviour_case():
    """The map of sdf_cases.behaviour_case (32 x 32 at 0.1 m, a wall four cells thick, a gap of eight cells) with the 1 m x 0.5 m
    box, 32 slices from rectangle_labels, and its eight SE(2) problems whose straight seeds cross the wall beside the gap.
    -> dict(grid, layers, box, points, margin, gain, hyper, starts, goals, n_waypoints, reparam_freq, draws)."""
    base = sc.behaviour_case()
    g = base["grid"]
    layers = make_layers(box_layers(g.occupancy, g.resolution, BEHAVIOUR_BOX, BEHAVIOUR_LAYERS), (0.0, 0.0), g.resolution)
    points = omr.grid_points(g.occupancy.astype(F32), g.resolution, (0.0, 0.0, 0.0))
    draws = np.random.default_rng(8).uniform(0, 1, (BEHAVIOUR_STEPS, 8, 31)).astype(F32)
    return dict(grid=g, layers=layers, box=BEHAVIOUR_BOX, points=points, margin=0.1, gain=10.0, hyper=base["hyper"],
                starts=base["starts"], goals=base["goals"], n_waypoints=base["n_waypoints"], reparam_freq=base["reparam_freq"],
                draws=draws)


# ---- trajectory mode -------------------------------------------------------------------------------------------------------------
TRAJ_SHAPES = sc.TRAJ_SHAPES


def random_trajectories(layers, batch, n, seed=7):
    return sc.random_trajectories(sc.Grid(layers.occupancy[0], layers.boundaries, layers.resolution), batch, n, 3, seed)
