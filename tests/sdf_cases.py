"""The grids, robots and poses of the distance-field tests (tests/test_sdf_field_cpu.py, tests/test_gpu_sdf_field.py).
Everything is generated from fixed seeds; nothing here needs a device."""
import collections

import numpy as np

import sdf_ref as ref

F32 = np.float32

Grid = collections.namedtuple("Grid", "occupancy boundaries resolution")


def make_grid(occupancy, origin, resolution):
    occ = np.ascontiguousarray(np.asarray(occupancy) != 0, dtype=np.uint8)
    rows, cols = occ.shape
    x0, y0 = origin
    return Grid(occ, (x0, x0 + cols * resolution, y0, y0 + rows * resolution), resolution)


def random_blocks(rows, cols, n_blocks, seed):
    """`n_blocks` axis-aligned wall blocks of 1 .. 1/4 of each side, placed at random."""
    rng = np.random.default_rng(seed)
    occ = np.zeros((rows, cols), np.uint8)
    for _ in range(n_blocks):
        h, w = rng.integers(1, max(rows // 4, 1) + 1), rng.integers(1, max(cols // 4, 1) + 1)
        r, c = rng.integers(0, rows - h + 1), rng.integers(0, cols - w + 1)
        occ[r:r + h, c:c + w] = 1
    return occ


# ---- the images whose signed distance is pinned bit for bit --------------------------------------------------------------------
FIELD_GRIDS = {
    "2x2": make_grid([[0, 1], [0, 0]], (0.0, 0.0), 0.5),
    "2x9": make_grid([[0, 0, 1, 0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 1, 0, 0, 0, 0]], (-1.0, 2.0), 0.3),
    "37x53": make_grid(random_blocks(37, 53, 9, 1), (-1.3, 0.7), 0.1),
    "no_walls": make_grid(np.zeros((5, 7), np.uint8), (0.0, 0.0), 0.25),
    "all_walls": make_grid(np.ones((6, 4), np.uint8), (1.0, -1.0), 0.2),
}

THREE_DISCS = [(-0.2, 0.0, 0.15), (0.0, 0.0, 0.15), (0.25, 0.05, 0.15)]


def field_of(grid, discs, margin=0.05, gain=10.0, border=False):
    return ref.make_field(ref.signed_distance(grid.occupancy, grid.resolution, border), grid.boundaries, grid.resolution,
                          discs, margin, gain)


def random_poses(grid, count, seed, outside=0.5, dim=3):
    """fp32 [count, dim] uniform over the grid's box grown by `outside` metres, headings over (-pi, pi)."""
    rng = np.random.default_rng(seed)
    b = grid.boundaries
    cols = [rng.uniform(b[0] - outside, b[1] + outside, count), rng.uniform(b[2] - outside, b[3] + outside, count),
            rng.uniform(-np.pi, np.pi, count)]
    return np.stack(cols[:dim], 1).astype(F32)


# ---- the cases held against float64 (three-disc robots: numpy's sine and the device's may differ in the last place) ---------
# name -> (grid, discs, margin, gain, border, poses).  The share of poses at which the float32 and the float64 restatement take
# a different branch may be at most 2 % in each of them (tests/test_sdf_field_cpu.py asserts it).
def _box_robot():
    # DistanceField.discs_for_box((-0.3, 0.5, -0.12, 0.12), 5), written out: the cases must not need the package
    part, width = 0.8 / 5, 0.24
    return [(-0.3 + (k + 0.5) * part, 0.0, 0.5 * float(np.hypot(part, width))) for k in range(5)]


F64_CASES = {
    "trial": (FIELD_GRIDS["37x53"], THREE_DISCS, 0.05, 10.0, False, random_poses(FIELD_GRIDS["37x53"], 4096, 2)),
    "box_border": (make_grid(random_blocks(24, 31, 6, 3), (2.0, -3.0), 0.25), _box_robot(), 0.0, 4.0, True,
                   random_poses(make_grid(np.zeros((24, 31)), (2.0, -3.0), 0.25), 1000, 4, outside=0.8)),
}
MAX_EXCLUDED_SHARE = 0.02


# ---- explicit poses without trigonometry -----------------------------------------------------------------------------------------
def edge_poses(grid, dim):
    """Poses on grid nodes, exactly on u = 0 and u = cols - 1 (v likewise), outside on each side and corner, and with
    non-finite components.  -> (poses fp32 [P, dim], outside_x bool [P], outside_y bool [P], bad bool [P]): whether the pose
    lies at or beyond the first / last node along x / y (its gradient component there is exactly 0), and whether a component
    is not finite (four NaNs).  `first` and `last` are exact only on a grid whose frame is (exact_frame_grid)."""
    rows, cols = grid.occupancy.shape
    res, (bx0, _, by0, _) = grid.resolution, grid.boundaries
    node_x = lambda i: bx0 + (i + 0.5) * res      # noqa: E731
    node_y = lambda j: by0 + (j + 0.5) * res      # noqa: E731
    xs = {"node": node_x(min(1, cols - 1)), "first": node_x(0), "last": node_x(cols - 1), "below": bx0 - 0.37, "above": node_x(cols - 1) + 0.41,
          "mid": bx0 + 0.5 * cols * res + 0.013}
    ys = {"node": node_y(min(1, rows - 1)), "first": node_y(0), "last": node_y(rows - 1), "below": by0 - 0.29, "above": node_y(rows - 1) + 0.33,
          "mid": by0 + 0.5 * rows * res - 0.017}
    poses, out_x, out_y = [], [], []
    for kx, x in xs.items():
        for ky, y in ys.items():
            poses.append((x, y, 0.7))
            out_x.append(kx in ("first", "last", "below", "above"))
            out_y.append(ky in ("first", "last", "below", "above"))
    n_good = len(poses)
    for bad in (np.nan, np.inf, -np.inf):
        for comp in range(dim):
            p = [xs["mid"], ys["mid"], -1.1]
            p[comp] = bad
            poses.append(tuple(p))
    poses = np.asarray(poses, np.float64)[:, :dim].astype(F32)
    bad = np.arange(len(poses)) >= n_good
    pad = np.zeros(len(poses) - n_good, bool)
    return poses, np.concatenate([out_x, pad]), np.concatenate([out_y, pad]), bad


def exact_frame_grid():
    """A grid whose frame is exact in fp32 (resolution 0.25, origin (1, -2)): a pose written as x0 + (i + 0.5) * res lies on
    node i exactly, so `first` / `last` of edge_poses hit u = 0 and u = cols - 1 to the bit."""
    return make_grid(random_blocks(9, 12, 4, 5), (1.0, -2.0), 0.25)


POINT_COUNTS = (1, 63, 64, 65, 257)


def point_poses(grid, count, dim, seed=6):
    """`count` poses: the edge poses first (as many as fit), random ones behind them."""
    edge = edge_poses(grid, dim)[0]
    rnd = random_poses(grid, count, seed, dim=dim)
    return np.concatenate([edge, rnd])[:count] if count >= len(edge) else np.concatenate([rnd[:count - 1], edge[-1:]])[:count]


# ---- a tie between two discs -----------------------------------------------------------------------------------------------------
def tie_case():
    """A field symmetric about the line y = 1 (walls in the first and last row of 8, resolution 0.25: every value a multiple of
    0.25) and two discs mirrored about the body's x axis at heading 0 (cos = 1 and sin = 0 exactly on every implementation).
    Both discs see the distance 0.5625 exactly, so their penetrations tie; their y gradients are opposite.  -> (grid, discs, poses, gain)."""
    occ = np.zeros((8, 6), np.uint8)
    occ[0] = occ[7] = 1
    return make_grid(occ, (0.0, 0.0), 0.25), [(0.0, -0.3125, 0.125), (0.0, 0.3125, 0.125)], \
        np.asarray([[0.7, 1.0, 0.0], [0.55, 1.0, 0.0]], F32), 2.0


# ---- behaviour: straight seeds through a wall end up in its gap -----------------------------------------------------------------
BEHAVIOUR_STEPS = 100      # what the GPU test runs; the restated pipeline first passes at BEHAVIOUR_FIRST_PASS
BEHAVIOUR_FIRST_PASS = 23


def behaviour_case():
    """A 32 x 32 map at 0.1 m with a wall four cells thick across it and a gap of eight cells, eight SE(2) problems whose
    straight seeds cross the wall beside the gap, one disc of 0.1 m with a 0.1 m margin.
    -> dict(grid, discs, margin, gain, hyper (keyword arguments of orc.Hyper), starts, goals, n_waypoints, reparam_freq, draws):
    draws fp32 [BEHAVIOUR_STEPS, 8, 31] are the interpolation parameters injected into every step, on the CPU and on the GPU."""
    occ = np.zeros((32, 32), np.uint8)
    occ[:, 14:18] = 1
    occ[12:20, 14:18] = 0
    grid = make_grid(occ, (0.0, 0.0), 0.1)
    # the crossings lie within 0.15 m of the gap (y in 1.2 .. 2.0): inside a wall the field's gradient points to the nearest
    # free cell, so a seed that crosses further from the gap is pushed along the wall's normal and stays (the local minimum
    # every distance-field optimiser has; a grid seeder is the cure, not the collision term)
    ys = np.asarray([1.05, 1.08, 1.11, 1.14, 2.06, 2.09, 2.12, 2.15])
    zeros = np.zeros(8)
    starts = np.stack([np.full(8, 0.45), ys - 0.05, zeros], 1).astype(F32)
    goals = np.stack([np.full(8, 2.75), ys + 0.05, zeros], 1).astype(F32)
    hyper = dict(collision_weight=20.0, collision_beta=2.0, direction_delta_weight=1.0, lr=1e-2, bounds=grid.boundaries)
    draws = np.random.default_rng(8).uniform(0, 1, (BEHAVIOUR_STEPS, 8, 31)).astype(F32)
    return dict(grid=grid, discs=[(0.0, 0.0, 0.1)], margin=0.1, gain=10.0, hyper=hyper, starts=starts, goals=goals,
                n_waypoints=32, reparam_freq=10, draws=draws)


# ---- trajectory mode -------------------------------------------------------------------------------------------------------------
TRAJ_SHAPES = ((3, 5), (1, 2), (2, 65), (2, 66))


def random_trajectories(grid, batch, n, dim, seed=7):
    rng = np.random.default_rng(seed)
    b = grid.boundaries
    tr = np.stack([rng.uniform(b[0] - 0.2, b[1] + 0.2, (batch, n)), rng.uniform(b[2] - 0.2, b[3] + 0.2, (batch, n)),
                   rng.uniform(-3.5, 3.5, (batch, n))], 2)
    return np.ascontiguousarray(tr[..., :dim]).astype(F32)
