"""Heading-aware lattice search for car-like trajectory seeds (csrc/lattice_search.hip; the rule: include/nfopp_hip.h).

The state of the search is (cell, heading), heading h in 0 .. 7 standing for h * pi / 4; moves are forward only, along the
heading the robot has after the move, which differs from the one before by at most one step.  A seed therefore leaves the
start along the start heading and reaches the goal along the goal heading, and with eight occupancy layers
(`LatticeGrid.from_checker`) it threads only the gaps the robot fits through at the heading it has there.  The traced cells
go through the seeding stage of the 8-connected search (`seed_trajectories`) unchanged.

The `lattice_gear_*` functions (csrc/lattice_gears.hip) search (cell, heading, gear) states: a reverse move backs along the
heading the robot had before it, `reverse_cost` is charged per reverse move and `cusp_cost` per gear change.  Their seeds go
through `seed_lattice_trajectories`, which takes theta from the headings of the lattice states, so a reverse run keeps the
body heading it is driven at."""

import numpy as np
import torch

from . import _lib
from ._grid import (GridFrame, as_device_points, cell_centres, cell_keys, checker_boundaries, checker_device, goal_table, heading_poses,
                    int32_on, seed_launch, traced_search, workspace)
from .grid_search import seed_trajectories

HEADINGS = 8
GOAL_HEADING_MODES = ("fixed", "free")


def heading_index(theta):
    """theta (radians, any float tensor) -> int32 heading index: round(theta / (pi / 4)) in float64 with torch's
    half-to-even, then mod 8; -1 (which the search refuses with status 2) where theta is not finite."""
    t = theta.double()
    idx = torch.remainder(torch.round(t / (np.pi / 4)), HEADINGS)
    return torch.where(torch.isfinite(t), idx, torch.full_like(idx, -1.0)).to(torch.int32)


class LatticeGrid(GridFrame):
    """uint8 occupancy layers [L, rows = y cells, cols = x cells] with L = 1 or 8 (non-zero = blocked; state (cell, h) reads
    layer h mod L) and the geometry of OccupancyGrid (GridFrame: `cells_of`, `cell_centres`)."""

    def __init__(self, layers, boundaries, resolution, device="cuda"):
        if torch.is_tensor(layers) and not layers.is_cuda:
            layers = layers.numpy()
        if torch.is_tensor(layers):
            if layers.dtype != torch.uint8:
                raise ValueError("layers must be uint8")
            host, dev_layers = None, layers
            shape = tuple(layers.shape)
        else:
            host = np.ascontiguousarray(np.asarray(layers) != 0, dtype=np.uint8)
            dev_layers, shape = None, host.shape
        if len(shape) != 3 or shape[0] not in (1, HEADINGS) or shape[1] < 1 or shape[2] < 1:
            raise ValueError("layers must be a non-empty [L, rows, cols] array with L = 1 or 8")
        GridFrame.__init__(self, boundaries, resolution, four_sides=True)
        self._layers_host, self._layers_dev = host, None
        self.device = device
        if dev_layers is not None:
            self._layers_dev = (dev_layers != 0).to(torch.uint8).contiguous()
            self.device = dev_layers.device
        self._shape = shape

    @property
    def shape(self):
        """(rows, cols)"""
        return self._shape[1:]

    @property
    def n_layers(self):
        return self._shape[0]

    @property
    def layers(self):
        """The device copy (uploaded on first use)."""
        if self._layers_dev is None:
            _lib.require_gpu()
            self._layers_dev = torch.tensor(self._layers_host, device=self.device)
        return self._layers_dev

    @property
    def layers_host(self):
        if self._layers_host is None:
            self._layers_host = self._layers_dev.cpu().numpy()
        return self._layers_host

    @classmethod
    def from_grid(cls, grid):
        """One layer: the OccupancyGrid's image at every heading."""
        if grid._occupancy_dev is not None:
            return cls(grid._occupancy_dev[None], grid.boundaries, grid.resolution)
        return cls(grid.occupancy_host[None], grid.boundaries, grid.resolution, grid.device)

    @classmethod
    def from_checker(cls, checker, resolution, boundaries=None, device=None):
        """Eight layers from one `labels` call of a device checker over 8 * cells poses (cell centre, float32(h * pi / 4)):
        the box robot gets its footprint per heading from the checker's own kernels."""
        if resolution is None:
            raise TypeError("from_checker() needs a resolution")
        if not hasattr(checker, "labels"):
            raise TypeError("LatticeGrid.from_checker needs a device checker (one with `labels`)")
        boundaries = checker_boundaries(checker, boundaries)
        x, y, x_cells, y_cells = cell_centres(boundaries, resolution)
        dev = checker_device(checker, device)
        labels = checker.labels(torch.tensor(heading_poses(x, y, HEADINGS), device=dev))   # h * 2 pi / 8 = h * pi / 4 to the bit
        return cls((labels > 0).to(torch.uint8).reshape(HEADINGS, y_cells, x_cells), boundaries, resolution)

    def states_of(self, points, free_heading=False):
        """[B, 3] device poses -> int32 [B, 3] (row, col, heading index); heading -1 everywhere with `free_heading`."""
        cells = self.cells_of(points)
        h = torch.full_like(cells[:, 0], -1) if free_heading else heading_index(points[:, 2])
        return torch.cat([cells, h[:, None]], 1).contiguous()


def _cost(value, name="turn_cost"):
    if int(value) != value or not 0 <= int(value) <= 255:
        raise ValueError("%s must be an integer 0 .. 255" % name)
    return int(value)


def _gear_costs(turn_cost, reverse_cost, cusp_cost):
    return _cost(turn_cost), _cost(reverse_cost, "reverse_cost"), _cost(cusp_cost, "cusp_cost")


def _check_bound(lgrid, costs, gear_layers):
    """costs: (turn_cost,) with gear_layers 1, (turn_cost, reverse_cost, cusp_cost) with gear_layers 2."""
    rows, cols = lgrid.shape
    if gear_layers * HEADINGS * rows * cols * (1 + sum(costs)) >= 2 ** 21:
        if gear_layers == 2:
            raise ValueError("16 * rows * cols * (1 + turn_cost + reverse_cost + cusp_cost) must stay below 2^21 (%d x %d, costs %s)"
                             % (rows, cols, costs))
        raise ValueError("8 * rows * cols * (1 + turn_cost) must stay below 2^21 (%d x %d, turn_cost %d)" % (rows, cols, costs[0]))


def _fields(lgrid, goal_states, costs, gear_layers):
    """The fields of either search: [G, 8, rows, cols, 2] with gear_layers 1, [G, 2, 8, rows, cols, 2] with gear_layers 2."""
    lib = _lib.load()
    _check_bound(lgrid, costs, gear_layers)
    layers = lgrid.layers
    rows, cols = lgrid.shape
    goal_states, = int32_on(layers.device, goal_states)
    if goal_states.dim() != 2 or goal_states.shape[1] != 3:
        raise ValueError("goal_states must be [G, 3] (row, col, heading)")
    g = goal_states.shape[0]
    fields = torch.empty((g,) + (2,) * (gear_layers - 1) + (HEADINGS, rows, cols, 2), dtype=torch.int32, device=layers.device)
    query, entry = ((lib.nfopp_lattice_fields_workspace_bytes, lib.nfopp_lattice_distance_fields) if gear_layers == 1 else
                    (lib.nfopp_lattice_gear_fields_workspace_bytes, lib.nfopp_lattice_gear_distance_fields))
    ws = workspace(query(rows, cols, *costs, g), layers.device)
    _lib.check(entry(_lib.ptr(layers, torch.uint8), lgrid.n_layers, rows, cols, _lib.ptr(goal_states, torch.int32), g, *costs,
                     _lib.ptr(fields, torch.int32), ws.ptr, ws.nbytes, _lib.stream_ptr()))
    return fields


def lattice_fields(lgrid, goal_states, turn_cost=0):
    """goal_states int32 [G, 3] (row, col, heading or -1) on the device -> int32 [G, 8, rows, cols, 2]: the exact cost (a, b)
    from every state to the goal state; (-1, -1) = blocked or unreachable."""
    return _fields(lgrid, goal_states, (_cost(turn_cost),), 1)


def lattice_gear_fields(lgrid, goal_states, turn_cost=0, reverse_cost=0, cusp_cost=0):
    """goal_states int32 [G, 3] (row, col, heading or -1) on the device -> int32 [G, 2, 8, rows, cols, 2]: the exact cost (a, b)
    from every state (gear, heading, cell) to the goal state with reverse moves allowed; (-1, -1) = blocked or unreachable."""
    return _fields(lgrid, goal_states, _gear_costs(turn_cost, reverse_cost, cusp_cost), 2)


def _search(lgrid, starts, goals, turn_cost, goal_heading, max_field_bytes, gear_costs=None):
    """-> (cells, headings, count, status, cost, starts, goals), all on the device; with `gear_costs` = (reverse_cost,
    cusp_cost) the search over (cell, heading, gear) states, and `gears` [B, max_len] behind the seven."""
    lib = _lib.load()
    if not isinstance(lgrid, LatticeGrid):
        raise TypeError("the lattice search needs a LatticeGrid")
    if goal_heading not in GOAL_HEADING_MODES:
        raise ValueError("goal_heading must be 'fixed' or 'free'")
    # the two searches differ in their costs, their field and trace entries, and the gear layer of the field; nothing below
    # this block asks which one runs
    if gear_costs is None:
        costs, trace_entry, gear_layers = (_cost(turn_cost),), lib.nfopp_lattice_trace_paths, 1
    else:
        costs, trace_entry, gear_layers = _gear_costs(turn_cost, *gear_costs), lib.nfopp_lattice_gear_trace_paths, 2
    _check_bound(lgrid, costs, gear_layers)
    starts, goals = as_device_points(lgrid, starts), as_device_points(lgrid, goals)
    if starts.shape != goals.shape or starts.shape[1] != 3:
        raise ValueError("starts and goals must both be [B, 3] poses (x, y, theta)")
    rows, cols = lgrid.shape
    b = starts.shape[0]
    i32 = torch.int32
    start_states = lgrid.states_of(starts)
    goal_states = lgrid.states_of(goals, free_heading=goal_heading == "free")
    # the key of a goal: (flat cell index, heading + 1), the heading -1 .. 7 in the low digit
    inside, flat = cell_keys(goal_states, lgrid.shape)
    key = flat * (HEADINGS + 1) + goal_states[:, 2].long() + 1
    uniq, field_index = goal_table(torch.where(inside, key, torch.full_like(key, -1)))
    cell = uniq // (HEADINGS + 1)
    unique_states = torch.stack([cell // cols, cell % cols, uniq % (HEADINGS + 1) - 1], 1).to(i32).contiguous()
    n_total = unique_states.shape[0]
    per_field = gear_layers * HEADINGS * rows * cols * 8

    def trace(fields, first, paths, count, status, cost):
        # the gear trace writes `gears` behind the headings: its third path tensor
        _lib.check(trace_entry(
            _lib.ptr(fields, i32), first, 0 if fields is None else fields.shape[0], n_total, rows, cols, *costs,
            _lib.ptr(start_states, i32), _lib.ptr(goal_states, i32), _lib.ptr(field_index, i32), b, paths[0].shape[1] if paths else 0,
            *[_lib.ptr(t, i32) for t in paths or (None,) * (1 + gear_layers)], _lib.ptr(count, i32), _lib.ptr(status, i32),
            _lib.ptr(cost, i32), _lib.stream_ptr()))

    paths, count, status, cost = traced_search(
        b, starts.device, n_total, max(1, int(max_field_bytes) // per_field), ((2,), ()) + ((),) * (gear_layers - 1),
        lambda first, last: _fields(lgrid, unique_states[first:last], costs, gear_layers), trace)
    return (paths[0], paths[1], count, status, cost, starts, goals) + tuple(paths[2:])


def lattice_search_paths(lgrid, starts, goals, turn_cost=0, goal_heading="fixed", max_field_bytes=2 ** 30):
    """starts, goals [B, 3] poses -> (cells int32 [B, max_len, 2] (row, col), headings int32 [B, max_len], counts [B], status
    [B], costs [B, 2] = (a, b)), on the device; what lies behind a row's count is zero.  goal_heading "fixed": the goal state
    is (goal cell, heading_index(goal theta)); "free": the goal cell at any heading.  Distinct goal states are searched once,
    in chunks whose fields stay within `max_field_bytes` (at least one field per chunk)."""
    return _search(lgrid, starts, goals, turn_cost, goal_heading, max_field_bytes)[:5]


def lattice_search_init(lgrid, starts, goals, n_waypoints, init_angles_with_trajectory=True, out=None, turn_cost=0,
                        goal_heading="fixed"):
    """-> (traj [B, N, 3] fp32, status [B] int32) on the device: the lattice path's cells through seed_trajectories.  status 0
    = seeded along a minimum-cost lattice path; 1 = goal state unreachable, 2 = start or goal outside the grid (or a start
    heading that is not finite): those problems get the straight line of `init_trajectories`."""
    cells, _, count, status, _, starts, goals = _search(lgrid, starts, goals, turn_cost, goal_heading, 2 ** 30)
    traj = seed_trajectories(lgrid, cells, count, status, starts, goals, n_waypoints, init_angles_with_trajectory, out)
    return traj, status


def lattice_gear_search_paths(lgrid, starts, goals, turn_cost=0, reverse_cost=0, cusp_cost=0, goal_heading="fixed",
                              max_field_bytes=2 ** 30):
    """lattice_search_paths with reverse moves: -> (cells int32 [B, max_len, 2], headings int32 [B, max_len], gears int32
    [B, max_len], counts [B], status [B], costs [B, 2]) on the device.  gears[k] is the gear (0 forward, 1 reverse) of the move
    into state k, gears[0] the gear of the first move.  `reverse_cost` is charged per reverse move, `cusp_cost` per change of
    gear after the first move.  Goal states are shared and chunked as in lattice_search_paths."""
    cells, headings, count, status, cost, _, _, gears = _search(lgrid, starts, goals, turn_cost, goal_heading, max_field_bytes,
                                                                (reverse_cost, cusp_cost))
    return cells, headings, gears, count, status, cost


def seed_lattice_trajectories(lgrid, cells, headings, count, status, starts, goals, n_waypoints, out=None):
    """Lattice paths -> [B, N, 3] fp32 trajectories (nfopp_lattice_seed_trajectories): xy as `seed_trajectories` gives for the
    same cells, theta the body heading of the lattice states, unwound and interpolated over the spline's parameter.  A
    problem with status != 0 gets the straight line of `init_trajectories(..., False)`."""
    lib = _lib.load()
    starts, goals = as_device_points(lgrid, starts), as_device_points(lgrid, goals)
    if starts.shape != goals.shape or starts.shape[1] != 3:
        raise ValueError("starts and goals must both be [B, 3] poses (x, y, theta)")
    b = starts.shape[0]
    cells, headings, count, status = int32_on(starts.device, cells, headings, count, status)
    if cells.dim() != 3 or cells.shape[0] != b or cells.shape[2] != 2 or headings.shape != cells.shape[:2] or \
            count.shape != (b,) or status.shape != (b,):
        raise ValueError("cells [B, max_len, 2], headings [B, max_len], count [B] and status [B] must agree with the poses")
    return seed_launch(lib.nfopp_lattice_seed_workspace_bytes, lib.nfopp_lattice_seed_trajectories, [cells, headings], count, status,
                       starts, goals, n_waypoints, lgrid.origin_resolution, out)


def gear_changes(gears, count, status):
    """int32 [B] on the device: the moves of each traced path whose gear differs from the one before (0 where status != 0)."""
    k = torch.arange(gears.shape[1], device=gears.device)[None, :]
    differ = (gears[:, 1:] != gears[:, :-1]) & (k[:, 1:] >= 2) & (k[:, 1:] < count[:, None]) & (status[:, None] == 0)
    return differ.sum(1).to(torch.int32)


def lattice_gear_search_init(lgrid, starts, goals, n_waypoints, out=None, turn_cost=0, reverse_cost=0, cusp_cost=0,
                             goal_heading="fixed"):
    """-> (traj [B, N, 3] fp32, status [B] int32, gear_changes [B] int32) on the device: the minimum-cost path over forward
    and reverse moves through seed_lattice_trajectories.  status as lattice_search_init; gear_changes counts the cusps of the
    seed (0 where status != 0)."""
    cells, headings, count, status, _, starts, goals, gears = _search(lgrid, starts, goals, turn_cost, goal_heading, 2 ** 30,
                                                                      (reverse_cost, cusp_cost))
    traj = seed_lattice_trajectories(lgrid, cells, headings, count, status, starts, goals, n_waypoints, out)
    return traj, status, gear_changes(gears, count, status)


class GearLattice(object):
    """Initializer for BatchPlanner.init: a LatticeGrid searched with reverse moves at the given costs."""

    def __init__(self, lgrid, reverse_cost=0, cusp_cost=0):
        if not isinstance(lgrid, LatticeGrid):
            raise TypeError("GearLattice needs a LatticeGrid")
        self.lgrid = lgrid
        self.reverse_cost = _cost(reverse_cost, "reverse_cost")
        self.cusp_cost = _cost(cusp_cost, "cusp_cost")
