"""Prioritised start-delay scheduling of a fleet (csrc/fleet_schedule.hip): every robot keeps its path and only when it leaves
changes -- in priority order each robot takes the smallest start delay, in steps of the time grid, that keeps it clear of every
robot scheduled before it and of every predicted obstacle.  The rule is stated in include/nfopp_hip.h; nothing here
synchronises when the inputs are device tensors.  The uint64 mask words travel in int64 tensors (the same bits), on which
torch's bitwise operators work."""
import numpy as np
import torch

from . import _lib
from ._grid import workspace
from ._tracks import check_tracks, hip_device, per_row, raw_ptr

# values of FleetSchedule.status (NFOPP_SCHEDULE_*)
SCHEDULE_OK, SCHEDULE_BAD_TRACK, SCHEDULE_UNRESOLVED, SCHEDULE_NOT_ORDERED = 0, 1, 2, 3
SCHEDULE_MAX_DELAY = _lib.SCHEDULE_MAX_DELAY


def _check_max_delay(max_delay):
    if int(max_delay) != max_delay or not 0 <= int(max_delay) <= SCHEDULE_MAX_DELAY:
        raise ValueError("max_delay must be an integer in 0 .. %d, got %r" % (SCHEDULE_MAX_DELAY, max_delay))
    return int(max_delay)


class FleetSchedule(object):
    """What the assignment pass decided.  Device tensors [B]: `delay` int32 (grid steps; -1 = not scheduled), `status` int32
    (0, SCHEDULE_BAD_TRACK, SCHEDULE_UNRESOLVED, SCHEDULE_NOT_ORDERED), `forbidden` int64 (bit d: delay d was taken from the
    robot by an obstacle or by a robot scheduled before it).  `TimedPaths.schedule` adds `delay_seconds` [B] float64 (NaN = not
    scheduled) and `complete` [B] bool: the robot reaches its goal within the sampled instants, so "parked at its last
    sample" is "parked at its goal"."""
    OK, BAD_TRACK, UNRESOLVED, NOT_ORDERED = SCHEDULE_OK, SCHEDULE_BAD_TRACK, SCHEDULE_UNRESOLVED, SCHEDULE_NOT_ORDERED

    def __init__(self, delay, status, forbidden, max_delay, delay_seconds=None, complete=None):
        self.delay, self.status, self.forbidden, self.max_delay = delay, status, forbidden, max_delay
        self.delay_seconds, self.complete = delay_seconds, complete
        # set by `TimedPaths.schedule`, for `replan`: the sampled tracks, the margin as a number, the sampled obstacles
        self.tracks = self.margin = self.obstacles = self.obstacle_radius = None

    @property
    def scheduled(self):
        """[B] bool device tensor: the robots that got a delay."""
        return self.status == SCHEDULE_OK

    def replan(self, tracks, grid, count, *, robot_radius, margin="snap", base_margin=0.0, obstacles=None, obstacle_radius=None):
        """Another path, chosen with time in it, for every robot this schedule left SCHEDULE_UNRESOLVED (`nfopp.spacetime_plan`).
        `tracks` [B, K, >= 2] are the tracks the schedule was made from.  The scheduled robots' `delay_tracks` over `count`
        instants become the visible movers (radius `robot_radius`); every unresolved robot is searched on `grid` (an
        OccupancyGrid, inflated by the caller for the robot's footprint) from the cell of its first sample to the cell of its
        last, in index order, each against the movers, `obstacles` [M, count, >= 2] and the robots re-planned before it.  A
        robot with a bad track (SCHEDULE_BAD_TRACK: its samples are not finite, so it has no cells) or one the schedule never
        visited (SCHEDULE_NOT_ORDERED) is not searched: it comes back SPACETIME_NOT_ORDERED and is not on the floor, as in
        the schedule.  A re-planned track starts at the centre of its start cell, up to res / sqrt(2) from where the robot
        stands: `margin="snap"` is `base_margin` (the margin of the schedule) plus that, a number is taken as it is.
        Everything is built from torch operations on device tensors: nothing synchronises.
        -> (`SpaceTimePlan`, merged [B, count, 2] fp32: the delayed track of a scheduled robot, the planned track of a
        re-planned one, NaN rows for every other robot -- it still has no place -- ready for `track_conflicts`)."""
        from .spacetime import spacetime_plan
        if isinstance(margin, str):
            if margin != "snap":
                raise ValueError("margin must be \"snap\" or a number, got %r" % (margin,))
            margin = float(base_margin) + grid.resolution / np.sqrt(2.0)
        b = tracks.shape[0]
        if self.status.numel() != b:
            raise ValueError("tracks must be the [B] = [%d] tracks of this schedule, got %d" % (self.status.numel(), b))
        on = self.scheduled
        moved = delay_tracks(tracks[:, :, :2], self.delay, count)
        order = torch.where(self.status == SCHEDULE_UNRESOLVED, torch.arange(b, dtype=torch.int32, device=self.status.device),
                            torch.full_like(self.status, -1))
        radius = torch.full((b,), float(np.float32(robot_radius)), dtype=torch.float32, device=moved.device)
        visible = on
        if obstacles is not None:
            m = obstacles.shape[0]
            moved_all = torch.cat([moved, obstacles[:, :, :2].to(torch.float32)], 0).contiguous()
            radius = torch.cat([radius, per_row(0.0 if obstacle_radius is None else obstacle_radius, m, moved.device, "obstacle_radius")])
            visible = torch.cat([on, torch.ones(m, dtype=torch.bool, device=on.device)])
        else:
            moved_all = moved
        plan = spacetime_plan(grid, tracks[:, 0, :2], tracks[:, -1, :2], count, robot_radius=robot_radius, margin=margin, tracks=moved_all,
                              track_radius=radius, visible=visible, order=order)
        merged = torch.where(plan.planned[:, None, None], plan.tracks,
                             torch.where(on[:, None, None], moved, torch.full_like(moved, float("nan"))))
        return plan, merged


class FleetMasks(object):
    """What `fleet_shift_masks` found.  Device tensors: `pair` [B, B, 2] int64 (the 128-bit mask of every pair as two
    little-endian words: bit r + max_delay says that robot i delayed by r grid steps more than robot j conflicts with it),
    `base` [B] int64 (bit d: robot i delayed by d conflicts with an obstacle), `bad` [B] int32.  `assign` may be called any
    number of times, with other priority orders, without recomputing the masks.  `box` [B, 4] and `refine`: the boxes and
    the refinement depth of `fleet_box_shift_masks` (a set bit then says "not FREE by the box check"); None and 0 for discs."""

    def __init__(self, pair, base, bad, max_delay, box=None, refine=0):
        self.pair, self.base, self.bad, self.max_delay = pair, base, bad, _check_max_delay(max_delay)
        self.box, self.refine = box, refine

    def assign(self, order=None, want_forbidden=True):
        """order: None (robot 0 first), or [B] integers: the robots in priority order (an entry out of range or repeated is
        skipped on the device; a robot that never occurs is SCHEDULE_NOT_ORDERED) -> `FleetSchedule`."""
        b = self.pair.shape[0]
        device = self.pair.device
        if order is not None:
            if not isinstance(order, torch.Tensor):
                order = torch.from_numpy(np.array(order, np.int64).reshape(-1))
            if order.dim() != 1 or order.numel() != b or order.is_floating_point():
                raise ValueError("order must be [B] = [%d] integers, got %s %s" % (b, tuple(order.shape), order.dtype))
            order = order.to(device=device, dtype=torch.int32).contiguous()
        i32 = dict(dtype=torch.int32, device=device)
        delay, status = torch.empty(b, **i32), torch.empty(b, **i32)
        forbidden = torch.empty(b, dtype=torch.int64, device=device) if want_forbidden else None
        _lib.check(_lib.load().nfopp_fleet_assign_delays(
            _lib.ptr(self.pair, torch.int64), _lib.ptr(self.base, torch.int64), _lib.ptr(self.bad, torch.int32),
            _lib.ptr(order, torch.int32), b, self.max_delay, _lib.ptr(delay, torch.int32), _lib.ptr(status, torch.int32),
            _lib.ptr(forbidden, torch.int64), _lib.stream_ptr()))
        return FleetSchedule(delay, status, forbidden, self.max_delay)


def fleet_shift_masks(tracks, *, max_delay, radius=0.0, margin=0.0, obstacles=None, obstacle_radius=None):
    """tracks [B, K, >= 2]: fp32 HIP tensor of positions on a common time grid, x and y first in a row (`TimedPaths.sample`
    returns such a tensor); candidate delays are 0 .. max_delay <= 63 grid steps.  `radius` / `obstacle_radius`: a number or one
    per track; `margin` is added to every sum of radii.  `obstacles` [M, K + max_delay, >= 2]: predicted tracks in absolute
    time, never shifted -> `FleetMasks`."""
    max_delay = _check_max_delay(max_delay)
    b, k, stride = check_tracks(tracks, "tracks")
    m, stride_o = 0, 2
    if obstacles is not None:
        m, ko, stride_o = check_tracks(obstacles, "obstacles")
        if ko != k + max_delay:
            raise ValueError("obstacles must cover K + max_delay = %d instants, got %d" % (k + max_delay, ko))
    device = hip_device("fleet_shift_masks", "tracks", tracks, "obstacles", obstacles)
    radius = per_row(radius, b, device, "radius")
    obstacle_radius = None if obstacles is None else per_row(obstacle_radius, m, device, "obstacle_radius")
    lib = _lib.load()
    pair = torch.empty(b, b, 2, dtype=torch.int64, device=device)
    base = torch.empty(b, dtype=torch.int64, device=device)
    bad = torch.empty(b, dtype=torch.int32, device=device)
    ws = workspace(lib.nfopp_fleet_shift_masks_workspace_bytes(b, m), device)
    _lib.check(lib.nfopp_fleet_shift_masks(
        raw_ptr(tracks), b, stride, k, _lib.ptr(radius), float(margin), max_delay, raw_ptr(obstacles) if m else None, m, stride_o,
        _lib.ptr(obstacle_radius) if m else None, _lib.ptr(pair, torch.int64), _lib.ptr(base, torch.int64), _lib.ptr(bad, torch.int32),
        ws.ptr, ws.nbytes, _lib.stream_ptr()))
    return FleetMasks(pair, base, bad, max_delay)


def schedule_delays(tracks, *, max_delay, radius=0.0, margin=0.0, obstacles=None, obstacle_radius=None, order=None):
    """`fleet_shift_masks` and `FleetMasks.assign` in one call -> `FleetSchedule`."""
    return fleet_shift_masks(tracks, max_delay=max_delay, radius=radius, margin=margin, obstacles=obstacles,
                             obstacle_radius=obstacle_radius).assign(order)


def fleet_box_shift_masks(tracks, *, max_delay, box, radius=0.0, margin=0.0, refine=0, obstacles=None, obstacle_box=None,
                          obstacle_radius=None):
    """`fleet_shift_masks` for oriented boxes (csrc/fleet_box_schedule.hip).  tracks [B, K, >= 3]: fp32 HIP tensor of poses on
    a common time grid, x, y, theta first in a row; `box`: one box (x0, x1, y0, y1) in the body frame or [B, 4]; `radius`: the
    rounding radius, a number or [B]; `refine` (0 .. 8): how often an interval the certificate leaves undecided is halved.  A
    bit is set when `box_track_conflicts` would not call the shifted pair FREE.  `obstacles` [M, K + max_delay, >= 3] with
    `obstacle_box` (default: `box`, which must then be one box) and `obstacle_radius` -> `FleetMasks`."""
    from .conflicts import _per_row_boxes, track_headings
    max_delay = _check_max_delay(max_delay)
    b, k, stride = check_tracks(tracks, "tracks")
    if box is None:
        raise ValueError("fleet_box_shift_masks needs box; discs go to fleet_shift_masks")
    m, stride_o = 0, 3
    if obstacles is not None:
        m, ko, stride_o = check_tracks(obstacles, "obstacles")
        if ko != k + max_delay:
            raise ValueError("obstacles must cover K + max_delay = %d instants, got %d" % (k + max_delay, ko))
    if tracks.shape[2] < 3 or (obstacles is not None and obstacles.shape[2] < 3):
        raise ValueError("box tracks must be [B, K, >= 3] (x, y, theta)")
    refine = int(refine)
    if not 0 <= refine <= _lib.BOX_CONFLICT_MAX_REFINE:
        raise ValueError("refine must be 0 .. %d, got %d" % (_lib.BOX_CONFLICT_MAX_REFINE, refine))
    device = hip_device("fleet_box_shift_masks", "tracks", tracks, "obstacles", obstacles)
    given_box, box = box, _per_row_boxes(box, b, device, "box")
    radius = per_row(radius, b, device, "radius")
    heading = track_headings(tracks)
    obstacle_heading = None
    if m:
        if obstacle_box is None:
            if int(np.prod(np.shape(given_box))) != 4:
                raise ValueError("obstacles need obstacle_box when box is one per robot")
            obstacle_box = given_box
        obstacle_box = _per_row_boxes(obstacle_box, m, device, "obstacle_box")
        obstacle_radius = per_row(0.0 if obstacle_radius is None else obstacle_radius, m, device, "obstacle_radius")
        obstacle_heading = track_headings(obstacles)
    lib = _lib.load()
    pair = torch.empty(b, b, 2, dtype=torch.int64, device=device)
    base = torch.empty(b, dtype=torch.int64, device=device)
    bad = torch.empty(b, dtype=torch.int32, device=device)
    ws = workspace(lib.nfopp_fleet_box_shift_masks_workspace_bytes(b, m, k, max_delay), device)
    _lib.check(lib.nfopp_fleet_box_shift_masks(
        raw_ptr(tracks), _lib.ptr(heading, torch.float64), b, stride, k, _lib.ptr(box), _lib.ptr(radius), float(margin), refine,
        max_delay, raw_ptr(obstacles) if m else None, _lib.ptr(obstacle_heading, torch.float64), m, stride_o,
        _lib.ptr(obstacle_box) if m else None, _lib.ptr(obstacle_radius) if m else None, _lib.ptr(pair, torch.int64),
        _lib.ptr(base, torch.int64), _lib.ptr(bad, torch.int32), ws.ptr, ws.nbytes, _lib.stream_ptr()))
    return FleetMasks(pair, base, bad, max_delay, box=box, refine=refine)


def schedule_box_delays(tracks, *, max_delay, box, radius=0.0, margin=0.0, refine=0, obstacles=None, obstacle_box=None,
                        obstacle_radius=None, order=None):
    """`fleet_box_shift_masks` and `FleetMasks.assign` in one call -> `FleetSchedule`: `schedule_delays` for oriented boxes."""
    return fleet_box_shift_masks(tracks, max_delay=max_delay, box=box, radius=radius, margin=margin, refine=refine, obstacles=obstacles,
                                 obstacle_box=obstacle_box, obstacle_radius=obstacle_radius).assign(order)


def delay_tracks(tracks, delay, count):
    """tracks [B, K, S], delay [B] integers (a negative one counts as 0) -> [B, count, S]: robot i at
    tracks[i, clamp(h - delay[i], 0, K - 1)] at instant h -- it waits at its first sample and stays parked at its last.  The
    form to hand to `track_conflicts` or to a controller."""
    if tracks.dim() != 3 or tracks.shape[1] < 1:
        raise ValueError("tracks must be [B, K, S] with K >= 1, got %s" % (tuple(tracks.shape),))
    delay = torch.as_tensor(delay, device=tracks.device).reshape(-1).to(torch.int64).clamp(min=0)
    if delay.numel() != tracks.shape[0]:
        raise ValueError("delay must be [B] = [%d], got %d values" % (tracks.shape[0], delay.numel()))
    h = torch.arange(int(count), device=tracks.device)
    idx = (h[None, :] - delay[:, None]).clamp(0, tracks.shape[1] - 1)
    return torch.gather(tracks, 1, idx[:, :, None].expand(-1, -1, tracks.shape[2])).contiguous()
