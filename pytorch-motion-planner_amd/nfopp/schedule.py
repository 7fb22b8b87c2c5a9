"""Prioritised start-delay scheduling of a fleet (csrc/fleet_schedule.hip): every robot keeps its path and only when it leaves
changes -- in priority order each robot takes the smallest start delay, in steps of the time grid, that keeps it clear of every
robot scheduled before it and of every predicted obstacle.  The rule is stated in include/nfopp_hip.h; nothing here
synchronises when the inputs are device tensors.  The uint64 mask words travel in int64 tensors (the same bits), on which
torch's bitwise operators work."""
import numpy as np
import torch

from . import _lib
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

    @property
    def scheduled(self):
        """[B] bool device tensor: the robots that got a delay."""
        return self.status == SCHEDULE_OK


class FleetMasks(object):
    """What `fleet_shift_masks` found.  Device tensors: `pair` [B, B, 2] int64 (the 128-bit mask of every pair as two
    little-endian words: bit r + max_delay says that robot i delayed by r grid steps more than robot j conflicts with it),
    `base` [B] int64 (bit d: robot i delayed by d conflicts with an obstacle), `bad` [B] int32.  `assign` may be called any
    number of times, with other priority orders, without recomputing the masks."""

    def __init__(self, pair, base, bad, max_delay):
        self.pair, self.base, self.bad, self.max_delay = pair, base, bad, _check_max_delay(max_delay)

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
    nbytes = int(lib.nfopp_fleet_shift_masks_workspace_bytes(b, m))
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _lib.check(lib.nfopp_fleet_shift_masks(
        raw_ptr(tracks), b, stride, k, _lib.ptr(radius), float(margin), max_delay, raw_ptr(obstacles) if m else None, m, stride_o,
        _lib.ptr(obstacle_radius) if m else None, _lib.ptr(pair, torch.int64), _lib.ptr(base, torch.int64), _lib.ptr(bad, torch.int32),
        _lib.ptr(workspace, torch.uint8), nbytes, _lib.stream_ptr()))
    return FleetMasks(pair, base, bad, max_delay)


def schedule_delays(tracks, *, max_delay, radius=0.0, margin=0.0, obstacles=None, obstacle_radius=None, order=None):
    """`fleet_shift_masks` and `FleetMasks.assign` in one call -> `FleetSchedule`."""
    return fleet_shift_masks(tracks, max_delay=max_delay, radius=radius, margin=margin, obstacles=obstacles,
                             obstacle_radius=obstacle_radius).assign(order)


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
