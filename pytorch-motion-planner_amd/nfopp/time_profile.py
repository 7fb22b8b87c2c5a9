"""Time parametrisation of planned paths under motion limits (csrc/time_profile.hip): the velocity profile and the timed
trajectory of a whole batch, on the device.  The rule is stated in include/nfopp_hip.h; nothing here synchronises when the
inputs are device tensors."""
import collections

import numpy as np
import torch

from . import _lib
from ._tracks import per_row

# slots of TimedPaths.profile [B, N + 2, 4] (NFOPP_TIME_SLOT_*) and TimedPaths.summary [B, 4] (NFOPP_TIME_SUMMARY_*)
TIME_SLOT_S, TIME_SLOT_T, TIME_SLOT_V, TIME_SLOT_V_PEAK = range(_lib.NUM_TIME_SLOTS)
TIME_SUMMARY_TIME, TIME_SUMMARY_LENGTH, TIME_SUMMARY_STOPS, TIME_SUMMARY_STATUS = range(_lib.NUM_TIME_SUMMARY)
# bits of the status slot (NFOPP_TIME_*)
TIME_START_TOO_FAST, TIME_GOAL_UNREACHABLE, TIME_OUT_OF_RANGE = 1, 2, 4


class MotionLimits(collections.namedtuple("MotionLimits", "v_max a_max d_max a_lat w_max cusp_angle")):
    """What the robot may do along a path: top speed [m/s], acceleration and deceleration [m/s^2], lateral acceleration
    v^2 * kappa and turn rate v * kappa (inf = no such limit), and the cusp rule of `BatchPlanner.path_stats`: the robot
    stops at a vertex where the path folds back to within `cusp_angle` of the way it came (None = no cusp stops)."""
    __slots__ = ()

    def __new__(cls, v_max, a_max, d_max=None, a_lat=float("inf"), w_max=float("inf"), cusp_angle=np.pi / 3):
        return super().__new__(cls, float(v_max), float(a_max), float(a_max if d_max is None else d_max), float(a_lat),
                               float(w_max), None if cusp_angle is None else float(cusp_angle))

    @property
    def cos_cusp(self):
        return -1.0 if self.cusp_angle is None else float(np.cos(np.pi - self.cusp_angle))

    def to_c(self):
        return _lib.MotionLimitsC(self.v_max, self.a_max, self.d_max, self.a_lat, self.w_max, self.cos_cusp)


def _chord_margin_or_number(margin, v_self, v_other, dt):
    """`margin` of `TimedPaths.conflicts` / `.schedule`: a number as it is, "chord" -> `chord_margin` of the two top speeds
    (v_other None: the other side is a tracks tensor whose top speed was not given)."""
    if not isinstance(margin, str):
        return margin
    if margin != "chord":
        raise ValueError("margin must be a number or \"chord\", got %r" % (margin,))
    if v_other is None:
        raise ValueError("margin=\"chord\" against a tracks tensor needs other_v_max, the top speed of those tracks")
    from .conflicts import chord_margin
    return chord_margin(v_self, v_other, dt)


def _box_turn_margin(box, w_max, dt):
    """The rotation term of the chord margin for one side: reach * w_max * dt / 2, reach the farthest corner of the largest
    of the side's boxes (host values: one box or [B, 4])."""
    from .conflicts import box_reach
    if isinstance(box, torch.Tensor):
        raise ValueError("margin=\"chord\" needs the boxes as host values; give a number for boxes held on the device")
    if w_max is None or not np.isfinite(w_max):
        raise ValueError("margin=\"chord\" for boxes needs a finite turn-rate limit (MotionLimits.w_max / other_w_max)")
    reach = max(box_reach(b) for b in np.asarray(box, np.float64).reshape(-1, 4))
    return reach * float(w_max) * float(dt) / 2.0


def _box_margin_or_number(margin, v_self, v_other, dt, box, w_self, other_box=None, w_other=None, one_for_both=False):
    """`margin` of `TimedPaths.conflicts(box=)` / `.schedule_boxes`: a number as it is, "chord" -> the chord margin of the two
    top speeds plus `_box_turn_margin` of the first side plus that of the second (`other_box` None: the paths against each
    other, the second side is the first).  `one_for_both`: one margin for robot pairs and obstacle pairs alike, so the second
    term is the larger of the two sides'."""
    if not isinstance(margin, str):
        return margin
    chord = _chord_margin_or_number(margin, v_self, v_other, dt)
    own = _box_turn_margin(box, w_self, dt)
    far = own if other_box is None else _box_turn_margin(other_box, w_other, dt)
    return chord + own + (max(own, far) if one_for_both else far)


def _check_paths(traj, start, goal):
    """traj [B, N, D] with N >= 1 and D = 2 or 3, start / goal [B, D]: what the kernels index by."""
    if not all(isinstance(x, torch.Tensor) for x in (traj, start, goal)):
        raise TypeError("traj, start and goal must be tensors")
    if traj.dim() != 3 or traj.shape[1] < 1 or traj.shape[2] not in (2, 3):
        raise ValueError("traj must be [B, N, D] with N >= 1 and D = 2 or 3, got %s" % (tuple(traj.shape),))
    b, _, d = traj.shape
    if tuple(start.shape) != (b, d) or tuple(goal.shape) != (b, d):
        raise ValueError("start and goal must be [B, D] = [%d, %d], got %s and %s" % (b, d, tuple(start.shape), tuple(goal.shape)))


class TimedPaths(object):
    """The velocity profile of a batch of paths.  Device tensors: `profile` [B, N + 2, 4] float64 (TIME_SLOT_*: arc length
    s, time t, speed v at every vertex, and the peak speed of the segment that starts there), `gear` [B, N + 1] int8
    (+1 forward, -1 reverse; None = forward throughout), `summary` [B, 4] float64 (TIME_SUMMARY_*: total time, length,
    stops, status bits).  `traj`, `start`, `goal` are the poses the profile was computed for; `time_parametrize` stores its
    own copy of them, so the object stays valid when the planner moves on."""

    def __init__(self, traj, start, goal, limits, profile, gear, summary):
        _check_paths(traj, start, goal)
        b, n, _ = traj.shape
        if tuple(profile.shape) != (b, n + 2, _lib.NUM_TIME_SLOTS) or tuple(summary.shape) != (b, _lib.NUM_TIME_SUMMARY):
            raise ValueError("profile must be [B, N + 2, 4] and summary [B, 4] for traj %s, got %s and %s"
                             % (tuple(traj.shape), tuple(profile.shape), tuple(summary.shape)))
        if gear is not None and tuple(gear.shape) != (b, n + 1):
            raise ValueError("gear must be [B, N + 1] = [%d, %d], got %s" % (b, n + 1, tuple(gear.shape)))
        self.traj, self.start, self.goal, self.limits = traj, start, goal, limits
        self.profile, self.gear, self.summary = profile, gear, summary

    def sample(self, dt, count, t0=0.0, want_segment=False):
        """[B, count, D + 1] fp32 device tensor: pose and signed speed at t0 + k * dt; with `want_segment` also the int32
        [B, count] segment each instant falls in (-1 before the start, N + 1 from the goal on)."""
        b, n, d = self.traj.shape
        count = int(count)
        states = torch.empty(b, max(count, 0), d + 1, dtype=torch.float32, device=self.traj.device)
        segment = torch.empty(b, max(count, 0), dtype=torch.int32, device=self.traj.device) if want_segment else None
        lim = self.limits.to_c()
        _lib.check(_lib.load().nfopp_path_time_sample(
            _lib.ptr(self.traj), _lib.ptr(self.start), _lib.ptr(self.goal), b, n, d, lim, _lib.ptr(self.profile, torch.float64),
            _lib.ptr(self.gear, torch.int8), float(t0), float(dt), count, _lib.ptr(states), _lib.ptr(segment, torch.int32),
            _lib.stream_ptr()))
        return (states, segment) if want_segment else states

    def conflicts(self, dt, count, other=None, radius=0.0, other_radius=None, margin=0.0, t0=0.0, want_pairs=False,
                  other_v_max=None, box=None, refine=0, other_box=None, other_w_max=None):
        """The B timed paths as B robots on one floor, sampled at t0 + k * dt (k < count): who comes closer to whom than
        the radii allow, and when first (`nfopp.track_conflicts`, self mode) -> `nfopp.TrackConflicts`.  With `other` -- a
        `TimedPaths`, sampled on the same grid, or a tracks tensor [M, count, >= 2] such as `constant_velocity_tracks`
        returns -- the paths are checked against those tracks instead.  `radius` / `other_radius`: a number or one per track.
        `margin="chord"` is (v_max + the other side's v_max) * dt / 2, what the straight line between two instants can
        hide; for a tracks tensor it needs `other_v_max`.

        With `box` -- (x0, x1, y0, y1) in the body frame, or one per path -- the robots are oriented boxes on SE(2) paths
        (`nfopp.box_track_conflicts` -> `nfopp.BoxTrackConflicts`): `radius` is then the rounding radius, `refine` (0 .. 8)
        how often an undecided interval is halved, `other_box` the boxes of `other` (default: `box`, which must then be one
        box), whose tracks carry x, y, theta.  `margin="chord"` gains reach * w_max * dt / 2 per side (reach: the farthest
        corner of the side's largest box; w_max from the limits, `other_w_max` for a tracks tensor)."""
        from .conflicts import box_track_conflicts, track_conflicts
        tracks_b, vb, wb = None, self.limits.v_max, self.limits.w_max
        if isinstance(other, TimedPaths):
            tracks_b, vb, wb = other.sample(dt, count, t0=t0), other.limits.v_max, other.limits.w_max
        elif other is not None:
            tracks_b, vb, wb = other, other_v_max, other_w_max
        if box is None:
            if refine != 0 or other_box is not None:
                raise ValueError("refine and other_box belong to the box check: give box")
            margin = _chord_margin_or_number(margin, self.limits.v_max, vb, dt)
            if other is None:
                return track_conflicts(self.sample(dt, count, t0=t0), dt=dt, t0=t0, radius_a=radius, margin=margin,
                                       want_pairs=want_pairs)
            return track_conflicts(self.sample(dt, count, t0=t0), tracks_b, dt=dt, t0=t0, radius_a=radius, radius_b=other_radius,
                                   margin=margin, want_pairs=want_pairs)
        if self.traj.shape[2] != 3:
            raise ValueError("the box check needs SE(2) paths (x, y, theta)")
        if other is not None and other_box is None:
            other_box = box
        margin = _box_margin_or_number(margin, self.limits.v_max, vb, dt, box, self.limits.w_max, other_box, wb)
        if other is None:
            return box_track_conflicts(self.sample(dt, count, t0=t0), dt=dt, t0=t0, box_a=box, radius_a=radius, margin=margin,
                                       refine=refine, want_pairs=want_pairs)
        return box_track_conflicts(self.sample(dt, count, t0=t0), tracks_b, dt=dt, t0=t0, box_a=box, box_b=other_box,
                                   radius_a=radius, radius_b=0.0 if other_radius is None else other_radius, margin=margin,
                                   refine=refine, want_pairs=want_pairs)

    def schedule(self, dt, count, max_delay, radius, margin="chord", order=None, other=None, other_radius=None, other_v_max=None):
        """The B timed paths as B robots that may leave late: sampled at k * dt (k < count), every robot gets, in priority
        `order`, the smallest start delay of 0 .. max_delay grid steps that keeps it clear of the robots scheduled before it
        (`nfopp.schedule_delays`) -> `nfopp.FleetSchedule` with `delay_seconds` and `complete`.  `order`: None (robot 0
        first), "longest_first" (a stable device argsort of the total time, descending), or [B] indices.  `other`: a
        `TimedPaths`, sampled at count + max_delay instants, or a tracks tensor [M, count + max_delay, >= 2] of predicted
        obstacles in absolute time.  `margin="chord"` is (v_max + the larger of v_max and the other side's v_max) * dt / 2:
        one margin serves robot pairs and obstacle pairs alike; for a tracks tensor it needs `other_v_max`.  A robot is
        `complete` when its total time fits the sampled instants, so that its last sample is its goal."""
        return self._schedule(dt, count, max_delay, radius, margin, order, other, other_radius, other_v_max)

    def schedule_boxes(self, dt, count, max_delay, box, radius=0.0, margin="chord", order=None, refine=0, other=None,
                       other_box=None, other_radius=None, other_v_max=None, other_w_max=None):
        """`schedule` for oriented boxes on SE(2) paths (`nfopp.fleet_box_shift_masks`): a delay is taken from a robot when
        `conflicts(box=, refine=)` would not call the delayed pair FREE, so the scheduled fleet is FREE by that check.  `box`:
        (x0, x1, y0, y1) in the body frame, or one per path; `radius` the rounding radius; `other` a `TimedPaths` or a tracks
        tensor [M, count + max_delay, >= 3] with x, y, theta, `other_box` its boxes (default: `box`, which must then be one
        box).  `margin="chord"` is the box chord margin as `conflicts(box=)` forms it, the larger of the robot-robot and the
        robot-obstacle value: (v_max + the larger top speed) * dt / 2 plus reach * w_max * dt / 2 of the robots' side plus the
        larger such term of the two sides (`other_w_max` for a tracks tensor)."""
        if box is None:
            raise ValueError("schedule_boxes needs box; discs go to schedule")
        if self.traj.shape[2] != 3:
            raise ValueError("the box schedule needs SE(2) paths (x, y, theta)")
        return self._schedule(dt, count, max_delay, radius, margin, order, other, other_radius, other_v_max,
                              shape=dict(box=box, refine=refine, other_box=other_box, other_w_max=other_w_max))

    def _schedule(self, dt, count, max_delay, radius, margin, order, other, other_radius, other_v_max, shape=None):
        from .schedule import fleet_box_shift_masks, fleet_shift_masks
        count, max_delay = int(count), int(max_delay)
        obstacles, vb, wb = None, self.limits.v_max, None
        if isinstance(other, TimedPaths):
            obstacles, vb, wb = other.sample(dt, count + max_delay), max(vb, other.limits.v_max), other.limits.w_max
        elif other is not None:
            obstacles, vb = other, None if other_v_max is None else max(vb, float(other_v_max))
            wb = None if shape is None else shape["other_w_max"]
        other_box = None
        if shape is None:
            margin = _chord_margin_or_number(margin, self.limits.v_max, vb, dt)
        else:
            if other is not None:
                other_box = shape["box"] if shape["other_box"] is None else shape["other_box"]
            margin = _box_margin_or_number(margin, self.limits.v_max, vb, dt, shape["box"], self.limits.w_max, other_box, wb,
                                           one_for_both=True)
        total = self.summary[:, TIME_SUMMARY_TIME]
        if isinstance(order, str):
            if order != "longest_first":
                raise ValueError("order must be None, \"longest_first\" or [B] indices, got %r" % (order,))
            order = torch.argsort(total, descending=True, stable=True)
        states = self.sample(dt, count)
        if shape is None:
            masks = fleet_shift_masks(states, max_delay=max_delay, radius=radius, margin=margin, obstacles=obstacles,
                                      obstacle_radius=other_radius)
        else:
            masks = fleet_box_shift_masks(states, max_delay=max_delay, box=shape["box"], radius=radius, margin=margin,
                                          refine=shape["refine"], obstacles=obstacles, obstacle_box=other_box,
                                          obstacle_radius=other_radius)
            if obstacles is not None:
                # FleetSchedule.replan reserves discs: an obstacle box as its circumscribed disc plus its rounding radius
                from .conflicts import box_disc_radius
                other_radius = box_disc_radius(other_box, other_radius, obstacles.shape[0], obstacles.device)
        out = masks.assign(order)
        step = torch.tensor(float(dt), dtype=torch.float64, device=out.delay.device)
        out.delay_seconds = torch.where(out.delay >= 0, out.delay.double() * step, torch.full_like(step, float("nan")))
        out.complete = total <= (count - 1) * float(dt)
        # what FleetSchedule.replan goes on from: the sampled tracks, the margin as a number, the obstacles as sampled (box
        # obstacles with the radius of the disc that covers them)
        out.tracks, out.margin, out.obstacles, out.obstacle_radius = states, margin, obstacles, other_radius
        return out


def time_parametrize(traj, start, goal, limits, v_start=None, v_goal=None):
    """traj [B, N, D], start / goal [B, D]: fp32 HIP tensors (D = 2 or 3).  `v_start` / `v_goal`: the speed the robot has
    at the start and shall have at the goal -- None (rest), a number, or [B] -> `TimedPaths`.  The poses are copied on the
    device (no synchronisation): the result does not follow later changes of `traj`, `start` or `goal`."""
    _check_paths(traj, start, goal)
    if not traj.is_cuda:
        raise _lib.NfoppError("time_parametrize needs HIP tensors (there is no CPU path)")
    if not isinstance(limits, MotionLimits):
        raise TypeError("limits must be a MotionLimits")
    b, n, d = traj.shape
    v_start, v_goal = (per_row(v, b, traj.device, "a start / goal speed") for v in (v_start, v_goal))
    traj, start, goal = (x.clone(memory_format=torch.contiguous_format) for x in (traj, start, goal))
    f64 = dict(dtype=torch.float64, device=traj.device)
    profile = torch.empty(b, n + 2, _lib.NUM_TIME_SLOTS, **f64)
    gear = torch.empty(b, n + 1, dtype=torch.int8, device=traj.device)
    summary = torch.empty(b, _lib.NUM_TIME_SUMMARY, **f64)
    lim = limits.to_c()
    _lib.check(_lib.load().nfopp_path_time_profile(
        _lib.ptr(traj), _lib.ptr(start), _lib.ptr(goal), b, n, d, lim, _lib.ptr(v_start), _lib.ptr(v_goal),
        _lib.ptr(profile, torch.float64), _lib.ptr(gear, torch.int8), _lib.ptr(summary, torch.float64), _lib.stream_ptr()))
    return TimedPaths(traj, start, goal, limits, profile, gear, summary)
