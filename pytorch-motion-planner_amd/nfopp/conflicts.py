"""Conflicts between timed tracks (csrc/track_conflict.hip): which robots of a fleet come closer than their radii allow, when
first and with whom, and the same for timed paths against predicted tracks of moving obstacles -- all pairs, on the device.
The rule is stated in include/nfopp_hip.h; nothing here synchronises when the inputs are device tensors."""
import numpy as np
import torch

from . import _lib
from ._grid import workspace
from ._tracks import check_tracks, hip_device, per_row, raw_ptr

# slots of TrackConflicts.summary [B, 7] (NFOPP_CONFLICT_SLOT_*)
(CONFLICT_MIN_GAP, CONFLICT_MIN_PARTNER, CONFLICT_MIN_TIME, CONFLICT_FIRST_TIME, CONFLICT_FIRST_PARTNER, CONFLICT_COUNT,
 CONFLICT_STATUS) = range(_lib.NUM_CONFLICT_SLOTS)
# values of the status slot (NFOPP_CONFLICT_*)
CONFLICT_BAD_TRACK, CONFLICT_NO_PARTNER = 1, 2


class TrackConflicts(object):
    """What `track_conflicts` found.  Device tensors, float64: `summary` [Ba, 7] (CONFLICT_*: the smallest gap to any partner,
    that partner, the time of that closest approach, the time of the first conflict (+inf: none), its partner, the number of
    partners in conflict, status), `summary_b` [Bb, 7] the same from set B's side (None in self mode), and with `want_pairs`
    `pair_gap` / `pair_first` [Ba, Bb]: gap and first-conflict time of every pair (self mode: symmetric, +inf on the
    diagonal), else None."""
    MIN_GAP, MIN_PARTNER, MIN_TIME, FIRST_TIME, FIRST_PARTNER, COUNT, STATUS = range(_lib.NUM_CONFLICT_SLOTS)
    BAD_TRACK, NO_PARTNER = CONFLICT_BAD_TRACK, CONFLICT_NO_PARTNER

    def __init__(self, summary, summary_b=None, pair_gap=None, pair_first=None):
        self.summary, self.summary_b, self.pair_gap, self.pair_first = summary, summary_b, pair_gap, pair_first

    @property
    def in_conflict(self):
        """[Ba] bool device tensor: the tracks of set A with at least one partner in conflict."""
        return self.summary[:, CONFLICT_COUNT] > 0


def track_conflicts(tracks_a, tracks_b=None, *, dt, t0=0.0, radius_a=0.0, radius_b=None, margin=0.0, want_pairs=False):
    """tracks_a [Ba, K, >= 2], tracks_b [Bb, K, >= 2] or None: fp32 HIP tensors of positions at t0 + k * dt, x and y first in a
    row (`TimedPaths.sample` returns such a tensor).  Without `tracks_b` the tracks of A are checked against each other.
    `radius_a` / `radius_b`: a number or [B] (metres; a box robot takes its circumscribed disc); `margin` is added to every
    sum of radii -- put (va_max + vb_max) * dt / 2 there to cover what the robots do between two instants.
    -> `TrackConflicts`."""
    ba, k, stride_a = check_tracks(tracks_a, "tracks_a")
    self_mode = tracks_b is None
    bb, stride_b = 0, 2
    if not self_mode:
        bb, kb, stride_b = check_tracks(tracks_b, "tracks_b")
        if kb != k:
            raise ValueError("tracks_a and tracks_b must share the time grid: K = %d and %d" % (k, kb))
    device = hip_device("track_conflicts", "tracks_a", tracks_a, "tracks_b", tracks_b)
    radius_a = per_row(radius_a, ba, device, "radius_a")
    radius_b = None if self_mode else per_row(radius_b, bb, device, "radius_b")
    lib = _lib.load()
    f64 = dict(dtype=torch.float64, device=device)
    cols = ba if self_mode else bb
    summary = torch.empty(ba, _lib.NUM_CONFLICT_SLOTS, **f64)
    summary_b = None if self_mode else torch.empty(bb, _lib.NUM_CONFLICT_SLOTS, **f64)
    pair_gap = torch.empty(ba, cols, **f64) if want_pairs else None
    pair_first = torch.empty(ba, cols, **f64) if want_pairs else None
    ws = workspace(lib.nfopp_track_conflicts_workspace_bytes(ba, bb, k), device)
    # a set of no obstacles still needs a non-null pointer (null selects self mode); it is never read
    b_ptr = None if self_mode else (raw_ptr(tracks_b) or raw_ptr(tracks_a))
    _lib.check(lib.nfopp_track_conflicts(
        raw_ptr(tracks_a), ba, stride_a, b_ptr, bb, stride_b, k, float(t0), float(dt), _lib.ptr(radius_a), _lib.ptr(radius_b),
        float(margin), _lib.ptr(summary, torch.float64), _lib.ptr(summary_b, torch.float64), _lib.ptr(pair_gap, torch.float64),
        _lib.ptr(pair_first, torch.float64), ws.ptr, ws.nbytes, _lib.stream_ptr()))
    if ba == 0 and bb > 0:      # the entry writes nothing for an empty set A: every obstacle is without a partner
        summary_b[:] = torch.tensor([np.inf, -1.0, np.nan, np.inf, -1.0, 0.0, CONFLICT_NO_PARTNER], **f64)
    return TrackConflicts(summary, summary_b, pair_gap, pair_first)


def constant_velocity_tracks(p0, velocity, dt, count, t0=0.0):
    """p0 [M, 2], velocity [M, 2] (tensors, any float type) -> [M, count, 2] fp32: the positions p0 + velocity * t at
    t = t0 + k * dt, k = 0 .. count - 1, with p0 the position at t = 0 -- the predicted-obstacle form a tracker hands over."""
    p0, velocity = torch.as_tensor(p0), torch.as_tensor(velocity)
    if p0.dim() != 2 or p0.shape[1] != 2 or tuple(velocity.shape) != tuple(p0.shape):
        raise ValueError("p0 and velocity must be [M, 2], got %s and %s" % (tuple(p0.shape), tuple(velocity.shape)))
    t = float(t0) + torch.arange(int(count), dtype=torch.float64, device=p0.device) * float(dt)
    return (p0.double()[:, None, :] + velocity.double().to(p0.device)[:, None, :] * t[None, :, None]).float()


def chord_margin(va_max, vb_max, dt):
    """What linearity between two instants costs: two points moving at up to va_max and vb_max stay within
    (va_max + vb_max) * dt / 2 of their chords' distance."""
    return (float(va_max) + float(vb_max)) * float(dt) / 2.0
