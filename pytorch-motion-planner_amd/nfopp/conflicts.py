"""Conflicts between timed tracks (csrc/track_conflict.hip): which robots of a fleet come closer than their radii allow, when
first and with whom, and the same for timed paths against predicted tracks of moving obstacles -- all pairs, on the device.
`box_track_conflicts` (csrc/box_conflict.hip) is the same question for oriented boxes on SE(2) tracks.
The rules are stated in include/nfopp_hip.h; nothing here synchronises when the inputs are device tensors."""
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


class BoxTrackConflicts(object):
    """What `box_track_conflicts` found.  Device tensors: `summary` [Ba, 7] float64 (FIRST_TIME: the first conflict with any
    partner, +inf if none; FIRST_PARTNER; CONFLICTS: partners in conflict; UNDECIDED_TIME: the first instant some pair was left
    undecided, +inf if none; UNDECIDED_PARTNER; UNDECIDED: partners left undecided; STATUS as for `TrackConflicts`),
    `summary_b` [Bb, 7] the same from set B's side (None in self mode), and with `want_pairs` `pair_status` [Ba, Bb] int32
    (FREE, CONFLICT, UNDECIDED; BAD for a pair with a bad track), `pair_first` / `pair_undecided` [Ba, Bb] float64, else None."""
    FIRST_TIME, FIRST_PARTNER, CONFLICTS, UNDECIDED_TIME, UNDECIDED_PARTNER, UNDECIDED, STATUS = range(_lib.NUM_BOX_CONFLICT_SLOTS)
    BAD_TRACK, NO_PARTNER = CONFLICT_BAD_TRACK, CONFLICT_NO_PARTNER
    BAD, FREE, CONFLICT, UNDECIDED_PAIR = -1, 0, 1, 2

    def __init__(self, summary, summary_b=None, pair_status=None, pair_first=None, pair_undecided=None):
        self.summary, self.summary_b = summary, summary_b
        self.pair_status, self.pair_first, self.pair_undecided = pair_status, pair_first, pair_undecided

    @property
    def in_conflict(self):
        """[Ba] bool device tensor: the tracks of set A with at least one partner in conflict."""
        return self.summary[:, self.CONFLICTS] > 0

    @property
    def undecided(self):
        """[Ba] bool device tensor: the tracks of set A with at least one partner left undecided."""
        return self.summary[:, self.UNDECIDED] > 0


def track_headings(tracks):
    """tracks [B, K, >= 3] fp32 HIP tensor, x, y, theta first in a row -> [B, K, 2] float64 (cos theta, sin theta): the
    headings pass of `box_track_conflicts` (nfopp_track_headings)."""
    b, k, stride = check_tracks(tracks, "tracks")
    if tracks.shape[2] < 3:
        raise ValueError("tracks must be [B, K, >= 3] (x, y, theta), got %s" % (tuple(tracks.shape),))
    device = hip_device("track_headings", "tracks", tracks)
    out = torch.empty(b, k, 2, dtype=torch.float64, device=device)
    _lib.check(_lib.load().nfopp_track_headings(raw_ptr(tracks), b, stride, k, _lib.ptr(out, torch.float64), _lib.stream_ptr()))
    return out


def _per_row_boxes(box, batch, device, name):
    """One box (x0, x1, y0, y1) or [B, 4] -> a [B, 4] fp32 device tensor (a tensor is not copied to the host)."""
    if isinstance(box, torch.Tensor):
        box = box.to(device=device, dtype=torch.float32)
    else:
        box = torch.from_numpy(np.array(box, np.float32)).to(device)
    if box.numel() == 4:
        box = box.reshape(1, 4)
    if box.dim() != 2 or box.shape[1] != 4 or box.shape[0] not in (1, batch):
        raise ValueError("%s must be one box (x0, x1, y0, y1) or [B, 4] = [%d, 4], got %s" % (name, batch, tuple(box.shape)))
    return box.expand(batch, 4).contiguous()


def box_track_conflicts(tracks_a, tracks_b=None, *, dt, t0=0.0, box_a, box_b=None, radius_a=0.0, radius_b=None, margin=0.0,
                        refine=0, want_pairs=False):
    """tracks_a [Ba, K, >= 3], tracks_b [Bb, K, >= 3] or None: fp32 HIP tensors of poses at t0 + k * dt, x, y, theta first in a
    row (`TimedPaths.sample` returns such a tensor for SE(2) paths).  Without `tracks_b` the tracks of A are checked against
    each other.  `box_a` / `box_b`: one box (x0, x1, y0, y1) in the body frame or [B, 4]; `radius_a` / `radius_b`: a rounding
    radius, a number or [B]; `margin` is added to every sum of radii; `refine` (0 .. 8) is how often an interval that the
    certificate leaves undecided is halved.  -> `BoxTrackConflicts`."""
    ba, k, stride_a = check_tracks(tracks_a, "tracks_a")
    self_mode = tracks_b is None
    bb, stride_b = 0, 3
    if not self_mode:
        bb, kb, stride_b = check_tracks(tracks_b, "tracks_b")
        if kb != k:
            raise ValueError("tracks_a and tracks_b must share the time grid: K = %d and %d" % (k, kb))
        if box_b is None:
            raise ValueError("tracks_b needs box_b")
    if tracks_a.shape[2] < 3 or (not self_mode and tracks_b.shape[2] < 3):
        raise ValueError("box tracks must be [B, K, >= 3] (x, y, theta)")
    refine = int(refine)
    if not 0 <= refine <= _lib.BOX_CONFLICT_MAX_REFINE:
        raise ValueError("refine must be 0 .. %d, got %d" % (_lib.BOX_CONFLICT_MAX_REFINE, refine))
    device = hip_device("box_track_conflicts", "tracks_a", tracks_a, "tracks_b", tracks_b)
    box_a = _per_row_boxes(box_a, ba, device, "box_a")
    box_b = None if self_mode else _per_row_boxes(box_b, bb, device, "box_b")
    radius_a = per_row(radius_a, ba, device, "radius_a")
    radius_b = None if self_mode else per_row(radius_b, bb, device, "radius_b")
    heading_a = track_headings(tracks_a)
    heading_b = None if self_mode else track_headings(tracks_b)
    lib = _lib.load()
    f64 = dict(dtype=torch.float64, device=device)
    cols = ba if self_mode else bb
    summary = torch.empty(ba, _lib.NUM_BOX_CONFLICT_SLOTS, **f64)
    summary_b = None if self_mode else torch.empty(bb, _lib.NUM_BOX_CONFLICT_SLOTS, **f64)
    pair_status = torch.empty(ba, cols, dtype=torch.int32, device=device) if want_pairs else None
    pair_first = torch.empty(ba, cols, **f64) if want_pairs else None
    pair_undecided = torch.empty(ba, cols, **f64) if want_pairs else None
    ws = workspace(lib.nfopp_box_track_conflicts_workspace_bytes(ba, bb, k), device)
    # a set of no obstacles still needs a non-null pointer (null selects self mode); it is never read
    b_ptr = None if self_mode else (raw_ptr(tracks_b) or raw_ptr(tracks_a))
    _lib.check(lib.nfopp_box_track_conflicts(
        raw_ptr(tracks_a), _lib.ptr(heading_a, torch.float64), ba, stride_a, b_ptr, _lib.ptr(heading_b, torch.float64), bb, stride_b,
        k, float(t0), float(dt), _lib.ptr(box_a), _lib.ptr(box_b), _lib.ptr(radius_a), _lib.ptr(radius_b), float(margin), refine,
        _lib.ptr(summary, torch.float64), _lib.ptr(summary_b, torch.float64), _lib.ptr(pair_status, torch.int32),
        _lib.ptr(pair_first, torch.float64), _lib.ptr(pair_undecided, torch.float64), ws.ptr, ws.nbytes, _lib.stream_ptr()))
    if ba == 0 and bb > 0:      # the entry writes nothing for an empty set A: every obstacle is without a partner
        summary_b[:] = torch.tensor([np.inf, -1.0, 0.0, np.inf, -1.0, 0.0, CONFLICT_NO_PARTNER], **f64)
    return BoxTrackConflicts(summary, summary_b, pair_status, pair_first, pair_undecided)


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


def box_reach(box):
    """Largest distance from the body origin to a corner of one box (x0, x1, y0, y1)."""
    x0, x1, y0, y1 = (float(v) for v in box)
    return float(np.hypot(max(abs(x0), abs(x1)), max(abs(y0), abs(y1))))


def box_disc_radius(box, radius, batch, device):
    """[B] fp32 device tensor: the radius of the disc about the body origin that covers each rounded box at every heading --
    the farthest corner, times 1.000001 as the box check's reach, plus the rounding radius -- for callers that reserve
    discs (the space-time search).  `box`: one box or [B, 4]; `radius`: None, a number or [B].  Nothing is copied to the host."""
    box = _per_row_boxes(box, batch, device, "box")
    reach = torch.hypot(box[:, :2].abs().amax(1), box[:, 2:].abs().amax(1)) * 1.000001
    return reach + per_row(0.0 if radius is None else radius, batch, device, "radius")


def box_chord_margin(va_max, vb_max, dt, reach_a, wa_max, reach_b, wb_max):
    """`chord_margin` for boxes: a point at up to `reach` from the origin of a body that turns at up to w_max moves at up to
    v_max + reach * w_max, which adds reach * w_max * dt / 2 per side."""
    return chord_margin(va_max, vb_max, dt) + (float(reach_a) * float(wa_max) + float(reach_b) * float(wb_max)) * float(dt) / 2.0
