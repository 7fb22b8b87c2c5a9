"""The moving-obstacle collision term (csrc/track_field.hip): predicted tracks inside the optimisation step.

`MovingObstacles(tracks, dt, ...)` holds M predicted tracks [M, K, >= 2] on a uniform time grid -- `constant_velocity_tracks`,
or `TimedPaths.sample` of robots already scheduled -- and a robot of discs.  Handed to `BatchPlanner(..., moving=)` together
with waypoint times, it makes every step look at where each obstacle is at the moment the robot is at the sample: a row of the
static collision model (ONF, `DistanceField`, `HeadingDistanceField`) is replaced wherever a moving obstacle penetrates deeper."""
import numpy as np
import torch

from . import _lib
from ._tracks import check_tracks, hip_device, per_row, raw_ptr
from .distance_field import MAX_DISCS


class MovingObstacles(object):
    """tracks: fp32 HIP tensor [M, K, >= 2], positions at t0 + k * dt, x and y first in a row (borrowed, not copied: see
    `update`).  `radius`: the obstacles' radii, a number or [M].  The robot: `robot_radius` (one disc at the body origin) or
    `discs` [(ox, oy, r), ...], up to 8 in the body frame; with dim = 2 one centred disc only.  `margin` (metres) is added to
    every sum of radii -- `nfopp.conflicts.chord_margin` is what linearity between two instants costs; `gain` is the logit per
    metre of penetration (default 10).  Every argument is checked before the device is touched."""

    def __init__(self, tracks, dt, t0=0.0, radius=0.0, robot_radius=None, discs=None, margin=0.0, gain=10.0, dim=3):
        if (robot_radius is None) == (discs is None):
            raise TypeError("MovingObstacles takes robot_radius= (one centred disc) or discs= [(ox, oy, r), ...], not both and not neither")
        discs = np.array([[0.0, 0.0, float(robot_radius)]] if discs is None else discs, dtype=np.float64)
        if discs.ndim != 2 or discs.shape[1] != 3 or not 1 <= len(discs) <= MAX_DISCS:
            raise ValueError("discs must be [1..%d, 3]: (ox, oy, r) per disc" % MAX_DISCS)
        if not np.isfinite(discs).all() or (discs[:, 2] < 0).any():
            raise ValueError("disc offsets must be finite and radii finite and >= 0")
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        if dim == 2 and (len(discs) != 1 or discs[0, 0] != 0 or discs[0, 1] != 0):
            raise ValueError("a robot without a heading (dim 2) is one disc with a zero offset")
        dt, t0, margin, gain = float(dt), float(t0), float(margin), float(gain)
        if not (np.isfinite(dt) and dt > 0 and np.isfinite(np.float32(1.0 / dt))):
            raise ValueError("dt must be positive and finite")
        if not (np.isfinite(np.float32(t0)) and np.isfinite(np.float32(margin)) and np.isfinite(np.float32(gain))):
            raise ValueError("t0, margin and gain must be finite")
        m, k, stride = self._checked(tracks)
        if (radius.numel() if isinstance(radius, torch.Tensor) else np.size(radius)) not in (1, m):
            raise ValueError("radius must be a number or [M] = [%d]" % m)
        self.point_dim, self.discs, self.dt, self.margin, self.gain = int(dim), discs, dt, margin, gain
        device = hip_device("MovingObstacles", "tracks", tracks)
        self.radius = per_row(radius, m, device, "radius")
        c = self._c = _lib.TrackFieldC()
        c.radius_dev = _lib.ptr(self.radius)
        # each rounded once from double, by the assignment to a float field
        c.inv_dt = 1.0 / dt
        c.n_discs = len(discs)
        for j, disc in enumerate(discs):
            for i in range(3):
                c.disc[j][i] = disc[i]
        c.margin, c.gain = margin, gain
        self._bind(tracks, (m, k, stride), t0)

    @staticmethod
    def _checked(tracks):
        m, k, stride = check_tracks(tracks, "tracks")
        if m * k * stride > 2 ** 31 - 1:
            raise ValueError("M * K * stride must fit a 32-bit index")
        return m, k, stride

    def _bind(self, tracks, shape, t0):
        self.tracks, self.shape, self.t0 = tracks, shape, float(t0)
        c = self._c
        c.tracks_dev = raw_ptr(tracks)
        c.m, c.k, c.stride = shape
        c.t0 = self.t0

    def config_c(self):
        """The nfopp_track_field block of the C entries (tracks and radii are borrowed: they live as long as this object)."""
        return self._c

    def update(self, tracks, t0=None):
        """New predictions, for receding-horizon use.  Tracks of the shape and layout held so far are copied into the tensor
        this object holds (the same `data_ptr`: engines, and work already enqueued behind the copy, see the new tracks); any
        other [M, K, >= 2] with the same M is taken over as it is.  `t0`: the time of the new first instant (None: as before)."""
        t0 = self.t0 if t0 is None else float(t0)
        if not np.isfinite(np.float32(t0)):
            raise ValueError("t0 must be finite")
        shape = self._checked(tracks)
        if shape[0] != self.shape[0]:
            raise ValueError("update() takes tracks of the same obstacles: M = %d, not %d" % (self.shape[0], shape[0]))
        hip_device("MovingObstacles.update", "tracks", tracks, "the held tracks", self.tracks)
        if shape == self.shape and tuple(tracks.shape) == tuple(self.tracks.shape):
            self.tracks.copy_(tracks)
            tracks = self.tracks
        self._bind(tracks, shape, t0)

    def eval(self, points, times, base=None, out=None):
        """points [P, dim] and times [P] (fp32 device tensors, or arrays: one upload each) -> fp32 [P, 4] on the device: per
        pose the row of `base` [P, 4], replaced by the track row where that one's logit is larger
        (nfopp_track_field_eval_points).  `base=None` stands for rows of logit -inf: the pure track row comes back (and a row
        of -inf, 0, 0, 0 where no track gives one: no obstacles, or a pose or time that is not finite)."""
        device = self.tracks.device
        if not torch.is_tensor(points):
            points = torch.as_tensor(np.asarray(points, np.float32)).to(device)
        if not torch.is_tensor(times):
            times = torch.as_tensor(np.asarray(times, np.float32)).to(device)
        points, times = points.detach().float().contiguous(), times.detach().float().contiguous()
        if points.dim() != 2 or points.shape[1] != self.point_dim:
            raise ValueError("points must be [P, %d]" % self.point_dim)
        p = points.shape[0]
        if times.numel() != p:
            raise ValueError("times must be [P] = [%d]" % p)
        if out is None:
            out = torch.empty(p, 4, dtype=torch.float32, device=device)
        elif out.numel() != 4 * p:
            raise ValueError("out must hold [P, 4] fp32")
        if base is None:
            out.view(p, 4).copy_(torch.tensor([-np.inf, 0.0, 0.0, 0.0], device=device))
        else:
            if not torch.is_tensor(base):
                base = torch.as_tensor(np.asarray(base, np.float32)).to(device)
            if base.numel() != 4 * p:
                raise ValueError("base must be [P, 4]")
            out.view(p, 4).copy_(base.view(p, 4))
        _lib.check(_lib.load().nfopp_track_field_eval_points(self._c, _lib.ptr(points), _lib.ptr(times), p, self.point_dim,
                                                             _lib.ptr(out), _lib.stream_ptr()))
        return out.view(p, 4)
