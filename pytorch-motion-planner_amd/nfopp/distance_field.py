"""The distance-field collision model (csrc/sdf_field.hip): planning on an occupancy grid without fitting an ONF.

`DistanceField(grid, ...)` holds the grid's signed distance image and a robot of discs, and stands where an ONF stands in
`TrajectoryEngine` and `BatchPlanner`: every collision sample gets a logit gain * ((radius + margin) - distance) and its
gradient from one bilinear tap per disc -- the obstacle cost of CHOMP and GPMP2 -- and the rest of the step (update,
multipliers, Adam, reparametrisation) runs as it does behind the network."""
import numpy as np
import torch

from . import _lib

MAX_DISCS = 8


class DistanceField(object):
    """grid: an OccupancyGrid of at least 2 x 2 cells.  The robot: `radius` (one disc at the body origin) or `discs`
    [(ox, oy, r), ...], up to 8 in the body frame (`discs_for_box` covers a box); with dim = 2 (no heading) one centred
    disc only.  `margin` (metres) is added to every radius; `gain` is the logit per metre of penetration, by default
    1 / resolution: one logit per cell.  `border` counts the outside of the grid as wall (OccupancyGrid.signed_distance_field).

    Attributes: `point_dim` (= dim), `field` (the fp32 [rows, cols] image on the device)."""

    def __init__(self, grid, radius=None, discs=None, margin=0.0, gain=None, dim=3, border=False):
        if (radius is None) == (discs is None):
            raise TypeError("DistanceField takes radius= (one centred disc) or discs= [(ox, oy, r), ...], not both and not neither")
        discs = np.array([[0.0, 0.0, float(radius)]] if discs is None else discs, dtype=np.float64)
        if discs.ndim != 2 or discs.shape[1] != 3 or not 1 <= len(discs) <= MAX_DISCS:
            raise ValueError("discs must be [1..%d, 3]: (ox, oy, r) per disc" % MAX_DISCS)
        if not np.isfinite(discs).all() or (discs[:, 2] < 0).any():
            raise ValueError("disc offsets must be finite and radii finite and >= 0")
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        if dim == 2 and (len(discs) != 1 or discs[0, 0] != 0 or discs[0, 1] != 0):
            raise ValueError("a robot without a heading (dim 2) is one disc with a zero offset")
        rows, cols = grid.shape
        if rows < 2 or cols < 2:
            raise ValueError("a distance field needs a grid of at least 2 x 2 cells")
        self.point_dim = int(dim)
        self.discs, self.margin, self.border = discs, float(margin), bool(border)
        self.gain = 1.0 / grid.resolution if gain is None else float(gain)
        self.boundaries, self.resolution, self.shape = tuple(grid.boundaries), float(grid.resolution), (rows, cols)
        self.field = grid.signed_distance_field(self.border).clone()
        c = self._c = _lib.SdfFieldC()
        c.sd_dev = _lib.ptr(self.field)
        c.rows, c.cols = rows, cols
        # each of the three rounded once from double, by the assignment to a float field
        c.x0, c.y0, c.inv_res = self.boundaries[0], self.boundaries[2], 1.0 / self.resolution
        c.n_discs = len(discs)
        for k, disc in enumerate(discs):
            for m in range(3):
                c.disc[k][m] = disc[m]
        c.margin, c.gain = self.margin, self.gain

    def config_c(self):
        """The nfopp_sdf_field block of the C entries (the image is borrowed: it lives as long as this object)."""
        return self._c

    def update(self, grid):
        """A new occupancy in the same frame (shape, boundaries, resolution): the image is re-derived into the buffer it
        already has, so engines and planners built on this field see the new map at their next step."""
        if tuple(grid.shape) != self.shape or tuple(grid.boundaries) != self.boundaries or float(grid.resolution) != self.resolution:
            raise ValueError("update() takes a grid of the same shape, boundaries and resolution")
        self.field.copy_(grid.signed_distance_field(self.border))

    def eval(self, points, out=None):
        """points [P, point_dim] (fp32 device tensor, or an array: one upload) -> fp32 [P, 4] on the device: logit and its
        gradient in x, y, theta per pose (nfopp_sdf_eval_points)."""
        if not torch.is_tensor(points):
            points = torch.as_tensor(np.asarray(points, np.float32)).to(self.field.device)
        points = points.detach().float().contiguous()
        if points.dim() != 2 or points.shape[1] != self.point_dim:
            raise ValueError("points must be [P, %d]" % self.point_dim)
        p = points.shape[0]
        if out is None:
            out = torch.empty(p, 4, dtype=torch.float32, device=points.device)
        elif out.numel() != 4 * p:
            raise ValueError("out must hold [P, 4] fp32")
        _lib.check(_lib.load().nfopp_sdf_eval_points(self._c, _lib.ptr(points), p, self.point_dim, _lib.ptr(out),
                                                     _lib.stream_ptr()))
        return out.view(p, 4)

    @staticmethod
    def discs_for_box(box, n):
        """`n` equal discs along the longer axis of the body-frame box (x0, x1, y0, y1), at the centres of its n equal
        parts, with the smallest radius at which they cover the box: each disc covers its own part, half of whose diagonal
        it is.  -> float64 [n, 3] (ox, oy, r)."""
        x0, x1, y0, y1 = (float(b) for b in box)
        n = int(n)
        if not (x1 >= x0 and y1 >= y0) or not 1 <= n <= MAX_DISCS:
            raise ValueError("box must be (x0, x1, y0, y1) with x1 >= x0, y1 >= y0, and 1 <= n <= %d" % MAX_DISCS)
        along = (np.arange(n) + 0.5) / n
        discs = np.empty((n, 3))
        if x1 - x0 >= y1 - y0:
            discs[:, 0], discs[:, 1] = x0 + along * (x1 - x0), 0.5 * (y0 + y1)
            part, width = (x1 - x0) / n, y1 - y0
        else:
            discs[:, 0], discs[:, 1] = 0.5 * (x0 + x1), y0 + along * (y1 - y0)
            part, width = (y1 - y0) / n, x1 - x0
        discs[:, 2] = 0.5 * np.hypot(part, width)
        return discs
