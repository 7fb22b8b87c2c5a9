"""The heading-layered distance field (csrc/heading_field.hip): planning for a robot of any shape on an
occupancy grid, with no network to fit and no discs to cover the robot with.

`HeadingDistanceField(layers, ...)` holds L occupancy slices -- slice k is what the robot's footprint leaves free at the heading
k * 2 pi / L, as a device checker answers it (`from_checker`) -- and the signed distance image of each.  Stacked, they are the
signed distance of the robot's configuration space: how far the centre may move at this heading before the checker says
"collision".  It stands where an ONF or a `DistanceField` stands in `TrajectoryEngine` and `BatchPlanner`: every collision
sample gets the logit gain * (margin - distance) and its gradient in x, y and theta from one trilinear tap.

Between two slices the distance is interpolated, so a long robot at a heading between them is judged by its two neighbours:
choose L and `margin` for the robot's length."""
import numpy as np
import torch

from . import _lib
from ._grid import cell_centres, checker_boundaries, checker_device, heading_poses
from .grid_search import OccupancyGrid

MIN_LAYERS, MAX_LAYERS = 2, 64


class HeadingDistanceField(object):
    """layers: uint8 occupancy slices [L, rows, cols] (array or device tensor, non-zero = blocked), L in 2 .. 64, at least
    2 x 2 cells; slice k belongs to the heading k * 2 pi / L.  `boundaries` (x0, x1, y0, y1) and `resolution` are the frame of
    OccupancyGrid.  `margin` (metres) is the clearance asked for; `gain` is the logit per metre, by default 1 / resolution: one
    logit per cell.  `border` counts the outside of the grid as blocked (OccupancyGrid.signed_distance_field).

    Attributes: `point_dim` (3: the poses are SE(2)), `field` (the fp32 [L, rows, cols] image on the device)."""

    point_dim = 3

    def __init__(self, layers, boundaries, resolution, margin=0.0, gain=None, border=False, device="cuda"):
        boundaries = tuple(float(b) for b in boundaries)
        resolution = float(resolution)
        if len(boundaries) != 4 or not np.isfinite(boundaries).all():
            raise ValueError("boundaries must be four finite numbers (x0, x1, y0, y1)")
        if not (resolution > 0 and np.isfinite(resolution)):
            raise ValueError("resolution must be positive and finite")
        self.margin, self.border = float(margin), bool(border)
        self.gain = 1.0 / resolution if gain is None else float(gain)
        if not (np.isfinite(self.margin) and np.isfinite(self.gain)):
            raise ValueError("margin and gain must be finite")
        self.boundaries, self.resolution = boundaries, resolution
        self.shape = self._checked_shape(layers)
        n_layers, rows, cols = self.shape
        self.n_layers = n_layers
        occ = self._on_device(layers, device)
        self.field = torch.empty(n_layers, rows, cols, dtype=torch.float32, device=occ.device)
        self._derive(occ)
        c = self._c = _lib.HeadingFieldC()
        c.sd_dev = _lib.ptr(self.field)
        c.layers, c.rows, c.cols = n_layers, rows, cols
        # each rounded once from double, by the assignment to a float field
        c.x0, c.y0, c.inv_res = boundaries[0], boundaries[2], 1.0 / resolution
        c.layers_per_rad = n_layers / (2 * np.pi)
        c.margin, c.gain = self.margin, self.gain

    @staticmethod
    def _checked_shape(layers):
        if torch.is_tensor(layers) and layers.dtype != torch.uint8:
            raise ValueError("layers must be uint8")
        shape = tuple(layers.shape) if torch.is_tensor(layers) else np.shape(layers)
        if len(shape) != 3 or not MIN_LAYERS <= shape[0] <= MAX_LAYERS or shape[1] < 2 or shape[2] < 2:
            raise ValueError("layers must be [L, rows, cols] with L in %d .. %d and at least 2 x 2 cells" % (MIN_LAYERS, MAX_LAYERS))
        if shape[0] * shape[1] * shape[2] > 2 ** 31 - 1:
            raise ValueError("L * rows * cols must fit a 32-bit index")
        return tuple(int(s) for s in shape)

    @staticmethod
    def _on_device(layers, device):
        """-> the slices as a contiguous uint8 0 / 1 device tensor."""
        if torch.is_tensor(layers) and layers.is_cuda:
            return (layers != 0).to(torch.uint8).contiguous()
        _lib.require_gpu()
        host = np.ascontiguousarray(np.asarray(layers.numpy() if torch.is_tensor(layers) else layers) != 0, dtype=np.uint8)
        return torch.tensor(host, device=device)

    def _derive(self, occ):
        """Slice by slice: the signed distance image of OccupancyGrid, written into the buffer this field owns."""
        for k in range(self.n_layers):
            grid = OccupancyGrid._from_device(occ[k], self.boundaries, self.resolution)
            self.field[k].copy_(grid.signed_distance_field(self.border))

    @classmethod
    def from_checker(cls, checker, resolution, layers=16, boundaries=None, device=None, **kw):
        """L slices from one `labels` call of a device checker over L * cells poses (cell centre, float32(k * 2 pi / L)): the
        robot's footprint per heading comes from the checker's own kernels, as in LatticeGrid.from_checker."""
        boundaries = checker_boundaries(checker, boundaries)
        occ = cls._labels_of(checker, boundaries, resolution, layers, checker_device(checker, device))
        return cls(occ, boundaries, resolution, **kw)

    @staticmethod
    def _labels_of(checker, boundaries, resolution, n_layers, device):
        if resolution is None:
            raise TypeError("from_checker() needs a resolution")
        if not hasattr(checker, "labels"):
            raise TypeError("HeadingDistanceField.from_checker needs a device checker (one with `labels`)")
        n_layers = int(n_layers)
        if not MIN_LAYERS <= n_layers <= MAX_LAYERS:
            raise ValueError("layers must be %d .. %d" % (MIN_LAYERS, MAX_LAYERS))
        x, y, x_cells, y_cells = cell_centres(boundaries, resolution)
        labels = checker.labels(torch.tensor(heading_poses(x, y, n_layers), device=device))
        return (labels > 0).to(torch.uint8).reshape(n_layers, y_cells, x_cells)

    @classmethod
    def from_lattice(cls, lgrid, **kw):
        """The eight footprint layers of a LatticeGrid (LatticeGrid.from_checker) as an 8-slice field."""
        if lgrid.n_layers != 8:
            raise ValueError("from_lattice() takes a LatticeGrid of 8 layers, not %d" % lgrid.n_layers)
        return cls(lgrid.layers, lgrid.boundaries, lgrid.resolution, **kw)

    def config_c(self):
        """The nfopp_heading_field block of the C entries (the image is borrowed: it lives as long as this object)."""
        return self._c

    def update(self, layers):
        """New occupancy slices in the same frame and of the same shape: the image is re-derived into the buffer it already
        has, so engines and planners built on this field see the new map at their next step."""
        if self._checked_shape(layers) != self.shape:
            raise ValueError("update() takes layers of the same shape %s" % (self.shape,))
        self._derive(self._on_device(layers, self.field.device))

    def update_from_checker(self, checker):
        """update() with the slices a device checker gives in this field's frame (from_checker's one `labels` call)."""
        occ = self._labels_of(checker, self.boundaries, self.resolution, self.n_layers, self.field.device)
        if tuple(occ.shape) != self.shape:
            raise ValueError("the checker's raster does not have this field's shape")
        self._derive(occ)

    def eval(self, points, out=None):
        """points [P, 3] (fp32 device tensor, or an array: one upload) -> fp32 [P, 4] on the device: logit and its gradient
        in x, y, theta per pose (nfopp_hdf_eval_points)."""
        if not torch.is_tensor(points):
            points = torch.as_tensor(np.asarray(points, np.float32)).to(self.field.device)
        points = points.detach().float().contiguous()
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be [P, 3]")
        p = points.shape[0]
        if out is None:
            out = torch.empty(p, 4, dtype=torch.float32, device=points.device)
        elif out.numel() != 4 * p:
            raise ValueError("out must hold [P, 4] fp32")
        _lib.check(_lib.load().nfopp_hdf_eval_points(self._c, _lib.ptr(points), p, _lib.ptr(out), _lib.stream_ptr()))
        return out.view(p, 4)
