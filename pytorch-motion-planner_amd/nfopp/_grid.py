"""What the host side of the grid searches shares (grid_search.py, lattice.py, spacetime.py): the frame of a
grid (boundaries, resolution, cell of a point, centre of a cell), what a collision checker says about boundaries and device,
the int32 and workspace idioms in front of a C entry, the table of distinct goals, the sized trace and the seeding launch.
A search keeps what is its own: how a goal packs into a key, its field and trace entries, its path tensors."""
import collections

import numpy as np
import torch

from . import _lib


# ---- the frame ---------------------------------------------------------------------------------------------------------------
def cell_counts(boundaries, resolution):
    # astar_trajectory_initializer.py:29-30
    x_cells = int((boundaries[1] - boundaries[0]) // resolution) + 1
    y_cells = int((boundaries[3] - boundaries[2]) // resolution) + 1
    return x_cells, y_cells


def cell_centres(boundaries, resolution):
    # astar_trajectory_initializer.py:35-37 (float64, x fastest)
    x_cells, y_cells = cell_counts(boundaries, resolution)
    x, y = np.meshgrid(range(x_cells), range(y_cells))
    x = x.reshape(-1) * resolution + resolution / 2 + boundaries[0]
    y = y.reshape(-1) * resolution + resolution / 2 + boundaries[2]
    return x, y, x_cells, y_cells


def heading_poses(x, y, n_headings):
    """The poses a checker is asked at for `n_headings` footprint layers: float32 [n_headings * cells, 3], (cell centre,
    float32(h * 2 pi / n_headings)) for h = 0 .. n_headings - 1, heading slowest (LatticeGrid.from_checker,
    HeadingDistanceField.from_checker)."""
    xy = np.stack([x, y], 1).astype(np.float32)
    return np.concatenate([np.concatenate([xy, np.full((len(xy), 1), np.float32(h * (2 * np.pi) / n_headings), np.float32)], 1)
                           for h in range(n_headings)], 0)


class GridFrame(object):
    """`boundaries` (x0, x1, y0, y1) and `resolution` of the reference's raster: cell of a point = int((x - b0) // resolution),
    cell centre = j * resolution + resolution / 2 + b0 (csrc/grid_frame.h on the device).  OccupancyGrid and LatticeGrid are
    frames with an image."""

    def __init__(self, boundaries, resolution, four_sides=False):
        self.boundaries = tuple(float(b) for b in boundaries)
        if four_sides and len(self.boundaries) != 4:
            raise ValueError("boundaries must be (x0, x1, y0, y1)")
        self.resolution = float(resolution)
        if not self.resolution > 0:
            raise ValueError("resolution must be positive")

    @property
    def origin_resolution(self):
        """(x0, y0, resolution): the three doubles a C entry takes for the frame."""
        return self.boundaries[0], self.boundaries[2], self.resolution

    def cell_counts(self):
        """-> (x cells, y cells)"""
        return cell_counts(self.boundaries, self.resolution)

    def cell_centres(self):
        """-> (x, y, x cells, y cells): the float64 centres of all cells, x fastest."""
        return cell_centres(self.boundaries, self.resolution)

    def cells_of(self, points):
        """[B, >= 2] points (tensor on any device, or array) -> int32 [B, 2] (row, col); float64 floor division as the
        reference's `//`, clamped to +-2^30."""
        b = self.boundaries
        xy = torch.as_tensor(points)[:, :2].double()
        col = torch.floor((xy[:, 0] - b[0]) / self.resolution)
        row = torch.floor((xy[:, 1] - b[2]) / self.resolution)
        lim = float(2 ** 30)
        return torch.stack([row, col], 1).clamp_(-lim, lim).to(torch.int32).contiguous()


def checker_boundaries(checker, boundaries=None):
    """The boundaries a from_checker works with: the given ones, else the checker's own."""
    if boundaries is None:
        boundaries = checker.get_boundaries() if hasattr(checker, "get_boundaries") else getattr(checker, "boundaries", None)
    if boundaries is None:
        raise ValueError("the checker carries no boundaries: pass boundaries=(x0, x1, y0, y1)")
    return tuple(float(b) for b in boundaries)


def checker_device(checker, device=None):
    """The device a device checker is asked on: the given one, else where its grid or its obstacles live."""
    return device or getattr(getattr(checker, "grid", None), "device", None) or \
        getattr(getattr(checker, "obstacles", None), "device", None) or "cuda"


# ---- in front of a C entry ---------------------------------------------------------------------------------------------------
def as_device_points(grid, pts):
    if not torch.is_tensor(pts):
        pts = torch.as_tensor(np.asarray(pts, np.float32))
    if not pts.is_cuda:
        _lib.require_gpu()
        pts = pts.to(grid.device)
    pts = pts.detach().float().contiguous()
    if pts.dim() != 2 or pts.shape[1] not in (2, 3):
        raise ValueError("starts / goals must be [B, 2] or [B, 3]")
    return pts


def int32_on(device, *tensors):
    """-> each of `tensors` (tensor, array or list) as a contiguous int32 tensor on `device`."""
    return [torch.as_tensor(t, dtype=torch.int32, device=device).contiguous() for t in tensors]


Workspace = collections.namedtuple("Workspace", "ptr nbytes buffer")


def workspace(nbytes, device):
    """-> (ptr, nbytes, buffer): the two workspace arguments of a C entry and the buffer behind them, which lives as long as the
    caller holds the result, so for the call.  NULL for 0 bytes.  One allocation of bytes: the entries ask for 8-byte (4-byte:
    nfopp_grid_edt) alignment, which every allocation of torch's device allocator has (it hands out multiples of 512 bytes)."""
    nbytes = int(nbytes)
    if nbytes == 0:
        return Workspace(None, 0, None)
    buffer = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return Workspace(_lib.ptr(buffer, torch.uint8) if buffer.is_cuda else buffer.data_ptr(), nbytes, buffer)


# ---- the goal table ----------------------------------------------------------------------------------------------------------
def cell_keys(cells, shape):
    """Integer cells [B, >= 2] (row, col) on a grid of `shape` (rows, cols) -> (inside bool [B], row * cols + col int64 [B])."""
    rows, cols = shape
    r, c = cells[:, 0].long(), cells[:, 1].long()
    return (r >= 0) & (r < rows) & (c >= 0) & (c < cols), r * cols + c


def goal_table(key):
    """Problems that share a goal share a field.  key int64 [B], -1 for a goal outside the grid -> (the distinct keys ascending
    without the -1, field_index int32 [B]: each problem's entry among them, -1 for outside).  One read-back: uniq[0]."""
    uniq, inverse = torch.unique(key, return_inverse=True)
    if uniq.numel() and int(uniq[0]) < 0:
        uniq, inverse = uniq[1:], inverse - 1
    return uniq, inverse.to(torch.int32).contiguous()


# ---- the sized trace ---------------------------------------------------------------------------------------------------------
def traced_search(b, device, n_fields, chunk, path_tails, fields_of, trace):
    """The search of `b` problems over `n_fields` goal fields, `chunk` of them in memory at a time.
    `fields_of(first, last)` computes the fields first .. last - 1; `trace(fields, first, paths, count, status, cost)` descends
    them for the problems whose field is among them: with paths None it only sizes (writes count, status, cost), else it fills
    `paths`, int32 tensors [b, max_len] + tail for every tail of `path_tails`; fields None = there is no field at all.
    -> (paths, count, status, cost).  Per chunk one sizing pass, one count.max() read-back and one filling pass; the buffers
    grow to the largest count so far and never shrink; what lies behind a row's count is zero.  max_len is at least 1."""
    i32 = dict(dtype=torch.int32, device=device)
    # a trace writes the problems of its own fields and the refused ones, so only with several chunks does a problem read what
    # it was allocated with between two of them
    alloc = torch.zeros if n_fields > chunk else torch.empty
    count, status, cost = alloc(b, **i32), alloc(b, **i32), alloc(b, 2, **i32)
    paths = None

    def sized(max_len):
        grown = [torch.zeros((b, max_len) + tuple(tail), **i32) for tail in path_tails]
        for new, old in zip(grown, paths or ()):
            new[:, :old.shape[1]] = old
        return grown

    if b and not n_fields:
        trace(None, 0, None, count, status, cost)   # every goal is outside the grid: status 2 throughout
    for first in range(0, n_fields if b else 0, chunk):
        fields = fields_of(first, min(first + chunk, n_fields))
        trace(fields, first, None, count, status, cost)
        max_len = max(int(count.max()), 1)   # counts of earlier chunks stay in `count`, so the maximum never falls
        if paths is None or max_len > paths[0].shape[1]:
            paths = sized(max_len)
        trace(fields, first, paths, count, status, cost)
    return paths or sized(1), count, status, cost


# ---- the seeding launch ------------------------------------------------------------------------------------------------------
def seed_launch(workspace_bytes, entry, paths, count, status, starts, goals, n_waypoints, scalars, out):
    """One seeding entry on checked device tensors: entry(*paths, count, status, B, max_len, starts, goals, N, *scalars, out,
    workspace, bytes, stream) -> out as [B, N, D].  `paths` are the entry's own path tensors [B, max_len, ...]."""
    b, d = starts.shape
    n, max_len = int(n_waypoints), paths[0].shape[1]
    if out is None:
        out = torch.empty(b, n, d, dtype=torch.float32, device=starts.device)
    elif out.numel() != b * n * d or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous fp32 tensor of B * N * D elements")
    ws = workspace(workspace_bytes(b, max_len), starts.device)
    i32 = torch.int32
    _lib.check(entry(*[_lib.ptr(t, t.dtype) for t in paths], _lib.ptr(count, i32), _lib.ptr(status, i32), b, max_len,
                     _lib.ptr(starts), _lib.ptr(goals), n, *scalars, _lib.ptr(out), ws.ptr, ws.nbytes, _lib.stream_ptr()))
    return out.view(b, n, d)
