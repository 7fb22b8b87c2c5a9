"""CPU-only tests of the obstacle-map path: the numpy restatement (tests/obstacle_map_ref.py) equals the reference's
GridMap and checkers on tests/golden/g21_obstacle_map.npz, and the three C-ABI entries reject bad arguments without
touching a device."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

import obstacle_map_ref as omr
from nfopp import _lib

F32 = np.float32
MAPS = "abcde"
CHECKERS = (("circle", 0.3), ("recta", (-0.34, 0.4, -0.27, 0.27)), ("rectb", (0.1, 0.5, -0.2, 0.2)))


@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_obstacle_map.npz")


@pytest.mark.parametrize("m", MAPS)
def test_point_cloud_and_boundaries_equal_the_reference(g21, m):
    data, res, origin = g21[m + "_data"], float(g21[m + "_resolution"]), g21[m + "_origin"]
    cloud = omr.grid_points(data, res, origin)
    assert cloud.dtype == np.float64 and cloud.shape == g21[m + "_cloud"].shape
    assert np.array_equal(cloud, g21[m + "_cloud"])
    assert omr.grid_boundaries(data.shape, res, origin) == tuple(g21[m + "_bounds"])
    if m == "c":
        assert data.dtype == np.int8 and set(np.unique(data)) == {-1, 0, 50, 51, 100}
        assert len(cloud) == int(((data == 51) | (data == 100)).sum())       # 50 -> 0.5 is not above the threshold
    if m == "a":
        assert (data == F32(0.5)).any() and len(cloud) == int((data > F32(0.5)).sum())


@pytest.mark.parametrize("m", MAPS)
def test_predicates_equal_the_reference_labels(g21, m):
    """float64 restatement on the float64 cloud: every pose, not only the kept ones."""
    poses, cloud, extra, bounds = g21[m + "_poses"], g21[m + "_cloud"], g21[m + "_extra"], tuple(g21[m + "_bounds"])
    updated = np.concatenate([extra, cloud], 0)
    for name, shape in CHECKERS:
        fn = omr.circle_labels if name == "circle" else omr.rectangle_labels
        keep = g21["%s_%s_keep" % (m, name)]
        before, after = fn(poses, cloud, shape, None), fn(poses, updated, shape, bounds)
        # the reference moves the points by the inverse pose instead of subtracting: equal away from the box edges
        assert np.array_equal(before[keep], g21["%s_%s_before" % (m, name)][keep].astype(bool))
        assert np.array_equal(after[keep], g21["%s_%s_after" % (m, name)][keep].astype(bool))
        assert keep.mean() > 0.99
        # fp32 evaluation (what the device does) agrees on the kept poses as well
        assert np.array_equal(fn(poses, updated.astype(F32), shape, bounds, dtype=F32)[keep], after[keep])


def test_cell_index_restatement():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-3, 7, (700, 2)).astype(F32)
    geom = omr.index_geometry(pts, omr.rectangle_reach((0.1, 0.5, -0.2, 0.2)))
    x0, y0, size, nx, ny = geom
    assert size >= F32(np.hypot(0.5, 0.2)) and nx * ny <= 65536
    ordered, start = omr.cell_index(pts, *geom)
    cell = omr.cell_ids(ordered, *geom)
    assert (np.diff(cell) >= 0).all() and start[0] == 0 and start[-1] == len(pts) and len(start) == nx * ny + 1
    for c in (0, nx * ny // 2, nx * ny - 1):
        assert (cell[start[c]:start[c + 1]] == c).all()
    # stable: inside a cell the points keep their input order
    first = {}
    for k, p in enumerate(map(tuple, pts)):
        first.setdefault(p, k)
    where = np.array([first[tuple(p)] for p in ordered])
    for c in np.unique(cell):
        assert (np.diff(where[cell == c]) > 0).all()
    # points outside the region land in the border cells
    far = np.array([[-1e9, 0], [1e9, 1e9], [np.float32(x0), 1e30]], F32)
    assert list(omr.cell_ids(far, *geom)) == [omr.cell_ids(far[:1], *geom)[0], nx * ny - 1, (ny - 1) * nx]
    assert omr.rectangle_reach((-0.34, 0.4, -0.27, 0.27)) == float(np.hypot(0.4, 0.27))


def test_c_abi_argument_checks():
    lib = _lib.load()
    one = ctypes.c_void_p(256)            # a non-null pointer that no rejected call may touch
    box = (ctypes.c_float * 4)(-0.34, 0.4, -0.27, 0.27)
    reach = float(np.hypot(0.4, 0.27))

    def err():
        return lib.nfopp_last_error()

    # nfopp_grid_to_points
    assert lib.nfopp_grid_to_points(None, 0, 4, 4, 0.5, 0.1, 0.0, 0.0, 1.0, 0.0, 0, None, None, one, None) == -1
    assert b"null" in err()
    assert lib.nfopp_grid_to_points(one, 0, 4, 4, 0.5, 0.1, 0.0, 0.0, 1.0, 0.0, 0, None, None, None, None) == -1
    assert lib.nfopp_grid_to_points(one, 0, 4, 4, 0.5, 0.1, 0.0, 0.0, 1.0, 0.0, 8, None, None, one, None) == -1
    assert b"null" in err()
    assert lib.nfopp_grid_to_points(one, 1, 4097, 4096, 0.5, 0.1, 0.0, 0.0, 1.0, 0.0, 0, None, None, one, None) == -1
    assert b"2^24" in err()
    assert lib.nfopp_grid_to_points(one, 0, 0, 4, 0.5, 0.1, 0.0, 0.0, 1.0, 0.0, 0, None, None, one, None) == -1
    # nfopp_build_cell_index
    assert lib.nfopp_cell_index_workspace_bytes(0) == 0
    need = lib.nfopp_cell_index_workspace_bytes(5000)
    assert need >= 5000 * 8 + 256 * 4 * 10
    assert lib.nfopp_build_cell_index(one, 100, 0.0, 0.0, 1.0, 257, 256, one, one, one, need, None) == -1
    assert b"65536" in err()
    assert lib.nfopp_build_cell_index(one, 100, 0.0, 0.0, 1.0, 0, 4, one, one, one, need, None) == -1
    assert lib.nfopp_build_cell_index(one, 100, 0.0, 0.0, 0.0, 4, 4, one, one, one, need, None) == -1
    assert lib.nfopp_build_cell_index(one, -1, 0.0, 0.0, 1.0, 4, 4, one, one, one, need, None) == -1
    assert lib.nfopp_build_cell_index(None, 100, 0.0, 0.0, 1.0, 4, 4, one, one, one, need, None) == -1
    assert b"null" in err()
    assert lib.nfopp_build_cell_index(one, 100, 0.0, 0.0, 1.0, 4, 4, one, None, one, need, None) == -1
    assert lib.nfopp_build_cell_index(one, 100, 0.0, 0.0, 1.0, 4, 4, one, one, None, need, None) == -1
    assert lib.nfopp_build_cell_index(one, 5000, 0.0, 0.0, 1.0, 4, 4, one, one, one, need - 1, None) == -1
    assert b"workspace" in err()
    assert lib.nfopp_build_cell_index(None, 0, 0.0, 0.0, 1.0, 4, 4, None, None, None, 0, None) == -1   # cell_start is written
    # nfopp_check_collision_rectangle_cells
    def rect(n=10, poses=one, pts=one, n_pts=50, start=one, nx=4, ny=4, size=0.6, bx=box, r=reach, labels=one):
        return lib.nfopp_check_collision_rectangle_cells(poses, n, pts, n_pts, start, nx, ny, 0.0, 0.0, size, bx, r, None,
                                                         labels, None)
    assert rect(n=0, poses=None, labels=None) == 0                   # no pose: nothing to do, nothing is launched
    assert rect(poses=None) == -1 and b"null" in err()
    assert rect(labels=None) == -1
    assert rect(bx=None) == -1 and b"box" in err()
    assert rect(pts=None) == -1 and rect(start=None) == -1 and rect(n_pts=0) == -1
    assert rect(size=float(np.nextafter(F32(reach), F32(0)))) == -1 and b"reach" in err()     # cell_size < reach
    assert rect(r=0.3) == -1 and b"reach" in err()                    # a reach that does not cover the box's corners
    assert rect(nx=0) == -1 and rect(n=-1) == -1
