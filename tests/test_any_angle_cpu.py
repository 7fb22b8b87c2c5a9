"""CPU: the restatement of the any-angle shortening (tests/any_angle_ref.py) against its definition and hand-checked
cases, the facts about the g19 fixture that keep tests/test_gpu_any_angle.py from being vacuous, the spline spread of the
any-angle seeding cases, and the C entries' argument checks.  No GPU is touched.

The fixture conditions below were measured when the cases were chosen (paths traced with gsr.dijkstra_field +
gsr.trace_path).  If the fixture is regenerated and one moves, replace the case it names; do not loosen the condition."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import nfopp
from nfopp import _lib

import any_angle_ref as aar
import edt_ref as er
import grid_search_ref as gsr

FX = gsr.load_fixture()


@functools.lru_cache(maxsize=None)
def _map(k):
    m = gsr.fixture_map(FX, k)
    return m, er.edt(m["occ"])[0], aar.traced_paths(m)


# ---- the traversal ---------------------------------------------------------------------------------------------------------
def test_traversal_equals_exact_clipping():
    pairs = 0
    for r0 in range(3):
        for c0 in range(3):
            for dr in range(-8, 9):
                for dc in range(-8, 9):
                    a, b = (r0, c0), (r0 + dr, c0 + dc)
                    got = aar.traverse(a, b)
                    assert len(set(got)) == len(got), (a, b)                          # no cell twice
                    assert got[0] == a and got[-1] == b
                    assert set(got) == aar.clipped_cells(a, b), (a, b)
                    assert got[::-1] == aar.traverse(b, a), (a, b)                    # seeing is mutual
                    pairs += 1
    assert pairs == 9 * 17 * 17


def test_named_geometry():
    assert aar.traverse((0, 0), (1, 1)) == [(0, 0), (1, 1)]
    walls = np.full((2, 2), 9, np.int64)
    walls[0, 1] = walls[1, 0] = 0
    assert aar.sees(walls, 0, (0, 0), (1, 1))                 # a diagonal move between two walls is legal
    assert aar.traverse((0, 0), (2, 2)) == [(0, 0), (1, 1), (2, 2)]
    assert aar.traverse((0, 0), (1, 3)) == [(0, 0), (0, 1), (1, 2), (1, 3)]       # through the corner (row 1, col 2)
    assert aar.traverse((0, 0), (0, 0)) == [(0, 0)]
    assert aar.traverse((2, 5), (2, 2)) == [(2, 5), (2, 4), (2, 3), (2, 2)]
    assert aar.traverse((0, 0), (1, 2)) == [(0, 0), (0, 1), (1, 1), (1, 2)]
    # the end cells are never tested; a blocked cell between them is
    d = np.full((1, 4), 9, np.int64)
    d[0, 0] = d[0, 3] = 0
    assert aar.sees(d, 0, (0, 0), (0, 3))
    d[0, 2] = 1
    assert aar.sees(d, 0, (0, 0), (0, 3)) and not aar.sees(d, 1, (0, 0), (0, 3))  # blocked iff dist2 <= threshold


def test_anchor_rule_is_farthest_visible():
    occ = np.zeros((3, 5), np.uint8)
    occ[1, 1] = 1
    dist2 = er.edt(occ)[0]
    path = [(2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (0, 1), (0, 0)]      # round the wall; (0, 0) is seen up column 0
    assert [aar.sees(dist2, 0, path[0], q) for q in path[1:]] == [True, True, False, False, False, True]
    assert aar.anchors(dist2, 0, path, 256) == [0, 6]                    # "the first blocked cell ends the scan" gives 2
    assert aar.anchors(dist2, 0, path, 5) == [0, 2, 4, 6]                # (2, 2) sees (0, 2) up column 2, not (0, 1)
    assert aar.anchors(dist2, 0, path, 1) == list(range(len(path)))
    # threshold 1 blocks the four cells beside the wall too; only touching cells are left to see: the diagonal moves
    assert aar.anchors(dist2, 1, path, 256) == [0, 1, 3, 5, 6]
    # not 8-connected and blocked in between: the fallback a + 1
    d = np.asarray([[9, 0, 9]])
    assert aar.anchors(d, 0, [(0, 0), (0, 2)], 256) == [0, 1]
    assert aar.anchors(d, 0, [(0, 0)], 256) == [0]


@pytest.mark.parametrize("lookahead,want", [(1, 200), (63, 5), (64, 5), (65, 5), (199, 2), (200, 2), (256, 2)])
def test_lookahead_on_an_empty_corridor(lookahead, want):
    dist2 = np.full((1, 200), er.NONE, np.int64)
    path = [(0, c) for c in range(200)]
    a, pts = aar.shorten(dist2, 0, path, lookahead, (0.0, 200.0, 0.0, 1.0), 1.0)
    assert len(a) == want and a[0] == 0 and a[-1] == 199
    assert np.array_equal(pts, gsr.polyline(path, (0, 0), (0, 0), (0.0, 200.0, 0.0, 1.0), 1.0)[1:-1])


def test_dense_points_hand_checked():
    b, res = (-3.0, 400.0, 2.0, 400.0), 0.25
    path = [(5, 7), (6, 8), (7, 10), (7, 10), (4, 10)]
    pts = aar.dense_points(path, [0, 2, 3, 4], b, res)      # segments (2, 3), (0, 0) -- nothing --, (-3, 0)
    u = [(7.0, 5.0), (8.0, 5 + 2 / 3), (9.0, 5 + 4 / 3), (10.0, 7.0), (10.0, 6.0), (10.0, 5.0), (10.0, 4.0)]
    want = np.asarray([((c * res + res / 2) + b[0], (r * res + res / 2) + b[2]) for c, r in u]).astype(np.float32)
    assert pts.dtype == np.float32 and np.array_equal(pts, want)
    whole = aar.dense_points(path[:2], [0, 1], b, res)      # integer u: the seeding stage's cell centres, bit for bit
    assert np.array_equal(whole, gsr.polyline(path[:2], (0, 0), (0, 0), b, res)[1:-1])


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def _length(xy):
    return float(np.linalg.norm(np.diff(xy.astype(np.float64), axis=0), axis=1).sum())


def test_map_1_is_shortened():
    m, dist2, paths = _map(1)
    assert len(paths) == 32
    for i, p in enumerate(paths):
        a, pts = aar.shorten(dist2, 0, p, 256, m["boundaries"], m["resolution"])
        assert len(a) < len(p), i                                                   # every path is shortened
        assert len(pts) <= len(p), i
        sa, sb = gsr.path_cost(p)
        assert _length(pts) <= (sa + sb * np.sqrt(2.0)) * m["resolution"] * (1 + 1e-6), i
        for k0, k1 in zip(a[:-1], a[1:]):
            assert aar.sees(dist2, 0, p[k0], p[k1])
    ratio = [_length(aar.shorten(dist2, 0, p, 256, m["boundaries"], m["resolution"])[1]) /
             _length(gsr.polyline(p, (0, 0), (0, 0), m["boundaries"], m["resolution"])[1:-1]) for p in paths]
    print("map 1 length ratio: mean %.3f, min %.3f" % (np.mean(ratio), np.min(ratio)))
    assert np.mean(ratio) < 0.97


def test_visibility_along_a_path_is_not_monotone():
    """From the start cell a later cell is seen after one that is not, on at least 4 of map 1's first 16 problems: there
    "farthest visible" and "the first blocked cell ends the scan" give different anchors."""
    m, dist2, paths = _map(1)
    found = 0
    for p in paths[:16]:
        vis = [aar.sees(dist2, 0, p[0], q) for q in p[1:]]
        first_blocked = vis.index(False) if False in vis else len(vis)
        if any(vis[first_blocked:]):
            found += 1
            assert aar.anchors(dist2, 0, p, 256)[1] > first_blocked                 # the two rules differ here
    assert found >= 4, found


@pytest.mark.parametrize("k", [3, 4])
def test_one_cell_corridors_have_nothing_to_shorten(k):
    m, dist2, paths = _map(k)
    assert len(paths) == 8
    for i, p in enumerate(paths):
        _, pts = aar.shorten(dist2, 0, p, 256, m["boundaries"], m["resolution"])
        cell_path = gsr.polyline(p, (0, 0), (0, 0), m["boundaries"], m["resolution"])[1:-1]
        assert pts.tobytes() == cell_path.tobytes(), (k, i)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_no_more_points_than_cells(k):
    m, dist2, paths = _map(k)
    for p in paths:
        if len(p):
            assert len(aar.shorten(dist2, 0, p, 256, m["boundaries"], m["resolution"])[1]) <= len(p)


def test_chords_keep_the_clearance_of_their_level():
    m, dist2, _ = _map(2)
    levels = [4, 1]
    paths, thr = aar.level_paths(m, levels)
    assert sorted(set(thr)) == [1, 4] and all(thr.count(v) >= 4 for v in (1, 4))      # every problem is seeded at a level
    shortened = {1: 0, 4: 0}
    for p, k in zip(paths, thr):
        a = aar.anchors(dist2, k, p, 256)
        shortened[k] += len(a) < len(p)
        for k0, k1 in zip(a[:-1], a[1:]):
            for r, c in aar.traverse(p[k0], p[k1])[1:-1]:
                assert dist2[r, c] > k
    assert all(v >= 1 for v in shortened.values()), shortened


def test_spread_of_the_any_angle_seeding_cases():
    """AA_SPREAD: |gsr.reparametrize - gsr.spline_longdouble| over the any-angle seeds of maps 1 and 2 (what
    test_gpu_any_angle.py gates the device's xy with), against the long-double reference, never against the kernel."""
    worst = 0.0
    for k in (1, 2):
        m, dist2, paths = _map(k)
        for i, p in enumerate(paths):
            _, pts = aar.shorten(dist2, 0, p, 256, m["boundaries"], m["resolution"])
            poly = aar.polyline(pts, m["starts"][i], m["goals"][i])
            d = np.abs(gsr.reparametrize(poly, aar.SEED_N + 2) - gsr.spline_longdouble(poly, aar.SEED_N + 2).astype(np.float64))
            worst = max(worst, float(d.max()))
    print("any-angle seeding cases: spread %.3e m" % worst)
    assert worst <= aar.AA_SPREAD <= gsr.SPREAD_CAP


# ---- the C entries ----------------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks():
    lib = _lib.load()
    one = ctypes.c_void_p(256)            # a non-null pointer that no rejected call may touch

    def shorten(dist2=one, rows=10, cols=10, cells=one, count=one, status=one, cells2=None, batch=1, max_len=8, lookahead=4,
                anchor=one, anchor_count=one, res=1.0, max_points=8, points=one, point_count=one):
        return lib.nfopp_grid_shorten_paths(dist2, rows, cols, cells, count, status, cells2, batch, max_len, lookahead, anchor,
                                            anchor_count, 0.0, 0.0, res, max_points, points, point_count, None)

    def err():
        return lib.nfopp_last_error()

    assert shorten(lookahead=0) == -1 and b"lookahead" in err()
    assert shorten(lookahead=-3) == -1 and b"lookahead" in err()
    assert shorten(rows=0) == -1 and shorten(cols=-1) == -1 and b"at least one" in err()
    assert shorten(rows=4097, cols=1) == -1 and b"4096" in err()
    assert shorten(rows=1, cols=4097) == -1 and b"4096" in err()
    assert shorten(rows=65536, cols=65536) == -1 and b"4096" in err()
    assert shorten(res=0.0) == -1 and b"resolution" in err()
    assert shorten(batch=-1) == -1 and shorten(max_len=-1) == -1 and shorten(max_points=-1) == -1
    assert shorten(max_len=(1 << 21) + 2) == -1
    for name in ("dist2", "cells", "count", "status", "anchor", "anchor_count", "point_count"):
        assert shorten(**{name: None}) == -1 and b"null" in err(), name
    assert shorten(batch=0, dist2=None) == 0                                       # nothing to do

    def seed(points=one, count=one, status=one, batch=1, max_len=8, start=one, goal=one, n=4, dim=2, directed=0, traj=one):
        return lib.nfopp_grid_seed_polylines(points, count, status, batch, max_len, start, goal, n, dim, directed, traj, None, 0, None)

    assert seed(dim=4) == -1 and b"dim" in err()
    assert seed(dim=2, directed=1) == -1 and b"SE(2)" in err()
    assert seed(n=0) == -1 and seed(batch=-1) == -1
    for name in ("points", "count", "status", "start", "goal", "traj"):
        assert seed(**{name: None}) == -1 and b"null" in err(), name
    assert seed(max_len=1168) == -1 and b"workspace" in err()                      # beyond LDS: needs the workspace
    assert seed(batch=0, points=None) == 0


def test_header_binding_and_library_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nfopp_hip.h")).read()
    declared = set(re.findall(r"\b(nfopp_[a-z0-9_]+)\s*\(", header))
    lib = nfopp.load_library()
    for name in ("nfopp_grid_shorten_paths", "nfopp_grid_seed_polylines"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert len(_lib._SIGNATURES["nfopp_grid_shorten_paths"][1]) == 19 and len(_lib._SIGNATURES["nfopp_grid_seed_polylines"][1]) == 14
    assert lib.nfopp_abi_version() == 6
    assert "farthest visible" in header.lower() and "lattice corner" in header


def test_python_arguments_are_checked_on_the_host():
    import inspect
    from nfopp import grid_search as gs
    sig = inspect.signature(nfopp.AstarTrajectoryInitializer.__init__)
    assert list(sig.parameters)[-3:] == ["clearance", "any_angle", "lookahead"]        # after the existing ones
    assert sig.parameters["any_angle"].default is False and sig.parameters["lookahead"].default == 256
    sig = inspect.signature(nfopp.grid_search_init)
    assert list(sig.parameters)[-3:] == ["clearance", "any_angle", "lookahead"] and sig.parameters["any_angle"].default is False
    assert inspect.signature(nfopp.BatchPlanner.init).parameters["seed_any_angle"].default is False
    assert inspect.signature(gs.shorten_paths).parameters["lookahead"].default == 256
    assert nfopp.shorten_paths is gs.shorten_paths and nfopp.seed_polylines is gs.seed_polylines
    grid = nfopp.OccupancyGrid(np.zeros((3, 3), np.uint8), (0, 3, 0, 3), 1.0)
    with pytest.raises(ValueError):
        nfopp.shorten_paths(grid, None, None, None, lookahead=0)
    with pytest.raises(ValueError):
        nfopp.grid_search_init(grid, None, None, 8, any_angle=True, lookahead=0)
    assert grid._occupancy_dev is None
