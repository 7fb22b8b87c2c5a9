"""CPU: the grid distance transform's restatement (tests/edt_ref.py) against itself and against hand-checked cases, the
host side of the clearance margin, the C entry's argument checks and the facts about the g19 fixture that keep the GPU
tests of tests/test_gpu_grid_edt.py from being vacuous.  No GPU is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import nfopp
from nfopp import _lib

import edt_ref as er
import grid_search_ref as gsr

FX = gsr.load_fixture()
M2_CELLS2 = 4   # the threshold at which m2 has problems of both kinds (test_gpu_grid_edt.py uses the same)


def _checkerboard(rows, cols):
    return ((np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2).astype(np.uint8)


def _cases():
    rng = np.random.default_rng(19)
    out = []
    for shape in ((1, 1), (1, 9), (13, 1), (7, 12), (40, 40), (23, 40)):
        for density in (0.0, 0.05, 0.5, 1.0):
            out.append(("random %s %.2f" % (shape, density), (rng.random(shape) < density).astype(np.uint8)))
        one = np.zeros(shape, np.uint8)
        one[rng.integers(shape[0]), rng.integers(shape[1])] = 1
        out.append(("one cell %s" % (shape,), one))
    out.append(("checkerboard", _checkerboard(9, 14)))
    # two cells placed symmetrically about a third cell: that cell, and the whole line between them, is a tie
    for a, b in (((4, 2), (4, 8)), ((1, 5), (9, 5)), ((2, 2), (8, 8)), ((2, 8), (8, 2))):
        tie = np.zeros((11, 11), np.uint8)
        tie[a] = tie[b] = 1
        out.append(("tie %s %s" % (a, b), tie))
    return out


@pytest.mark.parametrize("border", [False, True])
def test_all_pairs_and_separable_statements_agree(border):
    for name, occ in _cases():
        d_a, n_a = er.edt_all_pairs(occ, border)
        d_s, n_s = er.edt_separable(occ, border)
        assert d_a.dtype == np.int32 and n_a.dtype == np.int32
        assert np.array_equal(d_a, d_s), name
        assert np.array_equal(n_a, n_s), name
        d_e, n_e = er.edt(occ, border)
        assert np.array_equal(d_a, d_e) and np.array_equal(n_a, n_e), name


def test_a_tie_goes_to_the_smaller_flat_index():
    tie = np.zeros((11, 11), np.uint8)
    tie[4, 2] = tie[4, 8] = 1
    d, n = er.edt_all_pairs(tie)
    assert d[4, 5] == 9 and n[4, 5] == 4 * 11 + 2          # left and right equally far: the smaller column
    assert d[0, 5] == 16 + 9 and n[0, 5] == 4 * 11 + 2
    tie = np.zeros((11, 11), np.uint8)
    tie[1, 5] = tie[9, 5] = 1
    d, n = er.edt_separable(tie)
    assert d[5, 5] == 16 and n[5, 5] == 1 * 11 + 5         # above and below equally far: the smaller row
    assert d[5, 0] == 16 + 25 and n[5, 0] == 1 * 11 + 5
    tie = np.zeros((11, 11), np.uint8)
    tie[2, 8] = tie[8, 2] = 1
    d, n = er.edt_separable(tie)
    assert d[5, 5] == 18 and n[5, 5] == 2 * 11 + 8         # the smaller row wins although its column is the larger


def test_hand_checked_cases():
    corner = np.zeros((3, 4), np.uint8)
    corner[0, 0] = 1
    for fn in (er.edt_all_pairs, er.edt_separable):
        d, n = fn(corner)
        assert np.array_equal(d, [[0, 1, 4, 9], [1, 2, 5, 10], [4, 5, 8, 13]])
        assert (n == 0).all()
        d, n = fn(corner, border=True)
        assert np.array_equal(d, [[0, 1, 1, 1], [1, 2, 4, 1], [1, 1, 1, 1]])   # b = [[1 1 1 1] [1 2 2 1] [1 1 1 1]]
        assert (n == 0).all()
        d, n = fn(np.zeros((5, 2), np.uint8))
        assert (d == er.NONE).all() and (n == -1).all() and er.NONE == np.iinfo(np.int32).max
        d, n = fn(np.zeros((1, 1), np.uint8), border=True)
        assert d[0, 0] == 1 and n[0, 0] == -1                                  # b = 1: the cell just outside
        d, n = fn(np.ones((1, 1), np.uint8), border=True)
        assert d[0, 0] == 0 and n[0, 0] == 0
        d, n = fn(np.zeros((5, 7), np.uint8), border=True)
        assert np.array_equal(d[2], [1, 4, 9, 9, 9, 4, 1]) and (n == -1).all()


def test_threshold_of_a_margin():
    assert nfopp.margin_cells2(0.7, 0.1) == 49          # 0.7 / 0.1 = 6.999999999999999 in float64
    assert nfopp.margin_cells2(1.0, 1.0) == 1
    for s in (0.05, 0.1, 1.0, 3.0):
        assert nfopp.margin_cells2(0.0, s) == 0
    assert nfopp.margin_cells2(0.99, 1.0) == 0
    assert nfopp.margin_cells2(2.0, 1.0) == 4 and nfopp.margin_cells2(np.sqrt(2.0) * 0.5, 0.5) == 2
    assert nfopp.margin_cells2(0.3, 0.1) == 9 and nfopp.margin_cells2(0.29, 0.1) == 8
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            nfopp.margin_cells2(bad, 1.0)


def test_clearance_arguments_are_checked_on_the_host():
    from nfopp import grid_search as gs
    assert gs._margins(0.5) == [0.5] and gs._margins([1.0, 0.5]) == [1.0, 0.5] and gs._margins(()) == []
    for bad in ([0.5, 1.0], [0.5, 0.5], [-1.0], float("nan")):
        with pytest.raises(ValueError):
            gs._margins(bad)
    grid = nfopp.OccupancyGrid(np.zeros((3, 3), np.uint8), (0, 3, 0, 3), 1.0)
    with pytest.raises(TypeError):
        grid.inflated()
    with pytest.raises(TypeError):
        grid.inflated(1.0, cells2=1)
    with pytest.raises(ValueError):
        grid.inflated(cells2=-1)
    with pytest.raises(ValueError):
        grid.inflated(cells2=1.5)
    assert grid._occupancy_dev is None


def test_c_abi_argument_checks():
    lib = _lib.load()
    one = ctypes.c_void_p(256)            # a non-null pointer that no rejected call may touch

    def edt(occ=one, rows=10, cols=10, border=0, dist2=one, nearest=one, ws=one, ws_bytes=1 << 30):
        return lib.nfopp_grid_edt(occ, rows, cols, border, dist2, nearest, ws, ws_bytes, None)

    def err():
        return lib.nfopp_last_error()

    assert edt(occ=None) == -1 and b"null" in err()
    assert edt(dist2=None) == -1 and b"null" in err()
    assert edt(rows=0) == -1 and edt(cols=0) == -1 and edt(rows=-5) == -1 and b"at least one" in err()
    assert edt(rows=4097, cols=1) == -1 and b"4096" in err()
    assert edt(rows=1, cols=4097) == -1 and b"4096" in err()
    assert edt(rows=1 << 20, cols=1 << 20) == -1            # 2^40 cells: rejected, not wrapped to 0
    assert edt(rows=65536, cols=65536) == -1                # 2^32 cells: would wrap to 0 in 32 bits
    assert edt(ws=None) == -1 and b"workspace" in err()
    assert edt(ws_bytes=10 * 10 * 4 - 1) == -1 and b"workspace" in err()
    size = lib.nfopp_grid_edt_workspace_bytes
    assert size(10, 10) == 400 and size(4096, 4096) == 4 << 24 and size(1, 4096) == 4 * 4096
    for rows, cols in ((0, 5), (5, 0), (-1, 5), (4097, 1), (1, 4097), (65536, 65536), (1 << 20, 1 << 20)):
        assert size(rows, cols) == 0, (rows, cols)
    # "more than 2^24 cells" cannot be reached with both sides within 4096; the source keeps the test all the same
    src = open(os.path.join(os.path.dirname(_lib.__file__), "..", "csrc", "grid_edt.hip")).read()
    assert "EDT_MAX_CELLS = 1LL << 24" in src and "rows * cols <= EDT_MAX_CELLS" in src


def test_header_binding_and_library_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nfopp_hip.h")).read()
    declared = set(re.findall(r"\b(nfopp_[a-z0-9_]+)\s*\(", header))
    lib = nfopp.load_library()
    for name in ("nfopp_grid_edt", "nfopp_grid_edt_workspace_bytes"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert len(_lib._SIGNATURES["nfopp_grid_edt"][1]) == 9 and _lib._SIGNATURES["nfopp_grid_edt_workspace_bytes"][0] is ctypes.c_size_t
    assert lib.nfopp_abi_version() == 6
    assert "smallest flat index" in header.lower() and "INT32_MAX" in header      # the tie rule and the sentinels are stated


def test_fixture_has_problems_of_both_kinds():
    """The seeding rule on the g19 maps, restated with the exact Dijkstra: what the GPU tests rely on.

    m4 problem 6 starts in the cell next to its goal's.  The start cell is not tested and the goal cell is forced free, so
    its one-move path exists on any image, the all-wall one included: it is seeded at the margin, along the same two cells
    as on the plain grid.  Every other problem of m3 and m4 falls back."""
    m1 = gsr.fixture_map(FX, 1)
    at_margin = er.seed_levels(m1["occ"], m1["start_cells"], m1["goal_cells"], [1]) == 0
    assert len(at_margin) == 32 and at_margin.sum() >= 24
    for k in (3, 4):
        m = gsr.fixture_map(FX, k)
        assert er.edt(m["occ"])[0].max() == 1 and er.inflate(m["occ"], 1).all()   # one-cell corridors: all wall
        at_margin = er.seed_levels(m["occ"], m["start_cells"], m["goal_cells"], [1]) == 0
        touching = np.abs(m["start_cells"].astype(np.int64) - m["goal_cells"]).max(1) <= 1
        assert np.array_equal(at_margin, touching)
        assert np.flatnonzero(touching).tolist() == ([] if k == 3 else [6])
    m2 = gsr.fixture_map(FX, 2)
    at_margin = er.seed_levels(m2["occ"], m2["start_cells"], m2["goal_cells"], [M2_CELLS2]) == 0
    assert at_margin.sum() >= 4 and (~at_margin).sum() >= 4
    pair = er.seed_levels(m2["occ"], m2["start_cells"], m2["goal_cells"], [4, 1])
    assert (pair == 0).sum() >= 4 and (pair == 1).sum() >= 4                      # (2 cells, 1 cell): both levels are used
