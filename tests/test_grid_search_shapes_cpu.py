"""CPU: the references and the cases of test_gpu_grid_search_shapes.py, checked without a GPU: the trace rule against the
reference's paths, the fast field against the plain Dijkstra, the shape table against the library's own LDS / workspace
switches, and the conditioning of the seeding cases (SPREAD, heading cut)."""
import numpy as np
import pytest

import nfopp

import grid_search_ref as gsr

FX = gsr.load_fixture()
SMALL = [s for s in gsr.SHAPES if s[0] * s[1] <= 4096]


@pytest.mark.parametrize("k", [3, 4])
def test_trace_rule_reproduces_the_reference_paths(k):
    m = gsr.fixture_map(FX, k)
    for i, ref_path in enumerate(m["paths"]):
        f = gsr.dijkstra_field(m["occ"], m["goal_cells"][i])
        cells, cost = gsr.trace_path(f, m["start_cells"][i])
        assert np.array_equal(cells, ref_path) and tuple(cost) == tuple(m["cost"][i]), i
        got = gsr.trace_paths(f, m["start_cells"][i:i + 1])
        assert np.array_equal(got[0][0, :got[1][0]], ref_path) and got[2][0] == 0 and tuple(got[3][0]) == tuple(cost)


@pytest.mark.parametrize("shape", [(13, 15), (64, 64)])
def test_traced_paths_are_valid_and_optimal_from_every_cell(shape):
    occ = gsr.make_map("random", *shape)
    goals = gsr.shape_goals(occ)
    starts = np.argwhere(np.ones(shape, bool))
    for goal in goals[[0, 3]]:                       # a free goal and a wall goal (forced free)
        free = occ.copy()
        free[tuple(goal)] = 0
        f = gsr.dijkstra_field(occ, goal)
        many = gsr.trace_paths(f, np.concatenate([starts, [(-1, 0), (shape[0], 0), (0, shape[1])]]))
        assert list(many[2][-3:]) == [2, 2, 2] and (many[1][-3:] == 0).all() and (many[3][-3:] == -1).all()
        n_wall = n_stuck = 0
        for i, s in enumerate(starts):
            cells, cost = gsr.trace_path(f, s)
            assert many[1][i] == len(cells) and np.array_equal(many[0][i, :len(cells)], cells)
            assert tuple(many[3][i]) == tuple(cost) and many[2][i] == (0 if len(cells) else 1)
            if f[tuple(s)][0] >= 0:
                want = tuple(f[tuple(s)])
            else:                                    # a wall (or cut-off) start: the cheapest way over a free neighbour
                n_wall += 1
                cand = [gsr.Cost((int(f[n][0]) + (j < 4), int(f[n][1]) + (j >= 4)))
                        for j, n in enumerate((s[0] + dr, s[1] + dc) for dr, dc in gsr.MOVES)
                        if 0 <= n[0] < shape[0] and 0 <= n[1] < shape[1] and f[n][0] >= 0]
                want = tuple(min(cand)) if cand else (-1, -1)
            assert tuple(cost) == want, (s, cost, want)
            if len(cells):
                assert gsr.check_path(free, cells, s, goal) == want
            else:
                n_stuck += 1
        assert n_wall > shape[0] * shape[1] // 5     # the wall-start branch is really walked
        print(shape, goal, "wall or cut-off starts %d, without a way %d" % (n_wall, n_stuck))


@pytest.mark.parametrize("shape", SMALL)
def test_fast_field_equals_the_plain_dijkstra(shape):
    for kind in gsr.MAP_KINDS:
        occ = gsr.make_map(kind, *shape)
        for goal in gsr.shape_goals(occ):
            want = gsr.dijkstra_field(occ, goal)
            assert np.array_equal(gsr.fast_field(occ, goal), want), (shape, kind, goal)
            assert gsr.is_exact_field(occ, goal, want)
            if (want[..., 0] > 0).any():             # the proof refuses a field that is off by one move in one cell
                bad = want.copy()
                r, c = np.argwhere(want[..., 0] > 0)[-1]
                bad[r, c] += (1, 0)
                assert not gsr.is_exact_field(occ, goal, bad)
                bad = want.copy()
                bad[r, c] -= (1, 0)
                assert not gsr.is_exact_field(occ, goal, bad)


def test_map_makers():
    assert len(set(gsr.SHAPES)) == len(gsr.SHAPES) == 20
    for shape in ((13, 15), (3, 8), (1, 7), (7, 1)):
        assert not gsr.make_map("empty", *shape).any() and gsr.make_map("full", *shape).all()
        r = gsr.make_map("random", *shape)
        assert np.array_equal(r, gsr.make_map("random", *shape)) and r.shape == shape
    assert 0.25 < gsr.make_map("random", 64, 64).mean() < 0.35
    s = gsr.make_map("serpentine", 13, 15)
    assert not s[0::2].any() and (s[1::2].sum(1) == 14).all()
    assert [int(np.flatnonzero(row == 0)[0]) for row in s[1::2]] == [14, 0, 14, 0, 14, 0]
    assert not gsr.make_map("serpentine", 1, 12285).any() and not gsr.make_map("serpentine", 4094, 1).any()
    # the only way through is along every corridor
    f = gsr.fast_field(s, (12, 14))
    assert tuple(f[0, 14]) != (-1, -1) and f[0, 0, 0] + f[0, 0, 1] >= 6 * 13


def test_shape_table_straddles_the_library_switches():
    lib = nfopp.load_library()
    for i, (rows, cols) in enumerate(gsr.SHAPES):
        ws = lib.nfopp_grid_fields_workspace_bytes(rows, cols, 1)
        cols_p = (cols + 6) // 7 * 7
        if i < gsr.SHAPES_LDS:
            assert ws == 0, "(%d, %d) left the LDS kernel: replace it in grid_search_ref.SHAPES" % (rows, cols)
        else:
            assert ws == (rows + 2) * (cols_p + 2) * 8, "(%d, %d) left the global-memory kernel" % (rows, cols)
    assert (4094 + 2) * (7 + 2) == 36864 and gsr.SHAPES[gsr.SHAPES_LDS - 1] == (4094, 1)
    for cols in (1, 2, 7, 8, 6, 15, 64, 183):            # cols % 7 in {0, 1, 6} and grids narrower than one run
        assert any(s[1] == cols for s in gsr.SHAPES)
    assert {s[1] % 7 for s in gsr.SHAPES} >= {0, 1, 6}
    assert lib.nfopp_grid_seed_workspace_bytes(1, 1167) == 0
    assert lib.nfopp_grid_seed_workspace_bytes(1, 1168) == (7 * 1170 + 3) * 8
    assert lib.nfopp_grid_seed_workspace_bytes(3, 3000) == 3 * (7 * 3002 + 3) * 8


def test_seed_cases_are_well_conditioned():
    """SPREAD: the float64 reference against the same spline in long double, every waypoint of every case and N."""
    cases = gsr.seed_cases()
    assert [len(c["cells"]) for c in cases] == [1, 2, 3, 40, 1167, 1168, 3000]
    spread = 0.0
    b, res = gsr.SEED_BOUNDARIES, gsr.SEED_RESOLUTION
    for case in cases:
        poly = gsr.polyline(case["cells"], case["start"], case["goal"], b, res)
        assert np.array_equal(gsr.cells_of(poly[[0, -1]], b, res), case["cells"][[0, -1]])      # endpoints in their cells ...
        centres = poly[[1, -2]].astype(np.float64)
        assert (np.abs(poly[[0, -1]] - centres).max(1) >= 0.05 * res).all()                    # ... off the centres
        assert (np.linalg.norm(np.diff(poly.astype(np.float64), axis=0), axis=1) > 0.04 * res).all()   # no empty segment
        gsr.path_cost(case["cells"])                                                           # 8-connected
        worst = 0.0
        for n in gsr.SEED_NS:
            ref = gsr.reparametrize(poly, n + 2)
            exact = gsr.spline_longdouble(poly, n + 2)
            err = float(np.abs(ref.astype(np.longdouble) - exact).max())
            assert float(np.abs(exact[[0, -1]] - poly[[0, -1]]).max()) < 1e-15 * 400           # it interpolates
            worst = max(worst, err)
        spread = max(spread, worst)
        print("%-9s %4d cells: |float64 - long double| over all N: %.3e m" % (case["name"], len(case["cells"]), worst))
    print("SPREAD = %.3e m (recorded %.3e, cap %.1e)" % (spread, gsr.SPREAD, gsr.SPREAD_CAP))
    assert spread <= gsr.SPREAD <= gsr.SPREAD_CAP


def directed_margin(xy, start, goal):
    """min distance of heading - th from +-pi over the waypoints, float64 on fp32 xy (trajectory_initializer.py:23-41)."""
    n = len(xy)
    full = np.concatenate([start[None, :2], xy.astype(np.float32), goal[None, :2]]).astype(np.float64)
    heading = np.arctan2(full[2:, 1] - full[:-2, 1], full[2:, 0] - full[:-2, 0])
    s, g = float(start[2]), float(goal[2])
    goal_angle = (g - s + np.pi) % (2 * np.pi) - np.pi + s
    th = np.linspace(s, goal_angle, n + 2)[1:-1]
    d = heading - th
    assert np.abs(d).max() < 2 * np.pi
    return float(np.abs(np.abs(d) - np.pi).min())


def test_directed_cases_stay_off_the_heading_cut():
    cases = [c for c in gsr.seed_cases() if c["directed"]]
    assert [c["name"] for c in cases] == ["c40", "serp3000"]
    for case in cases:
        for n in gsr.SEED_DIRECTED_NS:
            margin = directed_margin(gsr.seed_reference(case, n), case["start"], case["goal"])
            print("%s N = %d: heading - th stays %.3f rad from +-pi" % (case["name"], n, margin))
            assert margin > 1e-3
