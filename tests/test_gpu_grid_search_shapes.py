"""GPU: the grid-search seeder (csrc/grid_search.hip) at the shapes where its code branches, against the exact references
of tests/grid_search_ref.py (test_grid_search_shapes_cpu.py checks those and the cases without a GPU).

Gates.  Fields, cells, counts, costs and status are integers: `==`.  Seeded xy against the float64 reference spline: one
fp32 ulp of the coordinate (the final cast) + 8 x SPREAD, the measured distance of that reference from the same spline in
long double (the device's tridiagonal elimination is a third evaluation order beside scipy's and the long-double one).
Undirected headings and every straight-line fallback row: bit-identical to nfopp.init_trajectories.  Directed headings:
1e-6 (atan2f rounding, the gate of test_gpu_path_tools.py) against initialize_angle_with_trajectory_direction restated
in float64 on the xy the kernel itself wrote.

Long paths of the 16 + 16-bit packing: the serpentine at (189, 183) and the corridor (1, 12285) reach straight counts above
10 000; (4094, 1), the grid that fills the LDS budget to the word, has 4094 cells, so 4093 is the most it can hold.
Counts above 32767 cannot be reached within the 36864-word LDS budget (a path has fewer cells than the grid), so the
sign bit of the packed half is not looked for."""
import functools

import numpy as np
import pytest
import torch

import nfopp
from nfopp import _lib

import grid_search_ref as gsr

pytestmark = pytest.mark.gpu
F32 = np.float32
I32 = torch.int32
SENT = -7            # sentinel of integer output buffers
GUARD = 300          # sentinel entries after every integer output buffer


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _grid(occ, origin=0.0):
    rows, cols = occ.shape
    return nfopp.OccupancyGrid(occ, (origin, origin + cols, origin, origin + rows), 1.0, device="cuda")


# ---- a. fields --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fields(shape, kind):
    """-> (occ, goals [6, 2], fields int32 [6, rows, cols, 2] from the device); two calls, bit-identical."""
    occ = gsr.make_map(kind, *shape)
    goals = gsr.shape_goals(occ)
    grid = _grid(occ)
    a = nfopp.distance_fields(grid, _dev(goals, I32)).cpu().numpy()
    b = nfopp.distance_fields(grid, _dev(goals, I32)).cpu().numpy()
    assert np.array_equal(a, b), "two runs differ"
    return occ, goals, a


@functools.lru_cache(maxsize=None)
def _exact(shape, kind, goal):
    occ = gsr.make_map(kind, *shape)
    return gsr.fast_field(occ, goal) if occ.size > 10000 else gsr.dijkstra_field(occ, goal)


@pytest.mark.parametrize("kind", gsr.MAP_KINDS)
@pytest.mark.parametrize("shape", gsr.SHAPES, ids=lambda s: "%dx%d" % s)
def test_fields_equal_the_exact_field(shape, kind):
    rows, cols = shape
    occ, goals, got = _fields(shape, kind)
    lds = nfopp.load_library().nfopp_grid_fields_workspace_bytes(rows, cols, len(goals)) == 0
    assert lds == (gsr.SHAPES.index(shape) < gsr.SHAPES_LDS)
    big = rows * cols > 10000
    for j, g in enumerate(goals):
        if j >= 4:                                       # goals outside the grid
            assert (got[j] == -1).all(), (shape, kind, j)
        elif big and j >= 2:                             # the CPU side stays within seconds: proved, not recomputed
            assert gsr.is_exact_field(occ, g, got[j]), (shape, kind, j)
        else:
            want = _exact(shape, kind, tuple(int(v) for v in g))
            assert np.array_equal(got[j], want), (shape, kind, j, int((got[j] != want).any(-1).sum()))
    assert np.array_equal(got[2], got[0])                # the duplicate
    if kind == "full":
        for j in range(4):
            want = np.full((rows, cols, 2), -1, np.int32)
            want[tuple(goals[j])] = 0                    # only the goal, forced free
            assert np.array_equal(got[j], want)
    else:
        wall = occ != 0
        wall[tuple(goals[3])] = False
        assert (got[3][wall] == -1).all() and tuple(got[3][tuple(goals[3])]) == (0, 0)
    # the long-path cases of the packed format
    longest = int(got[:4, ..., 0].max())
    if (shape, kind) == ((189, 183), "serpentine") or (shape == (1, 12285) and kind in ("empty", "serpentine")):
        print(shape, kind, "largest straight count", longest)
        assert longest > 10000
    if shape in ((4094, 1), (4095, 1), (1, 12285), (1, 12286)) and kind in ("empty", "serpentine"):
        assert longest == rows * cols - 1                # from the far end of the corridor to the last cell


# ---- b. trace ---------------------------------------------------------------------------------------------------------
def _trace(fields, rows, cols, starts, goal_cells, field_index, max_len, batch=None):
    """nfopp_grid_trace_paths on sentinel-filled buffers with GUARD sentinel entries behind each.
    -> cells [B, max_len, 2], count [B], status [B], cost [B, 2] (numpy)."""
    lib = _lib.load()
    b = len(starts) if batch is None else batch
    cells = torch.full((b * max_len * 2 + GUARD,), SENT, dtype=I32, device="cuda")
    count = torch.full((b + GUARD,), SENT, dtype=I32, device="cuda")
    status = torch.full((b + GUARD,), SENT, dtype=I32, device="cuda")
    cost = torch.full((2 * b + GUARD,), SENT, dtype=I32, device="cuda")
    _lib.check(lib.nfopp_grid_trace_paths(_lib.ptr(fields, I32), fields.shape[0], rows, cols, _lib.ptr(starts, I32),
                                          _lib.ptr(goal_cells, I32), _lib.ptr(field_index, I32), b, max_len,
                                          _lib.ptr(cells, I32) if max_len else None, _lib.ptr(count, I32),
                                          _lib.ptr(status, I32), _lib.ptr(cost, I32), _lib.stream_ptr()))
    cells, count, status, cost = [t.cpu().numpy() for t in (cells, count, status, cost)]
    for t, n in ((cells, b * max_len * 2), (count, b), (status, b), (cost, 2 * b)):
        assert (t[n:] == SENT).all(), "written behind the batch"
    return cells[:b * max_len * 2].reshape(b, max_len, 2), count[:b], status[:b], cost[:2 * b].reshape(b, 2)


def _trace_problems(shape, kind):
    """Starts (every cell, or 4096 random ones on the large grid; walls included) towards the goals 0, 1 and 3 of the
    field test, then the refused problems.  -> (fields, starts, goal_cells, field_index, reference tuple)."""
    rows, cols = shape
    occ, goals, fields = _fields(shape, kind)
    if rows * cols <= 4096:
        cells = np.argwhere(np.ones(shape, bool))
    else:
        rng = np.random.default_rng(rows)
        cells = np.stack([rng.integers(0, rows, 4096), rng.integers(0, cols, 4096)], 1)
        cells[:3] = goals[[0, 1, 3]]                     # start == goal is among them
    starts, goal_cells, fidx, ref = [], [], [], []
    for g in (0, 1, 3):
        starts.append(cells)
        goal_cells.append(np.repeat(goals[g][None], len(cells), 0))
        fidx.append(np.full(len(cells), g))
        ref.append(gsr.trace_paths(fields[g], cells))    # fields[g] is exact: test_fields_equal_the_exact_field
    # refused: field_index -1 and n_fields, start (-1, 0) and (rows, 0), a goal cell outside the grid
    n_bad = 5
    starts.append(np.asarray([(0, 0), (0, 0), (-1, 0), (rows, 0), (0, 0)]))
    goal_cells.append(np.asarray([goals[0], goals[0], goals[0], goals[0], goals[4]]))
    fidx.append(np.asarray([-1, len(goals), 0, 0, 4]))
    L = max(r[0].shape[1] for r in ref)
    want_cells = np.zeros((sum(len(s) for s in starts), L, 2), np.int32)
    k = 0
    for r in ref:
        want_cells[k:k + len(r[0]), :r[0].shape[1]] = r[0]
        k += len(r[0])
    want_count = np.concatenate([r[1] for r in ref] + [np.zeros(n_bad, np.int32)])
    want_status = np.concatenate([r[2] for r in ref] + [np.full(n_bad, 2, np.int32)])
    want_cost = np.concatenate([r[3] for r in ref] + [np.full((n_bad, 2), -1, np.int32)])
    return (_dev(fields, I32), _dev(np.concatenate(starts), I32), _dev(np.concatenate(goal_cells), I32),
            _dev(np.concatenate(fidx), I32), (want_cells, want_count, want_status, want_cost))


def _check_cells(cells, max_len, want_cells, want_count):
    """Exactly min(count, max_len) cells of each path are written, the rest of the buffer keeps the sentinel."""
    k = np.arange(max_len)[None, :]
    written = k < np.minimum(want_count, max_len)[:, None]
    assert (cells[~written] == SENT).all(), "cells written beyond min(count, max_len)"
    assert np.array_equal(cells[written], want_cells[:, :max_len][written])


@pytest.mark.parametrize("kind", ["empty", "random"])
@pytest.mark.parametrize("shape", [(13, 15), (64, 64), (190, 190)], ids=lambda s: "%dx%d" % s)
def test_trace_follows_the_documented_rule(shape, kind):
    rows, cols = shape
    fields, starts, goal_cells, fidx, (want_cells, want_count, want_status, want_cost) = _trace_problems(shape, kind)
    assert (want_count[want_status == 0] >= 1).all() and (want_count == 1).any()      # start == goal is among them
    if (shape, kind) == ((64, 64), "random"):
        assert (want_status == 1).any()                                 # cut-off cells: no way
    ok = np.flatnonzero(want_status == 0)
    probe = int(np.sort(want_count[ok])[len(ok) // 2])                  # a median path: others are shorter and longer
    assert probe >= 3
    for max_len in (0, 1, probe - 1, probe + 3, int(want_count.max())):
        cells, count, status, cost = _trace(fields, rows, cols, starts, goal_cells, fidx, max_len)
        assert np.array_equal(count, want_count), max_len               # always the full length
        assert np.array_equal(status, want_status) and np.array_equal(cost, want_cost), max_len
        _check_cells(cells, max_len, want_cells, want_count)
    for batch in (257, 513):                                            # the 256-thread tail
        cells, count, status, cost = _trace(fields, rows, cols, starts, goal_cells, fidx, probe, batch=batch)
        assert np.array_equal(count, want_count[:batch]) and np.array_equal(status, want_status[:batch])
        assert np.array_equal(cost, want_cost[:batch])
        _check_cells(cells, probe, want_cells[:batch], want_count[:batch])


def test_trace_start_without_a_way():
    occ = np.zeros((9, 9), np.uint8)
    occ[1:6, 1:6] = 1                      # a 5 x 5 block of walls ...
    occ[3, 3] = 0                          # ... around one free cell
    goal = (8, 8)
    field = gsr.dijkstra_field(occ, goal)
    got = nfopp.distance_fields(_grid(occ), _dev([goal], I32))
    assert np.array_equal(got.cpu().numpy()[0], field)
    # the enclosed free cell and the wall cells that touch nothing but it: no way.  The corner wall cells leave over a
    # free neighbour, (5, 5) diagonally; the goal itself is a path of one cell.
    starts = np.asarray([(3, 3), (3, 2), (4, 4), (2, 2), (1, 1), (5, 5), (8, 8), (0, 0)])
    want = gsr.trace_paths(field, starts)
    assert list(want[2]) == [1, 1, 1, 1, 0, 0, 0, 0] and tuple(want[0][5, 1]) == (6, 6) and want[1][6] == 1
    L = int(want[1].max())
    cells, count, status, cost = _trace(got[0:1].contiguous(), 9, 9, _dev(starts, I32),
                                        _dev(np.repeat([goal], len(starts), 0), I32), _dev(np.zeros(len(starts)), I32), L)
    assert np.array_equal(status, want[2]) and np.array_equal(count, want[1]) and np.array_equal(cost, want[3])
    _check_cells(cells, L, want[0], want[1])
    assert count[6] == 1 and tuple(cost[6]) == (0, 0) and (cost[:4] == -1).all() and (count[:4] == 0).all()


# ---- c. seeding -------------------------------------------------------------------------------------------------------
SEED_GRID = None


def _seed_grid():
    global SEED_GRID
    if SEED_GRID is None:   # the seeding stage reads the geometry only
        SEED_GRID = nfopp.OccupancyGrid(np.zeros((4, 4), np.uint8), gsr.SEED_BOUNDARIES, gsr.SEED_RESOLUTION, device="cuda")
    return SEED_GRID


@functools.lru_cache(maxsize=None)
def _seed_ref(name, n):
    case = [c for c in gsr.seed_cases() if c["name"] == name][0]
    return gsr.seed_reference(case, n)


def _seed(rows, max_len, n, D, directed):
    """rows: list of (cells [count, 2] or None, count, status, start [3], goal [3]) -> fp32 [B, n, D]; the output sits
    between two sentinel rows, which must stay untouched."""
    B = len(rows)
    cells = np.zeros((B, max_len, 2), np.int32)
    for i, (c, _, _, _, _) in enumerate(rows):
        if c is not None:
            cells[i, :min(len(c), max_len)] = c[:max_len]
    counts = np.asarray([r[1] for r in rows], np.int32)
    status = np.asarray([r[2] for r in rows], np.int32)
    starts = _dev(np.stack([r[3][:D] for r in rows]))
    goals = _dev(np.stack([r[4][:D] for r in rows]))
    buf = torch.full((B + 2, n, D), 12345.0, dtype=torch.float32, device="cuda")
    out = nfopp.seed_trajectories(_seed_grid(), _dev(cells, I32), _dev(counts, I32), _dev(status, I32), starts, goals, n,
                                  directed, out=buf[1:-1])
    buf = buf.cpu().numpy()
    assert (buf[0] == 12345.0).all() and (buf[-1] == 12345.0).all(), "a neighbouring row was written"
    line = nfopp.init_trajectories(starts, goals, n, bool(directed and D == 3)).cpu().numpy()
    return out.cpu().numpy(), line


def _xy_gate(got, ref, what):
    bound = np.spacing(np.abs(ref).astype(F32)).astype(np.float64) + 8 * gsr.SPREAD
    err = np.abs(got.astype(np.float64) - ref)
    print("%s: max xy err %.3e m, worst err / bound %.3f" % (what, err.max(), (err / bound).max()))
    assert (err <= bound).all(), (what, float(err.max()), float((err / bound).max()))


def _directed64(xy, start, goal, th):
    """initialize_angle_with_trajectory_direction (trajectory_initializer.py:32-41) in float64: xy fp32 [N, 2] as the
    kernel wrote them, th fp32 [N] the undirected headings."""
    n = len(xy)
    full = np.concatenate([start[None, :2], xy, goal[None, :2]]).astype(np.float64)
    angles = np.arctan2(full[2:, 1] - full[:-2, 1], full[2:, 0] - full[:-2, 0])
    w = torch.cat([torch.linspace(0., 1, n // 2), torch.linspace(1., 0, (n + 1) // 2)]).numpy().astype(np.float64)
    th = th.astype(np.float64)
    return th + ((angles - th + np.pi) % (2 * np.pi) - np.pi) * w


@pytest.mark.parametrize("n", gsr.SEED_NS)
@pytest.mark.parametrize("D", [2, 3])
def test_seeding_against_the_float64_spline(D, n):
    cases = {c["name"]: c for c in gsr.seed_cases()}
    lib = _lib.load()

    def good(name):
        c = cases[name]
        return (c["cells"], len(c["cells"]), 0, c["start"], c["goal"], name)

    def bad(kind, name, max_len):
        c = cases[name]
        cells = c["cells"][:max_len]
        count, status = {"unreachable": (len(cells), 1), "outside": (len(cells), 2), "empty": (0, 0),
                         "too long": (max_len + 1, 0)}[kind]
        return (cells, count, status, c["start"], c["goal"], None)

    def batch(names, max_len):
        rows = [bad("unreachable", "c40", max_len)]
        for i, name in enumerate(names):
            rows.append(good(name))
            if i == 1:
                rows.append(bad("outside", "c3", max_len))
            if i == 2:
                rows.append(bad("empty", "c2", max_len))
        rows.append(bad("too long", "row1168", max_len))
        return rows

    small = ["c1", "c2", "c3", "c40"]
    batches = [("LDS, max_len 40", batch(small, 40), 40),
               ("LDS, max_len 1167", batch(small + ["row1167"], 1167), 1167),
               ("workspace, max_len 1168", batch(small + ["row1167", "row1168"], 1168), 1168),
               ("workspace, max_len 3000", batch(small + ["row1167", "row1168", "serp3000"], 3000), 3000)]
    seen = {}
    for what, rows, max_len in batches:
        assert (lib.nfopp_grid_seed_workspace_bytes(len(rows), max_len) == 0) == what.startswith("LDS")
        plain, line = _seed([r[:5] for r in rows], max_len, n, D, False)
        settings = [(False, plain, line)]
        if D == 3:
            settings.append((True,) + _seed([r[:5] for r in rows], max_len, n, D, True))
        for directed, got, ln in settings:
            for i, r in enumerate(rows):
                name = r[5]
                tag = "%s D=%d N=%d dir=%d row %d (%s)" % (what, D, n, directed, i, name)
                if name is None:                                        # exactly the stock initialiser's trajectory
                    assert np.array_equal(got[i], ln[i]), tag
                    continue
                assert np.array_equal(got[i][:, :2], plain[i][:, :2]), tag         # headings do not move xy
                if not directed:
                    _xy_gate(got[i][:, :2], _seed_ref(name, n), tag)
                    # the same path in a longer buffer, in LDS or in the workspace: the same bits
                    assert np.array_equal(got[i], seen.setdefault(name, got[i])), tag
                    if D == 3:
                        assert np.array_equal(got[i][:, 2], ln[i][:, 2]), tag
                elif cases[name]["directed"] and n in gsr.SEED_DIRECTED_NS:
                    want = _directed64(got[i][:, :2], r[3], r[4], plain[i][:, 2])
                    err = np.abs(got[i][:, 2].astype(np.float64) - want).max()
                    print("%s: max heading err %.3e rad" % (tag, err))
                    assert err < 1e-6, (tag, float(err))
    assert set(seen) == set(cases)


def test_directed_seeding_of_2d_trajectories_is_refused():
    lib = _lib.load()
    c = gsr.seed_cases()[3]
    cells, counts, status = _dev(c["cells"][None], I32), _dev([len(c["cells"])], I32), _dev([0], I32)
    start, goal = _dev(c["start"][None, :2]), _dev(c["goal"][None, :2])
    out = torch.full((1, 16, 2), 12345.0, dtype=torch.float32, device="cuda")
    b = gsr.SEED_BOUNDARIES

    def call(directed):
        return lib.nfopp_grid_seed_trajectories(_lib.ptr(cells, I32), _lib.ptr(counts, I32), _lib.ptr(status, I32), 1,
                                                cells.shape[1], _lib.ptr(start), _lib.ptr(goal), 16, 2, directed, b[0], b[2],
                                                gsr.SEED_RESOLUTION, _lib.ptr(out), None, 0, _lib.stream_ptr())

    assert call(1) == -1
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all())
    assert call(0) == 0
    _xy_gate(out.cpu().numpy()[0], _seed_ref("c40", 16), "C entry, D=2")


# ---- d. end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_end_to_end_on_a_grid_beyond_the_lds_kernel(D):
    shape, n, B = (190, 190), 257, 300
    rows, cols = shape
    occ = gsr.make_map("random", *shape).copy()
    occ[10:15, 10:15] = 1
    occ[11:14, 11:14] = 0                             # a walled-in pocket of free cells
    grid = _grid(occ, origin=1.0)                     # coordinates from 1 m up: an fp32 ulp there is above 1e-7
    goal_cells = gsr.shape_goals(occ)[[0, 1, 3]]
    fields = [gsr.fast_field(occ, g) for g in goal_cells]
    rng = np.random.default_rng(300)
    sc = np.stack([rng.integers(0, rows, B), rng.integers(0, cols, B)], 1)
    sc[:3] = [(11, 11), (12, 12), (13, 11)]                             # free cells that cannot reach the goals: status 1
    gi = rng.integers(0, 3, B)
    gi[:3] = 0
    gc = goal_cells[gi].astype(np.int64)
    sc[3], gc[4], gc[5] = (-1, 4), (2, cols), (rows, 0)   # off the grid: status 2

    def points(cells):   # at least 0.05 cell from the centre and from the edges
        off = rng.uniform(0.05, 0.45, (B, 2)) + 0.5 * rng.integers(0, 2, (B, 2))
        xy = 1.0 + cells[:, ::-1] + off
        return np.concatenate([xy, rng.uniform(-3, 3, (B, 1))], 1).astype(F32)[:, :D]

    starts, goals = points(sc), points(gc)
    assert np.array_equal(gsr.cells_of(starts, grid.boundaries, 1.0), sc)
    assert np.array_equal(gsr.cells_of(goals, grid.boundaries, 1.0), gc)
    want_status = np.zeros(B, np.int32)
    want_cells = [None] * B
    want_cost = np.full((B, 2), -1, np.int32)
    for g in range(3):
        idx = np.flatnonzero((gi == g) & (np.arange(B) != 4) & (np.arange(B) != 5))
        cells, count, status, cost = gsr.trace_paths(fields[g], sc[idx])
        want_status[idx], want_cost[idx] = status, cost
        for j, i in enumerate(idx):
            want_cells[i] = cells[j, :count[j]]
    want_status[[4, 5]] = 2
    for i in (4, 5):
        want_cells[i] = np.zeros((0, 2), np.int32)
    assert list(want_status[:6]) == [1, 1, 1, 2, 2, 2] and (want_status == 0).sum() > B // 2
    cells, count, status, cost = [t.cpu().numpy() for t in nfopp.grid_search_paths(grid, _dev(starts), _dev(goals))]
    assert np.array_equal(status, want_status) and np.array_equal(cost, want_cost)
    for i in range(B):
        assert count[i] == len(want_cells[i]) and np.array_equal(cells[i, :count[i]], want_cells[i]), i
    for directed in ((False, True) if D == 3 else (False,)):
        traj, st = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), n, directed)
        assert np.array_equal(st.cpu().numpy(), want_status)
        traj = traj.cpu().numpy()
        line = nfopp.init_trajectories(_dev(starts), _dev(goals), n, directed).cpu().numpy()
        plain = nfopp.init_trajectories(_dev(starts), _dev(goals), n, False).cpu().numpy()
        worst = 0.0
        for i in range(B):
            if want_status[i] != 0:
                assert np.array_equal(traj[i], line[i]), i
                continue
            ref = gsr.reparametrize(gsr.polyline(want_cells[i], starts[i], goals[i], grid.boundaries, 1.0), n + 2)[1:-1]
            bound = np.spacing(np.abs(ref).astype(F32)).astype(np.float64) + 8 * gsr.SPREAD
            err = np.abs(traj[i][:, :2].astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (i, float(err.max()))
            if D == 3 and not directed:
                assert np.array_equal(traj[i][:, 2], plain[i][:, 2]), i
            elif D == 3:
                want = _directed64(traj[i][:, :2], starts[i], goals[i], plain[i][:, 2])
                full = np.concatenate([starts[i][None, :2], traj[i][:, :2], goals[i][None, :2]]).astype(np.float64)
                ang = np.arctan2(full[2:, 1] - full[:-2, 1], full[2:, 0] - full[:-2, 0]) - plain[i][:, 2]
                clear = np.abs(np.abs(ang) - np.pi) > 1e-3             # waypoints on the wrap may flip by 2 pi w
                assert np.abs(traj[i][:, 2].astype(np.float64) - want)[clear].max() < 1e-6, i
        print("D=%d directed=%d: worst xy err / bound %.3f" % (D, directed, worst))


# ---- one cell centre for the seeding stage, the any-angle shortening and the space-time search -------------------------------
def test_the_kernels_share_one_cell_centre():
    """A free 3 x 65 grid (65 columns: the last cell lies in the second 64-bit word of a reservation row) with boundaries
    (-0.3, 6.2, 0.2, 0.4) and resolution 0.1; a robot of radius 0 goes from cell (1, 0) to (1, 64) over 65 instants.  Its
    planned track, the any-angle points of the same 65 cells with lookahead 1 (every cell stays an anchor) and fp32 of the host
    frame's float64 centres are the same bits, and seeding those points gives what seeding the cells gives: the three kernels
    and the host form a centre one way (csrc/grid_frame.h, nfopp/_grid.py).

    This pins the sharing, not the `fp contract(off)` pragma of the shared function: a search on the CPU over 6 resolutions x
    5 origins x 4096 columns found no geometry where a fused multiply-add changes the fp32 centre.  The pragma stays because
    fractional coordinates and other geometries are not covered by that search."""
    import spacetime_ref as sr
    rows, cols, T = 3, 65, 65
    boundaries, res = (-0.3, 6.2, 0.2, 0.4), 0.1
    occ = np.zeros((rows, cols), np.uint8)
    grid = nfopp.OccupancyGrid(occ, boundaries, res, device="cuda")
    assert grid.cell_counts() == (cols, rows)
    path = np.stack([np.ones(T, np.int32), np.arange(T, dtype=np.int32)], 1)                # (row, col): (1, h)
    # the restated rule plans exactly these cells
    ref = sr.plan_fleet(sr.Reservation(occ, sr.Geometry(rows, cols, boundaries[0], boundaries[2], res), T, 0.0), [[1, 0]], [[1, 64]])
    assert ref["status"].tolist() == [0] and ref["arrival"].tolist() == [64]
    assert np.array_equal(ref["cells"][0], path[:, 0] * cols + path[:, 1])
    plan = nfopp.spacetime_plan(grid, _dev([[1, 0]], I32), _dev([[1, 64]], I32), T, robot_radius=0.0)
    assert plan.status.tolist() == [0] and np.array_equal(plan.cells[0].cpu().numpy(), ref["cells"][0])
    tracks = plan.tracks[0].cpu().numpy()
    cells, count, status = _dev(path[None], I32), _dev([T], I32), _dev([0], I32)
    points, point_counts, anchors, anchor_counts = nfopp.shorten_paths(grid, cells, count, status, lookahead=1)
    assert point_counts.tolist() == [T] and anchor_counts.tolist() == [T] and anchors[0].tolist() == list(range(T))
    x, y, x_cells, _ = grid.cell_centres()
    flat = path[:, 0] * x_cells + path[:, 1]
    want = np.stack([x[flat], y[flat]], 1).astype(F32)
    assert tracks.dtype == F32 and tracks.shape == (T, 2)
    assert tracks.tobytes() == want.tobytes()
    assert points[0].cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(tracks, ref["tracks"][0])
    starts, goals = _dev([[-0.27, 0.33]]), _dev([[6.13, 0.31]])
    assert grid.cells_of(starts).tolist() == [[1, 0]] and grid.cells_of(goals).tolist() == [[1, 64]]
    from_points = nfopp.seed_polylines(grid, points, point_counts, status, starts, goals, 8)
    from_cells = nfopp.seed_trajectories(grid, cells, count, status, starts, goals, 8)
    assert from_cells.shape == (1, 8, 2) and torch.isfinite(from_cells).all()
    assert from_points.cpu().numpy().tobytes() == from_cells.cpu().numpy().tobytes()
