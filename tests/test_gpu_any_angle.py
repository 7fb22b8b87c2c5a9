"""GPU: any-angle shortening of cell paths (csrc/grid_any_angle.hip), seeding through given polylines
(nfopp_grid_seed_polylines) and the `any_angle` flag of grid_search_init / AstarTrajectoryInitializer / BatchPlanner.init,
against the CPU restatement of tests/any_angle_ref.py (tests/test_any_angle_cpu.py checks that and the cases without a GPU).

Gates.  Anchors, counts and points: `==` (the points are compared as bytes).  Seeded xy against the float64 reference
spline of the restated dense polyline: one fp32 ulp of the coordinate + 8 x AA_SPREAD, the gate of
test_gpu_grid_search_shapes.py with the spread measured on these cases.  Undirected headings and every straight-line
fallback row: bit-identical to nfopp.init_trajectories.  Directed headings: 1e-6 against
initialize_angle_with_trajectory_direction restated in float64 on the xy the kernel itself wrote."""
import functools

import numpy as np
import pytest
import torch

import nfopp
from nfopp import _lib

import any_angle_ref as aar
import edt_ref as er
import grid_search_ref as gsr

pytestmark = pytest.mark.gpu
FX = gsr.load_fixture()
F32 = np.float32
I32 = torch.int32
SENT, FSENT = -7, 12345.0      # sentinels of the integer and the fp32 output buffers
GUARD = 300                    # sentinel entries behind every output buffer
BIG = 2 ** 30


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _grid(m):
    return nfopp.OccupancyGrid(m["occ"], m["boundaries"], m["resolution"], device="cuda")


@functools.lru_cache(maxsize=None)
def _map(k):
    m = gsr.fixture_map(FX, k)
    return m, er.edt(m["occ"])[0], aar.traced_paths(m)


GEOM = ((-3.0, 400.0, 2.0, 400.0), 0.25)     # boundaries and resolution of the hand-made cases: x crosses zero


def _run(dist2, rows, lookahead, max_len, max_points=None, cells2=None, batch=None, want_points=True, geom=GEOM):
    """nfopp_grid_shorten_paths on sentinel-filled buffers.  rows: list of (cells [k, 2], count, status).
    -> anchors [B, max_len], anchor_count [B], points fp32 [B, max_points, 2] or None, point_count [B] (numpy)."""
    lib = _lib.load()
    B = len(rows) if batch is None else batch
    max_points = max_len if max_points is None else max_points
    cells = np.zeros((len(rows), max_len, 2), np.int32)
    for i, (c, _, _) in enumerate(rows):
        c = np.asarray(c, np.int32).reshape(-1, 2)[:max_len]
        cells[i, :len(c)] = c
    count = _dev([r[1] for r in rows], I32)
    status = _dev([r[2] for r in rows], I32)
    d2 = _dev(dist2, I32)
    anchor = torch.full((B * max_len + GUARD,), SENT, dtype=I32, device="cuda")
    anchor_count = torch.full((B + GUARD,), SENT, dtype=I32, device="cuda")
    point_count = torch.full((B + GUARD,), SENT, dtype=I32, device="cuda")
    points = torch.full((B * max_points * 2 + GUARD,), FSENT, dtype=torch.float32, device="cuda")
    c2 = None if cells2 is None else _dev(cells2, I32)
    (b0, _, b2, _), res = geom
    rc = lib.nfopp_grid_shorten_paths(_lib.ptr(d2, I32), dist2.shape[0], dist2.shape[1], _lib.ptr(_dev(cells, I32), I32),
                                      _lib.ptr(count, I32), _lib.ptr(status, I32), _lib.ptr(c2, I32), B, max_len, lookahead,
                                      _lib.ptr(anchor, I32), _lib.ptr(anchor_count, I32), b0, b2, res, max_points,
                                      _lib.ptr(points) if want_points else None, _lib.ptr(point_count, I32), _lib.stream_ptr())
    assert rc == 0, lib.nfopp_last_error()
    anchor, anchor_count, point_count, points = [t.cpu().numpy() for t in (anchor, anchor_count, point_count, points)]
    for t, n, s in ((anchor, B * max_len, SENT), (anchor_count, B, SENT), (point_count, B, SENT), (points, B * max_points * 2, FSENT)):
        assert (t[n:] == s).all(), "written behind the batch"
    if not want_points:
        assert (points == FSENT).all()
    return (anchor[:B * max_len].reshape(B, max_len), anchor_count[:B],
            points[:B * max_points * 2].reshape(B, max_points, 2) if want_points else None, point_count[:B])


_WANT = {}


def _want(dist2, key, thr, path, lookahead, geom):
    """aar.shorten, remembered: the batches repeat paths."""
    k = (key, thr, path.tobytes(), lookahead, geom)
    if k not in _WANT:
        _WANT[k] = aar.shorten(dist2, thr, path, lookahead, geom[0], geom[1])
    return _WANT[k]


def _check(dist2, rows, lookahead, max_len, max_points=None, cells2=None, batch=None, want_points=True, geom=GEOM, what=""):
    """The kernel's rows against the restatement; what lies behind a row's counts, and the whole of a refused row, keeps the
    sentinel.  -> the raw outputs."""
    got = _run(dist2, rows, lookahead, max_len, max_points, cells2, batch, want_points, geom)
    anchor, anchor_count, points, point_count = got
    B = len(anchor_count)
    max_points = max_len if max_points is None else max_points
    key = (dist2.shape, hash(np.asarray(dist2, np.int64).tobytes()))
    for i in range(B):
        c, n, st = rows[i]
        c = np.asarray(c, np.int64).reshape(-1, 2)
        tag = (what, lookahead, i)
        if st != 0 or n < 1 or n > max_len or not aar.in_grid(c[:n], dist2.shape):
            assert anchor_count[i] == 0 and point_count[i] == 0, tag
            assert (anchor[i] == SENT).all() and (points is None or (points[i] == FSENT).all()), tag
            continue
        thr = 0 if cells2 is None else int(cells2[i])
        want_a, want_p = _want(dist2, key, thr, c[:n], lookahead, geom)
        assert anchor_count[i] == len(want_a) and point_count[i] == len(want_p), tag + (anchor_count[i], len(want_a))
        assert np.array_equal(anchor[i, :len(want_a)], want_a) and (anchor[i, len(want_a):] == SENT).all(), tag
        if points is not None:
            k = min(len(want_p), max_points)
            assert points[i, :k].tobytes() == want_p[:k].tobytes(), tag
            assert (points[i, k:] == FSENT).all(), tag
    return got


def _bad_rows(path):
    """Refused rows: status 1 and 2, count 0 and a negative count (the callers add count > max_len and a cell outside)."""
    return [(path, len(path), 1), (path, len(path), 2), (path, 0, 0), (path, -3, 0)]


# ---- a. the kernel against the restatement -------------------------------------------------------------------------------
def _occ(kind, rows, cols):
    if kind == "p0.2":
        return (np.random.default_rng(7 * rows + cols).uniform(size=(rows, cols)) < 0.2).astype(np.uint8)
    return gsr.make_map({"p0.3": "random"}.get(kind, kind), rows, cols)


@functools.lru_cache(maxsize=None)
def _paths_on(kind, rows, cols):
    """Traced paths towards three goals from starts spread over the grid (walls included: the start is untested)."""
    occ = _occ(kind, rows, cols)
    rng = np.random.default_rng(rows * 1009 + cols)
    goals = gsr.shape_goals(occ)[[0, 1, 3]]
    paths = []
    for g in goals:
        field = gsr.fast_field(occ, g) if occ.size > 1000 else gsr.dijkstra_field(occ, g)
        starts = np.stack([rng.integers(0, rows, 4), rng.integers(0, cols, 4)], 1)
        starts[0] = (0, 0)
        for s in starts:
            p = gsr.trace_path(field, s)[0]
            if len(p):
                paths.append(p)
    return occ, er.edt(occ)[0], paths


@pytest.mark.parametrize("kind", ["p0.2", "p0.3", "serpentine", "empty"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (13, 15), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_restatement(shape, kind):
    occ, dist2, paths = _paths_on(kind, *shape)
    assert len(paths) >= 1
    longest = max(len(p) for p in paths)
    if shape == (64, 64) and kind == "serpentine":
        assert longest > 1500                              # a maze path: many anchors, many rounds
        paths = sorted(paths, key=len)[-1:] + sorted(paths, key=len)[:2]
    rows = [(p, len(p), 0) for p in paths]
    rows[1:1] = _bad_rows(paths[0])
    rows.append((np.concatenate([paths[0], [(shape[0], 0)]]), len(paths[0]) + 1, 0))           # a cell outside the grid
    rows.append((paths[0], longest + 2, 0))                                                     # count > max_len
    max_len = longest + 1
    for lookahead in (1, 63, 64, 65, max_len, BIG):
        if longest > 1500 and lookahead in (63, 65, max_len):
            continue                                       # the CPU restatement of a maze path takes seconds per value
        _check(dist2, rows, lookahead, max_len, what=(shape, kind))


@pytest.mark.parametrize("lookahead", [1, 63, 64, 65, 129, BIG])
def test_round_edges_on_an_empty_grid(lookahead):
    """Path counts around the rounds of a 64-lane scan: a straight row and a staircase (one diagonal in three moves)."""
    dist2 = np.full((70, 130), er.NONE, np.int64)
    stair = np.stack([np.arange(129) // 3 + 2, np.arange(129)], 1)
    row = np.stack([np.full(129, 69), np.arange(129)[::-1]], 1)          # leftwards along the last row
    rows = [(p[:n], n, 0) for n in (1, 2, 3, 63, 64, 65, 66, 129) for p in (row, stair)]
    anchor, anchor_count, _, point_count = _check(dist2, rows, lookahead, 129, what="empty")
    assert np.array_equal(point_count, [r[1] for r in rows])             # nothing in the way: as many points as cells
    if lookahead >= 129:
        assert (anchor_count == np.minimum([r[1] for r in rows], 2)).all()


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 257])
def test_batch_edges(batch):
    """The edges of the wavefronts of a workgroup; rows behind the batch are not touched (_run's guard)."""
    m, dist2, paths = _map(1)
    rows = [(paths[i % 32], len(paths[i % 32]), 0) if i % 7 != 3 else (paths[i % 32], len(paths[i % 32]), 1 + i % 2)
            for i in range(batch)]
    _check(dist2, rows, 256, max(len(p) for p in paths), batch=batch, geom=(m["boundaries"], m["resolution"]), what="m1")


def test_refused_rows_short_buffers_and_optional_arguments():
    m, dist2, paths = _map(1)
    geom = (m["boundaries"], m["resolution"])
    max_len = max(len(p) for p in paths)
    rows = [(p, len(p), 0) for p in paths]
    rows[3:3] = _bad_rows(paths[3])
    rows.append((paths[1], max_len + 1, 0))
    full = _check(dist2, rows, 256, max_len, geom=geom, what="m1")
    again = _check(dist2, rows, 256, max_len, geom=geom, what="m1 again")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again))                       # a second run: the same bytes
    zero = _check(dist2, rows, 256, max_len, cells2=np.zeros(len(rows), np.int32), geom=geom, what="m1 zero thresholds")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, zero))                        # null = all 0
    # fewer point slots than points: the count is reported, the prefix written
    short = sorted(len(p) for p in paths)[len(paths) // 2]
    for max_points in (0, 1, short - 1, short):
        got = _check(dist2, rows, 256, max_len, max_points=max_points, geom=geom, what="m1 max_points %d" % max_points)
        assert np.array_equal(got[3], full[3]) and np.array_equal(got[0], full[0])
        assert (got[3] > max_points).any()
    none = _check(dist2, rows, 256, max_len, want_points=False, geom=geom, what="m1 no points")
    assert np.array_equal(none[0], full[0]) and np.array_equal(none[1], full[1]) and np.array_equal(none[3], full[3])


def test_thresholds_mixed_in_one_batch():
    m, dist2, plain = _map(2)
    paths, thr = aar.level_paths(m, [4, 1])
    rows = [(p, len(p), 0) for p in paths] + [(p, len(p), 0) for p in plain if len(p)]
    cells2 = np.asarray(thr + [0] * (len(rows) - len(thr)), np.int32)
    assert all((cells2 == v).sum() >= 4 for v in (0, 1, 4))
    max_len = max(len(r[0]) for r in rows)
    anchor, anchor_count, _, _ = _check(dist2, rows, 256, max_len, cells2=cells2, geom=(m["boundaries"], m["resolution"]), what="m2")
    # the thresholds matter: with all of them 0 some row of a level is shortened further
    a0, c0, _, _ = _check(dist2, rows, 256, max_len, geom=(m["boundaries"], m["resolution"]), what="m2 at 0")
    assert (c0[:len(thr)] < anchor_count[:len(thr)]).any()


def test_rejected_arguments_leave_the_buffers_alone():
    lib = _lib.load()
    buf = torch.full((64,), SENT, dtype=I32, device="cuda")
    pts = torch.full((64,), FSENT, dtype=torch.float32, device="cuda")
    one = torch.ones(1, dtype=I32, device="cuda")

    def call(rows=4, cols=4, lookahead=4):
        return lib.nfopp_grid_shorten_paths(_lib.ptr(buf, I32), rows, cols, _lib.ptr(buf, I32), _lib.ptr(one, I32), _lib.ptr(one, I32),
                                            None, 1, 4, lookahead, _lib.ptr(buf, I32), _lib.ptr(buf, I32), 0.0, 0.0, 1.0, 4,
                                            _lib.ptr(pts), _lib.ptr(buf, I32), _lib.stream_ptr())

    assert call(lookahead=0) == -1 and b"lookahead" in lib.nfopp_last_error()
    assert call(rows=4097) == -1 and b"4096" in lib.nfopp_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()) and bool((pts == FSENT).all())
    grid = _grid(_map(2)[0])
    with pytest.raises(ValueError):
        nfopp.shorten_paths(grid, np.zeros((1, 2, 2)), [2], [0], cells2=[-1])
    with pytest.raises(ValueError):
        nfopp.shorten_paths(grid, np.zeros((1, 2, 2)), [2], [0], cells2=_dev([-1], I32))


# ---- b. seeding ----------------------------------------------------------------------------------------------------------
def _padded(paths):
    L = max(max(len(p) for p in paths), 1)
    cells = np.zeros((len(paths), L, 2), np.int32)
    for i, p in enumerate(paths):
        cells[i, :len(p)] = p
    return cells, np.asarray([len(p) for p in paths], np.int32)


@pytest.mark.parametrize("n", [1, 2, 100, 257])
@pytest.mark.parametrize("D", [2, 3])
def test_polylines_of_cell_centres_seed_as_the_cells_do(D, n):
    for k in (1, 3):
        m, _, paths = _map(k)
        grid = _grid(m)
        cells, counts = _padded(paths)
        status = np.zeros(len(paths), np.int32)
        status[2], counts[5] = 1, 0                                   # fallback rows are the same rows
        points = np.zeros(cells.shape, F32)
        for i, p in enumerate(paths):
            points[i, :len(p)] = gsr.polyline(p, (0, 0), (0, 0), m["boundaries"], m["resolution"])[1:-1]
        starts, goals = _dev(m["starts"][:, :D]), _dev(m["goals"][:, :D])
        for directed in ((False, True) if D == 3 else (False,)):
            want = nfopp.seed_trajectories(grid, _dev(cells, I32), _dev(counts, I32), _dev(status, I32), starts, goals, n, directed)
            buf = torch.full((len(paths) + 2, n, D), FSENT, dtype=torch.float32, device="cuda")
            got = nfopp.seed_polylines(grid, _dev(points), _dev(counts, I32), _dev(status, I32), starts, goals, n, directed,
                                       out=buf[1:-1])
            assert torch.equal(got, want), (k, D, n, directed)
            assert bool((buf[0] == FSENT).all()) and bool((buf[-1] == FSENT).all())


@pytest.mark.parametrize("k", [3, 4])
def test_nothing_to_shorten_is_todays_seed_bit_for_bit(k):
    m = gsr.fixture_map(FX, k)
    grid = _grid(m)
    res = m["resolution"]
    starts, goals = _dev(m["starts"]), _dev(m["goals"])
    for directed in (False, True):
        for clearance in (None, res, [2 * res, res]):
            want = nfopp.grid_search_init(grid, starts, goals, 100, directed, clearance=clearance)
            got = nfopp.grid_search_init(grid, starts, goals, 100, directed, clearance=clearance, any_angle=True)
            assert len(got) == len(want) == (2 if clearance is None else 3)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (k, directed, clearance)


def _directed64(xy, start, goal, th):
    """initialize_angle_with_trajectory_direction (trajectory_initializer.py:32-41) in float64: xy fp32 [N, 2] as the
    kernel wrote them, th fp32 [N] the undirected headings."""
    n = len(xy)
    full = np.concatenate([start[None, :2], xy, goal[None, :2]]).astype(np.float64)
    angles = np.arctan2(full[2:, 1] - full[:-2, 1], full[2:, 0] - full[:-2, 0])
    w = torch.cat([torch.linspace(0., 1, n // 2), torch.linspace(1., 0, (n + 1) // 2)]).numpy().astype(np.float64)
    th = th.astype(np.float64)
    return th + ((angles - th + np.pi) % (2 * np.pi) - np.pi) * w, np.abs(np.abs(angles - th) - np.pi) > 1e-3


@pytest.mark.parametrize("k", [1, 2])
def test_any_angle_seeds_against_the_float64_spline(k):
    m, dist2, paths = _map(k)
    grid = _grid(m)
    n = aar.SEED_N
    starts, goals = _dev(m["starts"]), _dev(m["goals"])
    line = nfopp.init_trajectories(starts, goals, n, False).cpu().numpy()
    plain = nfopp.grid_search_init(grid, starts, goals, n)[0].cpu().numpy()
    worst, moved = 0.0, 0
    ulp = float(np.spacing(np.abs(np.asarray(m["boundaries"], F32)).max()))
    for directed in (False, True):
        traj, status = nfopp.grid_search_init(grid, starts, goals, n, directed, any_angle=True)
        traj, status = traj.cpu().numpy(), status.cpu().numpy()
        assert np.array_equal(status == 0, [len(p) > 0 for p in paths])
        for i, p in enumerate(paths):
            if not len(p):
                want = nfopp.init_trajectories(starts[i:i + 1], goals[i:i + 1], n, directed).cpu().numpy()[0]
                assert np.array_equal(traj[i], want), i
                continue
            _, pts = aar.shorten(dist2, 0, p, 256, m["boundaries"], m["resolution"])
            ref = aar.seed_reference(pts, m["starts"][i], m["goals"][i], n)
            bound = np.spacing(np.abs(ref).astype(F32)).astype(np.float64) + 8 * aar.AA_SPREAD
            err = np.abs(traj[i][:, :2].astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (k, i, float(err.max()), float((err / bound).max()))
            # where the two float64 splines lie further apart than both gates, the two seeds differ
            cell_ref = gsr.reparametrize(gsr.polyline(p, m["starts"][i], m["goals"][i], m["boundaries"], m["resolution"]), n + 2)[1:-1]
            if np.abs(ref - cell_ref).max() > 4 * (ulp + 8 * aar.AA_SPREAD):
                assert not np.array_equal(traj[i][:, :2], plain[i][:, :2]), i
                moved += 1
            if not directed:
                assert np.array_equal(traj[i][:, 2], line[i][:, 2]), i              # the ramp of init_trajectories
            else:
                want, clear = _directed64(traj[i][:, :2], m["starts"][i], m["goals"][i], line[i][:, 2])
                assert np.abs(traj[i][:, 2].astype(np.float64) - want)[clear].max() < 1e-6, i
    print("map %d: worst xy err / bound %.3f, %d seeds differ from the cell-path seed" % (k, worst, moved))
    assert moved >= 2 * 8                                   # the flag does something on these maps


# ---- c. the public surface -------------------------------------------------------------------------------------------------
def _host_checker(m):
    """A host checker that reads the fixture's occupancy (cell = floor((x - b0) / resolution))."""
    class Checker(object):
        def get_boundaries(self):
            return m["boundaries"]

        def check_collision(self, positions):
            rc = gsr.cells_of(np.stack([np.asarray(positions.x), np.asarray(positions.y)], 1), m["boundaries"], m["resolution"])
            ok = (rc >= 0).all(1) & (rc[:, 0] < m["occ"].shape[0]) & (rc[:, 1] < m["occ"].shape[1])
            out = np.ones(len(rc), bool)
            out[ok] = m["occ"][rc[ok, 0], rc[ok, 1]] != 0
            return out
    return Checker()


@pytest.mark.parametrize("with_clearance", [False, True])
def test_initializer_and_batch_planner_pass_the_flag_on(with_clearance):
    import gpu_common as gc
    m = gsr.fixture_map(FX, 1)
    grid = _grid(m)
    res = m["resolution"]
    clearance = res if with_clearance else None
    B, N = 8, 32
    z = np.load(gsr.GOLDEN.replace("g19_astar_init", "g1_onf"), allow_pickle=False)
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    starts, goals = m["starts"][:B], m["goals"][:B]
    for directed in (False, True):
        plain = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), N, directed, clearance=() if clearance is None else clearance)
        want = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), N, directed, clearance=() if clearance is None else clearance,
                                      any_angle=True)
        assert len(want) == 3 and not torch.equal(want[0], plain[0])
        assert torch.equal(want[1], plain[1]) and torch.equal(want[2], plain[2])           # same searches, same levels
        assert bool((want[2] > 0).any()) == with_clearance
        if clearance is None:
            two = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), N, directed, any_angle=True)
            assert len(two) == 2 and torch.equal(two[0], want[0]) and torch.equal(two[1], want[1])
        ini = nfopp.AstarTrajectoryInitializer(_host_checker(m), res, directed, clearance=clearance, any_angle=True)
        got = ini.initialize_batch(_dev(starts), _dev(goals), N)
        assert torch.equal(got, want[0]) and torch.equal(ini.status, want[1]) and torch.equal(ini.seed_margin, want[2])
        bp = nfopp.BatchPlanner(onf, B, N, nfopp.TrajectoryHyper(), init_angles_with_trajectory=directed)
        bp.init(starts, goals, m["boundaries"], initializer=grid, seed_clearance=clearance, seed_any_angle=True)
        assert torch.equal(bp.engine.traj, want[0]) and torch.equal(bp.seed_status, want[1]) and torch.equal(bp.seed_margin, want[2])
        bp.init(starts, goals, m["boundaries"], initializer=ini)
        assert torch.equal(bp.engine.traj, want[0]) and torch.equal(bp.seed_margin, want[2])
        with pytest.raises(ValueError):
            bp.init(starts, goals, m["boundaries"], initializer=ini, seed_any_angle=True)
        with pytest.raises(ValueError):
            bp.init(starts, goals, m["boundaries"], seed_any_angle=True)
        # without the flag: today's result
        for initializer in (grid, nfopp.AstarTrajectoryInitializer(_host_checker(m), res, directed, clearance=clearance)):
            bp.init(starts, goals, m["boundaries"], initializer=initializer,
                    seed_clearance=clearance if initializer is grid else None)
            assert torch.equal(bp.engine.traj, plain[0]) and torch.equal(bp.seed_status, plain[1])
        off = nfopp.grid_search_init(grid, _dev(starts), _dev(goals), N, directed, clearance=() if clearance is None else clearance,
                                     any_angle=False, lookahead=7)
        assert all(torch.equal(a, b) for a, b in zip(off, plain))


def test_device_anchors_are_mutually_visible():
    m, dist2, paths = _map(1)
    grid = _grid(m)
    cells, counts, status, _ = nfopp.grid_search_paths(grid, _dev(m["starts"]), _dev(m["goals"]))
    points, point_counts, anchors, anchor_counts = nfopp.shorten_paths(grid, cells, counts, status)
    assert points.is_cuda and points.dtype == torch.float32 and points.shape == (32, cells.shape[1], 2)
    assert anchors.dtype == I32 and anchors.shape == (32, cells.shape[1]) and point_counts.shape == anchor_counts.shape == (32,)
    cells, counts, anchors, anchor_counts, point_counts, points = [t.cpu().numpy() for t in (cells, counts, anchors, anchor_counts,
                                                                                           point_counts, points)]
    assert (status.cpu().numpy() == 0).all() and (anchor_counts < counts).all() and (point_counts <= counts).all()
    for i in range(32):
        a = anchors[i, :anchor_counts[i]]
        assert a[0] == 0 and a[-1] == counts[i] - 1 and (np.diff(a) > 0).all(), i
        for k0, k1 in zip(a[:-1], a[1:]):
            assert aar.sees(dist2, 0, cells[i, k0], cells[i, k1]) and aar.sees(dist2, 0, cells[i, k1], cells[i, k0]), (i, k0, k1)
        assert not anchors[i, anchor_counts[i]:].any() and not points[i, point_counts[i]:].any()       # zero behind the counts
        want_a, want_p = aar.shorten(dist2, 0, paths[i], 256, m["boundaries"], m["resolution"])
        assert np.array_equal(a, want_a) and points[i, :point_counts[i]].tobytes() == want_p.tobytes(), i
    again = nfopp.shorten_paths(grid, _dev(cells, I32), _dev(counts, I32), status, lookahead=8)
    for i in range(32):
        want_a = aar.anchors(dist2, 0, paths[i], 8)
        assert np.array_equal(again[2][i, :len(want_a)].cpu().numpy(), want_a) and int(again[3][i]) == len(want_a), i
