"""GPU tests of the obstacle update (csrc/obstacle_map.hip, the indexed rectangle checker of csrc/sampling.hip,
nfopp.DeviceGridMap and the checkers' update interface) against the reference's GridMap and checkers
(tests/golden/g21_obstacle_map.npz) and the numpy restatement in tests/obstacle_map_ref.py.  Everything is compared
exactly: point clouds and indices bit for bit, labels without exception."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
import obstacle_map_ref as omr  # noqa: E402
from nfopp import _lib  # noqa: E402

F32 = np.float32
MAPS = "abcde"
CHECKERS = (("circle", 0.3), ("recta", (-0.34, 0.4, -0.27, 0.27)), ("rectb", (0.1, 0.5, -0.2, 0.2)))
# internal boundaries of the compaction (csrc/obstacle_map.hip): a workgroup counts a chunk of GP_CHUNK = 2048 cells, one
# pass of the scan takes GP_SCAN_PASS = 256 chunk counts
GP_CHUNK, GP_SCAN_PASS = 2048, 256
# ... and of the index build: a wave sorts a segment of 512 points, a workgroup four of them
IX_WORKGROUP_SHARE = 2048


@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_obstacle_map.npz")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def device_map(g21, m):
    return nfopp.DeviceGridMap(g21[m + "_data"], float(g21[m + "_resolution"]), tuple(g21[m + "_origin"]))


def make_checker(name, shape, points, boundaries=None):
    if name == "circle":
        return nfopp.DeviceCircleChecker(points, shape, boundaries)
    return nfopp.DeviceRectangleChecker(points, shape, boundaries)


# ---- point clouds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MAPS)
def test_point_cloud_equals_the_reference_bit_for_bit(g21, m):
    grid = device_map(g21, m)
    ref = g21[m + "_cloud"]
    p32, p64 = grid.as_point_cloud(), grid.as_point_cloud(torch.float64)
    assert p32.is_cuda and p32.dtype == torch.float32 and tuple(p32.shape) == ref.shape
    assert np.array_equal(bits(p64.cpu().numpy()), bits(ref))
    assert np.array_equal(bits(p32.cpu().numpy()), bits(ref.astype(F32)))
    assert grid.as_point_cloud() is p32                                  # cached, as in the reference
    assert grid.boundaries == tuple(g21[m + "_bounds"])
    if m == "c":    # the raw ROS message: data, width, height
        data = g21["c_data"]
        ros = nfopp.DeviceGridMap.from_occupancy_data(data.reshape(-1), data.shape[1], data.shape[0],
                                                      float(g21["c_resolution"]), tuple(g21["c_origin"]))
        assert np.array_equal(bits(ros.as_point_cloud(torch.float64).cpu().numpy()), bits(ref))
        assert ros.boundaries == tuple(g21["c_bounds"])


COMPACTION_SHAPES = {
    "one_cell_more_than_a_chunk": (3, 683),                 # 2049 cells: GP_CHUNK + 1
    "exactly_one_chunk": (32, 64),                          # 2048 cells
    "more_chunks_than_one_scan_pass": (725, 725),           # 525625 cells: 257 chunks > GP_SCAN_PASS
    "chunk_counts_end_inside_the_third_wave": (260, 1024),  # 266240 cells: 130 chunks, one per thread of the scan
}


@pytest.mark.parametrize("shape_name", sorted(COMPACTION_SHAPES))
@pytest.mark.parametrize("fill", ["random", "last_cell_only"])
def test_point_cloud_across_compaction_boundaries(shape_name, fill):
    rows, cols = COMPACTION_SHAPES[shape_name]
    cells = rows * cols
    assert {"one_cell_more_than_a_chunk": cells == GP_CHUNK + 1, "exactly_one_chunk": cells == GP_CHUNK,
            "more_chunks_than_one_scan_pass": -(-cells // GP_CHUNK) > GP_SCAN_PASS,
            "chunk_counts_end_inside_the_third_wave": 128 < -(-cells // GP_CHUNK) <= 192}[shape_name]
    rng = np.random.default_rng(cells)
    if fill == "random":
        data = rng.uniform(0, 0.72, (rows, cols)).astype(F32)
        data[-1, -1] = 1.0
    else:
        data = np.zeros((rows, cols), F32)
        data[-1, -1] = 1.0
    origin = (0.75, -3.5, 0.3)
    ref = omr.grid_points(data, 0.05, origin)
    grid = nfopp.DeviceGridMap(data, 0.05, origin)
    assert np.array_equal(bits(grid.as_point_cloud(torch.float64).cpu().numpy()), bits(ref))
    assert np.array_equal(bits(grid.as_point_cloud().cpu().numpy()), bits(ref.astype(F32)))
    assert len(ref) == (1 if fill == "last_cell_only" else int((data > F32(0.5)).sum()))
    # the int8 form of the same occupancy
    raw = np.where(data > F32(0.5), 100, rng.choice([-1, 0, 50], data.shape)).astype(np.int8)
    assert np.array_equal(bits(nfopp.DeviceGridMap(raw, 0.05, origin).as_point_cloud(torch.float64).cpu().numpy()), bits(ref))


def test_point_cloud_buffer_smaller_than_the_count():
    """max_points below the count: the count is still the full one and nothing is written past the buffer."""
    rng = np.random.default_rng(4)
    data = (rng.uniform(size=(50, 70)) < 0.4).astype(F32)
    ref = omr.grid_points(data, 0.1, (0.0, 0.0, 0.0))
    grid = torch.tensor(data, device="cuda")
    out = torch.full((12, 2), float("nan"), device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().nfopp_grid_to_points(_lib.ptr(grid), 0, 50, 70, 0.5, 0.1, 0.0, 0.0, 1.0, 0.0, 10, _lib.ptr(out),
                                                None, _lib.ptr(count, torch.int32), _lib.stream_ptr()))
    assert int(count.item()) == len(ref) > 12
    got = out.cpu().numpy()
    assert np.array_equal(bits(got[:10]), bits(ref[:10].astype(F32))) and np.isnan(got[10:]).all()


# ---- cell index -----------------------------------------------------------------------------------------------------
def build_index(points, x0, y0, size, nx, ny):
    lib = _lib.load()
    pts = torch.tensor(np.asarray(points, F32).reshape(-1, 2), device="cuda")
    n = pts.shape[0]
    nbytes = lib.nfopp_cell_index_workspace_bytes(n)
    work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    ordered = torch.full((n, 2), float("nan"), device="cuda")
    start = torch.full((nx * ny + 1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.nfopp_build_cell_index(_lib.ptr(pts), n, float(x0), float(y0), float(size), nx, ny, _lib.ptr(ordered),
                                          _lib.ptr(start, torch.int32), _lib.ptr(work, torch.uint8), nbytes,
                                          _lib.stream_ptr()))
    return ordered.cpu().numpy(), start.cpu().numpy()


def index_cases():
    rng = np.random.default_rng(77)
    one_cell = (0.0, 0.0, 1.0, 9, 7)
    cases = {
        "n0": (np.zeros((0, 2), F32), one_cell),
        "n31": (rng.uniform(-1, 10, (31, 2)), one_cell),
        "n32": (rng.uniform(-1, 10, (32, 2)), one_cell),
        "n5000_all_in_one_cell": (rng.uniform(4.01, 4.99, (5000, 2)), one_cell),
        # a 6 x 4 region under points spread over 30 x 30: most are clamped into the border cells
        "outside_the_region": (rng.uniform(-10, 20, (3000, 2)), (2.0, 3.0, 1.0, 6, 4)),
        # above one workgroup's share of 2048 points, and more than 256 cells, so both radix passes carry information
        "above_a_workgroup_share": (rng.uniform(0, 100, (IX_WORKGROUP_SHARE * 3 + 77, 2)), (0.0, 0.0, 0.5, 200, 300)),
        "the_largest_index": (rng.uniform(0, 256, (4097, 2)), (0.0, 0.0, 1.0, 256, 256)),
    }
    pts = rng.uniform(0, 50, (20000, 2)).astype(F32)
    cases["the_checkers_own_geometry"] = (pts, omr.index_geometry(pts, 0.3))
    return cases


@pytest.mark.parametrize("case", sorted(index_cases()))
def test_cell_index_equals_the_numpy_stable_sort(case):
    pts, geom = index_cases()[case]
    pts = np.asarray(pts, F32)
    ref_sorted, ref_start = omr.cell_index(pts, *geom)
    got_sorted, got_start = build_index(pts, *geom)
    assert np.array_equal(got_start, ref_start)
    assert np.array_equal(bits(got_sorted), bits(ref_sorted))
    if case == "n0":
        assert (got_start == 0).all()
    if case == "n5000_all_in_one_cell":
        assert len(np.unique(omr.cell_ids(pts, *geom))) == 1 and np.array_equal(bits(got_sorted), bits(pts))
    if case == "outside_the_region":
        assert (omr.cell_ids(pts, *geom) != omr.cell_ids(np.clip(pts, [2, 3], [7.99, 6.99]), *geom)).sum() == 0
        assert ((pts < [2, 3]) | (pts > [8, 7])).any(1).mean() > 0.8
    again_sorted, again_start = build_index(pts, *geom)                   # identical bytes from run to run
    assert got_sorted.tobytes() == again_sorted.tobytes() and got_start.tobytes() == again_start.tobytes()


def test_checkers_build_their_index_on_the_device():
    """The constructors go through update_obstacle_points: the index equals the numpy one; below INDEX_FROM there is none."""
    rng = np.random.default_rng(9)
    pts = rng.uniform(0, 30, (900, 2))
    for checker, reach in ((nfopp.DeviceCircleChecker(pts, 0.4), 0.4),
                           (nfopp.DeviceRectangleChecker(pts, (0.1, 0.5, -0.2, 0.2)), omr.rectangle_reach((0.1, 0.5, -0.2, 0.2)))):
        x0, y0, size, nx, ny = omr.index_geometry(pts, reach)
        start, gx, gy, cx0, cy0, csize = checker.cells
        assert (gx, gy, F32(cx0), F32(cy0), F32(csize)) == (nx, ny, x0, y0, size)
        ref_sorted, ref_start = omr.cell_index(pts, x0, y0, size, nx, ny)
        assert np.array_equal(start.cpu().numpy(), ref_start)
        assert np.array_equal(bits(checker.obstacles.cpu().numpy()), bits(ref_sorted))
        few = pts[:type(checker).INDEX_FROM - 1]
        checker.update_obstacle_points(torch.tensor(few, device="cuda"))      # a device tensor, float64
        assert checker.cells is None and np.array_equal(checker.obstacles.cpu().numpy(), few.astype(F32))
        checker.update_obstacle_points(np.zeros((0, 2)))
        assert checker.cells is None and checker.obstacles.shape == (0, 2)
        assert checker.labels(torch.zeros(5, 3, device="cuda")).sum().item() == 0


# ---- labels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MAPS)
def test_g21_labels_before_and_after_update_from_map(g21, m):
    grid = device_map(g21, m)
    poses = torch.tensor(g21[m + "_poses"], device="cuda")
    bounds = tuple(g21[m + "_bounds"])
    n_map = len(g21[m + "_cloud"])
    for name, shape in CHECKERS:
        keep = g21["%s_%s_keep" % (m, name)]
        checker = make_checker(name, shape, grid.as_point_cloud())
        assert (checker.cells is not None) == (n_map >= type(checker).INDEX_FROM)
        assert checker.get_boundaries() is None
        before = checker.labels(poses).cpu().numpy().astype(np.uint8)
        assert np.array_equal(before[keep], g21["%s_%s_before" % (m, name)][keep])
        checker.update_from_map(grid, g21[m + "_extra"])
        assert checker.get_boundaries() == bounds and checker.obstacles.shape[0] == n_map + 25
        after = checker.labels(poses).cpu().numpy().astype(np.uint8)
        assert np.array_equal(after[keep], g21["%s_%s_after" % (m, name)][keep])
        assert (before[keep] != after[keep]).any()
        # the brute-force kernel on the same points: every pose, kept or not
        plain = make_checker(name, shape, np.zeros((0, 2)), bounds)
        plain.obstacles = torch.cat([torch.tensor(g21[m + "_extra"].astype(F32), device="cuda"), grid.as_point_cloud()], 0)
        assert plain.cells is None and np.array_equal(plain.labels(poses).cpu().numpy().astype(np.uint8), after)


@pytest.mark.parametrize("box", [(-2.0, 3.0, -1.2, 1.2), (0.5, 4.0, -1.0, 1.5)])
def test_cell_indexed_rectangle_checker_equals_the_plain_one(box):
    """300 points (bench.py's map): the cell-indexed kernel must give the labels of the all-pairs kernel on poses that put
    an obstacle within 1e-4 / 1e-6 of a box edge or a box corner, on map corners and on far-away poses."""
    rng = np.random.default_rng(1234)
    pts = rng.uniform(5, 95, (300, 2))
    bounds = (0.0, 100.0, 0.0, 100.0)
    fast = nfopp.DeviceRectangleChecker(pts, box, bounds)
    assert fast.cells is not None and fast.cells[5] >= omr.rectangle_reach(box)
    slow = nfopp.DeviceRectangleChecker(pts, box, bounds)
    slow.cells = None
    slow.obstacles = torch.tensor(pts.astype(F32), device="cuda")
    rng = np.random.default_rng(7)
    n_rim = 20000
    x0, x1, y0, y1 = box
    eps = rng.choice([-1e-4, 0, 1e-4, -1e-6, 1e-6], n_rim)
    edge = rng.integers(0, 4, n_rim)
    along = rng.uniform(0, 1, n_rim)
    corner = rng.uniform(size=n_rim) < 0.25                   # a quarter of the set sits on the corners
    along = np.where(corner, rng.integers(0, 2, n_rim).astype(float), along)
    rx = np.select([edge == 0, edge == 1], [x0 - eps, x1 + eps], x0 + along * (x1 - x0))
    ry = np.select([edge == 2, edge == 3], [y0 - eps, y1 + eps], y0 + along * (y1 - y0))
    theta = rng.uniform(-np.pi, np.pi, n_rim)
    c, s = np.cos(theta), np.sin(theta)
    target = pts[rng.integers(0, 300, n_rim)]
    rim = np.stack([target[:, 0] - (c * rx - s * ry), target[:, 1] - (s * rx + c * ry), theta], 1)
    n_far = 200000
    far = np.concatenate([rng.uniform(-20, 120, (n_far, 2)), rng.uniform(-np.pi, np.pi, (n_far, 1))], 1)
    poses = np.concatenate([far, rim, [[0, 0, 0.3], [100, 100, -2.0], [-1e6, 3, 1.0], [50, 1e6, 0.0]]]).astype(F32)
    p = torch.tensor(poses, device="cuda")
    a, b = fast.labels(p).cpu().numpy(), slow.labels(p).cpu().numpy()
    assert np.array_equal(a, b), (int((a != b).sum()), poses[a != b][:5])
    assert 0.1 < a.mean() < 0.9
    ref = omr.rectangle_labels(poses.astype(np.float64), pts.astype(F32).astype(np.float64), box, bounds)
    bad = a.astype(bool) != ref
    # float64 at the same fp32 poses: fp32 errs by < 1e-4 m at these coordinates, so only poses that put a point within
    # 1e-4 m of the box's perimeter may differ -- 300 points x perimeter x 2e-4 / (140 m)^2 of the uniform poses
    perimeter = 2 * (x1 - x0 + y1 - y0)
    assert bad[:n_far].mean() <= 300 * perimeter * 2e-4 / 140.0 ** 2 and not bad[-4:].any()


def test_indexed_and_all_pairs_labels_agree_on_unrepresentable_poses():
    """Poses whose cell arithmetic leaves int's range (NaN, +-inf, +-3e9, +-1e30) in x, y or both: the pose's cell comes
    from the float-clamped CellIndex::cell (csrc/point_cloud.h) that sorted the points, so the indexed kernels label them
    like the all-pairs kernels; the finite ones are far from every obstacle and outside the bounds."""
    pts = np.random.default_rng(5).uniform(0, 20, (64, 2))
    values = [np.nan, np.inf, -np.inf, 3e9, -3e9, 1e30, -1e30, 10.0]
    poses = np.array([(x, y, 0.3) for x in values for y in values if not (x == 10.0 and y == 10.0)], F32)
    assert len(poses) == 63
    finite = np.isfinite(poses).all(1)
    p = torch.tensor(poses, device="cuda")
    for name, shape in (("circle", 0.4), ("rect", (0.1, 0.5, -0.2, 0.2))):
        for bounds in (None, (0.0, 20.0, 0.0, 20.0)):
            fast = make_checker(name, shape, pts, bounds)
            assert fast.cells is not None and len(pts) >= type(fast).INDEX_FROM
            slow = make_checker(name, shape, pts, bounds)
            slow.cells, slow.obstacles = None, torch.tensor(pts.astype(F32), device="cuda")
            a, b = fast.labels(p).cpu().numpy(), slow.labels(p).cpu().numpy()
            assert np.array_equal(a, b), (name, bounds, poses[a != b][:5])
            assert np.array_equal(a[finite], np.full(int(finite.sum()), 0.0 if bounds is None else 1.0, F32))


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_batch_planner_follows_a_map_update(g21):
    """Continuous learning, B = 4, N = 32: after update_from_map between two steps the next fit is labelled by the new
    obstacle set -- exactly the labels of a fresh checker built from the new points."""
    torch.random.manual_seed(11)
    onf = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=True).to("cuda")
    box = (-0.34, 0.4, -0.27, 0.27)
    old_map, new_map = device_map(g21, "a"), device_map(g21, "c")
    checker = nfopp.DeviceRectangleChecker(old_map.as_point_cloud(), box, old_map.boundaries)
    B, N = 4, 32
    rng = np.random.default_rng(2)
    lo, hi = np.array([0.4, -2.0]), np.array([6.8, 4.4])
    starts = np.concatenate([rng.uniform(lo, hi, (B, 2)), rng.uniform(-1, 1, (B, 1))], 1).astype(F32)
    goals = np.concatenate([rng.uniform(lo, hi, (B, 2)), rng.uniform(-1, 1, (B, 1))], 1).astype(F32)
    hyper = nfopp.TrajectoryHyper(collision_weight=1, constraint_deltas_weight=20, multipliers_lr=0.1, bounds=old_map.boundaries)
    planner = nfopp.BatchPlanner(onf, B, N, hyper, checker=checker, fit_lr=5e-2, angle_offset=0.3, seed=3)
    planner.init(starts, goals, old_map.boundaries)
    planner.step()
    extra = g21["c_extra"]
    checker.update_from_map(new_map, extra)
    planner.set_boundaries(new_map.boundaries)
    planner.replan(starts=starts, n=1)
    samples = planner.sampler.samples.view(-1, 3)
    used = planner.sampler.labels.cpu().numpy()
    fresh = nfopp.DeviceRectangleChecker(np.concatenate([extra, g21["c_cloud"]], 0), box, new_map.boundaries)
    assert np.array_equal(used, fresh.labels(samples).cpu().numpy())
    stale = nfopp.DeviceRectangleChecker(old_map.as_point_cloud(), box, old_map.boundaries)
    assert not np.array_equal(used, stale.labels(samples).cpu().numpy())
    assert 0.0 < used.mean() < 1.0 and np.isfinite(planner.get_paths()).all()
