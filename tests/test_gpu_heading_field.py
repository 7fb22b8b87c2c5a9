"""GPU: the heading-layered distance field (csrc/heading_field.hip, nfopp/heading_field.py) against its float32 restatement
(tests/heading_field_ref.py), bit for bit throughout: no transcendental is taken, so there is no tolerance in this file.  The
stacked image, the row at explicit poses, trajectory mode against the disc field's draws and the oracle's samples, the engine
and the batch planner on a layered field, the Python layer, and a box planned through a wall's gap."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import guarded as gd  # noqa: E402
import heading_field_cases as hc  # noqa: E402
import heading_field_ref as ref  # noqa: E402
import nfopp  # noqa: E402
import obstacle_map_ref as omr  # noqa: E402
from nfopp import _grid, _lib  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402

F32 = np.float32
DEV = "cuda"
FILLS = (0x00, 0xFF)


def _field(layers, margin=0.05, gain=10.0, border=False):
    return nfopp.HeadingDistanceField(layers.occupancy, layers.boundaries, layers.resolution, margin=margin, gain=gain,
                                      border=border, device=DEV)


@functools.lru_cache(maxsize=None)
def _device_field(name):
    return _field(hc.FIELD_LAYERS[name])


@functools.lru_cache(maxsize=None)
def _ref_field(name):
    return hc.field_of(hc.FIELD_LAYERS[name])


def _same_bits(got, want):
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ---- the image -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hc.FIELD_LAYERS))
@pytest.mark.parametrize("border", [False, True])
def test_stacked_image_bits(name, border):
    lay = hc.FIELD_LAYERS[name]
    field = _field(lay, border=border)
    assert field.field.dtype == torch.float32 and tuple(field.field.shape) == lay.occupancy.shape and field.field.is_contiguous()
    assert np.array_equal(gd.bits(field.field), ref.signed_distance_stack(lay.occupancy, lay.resolution, border).view(np.uint32))
    c = field.config_c()
    want = hc.field_of(lay, border=border)
    assert (c.layers, c.rows, c.cols) == lay.occupancy.shape and c.sd_dev == field.field.data_ptr()
    for got, exp in ((c.x0, want.x0), (c.y0, want.y0), (c.inv_res, want.inv_res), (c.layers_per_rad, want.layers_per_rad),
                     (c.margin, want.margin), (c.gain, want.gain)):
        assert F32(got) == exp
    # a device tensor of slices gives the same image
    again = nfopp.HeadingDistanceField(torch.tensor(lay.occupancy, device=DEV), lay.boundaries, lay.resolution, border=border)
    assert np.array_equal(gd.bits(again.field), gd.bits(field.field))


# ---- explicit poses ----------------------------------------------------------------------------------------------------------------
def _eval_guarded(field, poses, fill):
    """nfopp_hdf_eval_points with out4 inside guard bytes -> the [P, 4] result (numpy)."""
    pts, pts_parent = gd.from_array(poses, DEV)
    snap = gd.snapshot(pts_parent)
    out, parent = gd.guarded((len(poses), 4), torch.float32, DEV, fill)
    _lib.check(_lib.load().nfopp_hdf_eval_points(field.config_c(), _lib.ptr(pts), len(poses), _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert gd.guards_intact(parent) and gd.unchanged(pts_parent, snap)
    return out.cpu().numpy()


@pytest.mark.parametrize("count", hc.POINT_COUNTS)
def test_point_counts_bits(count):
    lay = hc.FIELD_LAYERS[hc.EXACT_FRAME]
    poses = hc.point_poses(lay, count)
    want, _ = ref.eval_points(_ref_field(hc.EXACT_FRAME), poses, F32)
    for fill in FILLS:
        _same_bits(_eval_guarded(_device_field(hc.EXACT_FRAME), poses, fill), want)


def test_edge_poses():
    """On nodes, exactly on the first and last node, outside on every side and corner, and not finite in each component."""
    lay = hc.FIELD_LAYERS[hc.EXACT_FRAME]
    poses, out_x, out_y, bad = hc.edge_poses(lay)
    want, _ = ref.eval_points(_ref_field(hc.EXACT_FRAME), poses, F32)
    for fill in FILLS:
        got = _eval_guarded(_device_field(hc.EXACT_FRAME), poses, fill)
        _same_bits(got, want)
        assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
        assert (got[out_x, 1] == 0).all() and (got[out_y, 2] == 0).all()
    assert (want[~bad & ~out_x, 1] != 0).any() and (want[~bad & ~out_y, 2] != 0).any() and (want[~bad, 3] != 0).any()


@pytest.mark.parametrize("name", sorted(hc.FIELD_LAYERS))
def test_heading_list_bits(name):
    """Zeros, half turns, huge arguments, the largest float, denormals, and every slice heading with both float32 neighbours,
    at L = 2, 3, 16, 64."""
    lay = hc.FIELD_LAYERS[name]
    poses = hc.heading_poses(lay)
    want, choice = ref.eval_points(_ref_field(name), poses, F32)
    got = _eval_guarded(_device_field(name), poses, 0xFF)
    _same_bits(got, want)
    assert np.isfinite(got[choice[:, 6] == 0]).all()


@pytest.mark.parametrize("name", ["3x2x9", "16x37x53"])
def test_random_poses_bits_and_repeatability(name):
    lay = hc.FIELD_LAYERS[name]
    poses = hc.random_poses(lay, 4096, 31)
    want, _ = ref.eval_points(_ref_field(name), poses, F32)
    first = _device_field(name).eval(poses).cpu().numpy()
    _same_bits(first, want)
    _same_bits(_device_field(name).eval(torch.tensor(poses, device=DEV)).cpu().numpy(), first)      # a second run: the same bits


# ---- trajectory mode -----------------------------------------------------------------------------------------------------------------
def _traj_eval(field, traj, t, t_mode, seed, offset, index_offset, fill, active=None):
    """nfopp_traj_hdf_collision_eval with t and out4 inside guard bytes -> (t, out4) as numpy."""
    B, N = traj.shape[:2]
    tr, tr_parent = gd.from_array(traj, DEV)
    snap = gd.snapshot(tr_parent)
    if t is None:
        t_dev, t_parent = gd.guarded((B, N - 1), torch.float32, DEV, fill)
    else:
        t_dev, t_parent = gd.from_array(t, DEV)
    out, out_parent = gd.guarded((B, N - 1, 4), torch.float32, DEV, fill)
    _lib.check(_lib.load().nfopp_traj_hdf_collision_eval(field.config_c(), _lib.ptr(tr), B, N, _lib.ptr(t_dev), t_mode, seed, offset,
                                                         index_offset, _lib.ptr(out), _lib.ptr(active, torch.uint8),
                                                         _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert gd.guards_intact(t_parent) and gd.guards_intact(out_parent) and gd.unchanged(tr_parent, snap)
    return t_dev.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("B,N", hc.TRAJ_SHAPES)
def test_trajectory_mode(B, N):
    name = "16x37x53"
    lay, field = hc.FIELD_LAYERS[name], _device_field(name)
    traj = hc.random_trajectories(lay, B, N)
    seed, offset, index_offset = 1234, 5, 7
    # the draws of the disc field's entry for the same seed, offset and traj_index_offset
    discs = nfopp.DistanceField(nfopp.OccupancyGrid(lay.occupancy[0], lay.boundaries, lay.resolution, device=DEV), radius=0.1)
    t_sdf = torch.zeros(B, N - 1, device=DEV)
    out_sdf = torch.zeros(B, N - 1, 4, device=DEV)
    _lib.check(_lib.load().nfopp_traj_sdf_collision_eval(discs.config_c(), _lib.ptr(torch.tensor(traj, device=DEV)), B, N, 3,
                                                         _lib.ptr(t_sdf), 1, seed, offset, index_offset, _lib.ptr(out_sdf), None,
                                                         _lib.stream_ptr()))
    for fill in FILLS:
        t, out = _traj_eval(field, traj, None, 1, seed, offset, index_offset, fill)
        assert np.array_equal(t.view(np.uint32), gd.bits(t_sdf))
        pts = orc.sample_collision_points(traj, t)
        want = field.eval(pts.reshape(-1, 3)).cpu().numpy().reshape(B, N - 1, 4)
        _same_bits(out, want)
        _same_bits(out, ref.eval_points(_ref_field(name), pts.reshape(-1, 3), F32)[0].reshape(B, N - 1, 4))
        # t_mode 0 reads the same draws, gives the same rows and leaves t alone
        t0, out0 = _traj_eval(field, traj, t, 0, 99, 98, 97, fill)
        _same_bits(t0, t)
        _same_bits(out0, out)
        # with a mask: retired rows keep their bytes, live rows are those of the unmasked launch
        active = torch.tensor(np.arange(B) % 2 == 0, device=DEV).to(torch.uint8)
        tm, outm = _traj_eval(field, traj, None, 1, seed, offset, index_offset, fill, active)
        live = active.cpu().numpy() != 0
        _same_bits(tm[live], t[live])
        _same_bits(outm[live], out[live])
        assert (tm[~live].view(np.uint8) == fill).all() and (outm[~live].view(np.uint8) == fill).all()


# ---- engine and planner ----------------------------------------------------------------------------------------------------------------
def _planner(field, B, N, freq=3, seed=5):
    b = field.boundaries
    rng = np.random.default_rng(11)
    ends = [np.stack([rng.uniform(b[0] + 0.3, b[1] - 0.3, B), rng.uniform(b[2] + 0.3, b[3] - 0.3, B), rng.uniform(-3, 3, B)], 1)
            .astype(F32) for _ in range(2)]
    hp = nfopp.TrajectoryHyper(collision_weight=5, collision_beta=2, direction_delta_weight=1, bounds=b)
    p = nfopp.BatchPlanner(field, B, N, hp, device=DEV, seed=seed, reparametrize_trajectory_freq=freq)
    p.init(ends[0], ends[1], b)
    return p


def _state(p):
    e = p.engine
    torch.cuda.synchronize()
    bufs = [e.traj, e.lam, e.cm, e.adam_m, e.adam_v, e.terms, e.t, e.onf_out]
    return [x.cpu().numpy().copy() for x in bufs] + [e.adam_step, e.rng_offset, p.step_count]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint32) if isinstance(x, np.ndarray) else x,
                              np.asarray(y).view(np.uint32) if isinstance(y, np.ndarray) else y)


def test_engine_step_is_collision_entry_then_update():
    field = _device_field("16x37x53")
    p = _planner(field, 3, 20)
    e = p.engine
    lib, P = _lib.load(), _lib.ptr
    # the same step by hand on copies of the state
    c = {k: getattr(e, k).clone() for k in ("traj", "lam", "cm", "adam_m", "adam_v", "t", "onf_out", "terms")}
    _lib.check(lib.nfopp_traj_hdf_collision_eval(field.config_c(), P(c["traj"]), e.B, e.N, P(c["t"]), 1, e.seed, e.rng_offset,
                                                 e.traj_index_offset, P(c["onf_out"]), None, _lib.stream_ptr()))
    _lib.check(lib.nfopp_traj_update(e.hyper.to_c(e.adam_step + 1), e.B, e.N, e.D, P(c["traj"]), P(e.start), P(e.goal), P(c["lam"]),
                                     P(c["cm"]), P(c["adam_m"]), P(c["adam_v"]), P(c["t"]), P(c["onf_out"]), P(e.hinv_band),
                                     e.half_width, e.interior[0], e.interior[1], P(c["terms"]), None, _lib.stream_ptr()))
    seed = e.traj.clone()
    e.optimize_trajectory(want_terms=True)
    torch.cuda.synchronize()
    for k, v in c.items():
        assert np.array_equal(gd.bits(v), gd.bits(getattr(e, k))), k
    assert not torch.equal(e.traj, seed) and bool(torch.isfinite(e.onf_out).all())


@pytest.mark.parametrize("injected", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_step_n_equals_n_steps(injected, masked):
    B, N, n = 4, 33, 7
    one, many = (_planner(_device_field("16x37x53"), B, N, freq=3) for _ in range(2))
    if masked:
        for p in (one, many):
            p.engine.active = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device=DEV)
    t = np.random.default_rng(2).uniform(0, 1, (n, B, N - 1)).astype(F32) if injected else None
    seed = many.engine.traj.clone()
    for k in range(n):
        one.step(None if t is None else t[k], want_terms=True)
    many.step(t, want_terms=True, n=n)
    a, b = _state(one), _state(many)
    if injected:      # the single steps copy the draws into the engine's t; step(n) reads them where they are
        a.pop(6), b.pop(6)
    _same(a, b)
    assert one.step_count == n and np.isfinite(many.get_paths()).all()
    moved = [not torch.equal(many.engine.traj[b], seed[b]) for b in range(B)]
    assert moved == [True, not masked, True, True]      # a retired row never moves


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_update_keeps_the_buffer_and_gives_a_fresh_fields_bits():
    lay = hc.FIELD_LAYERS["16x37x53"]
    other = hc.make_layers(hc.random_layers(16, 37, 53, 9), (-1.3, 0.7), 0.1)
    field = _field(lay)
    ptr, before = field.field.data_ptr(), field.field.clone()
    field.update(other.occupancy)
    fresh = _field(other)
    assert field.field.data_ptr() == ptr and field.config_c().sd_dev == ptr
    assert np.array_equal(gd.bits(field.field), gd.bits(fresh.field)) and not torch.equal(field.field, before)
    poses = hc.random_poses(other, 300, 12)
    assert np.array_equal(gd.bits(field.eval(poses)), gd.bits(fresh.eval(poses)))
    _same_bits(field.eval(poses).cpu().numpy(), ref.eval_points(hc.field_of(other), poses, F32)[0])
    field.update(torch.tensor(lay.occupancy, device=DEV))
    assert field.field.data_ptr() == ptr and torch.equal(field.field, before)
    with pytest.raises(ValueError):
        field.update(hc.FIELD_LAYERS["3x2x9"].occupancy)


@functools.lru_cache(maxsize=None)
def _hand():
    g, layers = hc.hand_case()
    points = omr.grid_points(g.occupancy.astype(F32), g.resolution, (0.0, 0.0, 0.0))
    return g, layers, nfopp.DeviceRectangleChecker(points, hc.HAND_BOX, g.boundaries, device=DEV)


def test_from_checker_is_the_constructor_on_the_checkers_own_labels():
    """A consistency check on the device's own labels (not against numpy: the checker takes a sine per pose)."""
    g, _, checker = _hand()
    field = nfopp.HeadingDistanceField.from_checker(checker, g.resolution, layers=hc.HAND_LAYERS, margin=0.0, gain=10.0)
    x, y, x_cells, y_cells = _grid.cell_centres(g.boundaries, g.resolution)
    poses = torch.tensor(_grid.heading_poses(x, y, hc.HAND_LAYERS), device=DEV)
    assert np.array_equal(poses[:, 2].reshape(hc.HAND_LAYERS, -1)[:, 0].cpu().numpy().view(np.uint32),
                          ref.slice_headings(hc.HAND_LAYERS).view(np.uint32))
    occ = (checker.labels(poses) > 0).to(torch.uint8).reshape(hc.HAND_LAYERS, y_cells, x_cells)
    direct = nfopp.HeadingDistanceField(occ, g.boundaries, g.resolution, margin=0.0, gain=10.0)
    assert tuple(field.field.shape) == (hc.HAND_LAYERS, 40, 40) and field.boundaries == tuple(g.boundaries)
    assert np.array_equal(gd.bits(field.field), gd.bits(direct.field))
    assert 0 < int(occ.sum()) < occ.numel()
    # update_from_checker: the same image again, in the same buffer
    ptr = field.field.data_ptr()
    field.field.zero_()
    field.update_from_checker(checker)
    assert field.field.data_ptr() == ptr and np.array_equal(gd.bits(field.field), gd.bits(direct.field))


def test_from_lattice():
    g, _, checker = _hand()
    lgrid = nfopp.LatticeGrid.from_checker(checker, g.resolution)
    field = nfopp.HeadingDistanceField.from_lattice(lgrid, margin=0.02)
    direct = nfopp.HeadingDistanceField.from_checker(checker, g.resolution, layers=8, margin=0.02)
    assert field.n_layers == 8 and field.margin == 0.02
    assert np.array_equal(gd.bits(field.field), gd.bits(direct.field))
    with pytest.raises(ValueError):
        nfopp.HeadingDistanceField.from_lattice(nfopp.LatticeGrid(g.occupancy[None], g.boundaries, g.resolution, device=DEV))


def test_hand_case_through_the_python_interface():
    g, layers, checker = _hand()
    poses = np.asarray((hc.HAND_FREE,) + hc.HAND_BLOCKED + (hc.HAND_BETWEEN,), F32)
    field = _field(layers, margin=0.0, gain=10.0)
    got = field.eval(poses).cpu().numpy()
    _same_bits(got, ref.eval_points(hc.field_of(layers, margin=0.0, gain=10.0), poses, F32)[0])
    hit = checker.labels(torch.tensor(poses, device=DEV)).cpu().numpy() > 0
    assert hit.tolist() == [False, True, True, False]
    assert got[0, 0] < 0 and (got[1:3, 0] > 0).all()
    assert got[3, 0] > 0          # the model's limit between two slices
    # the disc cover calls the free pose colliding
    grid = nfopp.OccupancyGrid(g.occupancy, g.boundaries, g.resolution, device=DEV)
    discs = nfopp.DistanceField(grid, discs=nfopp.DistanceField.discs_for_box(hc.HAND_BOX, 4), margin=0.0, gain=10.0)
    assert float(discs.eval(poses[:1])[0, 0]) > 0
    # the same through from_checker: slices from the device's own labels
    made = nfopp.HeadingDistanceField.from_checker(checker, g.resolution, layers=hc.HAND_LAYERS, margin=0.0, gain=10.0)
    logit = made.eval(poses).cpu().numpy()[:, 0]
    assert logit[0] < 0 and (logit[1:3] > 0).all()


def test_planner_and_engine_refusals():
    lay = hc.FIELD_LAYERS["16x37x53"]
    field = _device_field("16x37x53")
    hp = nfopp.TrajectoryHyper(bounds=lay.boundaries)
    checker = nfopp.DeviceGridChecker(lay.occupancy[0], lay.boundaries[0], lay.boundaries[2], lay.resolution, device=DEV)
    with pytest.raises(ValueError):
        nfopp.BatchPlanner(field, 2, 8, hp, device=DEV, checker=checker)
    with pytest.raises(ValueError):
        nfopp.TrajectoryEngine(field, 2, 8, 2, hp, 0.5, DEV)
    with pytest.raises(ValueError):
        field.eval(np.zeros((4, 2), F32))
    # freeze_field does not apply: both values construct, and nothing is frozen
    for freeze in (True, False):
        nfopp.BatchPlanner(field, 2, 8, hp, device=DEV, freeze_field=freeze)


def test_rejected_arguments_leave_the_outputs_untouched():
    lay = hc.FIELD_LAYERS["16x37x53"]
    good = _device_field("16x37x53")
    lib, P = _lib.load(), _lib.ptr
    B, N = 2, 6
    traj = torch.tensor(hc.random_trajectories(lay, B, N), device=DEV)
    pts = torch.tensor(hc.random_poses(lay, 8, 1), device=DEV)
    st = _lib.stream_ptr()

    def field(**changes):
        f = _lib.HeadingFieldC.from_buffer_copy(good.config_c())
        for key, value in changes.items():
            setattr(f, key, value)
        return f

    def fresh():
        t, tp = gd.guarded((B, N - 1), torch.float32, DEV, 0x5A)
        out, op = gd.guarded((max(B * (N - 1), 8), 4), torch.float32, DEV, 0x5A)
        return t, out, (tp, op)

    def untouched(parents):
        torch.cuda.synchronize()
        for parent in parents:
            off, n = gd.span(parent)
            assert gd.guards_intact(parent) and bool((parent[off:off + n] == 0x5A).all())

    bad = [field(layers=1), field(layers=65), field(rows=1), field(cols=1), field(sd_dev=None), field(rows=2 ** 20, cols=2 ** 20)]
    bad += [field(**{name: np.nan}) for name in ("x0", "y0", "inv_res", "layers_per_rad", "margin", "gain")]
    for f in bad:
        t, out, parents = fresh()
        assert lib.nfopp_hdf_eval_points(f, P(pts), 8, P(out), st) == -1 and lib.nfopp_last_error()
        assert lib.nfopp_traj_hdf_collision_eval(f, P(traj), B, N, P(t), 1, 0, 0, 0, P(out), None, st) == -1
        untouched(parents)
    t, out, parents = fresh()
    ok = good.config_c()
    assert lib.nfopp_hdf_eval_points(None, P(pts), 8, P(out), st) == -1
    assert lib.nfopp_hdf_eval_points(ok, None, 8, P(out), st) == -1
    assert lib.nfopp_hdf_eval_points(ok, P(pts), 8, None, st) == -1
    assert lib.nfopp_hdf_eval_points(ok, P(pts), 8, P(out) + 4, st) == -1
    for t_mode in (-1, 2):
        assert lib.nfopp_traj_hdf_collision_eval(ok, P(traj), B, N, P(t), t_mode, 0, 0, 0, P(out), None, st) == -1
    assert lib.nfopp_traj_hdf_collision_eval(ok, None, B, N, P(t), 1, 0, 0, 0, P(out), None, st) == -1
    assert lib.nfopp_traj_hdf_collision_eval(ok, P(traj), B, N, None, 1, 0, 0, 0, P(out), None, st) == -1
    assert lib.nfopp_traj_hdf_collision_eval(ok, P(traj), B, N, P(t), 1, 0, 0, 0, None, None, st) == -1
    assert lib.nfopp_traj_hdf_collision_eval(ok, P(traj), B, 1, P(t), 1, 0, 0, 0, P(out), None, st) == -1
    untouched(parents)
    # the step loop: a bad field or schedule is refused before the first launch
    p = _planner(good, B, N)
    e = p.engine
    before = _state(p)

    def buffers(dim=3):
        return _lib.TrajBuffersC(P(e.traj), P(e.start), P(e.goal), P(e.lam), P(e.cm), P(e.adam_m), P(e.adam_v), P(e.t), P(e.onf_out),
                                 P(e.hinv_band), P(e.u), None, None, e.B, e.N, dim, e.half_width, e.interior[0], e.interior[1])

    hp = e.hyper.to_c(1)

    def sched(t_mode=1, freq=3):
        return _lib.StepScheduleC(1e-2, 0.9, 0.9, 0, 0, 0, 0, 0, freq, t_mode)

    buf = buffers()
    assert lib.nfopp_traj_steps_hdf(field(layers=1), hp, buf, sched(), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_hdf(field(rows=1), hp, buf, sched(), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_hdf(field(gain=np.inf), hp, buf, sched(), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_hdf(ok, hp, buffers(dim=2), sched(), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_hdf(ok, hp, buf, sched(t_mode=2), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_hdf(ok, hp, buf, sched(t_mode=0), 2, None, None, st) == -1     # injected draws without draws
    assert lib.nfopp_traj_steps_hdf(ok, hp, buf, sched(freq=0), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_hdf(None, hp, buf, sched(), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_hdf(ok, None, buf, sched(), 2, None, None, st) == -1
    _same(before, _state(p))
    # and the Python layer refuses what the C layer would
    with pytest.raises(ValueError):
        nfopp.HeadingDistanceField(lay.occupancy[:1], lay.boundaries, lay.resolution)
    with pytest.raises(ValueError):
        nfopp.HeadingDistanceField(lay.occupancy, lay.boundaries, lay.resolution, gain=float("nan"))


# ---- behaviour -----------------------------------------------------------------------------------------------------------------------
def test_plans_a_box_through_the_gap():
    """Straight seeds that cross a wall beside its gap: in collision before, free after BEHAVIOUR_STEPS steps by the rectangle
    checker the model's slices restate.  The restated pipeline (tests/test_heading_field_cpu.py) is free from step
    BEHAVIOUR_FIRST_PASS on with the same injected draws."""
    case = hc.behaviour_case()
    g, lay = case["grid"], case["layers"]
    field = _field(lay, margin=case["margin"], gain=case["gain"])
    hp = gc.hyper_from(orc.Hyper(**case["hyper"]))
    B, N = len(case["starts"]), case["n_waypoints"]
    p = nfopp.BatchPlanner(field, B, N, hp, device=DEV, reparametrize_trajectory_freq=case["reparam_freq"])
    p.init(case["starts"], case["goals"], g.boundaries, trajectories=nfopp.straight_line_init(case["starts"], case["goals"], N))
    checker = nfopp.DeviceRectangleChecker(case["points"], case["box"], g.boundaries, device=DEV)
    collides, _ = p.evaluate(checker)
    assert collides.cpu().numpy().all()
    p.step(case["draws"], n=hc.BEHAVIOUR_STEPS)
    collides, length = p.evaluate(checker)
    assert not collides.cpu().numpy().any()
    assert np.isfinite(length.cpu().numpy()).all()
