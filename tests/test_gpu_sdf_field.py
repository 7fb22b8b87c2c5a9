"""GPU: the distance-field collision model (csrc/sdf_field.hip, nfopp/distance_field.py) against its restatement
(tests/sdf_ref.py): the signed distance image, the row at explicit poses (bit for bit where no sine is taken, within 16 x the
spread of the float32 and float64 restatements where one is), trajectory mode against the ONF entry's draws and the oracle's
samples, the engine and the batch planner on a field, and planning through a wall's gap."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import guarded as gd  # noqa: E402
import nfopp  # noqa: E402
import sdf_cases as sc  # noqa: E402
import sdf_ref as ref  # noqa: E402
from nfopp import _lib  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402

F32 = np.float32
DEV = "cuda"
FILLS = (0x00, 0xFF)


def _grid(g):
    return nfopp.OccupancyGrid(g.occupancy, g.boundaries, g.resolution, device=DEV)


def _field(g, discs, margin=0.05, gain=10.0, dim=3, border=False):
    return nfopp.DistanceField(_grid(g), discs=discs, margin=margin, gain=gain, dim=dim, border=border)


# The spread of the two restatements over each float64 case, per output column: computed here, on the CPU, at import.
SPREAD = {name: ref.spread(sc.field_of(g, discs, margin, gain, border), poses)
          for name, (g, discs, margin, gain, border, poses) in sc.F64_CASES.items()}


# ---- the field -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.FIELD_GRIDS))
@pytest.mark.parametrize("border", [False, True])
def test_signed_distance_field_bits(name, border):
    g = sc.FIELD_GRIDS[name]
    grid = _grid(g)
    got = grid.signed_distance_field(border)
    assert got.dtype == torch.float32 and tuple(got.shape) == g.occupancy.shape
    assert np.array_equal(gd.bits(got), ref.signed_distance(g.occupancy, g.resolution, border).view(np.uint32))
    assert grid.signed_distance_field(border) is got      # cached per border


# ---- explicit points, no trigonometry ----------------------------------------------------------------------------------------------
def _eval_guarded(field, poses, fill):
    """nfopp_sdf_eval_points with out4 inside guard bytes -> the [P, 4] result (numpy)."""
    pts, pts_parent = gd.from_array(poses, DEV)
    snap = gd.snapshot(pts_parent)
    out, parent = gd.guarded((len(poses), 4), torch.float32, DEV, fill)
    _lib.check(_lib.load().nfopp_sdf_eval_points(field.config_c(), _lib.ptr(pts), len(poses), poses.shape[1], _lib.ptr(out),
                                                 _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert gd.guards_intact(parent) and gd.unchanged(pts_parent, snap)
    return out.cpu().numpy()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("count", sc.POINT_COUNTS)
def test_points_without_trigonometry_bits(dim, count):
    g = sc.exact_frame_grid()
    disc = [(0.0, 0.0, 0.2)]
    field = _field(g, disc, dim=dim)
    poses = sc.point_poses(g, count, dim)
    want, _ = ref.eval_points(sc.field_of(g, disc), poses, F32)
    for fill in FILLS:
        got = _eval_guarded(field, poses, fill)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("dim", [2, 3])
def test_edge_poses(dim):
    """On nodes, exactly on the first and last node, outside on every side and corner, and not finite."""
    g = sc.exact_frame_grid()
    disc = [(0.0, 0.0, 0.2)]
    field = _field(g, disc, dim=dim)
    poses, out_x, out_y, bad = sc.edge_poses(g, dim)
    want, _ = ref.eval_points(sc.field_of(g, disc), poses, F32)
    for fill in FILLS:
        got = _eval_guarded(field, poses, fill)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
        assert (got[out_x, 1] == 0).all() and (got[out_y, 2] == 0).all()
        assert (got[~bad, 3] == 0).all()
    # the restatement agrees that something is left to see inside
    assert (want[~bad & ~out_x, 1] != 0).any() and (want[~bad & ~out_y, 2] != 0).any()


# ---- explicit points, several discs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.F64_CASES))
def test_points_with_discs_against_float64(name):
    """The device may differ from the float32 restatement only through sinf / cosf; it is held to 16 x the spread of the two
    restatements (this project's margin, DESIGN.md 8 "Tolerance") per output column, over the poses at which they take the
    same branch."""
    g, discs, margin, gain, border, poses = sc.F64_CASES[name]
    spread, kept = SPREAD[name]
    field = _field(g, discs, margin, gain, border=border)
    got = field.eval(poses).cpu().numpy()
    want, _ = ref.eval_points(sc.field_of(g, discs, margin, gain, border), poses, np.float64)
    dist = np.abs(got.astype(np.float64) - want)[kept].max(0)
    print("%s: SPREAD %s, device distance %s, excluded %d of %d" % (name, spread, dist, (~kept).sum(), len(kept)))
    assert np.isfinite(got).all()
    assert (dist <= 16 * spread).all(), (dist, spread)


def test_tie_takes_the_lower_index():
    g, discs, poses, gain = sc.tie_case()
    for order, sign in ((discs, -1.0), (discs[::-1], 1.0)):
        got = _field(g, order, gain=gain).eval(poses).cpu().numpy()
        want, _ = ref.eval_points(sc.field_of(g, order, gain=gain), poses, F32)
        assert (got[:, 2] == F32(sign * gain)).all()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # heading 0: cos = 1, sin = 0 exactly


# ---- trajectory mode -----------------------------------------------------------------------------------------------------------------
def _onf(dim):
    torch.random.manual_seed(3)
    return nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=dim == 3).to(DEV)


def _traj_eval(field, traj, dim, t, t_mode, seed, offset, index_offset, fill, active=None):
    """nfopp_traj_sdf_collision_eval with t and out4 inside guard bytes -> (t, out4) as numpy."""
    B, N = traj.shape[:2]
    tr, tr_parent = gd.from_array(traj, DEV)
    snap = gd.snapshot(tr_parent)
    if t is None:
        t_dev, t_parent = gd.guarded((B, N - 1), torch.float32, DEV, fill)
    else:
        t_dev, t_parent = gd.from_array(t, DEV)
    out, out_parent = gd.guarded((B, N - 1, 4), torch.float32, DEV, fill)
    _lib.check(_lib.load().nfopp_traj_sdf_collision_eval(field.config_c(), _lib.ptr(tr), B, N, dim, _lib.ptr(t_dev), t_mode, seed,
                                                         offset, index_offset, _lib.ptr(out), _lib.ptr(active, torch.uint8),
                                                         _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert gd.guards_intact(t_parent) and gd.guards_intact(out_parent) and gd.unchanged(tr_parent, snap)
    return t_dev.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("B,N", sc.TRAJ_SHAPES)
def test_trajectory_mode(dim, B, N):
    g = sc.FIELD_GRIDS["37x53"]
    field = _field(g, [(0.0, 0.0, 0.15)] if dim == 2 else sc.THREE_DISCS, dim=dim)
    traj = sc.random_trajectories(g, B, N, dim)
    seed, offset, index_offset = 1234, 5, 7
    # the draws of the ONF entry for the same seed, offset and traj_index_offset
    onf = _onf(dim)
    t_onf = torch.zeros(B, N - 1, device=DEV)
    out_onf = torch.zeros(B, N - 1, 4, device=DEV)
    _lib.check(_lib.load().nfopp_traj_collision_eval(onf.config_c(), _lib.ptr(onf.flat_parameters), _lib.ptr(torch.tensor(traj, device=DEV)),
                                                     B, N, dim, _lib.ptr(t_onf), 1, seed, offset, index_offset, _lib.ptr(out_onf),
                                                     None, None, _lib.stream_ptr()))
    for fill in FILLS:
        t, out = _traj_eval(field, traj, dim, None, 1, seed, offset, index_offset, fill)
        assert np.array_equal(t.view(np.uint32), gd.bits(t_onf))
        pts = (orc.sample_collision_points if dim == 3 else orc.sample_collision_points_2d)(traj, t)
        want = field.eval(pts.reshape(-1, dim)).cpu().numpy().reshape(B, N - 1, 4)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
        # t_mode 0 reads the same draws, gives the same rows and leaves t alone
        t0, out0 = _traj_eval(field, traj, dim, t, 0, 99, 98, 97, fill)
        assert np.array_equal(t0.view(np.uint32), t.view(np.uint32)) and np.array_equal(out0.view(np.uint32), out.view(np.uint32))
        # with a mask: retired rows keep their bytes, live rows are those of the unmasked launch
        active = torch.tensor(np.arange(B) % 2 == 0, device=DEV).to(torch.uint8)
        tm, outm = _traj_eval(field, traj, dim, None, 1, seed, offset, index_offset, fill, active)
        live = active.cpu().numpy() != 0
        assert np.array_equal(tm[live].view(np.uint32), t[live].view(np.uint32))
        assert np.array_equal(outm[live].view(np.uint32), out[live].view(np.uint32))
        assert (tm[~live].view(np.uint8) == fill).all() and (outm[~live].view(np.uint8) == fill).all()


# ---- engine and planner ----------------------------------------------------------------------------------------------------------------
def _planner(field, B, N, dim, freq=3, seed=5):
    g = sc.FIELD_GRIDS["37x53"]
    rng = np.random.default_rng(11)
    b = g.boundaries
    ends = [np.stack([rng.uniform(b[0] + 0.3, b[1] - 0.3, B), rng.uniform(b[2] + 0.3, b[3] - 0.3, B), rng.uniform(-3, 3, B)], 1)
            [:, :dim].astype(F32) for _ in range(2)]
    hp = nfopp.TrajectoryHyper(collision_weight=5, collision_beta=2, direction_delta_weight=1, bounds=b)
    p = nfopp.BatchPlanner(field, B, N, hp, device=DEV, seed=seed, reparametrize_trajectory_freq=freq)
    p.init(ends[0], ends[1], b)
    return p


def _state(p):
    e = p.engine
    torch.cuda.synchronize()
    bufs = [x for x in (e.traj, e.lam, e.cm, e.adam_m, e.adam_v, e.terms, e.t, e.onf_out) if x is not None]
    return [x.cpu().numpy().copy() for x in bufs] + [e.adam_step, e.rng_offset, p.step_count]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint32) if isinstance(x, np.ndarray) else x,
                              np.asarray(y).view(np.uint32) if isinstance(y, np.ndarray) else y)


@pytest.mark.parametrize("dim", [2, 3])
def test_engine_step_is_collision_entry_then_update(dim):
    g = sc.FIELD_GRIDS["37x53"]
    field = _field(g, [(0.0, 0.0, 0.15)] if dim == 2 else sc.THREE_DISCS, dim=dim)
    p = _planner(field, 3, 20, dim)
    e = p.engine
    lib, P = _lib.load(), _lib.ptr
    # the same step by hand on copies of the state
    c = {k: (None if getattr(e, k) is None else getattr(e, k).clone()) for k in ("traj", "lam", "cm", "adam_m", "adam_v", "t", "onf_out", "terms")}
    _lib.check(lib.nfopp_traj_sdf_collision_eval(field.config_c(), P(c["traj"]), e.B, e.N, e.D, P(c["t"]), 1, e.seed, e.rng_offset,
                                                 e.traj_index_offset, P(c["onf_out"]), None, _lib.stream_ptr()))
    _lib.check(lib.nfopp_traj_update(e.hyper.to_c(e.adam_step + 1), e.B, e.N, e.D, P(c["traj"]), P(e.start), P(e.goal), P(c["lam"]),
                                     P(c["cm"]), P(c["adam_m"]), P(c["adam_v"]), P(c["t"]), P(c["onf_out"]), P(e.hinv_band),
                                     e.half_width, e.interior[0], e.interior[1], P(c["terms"]), None, _lib.stream_ptr()))
    seed = e.traj.clone()
    e.optimize_trajectory(want_terms=True)
    torch.cuda.synchronize()
    for k, v in c.items():
        if v is not None:
            assert np.array_equal(gd.bits(v), gd.bits(getattr(e, k))), k
    assert not torch.equal(e.traj, seed) and bool(torch.isfinite(e.onf_out).all())


@pytest.mark.parametrize("injected", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_step_n_equals_n_steps(injected, masked):
    g = sc.FIELD_GRIDS["37x53"]
    B, N, n = 4, 33, 7
    one, many = (_planner(_field(g, sc.THREE_DISCS), B, N, 3, freq=3) for _ in range(2))
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


def test_update_keeps_the_buffer_and_gives_a_fresh_fields_bits():
    g1, g2 = sc.FIELD_GRIDS["37x53"], sc.make_grid(sc.random_blocks(37, 53, 7, 9), (-1.3, 0.7), 0.1)
    field = _field(g1, sc.THREE_DISCS)
    ptr, before = field.field.data_ptr(), field.field.clone()
    field.update(_grid(g2))
    fresh = _field(g2, sc.THREE_DISCS)
    assert field.field.data_ptr() == ptr and field.config_c().sd_dev == ptr
    assert np.array_equal(gd.bits(field.field), gd.bits(fresh.field)) and not torch.equal(field.field, before)
    poses = sc.random_poses(g2, 300, 12)
    assert np.array_equal(gd.bits(field.eval(poses)), gd.bits(fresh.eval(poses)))
    with pytest.raises(ValueError):
        field.update(_grid(sc.FIELD_GRIDS["2x9"]))


def test_planner_refuses_a_checker():
    g = sc.FIELD_GRIDS["37x53"]
    hp = nfopp.TrajectoryHyper(bounds=g.boundaries)
    checker = nfopp.DeviceGridChecker(g.occupancy, g.boundaries[0], g.boundaries[2], g.resolution, device=DEV)
    with pytest.raises(ValueError):
        nfopp.BatchPlanner(_field(g, sc.THREE_DISCS), 2, 8, hp, device=DEV, checker=checker)


# ---- behaviour -----------------------------------------------------------------------------------------------------------------------
def test_plans_through_the_gap():
    """Straight seeds that cross a wall beside its gap: in collision before, free after BEHAVIOUR_STEPS steps.  The restated
    pipeline (tests/test_sdf_field_cpu.py) first passes at step BEHAVIOUR_FIRST_PASS with the same injected draws."""
    case = sc.behaviour_case()
    g = case["grid"]
    field = nfopp.DistanceField(_grid(g), discs=case["discs"], margin=case["margin"], gain=case["gain"])
    hp = gc.hyper_from(orc.Hyper(**case["hyper"]))
    B, N = len(case["starts"]), case["n_waypoints"]
    p = nfopp.BatchPlanner(field, B, N, hp, device=DEV, reparametrize_trajectory_freq=case["reparam_freq"])
    p.init(case["starts"], case["goals"], g.boundaries, trajectories=nfopp.straight_line_init(case["starts"], case["goals"], N))
    checker = nfopp.DeviceGridChecker(g.occupancy, g.boundaries[0], g.boundaries[2], g.resolution, device=DEV)
    collides, _ = p.evaluate(checker)
    assert collides.cpu().numpy().all()
    p.step(case["draws"], n=sc.BEHAVIOUR_STEPS)
    collides, length = p.evaluate(checker)
    assert not collides.cpu().numpy().any()
    assert np.isfinite(length.cpu().numpy()).all()
    stats = p.path_stats(checker)
    assert np.isfinite(stats[:, nfopp.PATH_STAT_LENGTH].cpu().numpy()).all()


def test_seeding_and_replanning_on_a_field():
    """A grid-search seed, steps, a receding-horizon tick and the path statistics with a DistanceField in the ONF's place."""
    case = sc.behaviour_case()
    g = case["grid"]
    grid = _grid(g)
    field = nfopp.DistanceField(grid, discs=case["discs"], margin=case["margin"], gain=case["gain"])
    B, N = len(case["starts"]), case["n_waypoints"]
    p = nfopp.BatchPlanner(field, B, N, gc.hyper_from(orc.Hyper(**case["hyper"])), device=DEV)
    p.init(case["starts"], case["goals"], g.boundaries, initializer=grid)
    assert (p.seed_status.cpu().numpy() == 0).all()
    checker = nfopp.DeviceGridChecker(g.occupancy, g.boundaries[0], g.boundaries[2], g.resolution, device=DEV)
    p.step(n=20)
    moved = case["starts"].copy()
    moved[:, 0] += 0.05
    p.replan(starts=moved, n=10)
    collides, length = p.evaluate(checker)
    assert collides.shape == (B,) and np.isfinite(length.cpu().numpy()).all()
    paths = p.get_paths()
    assert np.array_equal(paths[:, 0], moved) and np.isfinite(paths).all()
    assert np.isfinite(p.path_stats(checker)[:, :5].cpu().numpy()).all()


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_leave_the_outputs_untouched():
    g = sc.FIELD_GRIDS["37x53"]
    good = _field(g, sc.THREE_DISCS)
    lib, P = _lib.load(), _lib.ptr
    B, N = 2, 6
    traj = torch.tensor(sc.random_trajectories(g, B, N, 3), device=DEV)
    pts = torch.tensor(sc.random_poses(g, 8, 1), device=DEV)
    st = _lib.stream_ptr()

    def field(**changes):
        f = _lib.SdfFieldC.from_buffer_copy(good.config_c())
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

    for f, dim in ((field(rows=1), 3), (field(cols=1), 3), (field(n_discs=0), 3), (field(n_discs=9), 3), (field(sd_dev=None), 3),
                   (field(), 2), (field(), 4)):
        t, out, parents = fresh()
        assert lib.nfopp_sdf_eval_points(f, P(pts), 8, dim, P(out), st) == -1 and lib.nfopp_last_error()
        assert lib.nfopp_traj_sdf_collision_eval(f, P(traj), B, N, dim, P(t), 1, 0, 0, 0, P(out), None, st) == -1
        untouched(parents)
    t, out, parents = fresh()
    ok = good.config_c()
    assert lib.nfopp_sdf_eval_points(None, P(pts), 8, 3, P(out), st) == -1
    assert lib.nfopp_sdf_eval_points(ok, None, 8, 3, P(out), st) == -1
    assert lib.nfopp_sdf_eval_points(ok, P(pts), 8, 3, None, st) == -1
    for t_mode in (-1, 2):
        assert lib.nfopp_traj_sdf_collision_eval(ok, P(traj), B, N, 3, P(t), t_mode, 0, 0, 0, P(out), None, st) == -1
    assert lib.nfopp_traj_sdf_collision_eval(ok, None, B, N, 3, P(t), 1, 0, 0, 0, P(out), None, st) == -1
    assert lib.nfopp_traj_sdf_collision_eval(ok, P(traj), B, N, 3, None, 1, 0, 0, 0, P(out), None, st) == -1
    assert lib.nfopp_traj_sdf_collision_eval(ok, P(traj), B, N, 3, P(t), 1, 0, 0, 0, None, None, st) == -1
    untouched(parents)
    # the step loop: a bad field or schedule is refused before the first launch
    p = _planner(good, B, N, 3)
    e = p.engine
    before = _state(p)
    buf = _lib.TrajBuffersC(P(e.traj), P(e.start), P(e.goal), P(e.lam), P(e.cm), P(e.adam_m), P(e.adam_v), P(e.t), P(e.onf_out),
                            P(e.hinv_band), P(e.u), None, None, e.B, e.N, e.D, e.half_width, e.interior[0], e.interior[1])
    hp = e.hyper.to_c(1)

    def sched(t_mode=1, freq=3):
        return _lib.StepScheduleC(1e-2, 0.9, 0.9, 0, 0, 0, 0, 0, freq, t_mode)

    assert lib.nfopp_traj_steps_sdf(field(n_discs=0), hp, buf, sched(), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_sdf(field(rows=1), hp, buf, sched(), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_sdf(ok, hp, buf, sched(t_mode=2), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_sdf(ok, hp, buf, sched(t_mode=0), 2, None, None, st) == -1     # injected draws without draws
    assert lib.nfopp_traj_steps_sdf(ok, hp, buf, sched(freq=0), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_sdf(None, hp, buf, sched(), 2, None, None, st) == -1
    assert lib.nfopp_traj_steps_sdf(ok, None, buf, sched(), 2, None, None, st) == -1
    _same(before, _state(p))
    # and the Python layer refuses what the C layer would
    with pytest.raises(ValueError):
        nfopp.DistanceField(_grid(g), discs=sc.THREE_DISCS, dim=2)
    with pytest.raises(ValueError):
        nfopp.DistanceField(_grid(g), discs=[(0, 0, 0.1)] * 9)
    with pytest.raises(TypeError):
        nfopp.DistanceField(_grid(g))
