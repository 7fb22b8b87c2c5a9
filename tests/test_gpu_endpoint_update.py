"""GPU: the batched start / goal update (nfopp_update_endpoints, csrc/endpoint_update.hip) and what is built on it --
against the reference's fixtures through the C ABI, against the formulation it replaces (torch ops + nfopp_reparametrize,
built here) bit for bit, batch invariance, the `moved` mask, BatchPlanner's update / set_boundaries / replan and the
drop-in planners."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import endpoint_ref as er  # noqa: E402
import nfopp  # noqa: E402
from nfopp import _lib, torch_ops  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402
from test_gpu_planner_api import _make  # noqa: E402

F32 = np.float32
DEV = "cuda"


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _grid(n):
    return torch.linspace(0, 1, n + 2)[1:-1].contiguous().to(DEV)   # CPU linspace: the reference's rounding


def _np(t):
    return None if t is None else t.cpu().numpy().copy()


class State(object):
    """Device copies of a batch's state: traj [B,N,D], start / goal [B,D], lam [B,N+1] / cm [B,N] (None for D = 2)."""

    def __init__(self, traj, start, goal, lam=None, cm=None):
        self.traj, self.start, self.goal, self.lam, self.cm = (_dev(x) for x in (traj, start, goal, lam, cm))
        self.B, self.N, self.D = self.traj.shape
        self.u = _grid(self.N)

    def clone(self):
        return State(*(_np(x) for x in (self.traj, self.start, self.goal, self.lam, self.cm)))

    def row(self, b):
        return State(*(None if x is None else _np(x)[b:b + 1] for x in (self.traj, self.start, self.goal, self.lam, self.cm)))

    def arrays(self):
        torch.cuda.synchronize()
        return {k: _np(getattr(self, k)) for k in ("traj", "start", "goal", "lam", "cm")}


def kernel_update(s, which, points, moved=None):
    """nfopp_update_endpoints on `s` in place; returns min_index [B] (int32, -7 where the kernel wrote nothing)."""
    idx = torch.full((s.B,), -7, dtype=torch.int32, device=DEV)
    P = _lib.ptr
    _lib.check(_lib.load().nfopp_update_endpoints(s.B, s.N, s.D, which, P(points), P(moved, torch.uint8), P(s.traj), P(s.start),
                                                  P(s.goal), P(s.lam), P(s.cm), P(s.u), P(idx, torch.int32), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return idx.cpu().numpy()


def parent_update(s, which, points):
    """What the planners did before the kernel existed (planner.py's update_goal_point / update_start_point: torch ops on the
    device tensors, then nfopp_reparametrize), written for a batch.  Returns min_index [B]."""
    ref = s.goal if which == 1 else s.start
    ref.copy_(points)
    delta = torch.sum((s.traj[:, :, :2] - ref[:, None, :2]) ** 2, dim=2)
    m = torch.argmin(delta, dim=1)
    if s.D == 3:
        m = torch.clamp(m + 1, max=s.N)
    w = torch.arange(s.N, device=DEV)[None, :]
    cut = (w >= m[:, None]) if which == 1 else (w < m[:, None])
    s.traj.copy_(torch.where(cut[:, :, None], ref[:, None, :], s.traj))
    _lib.check(_lib.load().nfopp_reparametrize(s.B, s.N, s.D, _lib.ptr(s.traj), _lib.ptr(s.start), _lib.ptr(s.goal),
                                               _lib.ptr(s.lam), _lib.ptr(s.cm), _lib.ptr(s.u), None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return m.to(torch.int32).cpu().numpy(), delta.cpu().numpy()


def _same_state(a, b, rows=None):
    for k in ("traj", "start", "goal", "lam", "cm"):
        if a[k] is None:
            assert b[k] is None
            continue
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y), k


# ---- the reference's fixtures through the C ABI, B = 1 --------------------------------------------------------------
CASES = er.g20_cases(load_golden("g20_endpoint_updates.npz")) + er.g4_cases(load_golden("g4_update_endpoints.npz"))


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_kernel_reproduces_the_reference(case):
    se2 = case["lam"] is not None
    s = State(case["traj"][None], case["start"][None], case["goal"][None], case["lam"][None] if se2 else None,
              case["cm"][None] if se2 else None)
    idx = kernel_update(s, case["which"], _dev(case["point"][None]))
    a = s.arrays()
    got = dict(traj=a["traj"][0], lam=a["lam"][0] if se2 else None, cm=a["cm"][0] if se2 else None, min_index=idx[0])
    bad, worst = er.mismatch(case, got)
    assert bad is None, bad
    assert np.array_equal(a["goal" if case["which"] else "start"][0], case["point"])
    assert np.array_equal(a["start" if case["which"] else "goal"][0], case["start" if case["which"] else "goal"])


# ---- the formulation it replaces, bit for bit -----------------------------------------------------------------------
_SOURCES = {100: ("traj_n100_hard.npz", None), 256: ("traj_benchmr_n256.npz", None), 512: ("traj_benchmr_n512.npz", None),
            2: ("traj_n100_hard.npz", [30, 60]), 3: ("traj_n100_hard.npz", [25, 50, 75])}
TIE_ROWS, DUP_ROWS, FIRST_ROW, LAST_ROW = (2, 3), (4, 5), 0, 1


def batch_state(n, d, which, B=257, seed=0):
    arrays, pts, i = batch_arrays(n, d, which, B, seed)
    return State(*arrays), pts, i


def batch_arrays(n, d, which, B=257, seed=0):
    """B jittered copies of a committed trajectory state and a new endpoint per row near a random waypoint; row 0 / 1 have
    their nearest waypoint at index 0 / N-1, rows 2-3 an exact fp32 tie between two waypoints mirrored about the diagonal
    through the new point, rows 4-5 a tie between two coincident waypoints."""
    name, pick = _SOURCES[n]
    z = load_golden(name)
    tr, lam, cm = z["g6_k10_traj"], z["g6_k10_lam"], z["g6_k10_cm"]
    if pick is not None:
        tr, cm, lam = tr[pick], cm[pick], lam[pick + [pick[-1] + 1]]
    rng = np.random.default_rng(seed + 17 * n + d)
    span = float(np.abs(tr[-1, :2] - tr[0, :2]).max())
    spacing = span / (n + 1)
    traj = (tr[None] + rng.normal(0, 0.05 * spacing, (B, n, 3))).astype(F32)
    start = (z["g6_k10_start"][None] + rng.normal(0, 0.05 * spacing, (B, 3))).astype(F32)
    goal = (z["g6_k10_goal"][None] + rng.normal(0, 0.05 * spacing, (B, 3))).astype(F32)
    lam = (lam[None] + rng.normal(0, 0.1, (B, n + 1))).astype(F32)
    cm = np.abs(cm[None] + rng.normal(0, 0.05, (B, n))).astype(F32)
    near = rng.integers(0, n, B)
    near[FIRST_ROW], near[LAST_ROW] = 0, n - 1
    pts = traj[np.arange(B), near].copy()
    pts[:, :2] += rng.normal(0, 0.2 * spacing, (B, 2)).astype(F32)
    pts[:, 2] = rng.uniform(-3.1, 3.1, B)
    pts[FIRST_ROW, :2], pts[LAST_ROW, :2] = traj[FIRST_ROW, 0, :2], traj[LAST_ROW, n - 1, :2]
    i = max(0, n // 2 - 1)
    for b in TIE_ROWS:      # p on a 2^-8 grid, offsets a few `spacing_unit`s (a power of two): every sum and difference is exact
        p = (np.round(traj[b, i, :2].astype(np.float64) * 256) / 256).astype(F32)
        k1, k2 = (11, 29) if b == TIE_ROWS[0] else (31, 13)
        a_, b_ = F32(k1 * spacing_unit(spacing)), F32(k2 * spacing_unit(spacing))
        traj[b, i, :2] = p + F32([a_, b_])
        traj[b, i + 1, :2] = p + F32([b_, a_])
        pts[b, :2] = p
    for b in DUP_ROWS:
        traj[b, i + 1] = traj[b, i]
        pts[b, :2] = traj[b, i, :2] + F32(0.01 * spacing)
    if d == 2:
        return (traj[..., :2], start[:, :2], goal[:, :2], None, None), np.ascontiguousarray(pts[:, :2]), i
    return (traj, start, goal, lam, cm), pts, i


def spacing_unit(spacing):
    """The power of two nearest below spacing / 128: tie offsets of 11-31 units stay well inside one waypoint spacing."""
    return 2.0 ** np.floor(np.log2(spacing / 128))


@pytest.mark.parametrize("which", [0, 1], ids=["start", "goal"])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [2, 3, 100, 256, 512])
def test_kernel_equals_the_formulation_it_replaces(n, d, which):
    s, pts, i = batch_state(n, d, which)
    old, new = s.clone(), s.clone()
    want_idx, delta = parent_update(old, which, _dev(pts))
    got_idx = kernel_update(new, which, _dev(pts))
    # the rows built for it do what they were built for
    arg = np.argmin(delta, 1)
    assert arg[FIRST_ROW] == 0 and arg[LAST_ROW] == n - 1
    for b in TIE_ROWS + DUP_ROWS:
        assert delta[b, i] == delta[b, i + 1] == delta[b].min() and arg[b] == i, b
    assert np.array_equal(got_idx, want_idx)
    _same_state(new.arrays(), old.arrays())
    assert np.isfinite(new.arrays()["traj"]).all()


@pytest.mark.parametrize("which", [0, 1], ids=["start", "goal"])
@pytest.mark.parametrize("n,d", [(100, 3), (256, 2), (3, 3), (512, 3)])
def test_batch_invariance(n, d, which):
    s, pts, _ = batch_state(n, d, which, seed=1)
    full = s.clone()
    idx = kernel_update(full, which, _dev(pts))
    fa = full.arrays()
    for b in (0, 1, 2, 4, 100, 256):
        one = s.row(b)
        i1 = kernel_update(one, which, _dev(pts[b:b + 1]))
        oa = one.arrays()
        assert i1[0] == idx[b]
        for k, v in oa.items():
            assert v is None or np.array_equal(v[0], fa[k][b]), (b, k)


# ---- the moved mask -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["start", "goal"])
@pytest.mark.parametrize("d", [2, 3])
def test_moved_mask(d, which):
    s, pts, _ = batch_state(100, d, which, seed=2)
    before = s.arrays()
    allrows = s.clone()
    idx_all = kernel_update(allrows, which, _dev(pts))
    mask = (np.random.default_rng(4).random(s.B) < 0.5).astype(np.uint8)
    mask[:2] = (1, 0)
    part = s.clone()
    idx = kernel_update(part, which, _dev(pts), _dev(mask, torch.uint8))
    pa = part.arrays()
    _same_state(pa, before, rows=mask == 0)                  # unmoved rows: bit for bit as they were, endpoint included
    _same_state(pa, allrows.arrays(), rows=mask == 1)        # moved rows: what the unmasked call gives
    assert np.array_equal(idx[mask == 1], idx_all[mask == 1]) and (idx[mask == 0] == -7).all()
    none = s.clone()
    idx0 = kernel_update(none, which, _dev(pts), _dev(np.zeros(s.B, np.uint8), torch.uint8))
    _same_state(none.arrays(), before)
    assert (idx0 == -7).all()


def _planner(B=6, N=64, freq=10, **kw):
    z = load_golden("traj_n100_hard.npz")
    onf, cfg = gc.make_onf(z["cfg"], z["params"])
    hp = gc.hyper_from(orc.Hyper.from_npz(z))
    rng = np.random.default_rng(11)
    starts = np.concatenate([rng.uniform(0.3, 0.9, (B, 2)), rng.uniform(-3, 3, (B, 1))], 1).astype(F32)
    goals = np.concatenate([rng.uniform(2.1, 2.7, (B, 2)), rng.uniform(-3, 3, (B, 1))], 1).astype(F32)
    p = nfopp.BatchPlanner(onf, B, N, hp, device=DEV, seed=5, reparametrize_trajectory_freq=freq, **kw)
    p.init(starts, goals, hp.bounds)
    return p, starts, goals, hp


def _engine_arrays(p):
    e = p.engine
    torch.cuda.synchronize()
    return {k: _np(getattr(e, k)) for k in ("traj", "start", "goal", "lam", "cm", "adam_m", "adam_v")}


def test_engine_updates_a_moved_row_that_is_retired():
    p, starts, goals, hp = _planner()
    p.step(n=7)
    eng = p.engine
    s = State(*(_np(x) for x in (eng.traj, eng.start, eng.goal, eng.lam, eng.cm)))
    pts = (_np(eng.traj)[:, 20] + F32([0.01, -0.01, 0.2])).astype(F32)
    want_idx = kernel_update(s, 0, _dev(pts))
    eng.active = _dev(np.array([1, 0, 1, 0, 1, 1], np.uint8), torch.uint8)
    idx = torch.zeros(eng.B, dtype=torch.int32, device=DEV)
    eng.update_endpoints("start", pts, min_index_out=idx)     # numpy points: one upload
    got = _engine_arrays(p)
    want = s.arrays()
    for k in ("traj", "start", "goal", "lam", "cm"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(got["start"], pts)


def test_torch_op_equals_the_ctypes_path():
    ops = torch_ops.load()
    for d in (2, 3):
        s, pts, _ = batch_state(100, d, 1, B=9, seed=3)
        a, b = s.clone(), s.clone()
        mask = _dev(np.array([1, 1, 0, 1, 0, 1, 1, 1, 0], np.uint8), torch.uint8)
        want = kernel_update(a, 1, _dev(pts), mask)
        idx = torch.full((9,), -7, dtype=torch.int32, device=DEV)
        ops.update_endpoints(b.traj, b.start, b.goal, b.lam, b.cm, b.u, _dev(pts), 1, mask, idx)
        _same_state(b.arrays(), a.arrays())
        assert np.array_equal(idx.cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="which"):
        ops.update_endpoints(b.traj, b.start, b.goal, b.lam, b.cm, b.u, _dev(pts), 2, None, None)


# ---- BatchPlanner ---------------------------------------------------------------------------------------------------
def test_batch_planner_update_keeps_adam_and_resets_the_rest():
    p, starts, goals, hp = _planner()
    p.step(n=13)
    assert p.step_count == 13
    eng = p.engine
    before = _engine_arrays(p)
    adam_step = eng.adam_step
    eng.active = _dev(np.array([1, 0, 0, 1, 0, 1], np.uint8), torch.uint8)
    p.best_length = _dev(np.array([1, 2, 3, 4, 5, 6], F32))
    p.best_traj = eng.traj.detach().clone().view(eng.B, eng.N, eng.D)
    moved = _dev(np.array([0, 1, 0, 1, 1, 0], np.uint8), torch.uint8)
    pts = (before["traj"][:, 10] + F32([0.01, 0.01, 0.1])).astype(F32)
    p.update_start_points(_dev(pts), moved)
    after = _engine_arrays(p)
    assert p.step_count == 0 and eng.adam_step == adam_step
    assert np.array_equal(after["adam_m"], before["adam_m"]) and np.array_equal(after["adam_v"], before["adam_v"])
    assert np.array_equal(_np(eng.active), [1, 1, 0, 1, 1, 1])              # moved rows re-activated, the others kept
    assert np.array_equal(_np(p.best_length), np.array([1, np.inf, 3, np.inf, np.inf, 6], F32))
    m = _np(moved) == 1
    _same_state(after, before, rows=~m)
    assert np.array_equal(after["start"][m], pts[m]) and not np.array_equal(after["traj"][m], before["traj"][m])
    p.step_count = 5
    gpts = (after["traj"][:, 50] + F32([0.0, 0.02, -0.1])).astype(F32)
    p.update_goal_points(gpts)                                                   # numpy, no mask: all rows
    assert p.step_count == 0 and eng.adam_step == adam_step
    assert np.array_equal(_np(eng.goal), gpts) and (_np(eng.active) == 1).all() and np.isinf(_np(p.best_length)).all()
    assert np.array_equal(_np(eng.adam_m), before["adam_m"])
    assert np.isfinite(p.get_paths()).all()


def test_batch_planner_set_boundaries_reaches_the_kernels():
    p, starts, goals, hp = _planner()
    p.step(n=3, want_terms=True)
    inside = p.engine.loss_terms()["boundary"].copy()           # the box the batch was planned in
    p.set_boundaries((1.4, 1.6, 1.4, 1.6))                      # every trajectory reaches far outside this one
    assert p.step_count == 0 and p.engine.hyper.bounds == (1.4, 1.6, 1.4, 1.6)
    p.step(n=1, want_terms=True)
    assert p.step_count == 1
    outside = p.engine.loss_terms()["boundary"]
    assert (outside > 0).all() and (outside > inside).all()


def _tick_starts(p):
    return p.engine.full_trajectory()[:, 3].contiguous()           # waypoint 3 of each current path, a device tensor


def test_replan_ticks():
    """Ten ticks of the receding-horizon loop on 64 problems (frozen field, device RNG): the path starts where it was
    told to, stays finite, row b is what a one-trajectory planner with traj_index_offset = b computes, and replan is the
    separate calls."""
    B, N, rows = 64, 64, (0, 17, 40, 63)
    big, starts, goals, hp = _planner(B, N)
    split, _, _, _ = _planner(B, N)
    singles = {}
    for b in rows:
        q = nfopp.BatchPlanner(big.onf, 1, N, hp, device=DEV, seed=5, reparametrize_trajectory_freq=10, traj_index_offset=b)
        q.init(starts[b:b + 1], goals[b:b + 1], hp.bounds)
        singles[b] = q
    for tick in range(10):
        s = _tick_starts(big)
        big.replan(starts=s, n=20)
        split.update_start_points(s.clone())
        split.step(n=20)
        paths = big.get_paths()
        assert np.array_equal(paths[:, 0], s.cpu().numpy()) and np.isfinite(paths).all(), tick
        assert big.step_count == 20 and big.engine.adam_step == 20 * (tick + 1)
        a, c = _engine_arrays(big), _engine_arrays(split)
        for k in a:
            assert np.array_equal(a[k], c[k]), (tick, k)
        for b, q in singles.items():
            q.replan(starts=s[b:b + 1].clone(), n=20)
            o = _engine_arrays(q)
            for k in a:
                assert np.array_equal(o[k][0], a[k][b]), (tick, b, k)


# ---- the drop-in planners -------------------------------------------------------------------------------------------
def _parent_drop_in(planner, point, is_goal):
    """update_goal_point / update_start_point as the planner classes had them (host argmin, four torch launches)."""
    eng = planner._engine
    tr = eng.traj.view(eng.N, eng.D)
    ref = eng.goal if is_goal else eng.start
    ref.copy_(torch.tensor(np.asarray(point, F32))[None])
    if eng.D == 3:
        m = min(int(torch.argmin(torch.sum((tr[:, :2] - ref[:, :2]) ** 2, dim=1))) + 1, tr.shape[0])
    else:
        m = int(torch.argmin(torch.sum((tr - ref) ** 2, dim=1)))
    if is_goal:
        tr[m:] = ref
    else:
        tr[:m] = ref
    eng.reparametrize()


def _drop_in_state(planner):
    e = planner._engine
    torch.cuda.synchronize()
    return {k: _np(getattr(e, k)) for k in ("traj", "start", "goal", "lam", "cm")}


def _check_drop_in(planner, calls):
    e = planner._engine
    saved = {k: v for k, v in _drop_in_state(planner).items() if v is not None}
    for is_goal, point in calls:
        planner._step_count = 9
        (planner.update_goal_point if is_goal else planner.update_start_point)(point)
        assert planner._step_count == 0
    new = _drop_in_state(planner)
    for k, v in saved.items():
        getattr(e, k).copy_(torch.tensor(v).reshape(getattr(e, k).shape))
    for is_goal, point in calls:
        _parent_drop_in(planner, point, is_goal)
    _same_state(new, _drop_in_state(planner))
    assert np.array_equal(new["goal" if calls[-1][0] else "start"][0], np.asarray(calls[-1][1], F32))


def test_drop_in_se2_planner_equals_its_former_formulation():
    z = load_golden("g4_update_endpoints.npz")
    planner = _make(load_golden("g9_full_steps.npz"))
    eng = planner._engine
    eng.traj.copy_(torch.tensor(z["in_traj"]))
    eng.lam.copy_(torch.tensor(z["in_lam"][None]))
    eng.cm.copy_(torch.tensor(z["in_cm"][None]))
    eng.set_endpoints(z["start"][None], z["goal"][None])
    _check_drop_in(planner, [(True, z["new_goal"]), (False, z["new_start"])])
    for c in er.g20_cases(load_golden("g20_endpoint_updates.npz")):
        if c["lam"] is None:
            continue
        eng.traj.copy_(torch.tensor(c["traj"]))
        eng.lam.copy_(torch.tensor(c["lam"][None]))
        eng.cm.copy_(torch.tensor(c["cm"][None]))
        eng.set_endpoints(c["start"][None], c["goal"][None])
        _check_drop_in(planner, [(c["which"] == 1, c["point"])])


def test_drop_in_2d_planner_equals_its_former_formulation():
    torch.random.manual_seed(100)
    np.random.seed(400)
    g11 = load_golden("g11_init_checkers.npz")
    cc = nfopp.CircleCollisionChecker(0.3, (0, 3, 0, 3))
    cc.update_obstacle_points(g11["corridor_obstacles"])
    planner = nfopp.PlannerFactory.make_onf_planner(cc)
    planner._init_collision_iteration = 2
    planner.init(np.array([0.5, 0.5], F32), np.array([2.5, 2.5], F32), (-0.1, 3.1, -0.1, 3.1))
    eng = planner._engine
    for c in er.g20_cases(load_golden("g20_endpoint_updates.npz")):
        if c["lam"] is not None:
            continue
        eng.traj.copy_(torch.tensor(c["traj"]).reshape(eng.traj.shape))
        eng.set_endpoints(c["start"][None], c["goal"][None])
        _check_drop_in(planner, [(c["which"] == 1, c["point"])])
        got = _drop_in_state(planner)["traj"].reshape(c["out_traj"].shape)
        assert np.array_equal(got, c["out_traj"]) or float(np.abs(got - c["out_traj"]).max()) < er.ARRAY_GATE
