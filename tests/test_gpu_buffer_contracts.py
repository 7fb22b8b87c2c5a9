"""GPU: exact extents and independence from prior contents of every buffer the C entries take (include/nfopp_hip.h).

Every other GPU test compares the region a kernel is meant to write with a reference, on exact-size `torch.empty` tensors
that the caching allocator rounds up to 512 bytes and recycles.  Here every entry is called through the raw C ABI three times
on the same inputs:

    plain    exact-size torch tensors, pure outputs and workspaces pre-filled with 0x00 -- the values the other tests pin;
    zeros    every device pointer inside a guarded allocation (tests/guarded.py), outputs and workspaces filled with 0x00;
    ones     the same with 0xFF (NaN as a float, -1 as an integer);

and the following is required, all of it with == on bits or bytes:

  1. every guard is intact and every `const` input allocation is unchanged byte for byte;
  2. every output and in/out buffer of `zeros` equals `plain`;
  3. every element the header says is written has the same bits in `zeros` and `ones`, every element it says is left alone
     still holds its fill, and the rows of in/out state a mask retires still hold the caller's bits.

One table of (entry, case) rows; a case is a list of buffers and a caller.  The shapes are the smallest that reach each code
path of the kernel behind the entry.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import guarded as gd

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
from nfopp import _lib  # noqa: E402
from nfopp import engine as eng  # noqa: E402

F32, I32, U8 = np.float32, np.int32, np.uint8
DEV = "cuda"

# role: "in" const input | "inout" state | "out" pure output | "ws" workspace (contents are the library's own business)
# data: the numpy array ("in", "inout") or (shape, numpy dtype) ("out", "ws")
# written ("out"): boolean mask of the elements the header says are written, None = all
# kept ("inout"): boolean mask of the elements that must keep the caller's bits, None = no such promise
Buf = namedtuple("Buf", "name role data written kept")


def In(name, a):
    return Buf(name, "in", np.ascontiguousarray(a), None, None)


def InOut(name, a, kept=None):
    return Buf(name, "inout", np.ascontiguousarray(a), None, kept)


def Out(name, shape, dtype=F32, written=None):
    return Buf(name, "out", (tuple(shape), np.dtype(dtype)), written, None)


def Ws(name, shape, dtype=U8):
    return Buf(name, "ws", (tuple(shape), np.dtype(dtype)), None, None)


_TORCH = {np.dtype(F32): torch.float32, np.dtype(I32): torch.int32, np.dtype(U8): torch.uint8, np.dtype(np.float64): torch.float64,
          np.dtype(np.int64): torch.int64, np.dtype(np.uint64): torch.int64, np.dtype(np.int8): torch.int8}


def P(t):
    """raw device pointer for ctypes (NULL for None and for an empty tensor)"""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _run(bufs, call, fill, guard):
    """one call of the entry; returns {name: bits} of every buffer but the workspaces"""
    t, parents, snaps = {}, {}, {}
    for b in bufs:
        if b.role in ("in", "inout"):
            a = b.data.view(np.int64) if b.data.dtype == np.uint64 else b.data
            if guard:
                t[b.name], parents[b.name] = gd.from_array(a, DEV)
            else:
                t[b.name] = torch.tensor(a, device=DEV)
        else:
            shape, dtype = b.data
            if guard:
                t[b.name], parents[b.name] = gd.guarded(shape, _TORCH[dtype], DEV, fill)
            else:
                t[b.name] = torch.empty(shape, dtype=_TORCH[dtype], device=DEV)
                t[b.name].view(-1).view(torch.uint8).fill_(fill)
        if guard:
            assert t[b.name].numel() == 0 or t[b.name].data_ptr() % 256 == 0
            if b.role == "in":
                snaps[b.name] = gd.snapshot(parents[b.name])
    torch.cuda.synchronize()
    call(t)
    torch.cuda.synchronize()
    for name, parent in parents.items():
        assert gd.guards_intact(parent), "a store outside %r (fill 0x%02X)" % (name, fill)
    for name, snap in snaps.items():
        assert gd.unchanged(parents[name], snap), "the const input %r was written" % name
    return {b.name: gd.bits(t[b.name]) for b in bufs if b.role != "ws"}


def check_contract(bufs, call):
    plain = _run(bufs, call, 0x00, False)
    zeros = _run(bufs, call, 0x00, True)
    ones = _run(bufs, call, 0xFF, True)
    for b in bufs:
        if b.role in ("in", "ws"):
            continue
        z, o = zeros[b.name], ones[b.name]
        assert np.array_equal(z, plain[b.name]), "%r differs between guarded and plain buffers" % b.name
        if b.role == "inout":
            assert np.array_equal(z, o), "%r depends on the fill of an output or workspace" % b.name
            if b.kept is not None:
                before = b.data.view(z.dtype)
                assert np.array_equal(z[b.kept], before[b.kept]), "%r: a retired element was written" % b.name
            continue
        w = np.ones(z.shape, bool) if b.written is None else np.broadcast_to(b.written, z.shape)
        bad = w & (z != o)
        assert not bad.any(), "%r: %d written elements depend on the prior contents, first at %s" % (
            b.name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert not z[~w].any(), "%r: an element the header leaves alone was written (fill 0x00)" % b.name
        assert (o[~w] == np.iinfo(o.dtype).max).all(), "%r: an element the header leaves alone was written (fill 0xFF)" % b.name


def test_a_planted_write_is_reported_on_the_device():
    """the CPU test of the helper, once more where the kernels run: a plain torch write inside the test's own allocation"""
    view, parent = gd.guarded((33, 4), torch.float32, DEV, 0xFF)
    off, n = gd.span(parent)
    snap = gd.snapshot(parent)
    assert gd.guards_intact(parent) and view.data_ptr() % 256 == 0 and bool(torch.isnan(view).all())
    for at in (off - 1, off + n):
        parent[at] = 0
        assert not gd.guards_intact(parent) and not gd.unchanged(parent, snap)
        parent[at] = gd.GUARD_BYTE
        assert gd.guards_intact(parent)
    view[32, 3] = 1.0
    assert gd.guards_intact(parent) and not gd.unchanged(parent, snap)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
# (use_cos, angle, bias): F = 220, 200, 120, 100, and 200 without the encoding bias
CONFIGS = [(True, True, True), (True, False, True), (False, True, False), (False, False, True), (True, False, False)]
_ONFS = {}


def _onf(cfg):
    if cfg not in _ONFS:
        use_cos, angle, bias = cfg
        torch.random.manual_seed(11)
        onf = nfopp.ONF(0.4, 2.5, use_cos=use_cos, use_normal_init=True, bias=bias, angle_encoding=angle).to(DEV)
        _ONFS[cfg] = (onf, onf.flat_parameters.cpu().numpy().copy())
    return _ONFS[cfg]


def _lib_on_path(path):
    lib = _lib.load()
    _lib.check(lib.nfopp_set_matrix_path(path))      # tests/conftest.py puts the switch back after every test
    return lib


def _poses(rng, n, d, lo=-4.0, hi=6.0):
    x = rng.uniform(lo, hi, (n, d)).astype(F32)
    if d == 3:
        x[:, 2] = rng.uniform(-3.3, 3.3, n)
    return x


def _walk(rng, B, N, D, step=0.15):
    """B trajectories of N waypoints that go somewhere: a random walk from a random start, headings anywhere"""
    tr = np.cumsum(rng.normal(0.05, step, (B, N + 2, D)), 1) + rng.uniform(0.5, 2.5, (B, 1, D))
    if D == 3:
        tr[..., 2] = rng.uniform(-3.3, 3.3, (B, N + 2))
    tr = tr.astype(F32)
    return tr[:, 1:-1].copy(), tr[:, 0].copy(), tr[:, -1].copy()


def _retired(B, mask):
    """None | "fml": the first, a middle and the last trajectory retire | "last": only the last one does"""
    if mask is None:
        return None
    active = np.ones(B, U8)
    active[[0, B // 2, B - 1] if mask == "fml" else [B - 1]] = 0
    return active


def _rows(active, B, *tail):
    """boolean mask [B, *tail] of the rows of live trajectories (None without a mask: everything)"""
    if active is None:
        return None
    return np.broadcast_to((active != 0).reshape((B,) + (1,) * len(tail)), (B,) + tail).copy()


def _kept(active, B, *tail):
    return None if active is None else ~_rows(active, B, *tail)


CASES = []


def table(name, rows):
    """one table row per parameter tuple: fn(*row) yields the (buffers, caller) pairs of the row (the test is at the end)"""
    def deco(fn):
        for row in rows:
            CASES.append(pytest.param(lambda row=row: fn(*row), id="%s-%s" % (name, "-".join(str(v) for v in row))))
        return fn
    return deco


# ---- nfopp_onf_eval_points / nfopp_onf_eval_logits ----------------------------------------------------------------------------
@table("onf_eval", [(e, p, k) for e in ("nfopp_onf_eval_points", "nfopp_onf_eval_logits") for p in (1, 2, 0) for k in range(5)])
def _onf_eval(entry, path, k):
    onf, flat = _onf(CONFIGS[k])
    lib = _lib_on_path(path)
    rng = np.random.default_rng(3)
    for n in (1, 33, 300, 4099, 70001):      # 70001: the second workgroup shape, two tiles per wave
        x = _poses(rng, n, onf.point_dim)

        def call(t, n=n):
            _lib.check(getattr(lib, entry)(onf.config_c(), P(t["params"]), P(t["points"]), n, P(t["out4"]), _lib.stream_ptr()))
        yield [In("params", flat), In("points", x), Out("out4", (n, 4))], call


# ---- nfopp_traj_collision_eval --------------------------------------------------------------------------------------------------
@table("collision_eval", [(D, B, N, tm, m) for D in (3, 2) for (B, N) in ((1, 2), (3, 17), (5, 100)) for tm in (0, 1)
                          for m in (None, "fml", "last")])
def _collision_eval(D, B, N, t_mode, mask):
    onf, flat = _onf(CONFIGS[0] if D == 3 else CONFIGS[1])
    lib = _lib.load()
    rng = np.random.default_rng(100 * B + N)
    traj, _, _ = _walk(rng, B, N, D)
    active = _retired(B, mask)
    bufs = [In("params", flat), In("traj", traj), Out("out4", (B, N - 1, 4), written=_rows(active, B, N - 1, 4))]
    bufs.append(In("t", rng.random((B, N - 1)).astype(F32)) if t_mode == 0 else Out("t", (B, N - 1), written=_rows(active, B, N - 1)))
    if active is not None:
        bufs += [In("active", active), Ws("live", (B + 1,), I32)]

    def call(t):
        _lib.check(lib.nfopp_traj_collision_eval(onf.config_c(), P(t["params"]), P(t["traj"]), B, N, D, P(t["t"]), t_mode, 1234, 5, 7,
                                                 P(t["out4"]), P(t.get("active")), P(t.get("live")), _lib.stream_ptr()))
    yield bufs, call


# ---- nfopp_traj_update ------------------------------------------------------------------------------------------------------------
BOUNDS = (-0.1, 3.1, -0.1, 3.1)
HYPER3 = nfopp.TrajectoryHyper(collision_weight=3, direction_delta_weight=7, collision_beta=2, bounds=BOUNDS)
HYPER2 = nfopp.TrajectoryHyper(collision_weight=0.01, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, bounds=BOUNDS)


def _band(N, w):
    band, half = eng.band_of(eng.inverse_hessian(N, w))
    return band, half, eng.interior_range(band)


def _state(rng, B, N, D, active):
    """the in/out state of a batch in mid-flight and its const companions, as buffers"""
    traj, start, goal = _walk(rng, B, N, D)
    bufs = [InOut("traj", traj, _kept(active, B, N, D)), In("start", start), In("goal", goal)]
    if D == 3:
        bufs += [InOut("lam", rng.normal(0, 0.1, (B, N + 1)).astype(F32), _kept(active, B, N + 1)),
                 InOut("cm", rng.uniform(0, 0.2, (B, N)).astype(F32), _kept(active, B, N))]
    if active is not None:
        bufs.append(In("active", active))
    return bufs


def _moments(rng, B, N, D, active):
    return [InOut("adam_m", rng.normal(0, 0.01, (B, N, D)).astype(F32), _kept(active, B, N, D)),
            InOut("adam_v", (rng.normal(0, 0.01, (B, N, D)) ** 2).astype(F32), _kept(active, B, N, D))]


UPDATE_SHAPES = [(3, 1, 2, 0.5), (3, 3, 17, 0.5), (3, 2, 300, 3.0), (3, 2, 256, 10.0),      # the last: boundary band from global memory
                 (2, 1, 2, 0.5), (2, 2, 300, 0.5)]


@table("traj_update", [s + (terms, m) for s in UPDATE_SHAPES for terms in (True, False) for m in (None, "fml", "last")])
def _traj_update(D, B, N, w, want_terms, mask):
    lib = _lib.load()
    rng = np.random.default_rng(7 * N + B)
    active = _retired(B, mask)
    band, half, interior = _band(N, w)
    out4 = rng.normal(0, 1, (B, N - 1, 4)).astype(F32)
    if D == 2:
        out4[..., 3] = 0
    bufs = _state(rng, B, N, D, active) + _moments(rng, B, N, D, active)
    bufs += [In("t", rng.random((B, N - 1)).astype(F32)), In("out4", out4), In("band", band)]
    if want_terms:
        bufs.append(Out("terms", (B, _lib.NUM_TERMS), written=_rows(active, B, _lib.NUM_TERMS)))
    hp = (HYPER3 if D == 3 else HYPER2).to_c(4)

    def call(t):
        _lib.check(lib.nfopp_traj_update(hp, B, N, D, P(t["traj"]), P(t["start"]), P(t["goal"]), P(t.get("lam")), P(t.get("cm")),
                                         P(t["adam_m"]), P(t["adam_v"]), P(t["t"]), P(t["out4"]), P(t["band"]), half, interior[0],
                                         interior[1], P(t.get("terms")), P(t.get("active")), _lib.stream_ptr()))
    yield bufs, call


# ---- nfopp_reparametrize ----------------------------------------------------------------------------------------------------------
def _u(N):
    return torch.linspace(0, 1, N + 2)[1:-1].contiguous().numpy()      # CPU linspace: the reference's rounding


@table("reparametrize", [s[:3] + (m,) for s in UPDATE_SHAPES for m in (None, "fml", "last")])
def _reparametrize(D, B, N, mask):
    lib = _lib.load()
    rng = np.random.default_rng(11 * N + B)
    active = _retired(B, mask)
    bufs = _state(rng, B, N, D, active) + [In("u", _u(N))]

    def call(t):
        _lib.check(lib.nfopp_reparametrize(B, N, D, P(t["traj"]), P(t["start"]), P(t["goal"]), P(t.get("lam")), P(t.get("cm")),
                                           P(t["u"]), P(t.get("active")), _lib.stream_ptr()))
    yield bufs, call


# ---- nfopp_traj_steps: every buffer of nfopp_traj_buffers ---------------------------------------------------------------------
@table("traj_steps", [(tm, m) for tm in (0, 1) for m in (None, "fml", "last")])
def _traj_steps(t_mode, mask):
    D, B, N, n_steps = 3, 3, 17, 3
    onf, flat = _onf(CONFIGS[0])
    lib = _lib.load()
    rng = np.random.default_rng(41)
    active = _retired(B, mask)
    band, half, interior = _band(N, 0.5)
    bufs = [In("params", flat)] + _state(rng, B, N, D, active) + _moments(rng, B, N, D, active)
    bufs += [In("band", band), In("u", _u(N)), Out("out4", (B, N - 1, 4), written=_rows(active, B, N - 1, 4)),
             Out("terms", (B, _lib.NUM_TERMS), written=_rows(active, B, _lib.NUM_TERMS))]
    if t_mode == 0:      # the draws come from t_steps; the scratch row of t_mode 1 is not touched
        bufs += [In("t_steps", rng.random((n_steps, B, N - 1)).astype(F32)), Out("t", (B, N - 1), written=np.zeros((B, N - 1), bool))]
    else:
        bufs.append(Out("t", (B, N - 1), written=_rows(active, B, N - 1)))
    if active is not None:
        bufs.append(Ws("live", (B + 1,), I32))
    hp = HYPER3.to_c(1)

    def call(t):
        pp = lambda name: P(t.get(name))      # noqa: E731
        buf = _lib.TrajBuffersC(pp("traj"), pp("start"), pp("goal"), pp("lam"), pp("cm"), pp("adam_m"), pp("adam_v"), pp("t"),
                                pp("out4"), pp("band"), pp("u"), pp("active"), pp("live"), B, N, D, half, interior[0], interior[1])
        sched = _lib.StepScheduleC(float(HYPER3.lr), 0.9, 0.9, 4, 6, 7, 1234, 5, 2, t_mode)
        _lib.check(lib.nfopp_traj_steps(onf.config_c(), pp("params"), hp, buf, sched, n_steps, pp("t_steps"), pp("terms"),
                                        _lib.stream_ptr()))
    yield bufs, call


# ---- nfopp_onf_train_grad_ex ------------------------------------------------------------------------------------------------------
@table("onf_train_grad", [(fp, n, k, mp) for (fp, counts) in ((1, (1, 33, 2047)), (2, (33, 4099, 70001))) for n in counts
                          for k in (0, 3) for mp in (1, 2, 0)])
def _onf_train_grad(fit_path, n, k, matrix_path):
    onf, flat = _onf(CONFIGS[k])
    lib = _lib_on_path(matrix_path)
    rng = np.random.default_rng(n)
    x = _poses(rng, n, onf.point_dim)
    y = (rng.uniform(size=n) < 0.35).astype(F32)
    need = lib.nfopp_onf_train_workspace_bytes(onf.config_c(), n)
    assert need > 0

    def call(t):
        _lib.check(lib.nfopp_onf_train_grad_ex(onf.config_c(), P(t["params"]), P(t["samples"]), P(t["labels"]), n, 1.0 / n,
                                               P(t["grad"]), P(t["ws"]), need, fit_path, _lib.stream_ptr()))
    # exactly the bytes the library asks for: the ragged last chunk of csrc/onf_wgrad.hip has nothing behind it
    yield [In("params", flat), In("samples", x), In("labels", y), Out("grad", (onf.n_params + 2,)), Ws("ws", (need,))], call


# ---- nfopp_adam_step --------------------------------------------------------------------------------------------------------------
@table("adam_step", [(n,) for n in (1, 255, 256, 257, 2048 * 256 + 3)])      # the last: past the grid cap, the stride loop runs
def _adam_step(n):
    lib = _lib.load()
    rng = np.random.default_rng(n)
    bufs = [InOut("param", rng.normal(0, 1, n).astype(F32)), In("grad", rng.normal(0, 1, n).astype(F32)),
            InOut("m", rng.normal(0, 0.1, n).astype(F32)), InOut("v", (rng.normal(0, 0.1, n) ** 2).astype(F32))]

    def call(t):
        _lib.check(lib.nfopp_adam_step(P(t["param"]), P(t["grad"]), P(t["m"]), P(t["v"]), n, 0.999, 1 - 0.9, 1 - 0.999, 1e-8,
                                       5e-2 / (1 - 0.9 ** 3), math.sqrt(1 - 0.999 ** 3), _lib.stream_ptr()))
    yield bufs, call


# ---- nfopp_init_trajectories / nfopp_path_interpolate / nfopp_path_select_best ------------------------------------------------
@table("init_trajectories", [(D, N, dr) for D in (3, 2) for N in (1, 33, 300) for dr in ((0, 1) if D == 3 else (0,))])
def _init_trajectories(D, N, directed):
    lib = _lib.load()
    B = 3
    rng = np.random.default_rng(N)
    _, start, goal = _walk(rng, B, N, D)

    def call(t):
        _lib.check(lib.nfopp_init_trajectories(P(t["start"]), P(t["goal"]), B, N, D, directed, P(t["traj"]), _lib.stream_ptr()))
    yield [In("start", start), In("goal", goal), Out("traj", (B, N, D))], call


@table("path_interpolate", [(D, N, sub) for D in (3, 2) for N in (1, 33, 300) for sub in (1, 5)])
def _path_interpolate(D, N, sub):
    lib = _lib.load()
    B = 3
    rng = np.random.default_rng(N + sub)
    traj, start, goal = _walk(rng, B, N, D)

    def call(t):
        _lib.check(lib.nfopp_path_interpolate(P(t["traj"]), P(t["start"]), P(t["goal"]), B, N, D, sub, P(t["poses"]), P(t["length"]),
                                              _lib.stream_ptr()))
    yield [In("traj", traj), In("start", start), In("goal", goal), Out("poses", (B, (N + 1) * sub + 1, D)), Out("length", (B,))], call


@table("path_select_best", [(D, N, m, act) for D in (3, 2) for N in (1, 33, 300) for m in (1, 171, 1506) for act in (False, True)])
def _path_select_best(D, N, m, with_active):
    """six paths: free and shorter (new best) | free, not shorter (retires) | colliding | free and shorter but already retired |
    colliding in the last pose only | free against an infinite best length.  N * D = 2 .. 900: below and above one trip of 256"""
    lib = _lib.load()
    B = 6
    rng = np.random.default_rng(N + m)
    traj, _, _ = _walk(rng, B, N, D)
    labels = np.zeros((B, m), F32)
    labels[2, m // 2] = 1
    labels[4, m - 1] = 1
    length = np.array([1, 3, 1, 1, 1, 5], F32)
    best_length = np.array([2, 2, 2, 2, 2, np.inf], F32)
    best = rng.normal(0, 1, (B, N, D)).astype(F32)
    improves = np.array([1, 0, 0, 0 if with_active else 1, 0, 1], bool)
    bufs = [In("labels", labels), In("length", length), In("traj", traj),
            InOut("best_traj", best, np.broadcast_to(~improves[:, None, None], best.shape).copy()),
            InOut("best_length", best_length, ~improves), Out("collides", (B,), U8)]
    if with_active:
        bufs.append(InOut("active", np.array([1, 1, 1, 0, 1, 1], U8), np.array([1, 0, 1, 1, 1, 1], bool)))

    def call(t):
        _lib.check(lib.nfopp_path_select_best(P(t["labels"]), P(t["length"]), P(t["traj"]), B, m, N, D, P(t["best_traj"]),
                                              P(t["best_length"]), P(t["collides"]), P(t.get("active")), _lib.stream_ptr()))
    yield bufs, call


# ---- nfopp_sample_candidates / nfopp_resample_pool: the shapes of test_batch_sampler_vs_oracle_and_shard_invariance -----------
SAMPLER = dict(B=5, N=60, cap=40, nf=10)


def _f4(v):
    return (ctypes.c_float * 4)(*v)


@table("sample_candidates", [(D, full) for D in (3, 2) for full in (False, True)])
def _sample_candidates(D, pool_full):
    lib = _lib.load()
    B, N, cap, nf = (SAMPLER[k] for k in ("B", "N", "cap", "nf"))
    C, S, pool_n = cap + N - 1, N - 1 + cap + nf, cap if pool_full else 0
    rng = np.random.default_rng(D)
    prev = rng.uniform(0.2, 2.8, (B, N, D)).astype(F32)
    cand_w = np.zeros((B, C), bool)
    cand_w[:, :pool_n + N - 1] = True                      # the retained pool, then the N - 1 fine copies
    smp_w = np.ones((B, S), bool)
    smp_w[:, N - 1:N - 1 + cap] = False                    # the pool's slot belongs to nfopp_resample_pool
    bufs = [In("prev", prev), In("pool", rng.uniform(0, 3, (B, cap, D)).astype(F32)), In("pool_age", rng.integers(1, 9, (B, cap)).astype(F32)),
            Out("cand", (B, C, D), written=cand_w[:, :, None]), Out("cand_age", (B, C), written=cand_w),
            Out("samples", (B, S, D), written=smp_w[:, :, None])]

    def call(t):
        _lib.check(lib.nfopp_sample_candidates(P(t["prev"]), B, N, D, cap, pool_n, nf, 1.5, 0.02, 0.3, _f4(BOUNDS), 21, 1, 3,
                                               P(t["pool"]), P(t["pool_age"]), P(t["cand"]), P(t["cand_age"]), P(t["samples"]),
                                               _lib.stream_ptr()))
    yield bufs, call


@table("resample_pool", [(D, full) for D in (3, 2) for full in (False, True)])
def _resample_pool(D, pool_full):
    lib = _lib.load()
    B, N, cap, nf = (SAMPLER[k] for k in ("B", "N", "cap", "nf"))
    C, S, pool_n = cap + N - 1, N - 1 + cap + nf, cap if pool_full else 0
    n_cand = pool_n + N - 1
    rng = np.random.default_rng(D + 10)
    smp_w = np.zeros((B, S), bool)
    smp_w[:, N - 1:N - 1 + cap] = True
    bufs = [In("cand", rng.uniform(0, 3, (B, C, D)).astype(F32)), In("cand_age", rng.integers(0, 9, (B, C)).astype(F32)),
            In("out4", rng.normal(0, 2, (B, C, 4)).astype(F32)), Out("pool", (B, cap, D)), Out("pool_age", (B, cap)),
            Out("samples", (B, S, D), written=smp_w[:, :, None])]

    def call(t):
        _lib.check(lib.nfopp_resample_pool(B, n_cand, C, cap, D, S, N - 1, 21, 1, 3, P(t["cand"]), P(t["cand_age"]), P(t["out4"]),
                                           P(t["pool"]), P(t["pool_age"]), P(t["samples"]), _lib.stream_ptr()))
    yield bufs, call


# ---- the five ground-truth checkers: every one of labels_dev[n] is written ------------------------------------------------
def _cell_index(obst, x0, y0, cell, cx, cy):
    """the index nfopp_build_cell_index builds, restated: fp32 cell numbers clamped into the region, a stable sort"""
    ix = np.clip(np.floor((obst[:, 0] - F32(x0)) / F32(cell)), 0, cx - 1).astype(np.int64)
    iy = np.clip(np.floor((obst[:, 1] - F32(y0)) / F32(cell)), 0, cy - 1).astype(np.int64)
    c = iy * cx + ix
    order = np.argsort(c, kind="stable")
    return obst[order].copy(), np.searchsorted(c[order], np.arange(cx * cy + 1)).astype(I32)


CHECKERS = ("circle", "circle_cells", "rectangle", "rectangle_cells", "grid")


@table("check_collision", [(kind, n) for kind in CHECKERS for n in (1, 255, 257)])
def _check_collision(kind, n):
    lib = _lib.load()
    rng = np.random.default_rng(n)
    poses = _poses(rng, n, 3, -0.3, 3.3)
    obst = rng.uniform(0, 3, (40, 2)).astype(F32)
    box = (-0.2, 0.4, -0.15, 0.15)
    reach = float(np.float32(math.hypot(0.4, 0.15)) * np.float32(1.001))
    cell, cx, cy = 0.5, 6, 6
    sorted_obst, cell_start = _cell_index(obst, 0.0, 0.0, cell, cx, cy)
    grid = (rng.uniform(size=(16, 20)) < 0.3).astype(U8)
    bufs = [In("poses", poses), Out("labels", (n,))]
    if kind == "grid":
        bufs.append(In("grid", grid))
    elif kind.endswith("_cells"):
        bufs += [In("obstacles", sorted_obst), In("cell_start", cell_start)]
    else:
        bufs.append(In("obstacles", obst))

    def call(t):
        st = _lib.stream_ptr()
        if kind == "circle":
            rc = lib.nfopp_check_collision_circle(P(t["poses"]), n, 3, P(t["obstacles"]), len(obst), 0.3, _f4(BOUNDS), P(t["labels"]), st)
        elif kind == "circle_cells":
            rc = lib.nfopp_check_collision_circle_cells(P(t["poses"]), n, 3, P(t["obstacles"]), len(obst), P(t["cell_start"]), cx, cy,
                                                        0.0, 0.0, cell, 0.3, _f4(BOUNDS), P(t["labels"]), st)
        elif kind == "rectangle":
            rc = lib.nfopp_check_collision_rectangle(P(t["poses"]), n, P(t["obstacles"]), len(obst), _f4(box), _f4(BOUNDS),
                                                     P(t["labels"]), st)
        elif kind == "rectangle_cells":
            rc = lib.nfopp_check_collision_rectangle_cells(P(t["poses"]), n, P(t["obstacles"]), len(obst), P(t["cell_start"]), cx, cy,
                                                           0.0, 0.0, cell, _f4(box), reach, _f4(BOUNDS), P(t["labels"]), st)
        else:
            rc = lib.nfopp_check_collision_grid(P(t["poses"]), n, 3, P(t["grid"]), 16, 20, 0.0, 0.0, 0.18, P(t["labels"]), st)
        _lib.check(rc)
    yield bufs, call


# ---- entries with a workspace_dev: exactly the bytes *_workspace_bytes returns, results independent of what it held ---------
# The smallest case of each entry's own GPU test that makes the entry use its workspace; the outputs carry sentinels in those
# tests already, so only their fill-independence and the guards are looked at here (every output element is written).
import fleet_schedule_cases as fc  # noqa: E402
import grid_search_ref as gsr  # noqa: E402
import lattice_cases as lc  # noqa: E402
import spacetime_cases as sc  # noqa: E402
import track_conflict_cases as tcc  # noqa: E402

F64, I64 = np.float64, np.int64


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, F32)


@table("grid_distance_fields", [(4095, 1, "random")])          # the first shape of the grid-search tests that relaxes in the workspace
def _grid_distance_fields(rows, cols, kind):
    lib = _lib.load()
    occ = gsr.make_map(kind, rows, cols)
    goals = np.ascontiguousarray(gsr.shape_goals(occ), I32)
    need = lib.nfopp_grid_fields_workspace_bytes(rows, cols, len(goals))
    assert need > 0

    def call(t):
        _lib.check(lib.nfopp_grid_distance_fields(P(t["occ"]), rows, cols, P(t["goals"]), len(goals), P(t["fields"]), P(t["ws"]), need,
                                                  _lib.stream_ptr()))
    yield [In("occ", occ), In("goals", goals), Out("fields", (len(goals), rows, cols, 2), I32), Ws("ws", (need,))], call


@table("grid_seed_trajectories", [(D, directed) for D, directed in ((3, 0), (3, 1), (2, 0))])
def _grid_seed_trajectories(D, directed):
    """a 3-cell path and the 1168-cell row: one cell more than the LDS form holds"""
    lib = _lib.load()
    cases = {c["name"]: c for c in gsr.seed_cases()}
    rows = [cases["c3"], cases["row1168"]]
    B, max_len, n = len(rows), 1168, 257
    cells = np.zeros((B, max_len, 2), I32)
    for i, c in enumerate(rows):
        cells[i, :len(c["cells"])] = c["cells"]
    count = np.asarray([len(c["cells"]) for c in rows], I32)
    start = np.stack([c["start"][:D] for c in rows]).astype(F32)
    goal = np.stack([c["goal"][:D] for c in rows]).astype(F32)
    need = lib.nfopp_grid_seed_workspace_bytes(B, max_len)
    assert need > 0
    b = gsr.SEED_BOUNDARIES

    def call(t):
        _lib.check(lib.nfopp_grid_seed_trajectories(P(t["cells"]), P(t["count"]), P(t["status"]), B, max_len, P(t["start"]), P(t["goal"]),
                                                    n, D, directed, b[0], b[2], gsr.SEED_RESOLUTION, P(t["traj"]), P(t["ws"]), need,
                                                    _lib.stream_ptr()))
    yield [In("cells", cells), In("count", count), In("status", np.zeros(B, I32)), In("start", start), In("goal", goal),
           Out("traj", (B, n, D)), Ws("ws", (need,))], call


@table("build_cell_index", [(n,) for n in (1, 33, 3000)])
def _build_cell_index(n):
    lib = _lib.load()
    rng = np.random.default_rng(n)
    pts = rng.uniform(-1, 10, (n, 2)).astype(F32)
    nx, ny = 9, 7
    need = lib.nfopp_cell_index_workspace_bytes(n)
    assert need > 0

    def call(t):
        _lib.check(lib.nfopp_build_cell_index(P(t["points"]), n, 0.0, 0.0, 1.0, nx, ny, P(t["sorted"]), P(t["cell_start"]), P(t["ws"]), need,
                                              _lib.stream_ptr()))
    yield [In("points", pts), Out("sorted", (n, 2)), Out("cell_start", (nx * ny + 1,), I32), Ws("ws", (need,))], call


@table("grid_edt", [(13, 15, 0), (13, 15, 1), (64, 300, 0)])
def _grid_edt(rows, cols, border):
    lib = _lib.load()
    occ = gsr.make_map("random", rows, cols)
    need = lib.nfopp_grid_edt_workspace_bytes(rows, cols)
    assert need > 0

    def call(t):
        _lib.check(lib.nfopp_grid_edt(P(t["occ"]), rows, cols, border, P(t["dist2"]), P(t["nearest"]), P(t["ws"]), need, _lib.stream_ptr()))
    yield [In("occ", occ), Out("dist2", (rows, cols), I32), Out("nearest", (rows, cols), I32), Ws("ws", (need,))], call


@table("lattice_distance_fields", sorted(lc.WIDE)[:1])          # ("40x130", 1): 32 + 32-bit counts in the workspace
def _lattice_distance_fields(name, turn_cost):
    lib = _lib.load()
    rows, cols = lc.SHAPES[name][:2]
    layers = np.ascontiguousarray(lc.layers_of(name), U8)
    goals = np.ascontiguousarray(lc.goals_of(name), I32)
    need = lib.nfopp_lattice_fields_workspace_bytes(rows, cols, turn_cost, len(goals))
    assert need > 0

    def call(t):
        _lib.check(lib.nfopp_lattice_distance_fields(P(t["layers"]), layers.shape[0], rows, cols, P(t["goals"]), len(goals), turn_cost,
                                                     P(t["fields"]), P(t["ws"]), need, _lib.stream_ptr()))
    yield [In("layers", layers), In("goals", goals), Out("fields", (len(goals), 8, rows, cols, 2), I32), Ws("ws", (need,))], call


@table("track_conflicts", [(3, 5, 7), (3, None, 7)])            # A against B, and self mode
def _track_conflicts(ba, bb, k):
    lib = _lib.load()
    c = tcc.random_case(1000 * ba + k, ba, bb, k, bad=True)
    self_mode = c["b"] is None
    a, b = _f32(c["a"]), _f32(c["b"])
    nb, sb = (0, 2) if self_mode else (b.shape[0], b.shape[2])
    need = lib.nfopp_track_conflicts_workspace_bytes(ba, nb, k)
    assert need > 0
    bufs = [In("a", a), In("radius_a", _f32(c["radius_a"])), Out("summary", (ba, 7), F64),
            Out("pair_gap", (ba, ba if self_mode else nb), F64), Out("pair_first", (ba, ba if self_mode else nb), F64), Ws("ws", (need,))]
    if not self_mode:
        bufs += [In("b", b), In("radius_b", _f32(c["radius_b"])), Out("summary_b", (nb, 7), F64)]

    def call(t):
        _lib.check(lib.nfopp_track_conflicts(P(t["a"]), ba, a.shape[2], P(t.get("b")), nb, sb, k, c["t0"], c["dt"], P(t["radius_a"]),
                                             P(t.get("radius_b")), c["margin"], P(t["summary"]), P(t.get("summary_b")), P(t["pair_gap"]),
                                             P(t["pair_first"]), P(t["ws"]), need, _lib.stream_ptr()))
    yield bufs, call


@table("fleet_shift_masks", [(3, 5, 3, 1, 3), (33, 33, 32, 33, 2)])      # the workspace is the obstacles' side: m >= 1
def _fleet_shift_masks(b, k, max_delay, m, stride):
    lib = _lib.load()
    c = fc.sized_case(b, k, max_delay, m=m, stride=stride)
    tracks, obst = _f32(c["tracks"]), _f32(c["obstacles"])
    need = lib.nfopp_fleet_shift_masks_workspace_bytes(b, m)
    assert need > 0 and obst.shape[0] == m

    def call(t):
        _lib.check(lib.nfopp_fleet_shift_masks(P(t["tracks"]), b, tracks.shape[2], k, P(t["radius"]), c["margin"], max_delay,
                                               P(t["obstacles"]), m, obst.shape[2], P(t["obstacle_radius"]), P(t["pair"]), P(t["base"]),
                                               P(t["bad"]), P(t["ws"]), need, _lib.stream_ptr()))
    yield [In("tracks", tracks), In("radius", _f32(c["radius"])), In("obstacles", obst), In("obstacle_radius", _f32(c["obstacle_radius"])),
           Out("pair", (b, b, 2), I64), Out("base", (b,), I64), Out("bad", (b,), I32), Ws("ws", (need,))], call


def _spacetime_geometry(c):
    g = c["geo"]
    return g.rows, g.cols, c["T"], g.b0, g.b2, g.res, c["robot_radius"], c["margin"]


def _reservation(c, movers):
    """the reservation of case `c` as int64 words from the device's own entries on plain tensors: static part, then the movers"""
    lib = _lib.load()
    g = c["geo"]
    nbytes = lib.nfopp_spacetime_reservation_bytes(g.rows, g.cols, c["T"])
    words = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    occ = torch.tensor(c["occ"], device=DEV)
    _lib.check(lib.nfopp_spacetime_reservation_init(P(occ), g.rows, g.cols, c["T"], P(words), nbytes, _lib.stream_ptr()))
    if movers and c["tracks"] is not None:
        tr = torch.tensor(_f32(c["tracks"]), device=DEV)
        radius = torch.tensor(_f32(c["radius"]), device=DEV)
        visible = None if c["visible"] is None else torch.tensor(np.ascontiguousarray(c["visible"], U8), device=DEV)
        need = lib.nfopp_spacetime_reserve_workspace_bytes(tr.shape[0])
        ws = torch.zeros(max(need, 1), dtype=torch.uint8, device=DEV)
        _lib.check(lib.nfopp_spacetime_reserve(*_spacetime_geometry(c), P(tr), tr.shape[0], tr.shape[2], P(radius), P(visible), P(words),
                                               nbytes, P(ws), need, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return words.cpu().numpy(), nbytes


@table("spacetime_reservation_init", [("sized", 2), ("sized", 5), ("T1", 0)])
def _spacetime_reservation_init(kind, n):
    """the whole reservation is a pure output: walls, the image edge, the padding bits and a cleared `last`, T = 1 included"""
    lib = _lib.load()
    c = sc.sized_case(n) if kind == "sized" else sc.single_instant((0, 2), False)
    g = c["geo"]
    assert kind == "sized" or c["T"] == 1
    nbytes = lib.nfopp_spacetime_reservation_bytes(g.rows, g.cols, c["T"])
    assert nbytes > 0 and nbytes % 8 == 0

    def call(t):
        _lib.check(lib.nfopp_spacetime_reservation_init(P(t["occ"]), g.rows, g.cols, c["T"], P(t["words"]), nbytes, _lib.stream_ptr()))
    yield [In("occ", np.ascontiguousarray(c["occ"], U8)), Out("words", (nbytes // 8,), I64)], call


@table("spacetime_reserve", [(3,), (6,)])
def _spacetime_reserve(n):
    lib = _lib.load()
    c = sc.sized_case(n)
    words, nbytes = _reservation(c, movers=False)
    tr = _f32(c["tracks"])
    m = tr.shape[0]
    need = lib.nfopp_spacetime_reserve_workspace_bytes(m)
    assert need > 0
    bufs = [In("tracks", tr), In("radius", _f32(c["radius"])), InOut("words", words), Ws("ws", (need,))]
    if c["visible"] is not None:
        bufs.append(In("visible", np.ascontiguousarray(c["visible"], U8)))

    def call(t):
        _lib.check(lib.nfopp_spacetime_reserve(*_spacetime_geometry(c), P(t["tracks"]), m, tr.shape[2], P(t["radius"]), P(t.get("visible")),
                                               P(t["words"]), nbytes, P(t["ws"]), need, _lib.stream_ptr()))
    yield bufs, call


@table("spacetime_plan_fleet", [(3,), (6,)])
def _spacetime_plan_fleet(n):
    lib = _lib.load()
    c = sc.sized_case(n)
    g, T = c["geo"], c["T"]
    words, nbytes = _reservation(c, movers=True)
    starts, goals = np.ascontiguousarray(c["starts"], I32).reshape(-1, 2), np.ascontiguousarray(c["goals"], I32).reshape(-1, 2)
    r = len(starts)
    need = lib.nfopp_spacetime_plan_workspace_bytes(g.rows, g.cols, T, r)
    assert need > 0
    bufs = [In("occ", np.ascontiguousarray(c["occ"], U8)), In("starts", starts), In("goals", goals), InOut("words", words),
            Out("cells", (r, T), I32), Out("arrival", (r,), I32), Out("status", (r,), I32), Out("tracks", (r, T, 2)), Ws("ws", (need,))]
    if c["order"] is not None:
        bufs.append(In("order", np.ascontiguousarray(c["order"], I32)))

    def call(t):
        _lib.check(lib.nfopp_spacetime_plan_fleet(P(t["occ"]), *_spacetime_geometry(c), P(t["starts"]), P(t["goals"]), P(t.get("order")), r,
                                                  P(t["words"]), nbytes, P(t["cells"]), P(t["arrival"]), P(t["status"]), P(t["tracks"]),
                                                  P(t["ws"]), need, _lib.stream_ptr()))
    yield bufs, call


@pytest.mark.parametrize("build", CASES)
def test_buffer_contract(build):
    for bufs, call in build():
        check_contract(bufs, call)
