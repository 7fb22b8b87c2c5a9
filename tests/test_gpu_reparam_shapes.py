"""GPU: nfopp_reparametrize (csrc/reparam.hip, body in csrc/reparam.h) bit for bit against the oracle and the reference's
recorded digests (tests/golden/g23_reparam_shapes.npz) at every size at which the kernel takes another branch and on every
input kind of tests/reparam_cases.py, through the C ABI: the LDS limits, mixed batches, the active mask, idempotence on the
initialiser's line, and nfopp_update_endpoints -- which runs the same device functions -- against tests/endpoint_ref.py at
sizes that cross the sum and scan branches.  tests/test_reparam_shapes_cpu.py holds the oracle to the reference, exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import endpoint_ref as er  # noqa: E402
import reparam_cases as rc  # noqa: E402
from nfopp import _lib  # noqa: E402

F32 = np.float32
DEV = "cuda"
_GRIDS = {}


def _grid(n):
    """The CPU torch.linspace, as nfopp/engine.py builds it: the reference's rounding of the grid."""
    if n not in _GRIDS:
        _GRIDS[n] = torch.linspace(0, 1, n + 2)[1:-1].contiguous().to(DEV)
    return _GRIDS[n]


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


class Batch(object):
    """Device copies of the rows `cases` (all of one N and D): traj [B,N,D], start / goal [B,D], lam [B,N+1], cm [B,N]."""
    NAMES = ("traj", "start", "goal", "lam", "cm")

    def __init__(self, cases):
        self.host = {k: (None if cases[0][k] is None else np.stack([c[k] for c in cases])) for k in self.NAMES}
        self.B, self.N, self.D = self.host["traj"].shape
        self.dev = {k: _dev(v) for k, v in self.host.items()}

    def reparametrize(self, active=None):
        """One launch; returns the status (0 = NFOPP_OK).  For D = 2 lam and cm are NULL."""
        d, P = self.dev, _lib.ptr
        mask = _dev(active, torch.uint8)                      # held until the launch has finished
        status = _lib.load().nfopp_reparametrize(self.B, self.N, self.D, P(d["traj"]), P(d["start"]), P(d["goal"]), P(d["lam"]),
                                                 P(d["cm"]), P(_grid(self.N)), P(mask, torch.uint8), _lib.stream_ptr())
        torch.cuda.synchronize()
        return status

    def update_endpoints(self, which, points):
        d, P = self.dev, _lib.ptr
        idx, pts = torch.full((self.B,), -7, dtype=torch.int32, device=DEV), _dev(points)
        _lib.check(_lib.load().nfopp_update_endpoints(self.B, self.N, self.D, which, P(pts), None, P(d["traj"]),
                                                      P(d["start"]), P(d["goal"]), P(d["lam"]), P(d["cm"]), P(_grid(self.N)),
                                                      P(idx, torch.int32), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return idx.cpu().numpy()

    def arrays(self):
        return {k: (None if v is None else v.cpu().numpy()) for k, v in self.dev.items()}


def _assert_same(got, want, what):
    assert rc.same(got, want), (what, "first difference (index, got, want, count):", rc.first_difference(got, want))


def _assert_row_is(got, b, want, what):
    for k in rc.OUTPUTS:
        if want[k] is not None:
            _assert_same(got[k][b], want[k], (what, k))


def _run_single(case):
    """The case alone (B = 1): dict(traj, lam, cm) the kernel left, after checking that it left start and goal alone."""
    one = Batch([case])
    assert one.reparametrize() == 0, _lib.load().nfopp_last_error()
    a = one.arrays()
    assert a["start"].tobytes() == case["start"].tobytes() and a["goal"].tobytes() == case["goal"].tobytes()
    return {k: (None if a[k] is None else a[k][0]) for k in rc.OUTPUTS}


# ---- every case, B = 1 ------------------------------------------------------------------------------------------------
CASES = rc.all_cases()


@pytest.mark.parametrize("d,n,kind", CASES, ids=[rc.case_name(*c) for c in CASES])
def test_kernel_reproduces_oracle_and_reference(d, n, kind):
    case = rc.make_case(d, n, kind)
    assert (case["lam"] is None) == (d == 2)
    got = _run_single(case)
    want = rc.oracle_outputs(d, n, kind, case)
    _, digests = rc.fixture_digests(d, n, kind)
    for k in rc.OUTPUTS:
        if want[k] is None:
            assert got[k] is None
            continue
        _assert_same(got[k], want[k], (kind, k))
        assert np.array_equal(rc.digest(got[k]), digests[k]), (kind, k)
    finite = [np.isfinite(v).all() for v in got.values() if v is not None]
    nan = [np.isnan(v).all() for v in got.values() if v is not None]
    assert all(nan) if kind in rc.NONFINITE_KINDS else all(finite)


# ---- the LDS limits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
def test_lds_limits(d):
    at, above, last = rc.SIZES[d][-3:]
    assert rc.lds_bytes(at, d) <= 64 * 1024 < rc.lds_bytes(above, d) and rc.lds_bytes(last, d) <= 160 * 1024
    for n in (at, above, last):
        one = Batch([rc.make_case(d, n, "zigzag")])
        assert one.reparametrize() == 0, (n, _lib.load().nfopp_last_error())
        _assert_row_is(one.arrays(), 0, rc.oracle_outputs(d, n, "zigzag"), n)
    n = rc.FIRST_REFUSED[d]
    assert n == last + 1 and rc.lds_bytes(n, d) > 160 * 1024
    case = rc.make_case(d, n, "zigzag")
    one = Batch([case])
    assert one.reparametrize() != 0                              # refused by the argument check: nothing is launched
    assert "trajectory too long" in _lib.load().nfopp_last_error().decode()
    after = one.arrays()
    for k in Batch.NAMES:
        assert case[k] is None or after[k][0].tobytes() == case[k].tobytes(), k


# ---- mixed batch, active mask -----------------------------------------------------------------------------------------
MIXED = ("zigzag", "tinyseg", "line", "nan", "allsame", "dups")     # both scans and non-finite rows, side by side


def _mixed(d, n):
    return [rc.make_case(d, n, kind) for kind in MIXED]


@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("n", [300, 513])
def test_mixed_batch_rows_equal_their_single_runs(d, n):
    cases = _mixed(d, n)
    assert [rc.takes_parallel_scan(c) for c in cases] == [True, False, True, False, False, True]
    full = Batch(cases)
    assert full.reparametrize() == 0
    got = full.arrays()
    for b, case in enumerate(cases):
        single = _run_single(case)
        want = rc.oracle_apply(case)
        for k in rc.OUTPUTS:
            if want[k] is not None:
                _assert_same(got[k][b], single[k], (MIXED[b], k, "batch vs single"))
                _assert_same(got[k][b], want[k], (MIXED[b], k, "batch vs oracle"))
        assert np.isnan(got["traj"][b]).all() == (MIXED[b] in rc.NONFINITE_KINDS)
    assert got["start"].tobytes() == full.host["start"].tobytes() and got["goal"].tobytes() == full.host["goal"].tobytes()


@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("n", [300, 513])
def test_active_mask(d, n):
    cases = _mixed(d, n)
    active = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    full, part = Batch(cases), Batch(cases)
    assert full.reparametrize() == 0 and part.reparametrize(active) == 0
    want, got = full.arrays(), part.arrays()
    for k in Batch.NAMES:
        if got[k] is None:
            continue
        for b in range(len(cases)):
            if active[b]:
                _assert_same(got[k][b], want[k][b], (k, b))
            else:
                assert got[k][b].tobytes() == part.host[k][b].tobytes(), (k, b)     # every bit, NaN payloads included


# ---- idempotence on the initialiser's line ----------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(d, n) for d in (3, 2) for n in rc.SIZES[d]], ids=lambda v: str(v))
def test_line_twice(d, n):
    case = rc.make_case(d, n, "line")
    one = Batch([case])
    assert one.reparametrize() == 0 and one.reparametrize() == 0
    first = rc.oracle_outputs(d, n, "line", case)
    again = rc.oracle_apply(dict(case, **{k: v for k, v in first.items() if v is not None}))
    _assert_row_is(one.arrays(), 0, again, n)
    # the line is arc-length parametrised already: nothing moves by more than rounding
    assert np.abs(again["traj"][:, :2] - case["traj"][:, :2]).max() < 1e-5


# ---- nfopp_update_endpoints at sizes that cross the sum and scan branches ----------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["start", "goal"])
@pytest.mark.parametrize("kind", ["zigzag", "dups"])
@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("n", [7, 300, 511, 700, 2337])
def test_update_endpoints_vs_oracle(n, d, kind, which):
    case = rc.make_case(d, n, kind)
    rng = np.random.default_rng([n, d, which])
    j = int(rng.integers(n // 4, n - n // 4))
    point = case["traj"][j].copy()
    point[:2] += rng.normal(0, 0.01, 2).astype(F32)
    if d == 3:
        point[2] = rng.uniform(-3.1, 3.1)
    want = er.update_endpoint(which, point, case["traj"], case["start"], case["goal"], case["lam"], case["cm"])
    one = Batch([case])
    idx = one.update_endpoints(which, point[None])
    got = one.arrays()
    assert int(idx[0]) == want["min_index"]
    for k in Batch.NAMES:
        if want[k] is not None:
            _assert_same(got[k][0], want[k], (k,))
    assert np.isfinite(got["traj"]).all()
