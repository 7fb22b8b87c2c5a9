"""CPU: the start / goal update (nfopp_update_endpoints, csrc/endpoint_update.hip) without a GPU -- the fp32 numpy
statement of it (tests/endpoint_ref.py) against what the reference computed (tests/golden/g20_endpoint_updates.npz, made by
tests/golden/make_golden_endpoints.py, and g4_update_endpoints.npz), the power of those fixtures against six ways of
getting it wrong, torch's argmin order, the host-side argument checks of the C entry and the torch op's registration."""
import ctypes

import numpy as np
import pytest
import torch

import endpoint_ref as er
from conftest import load_golden

CASES = er.g20_cases(load_golden("g20_endpoint_updates.npz")) + er.g4_cases(load_golden("g4_update_endpoints.npz"))


def _run(case, **mutant):
    return er.update_endpoint(case["which"], case["point"], case["traj"], case["start"], case["goal"], case["lam"], case["cm"],
                              **mutant)


def test_fixture_holds_the_cases_the_feature_is_specified_on():
    z = load_golden("g20_endpoint_updates.npz")
    tags = {c["tag"] for c in er.g20_cases(z)}
    assert tags == {"se2_a", "se2_b", "se2_c", "se2_d", "se2_e", "se2_f", "se2_g", "se2_h1", "se2_h2",
                    "p2d_a", "p2d_b", "p2d_c", "p2d_d"}
    by = {c["tag"]: c for c in er.g20_cases(z)}
    n = by["se2_a"]["traj"].shape[0]
    assert by["se2_b"]["min_index"] == n and by["se2_b"]["which"] == 1      # capped: nothing overwritten
    assert by["se2_c"]["min_index"] == 1 and by["se2_e"]["min_index"] == n and by["se2_e"]["which"] == 0
    assert by["p2d_c"]["min_index"] == 0 and by["p2d_c"]["which"] == 0
    for tag in ("se2_f", "p2d_d"):                                         # the ties are exact in fp32, and only there
        c = by[tag]
        d = er.delta_unfused(c["traj"], c["point"])
        assert d[50] == d[51] == d.min() and np.sum(d == d.min()) == 2
        f = er.delta_fused(c["traj"], c["point"])
        assert f[51] < f[50]
    assert np.array_equal(by["se2_h2"]["traj"], by["se2_h1"]["out_traj"])   # goal update, then start update
    for c in by.values():
        assert not np.array_equal(c["start"] if c["which"] else c["point"], c["point"] if c["which"] else c["goal"])


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_helper_reproduces_the_reference(case):
    got = _run(case)
    bad, worst = er.mismatch(case, got)
    assert bad is None, bad
    assert np.array_equal(got["goal" if case["which"] else "start"], case["point"])


def test_argmin_follows_torch_on_ties_nan_and_inf():
    inf, nan = float("inf"), float("nan")
    rows = [[3, 1, 1, 2], [3, nan, 0, nan], [inf, inf, inf], [2, 2, 2, 2], [nan, nan], [5, -inf, -inf, nan], [1, 0, inf, 0],
            [inf, 4, inf]]
    assert er.argmin_torch([3, 1, 1, 2]) == 1 and er.argmin_torch([3, nan, 0, nan]) == 1 and er.argmin_torch([inf] * 3) == 0
    for row in rows:
        assert er.argmin_torch(row) == int(torch.argmin(torch.tensor(row, dtype=torch.float32))), row
    rng = np.random.default_rng(3)
    for _ in range(200):
        row = rng.integers(0, 4, rng.integers(1, 40)).astype(np.float32)
        row[rng.random(row.size) < 0.05] = nan
        assert er.argmin_torch(row) == int(torch.argmin(torch.tensor(row))), row


MUTANTS = {
    "no +1 for SE(2)": dict(plus_one=False),
    "+1 for 2-D": dict(plus_one=True),
    "last-index tie-break": dict(last_tie=True),
    "fma-contracted delta": dict(fused=True),
    "overwriting the other side": dict(other_side=True),
    "overwriting multipliers": dict(overwrite_multipliers=True),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_fixture_catches_the_mutant(name, capsys):
    g20 = er.g20_cases(load_golden("g20_endpoint_updates.npz"))
    caught = [c["tag"] for c in g20 if er.mismatch(c, _run(c, **MUTANTS[name]))[0] is not None]
    capsys.readouterr()
    assert caught, "no g20 case fails under the mutant '%s'" % name
    if name == "fma-contracted delta":
        assert "se2_f" in caught and "p2d_d" in caught      # the tie cases are what this mutant is for


# ---- the C entry's argument checks run before any HIP call: no GPU needed ---------------------------------------------
def _call(lib, batch=1, n=8, dim=3, which=0, points=4096, moved=None, traj=4096, start=4096, goal=4096, lam=4096, cm=4096,
          u=4096, min_index=None):
    P = ctypes.c_void_p
    return lib.nfopp_update_endpoints(batch, n, dim, which, P(points), P(moved), P(traj), P(start), P(goal), P(lam), P(cm), P(u),
                                      P(min_index), None)


def test_argument_checks_of_the_c_entry():
    from nfopp import _lib
    assert "nfopp_update_endpoints" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.nfopp_abi_version() == 6
    assert _call(lib, which=2) == -1 and b"which" in lib.nfopp_last_error()
    assert _call(lib, which=-1) == -1
    assert _call(lib, dim=4) == -1 and b"dim" in lib.nfopp_last_error()
    assert _call(lib, dim=1) == -1
    assert _call(lib, n=1) == -1 and b"waypoints" in lib.nfopp_last_error()
    assert _call(lib, batch=-1) == -1
    for name in ("points", "traj", "start", "goal", "u"):
        assert _call(lib, **{name: None}) == -1 and b"null" in lib.nfopp_last_error(), name
    assert _call(lib, lam=None) == -1 and b"multiplier" in lib.nfopp_last_error()
    assert _call(lib, cm=None) == -1
    assert _call(lib, n=20000) == -1 and b"LDS" in lib.nfopp_last_error()
    assert _call(lib, batch=0) == 0                       # nothing to do: no launch, no pointer is looked at
    assert _call(lib, batch=0, dim=2, points=None, traj=None, lam=None, cm=None) == 0


def test_torch_op_is_registered_and_refuses_cpu_tensors():
    from nfopp import torch_ops
    ops = torch_ops.load()
    assert "update_endpoints" in torch_ops.OPS and hasattr(ops, "update_endpoints")
    schema = str(torch.ops.nfopp.update_endpoints.default._schema)
    assert "Tensor(a!) traj" in schema and "int which" in schema
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.update_endpoints(z(1, 4, 3), z(1, 3), z(1, 3), z(1, 5), z(1, 4), z(4), z(1, 3), 0, None, None)
