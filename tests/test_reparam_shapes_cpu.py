"""CPU: the oracle's reparametrisation against the reference's own output at every size and input kind of
tests/reparam_cases.py (tests/golden/g23_reparam_shapes.npz), without a tolerance -- it is the reference of
tests/test_gpu_reparam_shapes.py -- and that the cases still reach the branches of csrc/reparam.h they were built for."""
import numpy as np
import pytest
import torch

import reparam_cases as rc
from oracle import nfopp_oracle as orc

F32 = np.float32
DN = [(d, n) for d in (3, 2) for n in rc.SIZES[d]]
DN_IDS = ["d%d_n%d" % dn for dn in DN]


def test_the_fixture_holds_every_case():
    z = rc.fixture()
    assert [str(s) for s in z["names"]] == [rc.case_name(*c) for c in rc.all_cases()]
    assert z["in_digest"].shape == (len(z["names"]), 5, 32) and z["out_digest"].shape == (len(z["names"]), 3, 32)
    for d in (3, 2):
        for n in rc.SIZES[d]:
            assert (("d%d_n%d_traj" % (d, n)) in z) == (n <= rc.STORED_MAX_N)
    # -0.0 and a NaN's payload are outside the digest, a last bit is inside
    a = np.asarray([0.0, 1.0, np.nan], F32)
    b = np.asarray([-0.0, 1.0, -np.nan], F32)
    assert np.array_equal(rc.digest(a), rc.digest(b)) and rc.same(a, b)
    assert not np.array_equal(rc.digest(a), rc.digest(np.asarray([0.0, np.nextafter(F32(1), F32(2)), np.nan], F32)))


def test_sizes_sit_on_the_lds_boundaries():
    for d in (3, 2):
        at, above, last = rc.SIZES[d][-3:]
        assert rc.lds_bytes(at, d) <= 64 * 1024 < rc.lds_bytes(above, d) and above == at + 1   # D = 3: exactly 64 KB
        assert rc.lds_bytes(last, d) <= 160 * 1024 < rc.lds_bytes(last + 1, d) and rc.FIRST_REFUSED[d] == last + 1


@pytest.mark.parametrize("d,n", DN, ids=DN_IDS)
def test_inputs_are_the_ones_the_reference_saw(d, n):
    for kind in rc.kinds(d):
        case = rc.make_case(d, n, kind)
        want, _ = rc.fixture_digests(d, n, kind)
        for k in rc.INPUTS:
            assert np.array_equal(rc.digest(case[k]), want[k]), (kind, k)
            assert case[k] is None or (case[k].dtype == F32 and case[k].flags["C_CONTIGUOUS"])


@pytest.mark.parametrize("d,n", DN, ids=DN_IDS)
def test_oracle_reproduces_the_reference_exactly(d, n):
    for kind in rc.kinds(d):
        got = rc.oracle_outputs(d, n, kind)
        _, want = rc.fixture_digests(d, n, kind)
        arrays = rc.fixture_arrays(d, n, kind)
        for k in rc.OUTPUTS:
            if arrays is not None and arrays[k] is not None:
                assert np.array_equal(got[k], arrays[k], equal_nan=True), (kind, k, rc.first_difference(got[k], arrays[k]))
            assert np.array_equal(rc.digest(got[k]), want[k]), (kind, k)
        if kind in rc.NONFINITE_KINDS:
            assert all(np.isnan(v).all() for v in got.values() if v is not None), kind
        else:
            assert all(np.isfinite(v).all() for v in got.values() if v is not None), kind


@pytest.mark.parametrize("d,n", DN, ids=DN_IDS)
def test_cases_reach_the_scan_they_were_built_for(d, n):
    for kind in rc.kinds(d):
        case = rc.make_case(d, n, kind)
        sequential = kind in rc.SEQUENTIAL_KINDS and not (kind == "order" and n < 4)   # no room for its small steps there
        assert rc.takes_parallel_scan(case) == (not sequential), kind
    q, total = rc.quotients(rc.make_case(d, n, "tinyseg"))
    assert np.isfinite(total) and 0 < q[q != 0].min() < rc.TWO_POW_M29
    # `denormal`: the segment whose squared length is an fp32 denormal is the one that sends it to the sequential scan
    case = rc.make_case(d, n, "denormal")
    q, total = rc.quotients(case)
    mid = (n - 1) // 2
    dx = F32(case["traj"][mid + 1, 0] - case["traj"][mid, 0])
    assert 0 < F32(dx * dx) < np.finfo(F32).tiny and q[mid + 1] == q[q != 0].min() and 0 < q[mid + 1] < rc.TWO_POW_M29
    if n >= 6:
        assert case["traj"][1, 0] == F32(1e-37) and q[1] == 0            # its square underflows: a flat cdf step
    q, total = rc.quotients(rc.make_case(d, n, "allsame"))
    assert total == 0
    q, total = rc.quotients(rc.make_case(d, n, "overflow"))
    assert np.isinf(total)
    q, total = rc.quotients(rc.make_case(d, n, "nan"))
    assert np.isnan(total)
    q, total = rc.quotients(rc.make_case(d, n, "onemove"))
    assert total == 1 and np.array_equal(q, np.concatenate([np.zeros(n, F32), np.ones(1, F32)]))


@pytest.mark.parametrize("d,n", DN, ids=DN_IDS)
def test_parallel_scan_restatement_and_the_case_that_needs_the_sequential_one(d, n):
    for kind in rc.kinds(d):
        if kind in rc.SEQUENTIAL_KINDS:
            continue
        q, _ = rc.quotients(rc.make_case(d, n, kind))
        assert np.array_equal(rc.parallel_cdf(q), rc.sequential_cdf(q)), kind      # the exactness argument of csrc/reparam.h
    case = rc.make_case(d, n, "order")
    q, total = rc.quotients(case)
    assert total == 1 and q[0] == 0.5 and set(q[q != 0]) <= {F32(0.5), F32(2.0 ** -55), F32(2.0 ** -25), F32(0.5 - 2.0 ** -25)}
    if n >= 6:
        # were the parallel scan taken, the cdf -- and with it the output -- would differ: the 2^-29 threshold is load-bearing
        seq, par = rc.sequential_cdf(q), rc.parallel_cdf(q)
        k = int((q == F32(2.0 ** -55)).sum())
        assert k >= 4 and seq[k + 2] == 0.5 and par[k + 2] == np.nextafter(F32(0.5), F32(1)), (k, seq[k + 2], par[k + 2])
        hit, _, _ = _sampled_segments(case)
        assert k + 2 in hit                                      # the segment that starts at that cdf entry is sampled


def _sampled_segments(case):
    """Indices s of the segments (node s -> s + 1 of [start, waypoints, goal]) the grid interpolates on."""
    q, _ = rc.quotients(case)
    cdf = np.concatenate([np.zeros(1, F32), np.cumsum(q.astype(np.float64)).astype(F32)])
    n = len(case["traj"])
    idx = np.searchsorted(cdf, orc.linspace_f32(0, 1, n + 2)[1:-1], side="left")
    return set(int(i) - 1 for i in idx), cdf, idx


@pytest.mark.parametrize("n", rc.SIZES[3])
def test_turns_samples_its_special_heading_pairs(n):
    case = rc.make_case(3, n, "turns")
    hit, _, _ = _sampled_segments(case)
    th = case["traj"][:, 2]
    pairs = rc.turn_pair_waypoints(n)
    assert len(pairs) == (5 if n >= 14 else {2: 1, 3: 1, 6: 2, 7: 2, 8: 3}[n])
    for k, p in enumerate(pairs):
        assert p + 1 in hit, (k, p)                      # waypoint p is node p + 1: the segment between p and p + 1
        diff = F32(th[p + 1] - th[p])
        tag = rc.TURN_PAIRS[k]
        if tag == "pi":
            assert diff == orc.PI and orc.wrap_angle(diff) == -orc.PI
        elif tag == "equal":
            assert diff == 0
        elif tag == "minus_zero":
            assert np.signbit(th[p]) and not np.signbit(th[p + 1]) and diff == 0
        else:
            assert diff == (rc.TURN_NEG_15PI if tag == "neg_15pi" else rc.TURN_POS_5PI)
            # the quotient floor((a + pi) * (1 / 2 pi)) in fp32 is one above floor of the exact quotient
            x = F32(diff + orc.PI)
            assert np.floor(F32(x * F32(0.159154943))) == np.floor(np.float64(x) / np.float64(orc.TWO_PI)) + 1


@pytest.mark.parametrize("d", [3, 2])
def test_dups_clamp_and_line_reach_the_flat_runs_the_clamp_and_the_ties(d):
    for n in rc.SIZES[d]:
        _, cdf, idx = _sampled_segments(rc.make_case(d, n, "dups"))
        ia, ib = np.minimum(idx, n + 1), np.maximum(idx - 1, 0)
        den = (cdf[ia] - cdf[ib]).astype(F32)
        assert (np.diff(cdf) == 0).any() and (den > 0).all(), n               # flat runs of the cdf; no sample lands on one
        _, cdf, idx = _sampled_segments(rc.make_case(d, n, "clamp"))
        ia, ib = np.minimum(idx, n + 1), np.maximum(idx - 1, 0)
        den = (cdf[ia] - cdf[ib]).astype(F32)
        assert ((den > 0) & (den < F32(1e-5))).sum() == 1 and idx[n // 2] == max(1, n // 2) + 1, n   # the clamp is applied once
        # line: every segment has the same length up to rounding, so grid value w and cdf entry w + 1 are an ulp or so apart
        _, cdf, _ = _sampled_segments(rc.make_case(d, n, "line"))
        u = orc.linspace_f32(0, 1, n + 2)
        assert np.abs(cdf.astype(np.float64) - u).max() <= 8 * np.spacing(F32(1)), n


def test_linspace_restatement_at_every_size():
    for n in sorted(set(rc.SIZES[3] + rc.SIZES[2] + tuple(rc.FIRST_REFUSED.values()))):
        assert np.array_equal(orc.linspace_f32(0, 1, n + 2), torch.linspace(0, 1, n + 2).numpy()), n
    case = rc.make_case(3, 513, "line")
    for c in (0, 1):
        want = torch.linspace(float(case["start"][c]), float(case["goal"][c]), 515)[1:-1].numpy()
        assert np.array_equal(case["traj"][:, c], want)
