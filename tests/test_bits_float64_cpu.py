"""CPU: the words recorded in tests/golden/k1_bits.npz, k1_kind_bits.npz and k2_bits.npz are RIGHT -- every array that holds
values against a float64 restatement of the operation (tests/float64_ref.py), gated by 8 x the fp32 oracle's own error on
the same case and array (tests/bits_float64_gate.py).  tests/test_gpu_k1_bits.py, test_gpu_k1_kind_bits.py and
test_gpu_k2_bits.py assert that the device equals these files word for word; this module is what says the files may be
believed, so a re-recorded fixture has a correctness gate at exactly the shapes it exists for.

The gate has teeth: errors of the size a real bug has (a band tap off by 1e-3, two gradient rows swapped, Adam's step count
off by one, a hidden unit dropped, the sign of theta flipped) are planted into copies of the recorded arrays, and the same
comparer must reject each."""
import numpy as np
import pytest

from conftest import load_golden

import bits_float64_gate as bg
import float64_ref as f64
import k1_bits_cases as kc
import k1_kind_bits_cases as kk
import k2_bits_cases as k2

F32 = np.float32
K1 = {"k1_bits.npz": (kc, "k1_bits"), "k1_kind_bits.npz": (kk, "k1_kind")}
K2_IDS = [k2.tag(c) for c in k2.CASES]


@pytest.fixture(scope="module")
def k1():
    """{fixture name: (recorded arrays, reference)}: computed once, shared, never changed"""
    out = {}
    for name, (mod, _) in K1.items():
        z = load_golden(name)
        out[name] = (z, bg.k1_reference(mod, int(z["big_count"]) if "big_count" in z.files else None))
    return out


@pytest.fixture(scope="module")
def k2_ref():
    return {c: (bg.k2_reference(c), bg.k2_oracle32(c)) for c in k2.CASES}


def _recorded(case):
    z = load_golden("k2_bits.npz")
    return {k: z["%s_%s" % (k2.tag(case), k)] for k in k2.arrays_of(case)}


def _planted(recorded, want, wrong):
    """a copy of a recorded array with the error (wrong - want) of the float64 values planted into it"""
    return (np.asarray(recorded, np.float64) + (wrong - want).reshape(np.shape(recorded))).astype(F32)


def _report(rows):
    print("\n".join(bg.summary(rows)))
    print("worst ratio %.2f" % bg.worst_ratio(rows))


# ----------------------------------------------------------------------------------------------------------
# K1
@pytest.mark.parametrize("fin", sorted(kc.DIMS))
@pytest.mark.parametrize("name", sorted(K1))
def test_networks_are_the_recorded_ones(name, fin):
    """the precondition of everything below: the CPU build of the network under the case module's seed is the recorded one"""
    flat, _ = bg.cpu_network(fin)
    want = int(load_golden(name)["params_sum_F%d" % fin])
    assert int(kc.wsum(flat)) == want, \
        "ONF(use_normal_init=True) under torch seed %d no longer draws the parameters %s was recorded with: the initialiser " \
        "drifted (F = %d), every comparison below is void until the fixture is re-recorded" % (1000 + fin, name, fin)


@pytest.mark.parametrize("name", sorted(K1))
def test_k1_fixture_against_float64(name, k1):
    z, ref = k1[name]
    rows = bg.compare_k1(K1[name][1], z, ref)
    _report(rows)
    assert not bg.failures(rows), bg.failures(rows)
    assert bg.worst_ratio(rows) <= bg.FACTOR


@pytest.mark.parametrize("name", sorted(K1))
def test_no_recorded_value_is_left_out(name, k1):
    """every array of the fixture but the uint32 word sums, the parameter sums and the stored count is compared"""
    z, ref = k1[name]
    seen = set()
    for case, r in ref.items():
        if r["kind"] == "fit":
            seen |= {"%s_%s%s" % (case, k, "" if len(r["x"]) == 33 else "_rows") for k in ("h1", "dh1", "de", "rec")}
        else:
            seen.add(case)
    skipped = {n for n in z.files if n.startswith("params_sum_") or n.endswith(("_rowsum", "_colsum")) or n in ("big_sum", "big_count")}
    assert seen | skipped == set(z.files) and not (seen & skipped)
    assert all(z[n].dtype == np.float32 for n in seen)


@pytest.mark.parametrize("name", sorted(K1))
def test_rows_left_out_at_relu_kinks_stay_within_their_caps(name, k1):
    """from the float64 reference alone: at most 0.5 % of a case's rows are left out of the gradient and factor comparisons,
    none of an edge case, and only rows within KINK of a kink"""
    _, ref = k1[name]
    below = total = 0
    for case, r in ref.items():
        keep = bg.kink_free(r)
        out = int((~keep).sum())
        assert out <= bg.KINK_ROWS * len(keep), (case, out, len(keep))
        assert out == 0 or r["kind"] != "edge", case
        assert np.all(r["kink"][~keep] < f64.KINK), case
        below += int((r["kink"] < f64.KINK).sum())
        total += len(keep)
    print("%s: %d of %d rows are within %g of a kink" % (name, below, total, f64.KINK))
    edges = [r for r in ref.values() if r["kind"] == "edge"]
    assert (name == "k1_kind_bits.npz") == bool(edges) and all(bg.kink_free(r).all() for r in edges)


def test_k1_gates_are_no_looser_than_the_parity_tests(k1):
    for name, (z, ref) in k1.items():
        for r in bg.compare_k1(K1[name][1], z, ref):
            if r.array in ("logit", "grad"):
                assert r.bound <= bg.PARITY[r.array] * r.scale, r


def _unit_to_drop(c, row):
    """the active second-layer unit of that row whose contribution to the logit is the median one"""
    contrib = np.abs(c["h2"][row] * c["p"]["w3"].reshape(-1)[:100])
    active = np.nonzero(contrib > 0)[0]
    return int(active[np.argsort(contrib[active])[len(active) // 2]])


@pytest.mark.parametrize("name,case,row", [("k1_bits.npz", "pose_F220_P257", 130), ("k1_bits.npz", "pose_F100_P33", 32),
                                           ("k1_bits.npz", "traj_F120", 7), ("k1_kind_bits.npz", "pose_F200_P65", 64),
                                           ("k1_bits.npz", "logits_F200", 256)])
def test_planted_dropped_hidden_unit_is_rejected(name, case, row, k1):
    z, ref = k1[name]
    mod, tag = K1[name]
    j = _unit_to_drop(ref[case]["c"], row)
    wrong = bg.k1_reference(mod, plant=(case, dict(drop_unit=(row, j))), only=(case,))[case]
    bad = dict(z)
    out = np.array(z[case], np.float64)
    flat = out.reshape(-1, 4)
    flat[:, 0] += wrong["logit"] - ref[case]["logit"]
    if ref[case]["kind"] != "logits":
        d = wrong["grad"].shape[1]
        flat[:, 1:1 + d] += wrong["grad"] - ref[case]["grad"]
    bad[case] = out.astype(F32)
    assert int((bad[case] != z[case]).any(-1).sum()) == 1                  # one row carries the error
    rows = bg.compare_k1(tag, bad, ref, only=(case,))
    assert any(not r.ok and r.array == "logit" for r in rows), rows
    assert not bg.failures(bg.compare_k1(tag, z, ref, only=(case,)))       # and the recorded array itself passes


@pytest.mark.parametrize("row", [0, 1, 6, 7])      # theta = -1.3 and 2.1, each at a random place and at u = 0 (the angle features
                                                   # have period 2 pi: at +-pi a flipped sign changes nothing)
def test_planted_sign_of_theta_is_rejected(row, k1):
    z, ref = k1["k1_kind_bits.npz"]
    case = "edge_F220"
    assert ref[case]["x"][row, 2] != 0
    wrong = bg.k1_reference(kk, plant=(case, "theta", row), only=(case,))[case]
    bad = dict(z)
    out = np.array(z[case], np.float64)
    out[:, 0] += wrong["logit"] - ref[case]["logit"]
    out[:, 1:4] += wrong["grad"] - ref[case]["grad"]
    bad[case] = out.astype(F32)
    rows = bg.compare_k1("k1_kind", bad, ref, only=(case,))
    assert any(not r.ok for r in rows), rows


def test_planted_error_in_a_fit_factor_is_rejected(k1):
    """the factor arrays: one hidden unit's rho * dh1 zeroed in one row, and a pad position of de written"""
    z, ref = k1["k1_kind_bits.npz"]
    case = "fit_F120_P33"
    bad = dict(z)
    a = z[case + "_dh1"].copy()
    live = np.nonzero(a[17, :100])[0]
    j = int(live[np.argsort(np.abs(a[17, live]))[len(live) // 2]])
    a[17, j] = 0
    bad[case + "_dh1"] = a
    rows = bg.compare_k1("k1_kind", bad, ref, only=(case,))
    assert [r.array for r in rows if not r.ok] == ["rho_dh1"]
    bad = dict(z)
    a = z[case + "_de"].copy()
    a[5, 127] = F32(1e-30)
    bad[case + "_de"] = a
    assert [r.array for r in bg.compare_k1("k1_kind", bad, ref, only=(case,)) if not r.ok] == ["pad positions of de are zero"]


# ----------------------------------------------------------------------------------------------------------
# K2
@pytest.mark.parametrize("case", k2.CASES, ids=K2_IDS)
def test_k2_fixture_against_float64(case, k2_ref):
    want, o32 = k2_ref[case]
    rows = bg.compare_k2("k2_bits", case, _recorded(case), want, o32)
    _report(rows)
    assert len(rows) == len(k2.arrays_of(case)) - 1 + len(f64.TERMS)        # every array, every term
    assert not bg.failures(rows), bg.failures(rows)
    assert bg.worst_ratio(rows) <= bg.FACTOR


def test_k2_gates_are_no_looser_than_the_parity_tests(k2_ref):
    """at the parity tests' own conditions (default hyper block, coordinates within 3.1) the caps are the parity gates"""
    assert bg.PARITY["traj"] * max(1.0, 3.0 / bg.PARITY_TRAJ_SCALE) * max(1.0, 1e-2 / bg.PARITY_LR) == 2e-6
    for case in k2.CASES:
        want, o32 = k2_ref[case]
        for r in bg.compare_k2("k2_bits", case, _recorded(case), want, o32, names=("traj", "adam_m", "adam_v")):
            assert r.bound <= bg.k2_cap(r.array, r.scale), r


def _reject(case, k2_ref, wrong, must_fail):
    want, o32 = k2_ref[case]
    rec = _recorded(case)
    bad = {k: _planted(rec[k], want[k], wrong[k]) for k in rec}
    failed = {r.array for r in bg.compare_k2("k2_bits", case, bad, want, o32) if not r.ok}
    assert must_fail <= failed, (case, failed)
    return bad, rec


@pytest.mark.parametrize("case,column,tap", [((256, 0.5, 3), 3, 0), ((256, 0.5, 3), 250, -2), ((122, 0.5, 3), 0, 1), ((121, 0.5, 3), 60, 0),
                                             ((256, 2, 3), 10, 3), ((100, 0.5, 2), 99, -1), ((2, 0.5, 3), 1, 0)])
def test_planted_band_tap_is_rejected(case, column, tap, k2_ref):
    """one tap (offset `tap` from the diagonal) of one boundary column 1 + 1e-3 too large"""
    band, W, (lo, hi) = k2.band(case[0], case[1])
    assert not lo <= column < hi
    band = band.copy()
    band[W + tap, column] *= F32(1 + 1e-3)
    bad, rec = _reject(case, k2_ref, bg.k2_reference(case, band=band), {"adam_m", "adam_v"})      # (Adam's quotient hides it in traj)
    assert int((bad["adam_m"] != rec["adam_m"]).any(-1).sum()) == k2.B      # one waypoint per trajectory carries it


@pytest.mark.parametrize("case,b,w", [((122, 0.5, 3), 1, 60), ((257, 0.5, 3), 2, 255), ((9, 0.5, 3), 0, 0), ((256, 0.5, 2), 1, 28)])
def test_planted_swap_of_two_gradient_rows_is_rejected(case, b, w, k2_ref):
    _reject(case, k2_ref, bg.k2_reference(case, swap_grad_rows=(b, w)), {"traj", "adam_m", "adam_v"})


@pytest.mark.parametrize("case", k2.CASES, ids=K2_IDS)
@pytest.mark.parametrize("off", [-1, 1])
def test_planted_adam_step_off_by_one_is_rejected(case, off, k2_ref):
    """the count TrajectoryHyper.to_c takes is 1-based; one off moves traj by 1e-3 to 4e-2"""
    wrong = bg.k2_reference(case, adam_step=k2.ADAM_STEP + off)
    moved = float(np.abs(wrong["traj"] - k2_ref[case][0]["traj"]).max())
    assert 1e-4 < moved < 1e-1, moved
    bad, rec = _reject(case, k2_ref, wrong, {"traj"})
    assert np.array_equal(bad["adam_m"], rec["adam_m"]) and np.array_equal(bad["adam_v"], rec["adam_v"])


def test_planted_errors_in_multipliers_and_terms_are_rejected(k2_ref):
    """the arrays the planted errors above do not reach: lambda ascent without its rate, the collision multipliers at twice theirs, a term left out
    of the total"""
    case = (122, 0.5, 3)
    want, o32 = k2_ref[case]
    rec, s = _recorded(case), k2.inputs(case)
    for k, wrong in (("lam", s["lam"].astype(np.float64) + (want["lam"] - s["lam"]) / k2.HYPER.multipliers_lr),
                     ("cm", s["cm"].astype(np.float64) + 2 * (want["cm"] - s["cm"])),
                     ("terms", want["terms"] - np.eye(8)[0] * k2.HYPER.direction_delta_weight * want["terms"][:, 7:8])):
        assert np.any(wrong != want[k])
        bad = dict(rec)
        bad[k] = _planted(rec[k], want[k], wrong)
        failed = [r for r in bg.compare_k2("k2_bits", case, bad, want, o32) if not r.ok]
        assert failed and all(r.array == (k if k != "terms" else "total") for r in failed), (k, failed)
