"""CPU: the oracle's path post-processor and trajectory initialisers against the reference's own outputs at the edges
(tests/golden/g22_path_tools.npz, written by tests/golden/make_golden_path_tools.py), and the properties that make each
case of that fixture prove something: the count-boundary cases really separate the summation orders, the threshold
cases really sit on the threshold.  tests/test_gpu_path_tools_edges.py holds the kernels to the same fixture."""
import numpy as np
import pytest

import path_tools_edges as pe
from conftest import max_abs
from oracle import nfopp_oracle as orc

F32 = np.float32


def test_fixture_holds_the_cases():
    names = set(pe.post_names())
    want = {"len_%d" % n for n in pe.LENGTHS} | {"park_%d" % k for k in pe.PARKED_SEGMENTS}
    want |= {"cb_%s_%d" % (s, n) for s in ("straight", "curved") for n in (130, 258, 1026)} | {"cb_levels_1026"}
    want |= {"small_%d%s" % (k, s) for k in (1, 2, 3) for s in ("lo", "hi")} | {"trim_%d" % k for k in (1, 2, 5, 6, 7)}
    want |= {"trim_backward", "trim_end", "filter_edge", "filter_edge_kept", "head_pi", "head_turns", "head_spin",
             "scale_8000", "degenerate", "degenerate_control", "collapse"}
    assert want <= names
    for n in pe.LENGTHS:
        assert len(pe.post_case("len_%d" % n)[0]) == n
    for k in pe.PARKED_SEGMENTS:
        path, md, _, _, _ = pe.post_case("park_%d" % k)
        assert len(pe.filtered_segment_lengths(path, md)) == k and len(path) == k + 12
    z = pe.fixture()
    assert tuple(z["init_sizes"]) == pe.INIT_SIZES and set(z["cb_names"]) == {n for n in names if n.startswith("cb_")}


def test_oracle_post_processor_vs_reference_and_spread():
    spread_xy = spread_th = 0.0
    for name in pe.post_names():
        path, md, step, want, err = pe.post_case(name)
        if err is not None:
            with pytest.raises(ValueError) as e:
                orc.path_postprocess(path, md, step)
            assert type(e.value).__name__ == err, name          # the class the reference raised
            continue
        got = orc.path_postprocess(path, md, step)
        assert got.shape == want.shape and got.dtype == np.float64, name
        if len(want):
            s = pe.scale_of(want)
            spread_xy = max(spread_xy, max_abs(got[:, :2], want[:, :2]) / s)
            spread_th = max(spread_th, max_abs(got[:, 2], want[:, 2]) / s)
    print("SPREAD xy %.3e heading %.3e" % (spread_xy, spread_th))
    assert spread_xy <= pe.SPREAD_XY and spread_th <= pe.SPREAD_TH
    assert pe.DEVICE_MARGIN * max(pe.SPREAD_XY, pe.SPREAD_TH) <= pe.REL_CAP      # the cap does not bind


def test_count_boundary_cases_separate_the_summation_orders():
    z = pe.fixture()
    for name, k in zip(z["cb_names"], z["cb_k"]):
        path, md, step, want, _ = pe.post_case(str(name))
        dist = pe.filtered_segment_lengths(path, md)
        assert len(dist) == len(path) - 1
        numpy_total = orc._pairwise_sum_f32(dist)
        assert numpy_total == np.sum(dist) == pe.pairwise_sum_f32_levels(dist, 4)
        other = pe.pairwise_sum_f32_levels(dist, 3) if "levels" in name else pe.running_sum_f32(dist)
        counts = pe.count_of(numpy_total, step), pe.count_of(other, step)
        assert set(counts) == {int(k) - 1, int(k)}, (name, counts)              # opposite sides of the integer k
        assert len(want) == counts[0] - 1 != counts[1] - 1, name                # the reference follows numpy's order


def test_filter_threshold_is_strict():
    path, md, step, want, _ = pe.post_case("filter_edge")
    kept, _, _, want_kept, _ = pe.post_case("filter_edge_kept")
    assert md == 0.5 and np.array_equal(want, want_kept)        # dropping the poses by hand changes nothing
    # walking back from the goal: distances to the pose kept last
    at, above, below = F32(0.5), np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(0.5), F32(0))
    seen, prev = [], path[-1]
    for i in range(len(path) - 2, 0, -1):
        d = np.sqrt(F32(F32(prev[0] - path[i, 0]) ** 2 + F32(prev[1] - path[i, 1]) ** 2))
        seen.append(d)
        if d > F32(md):
            prev = path[i]
    assert seen.count(at) == 4 and seen.count(above) == 4 and seen.count(below) == 1
    assert len(pe.filtered_segment_lengths(path, md)) + 1 == len(kept) == 7
    assert np.hypot(*(path[1, :2] - path[0, :2])) < md          # the first pose stays although the second is close


def test_small_counts_and_trim_rule():
    kept = [len(pe.post_case("small_%d%s" % (k, s))[3]) for k in (1, 2, 3) for s in ("lo", "hi")]
    assert kept == [0, 0, 0, 1, 1, 2]                           # counts 0, 1, 1, 2, 2, 3
    for k, trimmed in ((1, 1), (2, 2), (5, 5), (6, 1), (7, 1)):
        path, md, step, want, _ = pe.post_case("trim_%d" % k)
        count = pe.count_of(orc._pairwise_sum_f32(pe.filtered_segment_lengths(path, md)), step)
        assert count - len(want) == trimmed, k                  # `other < 6`: index 5 trims five poses, 6 and 7 one
    for name in ("trim_backward", "trim_end"):
        path, md, step, want, _ = pe.post_case(name)
        assert pe.count_of(orc._pairwise_sum_f32(pe.filtered_segment_lengths(path, md)), step) - len(want) == 1


def test_degenerate_parametrisation_case():
    for name, pos, stalls in (("degenerate", 58, True), ("degenerate_control", 2, False)):
        path, md, _, _, err = pe.post_case(name)
        assert md == 0.0 and np.array_equal(path[pos, 1:], path[pos + 1, 1:]) and path[pos + 1, 0] - path[pos, 0] > 0
        dist = pe.filtered_segment_lengths(path, md)
        assert len(dist) == len(path) - 1                       # nothing is filtered: the pose is 1e-7 m away
        cum = [F32(0)]
        for d in dist:
            cum.append(F32(cum[-1] + d))
        assert (cum[pos + 1] == cum[pos]) == stalls and (cum[pos] > 32) == stalls
        assert (err == "ValueError") == stalls


def test_heading_case_sits_on_pi():
    path = pe.post_case("head_pi")[0]
    w = orc.wrap_angle(path[:, 2])
    d = set((w[1:] - w[:-1]).astype(F32).tolist())
    pi = F32(np.pi)
    for t in (pi, np.nextafter(pi, F32(4)), np.nextafter(pi, F32(0))):
        assert float(t) in d and float(-t) in d
    assert np.abs(pe.post_case("head_turns")[0][:, 2]).max() > 6 * np.pi
    assert np.abs(pe.post_case("head_spin")[3][:, 2]).max() > 60


@pytest.mark.parametrize("n", pe.INIT_SIZES)
def test_oracle_initialisers_vs_reference(n):
    names, cases, plain, directed = pe.init_cases(n)
    assert len(names) == (30 if n in (1, 2, 3, 4, 5, 257) else 2)
    tol = pe.init_heading_tol(plain, directed)
    for c, case in enumerate(cases):
        assert np.array_equal(orc.initialize_trajectory(case[:3], case[3:], n), plain[c]), names[c]
        got = orc.initialize_trajectory_directed(case[:3], case[3:], n)
        assert np.array_equal(got[:, :2], plain[c][:, :2]), names[c]
        assert max_abs(got[:, 2], directed[c]) <= tol[c], (names[c], max_abs(got[:, 2], directed[c]), tol[c])


def test_initialiser_cases_sit_on_pi():
    z = pe.fixture()
    names, cases = [str(n) for n in z["init_case_names"]], z["init_cases"]
    pi = F32(np.pi)
    diff = {n: F32(c[5] - c[2]) for n, c in zip(names, cases)}
    assert diff["diff_pi"] == pi and diff["diff_mpi"] == -pi and diff["diff_pi_from_negative"] == pi
    assert diff["diff_pi_up"] == np.nextafter(pi, F32(4)) and diff["diff_pi_down"] == np.nextafter(pi, F32(0))
    assert diff["diff_mpi_up"] == -np.nextafter(pi, F32(0)) and diff["diff_mpi_down"] == -np.nextafter(pi, F32(4))
    # at exactly +-pi the reference turns through -pi: (pi + pi) % 2 pi = 0
    c = names.index("diff_pi")
    assert z["init_%d_n5" % c][-1, 2] < cases[c][2] and z["init_%d_n5" % names.index("diff_mpi")][-1, 2] < cases[c][2]
