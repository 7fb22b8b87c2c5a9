"""CPU: every case of tests/spline_bits_cases.py sits at the branch it claims -- the number of poses after the filter from the
oracle, the seeder's LDS | workspace boundary and the post-processor's 64 KiB crossing from the size formulas -- no seeder case
has two equal sites, and the 400-cell seed of DESIGN.md section 9 has: the arithmetic of the open case, not the device."""
import numpy as np
import pytest

import spline_bits_cases as sc
from oracle import nfopp_oracle as orc


def _kept(name):
    paths, md, _, _ = sc.POST_CASES[name]
    return [len(orc.filter_path(p, md)) for p in paths]


def test_post_cases_have_the_claimed_number_of_poses_after_the_filter():
    shapes = {name: sc.POST_CASES[name][0].shape[:2] for name in sc.POST_CASES}
    assert shapes == {"m3_unfiltered": (1, 3), "m2": (1, 3), "m3_filtered": (1, 4), "m4": (1, 4), "n5": (1, 5), "n130": (1, 130),
                      "n1026": (1, 1026), "duplicate": (1, 62), "mixed": (3, 12)}
    assert _kept("m3_unfiltered") == [3] and _kept("m2") == [2] and _kept("m3_filtered") == [3] and _kept("m4") == [4]
    assert _kept("n5") == [5] and _kept("n130") == [130] and _kept("n1026") == [1026] and _kept("duplicate") == [62]
    assert _kept("mixed") == [12, 10, 6]
    assert 130 - 1 > 128                                          # a second block of numpy's pairwise sum
    for p in sc.POST_CASES.values():
        assert p[0].dtype == np.float32 and p[0].flags.c_contiguous


def test_post_cases_without_a_spline_are_the_ones_the_oracle_refuses():
    for name in sc.POST_CASES:
        paths, md, step, max_out = sc.POST_CASES[name]
        for p in paths:
            if name in ("m2", "duplicate"):
                with pytest.raises(ValueError):
                    orc.path_postprocess(p, md, step)
            elif name != "n1026":                                  # (the oracle's loops over 1026 poses: not worth the time here)
                assert len(orc.path_postprocess(p, md, step)) <= max_out
    kept = orc.filter_path(sc.duplicate_sites_path(), 0.0)
    par, _ = sc.chord_parameter(kept[:, :2])
    assert len(kept) == 62 and par[59] == par[58] and np.count_nonzero(np.diff(par) == 0) == 1
    total = float(np.sum(np.linalg.norm(np.diff(sc.POST_CASES["n1026"][0][0, :, :2].astype(np.float64), axis=0), axis=1)))
    assert total / 0.25 + 2 < sc.POST_CASES["n1026"][3]            # every pose of the longest path fits its buffer


def test_the_longest_path_needs_more_than_64_kib_of_lds():
    assert sc.post_lds_bytes(1026) == 73896 > sc.LDS_LIMIT > sc.post_lds_bytes(130)
    assert sc.post_lds_bytes(909) <= sc.LDS_LIMIT < sc.post_lds_bytes(910)


def test_seed_sizes_sit_on_both_sides_of_the_workspace_boundary():
    assert sc.seed_workspace_doubles(1167) * 8 <= sc.LDS_LIMIT < sc.seed_workspace_doubles(1168) * 8
    assert sc.SEED_SIZES["lds"][0] == 1167 and sc.SEED_SIZES["ws"][0] == 1168
    for size in ("lds", "ws"):
        max_len, _, counts, status = sc.SEED_SIZES[size]
        assert counts[0] == max_len and status[0] == 0             # a row of full length
    max_len, _, counts, status = sc.SEED_SIZES["base"]
    assert {1, 2, max_len} <= set(counts) and max(counts) > max_len and 1 in status
    assert status[counts.index(max(counts))] == 0                  # the straight line for its count alone
    assert sorted(sc.SEED_SIZES[s][1] for s in ("n1", "n2", "n257")) == [1, 2, 257]


def test_seed_cases_reach_every_entry_heading_rule_and_size():
    cases = set(sc.SEED_CASES)
    assert len(cases) == len(sc.SEED_CASES) == len({sc.seed_tag(c) for c in cases})
    for size in sc.SEED_SIZES:
        assert {c[0] for c in cases if c[1] == size} == {"cells", "points", "lattice"}
    for entry in ("cells", "points"):
        assert {(c[2], c[3]) for c in cases if c[0] == entry and c[1] == "base"} == {(2, 0), (3, 0), (3, 1)}
    assert all(c[2] == 3 and c[3] == 0 for c in cases if c[0] == "lattice")


def test_lattice_heading_sequences_step_by_minus_one_zero_and_plus_one():
    for c in (c for c in sc.SEED_CASES if c[0] == "lattice"):
        s = sc.seed_inputs(c)
        max_len = sc.SEED_SIZES[c[1]][0]
        seen = set()
        for heads, cnt in zip(s["headings"], s["count"]):
            h = heads[:min(cnt, max_len)]
            assert ((h >= 0) & (h < 8)).all()
            seen |= set((((h[1:] - h[:-1] + 4) & 7) - 4).tolist())
        assert seen == {-1, 0, 1}, (c, seen)


@pytest.mark.parametrize("case", sc.SEED_CASES, ids=[sc.seed_tag(c) for c in sc.SEED_CASES])
def test_no_seeder_case_has_two_equal_sites(case):
    lines = sc.seed_polylines(case)
    s = sc.seed_inputs(case)
    assert len(lines) == sum(1 for c, st in zip(s["count"], s["status"]) if st == 0 and 1 <= c <= sc.SEED_SIZES[case[1]][0])
    assert sc.seed_sites_distinct(case)
    for p in lines:
        assert p.dtype == np.float32 and np.all(np.diff(sc.chord_parameter(p)[0]) > 0)


def test_a_400_cell_seed_ending_on_its_goal_cell_centre_has_two_equal_sites():
    """DESIGN.md section 9, open: the seeder does not look at this (the post-processor does, since its section 8 fix)"""
    p = sc.stalled_seed_polyline()
    assert p.shape == (402, 2) and np.array_equal(p[-1], p[-2])
    par, dist = sc.chord_parameter(p)
    assert dist[-1] == np.float32(1e-6) and float(np.sum(dist[:-1], dtype=np.float64)) > 32.0
    assert par[-1] == par[-2] == 1.0 and np.all(np.diff(par[:-1]) > 0)
