"""CPU: the rule of nfopp_fleet_shift_masks / nfopp_fleet_assign_delays as restated in tests/fleet_schedule_ref.py -- hand cases
with exact expected delays, properties over the case families (tests/fleet_schedule_cases.py), coverage of the case set computed
from the restatement -- and the interface: header, binding and library agree, every argument check answers without a GPU, the
Python names and their shape checks exist."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import nfopp
from nfopp import _lib, torch_ops
from nfopp import schedule as ns

import fleet_schedule_cases as fc
import fleet_schedule_ref as fr
import track_conflict_ref as tr

F32 = np.float32
INF = np.inf


# ---- hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.hand_cases()))
def test_hand_cases_have_their_exact_delays(name):
    c = fc.hand_cases()[name]
    m, s = fc.solve(c)
    e = c["expect"]
    assert s["delay"].tolist() == e["delay"] and s["status"].tolist() == e["status"], (name, s)
    assert [int(x) for x in s["forbidden"]] == e["forbidden"], (name, s["forbidden"])
    if "base" in e:
        assert [int(x) for x in m["base"]] == e["base"]


def test_the_crossing_needs_two_steps_and_the_junction_too():
    for name in ("right_angle", "head_on_junction"):
        c = fc.hand_cases()[name]
        bits = fr.pair_bits(c["tracks"], c["max_delay"], c["radius"])[1, 0]     # robot 1 delayed by r against robot 0
        md = c["max_delay"]
        assert bits[md] and bits[md + 1] and not bits[md + 2], name


def test_max_delay_zero_is_the_conflict_check():
    for c in (fc.circle(16, 18, 0), fc.crowded(12, 10, 0, seed=3)):
        m = fr.shift_masks(c["tracks"], **fc.kwargs(c))
        want = tr.conflicts(c["tracks"], None, dt=1.0, radius_a=c["radius"], margin=c["margin"])
        assert np.array_equal(m["pair_bits"][:, :, 0], want["pair_first"] < INF)
        assert (m["pair"][:, :, 1] == 0).all() and (m["pair"][:, :, 0] <= 1).all()
        s = fr.assign(m)
        assert set(s["delay"].tolist()) <= {0, -1} and (s["delay"] == -1).any()


def test_lanes_at_exactly_r_set_no_bit_and_one_fp32_step_closer_sets_every_bit():
    m, _ = fc.solve(fc.lanes(False))
    assert not m["pair_bits"].any()
    m, _ = fc.solve(fc.lanes(True))
    assert m["pair_bits"][0, 1].all() and m["pair_bits"][1, 0].all() and not m["pair_bits"][0, 0].any()
    assert [int(x) for x in m["pair"][0, 1]] == [2 ** 64 - 1, 2 ** 63 - 1]         # 127 bits, the unused one clear


def test_pack_and_unpack_are_little_endian_words():
    bits = np.zeros((2, 127), bool)
    bits[0, [0, 63, 64, 126]] = True
    w = fr.pack(bits)
    assert w.dtype == np.uint64 and [int(x) for x in w[0]] == [1 | 1 << 63, 1 | 1 << 62] and not w[1].any()
    assert np.array_equal(fr.unpack(w, 127), bits)


def test_delay_tracks_waits_at_the_first_sample_and_parks_at_the_last():
    t = np.arange(10, dtype=F32).reshape(2, 5, 1) * np.ones((1, 1, 3), F32)
    got = fr.delay_tracks(t, [0, 2], 8)
    assert got[0, :, 0].tolist() == [0, 1, 2, 3, 4, 4, 4, 4] and got[1, :, 0].tolist() == [5, 5, 5, 6, 7, 8, 9, 9]
    dev = ns.delay_tracks(torch.from_numpy(t), torch.tensor([0, 2]), 8)
    assert np.array_equal(dev.numpy(), got) and dev.is_contiguous()
    assert np.array_equal(ns.delay_tracks(torch.from_numpy(t), torch.tensor([-1, 2], dtype=torch.int32), 8).numpy(), got)
    with pytest.raises(ValueError, match=r"\[B\]"):
        ns.delay_tracks(torch.from_numpy(t), torch.tensor([1, 2, 3]), 8)


# ---- properties over the families ------------------------------------------------------------------------------------------
def _families():
    yield "circle", fc.circle(16, 18, 31)
    yield "circle_short", fc.circle(16, 18, 7)
    yield "crowded", fc.crowded(24, 20, 15, seed=1)
    yield "circle_obstacles", fc.crossing_obstacles(fc.circle(16, 18, 31), 5, seed=2)
    yield "sized_33", dict(fc.sized_case(33, 33, 32, m=33, stride=3), order=fc.orders(33)["odd"])
    for name, c in sorted(fc.hand_cases().items()):
        yield name, c


@pytest.fixture(scope="module")
def solved():
    return [(name, c) + fc.solve(c) for name, c in _families()]


def test_mask_ji_is_the_bit_reversal_of_mask_ij(solved):
    for name, c, m, s in solved:
        pb = m["pair_bits"]
        assert np.array_equal(pb.transpose(1, 0, 2), pb[:, :, ::-1]), name
        assert np.array_equal(fr.unpack(m["pair"], pb.shape[2]), pb) and not fr.unpack(m["pair"], 128)[..., pb.shape[2]:].any()
        assert not pb[np.arange(len(pb)), np.arange(len(pb))].any(), name
        bad = m["bad"].astype(bool)
        assert not pb[bad].any() and not pb[:, bad].any() and not m["base_bits"][bad].any()


def test_the_predicate_on_the_delayed_tracks_agrees_and_no_scheduled_robot_conflicts(solved):
    seen = 0
    for name, c, m, s in solved:
        md, K = c["max_delay"], c["tracks"].shape[1]
        on = np.flatnonzero(s["status"] == 0)
        if len(on) < 1:
            continue
        moved = fr.delay_tracks(c["tracks"], np.maximum(s["delay"], 0), K + md)
        p = tr.pairs(moved[on], None, dt=1.0, radius_a=c["radius"][on], margin=c["margin"])
        hit = (p["tc"] < INF) & p["partner"]
        rel = s["delay"][on][:, None] - s["delay"][on][None, :] + md
        want = m["pair_bits"][on[:, None], on[None, :], rel]
        assert np.array_equal(hit, want), name                               # the relative-shift bit is the absolute-time answer
        assert not hit.any(), name                                           # and the schedule is clear
        seen += int(len(on) >= 2)
        if c["obstacles"] is not None:
            q = tr.pairs(moved[on], c["obstacles"], dt=1.0, radius_a=c["radius"][on], radius_b=c["obstacle_radius"], margin=c["margin"])
            assert not ((q["tc"] < INF) & q["partner"]).any(), name
    assert seen >= 6


def test_delays_are_minimal_and_unresolved_robots_have_every_bit_set(solved):
    for name, c, m, s in solved:
        D = c["max_delay"] + 1
        f = fr.unpack(np.stack([s["forbidden"], np.zeros_like(s["forbidden"])], -1), D)
        for i in range(len(s["delay"])):
            if s["status"][i] == 0:
                assert f[i, :s["delay"][i]].all() and not f[i, s["delay"][i]], (name, i)
            elif s["status"][i] == fr.STATUS_UNRESOLVED:
                assert f[i].all() and s["delay"][i] == -1, (name, i)
            else:
                assert not f[i].any() and s["delay"][i] == -1, (name, i)
        assert (s["forbidden"] >> np.uint64(D) == 0).all() if D < 64 else True


def test_an_unresolved_robot_is_not_on_the_floor_for_those_after_it():
    """Three parked robots in a row, 0.5 m apart, R = 1: the middle one overlaps both ends, the ends touch at exactly R."""
    c = fc.case([[(0, 0)], [(0.5, 0)], [(1, 0)]], 3)
    m = fr.shift_masks(c["tracks"], **fc.kwargs(c))
    s = fr.assign(m)
    assert s["delay"].tolist() == [0, -1, 0] and s["status"].tolist() == [0, fr.STATUS_UNRESOLVED, 0]      # 2 does not see 1
    s = fr.assign(m, np.array([1, 0, 2], np.int32))
    assert s["delay"].tolist() == [-1, 0, -1] and s["status"].tolist() == [fr.STATUS_UNRESOLVED, 0, fr.STATUS_UNRESOLVED]


def test_reordering_is_relabelling(solved):
    """A permutation as priority order gives what the identity order gives on the permuted fleet; repeats and entries out of
    range are skipped, and a robot that never occurs is NOT_ORDERED and invisible."""
    for name, c, m, s in solved:
        b = len(c["tracks"])
        if b < 4 or c["obstacles"] is not None and name != "circle_obstacles":
            continue
        o = fc.orders(b, seed=len(name))
        got = fr.assign(m, o["permutation"])
        perm = o["permutation"]
        moved = dict(c, tracks=c["tracks"][perm], radius=c["radius"][perm], order=None)
        _, want = fc.solve(moved)
        for key in ("delay", "status", "forbidden"):
            assert np.array_equal(got[key][perm], want[key]), (name, key)
        odd = fr.assign(m, o["odd"])
        visited = [i for n, i in enumerate(o["odd"]) if 0 <= i < b and i not in o["odd"][:n].tolist()]
        missing = sorted(set(range(b)) - set(visited))
        assert len(missing) >= 2 and (odd["status"][missing] == fr.STATUS_NOT_ORDERED).all() and (odd["delay"][missing] == -1).all()
        keep = np.array(visited)
        sub = dict(c, tracks=c["tracks"][keep], radius=c["radius"][keep], order=None)
        _, want = fc.solve(sub)
        for key in ("delay", "status", "forbidden"):
            assert np.array_equal(odd[key][keep], want[key]), (name, key)


def test_strides_and_junk_past_y_change_nothing():
    base = fc.sized_case(9, 7, 5, m=3, stride=2)
    want_m, want_s = fc.solve(base)
    for stride in (3, 4):
        c = fc.sized_case(9, 7, 5, m=3, stride=stride)
        assert c["tracks"].shape[2] == stride and np.isnan(c["tracks"][:, :, 2]).any()
        m, s = fc.solve(c)
        assert np.array_equal(m["pair"], want_m["pair"]) and np.array_equal(m["base"], want_m["base"])
        assert np.array_equal(s["delay"], want_s["delay"])


# ---- coverage, computed from the restatement -------------------------------------------------------------------------------
def test_case_set_covers_what_it_claims(solved):
    by = {name: (c, m, s) for name, c, m, s in solved}
    c, m, s = by["circle"]
    assert m["pair_bits"][:, :, c["max_delay"]].any(axis=1).all()            # every robot is in conflict when all leave together
    assert (s["status"] == 0).all() and (s["delay"] > 0).sum() >= 8          # delays resolve it; at least half wait
    assert (by["circle_short"][2]["status"] == fr.STATUS_UNRESOLVED).sum() >= 1
    crowded = by["crowded"][2]["status"]
    assert (crowded == fr.STATUS_UNRESOLVED).sum() * 2 > len(crowded)        # why it is not the main family
    statuses = set()
    both_words = base_some = False
    for name, c, m, s in solved:
        statuses |= set(s["status"].tolist())
        both_words |= bool(((m["pair"][:, :, 0] != 0) & (m["pair"][:, :, 1] != 0)).any())
        D = c["max_delay"] + 1
        full = np.uint64(2 ** D - 1)
        base_some |= bool(((m["base"] != 0) & (m["base"] != full)).any())
    assert statuses == {0, fr.STATUS_BAD_TRACK, fr.STATUS_UNRESOLVED, fr.STATUS_NOT_ORDERED}
    assert both_words and base_some
    # a shift whose only conflict is in the last-instant term: K = 1 at r = 0 (with an interval in front of it, the interval
    # that ends there reports the same value first)
    c = fc.hand_cases()["single_instant"]
    p = tr.pairs(c["tracks"], c["tracks"], dt=1.0, radius_a=c["radius"], radius_b=c["radius"], margin=c["margin"])
    assert p["branches"]["last_term_only"] > 0 and by["single_instant"][1]["pair_bits"][0, 1, c["max_delay"]]


# ---- interface -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    lib = nfopp.load_library()
    header = open(os.path.join(ROOT, "include", "nfopp_hip.h")).read()
    for name, n_args, res, ctype in (("nfopp_fleet_shift_masks", 17, "int", ctypes.c_int),
                                     ("nfopp_fleet_assign_delays", 10, "int", ctypes.c_int),
                                     ("nfopp_fleet_shift_masks_workspace_bytes", 2, "size_t", ctypes.c_size_t)):
        decl = re.search(r"\b%s %s\(([^;]*)\);" % (res, name), header)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == n_args and _lib._SIGNATURES[name][0] is ctype
    assert lib.nfopp_abi_version() == 6 and "#define NFOPP_ABI_VERSION 6" in header
    for name, value in (("MAX_DELAY", 63), ("BAD_TRACK", fr.STATUS_BAD_TRACK), ("UNRESOLVED", fr.STATUS_UNRESOLVED),
                        ("NOT_ORDERED", fr.STATUS_NOT_ORDERED)):
        assert "#define NFOPP_SCHEDULE_%s %d" % (name, value) in header, name
        assert getattr(nfopp, "SCHEDULE_" + name) == value
    assert fr.MAX_DELAY_LIMIT == _lib.SCHEDULE_MAX_DELAY == 63
    assert "fleet_schedule.hip" in open(os.path.join(ROOT, "pytorch-motion-planner_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "pytorch-motion-planner_amd", "csrc", "fleet_schedule.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include", 1)[1]
    for word in ("relative shift", "independent of any horizon", "lowest clear bit", "bits reversed"):
        assert word in header, word


def _masks_rc(b=3, stride=2, k=4, margin=0.0, max_delay=3, m=0, obstacle_stride=2, tracks=1, obstacles=0, pair=1, base=1, bad=1,
              workspace=0, workspace_bytes=0):
    P = lambda v: ctypes.c_void_p(v) if v else None
    return nfopp.load_library().nfopp_fleet_shift_masks(P(tracks), b, stride, k, None, margin, max_delay, P(obstacles), m, obstacle_stride,
                                                        None, P(pair), P(base), P(bad), P(workspace), workspace_bytes, None)


def _assign_rc(b=3, max_delay=3, pair=1, base=1, bad=1, delay=1, status=1):
    P = lambda v: ctypes.c_void_p(v) if v else None
    return nfopp.load_library().nfopp_fleet_assign_delays(P(pair), P(base), P(bad), None, b, max_delay, P(delay), P(status), None, None)


def test_every_argument_check_answers_without_a_gpu():
    lib = nfopp.load_library()

    def refused(rc, word):
        assert rc == -1, word
        assert word in lib.nfopp_last_error().decode(), (word, lib.nfopp_last_error())

    refused(_masks_rc(b=-1), "batch")
    refused(_masks_rc(b=2 ** 31), "batch")
    refused(_masks_rc(m=-1, obstacles=1), "batch")
    for md in (-1, 64):
        refused(_masks_rc(max_delay=md), "max_delay")
        refused(_assign_rc(max_delay=md), "max_delay")
    refused(_masks_rc(k=0), "k >= 1")
    refused(_masks_rc(k=2 ** 31 - 1), "too many instants")
    refused(_masks_rc(stride=1), "stride")
    refused(_masks_rc(m=2, obstacles=1, obstacle_stride=1, workspace=1, workspace_bytes=1 << 20), "stride")
    for margin in (np.nan, np.inf, -np.inf):
        refused(_masks_rc(margin=margin), "margin")
    for null in ("tracks", "pair", "base", "bad"):
        refused(_masks_rc(**{null: 0}), "null device pointer")
    assert _masks_rc(b=0, tracks=0, pair=0, base=0, bad=0) == 0                       # nothing to do
    refused(_masks_rc(b=2 ** 31 - 1), "too many")                                     # more tiles than a grid holds
    refused(_masks_rc(b=2 ** 20, m=2 ** 20, obstacles=1, workspace=1, workspace_bytes=2 ** 62), "too many")
    # the workspace: [b, tiles of 8 obstacles] words and one flag per obstacle; none without obstacles
    assert lib.nfopp_fleet_shift_masks_workspace_bytes(5, 0) == 0 == lib.nfopp_fleet_shift_masks_workspace_bytes(0, 5)
    for b, m in ((3, 2), (9, 8), (9, 9), (1, 17)):
        need = lib.nfopp_fleet_shift_masks_workspace_bytes(b, m)
        assert need >= b * -(-m // 8) * 8 + 4 * m
        refused(_masks_rc(b=b, m=m, obstacles=1, workspace=1, workspace_bytes=need - 1), "workspace")
        refused(_masks_rc(b=b, m=m, obstacles=1, workspace=0, workspace_bytes=need), "workspace")
    refused(_assign_rc(b=-1), "batch")
    refused(_assign_rc(b=2 ** 31), "batch")
    for null in ("pair", "base", "bad", "delay", "status"):
        refused(_assign_rc(**{null: 0}), "null device pointer")
    assert _assign_rc(b=0, pair=0, base=0, bad=0, delay=0, status=0) == 0
    refused(_assign_rc(b=160 * 1024), "too many robots")                              # a byte of LDS each, in one workgroup


def test_python_names_and_signatures():
    for name in ("FleetMasks", "FleetSchedule", "fleet_shift_masks", "schedule_delays", "delay_tracks", "SCHEDULE_OK",
                 "SCHEDULE_BAD_TRACK", "SCHEDULE_UNRESOLVED", "SCHEDULE_NOT_ORDERED", "SCHEDULE_MAX_DELAY"):
        assert hasattr(nfopp, name) and name in nfopp.__all__, name
    assert (nfopp.FleetSchedule.OK, nfopp.FleetSchedule.BAD_TRACK, nfopp.FleetSchedule.UNRESOLVED, nfopp.FleetSchedule.NOT_ORDERED) == (0, 1, 2, 3)
    sig = inspect.signature(nfopp.fleet_shift_masks).parameters
    assert list(sig) == ["tracks", "max_delay", "radius", "margin", "obstacles", "obstacle_radius"]
    assert sig["max_delay"].kind is inspect.Parameter.KEYWORD_ONLY and sig["max_delay"].default is inspect.Parameter.empty
    assert (sig["radius"].default, sig["margin"].default, sig["obstacles"].default, sig["obstacle_radius"].default) == (0.0, 0.0, None, None)
    assert list(inspect.signature(nfopp.schedule_delays).parameters) == list(sig) + ["order"]
    assert list(inspect.signature(nfopp.delay_tracks).parameters) == ["tracks", "delay", "count"]
    assert list(inspect.signature(nfopp.FleetMasks.assign).parameters)[:2] == ["self", "order"]
    ts = inspect.signature(nfopp.TimedPaths.schedule).parameters
    assert list(ts)[1:] == ["dt", "count", "max_delay", "radius", "margin", "order", "other", "other_radius", "other_v_max"]
    assert ts["margin"].default == "chord" and ts["order"].default is None
    fs = inspect.signature(nfopp.BatchPlanner.fleet_schedule).parameters
    assert list(fs)[1:10] == ["limits", "dt", "count", "radius", "max_delay", "margin", "order", "best", "obstacles"]
    assert fs["margin"].default == "chord" and fs["best"].default is False and fs["obstacles"].default is None
    assert "fleet_shift_masks" in torch_ops.OPS and "fleet_assign_delays" in torch_ops.OPS
    ops = torch_ops.load()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fleet_shift_masks(torch.zeros(2, 3, 2), 3, None, 0.0, None, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fleet_assign_delays(torch.zeros(2, 2, 2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), None, 3)
    with pytest.raises(nfopp.NfoppError, match="no CPU path"):
        nfopp.fleet_shift_masks(torch.zeros(2, 3, 2), max_delay=3)


def test_the_python_shape_and_type_checks():
    t = torch.zeros(4, 6, 3)
    for md in (-1, 64, 2.5):
        with pytest.raises(ValueError, match="max_delay"):
            nfopp.fleet_shift_masks(t, max_delay=md)
    with pytest.raises(ValueError, match="must be"):
        nfopp.fleet_shift_masks(torch.zeros(4, 6), max_delay=3)
    with pytest.raises(ValueError, match="float32"):
        nfopp.fleet_shift_masks(t.double(), max_delay=3)
    with pytest.raises(ValueError, match="K \\+ max_delay = 9"):
        nfopp.fleet_shift_masks(t, max_delay=3, obstacles=torch.zeros(2, 6, 2))
    with pytest.raises(ValueError, match="laid out"):
        nfopp.fleet_shift_masks(t.transpose(0, 1), max_delay=3)
    masks = nfopp.FleetMasks(torch.zeros(4, 4, 2, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), 3)
    for order in (torch.zeros(3, dtype=torch.int32), torch.zeros(4), [0, 1, 2], torch.zeros(4, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="order"):
            masks.assign(order)
    with pytest.raises(ValueError, match="max_delay"):
        nfopp.FleetMasks(masks.pair, masks.base, masks.bad, 64)
    with pytest.raises(nfopp.NfoppError, match="HIP tensor"):
        masks.assign()
    sched = nfopp.FleetSchedule(torch.tensor([0, -1, 2]), torch.tensor([0, 2, 0]), torch.tensor([0, 7, 3]), 2)
    assert sched.scheduled.tolist() == [True, False, True] and sched.delay_seconds is None and sched.complete is None
    lim = nfopp.MotionLimits(2.0, 1.0)
    timed = nfopp.TimedPaths(torch.zeros(3, 4, 3), torch.zeros(3, 3), torch.zeros(3, 3), lim, torch.zeros(3, 6, 4, dtype=torch.float64),
                             None, torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="other_v_max"):
        timed.schedule(0.1, 4, 3, 0.1, other=torch.zeros(2, 7, 2))
    with pytest.raises(ValueError, match="chord"):
        timed.schedule(0.1, 4, 3, 0.1, margin="cord")
    with pytest.raises(ValueError, match="longest_first"):
        timed.schedule(0.1, 4, 3, 0.1, margin=0.0, order="shortest_first")
