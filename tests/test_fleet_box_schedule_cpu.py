"""CPU: the rule of nfopp_fleet_box_shift_masks as restated in tests/fleet_box_schedule_ref.py -- the hand cases with their exact
bits, delays and statuses beside the disc schedule's, the density of the random cases, independence of the horizon, the mirror
rule -- and the interface: header, binding and library agree, every argument check answers without a GPU, the Python names and
their checks exist."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import nfopp
from nfopp import _lib

import box_conflict_ref as br
import fleet_box_schedule_cases as xc
import fleet_box_schedule_ref as xr
import fleet_schedule_ref as fr

F32 = np.float32
CSRC = os.path.join(ROOT, "pytorch-motion-planner_amd", "csrc")


def _text(row):
    return "".join("1" if x else "0" for x in row)


# ---- hand cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(xc.hand_cases()))
def test_hand_cases_have_their_exact_bits_delays_and_statuses(name):
    c = xc.hand_cases()[name]
    e = c["expect"]
    for refine, (want_bits, delay, status) in sorted(e["refines"].items()):
        m, s = xc.solve(c, refine)
        assert _text(m["pair_bits"][0, 1]) == want_bits, (name, refine)
        assert _text(m["pair_bits"][1, 0]) == want_bits[::-1], (name, refine)
        assert s["delay"].tolist() == delay and s["status"].tolist() == status, (name, refine, s)
    m, s = xc.disc_solve(c)
    assert _text(m["pair_bits"][0, 1]) == e["disc"][0] and s["delay"].tolist() == e["disc"][1] and s["status"].tolist() == e["disc"][2]
    order = np.array([1, 0], np.int32)
    for refine, (delay, status) in e.get("reordered", {}).items():
        s = xc.solve(c, refine, order)[1]
        assert s["delay"].tolist() == delay and s["status"].tolist() == status, (name, refine)
    if "disc_reordered" in e:
        s = xc.disc_solve(c, order)[1]
        assert s["delay"].tolist() == e["disc_reordered"][0] and s["status"].tolist() == e["disc_reordered"][1]


def test_the_hand_cases_are_the_issue_the_schedule_is_for():
    """lanes: the box check calls the undelayed fleet FREE at refine 2 while the disc schedule cannot place robot 1."""
    c = xc.hand_cases()["lanes"]
    free = br.pairs(c["tracks"], c["units"], dt=1.0, box_a=c["box"], radius_a=c["radius"], refine=2)["status"]
    assert free[0, 1] == br.FREE
    assert xc.disc_solve(c)[1]["status"].tolist() == [0, fr.STATUS_UNRESOLVED] and xc.solve(c, 2)[1]["status"].tolist() == [0, 0]


# ---- the random family -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    return [(n, xc.sized_case(n)) + xc.solve(xc.sized_case(n), xc.REFINES[n]) for n in range(len(xc.SIZES))]


def test_the_share_of_set_bits_of_every_random_case_is_between_a_tenth_and_nine_tenths(solved):
    seen_base = False
    for n, c, m, s in solved:
        if (m["bad"] == 0).sum() < 2:
            continue      # one robot: no off-diagonal bit
        assert 0.1 <= xc.density(m) <= 0.9, (xc.SIZES[n], xc.density(m))
        D = c["max_delay"] + 1
        seen_base |= bool(((m["base"] != 0) & (m["base"] != np.uint64(2 ** D - 1))).any())
    assert seen_base                                                          # a base mask that is neither empty nor full
    c = xc.random_case(3, 5, 9, 3, extent=3.0)
    assert 0.1 <= xc.density(xc.solve(c, 0)[0]) <= 0.9 and 0.1 <= xc.density(xc.solve(c, 2)[0]) <= 0.9


def test_each_kind_of_badness_appears(solved):
    robots = np.zeros(4, int)
    obstacles = np.zeros(4, int)
    for n, c, m, s in solved:
        t, u = c["tracks"], c["units"]
        robots += [int(np.isnan(t[:, :, 0]).any()), int(np.isnan(u).any() and np.isinf(t[:, :, 2]).any()),
                   int((c["box"][:, 0] >= c["box"][:, 1]).any()), int((c["radius"] < 0).any())]
        if c["obstacles"] is not None:
            obstacles += [int(np.isinf(c["obstacles"][:, :, 1]).any()), int(np.isnan(c["obstacle_box"]).any()),
                          int((c["obstacle_box"][:, 2] >= c["obstacle_box"][:, 3]).any()), int(np.isnan(c["obstacle_radius"]).any())]
        bad = m["bad"].astype(bool)
        assert not m["pair_bits"][bad].any() and not m["pair_bits"][:, bad].any() and not m["base_bits"][bad].any()
        assert (s["status"][bad] == fr.STATUS_BAD_TRACK).all()
    assert (robots >= 1).all() and (obstacles >= 1).all(), (robots, obstacles)


def test_mask_ji_is_the_bit_reversal_of_mask_ij(solved):
    for n, c, m, s in solved:
        pb = m["pair_bits"]
        assert np.array_equal(pb.transpose(1, 0, 2), pb[:, :, ::-1]), xc.SIZES[n]
        assert not pb[np.arange(len(pb)), np.arange(len(pb))].any()
        assert np.array_equal(fr.unpack(m["pair"], pb.shape[2]), pb) and not fr.unpack(m["pair"], 128)[..., pb.shape[2]:].any()


def _absolute(c, refine, qi, qj, i, j):
    """The box check on robots i and j delayed by qi and qj in absolute time over K + max_delay instants -> not FREE."""
    K, md = c["tracks"].shape[1], c["max_delay"]
    n = K + md
    a, ua = fr.delay_tracks(c["tracks"][[i]], qi, n), fr.delay_tracks(c["units"][[i]], qi, n)
    b, ub = fr.delay_tracks(c["tracks"][[j]], qj, n), fr.delay_tracks(c["units"][[j]], qj, n)
    p = br.pairs(a, ua, b, ub, dt=1.0, box_a=c["box"][[i]], box_b=c["box"][[j]], radius_a=c["radius"][[i]], radius_b=c["radius"][[j]],
                 margin=c["margin"], refine=refine)
    return p["status"][0, 0] != br.FREE


def test_the_bit_depends_on_the_two_delays_through_their_difference_alone():
    """For every (q_i, q_j): both tracks delayed in absolute time over K + max_delay instants agree with bit q_i - q_j.  The
    waiting intervals in front and the parked intervals behind add neither a CONFLICT nor an UNDECIDED."""
    lanes = xc.hand_cases()["lanes"]
    cases = [(lanes, 0), (lanes, 2)] + [(xc.random_case(40 + n, 2, 5, 3, extent=1.5), n % 3) for n in range(96)]
    seen = set()
    for c, refine in cases:
        md = c["max_delay"]
        pb = xr.pair_bits(c["tracks"], c["units"], md, box=c["box"], radius=c["radius"], margin=c["margin"], refine=refine)
        for qi in range(md + 1):
            for qj in range(md + 1):
                got = _absolute(c, refine, qi, qj, 0, 1)
                assert got == pb[0, 1, md + qi - qj], (refine, qi, qj)
                seen.add(bool(got))
    assert seen == {True, False}


def test_a_schedule_of_the_restatement_is_free_by_the_box_check(solved):
    seen = 0
    for n, c, m, s in solved:
        on = np.flatnonzero(s["status"] == 0)
        if len(on) < 2:
            continue
        K, md = c["tracks"].shape[1], c["max_delay"]
        moved = fr.delay_tracks(c["tracks"], np.maximum(s["delay"], 0), K + md)[on]
        units = fr.delay_tracks(c["units"], np.maximum(s["delay"], 0), K + md)[on]
        p = br.pairs(moved, units, dt=1.0, box_a=c["box"][on], radius_a=c["radius"][on], margin=c["margin"], refine=xc.REFINES[n])
        off = ~np.eye(len(on), dtype=bool)
        assert (p["status"][off] == br.FREE).all(), xc.SIZES[n]
        if c["obstacles"] is not None:
            q = br.pairs(moved, units, c["obstacles"], c["obstacle_units"], dt=1.0, box_a=c["box"][on], box_b=c["obstacle_box"],
                         radius_a=c["radius"][on], radius_b=c["obstacle_radius"], margin=c["margin"], refine=xc.REFINES[n])
            assert np.isin(q["status"], (br.FREE, br.BAD_PAIR)).all(), xc.SIZES[n]
        seen += 1
    assert seen >= 2


# ---- interface ---------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    lib = nfopp.load_library()
    header = open(os.path.join(ROOT, "include", "nfopp_hip.h")).read()
    for name, n_args, res, ctype in (("nfopp_fleet_box_shift_masks", 22, "int", ctypes.c_int),
                                     ("nfopp_fleet_box_shift_masks_workspace_bytes", 4, "size_t", ctypes.c_size_t)):
        decl = re.search(r"\b%s %s\(([^;]*)\);" % (res, name), header)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == n_args and _lib._SIGNATURES[name][0] is ctype
    assert lib.nfopp_abi_version() == 6
    assert "fleet_box_schedule.hip" in open(os.path.join(CSRC, "Makefile")).read()
    src = open(os.path.join(CSRC, "fleet_box_schedule.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include", 1)[1]
    # one statement of the box rule and of the mask layout: the kernel files call the shared headers and define none of it
    assert '#include "box_pairs.h"' in src and '#include "fleet_masks.h"' in src
    for word in ("box_separation(const", "classify_node(const", "axis_gap(double", "reverse_mask(unsigned"):
        owners = [f for f in sorted(os.listdir(CSRC)) if word in open(os.path.join(CSRC, f)).read()]
        assert len(owners) == 1 and owners[0].endswith(".h"), (word, owners)
    for word in ("not NFOPP_BOX_PAIR_FREE", "same clamped index", "bits reversed", "difference alone", "Arguments refused"):
        assert word in header, word


def _rc(b=3, stride=3, k=4, margin=0.0, refine=0, max_delay=3, m=0, obstacle_stride=3, tracks=1, heading=1, box=1, obstacles=0,
        obstacle_heading=1, obstacle_box=1, pair=1, base=1, bad=1, workspace=1, workspace_bytes=1 << 20):
    P = lambda v: ctypes.c_void_p(v) if v else None
    return nfopp.load_library().nfopp_fleet_box_shift_masks(
        P(tracks), P(heading), b, stride, k, P(box), None, margin, refine, max_delay, P(obstacles), P(obstacle_heading), m, obstacle_stride,
        P(obstacle_box), None, P(pair), P(base), P(bad), P(workspace), workspace_bytes, None)


def test_every_argument_check_answers_without_a_gpu():
    lib = nfopp.load_library()

    def refused(rc, word):
        assert rc == -1, word
        assert word in lib.nfopp_last_error().decode(), (word, lib.nfopp_last_error())

    refused(_rc(b=-1), "batch")
    refused(_rc(b=2 ** 31), "batch")
    refused(_rc(m=-1, obstacles=1), "batch")
    for md in (-1, 64):
        refused(_rc(max_delay=md), "max_delay")
    refused(_rc(k=0), "k >= 1")
    refused(_rc(k=2 ** 31 - 1), "too many instants")
    refused(_rc(stride=2), "stride")
    refused(_rc(m=2, obstacles=1, obstacle_stride=2), "stride")
    for refine in (-1, 9, 2 ** 31 - 1):
        refused(_rc(refine=refine), "refine")
    for margin in (np.nan, np.inf, -np.inf):
        refused(_rc(margin=margin), "margin")
    for null in ("tracks", "heading", "box", "pair", "base", "bad"):
        refused(_rc(**{null: 0}), "null device pointer")
    for null in ("obstacle_heading", "obstacle_box"):
        refused(_rc(m=2, obstacles=1, **{null: 0}), "null device pointer")
    assert _rc(b=0, tracks=0, heading=0, box=0, pair=0, base=0, bad=0, workspace=0, workspace_bytes=0) == 0      # nothing to do
    refused(_rc(b=2 ** 31 - 1, workspace_bytes=2 ** 62), "too many")                  # more tiles than a grid holds
    refused(_rc(b=2 ** 20, m=2 ** 20, obstacles=1, workspace_bytes=2 ** 62), "too many")
    # the workspace: a shape row of 8 doubles per robot and obstacle, one word per robot and tile of 8 obstacles
    assert lib.nfopp_fleet_box_shift_masks_workspace_bytes(0, 5, 4, 3) == 0
    for b, m in ((3, 0), (3, 2), (9, 8), (9, 9), (1, 17)):
        need = lib.nfopp_fleet_box_shift_masks_workspace_bytes(b, m, 4, 3)
        assert need == ((b + m) * 8 + b * -(-m // 8)) * 8
        refused(_rc(b=b, m=m, obstacles=1 if m else 0, workspace_bytes=need - 1), "workspace")
        refused(_rc(b=b, m=m, obstacles=1 if m else 0, workspace=0, workspace_bytes=need), "workspace")


def test_python_names_and_signatures():
    for name in ("fleet_box_shift_masks", "schedule_box_delays"):
        assert hasattr(nfopp, name) and name in nfopp.__all__, name
    sig = inspect.signature(nfopp.fleet_box_shift_masks).parameters
    assert list(sig) == ["tracks", "max_delay", "box", "radius", "margin", "refine", "obstacles", "obstacle_box", "obstacle_radius"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[1:])
    assert sig["box"].default is inspect.Parameter.empty and sig["max_delay"].default is inspect.Parameter.empty
    assert (sig["radius"].default, sig["margin"].default, sig["refine"].default, sig["obstacles"].default) == (0.0, 0.0, 0, None)
    assert list(inspect.signature(nfopp.schedule_box_delays).parameters) == list(sig) + ["order"]
    ts = inspect.signature(nfopp.TimedPaths.schedule_boxes).parameters
    assert list(ts)[1:] == ["dt", "count", "max_delay", "box", "radius", "margin", "order", "refine", "other", "other_box", "other_radius",
                            "other_v_max", "other_w_max"]
    assert ts["margin"].default == "chord" and ts["refine"].default == 0
    fs = inspect.signature(nfopp.BatchPlanner.fleet_schedule).parameters
    assert list(fs)[-6:] == ["box", "refine", "obstacle_box", "obstacle_w_max", "replan_radius", "replan"]
    assert fs["box"].default is None and fs["refine"].default == 0 and fs["replan_radius"].default is None
    masks = nfopp.FleetMasks(torch.zeros(2, 2, 2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 3)
    assert masks.box is None and masks.refine == 0                                    # the disc path
    boxed = nfopp.FleetMasks(masks.pair, masks.base, masks.bad, 3, box=torch.zeros(2, 4), refine=2)
    assert boxed.box.shape == (2, 4) and boxed.refine == 2


def test_the_python_shape_and_type_checks():
    t = torch.zeros(4, 6, 3)
    car = xc.CAR
    with pytest.raises(nfopp.NfoppError, match="no CPU path"):
        nfopp.fleet_box_shift_masks(t, max_delay=3, box=car)
    for md in (-1, 64, 2.5):
        with pytest.raises(ValueError, match="max_delay"):
            nfopp.fleet_box_shift_masks(t, max_delay=md, box=car)
    with pytest.raises(ValueError, match="needs box"):
        nfopp.fleet_box_shift_masks(t, max_delay=3, box=None)
    with pytest.raises(ValueError, match="x, y, theta"):
        nfopp.fleet_box_shift_masks(torch.zeros(4, 6, 2), max_delay=3, box=car)
    with pytest.raises(ValueError, match="refine"):
        nfopp.fleet_box_shift_masks(t, max_delay=3, box=car, refine=9)
    with pytest.raises(ValueError, match="K \\+ max_delay = 9"):
        nfopp.fleet_box_shift_masks(t, max_delay=3, box=car, obstacles=torch.zeros(2, 6, 3))
    with pytest.raises(ValueError, match="float32"):
        nfopp.fleet_box_shift_masks(t.double(), max_delay=3, box=car)
    lim = nfopp.MotionLimits(2.0, 1.0)
    flat = nfopp.TimedPaths(torch.zeros(3, 4, 2), torch.zeros(3, 2), torch.zeros(3, 2), lim, torch.zeros(3, 6, 4, dtype=torch.float64),
                            None, torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="SE\\(2\\)"):
        flat.schedule_boxes(0.1, 4, 3, car)
    timed = nfopp.TimedPaths(torch.zeros(3, 4, 3), torch.zeros(3, 3), torch.zeros(3, 3), lim, torch.zeros(3, 6, 4, dtype=torch.float64),
                             None, torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="needs box"):
        timed.schedule_boxes(0.1, 4, 3, None)
    with pytest.raises(ValueError, match="chord"):
        timed.schedule_boxes(0.1, 4, 3, car, margin="cord")
    with pytest.raises(ValueError, match="other_v_max"):
        timed.schedule_boxes(0.1, 4, 3, car, other=torch.zeros(2, 7, 3))


def test_the_disc_that_covers_a_box_for_callers_that_reserve_discs():
    """`box_disc_radius`: the farthest corner (times 1.000001) plus the rounding radius, per row, on the tensors' device."""
    from nfopp.conflicts import box_disc_radius
    boxes = torch.tensor([[-1.0, 1.0, -0.5, 0.5], [-0.1, 0.2, -0.05, 0.05]])
    got = box_disc_radius(boxes, torch.tensor([0.25, 0.0]), 2, boxes.device).numpy()
    want = np.hypot([1.0, 0.2], [0.5, 0.05]) + [0.25, 0.0]
    assert got.dtype == np.float32 and (got >= want.astype(np.float32)).all() and np.allclose(got, want, rtol=0, atol=1e-5)
    one = box_disc_radius(xc.CAR, None, 3, boxes.device).numpy()
    assert one.shape == (3,) and (one >= np.float32(xc.DISC)).all() and np.allclose(one, xc.DISC, rtol=0, atol=1e-5)
