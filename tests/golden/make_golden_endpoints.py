#!/usr/bin/env python3
"""Generate tests/golden/g20_endpoint_updates.npz from the reference's update_goal_point / update_start_point
(PyTorch-CPU): constrained_nerf_opt_planner.py:178-194 for SE(2), nerf_opt_planner.py:202-218 for the 2-D planner.

Needs the reference checkout (NFOPP_REFERENCE), imported unmodified through make_golden.py's shims.  Only inputs and the
numbers the reference computed from them are written.  Per case `<tag>`:
    <tag>_in_traj / _in_lam / _in_cm / _start / _goal     state before the call (lam / cm: SE(2) only)
    <tag>_which (0 start, 1 goal), <tag>_point             the call
    <tag>_out_traj / _out_lam / _out_cm                    state after it
    <tag>_min_index                                        the reference's `min_index` (its own expression, evaluated
                                                           by torch on the state before the call)
SE(2) cases (N = 100, 25 steps as g4_update_endpoints, frozen, random multipliers as g4_reparam):
    se2_a goal near mid-path          se2_b goal past the end (argmin last, m capped at N, nothing overwritten)
    se2_c goal nearest waypoint 0 (N-1 zero-length segments: denominator clamp, sequential cumsum)
    se2_d start near mid-path         se2_e start nearest the last waypoint (everything overwritten)
    se2_f exact tie (two waypoints mirrored about the diagonal through the new goal: equal fp32 deltas when every
          operation is rounded on its own, different ones when the sum is contracted to an fma)
    se2_g headings straddling +-pi across the cut        se2_h1 / se2_h2 goal update, then start update
2-D cases (g10's recipe): p2d_a goal mid-path, p2d_b start mid-path, p2d_c start with argmin 0 (nothing overwritten),
    p2d_d a tie built like se2_f.

Usage:  MPLBACKEND=Agg python tests/golden/make_golden_endpoints.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import F32, freeze, make_planner  # noqa: E402


def fused_delta(dx, dy):
    """fma(dx, dx, rn(dy * dy)) in fp32 -- what a contracting compiler makes of dx*dx + dy*dy (float64 holds the exact
    product and the sum of two fp32-representable terms rounds once more only in a tie)."""
    dx, dy = np.asarray(dx, F32), np.asarray(dy, F32)
    yy = (dy * dy).astype(F32).astype(np.float64)
    return (dx.astype(np.float64) * dx.astype(np.float64) + yy).astype(F32)


def tie_offsets(rng):
    """(a, b): multiples of 2^-20 near 0.01 for which the unfused deltas of (a, b) and (b, a) are equal (always) and
    the fused delta of (b, a) is strictly smaller, so a contracted kernel would pick the SECOND waypoint."""
    while True:
        a, b = (F32(k * 2.0 ** -20) for k in rng.integers(6000, 16000, 2))
        if a != b and fused_delta(b, a) < fused_delta(a, b):
            return a, b


def min_index_of(planner, point, plus_one):
    """The reference's own expression for min_index, on the state before the call."""
    ref = torch.tensor(np.asarray(point, F32))[None]
    tr = planner._trajectory.detach()
    if plus_one:
        delta = torch.sum((tr[:, :2] - ref[:, :2]) ** 2, dim=1)
        return int(min(torch.argmin(delta) + 1, tr.shape[0])), delta.numpy()
    delta = torch.sum((tr - ref) ** 2, dim=1)
    return int(torch.argmin(delta)), delta.numpy()


def point_nearest(traj, target, rng, away_from=None):
    """An xy point whose nearest waypoint is `target` (and which differs from `away_from`): random offsets around it."""
    for radius in (0.2, 0.1, 0.05, 0.02, 0.01, 0.005):
        for _ in range(200):
            q = (traj[target, :2] + rng.uniform(-radius, radius, 2)).astype(F32)
            d = ((traj[:, 0] - q[0]) ** 2 + (traj[:, 1] - q[1]) ** 2).astype(F32)
            if int(np.argmin(d)) == target and np.sum(d == d.min()) == 1 and (away_from is None or np.abs(q - away_from[:2]).max() > 1e-3):
                return q
    raise AssertionError("no point found whose nearest waypoint is %d" % target)


class Recorder(object):
    def __init__(self, planner, se2):
        self.planner, self.se2, self.out = planner, se2, {}

    def set_state(self, traj, start, goal, lam=None, cm=None):
        p = self.planner
        with torch.no_grad():
            p._trajectory.data = torch.tensor(np.asarray(traj, F32).copy())
            p._start_point = torch.tensor(np.asarray(start, F32).copy())[None]
            p._goal_point = torch.tensor(np.asarray(goal, F32).copy())[None]
            if self.se2:
                p._constraint_multipliers.data = torch.tensor(np.asarray(lam, F32).copy())
                p._collision_multipliers.data = torch.tensor(np.asarray(cm, F32).copy())

    def run(self, tag, which, point, expect_argmin=None):
        p, out = self.planner, self.out
        point = np.asarray(point, F32)
        out[tag + "_in_traj"] = p._trajectory.detach().numpy().copy()
        out[tag + "_start"] = p._start_point.numpy()[0].copy()
        out[tag + "_goal"] = p._goal_point.numpy()[0].copy()
        if self.se2:
            out[tag + "_in_lam"] = p._constraint_multipliers.detach().numpy().copy()
            out[tag + "_in_cm"] = p._collision_multipliers.detach().numpy().copy()
        m, delta = min_index_of(p, point, self.se2)
        if expect_argmin is not None:
            assert int(np.argmin(delta)) == expect_argmin, (tag, int(np.argmin(delta)), expect_argmin)
        (p.update_goal_point if which else p.update_start_point)(point)
        assert p._step_count == 0
        out[tag + "_which"] = np.asarray(which, np.int32)
        out[tag + "_point"] = point
        out[tag + "_min_index"] = np.asarray(m, np.int32)
        out[tag + "_out_traj"] = p._trajectory.detach().numpy().copy()
        if self.se2:
            out[tag + "_out_lam"] = p._constraint_multipliers.detach().numpy().copy()
            out[tag + "_out_cm"] = p._collision_multipliers.detach().numpy().copy()
        fin = out[tag + "_out_traj"]
        assert np.isfinite(fin).all(), tag
        return m, delta


def with_tie(traj, i, a, b):
    """Waypoints i, i+1 moved to p + (a, b) and p + (b, a) about the point p nearest their midpoint on the 2^-10 grid; returns
    (trajectory, p).  px, py below 2 (ulp at most 2^-23) and a, b multiples of 2^-20: every sum and difference below is
    exact (asserted)."""
    traj = traj.copy()
    mid = (traj[i, :2] + traj[i + 1, :2]) / 2
    p = (np.round(mid.astype(np.float64) * 2 ** 10) / 2 ** 10).astype(F32)
    assert (p >= 0.25).all() and (p < 2).all(), p
    traj[i, 0], traj[i, 1] = p[0] + a, p[1] + b
    traj[i + 1, 0], traj[i + 1, 1] = p[0] + b, p[1] + a
    assert F32(traj[i, 0] - p[0]) == a and F32(traj[i + 1, 1] - p[1]) == a
    assert F32(traj[i, 1] - p[1]) == b and F32(traj[i + 1, 0] - p[0]) == b
    return traj, p


def check_tie(delta, i, traj, p):
    assert delta[i] == delta[i + 1], "the fp32 deltas of the mirrored pair must be equal"
    others = np.delete(delta, [i, i + 1])
    assert (others > delta[i]).all(), "the pair must be the strict minimum"
    f = fused_delta(traj[:, 0] - p[0], traj[:, 1] - p[1])
    assert f[i + 1] < f[i] and int(np.argmin(f)) == i + 1, "a contracted delta must prefer the second waypoint"


def se2_cases(out):
    planner, env = make_planner(100)
    for _ in range(25):
        planner.step()
    freeze(planner)
    rng = np.random.default_rng(20)
    with torch.no_grad():
        planner._collision_multipliers.data = torch.tensor(rng.uniform(0, 0.2, 100).astype(F32))
        planner._constraint_multipliers.data = torch.tensor(rng.normal(0, 0.3, 101).astype(F32))
    base = dict(traj=planner._trajectory.detach().numpy().copy(), start=planner._start_point.numpy()[0].copy(),
                goal=planner._goal_point.numpy()[0].copy(), lam=planner._constraint_multipliers.detach().numpy().copy(),
                cm=planner._collision_multipliers.detach().numpy().copy())
    rec = Recorder(planner, True)
    tr, n = base["traj"], 100

    def reset(traj=None):
        rec.set_state(base["traj"] if traj is None else traj, base["start"], base["goal"], base["lam"], base["cm"])

    reset()
    rec.run("se2_a", 1, np.r_[tr[50, :2] + F32([0.03, -0.02]), 0.4])
    reset()
    m, _ = rec.run("se2_b", 1, np.r_[point_nearest(tr, n - 1, rng), base["goal"][2] + 0.2], expect_argmin=n - 1)
    assert m == n
    reset()
    m, _ = rec.run("se2_c", 1, np.r_[point_nearest(tr, 0, rng), -0.5], expect_argmin=0)
    assert m == 1
    reset()
    rec.run("se2_d", 0, np.r_[tr[40, :2] + F32([-0.02, 0.03]), 1.1])
    reset()
    new_start = np.r_[point_nearest(tr, n - 1, rng, away_from=base["goal"]), 0.3].astype(F32)
    assert not np.array_equal(new_start[:2], base["goal"][:2])
    m, _ = rec.run("se2_e", 0, new_start, expect_argmin=n - 1)
    assert m == n
    a, b = tie_offsets(rng)
    tied, p = with_tie(tr, 50, a, b)
    reset(tied)
    m, delta = rec.run("se2_f", 1, np.r_[p, 0.7], expect_argmin=50)
    check_tie(delta, 50, tied, p)
    assert m == 51
    wrapped = tr.copy()
    wrapped[:, 2] = mg.wrap_angle(torch.tensor(np.linspace(2.6, 3.9, n).astype(F32))).numpy()
    reset(wrapped)
    rec.run("se2_g", 1, np.r_[wrapped[38, :2] + F32([0.01, 0.02]), -3.0])
    assert wrapped[38, 2] > 3.0 and wrapped[45, 2] < -3.0         # +pi side before the cut, the new goal on the -pi side
    reset()
    rec.run("se2_h1", 1, np.r_[tr[70, :2] + F32([0.02, 0.02]), 0.9])
    rec.run("se2_h2", 0, np.r_[tr[20, :2] + F32([-0.01, 0.02]), 0.1])
    out.update(rec.out)


def p2d_cases(out):
    torch.random.manual_seed(100)
    np.random.seed(400)
    env = mg.TestEnvironmentBuilder().make_test_environment()
    cc = mg.CircleCollisionChecker(0.3, (0, 3, 0, 3))
    cc.update_obstacle_points(env.obstacle_points)
    planner = mg.PlannerFactory.make_onf_planner(cc)
    planner._init_collision_iteration = 40
    planner.init(env.start_point, env.goal_point, env.bounds)
    torch.autograd.set_detect_anomaly(False)
    for _ in range(15):
        planner.step()
    freeze(planner)
    base = dict(traj=planner._trajectory.detach().numpy().copy(), start=planner._start_point.numpy()[0].copy(),
                goal=planner._goal_point.numpy()[0].copy())
    rec = Recorder(planner, False)
    tr, n = base["traj"], base["traj"].shape[0]
    rng = np.random.default_rng(21)

    def reset(traj=None):
        rec.set_state(base["traj"] if traj is None else traj, base["start"], base["goal"])

    reset()
    rec.run("p2d_a", 1, tr[55] + F32([0.02, -0.03]))
    reset()
    rec.run("p2d_b", 0, tr[35] + F32([-0.03, 0.01]))
    reset()
    m, _ = rec.run("p2d_c", 0, point_nearest(tr, 0, rng), expect_argmin=0)
    assert m == 0
    a, b = tie_offsets(rng)
    tied, p = with_tie(tr, 50, a, b)
    reset(tied)
    m, delta = rec.run("p2d_d", 1, p, expect_argmin=50)
    check_tie(delta, 50, tied, p)
    assert m == 50
    out.update(rec.out)


def main():
    out = {}
    se2_cases(out)
    p2d_cases(out)
    for k, v in out.items():
        assert v.dtype != object, k
    path = os.path.join(HERE, "g20_endpoint_updates.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
