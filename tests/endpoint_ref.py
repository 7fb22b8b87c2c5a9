"""fp32 numpy statement of the start / goal update (csrc/endpoint_update.hip): the reference's
update_goal_point / update_start_point (nfop/constrained_nerf_opt_planner.py:178-194, nfop/nerf_opt_planner.py:202-218)
as unfused delta -> torch's argmin -> cut -> overwrite, followed by `oracle.reparametrize`, which already restates torch's
roundings bit for bit.  Both stages are index work plus that restatement, so the fixtures are expected to be reproduced
exactly.

The switches of `update_endpoint` are the mutants of tests/test_endpoint_update_cpu.py: each one is a way the kernel
could be wrong, and each has to fail at least one case of tests/golden/g20_endpoint_updates.npz.

Also the fixture access and the comparison rule shared by the CPU tests (on this helper) and the GPU tests (on the kernel).
"""
import numpy as np

from oracle import nfopp_oracle as orc

F32 = np.float32
ARRAY_GATE = 5e-6   # tests/test_gpu_planner_api.py::test_update_goal_and_start_point_vs_golden; only used if == fails


def delta_unfused(traj, point):
    """rn(rn(dx*dx) + rn(dy*dy)) over the xy columns: torch's `** 2` and its two-element `sum(dim=1)`."""
    dx = (np.asarray(traj, F32)[:, 0] - F32(point[0])).astype(F32)
    dy = (np.asarray(traj, F32)[:, 1] - F32(point[1])).astype(F32)
    return ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)


def delta_fused(traj, point):
    """fma(dx, dx, rn(dy*dy)): what a contracting compiler makes of the same expression (mutant)."""
    dx = (np.asarray(traj, F32)[:, 0] - F32(point[0])).astype(F32).astype(np.float64)
    dy = (np.asarray(traj, F32)[:, 1] - F32(point[1])).astype(F32)
    return (dx * dx + (dy * dy).astype(F32).astype(np.float64)).astype(F32)


def argmin_torch(keys, last=False):
    """torch.argmin: the first minimal index; a NaN counts as smallest, the first NaN wins.  `last`: mutant tie-break."""
    keys = np.asarray(keys, F32)
    nan = np.isnan(keys)
    hits = np.flatnonzero(nan) if nan.any() else np.flatnonzero(keys == keys.min())
    return int(hits[-1] if last else hits[0])


def update_endpoint(which, point, traj, start, goal, lam=None, cm=None, plus_one=None, last_tie=False, fused=False,
                    other_side=False, overwrite_multipliers=False):
    """One trajectory [N, D].  which: 0 start, 1 goal.  Returns dict(traj, lam, cm, start, goal, min_index)."""
    traj, point = np.asarray(traj, F32).copy(), np.asarray(point, F32)
    n, d = traj.shape
    if plus_one is None:
        plus_one = d == 3                      # the reference's asymmetry: +1 (capped) for SE(2), none for 2-D
    delta = (delta_fused if fused else delta_unfused)(traj, point)
    m = argmin_torch(delta, last=last_tie)
    if plus_one:
        m = min(m + 1, n)
    start, goal = np.asarray(start, F32).copy(), np.asarray(goal, F32).copy()
    tail = (which == 1) != other_side
    if tail:
        traj[m:] = point
    else:
        traj[:m] = point
    if which == 1:
        goal = point.copy()
    else:
        start = point.copy()
    if d == 2:
        out = orc.reparametrize(traj[None], start[None], goal[None])[0]
        return dict(traj=out, lam=None, cm=None, start=start, goal=goal, min_index=m)
    lam, cm = np.asarray(lam, F32).copy(), np.asarray(cm, F32).copy()
    if overwrite_multipliers:
        if tail:
            cm[m:], lam[m + 1:] = 0, 0
        else:
            cm[:m], lam[:m] = 0, 0
    out, new_lam, new_cm = orc.reparametrize(traj[None], start[None], goal[None], lam[None], cm[None])
    return dict(traj=out[0], lam=new_lam[0], cm=new_cm[0], start=start, goal=goal, min_index=m)


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def g20_cases(z):
    """Every case of g20_endpoint_updates.npz as dict(tag, which, point, in/out state, min_index)."""
    cases = []
    for key in sorted(z.files):
        if not key.endswith("_which"):
            continue
        tag = key[:-len("_which")]
        se2 = (tag + "_in_lam") in z.files
        cases.append(dict(tag=tag, which=int(z[key]), point=z[tag + "_point"], traj=z[tag + "_in_traj"], start=z[tag + "_start"],
                          goal=z[tag + "_goal"], lam=z[tag + "_in_lam"] if se2 else None, cm=z[tag + "_in_cm"] if se2 else None,
                          out_traj=z[tag + "_out_traj"], out_lam=z[tag + "_out_lam"] if se2 else None,
                          out_cm=z[tag + "_out_cm"] if se2 else None, min_index=int(z[tag + "_min_index"])))
    return cases


def g4_cases(z):
    """The two calls of g4_update_endpoints.npz (goal, then start on its result); the fixture has no min_index."""
    goal = dict(tag="g4_goal", which=1, point=z["new_goal"], traj=z["in_traj"], start=z["start"], goal=z["goal"], lam=z["in_lam"],
                cm=z["in_cm"], out_traj=z["goal_out_traj"], out_lam=z["goal_out_lam"], out_cm=z["goal_out_cm"], min_index=None)
    start = dict(tag="g4_start", which=0, point=z["new_start"], traj=z["goal_out_traj"], start=z["start"], goal=z["new_goal"],
                 lam=z["goal_out_lam"], cm=z["goal_out_cm"], out_traj=z["start_out_traj"], out_lam=z["start_out_lam"],
                 out_cm=z["start_out_cm"], min_index=None)
    return [goal, start]


def mismatch(case, got):
    """None if `got` (dict traj / lam / cm / min_index) reproduces the case under the rule of the tests: min_index with ==,
    arrays with np.array_equal -- else, per array, the largest difference, which must stay below ARRAY_GATE and is
    reported.  Returns a string naming what failed, and the largest array difference seen."""
    worst, bad = 0.0, []
    if case["min_index"] is not None and int(got["min_index"]) != case["min_index"]:
        bad.append("min_index %d != %d" % (int(got["min_index"]), case["min_index"]))
    for name in ("traj", "lam", "cm"):
        want = case["out_" + name]
        if want is None:
            continue
        have = np.asarray(got[name], F32).reshape(want.shape)
        if not np.array_equal(have, want):
            diff = float(np.max(np.abs(have.astype(np.float64) - want.astype(np.float64))))
            worst = max(worst, diff)
            print("%s: %s differs from the fixture, max |d| = %.3e" % (case["tag"], name, diff))
            if not diff < ARRAY_GATE:
                bad.append("%s max |d| = %.3e" % (name, diff))
    return ("; ".join(bad) or None), worst
