#!/usr/bin/env python3
"""Generate tests/golden/g23_reparam_shapes.npz: the reference's `reparametrize_trajectory` (SE(2):
constrained_nerf_opt_planner.py:132-171, 2-D: nerf_opt_planner.py:224-244) on every case of tests/reparam_cases.py -- the
sizes at which csrc/reparam.h takes another branch, times the input kinds described there.

Needs the reference checkout (NFOPP_REFERENCE), imported unmodified through make_golden.py's shims.  As
make_golden.py::g4_reparam does, it builds the reference's planner at each N (the SE(2) one through its factory, the 2-D
one with the factory's values restated, since the factory fixes N = 100), writes the case's inputs into the planner, calls
the planner's own method and records what comes out.  Written:
    names           [C] the cases, "d<D>_n<N>_<kind>"
    in_digest       [C, 5, 32] uint8: sha256 of traj, start, goal, lam, cm as handed to the reference (zeros: absent, D = 2)
    out_digest      [C, 3, 32] uint8: sha256 of the trajectory, lam and cm the reference left (reparam_cases.digest)
    d<D>_n<N>_traj  [K, N, D], d3_n<N>_lam [K, N + 1], d3_n<N>_cm [K, N]: those outputs themselves for N <= 257, over the
                    kinds of that D in the order of reparam_cases.kinds(D)

Usage:  MPLBACKEND=Agg python tests/golden/make_golden_reparam_shapes.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402  (installs the shims)
from make_golden import F32, ONF, CircleCollisionChecker  # noqa: E402
from neural_field_optimal_planner.nerf_opt_planner import NERFOptPlanner  # noqa: E402
import reparam_cases as rc  # noqa: E402


def se2_planner(n):
    planner, _ = make_golden.make_planner(n)
    return planner


def planner_2d(n):
    """PlannerFactory.make_onf_planner's planner with n waypoints; it is never initialised or stepped."""
    model = ONF(1.5, 1)
    trajectory = torch.zeros(n, 2, requires_grad=True)
    planner = NERFOptPlanner(trajectory, model, CircleCollisionChecker(0.3, (0, 3, 0, 3)),
                             torch.optim.Adam(model.parameters(), 1e-3, betas=(0.9, 0.9)),
                             torch.optim.Adam([trajectory], 1e-2, betas=(0.9, 0.999)), trajectory_random_offset=0.02,
                             collision_weight=0.01, velocity_hessian_weight=3, random_field_points=10,
                             init_collision_iteration=400)
    torch.autograd.set_detect_anomaly(False)
    return planner


def run(planner, case):
    """The case through the planner's own reparametrize_trajectory: dict(traj, lam, cm)."""
    with torch.no_grad():
        planner._trajectory.data = torch.tensor(case["traj"])
        planner._start_point = torch.tensor(case["start"])[None]
        planner._goal_point = torch.tensor(case["goal"])[None]
        if case["lam"] is not None:
            planner._constraint_multipliers.data = torch.tensor(case["lam"])
            planner._collision_multipliers.data = torch.tensor(case["cm"])
        planner.reparametrize_trajectory()
        out = dict(traj=planner._trajectory.detach().numpy().copy(), lam=None, cm=None)
        if case["lam"] is not None:
            out["lam"] = planner._constraint_multipliers.detach().numpy().copy()
            out["cm"] = planner._collision_multipliers.detach().numpy().copy()
    for k, v in out.items():
        assert v is None or (v.dtype == F32 and v.shape == case[k].shape), k
    return out


def generate():
    out, names, din, dout = {}, [], [], []
    for d in (3, 2):
        for n in rc.SIZES[d]:
            planner = se2_planner(n) if d == 3 else planner_2d(n)
            results = []
            for kind in rc.kinds(d):
                case = rc.make_case(d, n, kind)
                res = run(planner, case)
                if kind in rc.NONFINITE_KINDS:
                    assert all(np.isnan(v).all() for v in res.values() if v is not None), (d, n, kind)
                else:
                    assert all(np.isfinite(v).all() for v in res.values() if v is not None), (d, n, kind)
                names.append(rc.case_name(d, n, kind))
                din.append(np.stack([rc.digest(case[k]) for k in rc.INPUTS]))
                dout.append(np.stack([rc.digest(res[k]) for k in rc.OUTPUTS]))
                results.append(res)
            if n <= rc.STORED_MAX_N:
                for k in rc.OUTPUTS if d == 3 else ("traj",):
                    out["d%d_n%d_%s" % (d, n, k)] = np.stack([r[k] for r in results])
            print("D = %d  N = %4d  %d kinds" % (d, n, len(results)), flush=True)
    out["names"] = np.asarray(names)
    out["in_digest"] = np.stack(din)
    out["out_digest"] = np.stack(dout)
    return out


if __name__ == "__main__":
    torch.set_num_threads(1)
    out = generate()
    target = os.path.join(HERE, rc.FIXTURE)
    np.savez_compressed(target, **out)
    print("%-28s %8.1f KB, %d cases" % (os.path.basename(target), os.path.getsize(target) / 1024, len(out["names"])))
