#!/usr/bin/env python3
"""Generate tests/golden/g22_path_tools.npz: the reference's `PathPostprocessor.process` (ros/path_postprocessor.py:13-69)
and `TrajectoryInitializer` (trajectory_initializer.py:12-45, with and without `init_angles_with_trajectory`; its debug
prints are swallowed) at the edges of csrc/path_post.hip and csrc/traj_init.hip.

Needs the reference checkout (NFOPP_REFERENCE), imported unmodified through make_golden.py's shims.  Only fp32 inputs,
parameters and the numbers the reference computed from them are written (float64 poses; where the reference raises, the
exception's class name).

Post-processor, per case `<name>` of `post_names`:
    post_<name>_in      [n, 3] fp32 path            post_<name>_par   fp32 (minimal_distance, distance_step)
    post_<name>_out     [count, 3] float64          post_<name>_err   class name of the exception (then there is no _out)
Families (the helpers below say how each input is built):
    len_<n>             curved paths of every length at which the kernel takes another branch
    park_<k>            a parked stretch leaves k segments (k + 1 poses) after the filter, n is larger
    filter_edge         axis-aligned poses at exactly minimal_distance (dropped) and one fp32 step above (kept);
    filter_edge_kept    the same path with the dropped poses removed by hand: the reference returns the same bytes
    cb_<shape>_<n>      count boundary: numpy's pairwise fp32 total and the running fp32 total give different counts;
    cb_levels_1026      the pairwise total with one recursion level fewer gives a different count
    small_<k><lo|hi>    total length just below / above k distance steps
    trim_<k>            reversing start, first change of direction at segment k; trim_backward, trim_end
    head_pi, head_turns, head_spin      headings at exactly +-pi and one fp32 step either side, several turns outside
                        (-pi, pi], steadily spinning
    scale_8000          coordinates near 8000, 1 m step
    degenerate, degenerate_control      minimal_distance 0: a nearly repeated pose whose 1e-6 + 1e-7 m segment rounds away
                        in the fp32 running sum (after 40 m) -> two equal parameter values; early in the path it does not
    collapse            every interior pose within minimal_distance of the goal
`cb_names`, `cb_k`: the count-boundary cases and the integer their totals straddle.

Initialiser: `init_cases` [C, 6] fp32 (start, goal), `init_case_names`, `init_full` (indices of the cases run at every
size of `init_sizes`; the others run at `init_sizes_small`); per case c and size N: `init_<c>_n<N>` [N, 3] fp32 from the
plain initialiser and `init_<c>_n<N>_dir` [N] fp32, the heading column with init_angles_with_trajectory (its xy are the
same linspace).  The reference has no 2-D initialiser of its own: a 2-D trajectory is the xy of these.

Usage:  MPLBACKEND=Agg python tests/golden/make_golden_path_tools.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402,F401  (installs the shims)
from make_golden import F32, Position2, TrajectoryInitializer  # noqa: E402
from neural_field_optimal_planner.ros.path_postprocessor import PathPostprocessor  # noqa: E402
from neural_field_optimal_planner.utils.math import wrap_angles  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402

PI, TWO_PI = F32(np.pi), F32(2 * np.pi)
LENGTHS = (3, 4, 5, 8, 9, 10, 129, 130, 131, 137, 138, 257, 258, 909, 910, 911, 1025, 1026)
PARKED_SEGMENTS = (7, 8, 9, 128, 129)
INIT_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1025)
INIT_SIZES_SMALL = (1, 2, 3, 4, 5, 257)


def up(x, k=1):
    """x moved by k fp32 steps (k < 0: down)"""
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


# ----------------------------------------------------------------------------------------------------------
# path builders
def curve(n, length=30.0, amp=2.0, waves=5.0, phase=0.4, noise=0.0, seed=0, origin=(1.0, -2.0)):
    """A sine path of n poses with the tangent heading (plus optional heading noise)."""
    s = np.linspace(0, 1, n)
    x, y = origin[0] + length * s, origin[1] + amp * np.sin(waves * s + phase)
    th = np.arctan2(amp * waves * np.cos(waves * s + phase), length)
    if noise:
        th = th + np.random.default_rng(seed).normal(0, noise, n)
    return np.stack([x, y, th], 1).astype(F32)


def straight(n, length=30.0, origin=(0.3, 0.7), angle=0.35):
    s = np.linspace(0, 1, n)
    x, y = origin[0] + length * np.cos(angle) * s, origin[1] + length * np.sin(angle) * s
    return np.stack([x, y, np.full(n, angle)], 1).astype(F32)


def segment_lengths(path, minimal_distance):
    """fp32 segment lengths of the filtered path, as the reference forms them (and the filtered path)."""
    md = F32(minimal_distance)
    keep, prev = [len(path) - 1], path[-1]
    for i in range(len(path) - 2, 0, -1):
        if np.linalg.norm(prev[:2] - path[i, :2]) > md:
            keep.append(i)
            prev = path[i]
    keep.append(0)
    tr = path[keep[::-1]]
    return np.linalg.norm(tr[1:, :2] - tr[:-1, :2], axis=1) + 1e-6, tr


def running_sum(a):
    acc = F32(0)
    for v in a:
        acc = F32(acc + v)
    return acc


def pairwise_sum_levels(a, levels):
    """numpy's pairwise order with the recursion cut after `levels` splits (4 reach blocks of <= 128 for 1025 terms)"""
    a = np.asarray(a, F32)
    if levels > 0 and len(a) > 128:
        n2 = len(a) // 2
        n2 -= n2 % 8
        return F32(pairwise_sum_levels(a[:n2], levels - 1) + pairwise_sum_levels(a[n2:], levels - 1))
    if len(a) < 8:
        return running_sum(a)
    r = [F32(a[j]) for j in range(8)]
    i = 8
    while i < len(a) - (len(a) % 8):
        for j in range(8):
            r[j] = F32(r[j] + a[i + j])
        i += 8
    s = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
    for v in a[i:]:
        s = F32(s + v)
    return s


def count_of(total, step):
    return int(F32(total) / F32(step))


def boundary_step(total_a, total_b, ks=range(40, 260)):
    """(step, k): an fp32 distance_step for which the two totals fall on opposite sides of the integer k."""
    for k in ks:
        for t in (total_a, total_b):
            for j in range(-4, 5):
                step = up(F32(t) / F32(k), j)
                ca, cb = count_of(total_a, step), count_of(total_b, step)
                if ca != cb and {ca, cb} == {k - 1, k}:
                    return step, k
    return None, None


def count_boundary_case(make, n, other_sum):
    """The first path of the family make(n, variant) whose numpy total and `other_sum` total differ, with such a step."""
    for variant in range(400):
        path = make(n, variant)
        dist, tr = segment_lengths(path, 0.001)
        assert len(tr) == n
        total = np.sum(dist)
        assert total == orc._pairwise_sum_f32(dist) and total.dtype == F32
        other = other_sum(dist)
        if other != total:
            step, k = boundary_step(total, other)
            if step is not None:
                return path, step, k
    raise AssertionError("no count-boundary path found for n = %d" % n)


def filter_edge_path():
    """Walked from the goal backwards: a pose at exactly 0.5 from the kept one (dropped), then one at nextafter(0.5, 1)
    (kept), alternately along x and y; coordinates stay below 1 so every difference is exact.  The second pose lies
    0.1 from the first.  Returns (path, mask of the poses the filter keeps)."""
    e = 2.0 ** -24
    back = [((0.75, 0.75), True),
            ((0.25, 0.75), False), ((0.25 + e / 2, 0.75), False),    # at 0.5, and one fp32 step below it
            ((0.25 - e, 0.75), True),                                # at nextafter(0.5, 1)
            ((0.25 - e, 0.25), False), ((0.25 - e, 0.25 - e), True),
            ((-0.25 - e, 0.25 - e), False), ((-0.25 - 2 * e, 0.25 - e), True),
            ((-0.25 - 2 * e, -0.25 - e), False), ((-0.25 - 2 * e, -0.25 - 2 * e), True),
            ((-0.875 - 2 * e, -0.25 - 2 * e), True),
            ((-1.0 - 2 * e, -0.25 - 2 * e), True)]                   # the first pose: kept unconditionally
    assert all(float(F32(v)) == v for p, _ in back for v in p)
    back = back[::-1]
    path = np.zeros((len(back), 3), F32)
    keep = np.asarray([k for _, k in back])
    for i, (p, k) in enumerate(back):
        path[i] = (p[0], p[1], 0.1 * i if k else 1.0 + 0.3 * i)
    dist = []
    prev = path[-1]
    for i in range(len(path) - 2, 0, -1):
        d = np.linalg.norm(prev[:2] - path[i, :2])
        dist.append(d)
        if keep[i]:
            prev = path[i]
    assert sum(d == F32(0.5) for d in dist) == 4 and sum(d == up(0.5) for d in dist) == 4, dist
    return path, keep


def reversing_start(back_len):
    """Drives backwards along -x over `back_len` metres with heading 0, then forwards for 3 m."""
    xs = np.concatenate([np.linspace(back_len, 0, 12)[:-1], np.linspace(0, 3, 40)])
    return np.stack([xs + 0.25, np.full(len(xs), 0.5), np.zeros(len(xs))], 1).astype(F32)


def exact_heading_jumps():
    """Headings whose WRAPPED values differ, pair by pair in fp32, by exactly pi, pi +- 1 step, -pi, -pi -+ 1 step
    (`(a + pi) % 2 pi - pi` rounds, so both headings of a pair are searched among their fp32 neighbours); between the
    pairs lies a pose with an ordinary heading.  Returns (headings, the differences hit)."""
    th, hit = [], []
    for sign in (1, -1):
        for t in (PI, up(PI, 1), up(PI, -1)):
            t = F32(sign * t)
            found = None
            for i in range(-16, 17):
                for j in range(-16, 17):
                    prev, cur = up(-0.5 * sign, i), up(F32(-0.5 * sign) + t, j)
                    if F32(orc.wrap_angle(cur) - orc.wrap_angle(prev)) == t:
                        found = found or (prev, cur)
            assert found is not None, t
            th += [found[0], found[1], F32(1.0 * sign)]
            hit.append(t)
    return np.asarray(th, F32), hit


def post_cases():
    """[(name, path, minimal_distance, distance_step)] and {count-boundary name: k}"""
    cases, cb = [], {}
    for n in LENGTHS:
        cases.append(("len_%d" % n, curve(n, noise=0.02, seed=n), 0.001, 0.25))
    for k in PARKED_SEGMENTS:
        p = curve(k + 1, length=12.0, amp=1.0, waves=3.0)
        j = (k + 1) // 2
        cases.append(("park_%d" % k, np.concatenate([p[:j], np.repeat(p[j:j + 1], 11, 0), p[j:]]), 0.001, 0.1))
    path, keep = filter_edge_path()
    cases.append(("filter_edge", path, 0.5, 0.05))
    cases.append(("filter_edge_kept", path[keep], 0.5, 0.05))
    # count boundary
    shapes = dict(straight=lambda n, v: straight(n, length=27.0 + 0.37 * v, angle=0.35 + 0.01 * v),
                  curved=lambda n, v: curve(n, length=24.0 + 0.41 * v, amp=1.5 + 0.05 * v, noise=0.01, seed=v))
    for shape, make in shapes.items():
        for n in (130, 258, 1026):
            path, step, k = count_boundary_case(make, n, running_sum)
            cases.append(("cb_%s_%d" % (shape, n), path, 0.001, float(step)))
            cb["cb_%s_%d" % (shape, n)] = k
    path, step, k = count_boundary_case(shapes["curved"], 1026, lambda d: pairwise_sum_levels(d, 3))
    cases.append(("cb_levels_1026", path, 0.001, float(step)))
    cb["cb_levels_1026"] = k
    # small counts
    p = np.asarray([[0.0, 0.0, 0.2], [0.4, 0.1, 0.3], [0.9, 0.3, 0.5], [1.3, 0.7, 0.6]], F32)
    total = float(np.sum(segment_lengths(p, 0.001)[0]))
    for k in (1, 2, 3):
        cases.append(("small_%dlo" % k, p, 0.001, float(F32(total / k * 1.001))))
        cases.append(("small_%dhi" % k, p, 0.001, float(F32(total / k * 0.999))))
    # trim
    pp = PathPostprocessor(minimal_distance=float(F32(0.001)), distance_step=float(F32(0.05)))
    for k in (1, 2, 5, 6, 7):
        # the backward stretch (in steps of 5 mm) for which the reference's first change of direction is segment k
        back_len = next(b for b in np.arange(0.02, 0.6, 0.005) if first_other_direction(pp, reversing_start(b)) == (k, True))
        cases.append(("trim_%d" % k, reversing_start(back_len), 0.001, 0.05))
    p = curve(60, length=6.0, amp=0.5, waves=3.0)
    p[:, 2] += 3.0                                                   # driven backwards throughout
    cases.append(("trim_backward", p, 0.001, 0.05))
    xs = np.concatenate([np.linspace(0, 3, 50), np.linspace(3, 2.8, 6)[1:]])
    cases.append(("trim_end", np.stack([xs, 0.2 * xs, np.full(len(xs), 0.197)], 1).astype(F32), 0.001, 0.05))
    # headings
    w, _ = exact_heading_jumps()
    th = np.concatenate([w, w[-1] + 0.05 * np.arange(1, 25)])
    xs = 0.5 * np.arange(len(th))
    cases.append(("head_pi", np.stack([xs, 0.1 * xs, th], 1).astype(F32), 0.001, 0.05))
    p = curve(90, length=9.0, amp=1.0, waves=4.0)
    p[:, 2] = (p[:, 2].astype(np.float64) + 2 * np.pi * np.random.default_rng(3).integers(-4, 5, 90)).astype(F32)
    cases.append(("head_turns", p, 0.001, 0.05))
    p = curve(131, length=13.0, amp=1.0, waves=2.0)
    p[:, 2] = np.remainder(0.5 * np.arange(131) + np.pi, 2 * np.pi) - np.pi    # 65 rad, handed over wrapped
    cases.append(("head_spin", p.astype(F32), 0.001, 0.1))
    # scale
    cases.append(("scale_8000", curve(300, length=290.0, amp=25.0, waves=6.0, origin=(7900.0, -8050.0)), 0.001, 1.0))
    # degenerate parametrisation (minimal_distance 0)
    for name, pos in (("degenerate", 58), ("degenerate_control", 2)):
        p = np.zeros((61, 3), F32)
        p[:60, 1], p[60, 1], p[:, 2] = np.linspace(0, 40, 60), 41.0, np.pi / 2
        p = np.insert(p, pos + 1, p[pos], axis=0)
        p[pos + 1, 0] = 1e-7
        dist, tr = segment_lengths(p, 0.0)
        cum = np.cumsum(dist)
        assert len(tr) == 62 and cum.dtype == F32 and (cum[pos] == cum[pos - 1]) == (name == "degenerate")
        cases.append((name, p, 0.0, 1.0))
    p = curve(9, length=2.0)
    p[1:-1, :2] = p[-1, :2] + np.asarray([3e-4, -2e-4], F32)
    cases.append(("collapse", p, 0.001, 0.05))
    return cases, cb


def first_other_direction(pp, path):
    """The reference's own first change of direction on its un-trimmed output, and whether no direction product among
    the first segments is near zero (the decision is unambiguous)."""
    tr = pp._filter_trajectory(path.copy())
    count = int(pp._calculate_total_distance(tr) / pp._distance_step)
    out = pp._reparametrize_trajectory(tr, pp._calculate_parametrization(tr), np.linspace(0, 1, count))
    if len(out) < 2:
        return None, True
    delta = out[1:, :2] - out[:-1, :2]
    mean = out[:-1, 2] + wrap_angles(out[1:, 2] - out[:-1, 2]) / 2
    dot = np.cos(mean) * delta[:, 0] + np.sin(mean) * delta[:, 1]
    other = np.nonzero((dot > 0) != (dot[0] > 0))[0]
    return (int(other[0]) if len(other) else None), bool(np.abs(dot[:8]).min() > 1e-7)


def generate_post(out):
    cases, cb = post_cases()
    names = []
    for name, path, md, step in cases:
        assert path.dtype == F32 and path.ndim == 2 and 3 <= len(path) <= 1026, name
        md, step = float(F32(md)), float(F32(step))
        pp = PathPostprocessor(minimal_distance=md, distance_step=step)
        names.append(name)
        out["post_%s_in" % name] = path
        out["post_%s_par" % name] = np.asarray([md, step], F32)
        try:
            res = np.asarray(pp.process(Position2.from_vec(path.copy())).as_vec())
        except Exception as e:
            out["post_%s_err" % name] = np.asarray(type(e).__name__)
            continue
        assert res.dtype == np.float64 and np.isfinite(res).all(), name
        out["post_%s_out" % name] = res.reshape(-1, 3)
        # the reference's own decisions are unambiguous: no direction product near zero among the first segments
        other, clear = first_other_direction(pp, path)
        assert clear, name
        if name.startswith("trim_") and name[5:].isdigit():
            assert other == int(name[5:]), (name, other)
        if name == "trim_backward":
            assert other is None
        if name == "trim_end":
            assert other is not None and other > 40
    assert np.array_equal(out["post_filter_edge_out"], out["post_filter_edge_kept_out"])
    assert str(out["post_degenerate_err"]) == "ValueError" and str(out["post_collapse_err"]) == "ValueError"
    out["post_names"] = np.asarray(names)
    out["cb_names"] = np.asarray(sorted(cb))
    out["cb_k"] = np.asarray([cb[k] for k in sorted(cb)], np.int32)


# ----------------------------------------------------------------------------------------------------------
def heading_goal(start_th, target):
    """A goal heading whose fp32 difference to start_th is exactly `target`."""
    for j in range(-8, 9):
        g = up(F32(F32(start_th) + target), j)
        if F32(g - F32(start_th)) == target:
            return g
    raise AssertionError("no goal heading %g from %g" % (target, start_th))


def init_cases():
    """([name], [C, 6] fp32, indices of the cases run at every size)"""
    c = [("generic", [0.5, 0.5, 0.3, 2.5, 1.5, -1.2]),
         ("far_wrapping", [3700.25, -9100.5, 2.9, -8800.75, 6400.125, -2.7])]
    s_th = F32(0.25)
    for tag, t in (("pi", PI), ("pi_up", up(PI, 1)), ("pi_down", up(PI, -1)), ("mpi", -PI), ("mpi_up", -up(PI, -1)),
                   ("mpi_down", -up(PI, 1))):
        c.append(("diff_" + tag, [0.4, 2.6, s_th, 2.7, 0.5, heading_goal(s_th, t)]))
    for k in (-3, -1, 1, 3):
        c.append(("diff_pi_turn%+d" % k, [0.4, 2.6, s_th, 2.7, 0.5, F32(np.float64(s_th) + np.pi + 2 * np.pi * k)]))
        c.append(("diff_mpi_turn%+d" % k, [0.4, 2.6, s_th, 2.7, 0.5, F32(np.float64(s_th) - np.pi + 2 * np.pi * k)]))
    c.append(("diff_pi_from_negative", [0.4, 2.6, -2.5, 2.7, 0.5, heading_goal(-2.5, PI)]))
    c.append(("diff_mpi_from_positive", [0.4, 2.6, 2.5, 2.7, 0.5, heading_goal(2.5, -PI)]))
    c += [("opposite_pi", [0.0, 0.0, PI, 2.0, 0.0, PI]),             # travel +x, heading pi: wrap(0 - pi)
          ("opposite_mpi", [0.0, 0.0, -PI, 2.0, 0.0, -PI]),          # wrap(0 + pi)
          ("opposite_back", [2.0, 0.0, 0.0, 0.0, 0.0, 0.0]),         # travel -x: atan2(+0, -) = pi
          ("minus_zero_y", [1.0, 0.0, 0.5, -1.0, -0.0, 0.5]),        # atan2(-0, -) = -pi next to the goal
          ("minus_zero_x", [0.0, 0.0, 0.2, -0.0, 2.0, 0.1]),         # atan2(+, -0)
          ("coincident", [1.0, 1.0, 0.3, 1.0, 1.0, -0.4]),           # atan2(0, 0)
          ("axis_up", [1.0, 0.0, 0.2, 1.0, 3.0, 0.1]),               # atan2(+, 0)
          ("axis_down", [1.0, 3.0, 0.2, 1.0, 0.0, 0.1]),             # atan2(-, 0)
          ("axis_right", [0.0, 1.0, 0.2, 3.0, 1.0, 0.1])]            # atan2(0, +)
    for tag, m in (("1e-3", 1e-3), ("1", 1.0), ("1e4", 1e4)):
        c.append(("magnitude_" + tag, [0.37 * m, 0.91 * m, 1.1, 0.83 * m, -0.29 * m, -0.6]))
    return [n for n, _ in c], np.asarray([v for _, v in c], F32), np.asarray([0, 1], np.int32)


def generate_init(out):
    names, cases, full = init_cases()
    out["init_case_names"], out["init_cases"], out["init_full"] = np.asarray(names), cases, full
    out["init_sizes"], out["init_sizes_small"] = np.asarray(INIT_SIZES, np.int32), np.asarray(INIT_SIZES_SMALL, np.int32)
    plain, directed = TrajectoryInitializer(None), TrajectoryInitializer(None, init_angles_with_trajectory=True)
    for c, case in enumerate(cases):
        for n in (INIT_SIZES if c in full else INIT_SIZES_SMALL):
            res = []
            for ti in (plain, directed):
                tr = torch.zeros(n, 3)
                with contextlib.redirect_stdout(io.StringIO()):
                    ti.initialize_trajectory(tr, torch.tensor(case[None, :3]), torch.tensor(case[None, 3:]))
                res.append(tr.numpy().copy())
            assert np.array_equal(res[0][:, :2], res[1][:, :2]) and np.isfinite(res[1]).all()
            out["init_%d_n%d" % (c, n)] = res[0]
            out["init_%d_n%d_dir" % (c, n)] = res[1][:, 2].copy()


if __name__ == "__main__":
    torch.set_num_threads(1)
    out = {}
    generate_post(out)
    generate_init(out)
    target = os.path.join(HERE, "g22_path_tools.npz")
    np.savez_compressed(target, **out)
    print("%-28s %8.1f KB, %d post-processor cases, %d initialiser cases" % (
        os.path.basename(target), os.path.getsize(target) / 1024, len(out["post_names"]), len(out["init_cases"])))
