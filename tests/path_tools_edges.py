"""What the CPU and GPU edge tests of the path post-processor and the trajectory initialiser share: access to the cases of
tests/golden/g22_path_tools.npz (written by the reference itself, tests/golden/make_golden_path_tools.py), the fp32 sums
the count-boundary cases are built on, and the tolerances.

Tolerances.  Post-processor poses are float64: SPREAD_* is the measured distance of the oracle's restatement
(elimination without pivoting) from the reference's output (scipy: LAPACK gbsv), max over the fixture's cases of
|oracle - reference| / max(1, max |pose coordinate|), separately for xy and heading; tests/test_path_tools_edges_cpu.py
holds the oracle to them.  Both maxima come from `degenerate_control`, whose two sites 2.4e-8 apart make the collocation
matrix nearly singular; every other case stays below 4e-16.  The device is held to 16 x SPREAD (its division and fmod are
IEEE, the margin is for their order), capped at the 1e-11 the g12 test uses.
Directed initialiser headings are fp32 and differ by the atan2 implementation (torch: Sleef, device: ocml, both within
1 ulp of a result of magnitude <= pi, so <= 2 ulp(pi) apart); the difference can then cross one more rounding step in each
of `heading - th` and the sum with th (magnitudes up to 2 pi, steps of 2 ulp(pi), halved by round-to-nearest): 4 steps of
the larger of pi and the largest heading of the case.  xy and the plain headings are bit for bit."""
import numpy as np

from conftest import load_golden

F32 = np.float32
FIXTURE = "g22_path_tools.npz"
SPREAD_XY = 2.5e-13          # measured 2.47e-13 (degenerate_control; next: 3.5e-16)
SPREAD_TH = 1.4e-13          # measured 1.31e-13 (degenerate_control; next: 2.0e-16)
DEVICE_MARGIN = 16.0
REL_CAP = 1e-11

LENGTHS = (3, 4, 5, 8, 9, 10, 129, 130, 131, 137, 138, 257, 258, 909, 910, 911, 1025, 1026)
PARKED_SEGMENTS = (7, 8, 9, 128, 129)
INIT_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1025)

_Z = None


def fixture():
    global _Z
    if _Z is None:
        z = load_golden(FIXTURE)
        _Z = {k: z[k] for k in z.files}      # read once, shared by every test of the process
        for v in _Z.values():
            v.setflags(write=False)
    return _Z


def post_names():
    return [str(n) for n in fixture()["post_names"]]


def post_case(name):
    """(path [n, 3] fp32, minimal_distance, distance_step, expected float64 poses or None, exception class name or None)"""
    z = fixture()
    par = z["post_%s_par" % name]
    err = z.get("post_%s_err" % name)
    return (z["post_%s_in" % name], float(par[0]), float(par[1]), z.get("post_%s_out" % name),
            None if err is None else str(err))


def scale_of(want):
    return max(1.0, float(np.abs(want).max())) if want.size else 1.0


def device_tol(want):
    """(xy, heading) absolute tolerances of the device against the fixture's poses `want`"""
    s = scale_of(want)
    return min(DEVICE_MARGIN * SPREAD_XY, REL_CAP) * s, min(DEVICE_MARGIN * SPREAD_TH, REL_CAP) * s


def filtered_segment_lengths(path, minimal_distance):
    """fp32 segment lengths (+ 1e-6) of the path after the backwards filter, every operation rounded on its own."""
    path, md = np.asarray(path, F32), F32(minimal_distance)
    keep, prev = [len(path) - 1], path[-1]
    for i in range(len(path) - 2, 0, -1):
        dx, dy = F32(prev[0] - path[i, 0]), F32(prev[1] - path[i, 1])
        if np.sqrt(F32(F32(dx * dx) + F32(dy * dy))) > md:
            keep.append(i)
            prev = path[i]
    keep.append(0)
    tr = path[keep[::-1]]
    seg = (tr[1:, :2] - tr[:-1, :2]).astype(F32)
    return (np.sqrt((seg[:, 0] * seg[:, 0] + seg[:, 1] * seg[:, 1]).astype(F32)) + F32(1e-6)).astype(F32)


def running_sum_f32(a):
    acc = F32(0)
    for v in np.asarray(a, F32):
        acc = F32(acc + v)
    return acc


def pairwise_sum_f32_levels(a, levels):
    """numpy's pairwise order with the recursion cut after `levels` splits: a block that is still longer than 128 is
    then summed as one (8 partial sums + tail).  4 levels are numpy for up to 1025 terms."""
    a = np.asarray(a, F32)
    if levels > 0 and len(a) > 128:
        n2 = len(a) // 2
        n2 -= n2 % 8
        return F32(pairwise_sum_f32_levels(a[:n2], levels - 1) + pairwise_sum_f32_levels(a[n2:], levels - 1))
    if len(a) < 8:
        return running_sum_f32(a)
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
    """int(total / distance_step) as numpy evaluates it for an fp32 total and a python float step: one fp32 division"""
    return int(F32(F32(total) / F32(step)))


def init_cases(n):
    """(names, [C, 6] fp32 cases, plain [C, n, 3] fp32, directed headings [C, n] fp32) of the cases recorded at size n"""
    z = fixture()
    idx = [c for c in range(len(z["init_cases"])) if "init_%d_n%d" % (c, n) in z]
    return ([str(z["init_case_names"][c]) for c in idx], z["init_cases"][idx],
            np.stack([z["init_%d_n%d" % (c, n)] for c in idx]), np.stack([z["init_%d_n%d_dir" % (c, n)] for c in idx]))


def init_heading_tol(plain, directed):
    """per case [C]: 4 fp32 steps at the larger of pi and the largest heading of the case"""
    big = np.maximum(np.abs(plain[..., 2]).max(1), np.abs(directed).max(1))
    return 4.0 * np.spacing(np.maximum(big, F32(np.pi)).astype(F32)).astype(np.float64)
