"""What the generator, the CPU test and the GPU test of the reparametrisation's shape branches share: the cases (inputs built
from a per-case seed, never stored), the canonical digest of an array, access to tests/golden/g23_reparam_shapes.npz (written
by the reference itself, tests/golden/make_golden_reparam_shapes.py) and a numpy statement of the predicate by which
csrc/reparam.h chooses between its two float64 scans.

A case is (D, N, kind).  The sizes are those at which the kernel takes another branch ("Shape branches of the
reparametrisation"); the kinds:
    zigzag    uniform random waypoints in a 3 x 3 box, headings uniform in +-3.5
    smooth    unevenly spaced points on a curve, headings straddling +-pi (the "wrap" case of g4_reparam at every N)
    line      the initialiser's output: the fp32 linspace between start and goal, so every grid value ties with a cdf
              entry to within an ulp -- the first input of every real run
    dups      runs of identical waypoints: equal to the start at the beginning, in the middle, equal to the goal at the end
              (flat cdf runs, the 1e-5 clamp of the denominator)
    tinyseg   two consecutive waypoints at (0, 0) and (3e-9, 0): a non-zero quotient below 2^-29
    denormal  two consecutive waypoints 1e-20 apart in x only (dx*dx is an fp32 denormal, the segment's quotient lies far
              below 2^-29) and, from N = 6, a pair 1e-37 apart, whose squared difference underflows to zero
    onemove   every waypoint equal to the start, the goal one unit away: the cdf is 0, ..., 0, 1
    turns     (SE(2)) headings uniform in +-60 rad; on long segments, which the grid is certain to sample: consecutive
              headings that differ by exactly float32(pi), that are equal, that are -0.0 and 0.0, and that differ by the
              fp32 neighbours of -15 pi and 5 pi for which the device's floor(x / 2 pi) comes out one too large
    allsame   every xy equal: total length 0, the reference's output is all NaN
    overflow  one x coordinate of 2e19: dx*dx overflows, the total is inf
    nan       one NaN coordinate
    clamp     a path along x of length 1 + 2^-18 whose waypoints sit at the two ends of a step of 2^-18 placed around a grid
              value: that sample's denominator is positive and below the 1e-5 clamp (a flat run's never is: searchsorted
              steps over it)
    order     quotients 0.5, then a run of 2^-55 (steps up and down in y at x = 0), then 2^-25, then 0.5 - 2^-25; the total is
              exactly 1.  Walked in order, float64 drops every 2^-55 and the partial sum after the 2^-25 step is the fp32 tie
              0.5 + 2^-25, which rounds down; a scan that adds the small ones to each other first lands above the tie.  The
              one case whose OUTPUT depends on the sequential scan being taken (tinyseg's float64 sums differ between the
              scans as well, but nowhere near a rounding boundary of fp32)

NaN payload and sign and the sign of a zero are outside the contract (the digest maps them to one NaN and to +0.0);
every other bit is inside it."""
import hashlib

import numpy as np

from conftest import load_golden
from oracle import nfopp_oracle as orc

F32 = np.float32
FIXTURE = "g23_reparam_shapes.npz"
SIZES_COMMON = (2, 3, 6, 7, 8, 14, 15, 16, 100, 255, 256, 257, 510, 511, 512, 513, 700, 1023, 1024)
# (exactly 64 KB of LDS, the first size above it, the last size that fits into 160 KB), per D
SIZES = {3: SIZES_COMMON + (2336, 2337, 5846), 2: SIZES_COMMON + (2725, 2726, 6821)}
FIRST_REFUSED = {3: 5847, 2: 6822}
KINDS = ("zigzag", "smooth", "line", "dups", "tinyseg", "denormal", "onemove", "turns", "allsame", "overflow", "nan",
         "clamp", "order")
SEQUENTIAL_KINDS = ("tinyseg", "denormal", "allsame", "overflow", "nan", "order")
NONFINITE_KINDS = ("allsame", "overflow", "nan")
STORED_MAX_N = 257                 # the fixture holds the reference's output arrays up to this N, digests for every N
INPUTS = ("traj", "start", "goal", "lam", "cm")
OUTPUTS = ("traj", "lam", "cm")
TWO_POW_M29 = F32(2.0 ** -29)

# `turns`: the wrapped differences of the special pairs, in the order they are placed
TURN_NEG_15PI = F32(-47.12389373779297)     # a + pi = -14 * 2 pi - 1 step: floor((a + pi) * (1 / 2 pi)) = -14, not -15
TURN_POS_5PI = F32(15.707962989807129)      # a + pi = 3 * 2 pi - 1 step: floor gives 3, not 2
TURN_PAIRS = ("pi", "equal", "minus_zero", "neg_15pi", "pos_5pi")


def kinds(d):
    return tuple(k for k in KINDS if d == 3 or k != "turns")


def all_cases():
    return [(d, n, kind) for d in (3, 2) for n in SIZES[d] for kind in kinds(d)]


def case_name(d, n, kind):
    return "d%d_n%d_%s" % (d, n, kind)


def lds_bytes(n, d):
    """reparam_lds_bytes of csrc/reparam.h"""
    return ((n + 2) * d + 3 * (n + 2) + n + 8 + 12) * 4


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _pair_with_difference(first, diff):
    """An fp32 heading `second` with float32(second - first) == diff exactly."""
    first, diff = F32(first), F32(diff)
    guess = F32(first + diff)
    for j in range(-8, 9):
        second = guess
        for _ in range(abs(j)):
            second = np.nextafter(second, F32(np.inf if j > 0 else -np.inf))
        if F32(second - first) == diff:
            return second
    raise AssertionError("no heading %r away from %r" % (diff, first))


def turn_pair_waypoints(n):
    """Waypoint indices p of the special pairs (p, p + 1) of `turns`, as many of TURN_PAIRS as fit into n waypoints."""
    step = max(3, n // 5)
    return [k * step for k in range(len(TURN_PAIRS)) if k * step + 1 < n]


def make_case(d, n, kind):
    """dict(traj [n, d], start [d], goal [d], lam [n + 1], cm [n]) in fp32; lam and cm are None for d = 2."""
    rng = np.random.default_rng([d, n, KINDS.index(kind)])
    tr = np.empty((n, 3), F32)
    tr[:, :2] = rng.uniform(0, 3, (n, 2))
    tr[:, 2] = rng.uniform(-3.5, 3.5, n)
    start = np.concatenate([rng.uniform(0, 3, 2), rng.uniform(-3.1, 3.1, 1)]).astype(F32)
    goal = np.concatenate([rng.uniform(0, 3, 2), rng.uniform(-3.1, 3.1, 1)]).astype(F32)
    lam = rng.normal(0, 0.3, n + 1).astype(F32)
    cm = rng.uniform(0, 0.2, n).astype(F32)
    mid = (n - 1) // 2
    if kind == "smooth":
        s = np.sort(rng.uniform(0, 1, n)).astype(F32)
        tr[:, 0], tr[:, 1] = F32(0.5) + F32(2) * s * s, F32(0.5) + s
        tr[:, 2] = orc.wrap_angle(np.linspace(2.6, 3.9, n).astype(F32))
        start, goal = np.asarray([0.5, 0.5, 2.6], F32), np.asarray([2.5, 1.5, orc.wrap_angle(F32(3.9))], F32)
    elif kind == "line":
        start[:2], goal[:2] = F32(0.2) + start[:2] / F32(5), F32(2.2) + goal[:2] / F32(5)
        tr = orc.initialize_trajectory(start, goal, n)
    elif kind == "dups":
        k = max(1, n // 20)
        tr[:k], tr[n - k:] = start, goal
        a = n // 3
        b = min(a + max(2, n // 5), n - k)
        if a >= k and b > a:
            tr[a:b] = tr[a]
    elif kind == "tinyseg":
        start[:2], goal[:2] = F32(1) + start[:2] * F32(2.0 / 3), F32(1) + goal[:2] * F32(2.0 / 3)   # path length > 2.8
        tr[mid, :2], tr[mid + 1, :2] = (0.0, 0.0), (3e-9, 0.0)
    elif kind == "denormal":
        tr[mid, :2], tr[mid + 1, :2] = (0.0, 1.5), (1e-20, 1.5)
        if n >= 6:
            tr[0, :2], tr[1, :2] = (0.0, 0.5), (1e-37, 0.5)
    elif kind == "onemove":
        start[:2] = F32(0.5) + np.floor(start[:2] * F32(16)) / F32(32)      # on a 1/32 grid: the unit step is exact
        tr[:] = start
        goal[:2] = start[:2] + np.asarray([1.0, 0.0], F32)
    elif kind == "turns":
        tr[:, 2] = rng.uniform(-60, 60, n)
        for k, p in enumerate(turn_pair_waypoints(n)):
            tr[p, :2], tr[p + 1, :2] = (0.1, 0.1 + 0.01 * k), (2.9, 2.9 - 0.01 * k)     # a long segment: sampled for sure
            tag = TURN_PAIRS[k]
            if tag == "pi":
                tr[p, 2] = 0.5
                tr[p + 1, 2] = _pair_with_difference(0.5, orc.PI)
            elif tag == "equal":
                tr[p + 1, 2] = tr[p, 2]
            elif tag == "minus_zero":
                tr[p, 2], tr[p + 1, 2] = -0.0, 0.0
            elif tag == "neg_15pi":
                tr[p, 2] = 20.0
                tr[p + 1, 2] = _pair_with_difference(20.0, TURN_NEG_15PI)
            else:
                tr[p, 2] = -10.0
                tr[p + 1, 2] = _pair_with_difference(-10.0, TURN_POS_5PI)
    elif kind == "allsame":
        tr[:, :2], start[:2], goal[:2] = (1.25, 0.75), (1.25, 0.75), (1.25, 0.75)
    elif kind == "overflow":
        tr[n // 2, 0] = 2e19
    elif kind == "nan":
        tr[n // 2, 1] = np.nan
    elif kind == "clamp":
        m, eps = max(1, n // 2), 2.0 ** -18
        u = np.float64(orc.linspace_f32(0, 1, n + 2)[1:-1][n // 2])
        c = F32(u * (1 + eps) - eps / 2)
        tr[:, 1], start[1], goal[1] = 0.75, 0.75, 0.75
        start[0], tr[:m, 0], tr[m:, 0], goal[0] = 0.0, c, F32(c + F32(eps)), 1 + eps
    elif kind == "order":
        k = max(0, min(n - 2, max(8, 4 * ((n + 256) // 256)))) // 2 * 2          # an even number of 2^-55 steps
        tr[:, :2], start[:2], goal[:2] = (0.5, 0.0), (-0.5, 0.0), (0.5, 0.0)       # waypoints not needed wait at the goal
        tr[:k + 1, 0] = 0.0
        tr[1:k + 1:2, 1] = 2.0 ** -55
        if n >= 2:
            tr[k + 1, :2] = (2.0 ** -25, 0.0)
    elif kind != "zigzag":
        raise ValueError(kind)
    if d == 2:
        return dict(traj=np.ascontiguousarray(tr[:, :2]), start=start[:2].copy(), goal=goal[:2].copy(), lam=None, cm=None)
    return dict(traj=tr, start=start, goal=goal, lam=lam, cm=cm)


# ---- digest -----------------------------------------------------------------------------------------------------------
def canonical(a):
    """fp32 copy with every NaN replaced by one NaN and -0.0 by +0.0"""
    a = np.array(a, dtype="<f4", copy=True)
    a[np.isnan(a)] = np.nan
    a[a == 0] = 0.0
    return np.ascontiguousarray(a)


def digest(a):
    """sha256 of the canonical fp32 bytes, as uint8 [32]; zeros for an absent array"""
    if a is None:
        return np.zeros(32, np.uint8)
    return np.frombuffer(hashlib.sha256(canonical(a).tobytes()).digest(), np.uint8).copy()


def same(a, b):
    """equal in every bit the contract covers"""
    return np.array_equal(canonical(a), canonical(b), equal_nan=True)


def first_difference(a, b):
    """for messages: (flat index, a there, b there) of the first element that differs, or None"""
    a, b = canonical(a).reshape(-1), canonical(b).reshape(-1)
    bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
    return None if len(bad) == 0 else (int(bad[0]), float(a[bad[0]]), float(b[bad[0]]), len(bad))


# ---- the kernel's choice of scan --------------------------------------------------------------------------------------
def quotients(case):
    """(fp32 quotients [N + 1], fp32 total) as csrc/reparam.h and the reference form them"""
    q = orc.full_trajectory(case["traj"][None], case["start"][None], case["goal"][None])[0]
    with np.errstate(all="ignore"):
        seg = (q[1:, :2] - q[:-1, :2]).astype(F32)
        dist = orc.torch_norm2_f32(seg[:, 0], seg[:, 1])
        total = orc.torch_sum_f32(dist)
        return (dist / total).astype(F32), total


def takes_parallel_scan(case):
    """The `exact` predicate of reparam_from_lds: total positive and finite, every quotient in [0, 1], the smallest
    non-zero one at least 2^-29.  False: one lane walks the sequence."""
    q, total = quotients(case)
    if not (total > 0 and total < F32(3.0e38)):
        return False
    if not bool(np.all((q >= 0) & (q <= 1))):
        return False
    nz = q[q != 0]
    return bool(min(F32(1), nz.min() if len(nz) else F32(1)) >= TWO_POW_M29)


def sequential_cdf(q):
    """torch.cumsum on CPU: a float64 accumulator walks the fp32 quotients, every partial sum rounded to fp32"""
    return np.concatenate([np.zeros(1, F32), np.cumsum(np.asarray(q, F32).astype(np.float64)).astype(F32)])


def parallel_cdf(q, threads=256, wave=64):
    """The cdf as the parallel scan of reparam_from_lds forms it, whatever the predicate says: per-thread sums of
    ceil(len / 256) consecutive quotients, an inclusive shuffle scan inside each wave, the earlier waves' totals added
    in order, then each thread walks its own quotients.  Equal to sequential_cdf wherever the predicate holds."""
    q = np.asarray(q, F32).astype(np.float64)
    n_el = len(q)
    per = (n_el + threads - 1) // threads
    chunks = [q[t * per:min(t * per + per, n_el)] for t in range(threads)]
    part = np.zeros(threads)
    for t, c in enumerate(chunks):
        for v in c:
            part[t] = part[t] + v
    incl = part.copy()
    lane = np.arange(threads) % wave
    o = 1
    while o < wave:
        up = np.concatenate([np.zeros(o), incl[:-o]])
        incl = np.where(lane >= o, incl + up, incl)
        o *= 2
    totals = incl[wave - 1::wave]
    cdf = np.zeros(n_el + 1, F32)
    for t, c in enumerate(chunks):
        run = incl[t] - part[t]
        for w2 in range(t // wave):
            run = run + totals[w2]
        for j, v in enumerate(c):
            run = run + v
            cdf[1 + t * per + j] = F32(run)
    return cdf


# ---- oracle and fixture -----------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_outputs(d, n, kind, case=None):
    """dict(traj, lam, cm) of oracle.reparametrize on the case; computed once per process"""
    key = (d, n, kind)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_apply(case or make_case(d, n, kind))
    return _ORACLE[key]


def oracle_apply(case):
    with np.errstate(all="ignore"):
        if case["lam"] is None:
            out = dict(traj=orc.reparametrize(case["traj"][None], case["start"][None], case["goal"][None])[0], lam=None,
                       cm=None)
        else:
            tr, lam, cm = orc.reparametrize(case["traj"][None], case["start"][None], case["goal"][None], case["lam"][None],
                                            case["cm"][None])
            out = dict(traj=tr[0], lam=lam[0], cm=cm[0])
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


_Z = None


def fixture():
    global _Z
    if _Z is None:
        z = load_golden(FIXTURE)
        _Z = {k: z[k] for k in z.files}
        _Z["index"] = {str(name): i for i, name in enumerate(_Z["names"])}
        for v in _Z.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _Z


def fixture_digests(d, n, kind):
    """(inputs {name: uint8 [32]}, outputs {name: uint8 [32]}) recorded for the case"""
    z = fixture()
    i = z["index"][case_name(d, n, kind)]
    return ({k: z["in_digest"][i, j] for j, k in enumerate(INPUTS)}, {k: z["out_digest"][i, j] for j, k in enumerate(OUTPUTS)})


def fixture_arrays(d, n, kind):
    """dict(traj, lam, cm) of the reference's output arrays, or None above STORED_MAX_N"""
    if n > STORED_MAX_N:
        return None
    z = fixture()
    k = kinds(d).index(kind)
    return {name: (z["d%d_n%d_%s" % (d, n, name)][k] if d == 3 or name == "traj" else None) for name in OUTPUTS}
