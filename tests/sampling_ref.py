"""Plain float64 reference of the training-pose sampler and the pool resampling (csrc/sampling.hip), independent of the
kernel's Philox layout: the reference's weights and its `np.random.choice(p=w, replace=False)` (nfop/nerf_opt_planner.py:
122-133), restated with numpy alone.  It holds no generator of its own; where a test needs the kernel's uniforms it
takes them from `oracle.draw_uniform`, which the Random123 known answers pin (tests/test_sampling_oracle.py).

Also the statistics shared by the CPU tests (on the fp32 oracle and its mutants, tests/test_sampling_ref_cpu.py) and the
GPU tests (on the kernels, tests/test_gpu_sampling_reference.py), and the shapes both run, so that the CPU evidence of a
gate's power speaks about the very case the GPU runs.
"""
import itertools
import math

import numpy as np

DECAY = 0.03          # nerf_opt_planner.py:126
WEIGHT_FLOOR = 1e-6   # nerf_opt_planner.py:126

# gates (conditions set before anything was measured)
Z_GATE = 5.0          # standardised difference of a frequency / two-sample z of a mean
KS_GATE = 2.69        # sqrt(n) * Kolmogorov-Smirnov distance at the 1e-6 level (2 exp(-2 x^2) = 1e-6)
CORR_GATE = 5.0       # sqrt(n) * sample correlation
Z_MAX = math.sqrt(-2.0 * math.log(2.0 ** -24))   # largest |Box-Muller value| from a 24-bit uniform: 5.768

# Relative band of the fp32 race key  -log(u) / (sigmoid(logit) * exp(-0.03 age) + 1e-6)  around its float64 value.
# Derived from the kernel's operations, in units of 2^-23 (one fp32 ulp, relative), with the bounds of the HIP math
# documentation (expf 1 ulp, logf 1 ulp; + - * / correctly rounded, half an ulp; u = 1 - m 2^-24 and -logit are exact):
#   sigmoid: expf 1 + sum 0.5 + reciprocal 0.5;  decay: the product -0.03f * age is rounded and 0.03f is not 0.03, each
#   at most 2^-24 of an argument of at most 9 (age 300): 9 in all, + expf 1;  product 0.5;  + 1e-6f 0.5;  logf 1;
#   division 0.5  ->  14.5 * 2^-23 = 1.73e-6.
# Measured on the CPU between the fp32 numpy oracle and race_keys64 over the shapes of the selection test: 9.3e-7
# (tests/test_sampling_ref_cpu.py asserts it stays below the derived bound).  TAU = 4 x the larger of the two.
TAU_DERIVED = 14.5 * 2.0 ** -23
TAU = 4.0 * TAU_DERIVED

# distribution cases of the resampling: (C, cap, seed of logits / ages, kernel seed, rng_offset, traj_index_offset)
DISTRIBUTION_CASES = [(8, 3, 0, 99, 0, 0), (12, 5, 0, 99, 0, 0), (8, 3, 1, 99, 1000, 1 << 20), (12, 5, 1, 99, 1000, 1 << 20)]
DISTRIBUTION_B = 65536

# age dynamics (statistics): a first step of AGE_N - 1 new candidates fills the pool, every later step offers the pool
# plus AGE_NEW new candidates (fewer than pool slots, so poses stay long enough for the age decay to matter)
AGE_N, AGE_CAP, AGE_NEW, AGE_STEPS, AGE_B_DEV, AGE_B_REF = 33, 32, 2, 60, 4096, 1500


def weights64(logit, age, normalise=True, decay=DECAY, floor=WEIGHT_FLOOR):
    """sigmoid(logit) * exp(-decay age) + floor in float64 (nerf_opt_planner.py:125-126), normalised over the last
    axis like :127 unless told otherwise."""
    logit, age = np.asarray(logit, np.float64), np.asarray(age, np.float64)
    with np.errstate(over="ignore"):
        w = 1.0 / (1.0 + np.exp(-logit)) * np.exp(-decay * age) + floor
    return w / w.sum(-1, keepdims=True) if normalise else w


def race_keys64(u, w):
    """Exponential-race keys -log(u) / w in float64 from given uniforms in (0, 1]."""
    return -np.log(np.asarray(u, np.float64)) / np.asarray(w, np.float64)


def inclusion_exact(w, cap):
    """Sequential weighted draws without replacement (what np.random.choice(p=w, replace=False) samples), by
    enumeration of every ordered tuple -> (first-order inclusion probabilities [C], pairwise inclusion [C, C], law of
    the first pick [C])."""
    w = np.asarray(w, np.float64)
    w = w / w.sum()
    C = len(w)
    assert math.perm(C, cap) <= 95040, "enumeration is meant for C of 8 to 12 and cap of 3 to 5"
    tuples = np.array(list(itertools.permutations(range(C), cap)), np.int64)      # [T, cap]
    wt = w[tuples]
    left = 1.0 - np.concatenate([np.zeros((len(tuples), 1)), np.cumsum(wt, 1)[:, :-1]], 1)
    prob = np.prod(wt / left, 1)
    assert abs(prob.sum() - 1.0) < 1e-12
    member = np.zeros((len(tuples), C))
    np.put_along_axis(member, tuples, 1.0, 1)
    first = member.T @ prob
    pair = (member * prob[:, None]).T @ member
    first_pick = np.bincount(tuples[:, 0], weights=prob, minlength=C)
    return first, pair, first_pick


def choice_simulation(n_traj, steps, cap, n_first, n_new, seed, logit=0.0):
    """The reference's loop (nerf_opt_planner.py:122-133) over `steps` steps for `n_traj` independent trajectories, with
    one constant logit so that only the ages drive the weights: candidates = [pool | new (age 0)], weights normalised,
    np.random.RandomState.choice(replace=False, p=w), age + 1.  -> pool ages after the last step [n_traj, cap]."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n_traj, cap))
    for b in range(n_traj):
        pool_age = np.zeros(0)
        for k in range(steps):
            cand_age = np.concatenate([pool_age, np.zeros(n_first if k == 0 else n_new)])
            w = weights64(np.full(len(cand_age), logit), cand_age)
            pool_age = cand_age[rs.choice(len(cand_age), cap, replace=False, p=w)] + 1
        out[b] = pool_age
    return out


# ---- statistics ------------------------------------------------------------------------------------------------------
def standardised(freq, p, n):
    """(f - p) / sqrt(p (1 - p) / n)"""
    freq, p = np.asarray(freq, np.float64), np.asarray(p, np.float64)
    return (freq - p) / np.sqrt(p * (1.0 - p) / n)


def inclusion_statistics(chosen, w, cap):
    """chosen [B, cap] indices in pool order -> standardised differences to `inclusion_exact`: (first-order [C],
    first pick [C], pairwise [C (C - 1) / 2])."""
    chosen = np.asarray(chosen)
    B, C = len(chosen), len(w)
    first, pair, first_pick = inclusion_exact(w, cap)
    member = np.zeros((B, C))
    np.put_along_axis(member, chosen, 1.0, 1)
    iu = np.triu_indices(C, 1)
    z1 = standardised(member.mean(0), first, B)
    z0 = standardised(np.bincount(chosen[:, 0], minlength=C) / B, first_pick, B)
    z2 = standardised((member.T @ member / B)[iu], pair[iu], B)
    return z1, z0, z2


def two_sample_z(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))


def normal_cdf(x):
    from scipy.special import ndtr
    return ndtr(x)


def ks_sqrt_n(values, cdf):
    """sqrt(n) * sup |F_n - F| of a sample against a continuous law"""
    x = np.sort(np.asarray(values, np.float64).ravel())
    n = len(x)
    f = cdf(x)
    d = max(np.max(np.arange(1, n + 1) / n - f), np.max(f - np.arange(0, n) / n))
    return float(d * math.sqrt(n))


def corr_sqrt_n(a, b):
    """sqrt(n) * sample correlation of two equally long samples"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(len(a) ** 0.5 * (a @ b) / math.sqrt((a @ a) * (b @ b)))


def offset_correlations(zc, zf, t, zc_next=None):
    """The correlations of item 5c on recovered standard normals zc / zf [B, N - 1, D] (course / fine), the
    interpolation draws t [B, N - 1] and, if given, the course set of the next rng_offset.  -> {name: sqrt(n) * r}"""
    D = zc.shape[2]
    out = {"course~fine": corr_sqrt_n(zc, zf)}
    for name, z in (("course", zc), ("fine", zf)):
        out[name + " x~y"] = corr_sqrt_n(z[..., 0], z[..., 1])
        if D == 3:
            out[name + " x~theta"] = corr_sqrt_n(z[..., 0], z[..., 2])
            out[name + " y~theta"] = corr_sqrt_n(z[..., 1], z[..., 2])
        out[name + " j~j+1"] = corr_sqrt_n(z[:, :-1], z[:, 1:])
        out[name + " b~b+1"] = corr_sqrt_n(z[:-1], z[1:])
        out[name + " ~t"] = corr_sqrt_n(z, np.repeat(t[..., None], D, 2))
        # the pair of uniforms behind one normal is (2 i, 2 i + 1): a value against its neighbour along d catches a
        # shifted second uniform
        out[name + " d~d+1 flat"] = corr_sqrt_n(z.reshape(len(z), -1)[:, :-1], z.reshape(len(z), -1)[:, 1:])
    if zc_next is not None:
        out["offset k~k+1"] = corr_sqrt_n(zc, zc_next)
    return out


# ---- inputs shared by the CPU and GPU tests ----------------------------------------------------------------------------
def oracle_uniforms(seed, traj_index_offset, batch, n, offset, stream):
    """[batch, n] uniforms of the kernel's counter layout (trajectory traj_index_offset + b, draw index 0..n-1), from the
    oracle's Philox restatement, which the Random123 known answers pin."""
    from oracle import nfopp_oracle as orc
    idx = np.broadcast_to(np.arange(n, dtype=np.uint64), (batch, n))
    traj = (np.uint64(traj_index_offset) + np.arange(batch, dtype=np.uint64))[:, None]
    return orc.draw_uniform(seed, traj, idx, offset, stream)


def resample_inputs(batch, n_cand, seed):
    """Logits spread over [-30, 30] with a few at -100 / +100 (expf overflows: weight 1e-6, and about 1), integer ages
    in [0, 300] -> (logit [B, C] fp32, age [B, C] fp32)"""
    rng = np.random.default_rng(seed)
    logit = rng.uniform(-30, 30, (batch, n_cand)).astype(np.float32)
    special = rng.uniform(size=(batch, n_cand))
    logit[special < 0.02] = -100.0
    logit[special > 0.98] = 100.0
    age = rng.integers(0, 301, (batch, n_cand)).astype(np.float32)
    return logit, age


def distribution_inputs(n_cand, seed):
    """logits normal(0, 2), integer ages in [0, 40) of one candidate set (item 3c)"""
    rng = np.random.default_rng(seed)
    return rng.normal(0, 2, n_cand).astype(np.float32), rng.integers(0, 40, n_cand).astype(np.float32)


def lerp64(prev, t):
    """nerf_opt_planner.py:117  traj[1:] * (1 - t) + traj[:-1] * t  in float64; prev [B, N, D], t [B, N - 1]"""
    prev, t = np.asarray(prev, np.float64), np.asarray(t, np.float64)[..., None]
    return prev[:, 1:] * (1.0 - t) + prev[:, :-1] * t


def recover_offsets(prev, t, course, fine, course_sigma, fine_sigma, angle_sigma):
    """z = (pose - lerp) / sigma per coordinate (constrained_nerf_opt_planner.py:57-61: theta uses angle_sigma in both
    sets) -> (z_course, z_fine) float64 [B, N - 1, D]"""
    D = np.asarray(prev).shape[2]
    pos = lerp64(prev, t)
    sc = np.array([course_sigma, course_sigma, angle_sigma][:D], np.float64)
    sf = np.array([fine_sigma, fine_sigma, angle_sigma][:D], np.float64)
    return (np.asarray(course, np.float64) - pos) / sc, (np.asarray(fine, np.float64) - pos) / sf
