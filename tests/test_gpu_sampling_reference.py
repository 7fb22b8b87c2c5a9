"""GPU tests of `sample_candidates_kernel` and `resample_pool_kernel` (csrc/sampling.hip) against the reference's
semantics, through the C ABI: a float64 evaluation of the race keys, the exact law of numpy's sequential weighted
draws without replacement (enumerated), numpy's own `choice` for the age dynamics, and N(0, 1) / uniform laws for the
offsets and field poses (tests/sampling_ref.py).  The only thing taken from the oracle is the uniform stream, which the
Random123 known answers pin on both sides (tests/test_sampling_oracle.py, test_philox_known_answers_on_the_device).
tests/test_sampling_ref_cpu.py runs the same statistics on the fp32 oracle and on mutants of it: the gates used here
pass the first and reject every one of the second.

Not covered: the kernel's rule for EXACTLY equal keys (lower index first).  A key is -log(u) / w with u = 1 - philox in
(0, 1]; two equal keys in one trajectory need either u == 1 twice (2^-24 per draw) or an accidental collision of two
fp32 quotients, and neither can be arranged through the ABI without searching the generator's output, which these tests
do not do.  The near-tie band of the selection test says what may differ from the float64 order instead.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
import sampling_ref as ref  # noqa: E402
from nfopp import _lib  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402

F32 = np.float32
SENTINEL = F32(-12345.5)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def f4(values):
    return (ctypes.c_float * 4)(*[float(v) for v in values])


def resample(B, n_cand, cand_stride, cap, D, sample_stride, sample_off, seed, offset, tio, cand, age, out4, pool, pool_age,
             samples):
    _lib.check(_lib.load().nfopp_resample_pool(B, n_cand, cand_stride, cap, D, sample_stride, sample_off, seed, offset, tio,
                                               _lib.ptr(cand), _lib.ptr(age), _lib.ptr(out4), _lib.ptr(pool),
                                               _lib.ptr(pool_age), _lib.ptr(samples), _lib.stream_ptr()))
    torch.cuda.synchronize()


def sample(prev, cap, pool_count, n_field, sigmas, bounds, seed, offset, tio, pool, pool_age, cand, cand_age, samples):
    B, N, D = prev.shape
    _lib.check(_lib.load().nfopp_sample_candidates(_lib.ptr(prev), B, N, D, cap, pool_count, n_field, sigmas[0], sigmas[1],
                                                   sigmas[2], f4(bounds), seed, offset, tio, _lib.ptr(pool),
                                                   _lib.ptr(pool_age), _lib.ptr(cand), _lib.ptr(cand_age),
                                                   _lib.ptr(samples), _lib.stream_ptr()))
    torch.cuda.synchronize()


# ---- item 2: Philox known answers ---------------------------------------------------------------------------------------
def test_philox_known_answers_on_the_device():
    """Random123's Philox4x32-10 vectors, word 0, through nfopp_traj_collision_eval with t_mode 1, which writes
    t = (word0 >> 8) * 2^-24 of counter (c0 c1) = global sample index, (c2 c3) = rng_offset, key = seed.  With two
    waypoints (one segment) the sample index of trajectory 0 is traj_index_offset itself, so all three published vectors
    are reachable; the two whose low counter words have the top bit set need a negative int64 traj_index_offset (the
    kernel casts the index to uint64), which no product path passes but the ABI accepts."""
    z = load_golden("g1_onf.npz")
    onf, _ = gc.make_onf(z["a_cfg"], z["a_params"])
    D = onf.point_dim
    traj = torch.zeros(1, 2, D, device="cuda")
    vectors = [((0, 0, 0, 0), (0, 0), 0x6627e8d5), ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), 0x408f276d),
               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 0xd16cfe09)]
    for (c0, c1, c2, c3), (k0, k1), word in vectors:
        lo, hi, seed = c0 | (c1 << 32), c2 | (c3 << 32), k0 | (k1 << 32)
        tio = lo - (1 << 64) if lo >> 63 else lo
        t = torch.full((1, 1), -1.0, device="cuda")
        out = torch.zeros(1, 1, 4, device="cuda")
        _lib.check(_lib.load().nfopp_traj_collision_eval(onf.config_c(), _lib.ptr(onf.flat_parameters), _lib.ptr(traj), 1, 2, D,
                                                         _lib.ptr(t), 1, seed, hi, tio, _lib.ptr(out), None, None,
                                                         _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert float(t[0, 0]) == (word >> 8) * 2.0 ** -24, (hex(word), float(t[0, 0]) * 2 ** 24)
        # and the sampler's stream reaches the same generator: draw_uniform(seed, traj, idx, offset, stream)
        assert float(orc.philox_uniform(seed, np.array([lo], np.uint64), hi)[0]) == (word >> 8) * 2.0 ** -24


# ---- item 3a: selection against float64 keys ---------------------------------------------------------------------------
SELECT_OFFSETS = [(0, 0), (1000, 7), (123457, (1 << 33) + 5)]     # (rng_offset, traj_index_offset)
_select_report = {"band pairs": 0, "pairs": 0, "inversion": 0.0}


def _caps(C):
    return sorted({1, max(1, C // 2), C})


@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("C", [1, 2, 99, 128, 129, 511, 1022, 4097, 16384])
def test_resample_selects_the_float64_top_cap(C, D):
    """Candidates, ages and records built on the host; every candidate has the unique pose (b, c[, c / 2 + b]), so the
    chosen INDEX is read back from the pool.  The chosen set and the pool order must be those of the float64 keys
    -log(u) / weights64 up to the relative band TAU = 4 x 1.73e-6 = 6.9e-6 around the float64 key of rank `cap`
    (tests/sampling_ref.py: derived from the kernel's fp32 operations 1.73e-6, measured fp32 numpy oracle against
    float64 on the CPU 9.3e-7), and fewer than 1 in 10 000 (trajectory, candidate) pairs may lie inside that band."""
    lib_caps = _caps(C)
    for B in (1, 300):
        for ci, cap in enumerate(lib_caps):
            offset, tio = SELECT_OFFSETS[(ci + D + C) % 3]
            seed = 21 + C
            CS, S, SO = C + 3, cap + 11, 5
            logit, age = ref.resample_inputs(B, C, 7 * C + D + B)
            cand = np.full((B, CS, D), np.nan, F32)
            cand[:, :C, 0] = np.arange(B, dtype=F32)[:, None]
            cand[:, :C, 1] = np.arange(C, dtype=F32)[None]
            if D == 3:
                cand[:, :C, 2] = cand[:, :C, 1] * F32(0.5) + cand[:, :C, 0]
            age_p = np.full((B, CS), np.nan, F32)
            age_p[:, :C] = age
            out4 = np.full((B, CS, 4), np.nan, F32)
            out4[:, :C, 0] = logit
            out4[:, :C, 1:] = 1e30                                       # the other record fields must not matter
            rng = np.random.default_rng(C + cap)
            samples0 = rng.normal(size=(B, S, D)).astype(F32)
            pool_d, page_d = dev(np.full((B, cap, D), SENTINEL)), dev(np.full((B, cap), SENTINEL))
            samples_d = dev(samples0)
            resample(B, C, CS, cap, D, S, SO, seed, offset, tio, dev(cand), dev(age_p), dev(out4), pool_d, page_d, samples_d)
            pool, page, samples = host(pool_d), host(page_d), host(samples_d)
            tag = (C, cap, D, B)
            assert np.isfinite(pool).all() and np.isfinite(page).all(), tag       # no padding row chosen
            chosen = pool[..., 1].astype(np.int64)
            assert (chosen >= 0).all() and (chosen < C).all(), tag
            assert (np.diff(np.sort(chosen, 1), axis=1) > 0).all(), tag          # cap distinct indices
            if cap == C:
                assert np.array_equal(np.sort(chosen, 1), np.tile(np.arange(C), (B, 1))), tag
            picked = np.take_along_axis(cand, chosen[..., None], 1)
            assert same_bits(pool, picked), tag
            assert same_bits(samples[:, SO:SO + cap], picked), tag
            assert same_bits(samples[:, :SO], samples0[:, :SO]) and same_bits(samples[:, SO + cap:], samples0[:, SO + cap:]), tag
            assert np.array_equal(page, np.take_along_axis(age, chosen, 1) + 1), tag
            # float64 keys from the pinned uniforms
            u = (F32(1) - ref.oracle_uniforms(seed, tio, B, C, offset, orc.STREAM_KEY)).astype(F32)
            k64 = ref.race_keys64(u, ref.weights64(logit, age, normalise=False))
            kth = np.partition(k64, cap - 1, axis=1)[:, cap - 1:cap]
            kc = np.take_along_axis(k64, chosen, 1)
            member = np.zeros((B, C), bool)
            np.put_along_axis(member, chosen, True, 1)
            assert (kc <= kth * (1 + ref.TAU)).all(), tag
            assert (k64[~member] >= np.broadcast_to(kth * (1 - ref.TAU), k64.shape)[~member]).all(), tag
            assert (kc[:, 1:] >= kc[:, :-1] * (1 - ref.TAU)).all(), tag          # pool order = ascending key
            # the band is honest: candidates other than the one of rank cap inside it, counted with float64 keys alone
            in_band = int((np.abs(k64 - kth) <= ref.TAU * kth).sum()) - B
            assert in_band >= 0 and in_band < 1e-4 * B * C, (tag, in_band)
            inv = float(np.max(kc[:, :-1] / np.maximum(kc[:, 1:], 1e-300) - 1, initial=0.0))
            inv = max(inv, float(np.max(kc / np.maximum(kth, 1e-300) - 1)))
            _select_report["band pairs"] += in_band
            _select_report["pairs"] += B * C
            _select_report["inversion"] = max(_select_report["inversion"], inv)
    print("selection C %d D %d: so far %d of %d pairs inside the band, largest relative inversion against the float64 "
          "order %.3g (TAU %.3g)" % (C, D, _select_report["band pairs"], _select_report["pairs"], _select_report["inversion"],
                                     ref.TAU))


# ---- item 3c: the law of the chosen set ---------------------------------------------------------------------------------
def _device_choice(logit, age, cap, B, seed, offset, tio):
    """one candidate set shared by B trajectories -> chosen indices [B, cap] in pool order"""
    C, D = len(logit), 3
    cand = np.zeros((B, C, D), F32)
    cand[..., 0] = np.arange(C, dtype=F32)
    out4 = np.zeros((B, C, 4), F32)
    out4[..., 0] = logit
    pool_d, page_d, samples_d = dev(np.zeros((B, cap, D), F32)), dev(np.zeros((B, cap), F32)), dev(np.zeros((B, cap, D), F32))
    resample(B, C, C, cap, D, cap, 0, seed, offset, tio, dev(cand), dev(np.tile(age, (B, 1))), dev(out4), pool_d, page_d,
             samples_d)
    chosen = host(pool_d)[..., 0].astype(np.int64)
    assert np.array_equal(host(page_d), age[chosen] + 1)
    return chosen


@pytest.mark.parametrize("case", ref.DISTRIBUTION_CASES)
def test_resample_has_the_law_of_sequential_weighted_draws(case):
    """65 536 trajectories over one candidate set against the enumerated law of np.random.choice(p=w, replace=False):
    first-order inclusion, first pick (pool[0], proportional to w) and pairwise inclusion, every standardised
    difference below 5.  On the CPU the fp32 oracle's largest value over these four cases is 2.93, and the mutants
    (decay 0 / 0.02 / 0.06, no sigmoid, floor 1e-2, key * w) give 135 / 43 / 125 / 323 / 17 / 2166."""
    C, cap, data_seed, seed, offset, tio = case
    logit, age = ref.distribution_inputs(C, data_seed)
    chosen = _device_choice(logit, age, cap, ref.DISTRIBUTION_B, seed, offset, tio)
    assert (np.diff(np.sort(chosen, 1), axis=1) > 0).all()
    z1, z0, z2 = ref.inclusion_statistics(chosen, ref.weights64(logit, age), cap)
    worst = [float(np.abs(z).max()) for z in (z1, z0, z2)]
    print("device C %d cap %d offset %d: largest standardised difference first-order %.2f, first pick %.2f, pairwise %.2f "
          "(gate %.0f)" % (C, cap, offset, *worst, ref.Z_GATE))
    assert max(worst) < ref.Z_GATE


def test_resample_with_fewer_heavy_candidates_than_slots():
    """The reference switches to replace=True when fewer than `cap` weights exceed 1e-6 (nerf_opt_planner.py:130); the
    device does not (nfopp/learning.py).  What it does instead: the heavy candidates are all kept and the remaining
    slots are filled with DISTINCT floor-weight candidates, uniformly."""
    C, cap, B = 10, 5, 4096
    logit = np.full(C, -100.0, F32)
    logit[[2, 7]] = [0.0, 3.0]
    chosen = _device_choice(logit, np.zeros(C, F32), cap, B, seed=5, offset=2, tio=0)
    assert (np.diff(np.sort(chosen, 1), axis=1) > 0).all()
    member = np.zeros((B, C))
    np.put_along_axis(member, chosen, 1.0, 1)
    assert (member[:, [2, 7]] == 1).all()
    light = [c for c in range(C) if c not in (2, 7)]
    z = ref.standardised(member[:, light].mean(0), 3.0 / (C - 2), B)
    print("light candidates: largest standardised difference to 3 / (C - 2): %.2f (gate %.0f)" % (np.abs(z).max(), ref.Z_GATE))
    assert np.abs(z).max() < ref.Z_GATE


# ---- item 4a: provenance of every pool pose over 30 draws -----------------------------------------------------------------
@pytest.mark.parametrize("D,tag,N,cap", [(3, "a", 60, 40), (2, "c", 60, 40), (3, "a", 300, 100), (2, "c", 300, 100)])
def test_pool_provenance_over_many_draws(D, tag, N, cap):
    z = load_golden("g1_onf.npz")
    onf, _ = gc.make_onf(z[tag + "_cfg"], z[tag + "_params"])
    rng = np.random.default_rng(N + D)
    B, nf, draws = 4, 10, 30
    bounds = (-0.1, 3.1, -0.1, 3.1)
    base = rng.uniform(0.2, 2.8, (B, N, D)).astype(F32)
    sm = nfopp.BatchSampler(onf, B, N, 1.5, 0.02, 0.3, nf, cap, seed=8)
    assert sm.cap == cap
    made = []            # made[k][b] = set of the fine poses trajectory b made at draw k + 1 (as bytes)
    prev_pool = prev_age = None
    for now in range(1, draws + 1):
        prev = (base + F32(0.01) * now).astype(F32)
        s = host(sm.draw(dev(prev), bounds)).reshape(B, sm.S, D)
        pool_n = cap if now > 1 else 0
        cand, cage = host(sm.cand), host(sm.cand_age)
        fine = cand[:, pool_n:pool_n + N - 1]
        made.append([set(bits(row).tobytes() for row in fine[b]) for b in range(B)])
        assert all(len(made[-1][b]) == N - 1 for b in range(B))
        assert (cage[:, pool_n:pool_n + N - 1] == 0).all()
        if now > 1:      # the candidates start with the pool of the draw before, ages included
            assert same_bits(cand[:, :cap], prev_pool) and np.array_equal(cage[:, :cap], prev_age)
        pool, page = host(sm.pool), host(sm.pool_age)
        assert same_bits(s[:, N - 1:N - 1 + cap], pool)
        assert (page >= 1).all() and (page <= now).all() and np.array_equal(page, np.round(page))
        for b in range(B):
            rows = [bits(row).tobytes() for row in pool[b]]
            assert len(set(rows)) == cap, (now, b)
            for row, a in zip(rows, page[b].astype(int)):
                assert row in made[now - a][b], (now, b, a)
        prev_pool, prev_age = pool, page
    assert page.max() >= 3         # poses do survive: the check above was not vacuous


# ---- item 4b: age statistics against numpy's own choice -------------------------------------------------------------------
def test_age_dynamics_match_the_numpy_choice_simulation():
    """nfopp_sample_candidates + nfopp_resample_pool driven directly for 60 steps with every logit 0, so only
    exp(-0.03 age) drives the weights: step 1 offers 32 new candidates for 32 slots, every later step the pool plus the
    first 2 new candidates (n_candidates = cap + 2 below cand_stride), so poses stay for many steps.  The
    per-trajectory mean pool age of 4096 trajectories against 1500 runs of the reference's loop with
    np.random.RandomState.choice: two-sample z below 5.  The shape was chosen on the CPU (tests/test_sampling_ref_cpu.py):
    the fp32 oracle gives z 0.13; decay 0 gives 159, decay 0.06 gives -61, age not incremented gives -561."""
    N, cap, new, steps, B, D = ref.AGE_N, ref.AGE_CAP, ref.AGE_NEW, ref.AGE_STEPS, ref.AGE_B_DEV, 3
    C, S = cap + N - 1, (N - 1) + cap
    rng = np.random.default_rng(1)
    prev = dev(rng.uniform(0, 3, (B, N, D)).astype(F32))
    f32 = dict(dtype=torch.float32, device="cuda")
    pool, page = torch.zeros(B, cap, D, **f32), torch.zeros(B, cap, **f32)
    cand, cage, out4 = torch.zeros(B, C, D, **f32), torch.zeros(B, C, **f32), torch.zeros(B, C, 4, **f32)
    samples = torch.zeros(B, S, D, **f32)
    for k in range(steps):
        pool_n = cap if k else 0
        sample(prev, cap, pool_n, 0, (1.5, 0.02, 0.3), (0, 3, 0, 3), 17, k, 0, pool, page, cand, cage, samples)
        resample(B, N - 1 if k == 0 else cap + new, C, cap, D, S, N - 1, 17, k, 0, cand, cage, out4, pool, page, samples)
    ages = host(page).astype(np.float64)
    t0 = time.time()
    want = ref.choice_simulation(ref.AGE_B_REF, steps, cap, N - 1, new, seed=5)
    zval = ref.two_sample_z(ages.mean(1), want.mean(1))
    print("age dynamics: device mean pool age %.3f, numpy simulation %.3f, two-sample z %.2f (gate %.0f; simulation %.0f s)"
          % (ages.mean(), want.mean(), zval, ref.Z_GATE, time.time() - t0))
    assert abs(zval) < ref.Z_GATE


# ---- item 5a / 5b: layout and the plain lerp ----------------------------------------------------------------------------
def _sample_buffers(B, N, D, cap, n_field):
    C, S = cap + N - 1, (N - 1) + cap + n_field
    return (dev(np.full((B, C, D), SENTINEL)), dev(np.full((B, C), SENTINEL)), dev(np.full((B, S, D), SENTINEL)))


def _check_layout(B, N, D, cap, pool_n, n_field, cand, cage, samples, pool, page):
    """exactly the documented elements are written"""
    n_new = pool_n + N - 1
    untouched = lambda a: (bits(a) == bits(np.array(SENTINEL))).all()
    written = lambda a: (bits(a) != bits(np.array(SENTINEL))).all() and np.isfinite(a).all()
    assert written(cand[:, :n_new]) and written(cage[:, :n_new]) and untouched(cand[:, n_new:]) and untouched(cage[:, n_new:])
    assert written(samples[:, :N - 1]) and written(samples[:, N - 1 + cap:]) and untouched(samples[:, N - 1:N - 1 + cap])
    if pool_n:
        assert same_bits(cand[:, :cap], pool) and same_bits(cage[:, :cap], page)
    assert (cage[:, pool_n:n_new] == 0).all()


@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("cap_kind", ["0", "1", "N-1"])
@pytest.mark.parametrize("N", [2, 3, 60, 257, 700])
def test_sample_candidates_layout_and_plain_lerp(N, cap_kind, D):
    """All three sigmas 0: course and fine poses are traj[j+1] * (1 - t) + traj[j] * t (nerf_opt_planner.py:117) with t
    from the pinned uniform stream, within one fp32 ulp of the larger endpoint of the float64 lerp, and course is
    bit-equal to fine.  Buffers start as a sentinel: exactly the documented elements are written."""
    cap = {"0": 0, "1": 1, "N-1": N - 1}[cap_kind]
    combo = 0
    for pool_n in sorted({0, cap}):
        for n_field in (0, 10, 1000):
            combo += 1
            B = (1, 4096)[(combo + N + D) % 2] if N < 700 or n_field < 1000 else 1
            tio = (0, 1 << 33)[(combo + cap) % 2]
            seed, offset = 40 + N, combo
            rng = np.random.default_rng(N * 8 + combo)
            prev = rng.uniform(-3, 3, (B, N, D)).astype(F32) * rng.choice([1, 30], (B, N, 1)).astype(F32)
            pool = rng.normal(size=(B, cap, D)).astype(F32)
            page = rng.integers(1, 50, (B, cap)).astype(F32)
            cand_d, cage_d, samples_d = _sample_buffers(B, N, D, cap, n_field)
            bounds = (-0.1, 3.1, -0.2, 7.0)
            sample(dev(prev), cap, pool_n, n_field, (0.0, 0.0, 0.0), bounds, seed, offset, tio, dev(pool), dev(page), cand_d,
                   cage_d, samples_d)
            cand, cage, samples = host(cand_d), host(cage_d), host(samples_d)
            _check_layout(B, N, D, cap, pool_n, n_field, cand, cage, samples, pool, page)
            course, fine = samples[:, :N - 1], cand[:, pool_n:pool_n + N - 1]
            assert same_bits(course, fine), (N, cap, pool_n, n_field, B)
            t = ref.oracle_uniforms(seed, tio, B, N - 1, offset, orc.STREAM_T)
            want = ref.lerp64(prev, t)
            ulp = np.spacing(np.maximum(np.abs(prev[:, 1:]), np.abs(prev[:, :-1])).astype(F32)).astype(np.float64)
            worst = float(np.max(np.abs(course.astype(np.float64) - want) / ulp))
            print("lerp N %d cap %d pool %d field %d B %d: largest |device - float64 lerp| = %.3f ulp of the larger endpoint"
                  % (N, cap, pool_n, n_field, B, worst))
            assert worst <= 1.0, (N, cap, pool_n, n_field, B)
            field = samples[:, N - 1 + cap:]
            lo_x, hi_x, lo_y, hi_y = (F32(v) for v in bounds)
            assert (field[..., 0] >= lo_x).all() and (field[..., 0] <= hi_x).all()
            assert (field[..., 1] >= lo_y).all() and (field[..., 1] <= hi_y).all()
            if D == 3:
                assert (field[..., 2] >= 0).all() and (field[..., 2] <= orc.TWO_PI).all()


# ---- item 5c: the Gaussian offsets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 2])
def test_offsets_are_independent_standard_normals(D):
    """z = (pose - float64 lerp) / sigma of the course and the fine set (theta with angle_sigma in both), 4096 x 256
    segments: more than 1e6 values per coordinate set.  sqrt(n) KS to N(0, 1) below 2.69 per coordinate, |z| within the
    Box-Muller bound of a 24-bit uniform, and sqrt(n) * correlation below 5 for course~fine, x~y~theta, j~j+1, b~b+1,
    rng_offset k~k+1 and z~t.  On the CPU the fp32 oracle's largest values are KS 1.31 and correlation 1.90; shared
    streams, overlapping counters and a dropped cosine fail by orders of magnitude."""
    B, N = 4096, 257
    sigmas = (1.5, 0.02, 0.3)
    rng = np.random.default_rng(D)
    prev = rng.uniform(0.2, 0.8, (B, N, D)).astype(F32)
    tio, seed = 1 << 33, 31
    got = []
    for offset in (6, 7):
        cand_d, cage_d, samples_d = _sample_buffers(B, N, D, 0, 0)
        sample(dev(prev), 0, 0, 0, sigmas, (0, 1, 0, 1), seed, offset, tio, None, None, cand_d, cage_d, samples_d)
        t = ref.oracle_uniforms(seed, tio, B, N - 1, offset, orc.STREAM_T)
        got.append(ref.recover_offsets(prev, t, host(samples_d), host(cand_d), *sigmas) + (t,))
    (zc, zf, t), (zc_next, _, _) = got
    assert zc[..., 0].size >= 10 ** 6 and np.isfinite(zc).all() and np.isfinite(zf).all()
    worst_ks = 0.0
    for name, zz in (("course", zc), ("fine", zf)):
        for d in range(D):
            ks = ref.ks_sqrt_n(zz[..., d], ref.normal_cdf)
            worst_ks = max(worst_ks, ks)
            print("device D %d %s coordinate %d: sqrt(n) KS %.2f (gate %.2f), max |z| %.4f (bound %.4f)"
                  % (D, name, d, ks, ref.KS_GATE, np.abs(zz[..., d]).max(), ref.Z_MAX))
            assert ks < ref.KS_GATE
        assert np.abs(zz).max() <= ref.Z_MAX + 1e-3
    corr = ref.offset_correlations(zc, zf, t, zc_next)
    worst = max(corr, key=lambda k: abs(corr[k]))
    print("device D %d: largest sqrt(n) KS %.2f; largest sqrt(n) correlation %.2f (%s), gate %.0f"
          % (D, worst_ks, corr[worst], worst, ref.CORR_GATE))
    assert abs(corr[worst]) < ref.CORR_GATE


# ---- item 5d: field poses -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 2])
def test_field_poses_are_uniform_on_the_bounds(D):
    B, N, n_field = 4096, 2, 1000
    bounds = (-0.1, 3.1, -0.2, 7.0)
    cand_d, cage_d, samples_d = _sample_buffers(B, N, D, 0, n_field)
    sample(dev(np.zeros((B, N, D), F32)), 0, 0, n_field, (1.5, 0.02, 0.3), bounds, 77, 3, 12, None, None, cand_d, cage_d,
           samples_d)
    field = host(samples_d)[:, 1:].astype(np.float64)
    lims = [(F32(bounds[0]), F32(bounds[1])), (F32(bounds[2]), F32(bounds[3])), (F32(0), orc.TWO_PI)][:D]
    for d, (lo, hi) in enumerate(lims):
        lo, hi = float(lo), float(hi)
        assert field[..., d].min() >= lo and field[..., d].max() <= hi
        ks = ref.ks_sqrt_n(field[..., d], lambda x: np.clip((x - lo) / (hi - lo), 0, 1))
        print("field D %d coordinate %d: sqrt(n) KS %.2f (gate %.2f), range [%.6f, %.6f]" % (D, d, ks, ref.KS_GATE,
                                                                                            field[..., d].min(), field[..., d].max()))
        assert ks < ref.KS_GATE
    for a in range(D):
        for b in range(a + 1, D):
            r = ref.corr_sqrt_n(field[..., a], field[..., b])
            print("field D %d coordinates %d~%d: sqrt(n) correlation %.2f (gate %.0f)" % (D, a, b, r, ref.CORR_GATE))
            assert abs(r) < ref.CORR_GATE
    for d in range(D):                                                   # field pose r against r + 1
        assert abs(ref.corr_sqrt_n(field[:, :-1, d], field[:, 1:, d])) < ref.CORR_GATE


# ---- item 5e: shard invariance by index --------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("first", [0, 1 << 33])
def test_sample_candidates_shard_invariance(first, D):
    """trajectories [b0, b0 + k) as their own launch with traj_index_offset = b0 are bit-equal to rows b0.. of the full
    launch, for all three output buffers, at b0 = 3 and at 2^33 + 3"""
    B, N, cap, n_field, b0, k = 8, 60, 40, 10, 3, 4
    rng = np.random.default_rng(D)
    prev = rng.uniform(0, 3, (B, N, D)).astype(F32)
    pool, page = rng.normal(size=(B, cap, D)).astype(F32), rng.integers(1, 9, (B, cap)).astype(F32)
    out = []
    for lo, hi, tio in ((0, B, first), (b0, b0 + k, first + b0)):
        bufs = _sample_buffers(hi - lo, N, D, cap, n_field)
        sample(dev(prev[lo:hi]), cap, cap, n_field, (1.5, 0.02, 0.3), (-0.1, 3.1, -0.2, 7.0), 9, 4, tio, dev(pool[lo:hi]),
               dev(page[lo:hi]), *bufs)
        out.append([host(x) for x in bufs])
    for full, shard in zip(*out):
        assert same_bits(full[b0:b0 + k], shard)
    assert not same_bits(out[0][0][b0 + 1:b0 + 1 + k], out[1][0])
