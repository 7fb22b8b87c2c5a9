"""CPU checks behind tests/test_gpu_sampling_reference.py:

* the float64 reference helper (tests/sampling_ref.py) against `np.random.choice` itself;
* the statistics the GPU tests gate on (inclusion frequencies, age dynamics, Gaussian offsets), run here on the fp32
  oracle, which must pass with room, and on local mutants of it, each of which must break at least one gate.  That is
  the evidence that the GPU gates can fail: a wrong age decay, a pool that forgets to age, a mis-weighted race, a
  shared stream or a broken Box-Muller would not pass them.  The repository's oracle is not touched; the mutants live
  in this file.
"""
import numpy as np
import pytest

import sampling_ref as ref
from oracle import nfopp_oracle as orc

F32 = np.float32


# ---- the fp32 oracle, vectorised over trajectories, with switches for the mutants --------------------------------------
def variant_resample(cand_age, logits, cap, seed, offset, traj_index_offset=0, decay=0.03, use_sigmoid=True, floor=1e-6,
                     divide=True, increment=1.0):
    """oracle.resample_pool for [B, C] ages / logits at once; the defaults ARE the oracle (checked below)."""
    cand_age, logits = np.asarray(cand_age, F32), np.asarray(logits, F32)
    B, C = cand_age.shape
    u = (F32(1) - ref.oracle_uniforms(seed, traj_index_offset, B, C, offset, orc.STREAM_KEY)).astype(F32)
    s = orc.sigmoid(logits) if use_sigmoid else F32(1)
    w = (s * np.exp(F32(-decay) * cand_age) + F32(floor)).astype(F32)
    key = (-np.log(u) / w if divide else -np.log(u) * w).astype(F32)
    order = np.argsort(key, axis=1, kind="stable")[:, :cap]          # stable: equal keys by index
    return order, np.take_along_axis(cand_age, order, 1) + F32(increment)


def variant_age_dynamics(batch, seed, **mutant):
    """the pool ages after AGE_STEPS steps of the shape the GPU test runs (constant logit 0)"""
    pool_age = np.zeros((batch, 0), F32)
    for k in range(ref.AGE_STEPS):
        new = np.zeros((batch, ref.AGE_N - 1 if k == 0 else ref.AGE_NEW), F32)
        cand_age = np.concatenate([pool_age, new], 1)
        _, pool_age = variant_resample(cand_age, np.zeros_like(cand_age), ref.AGE_CAP, seed, k, **mutant)
    return pool_age


def variant_normal(seed, batch, n, offset, stream, cos_term=True):
    """oracle.draw_normal for [batch, n] values at once"""
    u = ref.oracle_uniforms(seed, 0, batch, 2 * n, offset, stream)
    u1, u2 = (F32(1) - u[:, 0::2]).astype(F32), u[:, 1::2]
    r = np.sqrt(F32(-2) * np.log(u1))
    return (r * np.cos(orc.TWO_PI * u2) if cos_term else r).astype(F32)


def test_vectorised_variants_are_the_oracle():
    rng = np.random.default_rng(4)
    B, C, cap = 7, 50, 20
    age = rng.integers(0, 50, (B, C)).astype(F32)
    logits = rng.normal(0, 3, (B, C)).astype(F32)
    cand = rng.normal(size=(B, C, 3)).astype(F32)
    _, want_age, want = orc.resample_pool(cand, age, logits, cap, seed=5, offset=9, traj_index_offset=11)
    got, got_age = variant_resample(age, logits, cap, 5, 9, 11)
    assert np.array_equal(got, want) and np.array_equal(got_age, want_age)
    z = variant_normal(3, 4, 30, 2, orc.STREAM_FINE)
    for b in range(4):
        assert np.array_equal(z[b], orc.draw_normal(3, b, np.arange(30), 2, orc.STREAM_FINE))


# ---- the helper against numpy ----------------------------------------------------------------------------------------
def test_weights_and_keys():
    logit, age = np.array([-100.0, -2.0, 0.0, 3.0, 100.0]), np.array([0.0, 10.0, 300.0, 1.0, 40.0])
    w = ref.weights64(logit, age, normalise=False)
    assert abs(w[0] - 1e-6) < 1e-20 and abs(w[4] - (np.exp(-1.2) + 1e-6)) < 1e-15
    assert abs(w[2] - (0.5 * np.exp(-9.0) + 1e-6)) < 1e-18
    assert abs(ref.weights64(logit, age).sum() - 1) < 1e-15
    assert np.allclose(ref.race_keys64([1.0, np.exp(-2.0)], [0.5, 4.0]), [0.0, 0.5], atol=1e-15)


def test_inclusion_exact_is_what_numpy_choice_samples():
    rng = np.random.default_rng(3)
    C, cap, trials = 8, 3, 40000
    w = ref.weights64(rng.normal(0, 2, C), rng.integers(0, 40, C))
    first, pair, first_pick = ref.inclusion_exact(w, cap)
    assert abs(first.sum() - cap) < 1e-12 and abs(first_pick.sum() - 1) < 1e-12 and np.allclose(first_pick, w)
    assert np.allclose(np.diag(pair), first) and np.allclose(pair.sum(1), cap * first)
    rs = np.random.RandomState(11)
    chosen = np.stack([rs.choice(C, cap, replace=False, p=w) for _ in range(trials)])
    z1, z0, z2 = ref.inclusion_statistics(chosen, w, cap)
    worst = max(np.abs(z1).max(), np.abs(z0).max(), np.abs(z2).max())
    print("np.random.choice against the enumeration: largest standardised difference %.2f" % worst)
    assert worst < ref.Z_GATE
    # two candidates, one pick: the closed form
    f, _, _ = ref.inclusion_exact([0.25, 0.75], 1)
    assert np.allclose(f, [0.25, 0.75])


def test_choice_simulation_is_the_reference_loop():
    # one step from an empty pool is one np.random.choice over equal weights, ages 1
    ages = ref.choice_simulation(3, 1, 5, 9, 2, seed=0)
    assert ages.shape == (3, 5) and (ages == 1).all()
    # two steps by hand
    rs = np.random.RandomState(7)
    rs.choice(9, 5, replace=False, p=np.full(9, 1 / 9))
    cand_age = np.array([1.0] * 5 + [0.0] * 2)
    want = cand_age[rs.choice(7, 5, replace=False, p=ref.weights64(np.zeros(7), cand_age))] + 1
    assert np.array_equal(ref.choice_simulation(1, 2, 5, 9, 2, seed=7)[0], want)


def test_fp32_keys_stay_inside_the_derived_band():
    """the measured half of TAU (tests/sampling_ref.py): fp32 numpy oracle against race_keys64, same inputs"""
    worst = 0.0
    for C in (2, 99, 1022, 4097):
        logit, age = ref.resample_inputs(64, C, C)
        u = (F32(1) - ref.oracle_uniforms(21, 5, 64, C, 3, orc.STREAM_KEY)).astype(F32)
        with np.errstate(over="ignore"):
            w = (orc.sigmoid(logit) * np.exp(F32(-0.03) * age) + F32(1e-6)).astype(F32)
        k32 = (-np.log(u) / w).astype(F32).astype(np.float64)
        k64 = ref.race_keys64(u, ref.weights64(logit, age, normalise=False))
        worst = max(worst, float(np.max(np.abs(k32 - k64) / np.maximum(k64, 1e-300))))
    print("largest relative key difference fp32 oracle / float64: %.3g (derived bound %.3g)" % (worst, ref.TAU_DERIVED))
    assert worst <= ref.TAU_DERIVED


# ---- item 3c: inclusion frequencies -------------------------------------------------------------------------------------
RESAMPLE_MUTANTS = {"decay 0": dict(decay=0.0), "decay 0.02": dict(decay=0.02), "decay 0.06": dict(decay=0.06),
                    "sigmoid dropped": dict(use_sigmoid=False), "floor 1e-2": dict(floor=1e-2),
                    "key = -log(u) * w": dict(divide=False)}


def _inclusion_worst(case, **mutant):
    C, cap, data_seed, seed, offset, tio = case
    logit, age = ref.distribution_inputs(C, data_seed)
    B = ref.DISTRIBUTION_B
    chosen, _ = variant_resample(np.tile(age, (B, 1)), np.tile(logit, (B, 1)), cap, seed, offset, tio, **mutant)
    z1, z0, z2 = ref.inclusion_statistics(chosen, ref.weights64(logit, age), cap)
    return float(np.abs(z1).max()), float(np.abs(z0).max()), float(np.abs(z2).max())


@pytest.mark.parametrize("case", ref.DISTRIBUTION_CASES)
def test_oracle_inclusion_frequencies_match_sequential_draws(case):
    worst = _inclusion_worst(case)
    print("fp32 oracle, C %d cap %d: largest standardised difference first-order %.2f, first pick %.2f, pairwise %.2f"
          % (case[0], case[1], *worst))
    assert max(worst) < 3.5


@pytest.mark.parametrize("name", sorted(RESAMPLE_MUTANTS))
def test_resampling_mutants_break_the_inclusion_gate(name):
    worst = max(max(_inclusion_worst(case, **RESAMPLE_MUTANTS[name])) for case in ref.DISTRIBUTION_CASES[:2])
    print("mutant %-18s: largest standardised difference %.1f (gate %.0f)" % (name, worst, ref.Z_GATE))
    assert worst > ref.Z_GATE


# ---- item 4b: age dynamics ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_mean_ages():
    return ref.choice_simulation(ref.AGE_B_REF, ref.AGE_STEPS, ref.AGE_CAP, ref.AGE_N - 1, ref.AGE_NEW, seed=5).mean(1)


def test_oracle_age_dynamics_match_the_numpy_simulation(reference_mean_ages):
    z = ref.two_sample_z(variant_age_dynamics(ref.AGE_B_DEV, 17).mean(1), reference_mean_ages)
    print("fp32 oracle: two-sample z of the mean pool age %.2f (reference mean %.3f)" % (z, reference_mean_ages.mean()))
    assert abs(z) < 3


@pytest.mark.parametrize("name,mutant", [("decay 0", dict(decay=0.0)), ("decay 0.06", dict(decay=0.06)),
                                         ("age not incremented", dict(increment=0.0))])
def test_age_mutants_break_the_age_gate(reference_mean_ages, name, mutant):
    z = ref.two_sample_z(variant_age_dynamics(ref.AGE_B_DEV, 17, **mutant).mean(1), reference_mean_ages)
    print("mutant %-20s: two-sample z of the mean pool age %.1f (condition: beyond 8; gate %.0f)" % (name, z, ref.Z_GATE))
    assert abs(z) > 8


# ---- item 5c: Gaussian offsets ------------------------------------------------------------------------------------------
OFFSET_B, OFFSET_N, OFFSET_SIGMAS = 1400, 257, (1.5, 0.02, 0.3)


def _oracle_offsets(D):
    rng = np.random.default_rng(D)
    prev = rng.uniform(0.2, 0.8, (OFFSET_B, OFFSET_N, D)).astype(F32)
    out = []
    for offset in (6, 7):
        cand, _, smp = orc.sample_candidates(prev, None, None, 0, 0, *OFFSET_SIGMAS, (0, 1, 0, 1), seed=31, offset=offset)
        t = ref.oracle_uniforms(31, 0, OFFSET_B, OFFSET_N - 1, offset, orc.STREAM_T)
        out.append(ref.recover_offsets(prev, t, smp, cand, *OFFSET_SIGMAS) + (t,))
    return out


@pytest.mark.parametrize("D", [3, 2])
def test_oracle_offsets_are_independent_standard_normals(D):
    (zc, zf, t), (zc_next, _, _) = _oracle_offsets(D)
    assert zc.size >= 700000 and np.isfinite(zc).all() and np.isfinite(zf).all()
    for name, z in (("course", zc), ("fine", zf)):
        for d in range(D):
            ks = ref.ks_sqrt_n(z[..., d], ref.normal_cdf)
            print("fp32 oracle D %d %s coordinate %d: sqrt(n) KS %.2f (gate %.2f), max |z| %.3f" % (D, name, d, ks, ref.KS_GATE,
                                                                                                 np.abs(z[..., d]).max()))
            assert ks < ref.KS_GATE
        assert np.abs(z).max() <= ref.Z_MAX + 1e-3
    corr = ref.offset_correlations(zc, zf, t, zc_next)
    worst = max(corr, key=lambda k: abs(corr[k]))
    print("fp32 oracle D %d: largest sqrt(n) correlation %.2f (%s), gate %.0f" % (D, corr[worst], worst, ref.CORR_GATE))
    assert abs(corr[worst]) < ref.CORR_GATE


def test_offset_mutants_break_their_gates():
    n = 255
    zc = variant_normal(31, OFFSET_B, 3 * n, 6, orc.STREAM_COURSE).reshape(OFFSET_B, n, 3).astype(np.float64)
    t = ref.oracle_uniforms(31, 0, OFFSET_B, n, 6, orc.STREAM_T)
    # COURSE and FINE sharing one stream
    shared = ref.offset_correlations(zc, zc.copy(), t)
    assert abs(shared["course~fine"]) > ref.CORR_GATE
    # FINE reading the COURSE stream one draw later (overlapping counters)
    zs = variant_normal(31, OFFSET_B, 3 * n + 1, 6, orc.STREAM_COURSE)[:, 1:].reshape(OFFSET_B, n, 3).astype(np.float64)
    assert abs(ref.corr_sqrt_n(zc[:, :, 1], zs[:, :, 0])) > ref.CORR_GATE
    # cos(2 pi u2) replaced by 1
    zr = variant_normal(31, OFFSET_B, 3 * n, 6, orc.STREAM_COURSE, cos_term=False)
    ks = ref.ks_sqrt_n(zr, ref.normal_cdf)
    print("mutant cos -> 1: sqrt(n) KS %.1f (gate %.2f)" % (ks, ref.KS_GATE))
    assert ks > ref.KS_GATE
