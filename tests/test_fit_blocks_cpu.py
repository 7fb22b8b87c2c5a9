"""CPU: the block-by-block gate of the fit gradient (tests/fit_blocks_gate.py) and its cases (tests/fit_blocks_cases.py),
without a device.

  conditions   the counts give the workgroups of pass 2 the trip counts they are listed for (K = 16 and 32, 256 and 8 compute
               units); every row of every case is kink-free, the fp32 oracle has the float64 ReLU masks on every row, and the
               sentinel rows carry |rho| >= 0.5 / P
  pass check   each of the two fp32 evaluations passes the gate the other one contributes to
  teeth        errors of the size a pipeline bug has -- the last sample dropped, the last ragged chunk dropped, a sample counted
               twice, the first chunk of the second round skipped, one ReLU mask bit of one sample flipped, the `we` block off
               by 2^-12, ang_f and ang_b swapped -- are planted into the oracle's fp32 gradient and must be rejected in every
               case where they apply
  the reason   the gate this one replaces (one number for the whole gradient: 2e-5 x max(1, max |g|)) ACCEPTS the scaled `we`
               block in every case, and at the largest count its tolerance is above the error of a dropped last sample in all
               blocks but w3 and b3

The planted cases run on 8 virtual compute units (counts up to 769 and the per-sample cap 4096 / 4097), the largest count
of 256 compute units (24 577) on both full networks."""
import numpy as np
import pytest

import fit_blocks_cases as fc
import fit_blocks_gate as fg
import float64_ref as f64
from bits_float64_gate import failures

F32 = np.float32
LARGEST = [(fin, max(fc.counts(256)), 256) for fin in fc.FULL_DIMS]


# ----------------------------------------------------------------------------------------------------------
# the counts
@pytest.mark.parametrize("C", [256, 8])
def test_counts_and_cases(C):
    counts = fc.counts(C)
    assert counts == sorted(set(counts)) and set(fc.SMALL) <= set(counts) and {4096, 4097} <= set(counts)
    assert set(fc.reduced_counts(C)) <= set(counts)
    cases = fc.cases(C)
    assert len(cases) == len(set(cases)) == 2 * len(counts) + 2 * 3
    for fin in fc.FULL_DIMS:
        assert [P for f, P in cases if f == fin] == counts
    for fin in fc.REDUCED_DIMS:
        assert [P for f, P in cases if f == fin] == [33, C * 32 + 1, 2 * C * 32 + 37]
    if C == 256:
        assert max(counts) == 24577 and len(counts) == 21      # C * 16 = 4096 and C * 16 + 1 = 4097 appear once


@pytest.mark.parametrize("K", fc.KS)
@pytest.mark.parametrize("C", [256, 8])
def test_grid_edges_give_the_listed_trip_counts(C, K):
    one, one_more, two, two_three, three_four = fc.grid_edges(C, K)
    assert all(P in fc.counts(C) for P in fc.grid_edges(C, K))
    trips, last = fc.trip_counts(one, K, C)
    assert len(trips) == C and (trips == 1).all() and last == K
    trips, last = fc.trip_counts(one_more, K, C)
    assert len(trips) == C and trips[0] == 2 and (trips[1:] == 1).all() and last == 1
    trips, last = fc.trip_counts(two, K, C)
    assert len(trips) == C and (trips == 2).all() and last == K - 1
    trips, last = fc.trip_counts(two_three, K, C)
    assert len(trips) == C and (trips[:2] == 3).all() and (trips[2:] == 2).all() and last == 5
    trips, last = fc.trip_counts(three_four, K, C)
    assert len(trips) == C and trips[0] == 4 and (trips[1:] == 3).all() and last == 1


@pytest.mark.parametrize("K", fc.KS)
def test_small_counts_are_the_chunk_edges(K):
    for P in (K - 1, K, K + 1):
        trips, last = fc.trip_counts(P, K, 256)
        assert P in fc.SMALL and trips.tolist() == [1] * (1 + (P > K)) and last == (P - 1) % K + 1
    # the per-sample path reduces ceil(P / 64) chunks, at most 64
    assert {63, 64, 65, 129, 4096, 4097} <= set(fc.counts(256))


# ----------------------------------------------------------------------------------------------------------
# the inputs: every case of a device of 256 compute units (those of 8 are checked with their references below)
def _conditions(ref_or_inputs, fin, P):
    kink, on_agree, rho = ref_or_inputs
    assert kink.min() >= fc.KINK_MARGIN, (fin, P)        # no row is left out of any comparison
    assert on_agree, (fin, P, "an fp32 ReLU mask differs from the float64 one")
    s = fc.sentinels(P)
    assert P - 1 in s and all(q % 32 == 0 or q == P - 1 for q in s) and P - s[0] <= 32
    assert (np.abs(rho[s]) >= 0.5 / P).all(), (fin, P, rho[s] * P)


@pytest.mark.parametrize("fin", sorted(fc.FULL_DIMS + fc.REDUCED_DIMS))
def test_inputs_of_every_case_at_256_compute_units(fin):
    flat, cfg = fg.network(fin)
    for f, P in fc.cases(256):
        if f != fin:
            continue
        x, y = fc.inputs(fin, P, flat, cfg)
        assert x.shape == (P, cfg.point_dim) and x.dtype == F32 and set(np.unique(y)) <= {0.0, 1.0}
        x2, y2 = fc.inputs(fin, P, flat, cfg)
        assert np.array_equal(x, x2) and np.array_equal(y, y2)
        r = f64.onf_fit64(flat, cfg, x, y, keep_eval=True)
        f32 = fg.factors32(flat, cfg, x, y)
        agree = np.array_equal(f32["on1"], r["eval"]["a1"] > 0) and np.array_equal(f32["on2"], r["eval"]["a2"] > 0)
        _conditions((r["kink"], agree, r["rho"]), fin, P)


# ----------------------------------------------------------------------------------------------------------
# the gate
@pytest.fixture(scope="module", params=[(fin, P, 8) for fin, P in fc.cases(8)] + LARGEST, ids=lambda c: "F%d_P%d_C%d" % c)
def ref(request):
    """the reference of one case with its float64 per-sample values: computed once, shared by the tests below, never changed"""
    return fg.reference(*request.param, keep_eval=True)


def _o32(ref):
    return fg.output_of(ref["o32"][0], ref["o32"][1], ref["P"])


def _planted(ref, delta):
    """the oracle's fp32 output with the float64 error `delta` planted into its gradient"""
    return fg.output_of(ref["o32"][0].astype(np.float64) + delta, ref["o32"][1], ref["P"])


def _contribution(ref, rows):
    return f64.fit_sums64(ref["eval"], ref["cfg"], ref["rho"], rows=np.asarray(rows))


def _rejected_blocks(ref, g):
    """the blocks outside the gate, under the yardstick of each chunk length: an error has to be rejected under both"""
    out = []
    for K in fc.KS:
        rows = fg.compare("planted", ref, g, K)
        assert rows[-1].ok and rows[-2].ok          # the count and the loss are untouched by every planted error
        out.append({r.array for r in rows if not r.ok})
    return out


def planted_errors(ref):
    """{name: output with the error} of every planted error that applies to the case"""
    P, C, cfg, bl = ref["P"], ref["C"], ref["cfg"], ref["blocks"]
    o32 = ref["o32"][0]
    out = {"last sample dropped": _planted(ref, -_contribution(ref, [P - 1])),
           "one sample counted twice": _planted(ref, _contribution(ref, [fc.sentinels(P)[0]]))}
    for K in fc.KS:
        if P % K:
            out["last ragged chunk of %d dropped" % K] = _planted(ref, -_contribution(ref, range(K * ((P - 1) // K), P)))
        if -(-P // K) > C:
            out["chunk %d of %d skipped" % (C, K)] = _planted(ref, -_contribution(ref, range(C * K, min(P, C * K + K))))
    # the a2 mask bit of one hidden unit of the last sample read as 0: its row of dh2 loses rho w3[j] (G2: w2 and b2)
    c = ref["eval"]
    w3 = c["p"]["w3"].reshape(-1)
    j = int(np.argmax(np.abs(w3[:100]) * (c["a2"][P - 1] > 0)))
    assert c["a2"][P - 1, j] > 0
    delta = np.zeros(cfg.n_params())
    delta[bl["w2"]][j * 100:(j + 1) * 100] = -ref["rho"][P - 1] * w3[j] * c["h1"][P - 1]
    delta[bl["b2"]][j] = -ref["rho"][P - 1] * w3[j]
    out["one mask bit flipped"] = _planted(ref, delta)
    g = _o32(ref)
    g[bl["we"]] = (o32[bl["we"]] * F32(1 + 2.0 ** -12)).astype(F32)
    out["we scaled by 1 + 2^-12"] = g
    if cfg.angle_encoding:
        g = _o32(ref)
        g[bl["ang_b"]], g[bl["ang_f"]] = o32[bl["ang_f"]], o32[bl["ang_b"]]
        out["ang_f and ang_b swapped"] = g
    return out


def test_case_conditions(ref):
    _conditions((ref["kink"], ref["masks_agree"], ref["rho"]), ref["fin"], ref["P"])


def test_each_fp32_evaluation_passes_the_gate_of_the_other(ref):
    for K in fc.KS:
        for name, (grad, loss) in (("oracle32", ref["o32"]), ("chunked32", ref["chunked"][K])):
            rows = fg.compare(name, ref, fg.output_of(grad, loss, ref["P"]), K)
            assert len(rows) == len(ref["blocks"]) + 2 and not failures(rows), (name, K, failures(rows))
        assert 1.0 <= ref["Y"][K] < 64, ref["Y"]        # a yardstick of hundreds of units would gate nothing
        # never looser than the old gate, block by block
        assert all(r.bound <= ref["old_grad"] for r in rows[:-2])


def test_planted_errors_are_rejected(ref):
    errors = planted_errors(ref)
    P, C = ref["P"], ref["C"]
    assert {"last sample dropped", "one sample counted twice", "one mask bit flipped", "we scaled by 1 + 2^-12"} <= set(errors)
    assert ("ang_f and ang_b swapped" in errors) == (ref["fin"] in (220, 120))
    for K in fc.KS:
        assert ("last ragged chunk of %d dropped" % K in errors) == (P % K != 0)
        assert ("chunk %d of %d skipped" % (C, K) in errors) == (P > C * K)
    for name, g in errors.items():
        for K, blocks in zip(fc.KS, _rejected_blocks(ref, g)):
            print("%-32s K = %2d  rejected in %s" % (name, K, sorted(blocks)))
            assert blocks, (name, K, "the gate accepts it")
            if name.startswith("we "):
                assert blocks == {"we"}
            if name.startswith("one mask"):
                assert blocks <= {"w2", "b2"}
            if name.startswith("ang_f"):
                assert blocks == {"ang_b", "ang_f"}


def test_the_old_gate_accepts_the_scaled_we_block(ref):
    g = planted_errors(ref)["we scaled by 1 + 2^-12"]
    assert fg.old_gate_accepts(ref, g)
    assert all("we" in blocks for blocks in _rejected_blocks(ref, g))


@pytest.mark.parametrize("fin,P,C", LARGEST)
def test_the_old_gate_at_a_dropped_last_sample_of_the_largest_count(fin, P, C):
    """The last sample is a sentinel: |rho| >= 0.5 / P = 2.03e-5 at P = 24 577, and b3 = sum rho, w3 = sum rho [h2 | in] hold
    rho itself -- there the error of the dropped sample is just above the old gate's absolute 2e-5 (by less than 2 x: at
    twice the count it is below).  In every other block the old tolerance is 3 to 30 times the error, i.e. the old gate
    accepts the dropped sample; the new one rejects it in EVERY block."""
    ref = fg.reference(fin, P, C, keep_eval=True)
    d = np.abs(_contribution(ref, [P - 1]))
    over = {k for k, s in ref["blocks"].items() if d[s].max() >= ref["old_grad"]}
    assert over <= {"w3", "b3"} and d.max() < 2 * ref["old_grad"], (over, d.max(), ref["old_grad"])
    others = [k for k in ref["blocks"] if k not in ("w3", "b3")]
    g = planted_errors(ref)["last sample dropped"]
    masked = g.copy()           # the same error without its w3 / b3 part: what the old gate lets through
    for k in ("w3", "b3"):
        masked[ref["blocks"][k]] = ref["o32"][0][ref["blocks"][k]]
    assert fg.old_gate_accepts(ref, masked)
    for blocks, blocks_masked in zip(_rejected_blocks(ref, g), _rejected_blocks(ref, masked)):
        assert blocks == set(ref["blocks"]) and blocks_masked == set(others)
