"""GPU: the trajectory-update kernel's outputs, bit for bit, against tests/golden/k2_bits.npz -- recorded by
tools/record_k2_bits.py from the build in front of the division-free staging of the boundary band columns
(csrc/traj_update.hip: staging by (tap, column), every load of the first phase in one flight, retired trajectories leave
first; no stencil, collision, band-product or Adam expression touched).  "The same results" means the same 32-bit words:
every comparison is np.array_equal.

Cases (tests/k2_bits_cases.py): B = 3, one nfopp_traj_update call per case at every shape branch of the staging; each case
with the loss terms, without them (the planner's own step: the state must not depend on it) and with the middle trajectory
retired by an `active` mask (its rows stay as they were)."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import k2_bits_cases as kc  # noqa: E402

IDS = [kc.tag(c) for c in kc.CASES]


@pytest.fixture(scope="module")
def want():
    return load_golden("k2_bits.npz")


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(_words(a), _words(b)), (what, int((_words(a) != _words(b)).sum()), "words differ")


def test_fixture_and_cases_name_the_same_arrays(want):
    assert sorted(want.files) == sorted("%s_%s" % (kc.tag(c), k) for c in kc.CASES for k in kc.arrays_of(c))


def test_the_case_list_reaches_every_staging_branch():
    """from engine.band_of / engine.interior_range, not from the kernel: a changed band rule must not silently move a case"""
    br = {c: kc.branch(c) for c in kc.CASES}
    assert any(not interior and staged and nb <= 64 for interior, nb, staged in br.values())       # no interior, one wave of columns
    assert any(not interior and staged and nb > 64 for interior, nb, staged in br.values())        # second column trip
    assert any(interior and staged and nb <= 64 for interior, nb, staged in br.values())           # the benchmark's
    assert any(interior and not staged for interior, nb, staged in br.values())                    # taps from global memory
    assert any(not interior and not staged for interior, nb, staged in br.values())
    assert br[(2, 0.5, 3)] == (False, 2, True) and br[(64, 0.5, 3)] == (False, 64, True)
    assert br[(121, 0.5, 3)] == (False, 121, True) and br[(122, 0.5, 3)] == (True, 58, True)
    assert br[(256, 0.5, 3)] == (True, 58, True) and br[(256, 2, 3)] == (True, 116, False)
    assert kc.band(256, 0.5)[2] == (29, 227) and kc.band(256, 2)[2] == (58, 198)


@pytest.mark.parametrize("case", kc.CASES, ids=IDS)
def test_state_and_terms(case, want):
    got = kc.run_case(case)
    for k in kc.arrays_of(case):
        _same(got[k], want["%s_%s" % (kc.tag(case), k)], (case, k))


@pytest.mark.parametrize("case", kc.CASES, ids=IDS)
def test_state_without_terms(case, want):
    got = kc.run_case(case, want_terms=False)
    for k in kc.arrays_of(case)[:-1]:
        _same(got[k], want["%s_%s" % (kc.tag(case), k)], (case, k))
    assert np.array_equal(got["terms"], np.full((kc.B, 8), kc.TERMS_FILL)), "a null terms pointer, yet the buffer was written"


@pytest.mark.parametrize("want_terms", (True, False))
@pytest.mark.parametrize("case", kc.CASES, ids=IDS)
def test_retired_trajectory_is_untouched(case, want_terms, want):
    got = kc.run_case(case, want_terms=want_terms, retired=1)
    before = kc.inputs(case)
    for k in kc.arrays_of(case)[:-1]:
        ref = want["%s_%s" % (kc.tag(case), k)].copy()
        ref[1] = before[k][1]
        _same(got[k], ref, (case, k))
    ref = want[kc.tag(case) + "_terms"].copy() if want_terms else np.full((kc.B, 8), kc.TERMS_FILL)
    ref[1] = kc.TERMS_FILL
    _same(got["terms"], ref, (case, "terms"))
