"""GPU: the outputs of the two kernels that fit the quadratic spline, bit for bit, against tests/golden/spline_bits.npz --
recorded by tools/record_spline_bits.py from the build in which path_post.hip and grid_search.hip each carried a fit of their
own, before csrc/spline2.h became its one owner.  "The same results" means the same words: every comparison is
np.array_equal on integer views (uint32 of the fp32 trajectories, uint64 of the float64 poses, the int32 counts as they are).

Cases and why each is there: tests/spline_bits_cases.py; that each sits at the branch it claims: tests/test_spline_bits_cpu.py."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import spline_bits_cases as sc  # noqa: E402


@pytest.fixture(scope="module")
def want():
    return load_golden("spline_bits.npz")


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    a, b = sc.words(got), sc.words(ref)
    assert np.array_equal(a, b), (what, int((a != b).sum()), "words differ")


def test_fixture_and_cases_name_the_same_arrays(want):
    names = ["post_%s_%s" % (n, k) for n in sc.POST_CASES for k in ("count", "out")]
    names += ["seed_%s_traj" % sc.seed_tag(c) for c in sc.SEED_CASES]
    assert sorted(want.files) == sorted(names)
    for k in want.files:
        assert want[k].dtype == (np.int32 if k.endswith("_count") else np.float64 if k.endswith("_out") else np.float32), k
        assert k.startswith("post_") or np.isfinite(want[k]).all(), k


@pytest.mark.parametrize("name", list(sc.POST_CASES))
def test_post_processor(name, want):
    got = sc.run_post(name)
    ref_count, ref_out = want["post_%s_count" % name], want["post_%s_out" % name]
    _same(got["count"], ref_count, (name, "count"))
    max_out = sc.POST_CASES[name][3]
    for b, cnt in enumerate(got["count"]):
        assert cnt <= max_out, (name, b, cnt, "the case no longer holds every pose")
        k = max(int(cnt), 0)
        _same(got["out"][b, :k], ref_out[b, :k], (name, b, "poses"))
        assert np.all(got["out"][b, k:] == sc.SENTINEL), (name, b, "a row behind the count was written")


@pytest.mark.parametrize("case", sc.SEED_CASES, ids=[sc.seed_tag(c) for c in sc.SEED_CASES])
def test_seeder(case, want):
    got = sc.run_seed(case)["traj"]
    assert np.isfinite(got).all()
    _same(got, want["seed_%s_traj" % sc.seed_tag(case)], case)
