"""GPU: the 32x32 ONF kernel's outputs, bit for bit, against tests/golden/k1_bits.npz -- recorded by
tools/x32/record_k1_bits.py from the build in front of the vector-instruction diet of csrc/onf_x32_impl.h (address forming,
register copies and arithmetic on constant zeros removed; no product, sum or its order touched).  The planner is chaotic
over a few hundred steps, so "the same results" means the same bits here: every comparison is np.array_equal.

Cases (tests/k1_bits_cases.py): pose mode at P = 1 / 33 / 255 / 257, trajectory mode at B = 3, N = 9 and forward-only logits
at P = 257 for each of the four feature dimensions; one pose launch of CUs x 256 + 31 points on the 512-thread shape; the fit's
pass-1 factors at P = 33 / 257 for 220 and 100 inputs."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import k1_bits_cases as kc  # noqa: E402


@pytest.fixture(scope="module")
def got():
    return kc.run_cases()


@pytest.fixture(scope="module")
def want():
    return load_golden("k1_bits.npz")


def _same(got, want, name):
    assert name in want.files, name
    a, b = np.asarray(got[name]), want[name]
    assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == np.float32:   # compare the words: NaN payloads and the sign of zero count
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    assert np.array_equal(a, b), (name, int((a != b).sum()), "words differ")


def test_fixture_and_cases_name_the_same_arrays(got, want):
    assert sorted(got) == sorted(want.files)


@pytest.mark.parametrize("fin", sorted(kc.DIMS))
def test_parameters_are_the_recorded_ones(fin, got, want):
    """not the kernel: the initialiser under the fixed seed (a mismatch here explains every other one)"""
    _same(got, want, "params_sum_F%d" % fin)


@pytest.mark.parametrize("P", kc.POSE_P)
@pytest.mark.parametrize("fin", sorted(kc.DIMS))
def test_pose_mode(fin, P, got, want):
    _same(got, want, "pose_F%d_P%d" % (fin, P))


@pytest.mark.parametrize("fin", sorted(kc.DIMS))
def test_trajectory_mode(fin, got, want):
    _same(got, want, "traj_F%d" % fin)


@pytest.mark.parametrize("fin", sorted(kc.DIMS))
def test_forward_only_logits(fin, got, want):
    _same(got, want, "logits_F%d" % fin)
    assert np.array_equal(got["logits_F%d" % fin][:, 1:], np.zeros((257, 3), np.float32))


def test_pose_mode_on_the_512_thread_shape_with_a_ragged_last_chunk(got, want):
    assert int(got["big_count"]) == int(want["big_count"]), "the fixture was recorded on a device with another CU count"
    _same(got, want, "big_rows")
    _same(got, want, "big_sum")


@pytest.mark.parametrize("P", kc.FIT_P)
@pytest.mark.parametrize("fin", kc.FIT_DIMS)
def test_fit_pass1_factors(fin, P, got, want):
    for part in ("h1", "dh1", "de", "rec"):
        name = "fit_F%d_P%d_%s" % (fin, P, part)
        if P == 33:
            _same(got, want, name)
        else:
            for suffix in ("_rows", "_rowsum", "_colsum"):
                _same(got, want, name + suffix)
