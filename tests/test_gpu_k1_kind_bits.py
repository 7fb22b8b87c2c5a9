"""GPU: the 32x32 ONF kernel's outputs, bit for bit, against tests/golden/k1_kind_bits.npz -- recorded by
tools/x32/record_k1_kind_bits.py from the build in front of the compile-time feature kinds of csrc/onf_x32_impl.h (Cfg::
group_kind: the input blocks from FS on evaluate each four-slot group by its kind instead of both argument forms and a
select, in L1 and in the last output tile's chain-rule epilogue; no product, sum or its order touched).  Every comparison
is np.array_equal on the words, so NaN payloads and the sign of zero count.

Cases (tests/k1_kind_bits_cases.py): pose mode at P = 33 / 65 for each of the four feature dimensions; poses with theta < 0,
-0, +0, > 0, +-pi at a random place and at u_x = u_y = 0 (the pads that share a group with angle features see both signs of
zero in the angle form); trajectory mode at B = 2, N = 5; the fit's pass-1 factors at P = 33 for 220 inputs and for 120,
the shape with a group whose lane halves hold different kinds."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import k1_kind_bits_cases as kk  # noqa: E402


@pytest.fixture(scope="module")
def got():
    return kk.run_cases()


@pytest.fixture(scope="module")
def want():
    return load_golden("k1_kind_bits.npz")


def _same(got, want, name):
    assert name in want.files, name
    a, b = np.asarray(got[name]), want[name]
    assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == np.float32:   # compare the words: NaN payloads and the sign of zero count
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    assert np.array_equal(a, b), (name, int((a != b).sum()), "words differ")


def test_fixture_and_cases_name_the_same_arrays(got, want):
    assert sorted(got) == sorted(want.files)


@pytest.mark.parametrize("fin", sorted(kk.DIMS))
def test_parameters_are_the_recorded_ones(fin, got, want):
    """not the kernel: the initialiser under the fixed seed (a mismatch here explains every other one)"""
    _same(got, want, "params_sum_F%d" % fin)


@pytest.mark.parametrize("P", kk.POSE_P)
@pytest.mark.parametrize("fin", sorted(kk.DIMS))
def test_pose_mode(fin, P, got, want):
    _same(got, want, "pose_F%d_P%d" % (fin, P))


@pytest.mark.parametrize("fin", sorted(kk.DIMS))
def test_poses_at_the_signs_of_zero(fin, got, want):
    x = kk.edge_poses(fin)
    assert np.isfinite(got["edge_F%d" % fin]).all()
    if kk.DIMS[fin][1]:   # the cases hold what they are for: both signs of theta, both zeros, u = 0
        th = x[:, 2]
        assert (th < 0).any() and (th > 0).any() and (np.signbit(th) & (th == 0)).any() and (~np.signbit(th) & (th == 0)).any()
    assert (x[:, 0] == np.float32(kk.MEAN)).any()
    _same(got, want, "edge_F%d" % fin)


@pytest.mark.parametrize("fin", kk.TRAJ_DIMS)
def test_trajectory_mode(fin, got, want):
    _same(got, want, "traj_F%d" % fin)


@pytest.mark.parametrize("fin", kk.FIT_DIMS)
def test_fit_pass1_factors(fin, got, want):
    for part in ("h1", "dh1", "de", "rec"):
        _same(got, want, "fit_F%d_P%d_%s" % (fin, kk.FIT_P, part))
