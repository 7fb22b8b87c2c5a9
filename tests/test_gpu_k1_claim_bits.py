"""GPU: the 32x32 ONF kernel hands the tiles of a workgroup's chunks to whichever wave claims them (csrc/onf_x32_impl.h,
"Tiles by claim"); the bits of every output row stay those of the fixed walk.  tests/golden/k1_claim_bits.npz was recorded by
tools/x32/record_k1_claim_bits.py on the build in front of that change.

Cases (tests/k1_claim_cases.py): pose and forward-only launches at the pool edges of both workgroup shapes for 220 inputs,
two of them for 100, one trajectory launch with every third trajectory retired.  For every case
  (a) the sha256 of the output rows and the first and last 64 rows equal the fixture (np.array_equal);
  (b) the buffer is filled with a NaN payload pattern and has 64 guard rows: no word of a row the launch owns keeps the
      pattern, the guard rows and the rows of retired trajectories keep every word of it (the draws of the trajectory
      launch likewise);
  (c) eight launches give identical bytes -- the assignment of tiles to waves differs from launch to launch, the results
      must not."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import k1_claim_cases as cc  # noqa: E402
from nfopp import _lib  # noqa: E402


@pytest.fixture(scope="module")
def want():
    return load_golden("k1_claim_bits.npz")


@pytest.fixture(scope="module")
def runner():
    return cc.Runner()


def test_fixture_was_recorded_for_this_device_and_these_parameters(runner, want):
    """not the kernel: the CU count fixes the threshold between the shapes, the seed the parameters"""
    assert int(want["cus"]) == cc.threshold() // 256, "the fixture was recorded on a device with another CU count"
    for fin, onf in runner.onf.items():
        assert np.array_equal(cc.kc.wsum(onf.flat_parameters.cpu().numpy()), want["params_sum_F%d" % fin])
    assert sorted(want.files) == sorted(["cus", "params_sum_F220", "params_sum_F100"]
                                        + [n + s for n in cc.case_names() for s in ("_sha", "_head", "_tail")])


@pytest.mark.parametrize("name", cc.case_names())
def test_bits_extent_and_repeatability(name, runner, want):
    _lib.check(_lib.load().nfopp_set_matrix_path(1))     # (conftest puts the process back on the path it was on)
    first, rows = runner.run(name)
    torch.cuda.synchronize()
    # (a) the recorded bits
    sha, head, tail = cc.digest(first, rows)
    assert np.array_equal(head, want[name + "_head"]), (name, "first rows differ")
    assert np.array_equal(tail, want[name + "_tail"]), (name, "last rows differ")
    assert np.array_equal(sha, want[name + "_sha"]), (name, "hash differs")
    # (b) what the launch wrote and what it left alone
    kept = (first == cc.PATTERN).cpu().numpy()
    assert kept[rows:].all(), (name, "guard rows written")
    if name == "traj_F220":
        retired = runner.retired_rows()
        assert kept[:rows][retired].all(), (name, "rows of retired trajectories written")
        assert not kept[:rows][~retired].any(), (name, "live rows keep the fill pattern")
        drawn = (runner.last_draws == cc.PATTERN).cpu().numpy()       # the draws t: one word per row, then the guard
        assert drawn[rows:].all(), (name, "guard words of the draws written")
        assert drawn[:rows][retired].all() and not drawn[:rows][~retired].any(), (name, "draws of the wrong rows written")
    else:
        assert not kept[:rows].any(), (name, "rows below P keep the fill pattern")
    # (c) launch after launch the same bytes
    for k in range(1, cc.REPEATS):
        again, _ = runner.run(name)
        assert torch.equal(again, first), (name, "launch %d differs from the first" % k)
