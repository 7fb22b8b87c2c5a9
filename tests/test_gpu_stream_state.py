"""GPU: library state that is keyed by stream -- the per-stream weight image of csrc/onf_x32_impl.h (tagged with the buffer,
its content version and the geometry it was built from), the per-stream blobs of csrc/onf_split.hip and the 16-slot pool
with least-recently-used eviction both live in (StreamScratch, csrc/common.h).

Two fields of one configuration with different parameters (A: the golden parameters, B: the same times 1.25) and one 300-pose
input.  Whatever stream a launch runs on, whatever ran on that stream before and whichever slot it was given, its output is
its field's baseline bit for bit.  Streams only, one process, nothing captured."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
from nfopp import _lib  # noqa: E402

N_STREAMS = 18     # two more than StreamScratch keeps buffers for


@pytest.fixture(params=[1, 2, 0])
def matrix_path(request):
    lib = _lib.load()
    before = lib.nfopp_get_matrix_path()
    _lib.check(lib.nfopp_set_matrix_path(request.param))
    assert lib.nfopp_get_matrix_path() == request.param
    yield request.param
    _lib.check(lib.nfopp_set_matrix_path(before))   # the switch is process-wide: leave it as it was found


def _fields(tag="a"):
    z = load_golden("g1_onf.npz")
    a, _ = gc.make_onf(z[tag + "_cfg"], z[tag + "_params"])
    b, _ = gc.make_onf(z[tag + "_cfg"], z[tag + "_params"])
    with torch.no_grad():
        b.flat_parameters.mul_(1.25)       # the same device multiplication the eviction test applies to A in place
    x = torch.tensor(np.resize(z[tag + "_x"], (300, z[tag + "_x"].shape[1])), device="cuda")
    return a, b, x


def _baseline(onf, x):
    out = onf.forward_with_grad(x).clone()
    torch.cuda.synchronize()
    return out


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fork(streams):
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)


def _join(streams):
    cur = torch.cuda.current_stream()
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()


def _on(stream, onf, x):
    with torch.cuda.stream(stream):
        return onf.forward_with_grad(x)


@pytest.mark.parametrize("frozen", [False, True])
def test_two_fields_on_two_streams(matrix_path, frozen):
    a, b, x = _fields()
    base_a, base_b = _baseline(a, x), _baseline(b, x)
    assert not _bits_equal(base_a, base_b)
    if frozen:
        a.freeze()
        b.freeze()
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for _ in range(2):
            _fork([s1, s2])
            outs = [(_on(s1, a, x), base_a), (_on(s2, b, x), base_b), (_on(s1, b, x), base_b), (_on(s2, a, x), base_a),
                    (_on(s1, a, x), base_a), (_on(s2, a, x), base_a)]
            _join([s1, s2])
            for k, (got, want) in enumerate(outs):
                assert _bits_equal(got, want), (matrix_path, frozen, k)
    finally:
        a.unfreeze()
        b.unfreeze()


def test_eviction_and_parameter_writes_seen_from_eighteen_streams(matrix_path):
    a, b, x = _fields()
    base_a, base_b = _baseline(a, x), _baseline(b, x)
    original = a.flat_parameters.clone()
    streams = [torch.cuda.Stream() for _ in range(N_STREAMS)]
    assert len({s.cuda_stream for s in streams}) == N_STREAMS      # eighteen distinct streams: the pool must evict
    a.freeze()
    try:
        _fork(streams)
        outs = [_on(s, a, x) for _ in range(2) for s in streams]   # launches 17 and 18 evict; the second pass re-acquires
        _join(streams)
        assert len(outs) == 2 * N_STREAMS
        for k, got in enumerate(outs):
            assert _bits_equal(got, base_a), (matrix_path, "pass", k // N_STREAMS, "stream", k % N_STREAMS)
        # an in-place torch write: the version counter moves, every stream's image is stale
        with torch.no_grad():
            a.flat_parameters.mul_(1.25)
        _fork(streams)
        outs = [_on(s, a, x) for s in streams]
        _join(streams)
        for k, got in enumerate(outs):
            assert _bits_equal(got, base_b), (matrix_path, "after mul_", k)
        # a write the counter does not see, announced with mark_modified()
        a.flat_parameters.data.copy_(original)
        a.mark_modified()
        _fork(streams)
        outs = [_on(s, a, x) for s in streams]
        _join(streams)
        for k, got in enumerate(outs):
            assert _bits_equal(got, base_a), (matrix_path, "after restore", k)
    finally:
        a.unfreeze()


@pytest.mark.parametrize("frozen", [False, True])
def test_a_field_of_another_geometry_on_a_stream_that_holds_an_image(matrix_path, frozen):
    big, _, x_big = _fields("a")        # F = 220
    small, _, x_small = _fields("c")    # F = 100
    assert big.feature_dim == 220 and small.feature_dim == 100
    base_big, base_small = _baseline(big, x_big), _baseline(small, x_small)
    if frozen:
        big.freeze()
        small.freeze()
    try:
        side = torch.cuda.Stream()
        _fork([side])
        outs = [(_on(side, big, x_big), base_big), (_on(side, small, x_small), base_small), (_on(side, big, x_big), base_big),
                (_on(side, small, x_small), base_small)]
        _join([side])
        for k, (got, want) in enumerate(outs):
            assert _bits_equal(got, want), (matrix_path, frozen, k)
    finally:
        big.unfreeze()
        small.unfreeze()
