"""CPU: the 32x32 ONF kernels fix the feature kinds of their last input blocks at compile time (csrc/onf_x32_impl.h,
Cfg::group_kind), one geometry per block count -- (n_enc, fin, angle_dim) = 200/220/10, 200/200/0, 100/120/10, 100/100/0.
Another angle dimension lands in the same number of 16-wide blocks and would be evaluated with the wrong kinds: the family's
launcher (csrc/onf_x32.hip: launch_x32) refuses it with NFOPP_ERR_ARG in front of every HIP call, so this needs no GPU.
Where a device is present the buffers are real and large enough for the refused geometry all the same."""
import ctypes

import pytest
import torch

import nfopp
from nfopp import _lib

# (use_cos, angle_dim) -> input blocks of the 32x32 kernel the geometry is routed to, (fin + 16) / 16
REFUSED = [((1, 5), 14), ((1, 11), 14), ((1, 2), 13), ((0, 3), 7), ((0, 6), 8), ((0, 11), 8)]
P = 8


def _buffers(cfg, n_params):
    if torch.cuda.is_available():
        bufs = [torch.zeros(n_params, device="cuda"), torch.zeros(P, 3, device="cuda"), torch.zeros(P, 4, device="cuda")]
        return bufs, [_lib.ptr(b) for b in bufs], _lib.stream_ptr()
    host = [(ctypes.c_float * n) () for n in (n_params, 3 * P, 4 * P)]     # never read: the refusal comes first
    return host, [ctypes.cast(h, ctypes.c_void_p) for h in host], None


@pytest.fixture()
def lib():
    lib = nfopp.load_library()
    before = lib.nfopp_get_matrix_path()
    assert lib.nfopp_set_matrix_path(1) == 0
    yield lib
    assert lib.nfopp_set_matrix_path(before) == 0


@pytest.mark.parametrize("shape,nkb", REFUSED)
def test_the_32x32_launcher_refuses_a_geometry_its_kind_table_was_not_written_for(lib, shape, nkb):
    use_cos, angle_dim = shape
    cfg = _lib.OnfConfigC(0.0, 1.0, use_cos, 1, angle_dim)
    n_params = lib.nfopp_onf_param_count(cfg)
    assert n_params > 0
    fin = (200 if use_cos else 100) + 2 * angle_dim
    assert (fin + 16) // 16 == nkb
    keep, (params, pts, out), stream = _buffers(cfg, n_params)
    for fn in (lib.nfopp_onf_eval_points, lib.nfopp_onf_eval_logits):
        rc = fn(cfg, params, pts, P, out, stream)
        msg = lib.nfopp_last_error().decode()
        assert rc == -1, (rc, msg)
        assert "%d input blocks" % nkb in msg and "fin %d" % fin in msg and "angle_dim %d" % angle_dim in msg, msg
    del keep


def test_the_stock_geometries_are_the_ones_the_tables_name():
    """the four shapes of nfopp.ONF, against the constants the refusal message quotes for each block count"""
    stock = {14: (200, 220, 10), 13: (200, 200, 0), 8: (100, 120, 10), 7: (100, 100, 0)}
    for use_cos in (True, False):
        for angle in (True, False):
            onf = nfopp.ONF(0.0, 1.0, use_cos=use_cos, use_normal_init=True, bias=True, angle_encoding=angle)
            c = onf.config_c()
            n_enc = 200 if c.use_cos else 100
            fin = n_enc + 2 * c.angle_dim
            assert stock[(fin + 16) // 16] == (n_enc, fin, c.angle_dim)
