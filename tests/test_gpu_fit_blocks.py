"""GPU: the fit's summed gradient, block by block against float64 (tests/fit_blocks_gate.py), at every chunk-count edge of
pass 2 and of the per-sample reduction (tests/fit_blocks_cases.py, for this device's CU count): nfopp_onf_train_grad_ex with
fit path 2 on matrix paths 1, 2 and 0 and with fit path 1 (per-sample).

Every launch gets a workspace of exactly nfopp_onf_train_workspace_bytes bytes and a gradient buffer, both filled with NaN
(include/nfopp_hip.h promises neither needs initialisation), and guard words behind the workspace that must not change.
After it: all ten blocks and the loss within the gate, the count slot = P, every word finite, a second launch bit-equal.

`python tests/test_gpu_fit_blocks.py` runs every case and prints the table kept in profiles/fit_blocks.txt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
from nfopp import _lib  # noqa: E402

import bits_float64_gate as bg  # noqa: E402
import fit_blocks_cases as fc  # noqa: E402
import fit_blocks_gate as fg  # noqa: E402
import k1_bits_cases as kc  # noqa: E402

CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
# (tag, fit path, matrix path, chunk length of the yardstick)
LAUNCHES = (("fit2 path1", 2, 1, 32), ("fit2 path2", 2, 2, 32), ("fit2 path0", 2, 0, 16), ("per-sample", 1, 1, 32))
GUARD_WORDS, FILL = 1024, 0x7FC12345        # a quiet NaN with a payload no kernel writes


def launch(onf, x, y, fit_path, matrix_path):
    """one nfopp_onf_train_grad_ex call on NaN-filled buffers -> gradient | loss | count, fp32 [n_params + 2]"""
    lib = _lib.load()
    before = lib.nfopp_get_matrix_path()
    _lib.check(lib.nfopp_set_matrix_path(matrix_path))
    try:
        P = x.shape[0]
        c = onf.config_c()
        need = lib.nfopp_onf_train_workspace_bytes(c, P)
        assert need > 0 and need % 4 == 0
        ws = torch.full((need // 4 + GUARD_WORDS,), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
        grad = torch.full((onf.n_params + 2,), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        _lib.check(lib.nfopp_onf_train_grad_ex(c, _lib.ptr(onf.flat_parameters), _lib.ptr(xd), _lib.ptr(yd), P, 1.0 / P, _lib.ptr(grad),
                                               _lib.ptr(ws), need, fit_path, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((ws[need // 4:].view(torch.int32) == FILL).all()), "words behind the workspace were written"
        return grad.cpu().numpy()
    finally:
        _lib.check(lib.nfopp_set_matrix_path(before))


def run_case(fin, P, onf=None):
    """every launch of the case (F, P) against one shared reference -> [Row]"""
    ref = fg.reference(fin, P, CUS)
    onf = kc.make_onf(fin) if onf is None else onf
    assert np.array_equal(onf.flat_parameters.cpu().numpy(), fg.network(fin)[0]), "the device network is not the CPU one"
    rows = []
    for tag, fit_path, matrix_path, K in LAUNCHES:
        g = launch(onf, ref["x"], ref["y"], fit_path, matrix_path)
        new = fg.compare(tag, ref, g, K)
        bg.fact(new, new[0].family, new[0].case, "every word is finite", np.isfinite(g).all())
        again = launch(onf, ref["x"], ref["y"], fit_path, matrix_path)
        bg.fact(new, new[0].family, new[0].case, "a second launch gives the same words",
                np.array_equal(g.view(np.uint32), again.view(np.uint32)))
        rows += new
    return rows


@pytest.mark.parametrize("fin,P", fc.cases(CUS))
def test_fit_gradient_block_by_block(fin, P):
    rows = run_case(fin, P)
    print("\n".join(fg.table(rows)))
    assert len(rows) == len(LAUNCHES) * (len(fg.network(fin)[1].layout()) + 4)
    assert not bg.failures(rows), bg.failures(rows)


def test_automatic_path_switches_at_2048_samples():
    """fit path 0 is the per-sample path up to 2047 samples and the MFMA path from 2048, word for word"""
    fin = 220
    onf = kc.make_onf(fin)
    flat, cfg = fg.network(fin)
    for P, same, other in ((2047, 1, 2), (2048, 2, 1)):
        x, y = fc.inputs(fin, P, flat, cfg)
        auto = launch(onf, x, y, 0, 1).view(np.uint32)
        assert np.array_equal(auto, launch(onf, x, y, same, 1).view(np.uint32)), P
        assert not np.array_equal(auto, launch(onf, x, y, other, 1).view(np.uint32)), P


if __name__ == "__main__":
    rows = []
    for fin, P in fc.cases(CUS):
        rows += run_case(fin, P)
    print("%d compute units, %d cases, %d outside the gate" % (CUS, len(fc.cases(CUS)), len(bg.failures(rows))))
    print("\n".join(fg.table(rows)))
    print("\n".join(bg.failures(rows)))
