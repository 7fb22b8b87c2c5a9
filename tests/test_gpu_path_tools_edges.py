"""GPU: csrc/path_post.hip and csrc/traj_init.hip at their edges, against the reference's own bytes
(tests/golden/g22_path_tools.npz; tolerances and what they come from: tests/path_tools_edges.py; the cases and why each
proves something: tests/golden/make_golden_path_tools.py and tests/test_path_tools_edges_cpu.py), and the batch / C-ABI
behaviour of the post-processor (mixed batches, max_out below the need, input forms, batch position) against the oracle,
which the CPU tests hold to the same fixture.

Measured on MI355X (largest |kernel - fixture| / max(1, max |coordinate|) over the cases): see DESIGN.md, section 8(f)."""
import numpy as np
import pytest
import torch

import path_tools_edges as pe
from conftest import max_abs

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
from nfopp import _lib  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402

F32 = np.float32
SENTINEL = -12345.678


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x, dtype=F32), device="cuda")


def _raw(paths, md, step, max_out, fill=SENTINEL):
    """nfopp_path_postprocess through the C ABI -> (out [B, max_out, 3] float64 or None, counts [B])"""
    paths = _dev(paths)
    b, n, _ = paths.shape
    counts = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((b, max_out, 3), fill, dtype=torch.float64, device="cuda") if max_out else None
    _lib.check(_lib.load().nfopp_path_postprocess(_lib.ptr(paths), b, n, float(md), float(step), max_out,
                                                  _lib.ptr(out, torch.float64) if max_out else None,
                                                  _lib.ptr(counts, torch.int32), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return (out.cpu().numpy() if max_out else None), counts.cpu().numpy()


@pytest.mark.parametrize("name", pe.post_names())
def test_post_processor_case_vs_reference(name):
    path, md, step, want, err = pe.post_case(name)
    pp = nfopp.PathPostprocessor(md, step)
    if err is not None:
        assert err == "ValueError"
        with pytest.raises(ValueError):                          # what the reference raised
            pp.process_batch(path[None])
        assert _raw(path[None], md, step, 0)[1][0] == -1
        return
    out, counts = pp.process_batch(path[None])
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert counts[0] == len(want) and out.shape == (1, len(want), 3) and out.dtype == np.float64
    if len(want):
        tol_xy, tol_th = pe.device_tol(want)
        s = pe.scale_of(want)
        assert np.isfinite(out).all()
        d_xy, d_th = max_abs(out[0, :, :2], want[:, :2]), max_abs(out[0, :, 2], want[:, 2])
        print("%s: count %d, |kernel - reference| / scale: xy %.3e heading %.3e (tolerance %.3e / %.3e)" % (
            name, len(want), d_xy / s, d_th / s, tol_xy / s, tol_th / s))
        assert d_xy <= tol_xy and d_th <= tol_th
        # the drop-in call returns the same poses
        res = pp.process(nfopp.Position2.from_vec(path.copy())).as_vec()
        assert np.array_equal(res, out[0])


def _scaled_paths():
    """[5, 10, 3]: one 10-pose curve at five sizes -> counts 0, 1 (nothing kept), many, and more"""
    s = np.linspace(0, 1, 10)
    base = np.stack([s, 0.3 * np.sin(2 * s), 0.6 * np.cos(2 * s)], 1)
    paths = np.stack([base * [k, k, 1] for k in (0.04, 0.09, 3.0, 7.5, 0.17)]).astype(F32)
    return paths


def test_mixed_batch_with_a_collapsing_path():
    paths = _scaled_paths()
    want = [orc.path_postprocess(p, 0.001, 0.05) for p in paths]
    assert [len(w) for w in want[:2]] == [0, 0] and len(want[4]) == 2 and min(len(want[2]), len(want[3])) > 50
    collapsing = paths[2].copy()
    collapsing[1:-1, :2] = collapsing[-1, :2] + F32(4e-4)       # every interior pose within 1 mm of the goal
    with pytest.raises(ValueError):
        orc.path_postprocess(collapsing, 0.001, 0.05)
    mixed = np.concatenate([paths[:3], collapsing[None], paths[3:]])
    cap = max(len(w) for w in want)
    out, counts = _raw(mixed, 0.001, 0.05, cap)
    assert counts.tolist() == [len(w) for w in want[:3]] + [-1] + [len(w) for w in want[3:]]
    assert np.all(out[3] == SENTINEL)                           # the collapsing path writes nothing
    for b, w in zip((0, 1, 2, 4, 5), want):
        assert max_abs(out[b, :len(w)], w) <= 1e-11 * pe.scale_of(w) if len(w) else True
        assert np.all(out[b, len(w):] == SENTINEL)
    with pytest.raises(ValueError):
        nfopp.PathPostprocessor().process_batch(mixed)
    # without it: rows beyond each path's count are exactly zero
    out, counts = nfopp.PathPostprocessor().process_batch(paths)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert counts.tolist() == [len(w) for w in want] and out.shape == (5, cap, 3)
    for b, w in enumerate(want):
        assert np.all(out[b, len(w):] == 0.0) and (len(w) == 0 or max_abs(out[b, :len(w)], w) <= 1e-11 * pe.scale_of(w))


def test_max_out_smaller_than_the_need():
    paths = _scaled_paths()
    want = [orc.path_postprocess(p, 0.001, 0.05) for p in paths]
    full, counts_full = _raw(paths, 0.001, 0.05, max(len(w) for w in want))
    for max_out in (1, 7, len(want[2]), len(want[2]) + 1):
        out, counts = _raw(paths, 0.001, 0.05, max_out)
        assert np.array_equal(counts, counts_full) and counts.tolist() == [len(w) for w in want]   # the full need
        for b in range(len(paths)):
            k = min(counts[b], max_out)
            assert np.array_equal(out[b, :k], full[b, :k])
            assert np.all(out[b, k:] == SENTINEL)               # not one row more
    assert np.array_equal(_raw(paths, 0.001, 0.05, 0)[1], counts_full)      # max_out 0, null output: counts only


def test_input_forms_give_the_same_bytes():
    paths = np.stack([pe.post_case(n)[0] for n in ("len_130", "cb_curved_130", "cb_straight_130")])
    pp = nfopp.PathPostprocessor(0.001, 0.25)
    want, want_counts = pp.process_batch(_dev(paths))
    wide = torch.zeros(3, 130, 6, dtype=torch.float64, device="cuda")
    wide[:, :, ::2] = torch.tensor(paths, dtype=torch.float64, device="cuda")
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous() and strided.dtype == torch.float64
    for form in (strided, paths, paths.astype(np.float64)):
        out, counts = pp.process_batch(form)
        assert torch.equal(out, want) and torch.equal(counts, want_counts)


def test_result_does_not_depend_on_the_batch_position():
    path, md, step, want, _ = pe.post_case("cb_curved_1026")    # its count flips with the summation order
    rng = np.random.default_rng(22)
    batch = np.repeat(path[None], 257, 0)
    batch[:, :, 1] += (rng.uniform(0.5, 2, (257, 1)) * np.sin(np.linspace(0, 9, 1026))[None]).astype(F32)
    where = (0, 128, 256)
    batch[list(where)] = path
    out, counts = nfopp.PathPostprocessor(md, step).process_batch(batch)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    single = nfopp.PathPostprocessor(md, step).process_batch(path[None])[0].cpu().numpy()[0]
    assert len(single) == len(want)
    for b in where:
        assert counts[b] == len(want) and np.array_equal(out[b, :counts[b]], single)
        assert np.all(out[b, counts[b]:] == 0.0)
    assert len(set(counts.tolist())) > 1                         # the other paths are different ones


@pytest.mark.parametrize("n", pe.INIT_SIZES)
def test_initialiser_cases_vs_reference(n):
    names, cases, plain, directed = pe.init_cases(n)
    s, g = _dev(cases[:, :3]), _dev(cases[:, 3:])
    got = nfopp.init_trajectories(s, g, n).cpu().numpy()
    for c, name in enumerate(names):                             # xy and plain headings: bit for bit, +-pi included
        assert np.array_equal(got[c], plain[c]), (name, max_abs(got[c], plain[c]))
    got2 = nfopp.init_trajectories(s[:, :2].contiguous(), g[:, :2].contiguous(), n).cpu().numpy()
    assert np.array_equal(got2, plain[..., :2])
    got = nfopp.init_trajectories(s, g, n, init_angles_with_trajectory=True).cpu().numpy()
    assert np.array_equal(got[..., :2], plain[..., :2])
    tol = pe.init_heading_tol(plain, directed)
    diff = np.abs(got[..., 2].astype(np.float64) - directed).max(1)
    worst = int(np.argmax(diff / tol))
    print("N = %d: directed headings, worst case %s: |kernel - reference| %.3e (tolerance %.3e)" % (
        n, names[worst], diff[worst], tol[worst]))
    assert np.all(diff <= tol), [(names[c], diff[c], tol[c]) for c in np.nonzero(diff > tol)[0]]
