"""CPU: the table, cases and comparers of tests/onf_geometry_cases.py, without a GPU.

  yardstick   at all 28 accepted geometries (and the three networks without an encoding bias) the fp32 oracle agrees with
              float64_ref within the parity tolerances, so the yardstick of the GPU gate is sane everywhere; no pose is left
              out of a comparison
  plants      errors of the kind the 16x16 kernels would make with a tile count that is one short, applied to the oracle's
              output: each must be rejected by the comparers the GPU test uses, at every geometry that has the position
  refusals    the unsupported and out-of-range angle dimensions are refused in front of every HIP call (host buffers), and
              so is every non-stock geometry on matrix path 1 (tests/test_x32_geometry_cpu.py pins six of them)"""
import ctypes

import numpy as np
import pytest
import torch

import nfopp
from nfopp import _lib
from oracle import nfopp_oracle as orc

import bits_float64_gate as bg
import fit_blocks_gate as fg
import float64_ref as f64
import onf_geometry_cases as gc

F64 = np.float64


# ----------------------------------------------------------------------------------------------------------
# the table itself
def test_the_table_lists_all_34_pairs_and_28_accepted_geometries():
    assert len(gc.TABLE) == 34 and set(gc.TABLE) == {(uc, ad) for uc in (0, 1) for ad in range(17)}
    assert len(gc.ACCEPTED) == 28 and len(gc.UNSUPPORTED) == 6
    assert gc.UNSUPPORTED == ((0, 15), (0, 16), (1, 13), (1, 14), (1, 15), (1, 16))
    for (uc, ad), e in gc.TABLE.items():
        assert e.fin == (200 if uc else 100) + 2 * ad
        if (uc, ad) in gc.UNSUPPORTED:
            assert set(e.inf) | set(e.fit) | {e.per_sample} == {"U"}
            continue
        # every feature has a tile under layout P, and the last tile holds one
        used = {(2 * (f >> 5) + ((f >> 3) & 1)) for f in range(e.fin)}
        assert max(used) + 1 == e.tiles and e.tiles in (7, 8, 13, 14)
        assert e.inf[0] == "fp32" and e.inf[2] == "s16" and e.per_sample == "ok"
        assert (e.inf[1] == "x32") == ((uc, ad) in gc.STOCK)
        assert (e.inf[1] == "s16") == (e.fin in (128, 224)) == (set(e.fit) == {"pad"})
    for geom in gc.NO_BIAS:
        assert geom not in gc.STOCK
    assert sorted({gc.TABLE[g].tiles for g in gc.NO_BIAS}) == [7, 8, 14]


def test_the_stock_geometries_of_the_table_are_the_ones_nfopp_builds():
    for use_cos in (True, False):
        for angle in (True, False):
            c = nfopp.ONF(0.0, 1.0, use_cos=use_cos, use_normal_init=True, bias=True, angle_encoding=angle).config_c()
            assert (int(c.use_cos), int(c.angle_dim)) in gc.STOCK


# ----------------------------------------------------------------------------------------------------------
# yardstick
@pytest.mark.parametrize("geom", gc.NETWORKS, ids=gc.name)
def test_the_oracle_agrees_with_float64_at_every_geometry(geom):
    flat, cfg = gc.network(*geom)
    assert np.all(flat[:2 * cfg.angle_dim] != 0) and np.array_equal(flat[2 * cfg.angle_dim:4 * cfg.angle_dim], np.tile(np.arange(1, cfg.angle_dim + 1), 2))
    ref = gc.inference_reference(*geom)
    sl, sg = ref["scale"]
    assert sl > 1e-2 and sg > 1e-3
    for P in gc.POSE_P:
        r = ref[P]
        assert r["x"].shape == (P, cfg.point_dim) and r["kink"].min() >= gc.KINK_MARGIN      # no row is left out
        e_logit, e_grad = np.abs(r["o32_logit"] - r["logit"]).max(), np.abs(r["o32_grad"] - r["grad"]).max()
        assert 0 < e_logit <= bg.PARITY["logit"] * sl and 0 < e_grad <= bg.PARITY["grad"] * sg
        # the oracle passes its own gate
        out = np.zeros((P, 4), np.float32)
        out[:, 0], out[:, 1:1 + cfg.point_dim] = r["o32_logit"], r["o32_grad"]
        fwd = np.zeros((P, 4), np.float32)
        fwd[:, 0] = r["o32_logit"]
        rows = gc.compare_inference("oracle32", geom, P, ref, out, fwd)
        assert len(rows) == (5 if cfg.point_dim == 2 else 4) and not bg.failures(rows), bg.failures(rows)


@pytest.mark.parametrize("geom", gc.NETWORKS, ids=gc.name)
def test_the_fit_yardstick_at_every_geometry(geom):
    ref = gc.fit_reference(*geom)
    assert ref["P"] == gc.FIT_P and ref["kink"].min() >= gc.KINK_MARGIN and ref["masks_agree"]
    o_grad, o_loss = ref["o32"]
    assert np.abs(o_grad - ref["grad"]).max() <= ref["old_grad"] and abs(o_loss - ref["loss"]) <= ref["old_loss"]
    for K in (16, 32):
        assert 1.0 <= ref["Y"][K] < 64
        for g, loss in (ref["o32"], ref["chunked"][K]):
            rows = gc.compare_fit("cpu", geom, ref, fg.output_of(g, loss, gc.FIT_P), K)
            assert len(rows) == len(ref["cfg"].layout()) + 2 and not bg.failures(rows), bg.failures(rows)


# ----------------------------------------------------------------------------------------------------------
# planted errors
def _last_tile_positions(cfg):
    """the positions of layout-P tile 7 (13) below F: 104 .. 111 (200 .. 207)"""
    first = 200 if cfg.use_cos else 104
    return np.arange(first, min(first + 8, cfg.feature_dim))


def _with(flat, cfg, change):
    """float64 parameters with `change(p)` applied to the named views"""
    p = f64.unpack64(flat, cfg)
    p = {k: v.copy() for k, v in p.items()}
    change(p)
    return np.concatenate([p[k].reshape(-1) for k, _ in cfg.layout()])


def _drop_forward(cols):
    def change(p):
        p["w1"][:, cols] = 0
        p["w3"][0, 100 + cols] = 0
    return change


def _cos_as_sin(p):       # cos(z) = sin(z + pi/2): the last (cosine) position as sin((theta + b) f)
    p["ang_b"][-1] -= np.pi / (2 * p["ang_f"][-1])


def _swap_f_b(p):
    p["ang_f"][-1], p["ang_b"][-1] = p["ang_b"][-1], p["ang_f"][-1]


def _planted_out(r, flat, cfg, planted_flat=None, grad_drop=None):
    """the oracle's out4 with the effect of the plant (float64 difference of the planted and the clean network) added"""
    P, dim = r["x"].shape
    logit, grad = r["o32_logit"].astype(F64), r["o32_grad"].astype(F64)
    if planted_flat is not None:
        c = f64.onf_eval64(planted_flat, cfg, r["x"])
        logit, grad = logit + (c["logit"] - r["logit"]), grad + (c["grad"] - r["grad"])
    if grad_drop is not None:
        p = f64.unpack64(flat, cfg)
        pos, ang = grad_drop[grad_drop < cfg.n_enc], grad_drop[grad_drop >= cfg.n_enc]
        grad = grad.copy()
        grad[:, :2] -= r["darg"][:, pos] @ p["we"][pos] / cfg.sigma
        if len(ang):
            grad[:, 2] -= (r["darg"][:, ang] * p["ang_f"][ang - cfg.n_enc][None]).sum(1)
    out = np.zeros((P, 4))
    out[:, 0], out[:, 1:1 + dim] = logit, grad
    return out


def _rejected(rows, arrays):
    bad = {r.array for r in rows if not r.ok}
    return all(a in bad for a in arrays)


@pytest.mark.parametrize("geom", gc.NETWORKS, ids=gc.name)
def test_planted_inference_errors_are_rejected(geom):
    flat, cfg = gc.network(*geom)
    ref = gc.inference_reference(*geom)
    cols = _last_tile_positions(cfg)
    checked = 0
    for P in gc.POSE_P:
        r = ref[P]
        if len(cols):
            # the features of tile 7 / 13 reach neither the hidden layer nor the skip sum nor the input gradient
            out = _planted_out(r, flat, cfg, planted_flat=_with(flat, cfg, _drop_forward(cols)))
            assert _rejected(gc.compare_inference("plant", geom, P, ref, out, out * [1, 0, 0, 0]), ("logit", "grad", "logit fwd"))
            # ... or only the input gradient loses them
            rows = gc.compare_inference("plant", geom, P, ref, _planted_out(r, flat, cfg, grad_drop=cols))
            assert _rejected(rows, ("grad",)) and not _rejected(rows, ("logit",))
            checked += 2
        if cfg.angle_dim:
            for change in (_cos_as_sin, _swap_f_b):
                out = _planted_out(r, flat, cfg, planted_flat=_with(flat, cfg, change))
                assert _rejected(gc.compare_inference("plant", geom, P, ref, out, out * [1, 0, 0, 0]), ("logit", "grad", "logit fwd")), change
                checked += 1
    has_tile = cfg.feature_dim > (200 if cfg.use_cos else 104)
    assert checked == 2 * (2 * has_tile + 2 * (cfg.angle_dim > 0))


@pytest.mark.parametrize("geom", gc.NETWORKS, ids=gc.name)
def test_planted_fit_errors_are_rejected(geom):
    flat, cfg = gc.network(*geom)
    ref = gc.fit_reference(*geom)
    o_grad, o_loss = ref["o32"]
    first = 200 if cfg.use_cos else 104
    w1 = ref["blocks"]["w1"]

    def planted(change):
        d = f64.onf_fit64(_with(flat, cfg, change), cfg, ref["x"], ref["y"])
        return fg.output_of(o_grad + (d["grad"] - ref["grad"]), o_loss + (d["loss"] - ref["loss"]), gc.FIT_P)

    for K in (16, 32):
        if cfg.feature_dim > first:
            # the W1 gradient column of position 104 / 200 is the one of position 0
            g = o_grad.copy()
            cols = g[w1].reshape(100, cfg.feature_dim)
            cols[:, first] = cols[:, 0]
            g[w1] = cols.reshape(-1)
            rows = gc.compare_fit("plant", geom, ref, fg.output_of(g, o_loss, gc.FIT_P), K)
            assert [r.array for r in rows if not r.ok] == ["w1"]
            # the features of tile 7 / 13 are not part of the network the fit differentiates
            rows = gc.compare_fit("plant", geom, ref, planted(_drop_forward(_last_tile_positions(cfg))), K)
            assert _rejected(rows, ("w1", "w3"))
        if cfg.angle_dim:
            for change in (_cos_as_sin, _swap_f_b):
                rows = gc.compare_fit("plant", geom, ref, planted(change), K)
                assert _rejected(rows, ("ang_b", "ang_f", "w1", "w3")), change


# ----------------------------------------------------------------------------------------------------------
# refusals, in front of every HIP call
P_REF = 8
N_HOST = 100 * 260 + 100 * 101 + 1024      # floats: more than any geometry's parameters


def _buffers(n_floats):
    """like tests/test_x32_geometry_cpu.py: host buffers that are never read, real ones where a device is present"""
    if torch.cuda.is_available():
        bufs = [torch.zeros(n, device="cuda") for n in n_floats]
        return bufs, [_lib.ptr(b) for b in bufs], _lib.stream_ptr()
    host = [(ctypes.c_float * n)() for n in n_floats]
    return host, [ctypes.cast(h, ctypes.c_void_p) for h in host], None


@pytest.fixture()
def lib():
    lib = nfopp.load_library()
    before = lib.nfopp_get_matrix_path()
    yield lib
    assert lib.nfopp_set_matrix_path(before) == 0


def _refused_everywhere(lib, cfg, dim, words, fit=True):
    keep, (params, pts, out, t, labels, grad, ws), stream = _buffers((N_HOST, 3 * P_REF, 4 * P_REF, P_REF, P_REF, N_HOST, 4096))
    calls = [lambda: lib.nfopp_onf_eval_points(cfg, params, pts, P_REF, out, stream),
             lambda: lib.nfopp_onf_eval_logits(cfg, params, pts, P_REF, out, stream),
             lambda: lib.nfopp_traj_collision_eval(cfg, params, pts, 1, 5, dim, t, 0, 0, 0, 0, out, None, None, stream)]
    if fit:
        calls += [lambda fp=fp: lib.nfopp_onf_train_grad_ex(cfg, params, pts, labels, P_REF, 1.0 / P_REF, grad, ws, 4096 * 4, fp, stream)
                  for fp in (1, 2)]
    for call in calls:
        rc = call()
        msg = lib.nfopp_last_error().decode()
        assert rc == -1, (rc, msg)
        assert all(w in msg for w in words), msg
    del keep


@pytest.mark.parametrize("path", gc.MATRIX_PATHS)
@pytest.mark.parametrize("geom", gc.UNSUPPORTED, ids=gc.name)
def test_an_unsupported_feature_dimension_is_refused_on_every_path(lib, geom, path):
    assert lib.nfopp_set_matrix_path(path) == 0
    e = gc.TABLE[geom]
    cfg = _lib.OnfConfigC(gc.MEAN, gc.SIGMA, e.use_cos, 1, e.angle_dim)
    assert lib.nfopp_onf_param_count(cfg) > 0
    _refused_everywhere(lib, cfg, 3, gc.refusal(e, "U") + ("%d" % e.fin,))


@pytest.mark.parametrize("path", gc.MATRIX_PATHS)
@pytest.mark.parametrize("angle_dim", (-1, 17))
@pytest.mark.parametrize("use_cos", (0, 1))
def test_an_angle_dimension_out_of_range_is_a_bad_configuration(lib, use_cos, angle_dim, path):
    assert lib.nfopp_set_matrix_path(path) == 0
    cfg = _lib.OnfConfigC(gc.MEAN, gc.SIGMA, use_cos, 1, angle_dim)
    assert lib.nfopp_onf_param_count(cfg) <= 0 and lib.nfopp_onf_train_workspace_bytes(cfg, P_REF) == 0
    _refused_everywhere(lib, cfg, 3, ("bad ONF configuration",))


@pytest.mark.parametrize("geom", [g for g, e in gc.TABLE.items() if e.inf[1] == "R32"], ids=gc.name)
def test_matrix_path_1_refuses_every_non_stock_geometry_of_its_block_counts(lib, geom):
    assert lib.nfopp_set_matrix_path(1) == 0
    e = gc.TABLE[geom]
    assert e.blocks == (e.fin + 16) // 16
    cfg = _lib.OnfConfigC(gc.MEAN, gc.SIGMA, e.use_cos, 1, e.angle_dim)
    _refused_everywhere(lib, cfg, 3 if e.angle_dim else 2, gc.refusal(e, "R32"), fit=False)
