"""CPU-only tests: the C-ABI library loads and exports every declared symbol (no compute without a GPU), and the
host-side logic (factory, ONF container, preconditioner band, sharding, initialiser, checkers) matches the golden
vectors produced by the reference."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, max_abs

import nfopp
from nfopp import _lib


def test_library_loads_and_exports_every_header_symbol():
    lib = nfopp.load_library()
    header = open(os.path.join(ROOT, "include", "nfopp_hip.h")).read()
    declared = set(re.findall(r"\b(nfopp_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.nfopp_abi_version() == 6
    assert lib.nfopp_device_count() >= 0


def test_no_packed_fp32_op_reads_a_high_dword_into_its_low_lane():
    """The build's own post-link check (tools/check_packed_opsel.sh), run again on the library the tests load: no gfx950
    code object holds a v_pk_*_f32 ... op_sel form whose low lane takes a pair's high dword (wrong low
    lanes on MI355X right behind an LDS read of the pair; replay in tools/micro/pk_opsel_lds.hip)."""
    import subprocess
    res = subprocess.run([os.path.join(ROOT, "tools", "check_packed_opsel.sh"), _lib.LIB_PATH], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    # fails closed: a file it cannot extract a gfx950 code object from was NOT checked and must not pass
    other = subprocess.run([os.path.join(ROOT, "tools", "check_packed_opsel.sh"), os.path.abspath(__file__)], capture_output=True,
                           text=True)
    assert other.returncode == 2, other.stderr
    assert "code-object extraction failed" in other.stderr, other.stderr
    # a valid object file without a gfx950 code object (the interpreter's own binary) reaches the "nothing was checked" exit
    import sys
    host_only = subprocess.run([os.path.join(ROOT, "tools", "check_packed_opsel.sh"), os.path.realpath(sys.executable)],
                               capture_output=True, text=True)
    assert host_only.returncode == 2, host_only.stderr
    assert "nothing was checked" in host_only.stderr, host_only.stderr
    missing = subprocess.run([os.path.join(ROOT, "tools", "check_packed_opsel.sh"), _lib.LIB_PATH], capture_output=True, text=True,
                             env=dict(os.environ, OBJDUMP="/nonexistent/llvm-objdump"))
    assert missing.returncode == 2, missing.stderr
    assert "failing closed" in missing.stderr, missing.stderr
    # the pattern the script looks for does match the offending form and not the harmless direction
    import re as _re
    pat = _re.compile(r"op_sel:\[[01,]*1[01,]*\]")
    assert pat.search("v_pk_fma_f32 v[206:207], v[14:15], v[152:153], v[18:19] op_sel:[0,1,0]")
    assert not pat.search("v_pk_fma_f32 v[206:207], v[10:11], v[152:153], v[206:207] op_sel_hi:[1,0,1]")


def test_struct_layouts_match_header():
    import ctypes
    assert ctypes.sizeof(_lib.OnfConfigC) == 20
    assert ctypes.sizeof(_lib.TrajHyperC) == 4 * (8 + 4 + 6)
    # nfopp_traj_buffers: 13 pointers, int64, 5 int32 (+4 tail padding); nfopp_step_schedule: 3 doubles, 3 int64, 2 uint64, 2 int32
    assert ctypes.sizeof(_lib.TrajBuffersC) == 13 * 8 + 8 + 5 * 4 + 4
    assert ctypes.sizeof(_lib.StepScheduleC) == 3 * 8 + 3 * 8 + 2 * 8 + 2 * 4


def test_param_count_and_argument_errors_without_gpu():
    lib = nfopp.load_library()
    assert lib.nfopp_onf_param_count(_lib.OnfConfigC(0, 1, 1, 1, 10)) == 33161
    assert lib.nfopp_onf_param_count(_lib.OnfConfigC(1.5, 1, 0, 1, 0)) == 100 * 100 + 100 + 100 * 100 + 100 + 200 + 1 + 200 + 100
    assert lib.nfopp_onf_param_count(_lib.OnfConfigC(0, 0, 1, 1, 10)) < 0            # sigma = 0 rejected
    assert b"ONF" in lib.nfopp_last_error()
    # argument validation happens before any HIP call
    rc = lib.nfopp_onf_eval_points(_lib.OnfConfigC(0, 1, 1, 1, 10), None, None, 4, None, None)
    assert rc == -1 and b"null" in lib.nfopp_last_error()
    rc = lib.nfopp_reparametrize(1, 10, 4, None, None, None, None, None, None, None, None)
    assert rc == -1
    # the neighbours of the step and the matrix-path switch (ABI 3)
    assert lib.nfopp_path_postprocess(None, 1, 2, 0.001, 0.05, 0, None, None, None) == -1     # < 3 poses
    assert b"3..1026" in lib.nfopp_last_error()
    assert lib.nfopp_path_postprocess(None, 1, 2000, 0.001, 0.05, 0, None, None, None) == -1  # > 1026 poses
    assert lib.nfopp_path_postprocess(None, 1, 10, 0.001, 0.0, 0, None, None, None) == -1     # zero step
    assert lib.nfopp_path_postprocess(None, 0, 10, 0.001, 0.05, 0, None, None, None) == 0     # empty batch: no-op
    assert lib.nfopp_init_trajectories(None, None, 1, 10, 2, 1, None, None) == -1             # headings need dim 3
    assert lib.nfopp_init_trajectories(None, None, 0, 10, 3, 0, None, None) == 0
    assert lib.nfopp_set_matrix_path(3) == -1 and b"matrix path" in lib.nfopp_last_error()
    before = lib.nfopp_get_matrix_path()
    assert before in (0, 1, 2)
    assert lib.nfopp_set_matrix_path(2) == 0 and lib.nfopp_get_matrix_path() == 2     # split, 16x16x32 kernels only
    assert lib.nfopp_set_matrix_path(0) == 0 and lib.nfopp_get_matrix_path() == 0
    assert lib.nfopp_set_matrix_path(1) == 0 and lib.nfopp_get_matrix_path() == 1
    assert lib.nfopp_set_matrix_path(before) == 0
    # ABI 4: an active mask needs its live-list workspace; the occupancy-grid geometry is float64
    rc = lib.nfopp_check_collision_grid(None, 0, 2, None, 1, 1, 0.0, 0.0, 1.0, None, None)
    assert rc == -1 and b"occupancy grid" in lib.nfopp_last_error()


@pytest.mark.parametrize("value, path", [(None, 1), ("fp32", 0), ("0", 0), ("1", 1), ("split", 1), ("2", 2)])
def test_matrix_path_environment_parse(value, path):
    """NFOPP_MATRIX_PATH as a fresh process sees it (read once, on first use; the getter touches no device)."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "NFOPP_MATRIX_PATH"}
    if value is not None:
        env["NFOPP_MATRIX_PATH"] = value
    child = "import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).nfopp_get_matrix_path())"
    res = subprocess.run([sys.executable, "-c", child, _lib.LIB_PATH], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout) == path


def test_device_guard_rejects_buffers_of_another_gpu():
    """every launch uses the CURRENT device's stream / CU count / scratch, so `_lib.ptr` refuses a buffer that
    lives on another card (the check itself is plain Python and needs no GPU)."""
    _lib.require_current_device(0, 0)
    _lib.require_current_device(3, 3)
    with pytest.raises(nfopp.NfoppError, match="cuda:1 but the current device is cuda:0"):
        _lib.require_current_device(1, 0)


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(nfopp.NfoppError):
        _lib.require_gpu()
    onf = nfopp.ONF(0, 1, use_cos=True, angle_encoding=True)
    with pytest.raises(nfopp.NfoppError):
        onf(torch.zeros(4, 3))
    with pytest.raises(RuntimeError):
        nfopp.PlannerFactory.make_onf_planner(nfopp.CollisionChecker(), device="cpu")


def test_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "pytorch-motion-planner_amd", "nfopp")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert "oracle" not in src.replace("nfopp_oracle.py", ""), f


def test_onf_container_matches_reference_init_and_state_dict():
    z = load_golden("g9_full_steps.npz")
    torch.random.manual_seed(100)
    m = nfopp.ONF(0, 1, use_cos=True, use_normal_init=True, bias=True, angle_encoding=True)
    assert list(m.state_dict().keys()) == [
        "_angle_encoder._biases", "_angle_encoder._frequencies", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight",
        "mlp.2.bias", "mlp2.0.weight", "mlp2.0.bias", "encoding_layer.weight", "encoding_layer.bias"]
    assert [tuple(v.shape) for v in m.state_dict().values()] == [(20,), (20,), (100, 220), (100,), (100, 100), (100,),
                                                                 (1, 320), (1,), (200, 2), (200,)]
    assert np.array_equal(m.flat_parameters.numpy(), z["params0"])   # same seed => the reference's initial field
    # parameters are views of the flat buffer, and stay so after .to()
    m.flat_parameters[0] = 7.0
    assert float(m.state_dict()["_angle_encoder._biases"][0]) == 7.0
    m2 = m.to(torch.float32)
    m2.load_flat(np.arange(m2.n_params, dtype=np.float32))
    assert float(m2.state_dict()["encoding_layer.bias"][-1]) == m2.n_params - 1
    assert len(list(m.parameters())) == 10
    m3 = nfopp.ONF(1.5, 1)
    assert m3.point_dim == 2 and m3.n_params == 20701


def test_inverse_hessian_and_band_vs_golden():
    z = load_golden("g5_hinv.npz")
    for n, w, key in ((100, 0.5, "n100_w0p5"), (100, 3.0, "n100_w3p0"), (16, 0.5, "n16_w0p5")):
        h = nfopp.inverse_hessian(n, w)
        assert max_abs(h, z[key]) < 1e-7
        band, hw = nfopp.band_of(h)
        # the banded product equals the dense product to far below fp32 rounding
        g = np.random.default_rng(0).normal(size=(n, 3)).astype(np.float32)
        dense = h.astype(np.float64) @ g
        banded = np.zeros_like(dense)
        for k in range(2 * hw + 1):
            j = np.arange(n) + k - hw
            ok = (j >= 0) & (j < n)
            banded[ok] += band[k, ok, None].astype(np.float64) * g[j[ok]]
        assert np.abs(banded - dense).max() < 1e-7 * np.abs(dense).max()
        assert hw < n
    h = nfopp.inverse_hessian(512, 0.5)
    band, hw = nfopp.band_of(h)
    assert hw < 40                                                     # decay 0.38^k: ~22 taps reach 1e-9
    zb = z["n512_w0p5_band64"]
    assert max_abs(band[hw, :], zb[:, 64]) < 1e-7                      # diagonal
    assert max_abs(band[hw + 3, :-3], zb[:-3, 67]) < 1e-7


def test_universal_factory_semantics():
    f = nfopp.UniversalFactory([nfopp.ONF, nfopp.TrajectoryInitializer])
    onf = f.make_from_parameters(nfopp.AttributeDict(name="ONF", mean=0, sigma=10, use_cos=True, bias=True,
                                                     use_normal_init=True, not_a_ctor_arg=5))
    assert isinstance(onf, nfopp.ONF) and onf.feature_dim == 200                  # unknown kwarg silently dropped
    with pytest.raises(KeyError, match="Unknown class"):
        f.make_from_parameters(nfopp.AttributeDict(name="Nope"))
    assert f.make_from_parameters(3) == 3
    assert f.make_from_parameters(nfopp.AttributeDict(lr=1)) == {"lr": 1}
    ti = f.make_from_parameters(nfopp.AttributeDict(name="TrajectoryInitializer", resolution=0.05), collision_checker=1)
    assert ti._collision_checker == 1
    with pytest.raises(NotImplementedError):
        nfopp.AstarTrajectoryInitializer(None)
    with pytest.raises(AttributeError):
        nfopp.DEFAULT_PARAMETERS.trajectory_initializer   # the reference's defaults lack it too (planner_factory.py:71)


def test_hyper_scalars_formed_like_torch():
    hp = nfopp.TrajectoryHyper(lr=1e-2, betas=(0.9, 0.9), bounds=(0, 1, 2, 3))
    c = hp.to_c(3)
    assert c.adam_omb1 == np.float32(1 - 0.9) and c.adam_omb1 != np.float32(1) - np.float32(0.9)
    assert c.adam_step_size == np.float32(1e-2 / (1 - 0.9 ** 3))
    assert c.adam_bc2_sqrt == np.float32((1 - 0.9 ** 3) ** 0.5)
    assert list(c.bounds) == [0, 1, 2, 3]


def _c_fields(block):
    """Every field of a TrajHyperC as plain Python values (the bounds array as a list)."""
    return {name: (list(getattr(block, name)) if name == "bounds" else getattr(block, name)) for name, _ in block._fields_}


def test_hyper_is_an_immutable_value():
    h = nfopp.TrajectoryHyper(collision_weight=3, betas=[0.9, 0.8], bounds=[0, 1, 2, 3])
    assert len(h.FIELDS) == 12 and h.betas == (0.9, 0.8) and h.bounds == (0, 1, 2, 3)
    for name in h.FIELDS:
        with pytest.raises(AttributeError, match=r"replace\(\)"):
            setattr(h, name, getattr(h, name))
    with pytest.raises(AttributeError):
        h.no_such_field = 1
    with pytest.raises(AttributeError):
        del h.lr
    with pytest.raises(TypeError):
        h.replace(no_such_field=1)
    # equal exactly when every field is equal
    assert h == nfopp.TrajectoryHyper(collision_weight=3, betas=(0.9, 0.8), bounds=(0, 1, 2, 3)) and not (h != h.replace())
    assert hash(h) == hash(h.replace())
    fresh = dict(collision_weight=4, angle_weight=1, constraint_deltas_weight=2, multipliers_lr=3, collision_multipliers_lr=5,
                 boundary_weight=6, collision_beta=7, direction_delta_weight=8, lr=9, betas=(0.5, 0.8), eps=1e-3,
                 bounds=(0, 1, 2, 4))
    assert set(fresh) == set(h.FIELDS)
    for name, value in fresh.items():
        other = h.replace(**{name: value})
        assert other != h and not (other == h), name
        assert getattr(other, name) == value and getattr(h, name) != value
    assert h != "hyper" and h != None  # noqa: E711


def test_hyper_replace_leaves_the_original_and_its_block_alone():
    h = nfopp.TrajectoryHyper(collision_weight=3, angle_weight=0.25, lr=2e-2, betas=(0.9, 0.8), eps=1e-6, bounds=(0, 1, 2, 3))
    c = h.to_c(5)
    assert h.to_c(5) is c and h.to_c(6) is c              # one block per object, refreshed in place
    before = _c_fields(h.to_c(5))
    g = h.replace(bounds=(1, 2, 3, 4))
    cg = g.to_c(5)
    assert cg is not c and g.to_c(5) is cg
    assert h.bounds == (0, 1, 2, 3) and _c_fields(h.to_c(5)) == before
    after = _c_fields(cg)
    assert after["bounds"] == [1, 2, 3, 4] and before["bounds"] == [0, 1, 2, 3]
    assert {k: v for k, v in after.items() if k != "bounds"} == {k: v for k, v in before.items() if k != "bounds"}
    # betas drive three step-invariant fields and both step scalars: all follow together, none on the original
    b = h.replace(betas=(0.5, 0.75))
    cb = _c_fields(b.to_c(5))
    assert cb["adam_beta2"] == np.float32(0.75) and cb["adam_omb1"] == np.float32(1 - 0.5) and cb["adam_omb2"] == np.float32(1 - 0.75)
    assert cb["adam_step_size"] == np.float32(2e-2 / (1 - 0.5 ** 5)) and cb["adam_bc2_sqrt"] == np.float32((1 - 0.75 ** 5) ** 0.5)
    assert _c_fields(h.to_c(5)) == before
    changed = {k for k in cb if cb[k] != before[k]}
    assert changed == {"adam_beta2", "adam_omb1", "adam_omb2", "adam_step_size", "adam_bc2_sqrt"}


def test_shard_range_partitions_the_batch():
    for total, world in ((32768, 8), (10, 4), (3, 8), (4096, 1)):
        spans = [nfopp.shard_range(total, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [hi - lo for lo, hi in spans]
        assert max(sizes) - min(sizes) <= 1


def test_initializer_and_checkers_vs_golden():
    z = load_golden("g11_init_checkers.npz")
    cases = z["init_cases"]
    got = nfopp.straight_line_init(cases[:, :3], cases[:, 3:], 50)
    assert max_abs(got, z["init_traj"]) < 1e-6
    ti = nfopp.TrajectoryInitializer(None)
    for c, ref in zip(cases, z["init_traj"]):
        tr = torch.zeros(50, 3)
        ti.initialize_trajectory(tr, torch.tensor(c[None, :3]), torch.tensor(c[None, 3:]))
        assert max_abs(tr.numpy(), ref) < 1e-6
    poses = nfopp.Position2.from_vec(z["poses"])
    rc = nfopp.RectangleCollisionChecker((-0.3, 0.2, -0.3, 0.2), (0, 3, 0, 3))
    rc.update_obstacle_points(z["car_obstacles"])
    assert np.array_equal(rc.check_collision(poses).astype(np.uint8), z["rect_truth"])
    cd = nfopp.CircleDirectedCollisionChecker(0.3, (0, 3, 0, 3))
    cd.update_obstacle_points(z["corridor_obstacles"])
    assert np.array_equal(cd.check_collision(poses).astype(np.uint8), z["circle_truth"])
    assert nfopp.CollisionChecker().check_collision(z["poses"]) is False
    inv = poses.inv()
    assert np.allclose(inv.rotation, -z["poses"][:, 2])


def test_device_trig_and_philox_restatements():
    """fp32 emulation of csrc/common.h sin_quadrant against float64: the polynomial sine of the per-sample fit kernels
    (csrc/onf_train.hip).  The MFMA paths evaluate their features with the hardware chain sin_halfturns_hw (a two-constant
    2 pi reduction, one fma into revolutions, v_sin_f32), which tests/test_gpu_feature_probe.py holds to float64 on the device;
    both emulations live in tests/feature_probe_gate.py."""
    from feature_probe_gate import sin_quadrant
    F = np.float32

    x = np.random.default_rng(0).uniform(-400, 400, 200000).astype(F)
    for q, fn in ((0, np.sin), (1, np.cos), (2, lambda v: -np.sin(v)), (3, lambda v: -np.cos(v))):
        assert np.abs(sin_quadrant(x, q) - fn(x.astype(np.float64))).max() < 1.2e-7
    import gpu_common as gc
    u = gc.philox_uniform_np(100, np.arange(100000), 7)
    assert 0 <= u.min() and u.max() < 1 and abs(u.mean() - 0.5) < 5e-3 and abs(u.var() - 1 / 12) < 2e-3
    assert not np.array_equal(u, gc.philox_uniform_np(101, np.arange(100000), 7))


def test_traj_steps_validates_its_arguments_without_a_gpu():
    """nfopp_traj_steps (ABI 6): the argument checks run before any launch, so they can be exercised here -- and a call for zero
    steps is a no-op that needs no device."""
    import ctypes
    lib = _lib.load()
    cfg = _lib.OnfConfigC(0.0, 1.0, 1, 1, 10)
    hp = _lib.TrajHyperC()
    buf = _lib.TrajBuffersC()
    buf.batch, buf.n_waypoints, buf.dim = 1, 8, 3
    buf.u_dev = 4096                       # never dereferenced: n_steps = 0 / the checks fail first
    sched = _lib.StepScheduleC(0.01, 0.9, 0.9, 0, 0, 0, 1, 0, 10, 1)
    params = ctypes.c_void_p(4096)
    assert lib.nfopp_traj_steps(cfg, params, hp, buf, sched, 0, None, None, None) == 0
    sched.reparam_freq = 0
    assert lib.nfopp_traj_steps(cfg, params, hp, buf, sched, 0, None, None, None) == -1
    assert b"reparam_freq" in lib.nfopp_last_error()
    sched.reparam_freq, sched.t_mode = 10, 0
    assert lib.nfopp_traj_steps(cfg, params, hp, buf, sched, 3, None, None, None) == -1      # injected draws without a buffer
    assert b"t_steps_dev" in lib.nfopp_last_error()
    sched.t_mode = 2
    assert lib.nfopp_traj_steps(cfg, params, hp, buf, sched, 0, None, None, None) == -1
    assert lib.nfopp_traj_steps(None, params, hp, buf, sched, 0, None, None, None) == -1


def test_kernels_carry_no_build_switches():
    """The library is built one way only: no HIP source or header tests a macro other than the device-compile pass.
    (A development switch left in the product could ship wrong results from one stray -D flag.)"""
    import glob
    allowed = {"__HIP_DEVICE_COMPILE__"}
    csrc = os.path.join(ROOT, "pytorch-motion-planner_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert files
    tested = {}
    for path in files:
        src = open(path).read().replace("\\\n", " ")
        for m in re.finditer(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b([^\n]*)", src, re.M):
            cond = re.sub(r"/\*.*|//.*", "", m.group(1))
            for name in set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}:
                tested.setdefault(name, os.path.basename(path))
    extra = {n: f for n, f in tested.items() if n not in allowed}
    assert not extra, extra
