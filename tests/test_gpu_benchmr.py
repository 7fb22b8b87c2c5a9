"""GPU parity on the settings the benchmark actually runs, and on the BASELINE configs round 1 left untested:

* the bench-mr hyper block (scripts/run_bench_mr.py:37-63: w_col 100, beta 10, w_dir 100, aw 5, lr 5e-2) with a FITTED
  sigma=10 field on the 100 m random-disc map, N = 256 and N = 512, against fixtures made by the reference itself
  (tests/golden/traj_benchmr_*.npz, g14_benchmr_batch.npz);
* BASELINE configs[1]: the drop-in `.step()` with ONF learning at N = 256 (g15);
* BASELINE configs[3]: the occupancy-grid map -- device labels equal the notebook's MapCollisionChecker (g16) and a
  4096 x 256 batch runs through `DeviceGridChecker`;
* early stop: retired trajectories leave the fused ONF kernel (ABI 4 `active_dev`).

Everything goes through the C ABI (ctypes -> libnfopp_hip.so)."""
import numpy as np
import pytest
import torch

from conftest import (BENCHMR_FIXTURES, benchmr_rollout_tol, check_benchmr_rollout, abs_percentile, check_batch_snapshot, load_golden, max_abs,
                      max_rel)

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
import nfopp  # noqa: E402
from oracle import nfopp_oracle as orc  # noqa: E402

F32 = np.float32


@pytest.mark.parametrize("name,ks", BENCHMR_FIXTURES)
def test_benchmr_settings_terms_step_rollouts_vs_golden(name, ks):
    z = load_golden(name)
    onf, cfg = gc.make_onf(z["cfg"], z["params"])
    hp = orc.Hyper.from_npz(z)
    s = gc.state_of(z, "s0_")
    eng = gc.engine_from_state(onf, s, hp)
    # G2: ONF logits at the reference's samples, every loss term, dL/dlambda
    eng.collision_eval(z["g2_t"][None])
    torch.cuda.synchronize()
    out = eng.onf_out.cpu().numpy()[0]
    assert gc.scaled_err(out[:, 0], z["g2_logit"]) < 1e-5
    eng.update()
    terms = eng.loss_terms()
    for ours, ref in (("total", "total"), ("distance", "l_dist"), ("softplus_sum", "l_col"), ("cm_tanh", "l_cm"),
                      ("boundary", "l_bnd")):
        assert max_rel(terms[ours][0], z["g2_" + ref], 1e-4) < 2e-5, ours
    assert max_rel(terms["c_squared"][0], np.sum(z["g2_c"].astype(np.float64) ** 2), 1e-6) < 2e-5
    r = np.maximum(z["g2_d"].astype(np.float64), 0)
    assert max_rel(terms["direction"][0], np.sum(r * r), 1e-6) < 2e-5        # forward-only term is active here
    lam_new = eng.lam.cpu().numpy()[0]
    assert max_abs((lam_new - s["lam"][0]) / hp.multipliers_lr, z["g2_c"]) < 2e-5
    # G3: one optimiser step
    eng = gc.engine_from_state(onf, s, hp)
    eng.optimize_trajectory(z["g3_t"][None])
    torch.cuda.synchronize()
    assert max_abs(eng.traj.cpu().numpy()[0], z["g3_traj"]) < 1e-5        # coordinates up to 100: 1 ulp = 7.6e-6
    assert max_abs(eng.lam.cpu().numpy()[0], z["g3_lam"]) < 2e-6
    assert max_abs(eng.cm.cpu().numpy()[0], z["g3_cm"]) < 1e-6
    assert gc.scaled_err(eng.adam_m.cpu().numpy()[0], z["g3_adam_m"]) < 1e-5
    assert gc.scaled_err(eng.adam_v.cpu().numpy()[0], z["g3_adam_v"]) < 2e-5
    # G6: frozen-field rollouts incl. reparametrisation
    s3 = gc.state_of(z, "g3_")
    eng = gc.engine_from_state(onf, s3, hp)
    step_count, done = s3["step_count"], 0
    for K in ks:
        while done < K:
            eng.optimize_trajectory(z["g6_t"][done][None], want_terms=False)
            if step_count % 10 == 0:
                eng.reparametrize()
            step_count += 1
            done += 1
        assert step_count == int(z["g6_k%d_step_count" % K])
        check_benchmr_rollout(name, K, eng.traj.cpu().numpy()[0], eng.lam.cpu().numpy()[0], eng.cm.cpu().numpy()[0], z)


def test_benchmr_small_batch_vs_golden():
    z = load_golden("g14_benchmr_batch.npz")
    onf, cfg = gc.make_onf(z["cfg"], z["params"])
    hp = orc.Hyper.from_npz(z)
    B, N = z["traj0"].shape[:2]
    s = dict(traj=z["traj0"].copy(), start=z["starts"], goal=z["goals"], lam=np.zeros((B, N + 1), F32),
             cm=np.zeros((B, N), F32), adam_m=np.zeros((B, N, 3), F32), adam_v=np.zeros((B, N, 3), F32), adam_step=0)
    eng = gc.engine_from_state(onf, s, hp)
    # the device initialiser reproduces the reference's straight-line start (coordinates up to 96: 1 ulp = 7.6e-6)
    ini = nfopp.init_trajectories(eng.start, eng.goal, N, False)
    assert max_abs(ini.cpu().numpy(), z["traj0"]) < 1e-5
    step_count = 1
    for k in range(int(z["steps"])):
        eng.optimize_trajectory(z["t"][:, k], want_terms=False)
        if step_count % 10 == 0:
            eng.reparametrize()
        step_count += 1
        if k + 1 in z["snapshots"]:
            check_batch_snapshot(k + 1, eng.traj.cpu().numpy(), eng.lam.cpu().numpy(), eng.cm.cpu().numpy(), z)


def _corridor_params(n):
    A = nfopp.AttributeDict
    return A(device="cuda", trajectory_length=n,
             collision_model=A(mean=0, sigma=1, use_cos=True, bias=True, use_normal_init=True, angle_encoding=True, name="ONF"),
             trajectory_initializer=A(name="TrajectoryInitializer", resolution=0.05),
             collision_optimizer=A(lr=5e-2, betas=(0.9, 0.9)), trajectory_optimizer=A(lr=1e-2, betas=(0.9, 0.9)),
             planner=A(name="ConstrainedNERFOptPlanner", trajectory_random_offset=0.02, collision_weight=1,
                       velocity_hessian_weight=0.5, random_field_points=10, init_collision_iteration=0,
                       constraint_deltas_weight=20, multipliers_lr=0.1, init_collision_points=100,
                       reparametrize_trajectory_freq=10, optimize_collision_model_freq=1, angle_weight=0.5,
                       angle_offset=0.3, boundary_weight=1, collision_multipliers_lr=1e-3))


def test_dropin_step_with_onf_learning_n256_follows_the_reference():
    """BASELINE configs[1]: 1 trajectory x 256 waypoints, corridor environment, ONF learning on, driven through the
    drop-in factory exactly like scripts/benchmark.py drives the reference (seeds torch 100 / numpy 400)."""
    z = load_golden("g15_full_steps_n256.npz")
    torch.random.manual_seed(100)
    np.random.seed(400)
    cc = nfopp.CircleDirectedCollisionChecker(0.3, (0, 3, 0, 3))
    cc.update_obstacle_points(z["obstacles"])
    cc.update_boundaries(tuple(z["bounds"]))
    planner = nfopp.PlannerFactory.make_constrained_onf_planner(cc, _corridor_params(256))
    planner.init(z["start"], z["goal"], tuple(z["bounds"]))
    assert np.array_equal(planner._collision_model.flat_parameters.cpu().numpy(), z["params0"])
    assert max_abs(planner._trajectory.detach().cpu().numpy(), z["traj0"]) < 1e-6
    K = int(z["steps"])
    for k in range(K):
        planner.step()
        checked = planner.checked_positions.as_vec()
        ref = z["k%d_checked" % k]
        assert checked.shape == ref.shape                                     # 255 course + pool + 10 field poses
        tol = 2e-6 * 4 ** k                                                    # ONF learning on: gates widen per step
        assert max_abs(checked[:255], ref[:255]) < max(tol, 1e-5)             # course samples: same numpy draws
        assert max_abs(checked[-10:], ref[-10:]) < 1e-12                      # uniform field samples
        if max_abs(checked, ref) < 1e-4:    # the retained pool is a weighted np.random.choice: same unless a draw ties
            assert np.array_equal(np.asarray(planner.truth_collision).astype(np.uint8), z["k%d_truth" % k])
        assert max_abs(planner._trajectory.detach().cpu().numpy(), z["k%d_traj" % k]) < 5e-6 * 4 ** k
        if "k%d_params" % k in z.files:
            # Adam's first steps: an entry whose gradient is ~eps moves by lr * g / (|g| + eps), so a rounding-level
            # change of g shows in that entry at the 1e-5 level (lr 5e-2) -- gate the bulk tightly, the maximum loosely
            # (measured on MI355X: p99 1.5e-8 / 2.6e-7, max 4.1e-5 / 4.9e-5 at steps 0 / 5)
            got = planner._collision_model.flat_parameters.cpu().numpy()
            assert abs_percentile(got, z["k%d_params" % k], 99) < 2e-7 * 4 ** k
            assert max_abs(got, z["k%d_params" % k]) < 2e-4
        assert max_abs(planner._constraint_multipliers.cpu().numpy(), z["k%d_lam" % k]) < 2e-5 * 4 ** k
        assert max_abs(planner._collision_multipliers.cpu().numpy(), z["k%d_cm" % k]) < 2e-5 * 4 ** k
    path = planner.get_path()
    assert path.shape == (258, 3) and path.dtype == np.float32
    assert np.array_equal(path[0], z["start"]) and np.array_equal(path[-1], z["goal"])


def test_device_grid_checker_equals_the_notebook_class():
    """Labels of the committed 100 x 100 corridor grid, bit for bit those of the reference's MapCollisionChecker
    (notebooks/onf_planner_image_map.ipynb cell 2, exec'd by make_golden.py g16) -- incl. poses on cell edges."""
    z = load_golden("g16_grid_checker.npz")
    for tag in ("unit", "fine"):
        ox, oy, cell = (float(v) for v in z[tag + "_geom"])
        chk = nfopp.DeviceGridChecker(z["grid"], ox, oy, cell)
        got = chk.labels(torch.tensor(z[tag + "_poses"], device="cuda")).cpu().numpy()
        assert np.array_equal(got.astype(np.uint8), z[tag + "_truth"]), tag
        got2 = chk.labels(torch.tensor(np.ascontiguousarray(z[tag + "_poses"][:, :2]), device="cuda")).cpu().numpy()
        assert np.array_equal(got2.astype(np.uint8), z[tag + "_truth"]), tag


def test_grid_map_full_size_batch():
    """BASELINE configs[3] per GPU: 4096 trajectories x 256 waypoints on the occupancy-grid map, frozen field.
    Size-independent properties: (i) every densified pose gets the label the oracle's (reference-pinned) grid check
    gives; (ii) the best-path bookkeeping equals the oracle's; (iii) a shard that holds trajectories 4000..4095 with
    `traj_index_offset` = 4000 reproduces those rows bit for bit (device Philox stream)."""
    z = load_golden("g16_grid_checker.npz")
    grid = z["grid"]
    g1 = load_golden("traj_benchmr_n256.npz")
    onf, cfg = gc.make_onf(g1["cfg"], g1["params"])
    hp = orc.Hyper.from_npz(g1)
    B, N = 4096, 256
    rng = np.random.default_rng(40)
    free = np.argwhere(grid[:-1, :-1] == 0)
    pick = free[rng.integers(0, len(free), 2 * B)]
    poses = np.concatenate([pick[:, ::-1] + 0.5 + rng.uniform(0, 1, (2 * B, 2)), rng.uniform(-np.pi, np.pi, (2 * B, 1))], 1).astype(F32)
    starts, goals = poses[:B], poses[B:]
    chk = nfopp.DeviceGridChecker(grid, 0.0, 0.0, 1.0)
    assert not chk.labels(torch.tensor(poses, device="cuda")).cpu().numpy().any()       # endpoints are free
    planner = nfopp.BatchPlanner(onf, B, N, gc.hyper_from(hp), device="cuda", seed=9, checker=None)
    planner.init(starts, goals, (0.0, 100.0, 0.0, 100.0))
    for _ in range(3):
        planner.step()
    collides, length = planner.evaluate(checker=chk, sub=2)
    torch.cuda.synchronize()
    tr = planner.engine.traj.cpu().numpy()
    assert np.isfinite(tr).all()
    dense, ln = orc.path_interpolate(tr, starts, goals, 2)
    assert max_abs(planner._poses.cpu().numpy(), dense) < 2e-5
    labels = planner._pose_labels.cpu().numpy().reshape(B, -1)
    dev_poses = planner._poses.cpu().numpy()
    want = orc.grid_check(dev_poses.reshape(-1, 3)[:, :2], grid, 0.0, 0.0, 1.0).reshape(B, -1)
    assert np.array_equal(labels.astype(bool), want)                                    # (i) 4096 x 515 poses
    assert np.array_equal(collides.cpu().numpy().astype(bool), want.any(1))            # (ii)
    assert max_rel(length.cpu().numpy(), ln, 1e-3) < 1e-5
    best = planner.best_length.cpu().numpy()
    assert np.array_equal(np.isfinite(best), ~want.any(1))
    assert 0 < want.any(1).sum() < B                                                    # both outcomes occur
    lo = 4000
    shard = nfopp.BatchPlanner(onf, B - lo, N, gc.hyper_from(hp), device="cuda", seed=9, traj_index_offset=lo)
    shard.init(starts[lo:], goals[lo:], (0.0, 100.0, 0.0, 100.0))
    for _ in range(3):
        shard.step()
    assert np.array_equal(shard.engine.traj.cpu().numpy(), tr[lo:])                    # (iii)


def test_retired_trajectories_leave_the_onf_kernel():
    """Early stop (scripts/run_bench_mr.py:121-126 `break`): with an `active` mask the fused ONF kernel walks the live
    trajectories only.  Live rows are bit-identical to an unmasked run, retired rows keep their state and their
    stale scratch bit for bit.  (The kernel time follows the live fraction: measured by tools/early_stop_timing.py.)"""
    z = load_golden("traj_benchmr_n256.npz")
    onf, cfg = gc.make_onf(z["cfg"], z["params"])
    hp = orc.Hyper.from_npz(z)
    B, N = 4096, 256
    s = gc.state_of(z, "s0_", reps=B)
    s["traj"] = s["traj"] + np.linspace(0, 0.5, B, dtype=F32)[:, None, None] * np.asarray([1, -1, 0.01], F32)
    rng = np.random.default_rng(8)
    mask = (rng.uniform(size=B) < 0.5).astype(np.uint8)
    mask[:3] = (0, 1, 0)
    ref = gc.engine_from_state(onf, s, hp)
    ref.seed = 77
    eng = gc.engine_from_state(onf, s, hp)
    eng.seed = 77
    eng.onf_out.fill_(-7.0)
    eng.t.fill_(-7.0)
    eng.active = torch.tensor(mask, device="cuda")
    for e in (ref, eng):
        for k in range(2):
            e.optimize_trajectory(want_terms=False)
            e.reparametrize()
    torch.cuda.synchronize()
    live = mask.astype(bool)
    for name in ("traj", "lam", "cm", "adam_m", "adam_v", "t", "onf_out"):
        a, b = getattr(eng, name).cpu().numpy(), getattr(ref, name).cpu().numpy()
        assert np.array_equal(a[live], b[live]), name
    assert np.array_equal(eng.traj.cpu().numpy()[~live], s["traj"][~live])
    assert np.array_equal(eng.lam.cpu().numpy()[~live], s["lam"][~live])
    assert (eng.onf_out.cpu().numpy()[~live] == -7.0).all() and (eng.t.cpu().numpy()[~live] == -7.0).all()
    # nobody live: nothing is touched, nothing faults
    eng.active.zero_()
    before = eng.traj.clone()
    eng.optimize_trajectory(want_terms=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.traj, before)

    # (that the kernel time follows the live fraction is a timing property: tools/early_stop_timing.py, not this suite)


@pytest.mark.parametrize("B", [1, 1024, 1025, 2049])
def test_the_live_list_across_thread_and_wave_boundaries(B):
    """The compaction behind the early stop is one workgroup of 1024 threads that scans the mask: one trajectory in all, one
    per thread, one thread with a second one, more than two per thread.  The list itself (count, then the live indices in
    rising order) and, as above, live rows bit-identical to an unmasked run and retired rows untouched."""
    z = load_golden("traj_benchmr_n256.npz")
    onf, cfg = gc.make_onf(z["cfg"], z["params"])
    hp = orc.Hyper.from_npz(z)
    s = gc.state_of(z, "s0_", reps=B)
    s["traj"] = s["traj"] + np.linspace(0, 0.5, B, dtype=F32)[:, None, None] * np.asarray([1, -1, 0.01], F32)
    mask = (np.random.default_rng(B).uniform(size=B) < 0.5).astype(np.uint8)
    mask[0], mask[-1] = 0, 1           # (B = 1: the one trajectory is live)
    ref = gc.engine_from_state(onf, s, hp)
    eng = gc.engine_from_state(onf, s, hp)
    eng.active = torch.tensor(mask, device="cuda")
    for e in (ref, eng):
        e.seed = 77
        e.optimize_trajectory(want_terms=False)
    torch.cuda.synchronize()
    live = np.flatnonzero(mask)
    got = eng._live.cpu().numpy()
    assert got[0] == len(live) and np.array_equal(got[1:1 + len(live)], live)
    for name in ("traj", "lam", "cm", "adam_m", "adam_v", "t", "onf_out"):
        assert np.array_equal(getattr(eng, name).cpu().numpy()[live], getattr(ref, name).cpu().numpy()[live]), name
    assert np.array_equal(eng.traj.cpu().numpy()[mask == 0], s["traj"][mask == 0])


def test_continuous_learning_full_size_and_two_shard_gradient():
    """BASELINE configs[4] per GPU at its real size: 4096 trajectories x 512 waypoints, forward-only constraints,
    continuous ONF learning on 4096 x 621 = 2 543 616 device-sampled poses per step (bench-mr hyper block, disc map).
    There is one GPU under test, so the multi-rank step is checked by its arithmetic: the gradient each of two ranks
    would contribute (its half of the trajectories, normalised by the GLOBAL sample count) must add up to the
    single-rank gradient -- that sum is all the RCCL all-reduce does -- and the fit must be bitwise reproducible."""
    z = load_golden("traj_benchmr_n512.npz")
    onf, cfg = gc.make_onf(z["cfg"], z["params"])
    hp = orc.Hyper.from_npz(z)
    B, N = 4096, 512
    bounds = (0.0, 100.0, 0.0, 100.0)
    rng = np.random.default_rng(45)
    starts = np.concatenate([rng.uniform(3, 97, (B, 2)), rng.uniform(-3, 3, (B, 1))], 1).astype(F32)
    goals = np.concatenate([rng.uniform(3, 97, (B, 2)), rng.uniform(-3, 3, (B, 1))], 1).astype(F32)
    checker = nfopp.DeviceCircleChecker(z["discs"], float(z["radius"]), bounds)
    planner = nfopp.BatchPlanner(onf, B, N, gc.hyper_from(hp), checker=checker, fit_lr=2e-2, angle_offset=0.3, seed=11)
    planner.init(starts, goals, bounds)
    assert planner.sampler.S == N - 1 + 100 + 10
    losses = []
    for _ in range(3):
        planner.step()
        losses.append(float(planner.fitter.last_loss))
    torch.cuda.synchronize()
    assert np.isfinite(planner.get_paths()).all() and np.isfinite(losses).all()
    assert planner.fitter.step_count == 3 and int(planner.fitter.grad[-1]) == B * planner.sampler.S
    # the two-rank arithmetic on the samples of the last fit
    samples = planner.sampler.samples.view(-1, 3)
    labels = planner.sampler.labels
    total = samples.shape[0]
    half = (B // 2) * planner.sampler.S
    fit = nfopp.OnfFitter(onf, 2e-2, (0.9, 0.9), distributed=False)
    fit._hip_grad(samples, labels, 1.0 / total)
    g_full = fit.grad.clone()
    fit._hip_grad(samples, labels, 1.0 / total)
    assert torch.equal(fit.grad, g_full)                                  # bitwise reproducible at full size
    fit._hip_grad(samples[:half].contiguous(), labels[:half].contiguous(), 1.0 / total)
    g_a = fit.grad.clone()
    fit._hip_grad(samples[half:].contiguous(), labels[half:].contiguous(), 1.0 / total)
    g_sum = (g_a + fit.grad).cpu().numpy()
    g_full = g_full.cpu().numpy()
    assert g_sum[-1] == total
    scale = float(np.abs(g_full[:-2]).max())
    assert max_abs(g_sum[:-2], g_full[:-2]) < 2e-5 * scale                # summation order only
    assert abs(g_sum[-2] - g_full[-2]) < 1e-5 * abs(g_full[-2])           # global mean loss


def test_fit_gradient_repeats_bit_for_bit():
    """The full-size ONF fit gradient (2 543 616 samples: pass 1 + the weight-gradient pass + fixed-order reductions), repeated 24
    times on the same inputs, must come out bit for bit the same.  This test found a hazard hipcc does not pad (a packed fma
    with op_sel reading a register pair an LDS load had just filled: csrc/onf_wgrad.hip) -- one process in ten
    saw single repeats differ in the 7th digit of dW1.  On failure it says which parameter blocks moved and whether pass 1's
    stored factors did."""
    z = load_golden("traj_benchmr_n512.npz")
    onf, cfg = gc.make_onf(z["cfg"], z["params"])
    P = 4096 * 621
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(P, 3, device="cuda", generator=gen) * torch.tensor([100.0, 100.0, 6.28], device="cuda")
    y = (torch.rand(P, device="cuda", generator=gen) < 0.35).float()
    fit = nfopp.OnfFitter(onf, 2e-2, (0.9, 0.9), distributed=False)
    fit._hip_grad(x, y, 1.0 / P)
    first = fit.grad.clone()
    n_factor = P * (2 * 112 + 224 + 12)              # pass 1's stored factors: h1 | dh1 | de | record
    factors = fit._ws[:n_factor].clone()
    assert torch.isfinite(first).all()
    for k in range(24):
        fit._hip_grad(x, y, 1.0 / P)
        if not torch.equal(fit.grad, first):
            d = (fit.grad - first).abs().cpu().numpy()
            idx = np.nonzero(d)[0]
            blocks = np.cumsum([0, 40, 22000, 100, 10000, 100, 320, 1, 400, 200, 2])
            names = ["angle", "W1", "b1", "W2", "b2", "W3", "b3", "We", "be", "loss/count"]
            per_block = {n: int(((idx >= a) & (idx < b)).sum()) for n, a, b in zip(names, blocks[:-1], blocks[1:])}
            same_factors = bool(torch.equal(fit._ws[:n_factor], factors))
            w1 = idx[(idx >= 40) & (idx < 22040)] - 40
            rows, cols = sorted(set((w1 // 220).tolist())), sorted(set((w1 % 220).tolist()))
            raise AssertionError("repeat %d differs in %d elements %s, max |d| %.3e; pass 1 factors identical: %s; W1 rows %s "
                                 "cols %s" % (k, len(idx), per_block, float(d.max()), same_factors, rows, cols))


def test_fused_onf_kernel_repeats_bit_for_bit():
    """K1 at the benchmark size (4096 x 256: 1 044 480 collision samples), 20 repeats on the same trajectories and the same
    injected t, in trajectory mode and in forward-only pose mode: bit for bit the same every time.  Companion of
    test_fit_gradient_repeats_bit_for_bit -- a timing-dependent hazard shows up as a repeat that differs, not as a wrong mean."""
    z = load_golden("traj_benchmr_n256.npz")
    onf, cfg = gc.make_onf(z["cfg"], z["params"])
    hp = orc.Hyper.from_npz(z)
    B, N = 4096, 256
    rng = np.random.default_rng(9)
    traj = (rng.random((B, N, 3)) * [100.0, 100.0, 6.0] - [0.0, 0.0, 3.0]).astype(F32)
    t = rng.random((B, N - 1)).astype(F32)
    zeros = np.zeros((B, 3), F32)
    s = dict(traj=traj, start=zeros, goal=zeros, lam=np.zeros((B, N + 1), F32), cm=np.zeros((B, N), F32),
             adam_m=np.zeros((B, N, 3), F32), adam_v=np.zeros((B, N, 3), F32), adam_step=0)
    eng = gc.engine_from_state(onf, s, hp)
    eng.collision_eval(t)
    first = eng.onf_out.clone()
    poses = torch.tensor(traj.reshape(-1, 3), device="cuda")
    first_logits = onf(poses).clone()
    assert torch.isfinite(first).all() and torch.isfinite(first_logits).all()
    for k in range(20):
        eng.collision_eval(t)
        assert torch.equal(eng.onf_out, first), k
        assert torch.equal(onf(poses), first_logits), k
