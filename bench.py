#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X-native NFOPP inner loop.

Metric (BASELINE.json): waypoint-evals/sec = trajectories x waypoints x planner steps / wall seconds, plus final-loss
parity.  Workloads (per GPU; trajectories shard contiguously over ranks, weak scaling):

  cfg3 (default, the configuration the metric is quoted on; = BASELINE configs[2], and configs[3]'s per-GPU share with
        the disc map): 4096 trajectories x 256 waypoints, random-obstacle map (300 discs r = 1.5 on 100 m x 100 m), SE(2)
        constrained planner with the bench-mr hyper-parameters (reference scripts/run_bench_mr.py:37-63), ONF F = 220
        pre-fitted on the map and then FROZEN.
  cfg4 (BASELINE configs[3] per GPU): the same on the committed 100 x 100 occupancy-grid map
        (tests/golden/g16_grid_checker.npz; ground truth = DeviceGridChecker, pinned to the reference notebook's class).
  cfg5 (BASELINE configs[4] per GPU): 4096 x 512, forward-only constraints, continuous ONF learning every step
        (device sampling + checker + MFMA fit + one all-reduce of the ONF gradient buffer).

One "step" is one planner `.step()` for every trajectory: fused collision sampling + ONF fwd/bwd (MFMA kernel), loss
terms + H^-1 + Adam + multiplier ascent (stencil kernel), and the arc-length reparametrisation every 10th step.  Inputs
are resident in HBM before the timed region; the interpolation draws come from the in-kernel Philox stream.

    python bench.py --gpus 1 --steps 200 --warmup 20
    python bench.py --gpus 1 --steps 200 --warmup 20 --full  # + CPU baselines and the gated parity block
    python bench.py --gpus 1 --steps 200 --warmup 20 --dump-outputs DIR   # + DIR/<name>.npy of the last timed step
    python bench.py --gpus N --steps K --warmup W          # no WORLD_SIZE in the env: starts its own N rank processes
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W              # launched from outside: runs as one rank, as before

A plain run sets up (ONF fit, spin-up), warms up, times the K steps and prints the line: the contract's fields, `config`
and `roofline` (both from the timed steps themselves).  `--full` adds the legs that take runs of their own after the
timed steps: `cpu_baseline`, `cpu_baseline_reference_faithful`, `cpu_host` and the gated `parity` block (N = 1 only,
`--cpu-sample 0` skips them).  `--dump-outputs DIR` writes what the last timed step left to a caller, float32:
`paths` [B, N+2, 3] (endpoints included), `lam` [B, N+1], `cm` [B, N] and, for cfg5, `onf_params` (the learnt field);
rows of all ranks in global trajectory order, a fixed seeded row sample above 64 MB.  The inputs depend on the
arguments only (fixed seeds), so two builds can be compared output for output.

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE is a LAUNCHER: that process never makes a GPU call (it asserts
so), starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free>
bench.py <same arguments>` as a child process group, relays rank 0's single JSON line to stdout and exits with the
children's return code.  The line carries `backend` and `ranks_seen` = an all-reduce of ones over the process group the
data path uses (== n_gpus, or the run did not span the ranks it claims).

Rank 0 prints ONE JSON line.  Beside the contract's fields:
  roofline      fused ONF kernel: algorithmic fp32 FLOPs (131 400 per collision sample) over its HIP-event
                duration, against the pipe it runs on (see `roofline()`).
  cpu_baseline  (--full) the STRONG CPU baseline (batched autograd-free torch restatement, all host cores) on a bounded sample;
                `cpu_baseline_reference_faithful` = the eager-autograd single-trajectory restatement per core
                (oracle/cpu_baselines.py, both validated against the reference's fixtures in tests/test_cpu_baselines.py;
                timed in a child process that never touches the GPU).
  parity        (--full) `ok` is a GATE: the run exits with code 4 when it is false (thresholds from the reference's own
                conditioning, `parity_gate`).  "final loss parity": (short) the first trajectories of THIS workload stepped by the GPU and by the numpy
                oracle (pinned to the reference) on the identical Philox draw stream from the same initial state --
                waypoint and per-term loss differences; (final) total loss and collision-free rate after all W + K
                steps, GPU vs the CPU restatement on the same sample, and the GPU's collision-free rate over the batch.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "pytorch-motion-planner_amd"))
sys.path.insert(0, ROOT)

import nfopp  # noqa: E402

FLOP_PER_SAMPLE = 131400.0      # 65 700 FMA per collision sample (fwd 32 740 + input-bwd 32 960)
PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak
SPLIT_PRODUCTS = 6              # bf16x3 split path: partial products issued per fp32 multiply (csrc/onf_split.hip)
B_PER_GPU = 4096
BOUNDS = (0.0, 100.0, 0.0, 100.0)
SEED = 100
HYPER = dict(collision_weight=100, angle_weight=5, constraint_deltas_weight=100, multipliers_lr=0.1,
             collision_multipliers_lr=1e-3, boundary_weight=1, collision_beta=10, direction_delta_weight=100,
             lr=5e-2, beta1=0.9, beta2=0.9, eps=1e-8)   # reference scripts/run_bench_mr.py:37-63


class DiscMap(object):
    """300 discs r = 1.5 on 100 m x 100 m (bench-mr "random grid, obstacle ratio 0.03")."""
    name = "random-obstacle map (300 discs r=1.5 on 100x100)"

    def __init__(self):
        self.discs, self.radius = np.random.default_rng(1234).uniform(5, 95, (300, 2)), 1.5

    def in_collision(self, xy, margin=0.0):
        d2 = ((xy[:, None, :] - self.discs[None]) ** 2).sum(-1)
        out = (d2 < (self.radius + margin) ** 2).any(1)
        return out | (xy[:, 0] < BOUNDS[0]) | (xy[:, 0] > BOUNDS[1]) | (xy[:, 1] < BOUNDS[2]) | (xy[:, 1] > BOUNDS[3])

    def free_poses(self, rng, n):
        out = np.zeros((0, 3))
        while len(out) < n:
            c = np.concatenate([rng.uniform(2, 98, (2 * n, 2)), rng.uniform(-np.pi, np.pi, (2 * n, 1))], 1)
            out = np.concatenate([out, c[~self.in_collision(c[:, :2], 0.5)]])
        return out[:n].astype(np.float32)

    def device_checker(self, device):
        return nfopp.DeviceCircleChecker(self.discs, self.radius, BOUNDS, device=device)


class GridMap(object):
    """The committed 100 x 100 occupancy grid (corridors of radius 3; bench-mr's own generator is absent)."""
    name = "occupancy-grid map (100x100 cells of 1 m, random-walk corridors, tests/golden/g16_grid_checker.npz)"

    def __init__(self):
        self.grid = np.load(os.path.join(ROOT, "tests", "golden", "g16_grid_checker.npz"), allow_pickle=False)["grid"]

    def in_collision(self, xy, margin=0.0):
        # MapCollisionChecker arithmetic (notebooks/onf_planner_image_map.ipynb cell 2), origin (0, 0), cell 1 m
        ix, iy = ((xy[:, 0] - 0.5) / 1.0).astype(np.int32), ((xy[:, 1] - 0.5) / 1.0).astype(np.int32)
        ok = (ix >= 0) & (iy >= 0) & (iy < self.grid.shape[0] - 1) & (ix < self.grid.shape[1] - 1)
        out = np.ones(len(xy), bool)
        out[ok] = self.grid[iy[ok], ix[ok]] > 0
        return out

    def free_poses(self, rng, n):
        # cells whose 3 x 3 neighbourhood is free, so that endpoints keep a clearance
        g = self.grid == 0
        core = g.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                core &= np.roll(np.roll(g, dy, 0), dx, 1)
        core[[0, -1]] = False
        core[:, [0, -1]] = False
        cells = np.argwhere(core)
        pick = cells[rng.integers(0, len(cells), n)]
        xy = pick[:, ::-1] + 0.5 + rng.uniform(0.05, 0.95, (n, 2))
        return np.concatenate([xy, rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)

    def device_checker(self, device):
        return nfopp.DeviceGridChecker(self.grid, 0.0, 0.0, 1.0, device=device)


def make_onf(device, env, fit_iters, fit_points):
    """ONF of scripts/run_bench_mr.py:28-36 (sigma=10), fitted to the map with the HIP training kernel, then frozen."""
    torch.random.manual_seed(100)
    onf = nfopp.ONF(0, 10, use_cos=True, use_normal_init=True, bias=True, angle_encoding=True).to(device)
    fitter = nfopp.OnfFitter(onf, lr=2e-2, betas=(0.9, 0.9), distributed=False)   # every rank fits the same field
    rng = np.random.default_rng(77)
    for _ in range(fit_iters):
        x = np.concatenate([rng.uniform(0, 100, (fit_points, 2)), rng.uniform(0, 2 * np.pi, (fit_points, 1))], 1)
        y = env.in_collision(x[:, :2]).astype(np.float32)
        fitter.step(torch.tensor(x.astype(np.float32), device=device), torch.tensor(y, device=device), global_count=fit_points)
    return onf, float(fitter.last_loss) if fit_iters else float("nan")


def bench_hyper():
    h = dict(HYPER)
    return nfopp.TrajectoryHyper(betas=(h.pop("beta1"), h.pop("beta2")), bounds=BOUNDS, **h)


# ---- CPU legs (the only places that touch oracle/) ----------------------------------------------------------------------
def oracle_rollout(onf_flat, starts, goals, n, steps, index_offset=0):
    """numpy oracle (pinned to the reference) on the DEVICE's draw stream: t[b, j] of step k = Philox(seed, counter =
    global sample index (index_offset + b) * (N - 1) + j, k) -- csrc/onf_layout.h load_point.  Returns the final
    state and the per-term loss sums of the first and the last step."""
    from oracle import nfopp_oracle as orc
    cfg = orc.OnfConfig(0, 10, True, True, True)
    hp = orc.Hyper(bounds=BOUNDS, **HYPER)
    b = len(starts)
    s = dict(traj=nfopp.straight_line_init(starts, goals, n), start=starts, goal=goals,
             lam=np.zeros((b, n + 1), np.float32), cm=np.zeros((b, n), np.float32),
             adam_m=np.zeros((b, n, 3), np.float32), adam_v=np.zeros((b, n, 3), np.float32), adam_step=0, step_count=0)
    hinv = orc.calculate_inv_hessian(n, 0.5)
    idx = (index_offset + np.arange(b)[:, None]) * (n - 1) + np.arange(n - 1)[None]
    terms = []
    t0 = time.perf_counter()
    for k in range(steps):
        t = orc.philox_uniform(SEED, idx.reshape(-1), k).reshape(b, n - 1)
        terms.append(orc.planner_step(s, t, onf_flat, cfg, hp, hinv))
    return s, terms, time.perf_counter() - t0


TERM_PAIRS = (("total", "total"), ("distance", "l_dist"), ("softplus_sum", "l_col"), ("lambda_dot_c", "l_lin"),
              ("c_squared", "l_c2"), ("boundary", "l_bnd"), ("cm_tanh", "l_cm"), ("direction", "l_dir"))


def short_parity(onf, starts, goals, n, sample, steps, device):
    """GPU vs oracle from the same straight-line state on the same draws, `sample` trajectories, `steps` steps."""
    gp = nfopp.BatchPlanner(onf, sample, n, bench_hyper(), velocity_hessian_weight=0.5, device=device, seed=SEED)
    gp.init(starts[:sample], goals[:sample], BOUNDS)
    gterms = []
    for _ in range(steps):
        gp.step(want_terms=True)
        gterms.append(gp.engine.loss_terms())
    got = gp.get_paths()[:, 1:-1]
    s, oterms, cpu_s = oracle_rollout(onf.flat_parameters.cpu().numpy(), starts[:sample], goals[:sample], n, steps)
    diff = np.abs(got.astype(np.float64) - s["traj"])
    out = {"steps": steps, "trajectories": sample, "max_abs_traj": float(diff.max()),
           "p99_abs_traj": float(np.percentile(diff, 99)), "median_abs_traj": float(np.median(diff)),
           "oracle_seconds": cpu_s}
    for tag, k in (("first_step", 0), ("last_step", steps - 1)):
        rel = {}
        for ours, theirs in TERM_PAIRS:
            a, b = float(np.sum(gterms[k][ours], dtype=np.float64)), float(np.sum(oterms[k][theirs], dtype=np.float64))
            rel[ours] = abs(a - b) / max(abs(b), 1e-6)
        out["loss_term_rel_diff_" + tag] = rel
    out["gate"] = parity_gate(diff, out["loss_term_rel_diff_first_step"], steps)
    return out


def parity_gate(diff, first_step_rel, steps):
    """The short parity leg as a GATE (exit code, not a note).  From a straight-line start single waypoint entries are
    ill-conditioned under Adam (zero-up-to-rounding gradient entries become +-lr moves), so the waypoint thresholds are
    the REFERENCE's own spread when it is restarted one fp32 ulp away from itself on these settings
    (tools/ref_conditioning.py -> tests/golden/g17_conditioning.npz, B = 4 straight-line problems, 12 steps:
    `batch_k12_pct` = 90th percentile, `batch_k12_max` = maximum; columns xy, theta): median <= 1e-4, 99th percentile
    <= 4 x batch_k12_pct, 99.99th percentile <= 1.5 x batch_k12_max and maximum <= 3 x batch_k12_max, xy and theta
    separately (g17's maximum is over 12 k entries, this leg's over 131 k: the 1.5 x level is held for all but 1e-4 of
    the entries and the outright maximum gets the headroom of the 11 x larger sample -- measured 0.245 vs g17's 0.168 on
    xy); and the per-term loss sums of the FIRST step (no conditioning involved: same state, same draws) within 1e-5
    relative.  A wrong gradient, tap or weight image moves the median / p99 by orders of magnitude, not the tail."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "g17_conditioning.npz"), allow_pickle=False)
    pct, mx = z["batch_k12_pct"], z["batch_k12_max"]
    checks = {}
    worst_term = max(first_step_rel.values())
    checks["first_step_terms_rel"] = {"value": worst_term, "limit": 1e-5, "ok": bool(worst_term <= 1e-5)}
    if steps <= 12:   # the conditioning file measures 12 steps; a longer leg has no reference spread to be held against
        for name, d, col in (("xy", diff[..., :2], 0), ("theta", diff[..., 2], 1)):
            med, p99, top = float(np.median(d)), float(np.percentile(d, 99)), float(d.max())
            p9999 = float(np.percentile(d, 99.99))
            lim = {"median": 1e-4, "p99": 4.0 * float(pct[col]), "p99.99": 1.5 * float(mx[col]), "max": 3.0 * float(mx[col])}
            checks[name] = {"median": med, "p99": p99, "p99.99": p9999, "max": top, "limits": lim,
                            "ok": bool(med <= lim["median"] and p99 <= lim["p99"] and p9999 <= lim["p99.99"]
                                       and top <= lim["max"])}
    return {"ok": all(c["ok"] for c in checks.values()), "checks": checks,
            "thresholds_from": "tests/golden/g17_conditioning.npz (batch_k12_pct, batch_k12_max): the reference restarted "
                               "1 ulp away from itself, straight-line starts, bench-mr settings"}


def final_parity(planner, checker, onf, starts, goals, n, total_steps, sample):
    """After all steps: mean total loss and collision-free rate, GPU (whole batch and the first `sample` rows) vs the CPU
    restatement stepped the same number of times on the same draws (statistics, not waypoints: chaotic horizon)."""
    from oracle import cpu_baselines as cb
    eng = planner.engine
    eng.collision_eval()
    eng.update(True)                       # one more step, with the per-trajectory loss terms
    torch.cuda.synchronize()
    gpu_total = eng.loss_terms()["total"].astype(np.float64)
    collides, _ = planner.evaluate(checker=checker, sub=4)
    free = 1.0 - collides.cpu().numpy().astype(np.float64)
    field = cb.Field(onf.flat_parameters.cpu().numpy(), 0, 10)
    sc = cb.Scalars(bounds=BOUNDS, **HYPER)
    cpu = cb.BatchedTorchPlanner(field, sc, nfopp.straight_line_init(starts[:sample], goals[:sample], n), starts[:sample],
                                 goals[:sample])
    from oracle import nfopp_oracle as orc
    idx = (np.arange(sample)[:, None]) * (n - 1) + np.arange(n - 1)[None]
    torch.set_num_threads(max(1, min(16, cb.usable_cores())))
    for k in range(total_steps):
        cpu.step(orc.philox_uniform(SEED, idx.reshape(-1), k).reshape(sample, n - 1))
    cpu.optimize_trajectory(orc.philox_uniform(SEED, idx.reshape(-1), total_steps).reshape(sample, n - 1))
    cpu_total = cpu.terms["total"].numpy().astype(np.float64)
    dense, _ = orc.path_interpolate(cpu.traj.numpy(), starts[:sample], goals[:sample], 4)
    cpu_lab = checker.labels(torch.tensor(dense.reshape(-1, 3), device=eng.device)).cpu().numpy().reshape(sample, -1)
    gm, cm_ = float(gpu_total[:sample].mean()), float(cpu_total.mean())
    return {"steps": total_steps + 1, "sample": sample,
            "final_total_loss": {"gpu_batch_mean": float(gpu_total.mean()), "gpu_sample_mean": gm, "cpu_sample_mean": cm_,
                                 "rel_diff": abs(gm - cm_) / max(abs(cm_), 1e-6)},
            "collision_free_rate": {"gpu_batch": float(free.mean()), "gpu_sample": float(free[:sample].mean()),
                                    "cpu_sample": float(1.0 - (cpu_lab != 0).any(1).mean())}}


def cpu_baselines(onf_flat, starts, goals, n, sample_b, seconds):
    """oracle/cpu_baselines.py in a child process (fresh interpreter, no GPU): strong batched torch-CPU baseline and the
    reference-faithful eager baseline, on a bounded sample of this workload."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "in.npz")
        kw = {"sc_" + k: np.asarray(v, np.float64) for k, v in dict(HYPER, bounds=BOUNDS).items()}
        np.savez(path, onf_flat=onf_flat, onf_cfg=np.asarray([0, 10, 1, 1, 1], np.float64), n_waypoints=n,
                 starts=starts[:sample_b], goals=goals[:sample_b], **kw)
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
        res = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "cpu_baselines.py"), "--input", path,
                              "--seconds-batched", str(seconds), "--seconds-eager", str(0.6 * seconds), "--procs", "1"],
                             capture_output=True, text=True, env=env, timeout=600)
    if res.returncode != 0:
        raise RuntimeError("cpu_baselines.py failed:\n" + res.stderr[-2000:])
    return json.loads(res.stdout.strip().splitlines()[-1])


def pmc_traffic(workload, batch, n):
    """HBM bytes per launch of the fused kernel from the newest committed PMC passes (profiles/r*_traffic.json, collected
    with tools/gpu_pmc_split.sh on the cfg3 workload in separate --pmc passes); None for other workloads."""
    if (workload, batch, n) != ("cfg3", B_PER_GPU, 256):
        return None, None
    for name in ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                return float(json.load(f)["bytes_per_launch"]), "profiles/" + name
        except Exception:
            continue
    return None, None


def roofline(matrix_path, achieved, k1_ms, samples, traffic, traffic_source):
    """`achieved` is ALGORITHMIC fp32 FLOP/s of the fused ONF kernel in both cases.  fp32 path: against the fp32 MFMA
    peak.  Split path: the kernel runs on the bf16 matrix pipe and issues 6 bf16 partial products per fp32 multiply,
    so the peak that bounds it is the dense bf16 peak / 6 (fp32-equivalent); the fp32-MFMA ratio is given beside it."""
    out = {"bound": "mfma", "achieved": achieved, "unit": "TFLOP/s", "traffic": traffic, "traffic_source": traffic_source,
           "kernel_ms": k1_ms, "algorithmic_flop_per_launch": samples * FLOP_PER_SAMPLE}
    if matrix_path in ("split", "split16"):
        peak = PEAK_BF16_MFMA_TFLOPS / SPLIT_PRODUCTS
        x32 = matrix_path == "split"
        out.update({"peak": peak, "frac": achieved / peak, "kernel": "onf_x32_kernel<14,0,512,1>" if x32 else "onf_split_kernel<14,2,0>",
                    "pipe": "bf16 MFMA %s, %d partial products per fp32 multiply (exact 3-level operand split)"
                            % ("32x32x16" if x32 else "16x16x32", SPLIT_PRODUCTS),
                    "pipe_peak": PEAK_BF16_MFMA_TFLOPS, "executed_tflops": achieved * SPLIT_PRODUCTS,
                    "vs_fp32_mfma_peak": achieved / PEAK_FP32_MFMA_TFLOPS})
        if x32:   # not measured in this run: a replayed observation, like `traffic`, with its source named
            out["clock_note"] = ("power-limited: `peak` assumes 2.4 GHz; under this kernel the engine clock is 1.9-2.05 GHz "
                                 "(2.41 GHz on all-zero weights at the same cycle count), profiles/r03_clock_under_load.txt")
    else:
        out.update({"peak": PEAK_FP32_MFMA_TFLOPS, "frac": achieved / PEAK_FP32_MFMA_TFLOPS,
                    "kernel": "onf_fwd_bwd_kernel<14,2,0>"})
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher around it: start N fresh rank processes (one per GPU) through
    torch.distributed.run and relay rank 0's JSON line.  This process must not have touched the GPU: a forked / spawned
    rank inherits nothing from it, and the box forbids replacing a process that initialised HIP."""
    if torch.cuda.is_initialized():
        raise SystemExit("bench.py launcher: the parent process has initialised the GPU; refusing to start ranks")
    port = os.environ.get("NFOPP_MASTER_PORT") or str(_free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL's intra-node transport needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, start_new_session=True)
    line = None
    try:
        for out in proc.stdout:
            if out.startswith("{") and '"metric"' in out:
                line = out.strip()           # rank 0's result line (the last one wins; there is exactly one)
            else:
                sys.stderr.write(out)        # anything else a rank printed to stdout is diagnostics
        rc = proc.wait()
    except BaseException:
        try:
            os.killpg(proc.pid, 15)          # the exact process group started above
        except OSError:
            pass
        raise
    if line is not None:
        print(line, flush=True)
    if rc == 0 and line is None:
        rc = 3                               # ranks exited cleanly but nobody printed the line
    if torch.cuda.is_initialized():
        raise SystemExit("bench.py launcher: the parent process initialised the GPU while waiting")
    sys.exit(rc)


def dry_run_rank(args, world, rank):
    """`--dry-run-ranks`: the rank flow without the workload (no GPU call): rendezvous, one all-reduce of ones on the
    gloo backend, rank 0 prints a line with n_gpus / ranks_seen.  tests/test_bench_launcher.py runs it on CPU."""
    if world > 1:
        torch.distributed.init_process_group("gloo")
    seen = ranks_seen(world, "gloo", torch.device("cpu"))
    if rank == 0:
        print(json.dumps({"metric": "waypoint-evals/sec", "value": None, "n_gpus": world, "ranks_seen": seen,
                          "backend": "gloo", "dry_run": True, "gpu_initialised": bool(torch.cuda.is_initialized())}), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def ranks_seen(world, backend, device):
    """All-reduce of ones over the process group the data path uses: what the collective saw, not what was asked for."""
    if world == 1:
        return 1
    one = torch.ones(1, dtype=torch.float32, device=device if backend == "nccl" else "cpu")
    torch.distributed.all_reduce(one)
    return int(round(float(one.item())))


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, planner, learn, world, rank):
    """`--dump-outputs DIR`: the state the last timed step left, as a caller of the planner reads it (see the module
    docstring).  Every rank takes part in the gather; rank 0 writes.  Above DUMP_LIMIT_BYTES the per-trajectory arrays
    keep a fixed, seeded sample of rows (sorted), the same rows in every file."""
    eng = planner.engine
    rows = {"paths": planner.get_paths(), "lam": eng.lam.cpu().numpy(), "cm": eng.cm.cpu().numpy()}
    if world > 1:
        parts = [None] * world
        torch.distributed.all_gather_object(parts, rows)
        rows = {k: np.concatenate([p[k] for p in parts]) for k in rows}
    if rank != 0:
        return
    out = {"onf_params": planner.onf.flat_parameters.detach().cpu().numpy()} if learn else {}
    n = len(rows["paths"])
    per_row = sum(a[0].nbytes for a in rows.values())
    keep = min(n, (DUMP_LIMIT_BYTES - sum(a.nbytes for a in out.values())) // per_row)
    if keep < n:
        pick = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        rows = {k: a[pick] for k, a in rows.items()}
        sys.stderr.write("bench.py: --dump-outputs keeps %d of %d trajectories (64 MB limit)\n" % (keep, n))
    out.update(rows)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch-per-gpu", type=int, default=B_PER_GPU)
    ap.add_argument("--fit-iters", type=int, default=300)
    ap.add_argument("--cpu-sample", type=int, default=256,
                    help="--full: trajectories in the CPU-baseline sample (0 = skip the CPU legs)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="--full: time budget of each CPU baseline")
    ap.add_argument("--parity-steps", type=int, default=10)
    ap.add_argument("--workload", choices=("cfg3", "cfg4", "cfg5"), default="cfg3")
    ap.add_argument("--spin-up", type=int, default=300, help="throw-away steps during setup (clock ramp), state reset after")
    ap.add_argument("--matrix-path", choices=("split", "split16", "fp32"), default=None,
                    help="fused ONF kernel: bf16x3 split-precision MFMA on 32x32x16 tiles (library default, fp32-faithful), the "
                         "same arithmetic on round 2's 16x16x32 kernel, or fp32 MFMA; not given = leave the library's choice "
                         "(NFOPP_MATRIX_PATH) alone")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the CPU baselines and the gated parity block (N = 1); a plain run "
                         "only sets up, warms up, times and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB)")
    ap.add_argument("--dry-run-ranks", action="store_true",
                    help="rank flow only (rendezvous + all-reduce of ones on gloo, no GPU call, no workload): launcher test")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args.gpus, sys.argv[1:])     # does not return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: the launcher around this process started a different number of "
                         "ranks (plain `python bench.py --gpus %d` starts its own)" % (args.gpus, world, args.gpus))
    if args.dry_run_ranks:
        return dry_run_rank(args, world, rank)
    from nfopp import _lib
    lib = _lib.load()
    if args.matrix_path is not None:
        _lib.check(lib.nfopp_set_matrix_path({"split": 1, "split16": 2, "fp32": 0}[args.matrix_path]))
    matrix_path = {1: "split", 2: "split16", 0: "fp32"}[lib.nfopp_get_matrix_path()]
    N = 512 if args.workload == "cfg5" else 256

    # one process per GPU; the modulo only matters for a rehearsal of the N-rank flow on a box with fewer GPUs
    # (NFOPP_DIST_BACKEND=gloo, several ranks sharing a card) -- on the benchmark node it is the identity
    dev_index = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    backend = os.environ.get("NFOPP_DIST_BACKEND", "nccl")
    if world > 1:
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=device)
        else:
            torch.distributed.init_process_group(backend)
    seen = ranks_seen(world, backend, device)

    B = args.batch_per_gpu
    env = GridMap() if args.workload == "cfg4" else DiscMap()
    onf, fit_loss = make_onf(device, env, args.fit_iters, 4096)
    rng = np.random.default_rng(4321)
    starts = env.free_poses(rng, world * B)
    goals = env.free_poses(rng, world * B)
    lo, hi = nfopp.shard_range(world * B, rank, world)
    truth = env.device_checker(device)
    learn = args.workload == "cfg5"   # continuous learning: ground truth on the device, forward-only constraints on
    planner = nfopp.BatchPlanner(onf, hi - lo, N, bench_hyper(), velocity_hessian_weight=0.5, device=device, seed=SEED,
                                 traj_index_offset=lo, checker=truth if learn else None, fit_lr=2e-2, angle_offset=0.3,
                                 global_batch=world * B)
    planner.init(starts[lo:hi], goals[lo:hi], BOUNDS)
    eng = planner.engine

    def one_step(ev=None):
        if learn and planner.step_count % planner.fit_freq == 0:
            planner.fit_field()
        if ev is not None:
            ev[0].record()
        eng.collision_eval()
        if ev is not None:
            ev[1].record()
        eng.update(False)
        if planner.step_count % planner.reparam_freq == 0:
            eng.reparametrize()
        planner.step_count += 1

    # setup, not measurement: a fresh box starts at idle clocks and the first process pays one-off costs (code-object
    # load, DVFS ramp).  Spin the device up on throw-away steps, then restore the initial planner state (and the draw
    # stream: step k of the run uses Philox word k, which is what the CPU parity legs replay).
    for _ in range(args.spin_up):
        one_step()
    torch.cuda.synchronize()
    if args.spin_up:
        planner.init(starts[lo:hi], goals[lo:hi], BOUNDS)
        eng.rng_offset = 0
    for _ in range(args.warmup):
        one_step()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        one_step(events[k])
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=device if backend == "nccl" else "cpu")
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tmax.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, planner, learn, world, rank)

    parity_failed = False
    if rank == 0:
        k1_ms = float(np.mean([a.elapsed_time(b) for a, b in events]))
        samples = (hi - lo) * (N - 1)
        achieved = samples * FLOP_PER_SAMPLE / (k1_ms * 1e-3) / 1e12
        paths = planner.get_paths()
        finite = bool(np.isfinite(paths).all())
        if learn:
            workload = ("BASELINE configs[4] per GPU: %d trajectories x %d waypoints, forward-only constraints, continuous ONF "
                        "learning every step on %d device-sampled poses per GPU, gradient all-reduce over ranks (last fit "
                        "loss %.3f)" % (B, N, planner.sampler.B * planner.sampler.S, float(planner.fitter.last_loss)))
        else:
            workload = ("BASELINE configs[%d] per GPU: %d trajectories x %d waypoints, %s, SE(2) constrained planner, frozen "
                        "pre-fitted ONF (F=220, fit loss %.3f)" % (3 if args.workload == "cfg4" else 2, B, N, env.name, fit_loss))
        traffic, traffic_source = pmc_traffic(args.workload, B, N)
        out = {
            "metric": "waypoint-evals/sec", "value": world * B * N * args.steps / elapsed, "unit": "waypoint-evals/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "ranks_seen": seen, "backend": (backend if world > 1 else "none (single process)"),
            "config": {"workload": workload, "trajectories_per_gpu": B, "waypoints": N, "global_batch": world * B,
                       "parallelism": "trajectory shards + one all-reduce of the 33163-float ONF gradient buffer per step"
                       if learn else "trajectory shards, no data-path collective",
                       "paths_finite": finite, "matrix_path": matrix_path, "planner_steps_per_s": args.steps / elapsed},
            "roofline": roofline(matrix_path, achieved, k1_ms, samples, traffic, traffic_source),
        }
        if args.full and args.cpu_sample > 0 and world == 1:   # CPU legs: N = 1 only (bench contract); N > 1 lines carry the rate
            sample = min(args.cpu_sample, hi - lo)
            flat = onf.flat_parameters.cpu().numpy()
            cpu = cpu_baselines(flat, starts, goals, N, sample, args.cpu_seconds)
            out["cpu_baseline"] = cpu["strong"]
            out["cpu_baseline_reference_faithful"] = cpu["reference_faithful"]
            out["cpu_host"] = {"visible_cores": cpu["host_cores"], "usable_cores": cpu["usable_cores"], "model": cpu["cpu_model"]}
            if not learn:   # frozen field: the CPU legs can replay the run exactly
                short = short_parity(onf, starts, goals, N, sample, args.parity_steps, device)
                out["parity"] = {"ok": bool(short["gate"]["ok"] and finite), "short": short,
                                 "final": final_parity(planner, truth, onf, starts, goals, N, args.warmup + args.steps,
                                                       min(32, sample))}
                parity_failed = not out["parity"]["ok"]
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if parity_failed:
        sys.stderr.write("bench.py: parity gate FAILED (see the line's parity.short.gate)\n")
        sys.exit(4)


if __name__ == "__main__":
    main()
