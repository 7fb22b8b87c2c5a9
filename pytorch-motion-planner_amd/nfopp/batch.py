"""Batched / sharded planning over B independent trajectories that share one ONF (the batch axis is new: the
reference plans one trajectory per process, nfop/planner_factory.py:55,69).

* `BatchPlanner`   -- B trajectories on one GPU: init / step / get_paths, frozen or continuously fitted ONF.
* `shard_range`    -- contiguous split of a global batch over ranks; each rank passes its first global index as
                      `traj_index_offset` so the in-kernel Philox stream (and hence every result) is independent of
                      how the batch is sharded.  The frozen-ONF step needs NO collective.
* `OnfFitter`      -- ONF fitting step for data-parallel continuous learning: local gradient kernel (normalised by
                      the GLOBAL sample count), one all-reduce(SUM) of the flat [n_params + 2] buffer (RCCL over
                      xGMI when the process group is "nccl"), then the identical Adam step on every rank, so the
                      replicated weights stay bit-identical across ranks.
"""
import numpy as np
import torch

from . import _lib
from .engine import TrajectoryEngine, field_model
from .grid_search import AstarTrajectoryInitializer, OccupancyGrid, grid_search_init
from .lattice import GearLattice, LatticeGrid, lattice_gear_search_init, lattice_search_init
from .path_tools import init_trajectories


def shard_range(global_batch, rank, world_size):
    """[lo, hi) of the trajectories owned by `rank` (contiguous, sizes differ by at most one)."""
    base, rem = divmod(int(global_batch), int(world_size))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def _linspace_rows(a, b, steps):
    """Row-wise torch.linspace (fp32 CPU rounding: fp32 step, one fused multiply-add per element, two-sided)."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    step = ((b - a) / np.float32(steps - 1)).astype(np.float32).astype(np.float64)
    i = np.arange(steps)
    lo = (a.astype(np.float64)[:, None] + step[:, None] * i[None]).astype(np.float32)
    hi = (b.astype(np.float64)[:, None] - step[:, None] * (steps - 1 - i)[None]).astype(np.float32)
    return np.where(i[None] < steps // 2, lo, hi)


def straight_line_init(starts, goals, n_waypoints):
    """Batched TrajectoryInitializer (nfop/trajectory_initializer.py:12-29): xy on the segment start->goal, theta
    interpolated along the wrapped shortest rotation.  Host numpy, one-time per `init`."""
    starts = np.asarray(starts, np.float32)
    goals = np.asarray(goals, np.float32)
    d = starts.shape[1]
    out = np.zeros((starts.shape[0], n_waypoints, d), np.float32)
    for k in range(2):
        out[:, :, k] = _linspace_rows(starts[:, k], goals[:, k], n_waypoints + 2)[:, 1:-1]
    if d == 3:
        pi, two_pi = np.float32(np.pi), np.float32(2 * np.pi)
        delta = (np.remainder((goals[:, 2] - starts[:, 2]) + pi, two_pi).astype(np.float32) - pi).astype(np.float32)
        out[:, :, 2] = _linspace_rows(starts[:, 2], (delta + starts[:, 2]).astype(np.float32), n_waypoints + 2)[:, 1:-1]
    return out


class OnfFitter(object):
    """One BCE/Adam step of the shared field on this rank's samples; gradients summed over `group` first."""

    def __init__(self, onf, lr, betas, eps=1e-8, group=None, grad_fn=None, distributed=True):
        self.onf, self.lr, self.betas, self.eps, self.group = onf, float(lr), tuple(betas), float(eps), group
        # distributed=False: purely local fit even inside an initialised process group (e.g. identical pre-fits)
        self.distributed = bool(distributed)
        flat = onf.flat_parameters
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.step_count = 0
        self.grad = torch.zeros(onf.n_params + 2, dtype=torch.float32, device=flat.device)
        self._ws = None
        self._grad_fn = grad_fn or self._hip_grad
        self._adam_fn = self._hip_adam if grad_fn is None else None
        self.last_loss = None

    def _hip_grad(self, samples, labels, inv_count):
        lib = _lib.load()
        cfg = self.onf.config_c()
        p = samples.shape[0]
        need = lib.nfopp_onf_train_workspace_bytes(cfg, p)
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=samples.device)
        _lib.check(lib.nfopp_onf_train_grad(cfg, _lib.ptr(self.onf.flat_parameters), _lib.ptr(samples),
                                            _lib.ptr(labels), p, inv_count, _lib.ptr(self.grad), _lib.ptr(self._ws),
                                            self._ws.numel() * 4, _lib.stream_ptr()))

    def _hip_adam(self, step_size, bc2_sqrt):
        b1, b2 = self.betas
        _lib.check(_lib.load().nfopp_adam_step(_lib.ptr(self.onf.flat_parameters), _lib.ptr(self.grad), _lib.ptr(self.m),
                                               _lib.ptr(self.v), self.onf.n_params, b2, 1 - b1, 1 - b2, self.eps,
                                               step_size, bc2_sqrt, _lib.stream_ptr()))
        self.onf.mark_modified()   # a raw-pointer write: torch's version counter does not see it

    def _in_group(self):
        return self.distributed and torch.distributed.is_available() and torch.distributed.is_initialized()

    def global_count(self, local_count):
        """Sample count over all ranks when the caller cannot state it: ONE extra all-reduce and a host sync.  The
        hot loop never takes this path -- `BatchPlanner` passes the count it knows statically (global batch x poses per
        trajectory); it exists for ragged, caller-managed sample sets."""
        if not self._in_group():
            return int(local_count)
        gloo = torch.distributed.get_backend(self.group) == "gloo"
        c = torch.tensor([float(local_count)], dtype=torch.float64, device="cpu" if gloo else self.grad.device)
        torch.distributed.all_reduce(c, group=self.group)
        return int(c.item())

    def world_size(self):
        return torch.distributed.get_world_size(self.group) if self._in_group() else 1

    def step(self, samples, labels, global_count=None, adam_fn=None):
        """samples [P_local, point_dim], labels [P_local] on this rank's device.  `global_count` = number of samples
        over ALL ranks (the BCE mean's denominator); pass it whenever it is known without communication.  Returns
        the global mean loss (a device scalar; no host sync)."""
        p = samples.shape[0]
        total = self.global_count(p) if global_count is None else int(global_count)
        self._grad_fn(samples, labels, 1.0 / total)
        if self._in_group():
            if self.grad.is_cuda and torch.distributed.get_backend(self.group) == "gloo":
                host = self.grad.cpu()           # rehearsal path only: gloo reduces host buffers
                torch.distributed.all_reduce(host, group=self.group)
                self.grad.copy_(host)
            else:
                torch.distributed.all_reduce(self.grad, group=self.group)   # SUM; RCCL on the "nccl" backend
        self.step_count += 1
        b1, b2 = self.betas
        step_size = self.lr / (1 - b1 ** self.step_count)
        bc2_sqrt = (1 - b2 ** self.step_count) ** 0.5
        (adam_fn or self._adam_fn)(step_size, bc2_sqrt)
        self.last_loss = self.grad[self.onf.n_params]
        return self.last_loss


class BatchPlanner(object):
    """B trajectories, one shared ONF, one GPU.  `step()` = the planner step of nfop/nerf_opt_planner.py:60-71 for the
    whole batch: [ONF fit on freshly sampled poses, when a ground-truth `checker` is given] -> one
    `_optimize_trajectory` per trajectory -> periodic reparametrisation.  Without a checker the field is frozen.

    The planner owns the field's update loop, so it FREEZES the ONF object (`ONF.freeze()`): launches reuse the pre-split
    weight image until the planner's own Adam step (or an in-place torch op) changes the parameters.  A caller who writes
    the parameters behind torch's back while a planner exists -- `dist.broadcast(onf.flat_parameters, 0)`, `.data`
    assignments -- must call `onf.mark_modified()` afterwards (or construct with `freeze_field=False`).

    `moving` (an nfopp.MovingObstacles) makes the step yield to predicted tracks: behind the collision model's rows runs the
    overlay of csrc/track_field.hip, which needs the time of every waypoint -- `set_waypoint_times`, before the
    first step (a step without them raises ValueError).  With `moving=None` every call is the one it was.

    `onf` may be a `DistanceField` or a `HeadingDistanceField` instead: the collision term then comes from the signed distance
    image of an occupancy grid (csrc/sdf_field.hip, csrc/heading_field.hip) and everything else -- init, step(n), replan,
    evaluate, path_stats, the seeders -- is as it is behind the network.  `freeze_field` does not apply and `checker=` raises ValueError: there is nothing to fit."""

    def __init__(self, onf, batch, n_waypoints, hyper, velocity_hessian_weight=0.5, reparametrize_trajectory_freq=10,
                 device="cuda", seed=0, traj_index_offset=0, checker=None, fit_lr=2e-2, fit_betas=(0.9, 0.9),
                 optimize_collision_model_freq=1, trajectory_random_offset=0.02, course_random_offset=1.5,
                 angle_offset=0.0, random_field_points=10, collision_point_count=100, group=None,
                 init_angles_with_trajectory=False, global_batch=None, freeze_field=True, moving=None):
        if field_model(onf):
            # a distance field (engine.FIELD_MODELS): the map is the model, there is nothing to freeze or to fit
            if checker is not None:
                raise ValueError("a distance field is not fitted: checker= goes with an ONF (pass the checker to evaluate())")
        elif freeze_field:
            onf.freeze()
        self.init_angles_with_trajectory = bool(init_angles_with_trajectory)
        # trajectories over ALL ranks (continuous learning: denominator of the BCE mean); default = equal shards
        self.global_batch = None if global_batch is None else int(global_batch)
        self.engine = TrajectoryEngine(onf, batch, n_waypoints, onf.point_dim, hyper, velocity_hessian_weight, device,
                                       seed=seed, traj_index_offset=traj_index_offset, moving=moving)
        self.onf = onf
        self.reparam_freq = int(reparametrize_trajectory_freq)
        self.step_count = 0
        self.checker = checker
        self.fit_freq = int(optimize_collision_model_freq)
        self.sampler = self.fitter = self._prev = None
        if checker is not None:
            from .learning import BatchSampler
            self.sampler = BatchSampler(onf, batch, n_waypoints, course_random_offset, trajectory_random_offset,
                                        angle_offset, random_field_points, collision_point_count, device,
                                        seed=seed + 1, traj_index_offset=traj_index_offset)
            self.fitter = OnfFitter(onf, fit_lr, fit_betas, group=group)

    seed_status = None   # per-problem status of the last grid-search seeding (nfopp/grid_search.py), else None
    seed_gear_changes = None   # gear changes of each problem's seed after a GearLattice initializer, else None
    seed_margin = None   # the clearance margin each problem was seeded at (all zero without one); None without grid seeding

    def init(self, starts, goals, boundaries, trajectories=None, initializer=None, seed_clearance=None, seed_any_angle=False,
             seed_turn_cost=0):
        """`seed_clearance` / `seed_any_angle`: grid_search_init's `clearance` / `any_angle` for an OccupancyGrid initializer
        (an AstarTrajectoryInitializer carries its own).  A LatticeGrid initializer seeds SE(2) batches through
        lattice_search_init with `seed_turn_cost`; it takes neither of the two: shortening by line of sight would undo the
        heading constraint, and a margin is built into the lattice (LatticeGrid.from_grid(grid.inflated(m))).  A GearLattice
        initializer does the same through lattice_gear_search_init, with reverse moves at its costs, and sets
        `seed_gear_changes`."""
        eng = self.engine
        eng.set_endpoints(starts, goals)
        eng.hyper = eng.hyper.replace(bounds=boundaries)
        self.seed_status = self.seed_margin = self.seed_gear_changes = None
        if isinstance(initializer, (LatticeGrid, GearLattice)):
            if seed_clearance is not None or seed_any_angle:
                raise ValueError("seed_clearance / seed_any_angle do not go with a LatticeGrid: build it from grid.inflated(m)")
            if eng.D != 3:
                raise ValueError("a LatticeGrid seeds SE(2) trajectories (D = 3) only")
        elif seed_turn_cost != 0:
            raise ValueError("seed_turn_cost goes with a LatticeGrid initializer")
        if seed_clearance is not None and not isinstance(initializer, OccupancyGrid):
            raise ValueError("seed_clearance goes with an OccupancyGrid initializer")
        if seed_any_angle and not isinstance(initializer, OccupancyGrid):
            raise ValueError("seed_any_angle goes with an OccupancyGrid initializer")
        if initializer is not None:
            # grid-search seeding of the whole batch (csrc/grid_search.hip): an OccupancyGrid or an AstarTrajectoryInitializer
            if trajectories is not None:
                raise ValueError("pass trajectories or an initializer, not both")
            if isinstance(initializer, OccupancyGrid):
                _, self.seed_status, self.seed_margin = grid_search_init(
                    initializer, eng.start, eng.goal, eng.N, self.init_angles_with_trajectory and eng.D == 3, out=eng.traj,
                    clearance=() if seed_clearance is None else seed_clearance, any_angle=bool(seed_any_angle))
            elif isinstance(initializer, LatticeGrid):
                _, self.seed_status = lattice_search_init(initializer, eng.start, eng.goal, eng.N,
                                                          self.init_angles_with_trajectory, out=eng.traj,
                                                          turn_cost=seed_turn_cost)
            elif isinstance(initializer, GearLattice):
                _, self.seed_status, self.seed_gear_changes = lattice_gear_search_init(
                    initializer.lgrid, eng.start, eng.goal, eng.N, out=eng.traj, turn_cost=seed_turn_cost,
                    reverse_cost=initializer.reverse_cost, cusp_cost=initializer.cusp_cost)
            elif isinstance(initializer, AstarTrajectoryInitializer):
                initializer.initialize_batch(eng.start, eng.goal, eng.N, out=eng.traj, boundaries=boundaries)
                self.seed_status, self.seed_margin = initializer.status, initializer.seed_margin
            else:
                raise TypeError("initializer must be an OccupancyGrid, a LatticeGrid, a GearLattice or an AstarTrajectoryInitializer")
        elif trajectories is None:
            # device initialiser (trajectory_initializer.py:12-45); eng.start / eng.goal were uploaded just above
            init_trajectories(eng.start, eng.goal, eng.N, self.init_angles_with_trajectory and eng.D == 3, out=eng.traj)
        else:
            eng.traj.copy_(torch.as_tensor(np.asarray(trajectories, np.float32)).reshape(eng.traj.shape))
        for buf in (eng.lam, eng.cm, eng.adam_m, eng.adam_v):
            if buf is not None:
                buf.zero_()
        eng.adam_step = 0
        self.step_count = 0
        self._prev = None

    def set_waypoint_times(self, times):
        """times [B, N], or [N] for every trajectory alike: when the robot is at interior waypoint i, for `moving`.  From a
        `TimedPaths` profile of these paths (`timed_paths(limits)`) they are `profile[:, 1:-1, nfopp.TIME_SLOT_T]`: the profile
        has the start and the goal around the N waypoints."""
        self.engine.set_waypoint_times(times)

    def uniform_waypoint_times(self, t_start, duration):
        """Sets and returns the times of a robot that leaves the start at `t_start` and reaches the goal `duration` later at a
        constant pace in the waypoint index: T[i] = t_start + duration * (i + 1) / (N + 1), formed in double and rounded once."""
        n = self.engine.N
        times = torch.from_numpy((float(t_start) + float(duration) * np.arange(1, n + 1) / (n + 1.0)).astype(np.float32))
        self.engine.set_waypoint_times(times)
        return times

    def fit_field(self):
        """One `_optimize_collision_model` over the batch (nerf:76-91): poses from the PREVIOUS trajectories, labels
        from the device checker, gradient all-reduced over the process group, identical Adam on every rank."""
        eng = self.engine
        if self._prev is None:
            self._prev = eng.traj.detach().clone()
        samples = self.sampler.draw(self._prev, eng.hyper.bounds)
        self._prev.copy_(eng.traj)
        labels = self.checker.labels(samples, out=self.sampler.labels)
        # the sample count over all ranks is known statically: no count all-reduce, no host sync in the step
        gb = self.global_batch if self.global_batch is not None else self.fitter.world_size() * eng.B
        return self.fitter.step(samples, labels, global_count=gb * self.sampler.S)

    def step(self, t=None, want_terms=False, n=1):
        """One planner step for the whole batch -- or `n` of them (`step(n=...)`): with a frozen field (no checker) the n
        steps are enqueued by ONE library call (nfopp_traj_steps), without returning to Python in between -- the form
        the callers' loops want (nfop/ros/goal_planner_adapter.py:50-52, scripts/run_planner.py:76-77).  With continuous
        learning every fit needs fresh samples, so the steps run one by one.  `t` [B, N-1] (n = 1) or [n, B, N-1]
        injects the draws.  Bit-identical to n calls of `step()`."""
        n = int(n)
        if n > 1 or (n == 1 and self.checker is None and t is None):
            if self.checker is None:
                self.engine.steps(n, self.step_count, self.reparam_freq, t_steps=t, want_terms=want_terms)
                self.step_count += n
                return
            for k in range(n):
                self.step(None if t is None else t[k], want_terms=want_terms and k == n - 1)
            return
        if n < 1:
            return
        if self.checker is not None and self.step_count % self.fit_freq == 0:
            self.fit_field()
        self.engine.optimize_trajectory(t, want_terms=want_terms)
        if self.step_count % self.reparam_freq == 0:
            self.engine.reparametrize()
        self.step_count += 1

    # ---- receding-horizon replanning (nfop/ros/goal_planner_adapter.py:44-53: update_start_point -> step()s -> get_path) ----
    def _update_endpoints(self, which, points, moved):
        """One nfopp_update_endpoints launch plus the bookkeeping the new endpoints invalidate.  `step_count` goes back to
        0 as in the reference (the next step fits, if learning is on, and reparametrises); the Adam moments and `adam_step`
        stay, as the reference keeps its optimiser state.  Nothing here synchronises when `points` / `moved` are device tensors."""
        eng = self.engine
        if moved is not None and not isinstance(moved, torch.Tensor):
            moved = torch.from_numpy(np.ascontiguousarray(moved).astype(np.uint8)).to(eng.device)
        eng.update_endpoints(which, points, moved)
        # the best path on record joined the old endpoints, and a retired trajectory has to move again: masked device ops
        if eng.active is not None:
            if moved is None:
                eng.active.fill_(1)
            else:
                eng.active.masked_fill_(moved.view(-1) != 0, 1)
        if hasattr(self, "best_length"):
            if moved is None:
                self.best_length.fill_(float("inf"))
            else:
                self.best_length.masked_fill_(moved.view(-1) != 0, float("inf"))
        self.step_count = 0

    def update_start_points(self, points, moved=None):
        """Batched `update_start_point` (constrained:187-194 / nerf:210-216): every trajectory -- or those with
        `moved[b] != 0` -- is cut back to its new start [B, D] and reparametrised; the others are left bit for bit."""
        self._update_endpoints(0, points, moved)

    def update_goal_points(self, points, moved=None):
        """Batched `update_goal_point` (constrained:178-185 / nerf:202-208)."""
        self._update_endpoints(1, points, moved)

    def set_boundaries(self, boundaries):
        """`set_boundaries` (nerf:218-220): new sampling / boundary-loss box, `step_count` back to 0.  The hyper value is
        replaced as `init()` replaces it, so the kernels' cached scalar block is formed afresh."""
        self.engine.hyper = self.engine.hyper.replace(bounds=boundaries)
        self.step_count = 0

    def replan(self, starts=None, goals=None, moved=None, n=1):
        """One tick of the receding-horizon loop: endpoint update(s), then `step(n=n)`.  With a frozen field and
        device-tensor inputs the whole tick is enqueued without a host synchronisation."""
        if starts is not None:
            self.update_start_points(starts, moved)
        if goals is not None:
            self.update_goal_points(goals, moved)
        self.step(n=n)

    def get_paths(self):
        return self.engine.full_trajectory().detach().cpu().numpy()

    # ---- path evaluation, best-path bookkeeping, early stop (scripts/run_bench_mr.py:109-132 for the batch) ---------
    def evaluate(self, checker=None, sub=4, early_stop=False, min_clearance=None, swept=False, refine=None):
        """Densifies every path (`sub` poses per segment), labels the poses with the ground-truth `checker`, keeps
        the shortest collision-free path per trajectory and -- with early_stop -- retires trajectories that are
        collision-free but no longer improving.  With `min_clearance` (point-cloud checkers only) a pose also counts as
        colliding when the footprint's clearance is below it: a safety margin without a fatter robot.  With `swept`
        (point-cloud checkers only) a path also counts as colliding unless every segment between two consecutive dense
        poses is certified free (`checker.swept`): the best path and the early stop then advance on certified paths only.
        With `refine=<max_depth>` as well (box checker only) the segments the one-shot certificate leaves undecided are
        bisected on the device (`checker.swept_refine`): a path counts as colliding only where a segment is a proven hit or
        still undecided at that depth.  Returns device tensors (collides uint8 [B], length [B])."""
        from . import _lib as L
        checker = checker or self.checker
        if checker is None:
            raise ValueError("evaluate() needs a ground-truth checker")
        if refine is not None:   # before anything is launched or overwritten
            if not swept:
                raise ValueError("refine= belongs to the swept check: pass swept=True")
            self._check_refine(checker, refine)
        eng = self.engine
        B, N, D = eng.B, eng.N, eng.D
        m = (N + 1) * int(sub) + 1
        f32 = dict(dtype=torch.float32, device=eng.device)
        if getattr(self, "_eval_sub", None) != sub:
            self._eval_sub = sub
            self._poses = torch.empty(B, m, D, **f32)
            self._pose_labels = torch.empty(B * m, **f32)
            self._length = torch.empty(B, **f32)
            self._collides = torch.zeros(B, dtype=torch.uint8, device=eng.device)
        if not hasattr(self, "best_length"):
            self.best_length = torch.full((B,), float("inf"), **f32)
            self.best_traj = eng.traj.detach().clone().view(B, N, D)
        if early_stop and eng.active is None:
            eng.active = torch.ones(B, dtype=torch.uint8, device=eng.device)
        lib = L.load()
        L.check(lib.nfopp_path_interpolate(L.ptr(eng.traj), L.ptr(eng.start), L.ptr(eng.goal), B, N, D, int(sub),
                                           L.ptr(self._poses), L.ptr(self._length), L.stream_ptr()))
        checker.labels(self._poses.view(B * m, D), out=self._pose_labels)
        if min_clearance is not None:   # combined on the device, no synchronisation
            clearance = checker.clearance(self._poses.view(B * m, D), out=self._pose_clearance(B * m))
            self._pose_labels.masked_fill_(clearance < float(min_clearance), 1.0)
        if swept:
            self._swept_labels(checker, self._poses, self._pose_labels, refine=refine)
        L.check(lib.nfopp_path_select_best(L.ptr(self._pose_labels), L.ptr(self._length), L.ptr(eng.traj), B, m, N, D,
                                           L.ptr(self.best_traj), L.ptr(self.best_length),
                                           L.ptr(self._collides, torch.uint8),
                                           L.ptr(eng.active, torch.uint8) if early_stop else None, L.stream_ptr()))
        return self._collides, self._length

    def _swept_labels(self, checker, poses, labels, status=None, worst=None, refine=None):
        """Segment values of the dense `poses` [B, m, D] and their reduction into `labels` [B * m]; no synchronisation.
        With `refine` (a depth) the segments go through `checker.swept_refine` and nfopp_path_refined_labels instead, and
        `worst` receives the reduction's `first`; the segment buffers are the same, the values' holding the hits' s."""
        if refine is not None:
            self._check_refine(checker, refine)
        if not hasattr(checker, "swept_labels"):
            raise NotImplementedError("the swept check needs a point cloud: use DeviceCircleChecker or "
                                      "DeviceRectangleChecker, not %s" % type(checker).__name__)
        B, m, D = poses.shape
        buf = getattr(self, "_segments", None)
        if buf is None or buf[0].shape != (B, m - 1, D):
            f32 = dict(dtype=torch.float32, device=poses.device)
            buf = self._segments = (torch.empty(B, m - 1, D, **f32), torch.empty(B, m - 1, D, **f32),
                                    torch.empty(B, m - 1, **f32))
        seg_a, seg_b, values = buf
        seg_a.copy_(poses[:, :-1])
        seg_b.copy_(poses[:, 1:])
        if refine is not None:
            seg_status = getattr(self, "_segment_status", None)
            if seg_status is None or seg_status.shape != (B, m - 1):
                seg_status = self._segment_status = torch.empty(B, m - 1, dtype=torch.uint8, device=poses.device)
            checker.swept_refine(seg_a, seg_b, max_depth=int(refine), status_out=seg_status.view(-1), s_out=values.view(-1),
                                 depth_out=False)
            checker.refined_labels(seg_status, values, labels, status, worst)
            return
        checker.swept(seg_a, seg_b, out=values.view(-1), index_out=False)
        checker.swept_labels(poses, values, labels, status, worst)

    @staticmethod
    def _check_refine(checker, refine):
        """refine= is a depth of the box robot's bisection: ValueError for any other checker or depth."""
        if getattr(checker, "_box", None) is None or not hasattr(checker, "swept_refine"):
            raise ValueError("refine= is the box robot's (DeviceRectangleChecker), not %s's: the disc's swept test is exact "
                             "and an occupancy image has no swept check" % type(checker).__name__)
        if int(refine) != refine or not 0 <= int(refine) <= 20:
            raise ValueError("refine= is a depth between 0 and 20, not %r" % (refine,))

    def certify(self, checker=None, sub=4, refine=None):
        """(status uint8 [B], worst fp32 [B, 2]) device tensors for the current paths, densified as `evaluate` densifies them:
        status 0 = every segment between consecutive poses certified free and no pose in collision, 1 = a pose (for the disc
        robot: or a segment) in collision, 2 = box robot only, no pose collides but a segment could not be certified --
        raise `sub`, or pass `refine`.  worst = the smallest segment value (`checker.swept`) and the segment attaining it.
        With `refine=<max_depth>` (box checker only; ValueError otherwise) the segments are bisected on the device
        (`checker.swept_refine`) and the result is (status, first): status 1 = a pose collides or a segment is a proven hit,
        2 = a segment is still undecided at that depth, 0 = proven free; first fp32 [B, 2] = the first segment that is not
        proven free and its s, (-1, -1) without one.  The best-path bookkeeping is not touched; nothing synchronises."""
        from . import _lib as L
        checker = checker or self.checker
        if checker is None:
            raise ValueError("certify() needs a ground-truth checker")
        if refine is not None:
            self._check_refine(checker, refine)
        eng = self.engine
        B, N, D = eng.B, eng.N, eng.D
        m = (N + 1) * int(sub) + 1
        f32 = dict(dtype=torch.float32, device=eng.device)
        poses, length = torch.empty(B, m, D, **f32), torch.empty(B, **f32)
        L.check(L.load().nfopp_path_interpolate(L.ptr(eng.traj), L.ptr(eng.start), L.ptr(eng.goal), B, N, D, int(sub),
                                                L.ptr(poses), L.ptr(length), L.stream_ptr()))
        labels = checker.labels(poses.view(B * m, D))
        status, worst = torch.empty(B, dtype=torch.uint8, device=eng.device), torch.empty(B, 2, **f32)
        self._swept_labels(checker, poses, labels, status, worst, refine=refine)
        return status, worst

    def _pose_clearance(self, count):
        buf = getattr(self, "_clearance", None)
        if buf is None or buf.numel() != count:
            buf = self._clearance = torch.empty(count, dtype=torch.float32, device=self.engine.device)
        return buf

    def path_stats(self, checker=None, sub=4, cusp_angle=np.pi / 3):
        """[B, 8] float64 device tensor of per-path statistics (nfopp_path_stats; slots nfopp.PATH_STAT_*): length, maximum
        Menger curvature and its vertex, cusps, reversals, minimum clearance and its pose, mean clearance.  The clearance
        is the checker's footprint clearance at the poses `evaluate` tests (`sub` per segment); without a point-cloud
        checker those three slots are +inf, -1, +inf.  A vertex is a cusp when the path folds back there to within
        `cusp_angle` of the way it came (the segments' directions differ by more than pi - cusp_angle).  Retired
        trajectories are included.  Nothing here synchronises."""
        from . import _lib as L
        checker = checker or self.checker
        eng = self.engine
        B, N, D = eng.B, eng.N, eng.D
        lib = L.load()
        dist, m = None, 0
        if checker is not None and hasattr(checker, "nearest"):
            m = (N + 1) * int(sub) + 1
            poses = torch.empty(B, m, D, dtype=torch.float32, device=eng.device)
            length = torch.empty(B, dtype=torch.float32, device=eng.device)
            L.check(lib.nfopp_path_interpolate(L.ptr(eng.traj), L.ptr(eng.start), L.ptr(eng.goal), B, N, D, int(sub),
                                               L.ptr(poses), L.ptr(length), L.stream_ptr()))
            dist = checker.clearance(poses.view(B * m, D))
            self._stat_poses, self._stat_clearance = poses, dist.view(B, m)
        stats = torch.empty(B, L.NUM_PATH_STATS, dtype=torch.float64, device=eng.device)
        L.check(lib.nfopp_path_stats(L.ptr(eng.traj), L.ptr(eng.start), L.ptr(eng.goal), B, N, D, L.ptr(dist), m,
                                     float(np.cos(np.pi - float(cusp_angle))), L.ptr(stats, torch.float64),
                                     L.ptr(eng.active, torch.uint8), L.stream_ptr()))
        return stats

    def _best_traj(self):
        """[B, N, D] device tensor: the waypoints `best_paths` returns."""
        eng = self.engine
        tr = eng.traj.view(eng.B, eng.N, eng.D)
        if not hasattr(self, "best_length"):
            return tr
        return torch.where(torch.isfinite(self.best_length)[:, None, None], self.best_traj, tr)

    def best_paths(self):
        """[B, N+2, D]: the best collision-free path found so far, the current path where none was found yet."""
        eng = self.engine
        if not hasattr(self, "best_length"):
            return self.get_paths()
        return torch.cat([eng.start[:, None], self._best_traj(), eng.goal[:, None]], dim=1).cpu().numpy()

    def timed_paths(self, limits, v_start=None, v_goal=None, best=False):
        """The velocity profile of every path under `limits` (nfopp.MotionLimits) as an nfopp.TimedPaths: `.profile`,
        `.gear`, `.summary` and `.sample(dt, count)` -- of the current paths, or with `best` of what `best_paths()` returns.
        `v_start` / `v_goal`: None (rest), a number or [B]; in a replanning tick `v_start` is the robot's current speed.
        With device-tensor (or no) speeds nothing here synchronises."""
        from .time_profile import time_parametrize
        eng = self.engine
        traj = self._best_traj() if best else eng.traj.view(eng.B, eng.N, eng.D)
        return time_parametrize(traj, eng.start, eng.goal, limits, v_start, v_goal)

    def fleet_conflicts(self, limits, dt, count, radius, margin="chord", v_start=None, v_goal=None, best=False, obstacles=None,
                        obstacle_radius=None, obstacle_v_max=None, want_pairs=False, box=None, refine=0, obstacle_box=None,
                        obstacle_w_max=None):
        """The B paths as B robots that start together on one floor: time-parametrise under `limits`, sample at k * dt
        (k < count) and check every robot against every other (nfopp.TrackConflicts: `.summary` [B, 7]).  `radius`: a
        number or [B]; `margin="chord"` covers what a robot can do between two instants.  With `obstacles` [M, count, >= 2]
        (predicted tracks on the same grid, e.g. `nfopp.constant_velocity_tracks`) the paths are also checked against
        those, and the result is the pair (fleet, against obstacles); the chord margin then needs `obstacle_v_max`.
        With `box` (x0, x1, y0, y1) the robots are oriented boxes (nfopp.BoxTrackConflicts; `radius` rounds them, `refine`
        halves undecided intervals, obstacles carry x, y, theta and take `obstacle_box` / `obstacle_w_max`): see
        `TimedPaths.conflicts`.  Nothing here synchronises with device-tensor arguments."""
        timed = self.timed_paths(limits, v_start=v_start, v_goal=v_goal, best=best)
        shape = {} if box is None and refine == 0 and obstacle_box is None else dict(box=box, refine=refine)
        fleet = timed.conflicts(dt, count, radius=radius, margin=margin, want_pairs=want_pairs, **shape)
        if obstacles is None:
            return fleet
        if shape:
            shape.update(other_box=obstacle_box, other_w_max=obstacle_w_max)
        return fleet, timed.conflicts(dt, count, other=obstacles, radius=radius, other_radius=obstacle_radius, margin=margin,
                                      other_v_max=obstacle_v_max, want_pairs=want_pairs, **shape)

    def fleet_schedule(self, limits, dt, count, radius, max_delay, margin="chord", order=None, best=False, obstacles=None,
                       obstacle_radius=None, obstacle_v_max=None, v_start=None, v_goal=None, box=None, refine=0, obstacle_box=None,
                       obstacle_w_max=None, replan_radius=None, replan=None):
        """The B paths as B robots on one floor that may leave late: time-parametrise under `limits`, sample at k * dt
        (k < count) and give every robot, in priority `order` (None: robot 0 first; "longest_first"; or [B] indices), the
        smallest start delay of 0 .. max_delay grid steps that keeps it clear of the robots scheduled before it and of
        `obstacles` -- a `TimedPaths`, or predicted tracks [M, count + max_delay, >= 2] (then the chord margin needs
        `obstacle_v_max`) -> nfopp.FleetSchedule.  Nothing here synchronises with device-tensor arguments.

        `replan`: an OccupancyGrid (inflated for the robot's footprint).  The robots the schedule could not place are then
        searched on it in space-time over count + max_delay instants (`FleetSchedule.replan`, with the snap added to the
        schedule's margin; `radius` must be one number); the schedule comes back with `plan` (an nfopp.SpaceTimePlan) and
        `merged` [B, count + max_delay, 2].  Without it nothing changes.

        With `box` (x0, x1, y0, y1) the robots are oriented boxes (`TimedPaths.schedule_boxes`: `radius` rounds them, `refine`
        halves undecided intervals, obstacles carry x, y, theta and take `obstacle_box` / `obstacle_w_max`), and the scheduled
        fleet is FREE by `fleet_conflicts(box=, refine=)`.  The space-time search still reserves discs: with `box` and
        `replan` it takes `replan_radius`, the radius of the disc it reserves for every robot (the box's circumscribed disc
        plus its rounding radius is the safe choice); every obstacle is reserved as the disc that covers its box at every
        heading, the farthest corner plus `obstacle_radius` (`nfopp.conflicts.box_disc_radius`)."""
        timed = self.timed_paths(limits, v_start=v_start, v_goal=v_goal, best=best)
        if box is None:
            if refine != 0 or obstacle_box is not None or obstacle_w_max is not None or replan_radius is not None:
                raise ValueError("refine, obstacle_box, obstacle_w_max and replan_radius belong to the box schedule: give box")
            sched = timed.schedule(dt, count, max_delay, radius, margin=margin, order=order, other=obstacles,
                                   other_radius=obstacle_radius, other_v_max=obstacle_v_max)
        else:
            if replan is not None and replan_radius is None:
                raise ValueError("replan reserves discs: with box it needs replan_radius, the radius of the disc of a robot")
            sched = timed.schedule_boxes(dt, count, max_delay, box, radius=radius, margin=margin, order=order, refine=refine,
                                         other=obstacles, other_box=obstacle_box, other_radius=obstacle_radius,
                                         other_v_max=obstacle_v_max, other_w_max=obstacle_w_max)
        if replan is not None:
            if box is not None:
                radius = replan_radius
            if isinstance(radius, torch.Tensor) or np.ndim(radius) != 0:
                raise ValueError("replan plans a fleet of one robot radius: radius must be a number")
            sched.plan, sched.merged = sched.replan(sched.tracks, replan, int(count) + int(max_delay), robot_radius=radius,
                                                    base_margin=sched.margin, obstacles=sched.obstacles,
                                                    obstacle_radius=sched.obstacle_radius)
        return sched
