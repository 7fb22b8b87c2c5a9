/*
 * nfopp_hip.h -- C ABI of the MI355X-native NFOPP inner loop (libnfopp_hip.so).
 *
 * Drop-in boundary for ONE hot path of MisterMap/pytorch-motion-planner: the per-step work of
 * NERFOptPlanner / ConstrainedNERFOptPlanner `.step()`.  The reference has no native interface for this path
 * (it is PyTorch-CPU eager + autograd); each entry point below replaces the PyTorch op sequence cited next to
 * it (file:line under the reference root, `nfop/` = neural_field_optimal_planner/).  All pointers named *_dev are
 * DEVICE pointers (HIP, gfx950) to contiguous fp32 row-major arrays; sizes are element counts unless they say
 * bytes; `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous on `stream`.
 * Every function returns 0 on success and a negative nfopp_status otherwise; nfopp_last_error() describes the
 * last failure of the calling thread.  No torch types, no ownership transfer: buffers are borrowed for the call.
 *
 * Buffer contract: a call stores nothing outside the arrays it is given, at the sizes stated here; an array declared `const`
 * is not written; a pure output and a workspace need no initialisation -- no element of either is read before the call has
 * written it, so results do not depend on what the memory held; and where an entry says that elements are left alone (rows
 * of retired trajectories, slots that belong to another entry) they keep their bytes.  Each entry says which elements of its
 * pure outputs it writes.  tests/test_gpu_buffer_contracts.py pins all of this on bits and bytes for the entries of the step
 * and fit pipeline and for every entry that takes a workspace_dev.
 *
 * A batch of B trajectories is B independent reference problems that share one ONF (occupancy neural field).
 */
#ifndef NFOPP_HIP_H
#define NFOPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFOPP_ABI_VERSION 6
#define NFOPP_HIDDEN 100 /* width of both hidden layers, nfop/onf_model.py:18-23 */

typedef enum nfopp_status {
  NFOPP_OK = 0,
  NFOPP_ERR_ARG = -1,     /* bad shape / null pointer / unsupported configuration */
  NFOPP_ERR_HIP = -2,     /* HIP runtime error (message holds hipGetErrorString) */
  NFOPP_ERR_NO_DEVICE = -3
} nfopp_status;

/* Shape and normalisation of an ONF instance: nfop/onf_model.py:8-31.
 * The parameter buffer is ONE flat fp32 array in `state_dict()` order:
 *   [_angle_encoder._biases (2*angle_dim), _angle_encoder._frequencies (2*angle_dim)]   if angle_dim > 0
 *   mlp.0.weight [100, F], mlp.0.bias [100], mlp.2.weight [100,100], mlp.2.bias [100],
 *   mlp2.0.weight [1, 100+F], mlp2.0.bias [1], encoding_layer.weight [E, 2], [encoding_layer.bias [E]] if has_bias
 * with E = use_cos ? 200 : 100 and F = E + 2*angle_dim (220 for every shipped script).
 *
 * angle_dim outside 0 .. 16 is a bad configuration for every entry.  Inside it:
 *   E = 100: angle_dim 0 .. 14 (F <= 128),  E = 200: angle_dim 0 .. 12 (F <= 224) are evaluated; a larger one is refused with
 *     "unsupported ONF feature dimension" by every ONF entry (inference, trajectory evaluation, both fit paths).
 *   The default matrix path (1) evaluates the four shapes of the reference -- angle_dim 0 and 10 -- on its 32x32 kernels, and
 *     F = 128 / 224 (angle_dim 14 / 12) on the 16x16 kernels; every other accepted angle_dim is REFUSED there (NFOPP_ERR_ARG,
 *     "the 32x32 ONF kernel for .. input blocks is built for ..") and needs nfopp_set_matrix_path(0) or (2), which evaluate
 *     all of them.
 *   The MFMA fit (nfopp_onf_train_grad_ex path 2) needs one free pad position in the last input tile: F = 128 and 224 are
 *     refused with "no pad feature available"; the per-sample fit (path 1) takes every accepted angle_dim.
 * A refused call launches nothing and writes no output.  (Table: DESIGN.md section 3; tests/onf_geometry_cases.py.) */
typedef struct nfopp_onf_config {
  float mean;         /* nfop/onf_model.py:38  x = (x - mean) / sigma */
  float sigma;
  int32_t use_cos;    /* 1: sin on the first 100 encodings, cos on the next 100 (onf_model.py:40-41) */
  int32_t has_bias;   /* encoding_layer bias present */
  int32_t angle_dim;  /* 0 = no AngleEncoder (2-D points), 10 = nfop/angle_encoder.py default; accepted: 0 .. 14 (use_cos: 0 .. 12),
                         and on the default matrix path only 0, 10 and 14 (12): see above */
} nfopp_onf_config;

/* Scalars of one trajectory optimisation step.  SE(2) terms: nfop/constrained_nerf_opt_planner.py:76-130,
 * boundary nfop/nerf_opt_planner.py:171-176, Adam = torch.optim.Adam single-tensor path, multiplier ascent
 * constrained:66-73.  adam_step_size = lr / (1 - beta1^k), adam_bc2_sqrt = sqrt(1 - beta2^k), both formed by the
 * caller in double precision for the 1-based step count k, exactly as torch does; adam_omb1/2 = 1 - beta1/2
 * likewise rounded from double (fp32(1 - 0.9) != 1.0f - 0.9f). */
typedef struct nfopp_traj_hyper {
  float collision_weight;
  float angle_weight;
  float constraint_deltas_weight;
  float multipliers_lr;
  float collision_multipliers_lr;
  float boundary_weight;
  float collision_beta;
  float direction_delta_weight;
  float bounds[4];          /* xmin, xmax, ymin, ymax */
  float adam_beta2, adam_omb1, adam_omb2, adam_eps;
  float adam_step_size, adam_bc2_sqrt;
} nfopp_traj_hyper;

#define NFOPP_NUM_TERMS 8 /* per-trajectory loss terms written by nfopp_traj_update (see below) */

int nfopp_abi_version(void);
const char* nfopp_last_error(void);
/* number of visible HIP devices (0 when none / no driver); never fails */
int nfopp_device_count(void);
/* number of fp32 parameters of an ONF with this configuration (33161 for the shipped one), <0 on bad config */
int64_t nfopp_onf_param_count(const nfopp_onf_config* cfg);

/* ONF forward + input gradient at explicit points.  Replaces `ONF.forward` (nfop/onf_model.py:33-50,
 * nfop/angle_encoder.py:15-18) followed by autograd w.r.t. the input.
 *   points_dev [P, point_dim]  point_dim = 3 (x, y, theta) when angle_dim > 0, else 2
 *   out4_dev   [P, 4]          logit, dlogit/dx, dlogit/dy, dlogit/dtheta (0 for 2-D fields); all 4 P floats are written,
 *                              on every matrix path and at every P (the tiles of the last, partly filled chunk store no row
 *                              past P) */
int nfopp_onf_eval_points(const nfopp_onf_config* cfg, const float* params_dev, const float* points_dev,
                          int64_t n_points, float* out4_dev, void* stream);

/* Forward only (the backward half of the kernel is skipped): out4_dev [P, 4] = logit, 0, 0, 0.  Used where the
 * reference evaluates the field without gradients (nfop/nerf_opt_planner.py:98-99,122-125, plotting).  The three zeros of
 * every row are written too. */
int nfopp_onf_eval_logits(const nfopp_onf_config* cfg, const float* params_dev, const float* points_dev,
                          int64_t n_points, float* out4_dev, void* stream);

/* Fused collision-point sampling + ONF forward + input gradient along a batch of trajectories: the ONF part
 * of `trajectory_loss` (constrained:78-85 for D = 3, nfop/nerf_opt_planner.py:113-117,157-169 for D = 2).
 *   traj_dev [B, N, D]   interior waypoints;  sample j of trajectory b lies between waypoints j and j+1
 *   t_dev    [B, N-1]    t_mode 0: read (injected draws);  t_mode 1: drawn here with Philox4x32-10
 *                        (key = seed, counter = (global sample index, rng_offset)) and WRITTEN for the
 *                        update kernel (t_mode 0 never writes t_dev);  traj_index_offset = global index of
 *                        trajectory 0 (multi-GPU shards
 *                        draw the same numbers as a single-GPU run)
 *   out4_dev [B, N-1, 4] as nfopp_onf_eval_points
 *   active_dev [B] uint8 or NULL (ABI 4): early stop, the reference's `break` (scripts/run_bench_mr.py:121-126).
 *                        Trajectories with active == 0 are compacted OUT of the sample stream, so the kernel's
 *                        work is proportional to the live ones; their t / out4 rows are left untouched and the
 *                        rows of live trajectories are bit-identical to a launch without the mask.
 *   live_ws_dev [B + 1] int32 workspace for the live list (required with active_dev, else may be NULL).  Needs no
 *                        initialisation: the call writes the live count to [0] and the live indices behind it, reads no
 *                        other element and leaves the slots behind the last live index alone.  With every trajectory
 *                        retired nothing of t / out4 is written. */
int nfopp_traj_collision_eval(const nfopp_onf_config* cfg, const float* params_dev, const float* traj_dev,
                              int64_t batch, int32_t n_waypoints, int32_t dim, float* t_dev, int32_t t_mode,
                              uint64_t seed, uint64_t rng_offset, int64_t traj_index_offset, float* out4_dev,
                              const uint8_t* active_dev, int32_t* live_ws_dev, void* stream);

/* One `_optimize_trajectory` for every trajectory of the batch, given the ONF outputs at its samples:
 * loss terms + closed-form gradients (constrained:87-130, nerf:171-176), g <- H^-1 g (nerf:151), Adam
 * (nerf:154), multiplier ascent + clamp (constrained:66-73).  State arrays are updated IN PLACE.
 *   traj_dev [B,N,D], start_dev/goal_dev [B,D], lam_dev [B,N+1], cm_dev [B,N] (both NULL for D = 2),
 *   adam_m_dev/adam_v_dev [B,N,D], t_dev [B,N-1], onf_out4_dev [B,N-1,4]
 *   hinv_band_dev [2*half_width+1, N]: band of the reference's fp32 inverse Hessian (nerf:45-48), transposed so
 *       that entry [k][i] = Hinv[i][i + k - half_width] (0 outside the matrix)
 *   interior_lo/hi: waypoints i in [lo, hi) whose band column equals column lo BIT FOR BIT (the inverse of a
 *       tridiagonal Toeplitz matrix is Toeplitz away from the ends); their coefficients are broadcast from LDS.
 *       Pass lo = hi = 0 to disable.
 *   terms_dev [B, 8] or NULL: total, distance, sum softplus, sum lam*c, sum c^2, boundary, sum cm*tanh, sum relu(d)^2
 *   active_dev [B] uint8 or NULL: trajectories with 0 are left untouched (early stop, see nfopp_path_select_best): their
 *       rows of traj, lam, cm, adam_m, adam_v AND of terms_dev keep their bytes; the 8 terms of every live row are written */
int nfopp_traj_update(const nfopp_traj_hyper* hp, int64_t batch, int32_t n_waypoints, int32_t dim,
                      float* traj_dev, const float* start_dev, const float* goal_dev, float* lam_dev,
                      float* cm_dev, float* adam_m_dev, float* adam_v_dev, const float* t_dev,
                      const float* onf_out4_dev, const float* hinv_band_dev, int32_t half_width,
                      int32_t interior_lo, int32_t interior_hi, float* terms_dev, const uint8_t* active_dev,
                      void* stream);

/* Arc-length reparametrisation (constrained:132-171 for D = 3 incl. multipliers; nerf:224-244 for D = 2).
 *   u_dev [N] = torch.linspace(0, 1, N+2)[1:-1] (formed by the caller so its rounding is the reference's)
 *   active_dev [B] uint8 or NULL: the rows of traj, lam and cm of trajectories with 0 keep their bytes */
int nfopp_reparametrize(int64_t batch, int32_t n_waypoints, int32_t dim, float* traj_dev,
                        const float* start_dev, const float* goal_dev, float* lam_dev, float* cm_dev,
                        const float* u_dev, const uint8_t* active_dev, void* stream);

/* Start / goal update of a batch in one launch: the receding-horizon tick of nfop/ros/goal_planner_adapter.py:44-53 calls
 * update_start_point every 100 ms.  Replaces, per trajectory, the op sequence of constrained:178-194 (D = 3) / nerf:202-218
 * (D = 2):  delta = torch.sum((traj[:, :2] - point[:, :2]) ** 2, dim=1);  min_index = torch.argmin(delta)
 *           D = 3 only: min_index = min(min_index + 1, N)          (the reference's own asymmetry between its two classes)
 *           which = 1: traj[min_index:] = goal = point;   which = 0: traj[:min_index] = start = point
 *           reparametrize_trajectory()                             (bit for bit what nfopp_reparametrize computes)
 * delta is rounded op by op (no fma) and argmin keeps torch's order: first minimal index, a NaN counts as smallest.
 *   new_points_dev [B, dim]; the rows are also written to start_dev (which = 0) or goal_dev (which = 1)
 *   moved_dev [B] uint8 or NULL (= all): rows with 0 keep traj, lam, cm and their endpoint bit for bit.  A row is updated
 *       whether or not an early-stop `active` mask has retired it.
 *   lam_dev / cm_dev: required for dim 3 (interpolated, never overwritten), ignored for dim 2
 *   min_index_out_dev [B] int32 or NULL: the cut index min_index above (rows with moved = 0 are not written)
 * LDS budget and the limit on N are those of nfopp_reparametrize.  Added within ABI 6 (no existing entry changed). */
int nfopp_update_endpoints(int64_t batch, int32_t n_waypoints, int32_t dim, int32_t which,
                           const float* new_points_dev, const uint8_t* moved_dev, float* traj_dev, float* start_dev,
                           float* goal_dev, float* lam_dev, float* cm_dev, const float* u_dev,
                           int32_t* min_index_out_dev, void* stream);

/* n planner steps of a FROZEN-field batch from one call (ABI 6): the step loops that drive the reference's hot path --
 * nfop/ros/goal_planner_adapter.py:50-52 (`while time < timeout: planner.step()`), scripts/run_planner.py:76-77,
 * scripts/run_bench_mr.py:109-132 -- without a host round trip per step.  Per step k = 0 .. n_steps-1, on `stream`:
 *   nfopp_traj_collision_eval (draws: t_mode 1 = Philox word rng_offset + k; t_mode 0 = row k of t_steps_dev [n_steps, B, N-1])
 *   nfopp_traj_update with the Adam scalars of step adam_steps_done + k + 1, formed here in double as torch.optim.Adam forms
 *     them (step_size = lr / (1 - beta1^k), bc2_sqrt = sqrt(1 - beta2^k); hp's two fields are ignored)
 *   nfopp_reparametrize when (step_count + k) % reparam_freq == 0           (nfop/nerf_opt_planner.py:60-71)
 * Same kernels and arguments as n single-step sequences: results are bit-identical to them.  terms_dev [B, 8] (or NULL)
 * receives the loss terms of the LAST step (rows of retired trajectories are left alone, as are their rows of t_dev and
 * onf_out4_dev; t_mode 0 does not touch t_dev at all).  The caller advances its own counters by n_steps afterwards.  Nothing
 * synchronises.  Not for steps with ONF learning: the reference's fit needs the host checker between steps. */
typedef struct nfopp_traj_buffers {
  float* traj_dev;             /* [B, N, D] */
  const float* start_dev;      /* [B, D] */
  const float* goal_dev;       /* [B, D] */
  float* lam_dev;              /* [B, N+1], NULL for D = 2 */
  float* cm_dev;               /* [B, N],   NULL for D = 2 */
  float* adam_m_dev;           /* [B, N, D] */
  float* adam_v_dev;           /* [B, N, D] */
  float* t_dev;                /* [B, N-1] scratch for t_mode 1 (may be NULL for t_mode 0) */
  float* onf_out4_dev;         /* [B, N-1, 4] scratch */
  const float* hinv_band_dev;  /* [2*half_width+1, N] */
  const float* u_dev;          /* [N] = torch.linspace(0, 1, N+2)[1:-1] */
  const uint8_t* active_dev;   /* [B] or NULL */
  int32_t* live_ws_dev;        /* [B+1], required with active_dev */
  int64_t batch;
  int32_t n_waypoints, dim, half_width, interior_lo, interior_hi;
} nfopp_traj_buffers;

typedef struct nfopp_step_schedule {
  double adam_lr, adam_beta1, adam_beta2; /* the trajectory optimiser's Adam group (eps, 1-beta in nfopp_traj_hyper) */
  int64_t adam_steps_done;                /* Adam steps taken before this call */
  int64_t step_count;                     /* planner step counter before this call (reparametrisation schedule) */
  int64_t traj_index_offset;              /* global index of trajectory 0 (Philox counter) */
  uint64_t seed, rng_offset;              /* t_mode 1: Philox key, word of the first step */
  int32_t reparam_freq;                   /* >= 1 */
  int32_t t_mode;                         /* 0 = injected draws (t_steps_dev), 1 = in-kernel Philox */
} nfopp_step_schedule;

int nfopp_traj_steps(const nfopp_onf_config* cfg, const float* params_dev, const nfopp_traj_hyper* hp,
                     const nfopp_traj_buffers* buf, const nfopp_step_schedule* sched, int32_t n_steps,
                     const float* t_steps_dev, float* terms_dev, void* stream);

/* The distance-field collision model (csrc/sdf_field.hip): the obstacle cost of CHOMP / GPMP2 as a second
 * producer of the [.., 4] rows nfopp_traj_update reads, for users who hold an occupancy grid and no fitted ONF.
 *   sd_dev [rows, cols]: signed distance in metres at the cell centres, free positive, wall negative, every value finite
 *     (OccupancyGrid.signed_distance_field).  The centre of cell (j, i) lies at (x0 + (i + 0.5) / inv_res, y0 + (j + 0.5) / inv_res).
 *   The robot is n_discs discs (centre ox, oy in the body frame, radius r).  Per disc, all in fp32 and every operation
 *   rounded on its own (no fused multiply-add):
 *     cx = (x + ox c) - oy s,  cy = (y + ox s) + oy c,  (c, s) = (cos theta, sin theta); a disc with ox = oy = 0 sits at (x, y)
 *       exactly, and a robot of such discs alone evaluates no sine: (c, s) = (1, 0) stands in
 *     u = (cx - x0) inv_res - 0.5;  in_x = 0 < u < cols - 1;  u clamped to [0, cols - 1];  i = min((int)floor(u), cols - 2);
 *       fu = u - i;  v, in_y, j, fv likewise with y0 and rows
 *     a = sd[j][i+1] - sd[j][i];  b = sd[j+1][i+1] - sd[j+1][i];  top = sd[j][i] + fu a;  bot = sd[j+1][i] + fu b
 *     d = top + fv (bot - top);  gx = in_x ? (a + fv (b - a)) inv_res : 0;  gy = in_y ? (bot - top) inv_res : 0
 *     pen = (r + margin) - d
 *   The disc that counts is the first one with the largest pen (strict >).  The row is
 *     gain pen,  gain (-gx),  gain (-gy),  gain ((-gx) ((-ox) s - oy c) + (-gy) (ox c - oy s))   (0 for poses of 2 components)
 *   A pose outside the image sees the clamped border value, with a zero gradient component along each clamped axis.  A pose
 *   with a non-finite component gives four NaNs and reads nothing of sd_dev. */
typedef struct nfopp_sdf_field {
  const float* sd_dev;          /* [rows, cols] */
  int32_t rows, cols;           /* both >= 2 */
  float x0, y0, inv_res;        /* float(boundaries[0]), float(boundaries[2]), float(1.0 / resolution): each rounded once from double */
  int32_t n_discs;              /* 1..8 */
  float disc[8][3];             /* body-frame centre (ox, oy) and radius */
  float margin, gain;           /* metres, logit per metre */
} nfopp_sdf_field;

/* The row above at explicit poses.
 *   points_dev [P, point_dim], point_dim 3 (x, y, theta) or 2 (x, y: one disc with a zero offset only)
 *   out4_dev   [P, 4], 16-byte aligned: all 4 P floats are written and nothing else
 * Added within ABI 6 (no existing entry changed), as are the two entries below. */
int nfopp_sdf_eval_points(const nfopp_sdf_field* field, const float* points_dev, int64_t n, int32_t point_dim,
                          float* out4_dev, void* stream);

/* The row above at the collision samples of a batch of trajectories: nfopp_traj_collision_eval with the distance field in
 * the ONF's place.  The sample between waypoints j and j+1, the draw t, its Philox counter and traj_index_offset are that
 * entry's (one device function forms the sample for both).
 *   traj_dev [B, N, dim];  t_dev [B, N-1]: t_mode 0 reads it and never writes it, t_mode 1 writes the draw of every live row
 *   out4_dev [B, N-1, 4], 16-byte aligned: the 4 floats of every live row are written
 *   active_dev [B] uint8 or NULL: the t and out4 rows of trajectories with 0 keep their bytes; the rows of the others are
 *     those of a launch without the mask.  No live-list workspace: one lane per sample, and a retired lane returns. */
int nfopp_traj_sdf_collision_eval(const nfopp_sdf_field* field, const float* traj_dev, int64_t batch, int32_t n_waypoints,
                                  int32_t dim, float* t_dev, int32_t t_mode, uint64_t seed, uint64_t rng_offset,
                                  int64_t traj_index_offset, float* out4_dev, const uint8_t* active_dev, void* stream);

/* nfopp_traj_steps with nfopp_traj_sdf_collision_eval as each step's first launch: the same loop (one function serves both
 * entries), the same Adam scalars, update and reparametrisation schedule, so n_steps here equal n_steps single-step sequences
 * bit for bit.  Writes what nfopp_traj_steps writes; buf->live_ws_dev is not used.  The field, the robot and the schedule are
 * checked before the first launch: a call refused for one of them has written nothing. */
int nfopp_traj_steps_sdf(const nfopp_sdf_field* field, const nfopp_traj_hyper* hp, const nfopp_traj_buffers* buf,
                         const nfopp_step_schedule* sched, int32_t n_steps, const float* t_steps_dev, float* terms_dev,
                         void* stream);

/* The heading-layered distance field (csrc/heading_field.hip): a third producer of the [.., 4] rows, for a robot
 * of any shape on an occupancy grid.  Slice k of the image is the signed distance of the occupancy the robot's footprint
 * leaves at the heading k * 2 pi / layers (nfopp.HeadingDistanceField.from_checker): how far the centre may move at that
 * heading before the checker says "collision".  A sample is one trilinear tap of the image; no sine or cosine is taken.
 *   sd_dev [layers, rows, cols]; the centre of cell (j, i) lies where nfopp_sdf_field puts it.
 *   All in fp32, every operation rounded on its own (no fused multiply-add); floorf and fmodf are exact:
 *     u, in_x, i, fu and v, in_y, j, fv from (x, y) itself as in nfopp_sdf_field
 *     w = theta layers_per_rad;  kf = floorf(w);  fw = w - kf
 *     r = fmodf(kf, (float)layers) (|r| < layers);  k0 = (int)r, plus layers if negative;  k1 = k0 + 1, or 0 when that is layers
 *     per slice l in {k0, k1}, s.. its four taps at (j, i):
 *       a = s01 - s00;  b = s11 - s10;  top = s00 + fu a;  bot = s10 + fu b
 *       d_l = top + fv (bot - top);  gx_l = (a + fv (b - a)) inv_res;  gy_l = (bot - top) inv_res
 *     d = d0 + fw (d1 - d0);  gx = in_x ? gx0 + fw (gx1 - gx0) : 0;  gy = in_y ? gy0 + fw (gy1 - gy0) : 0
 *     gth = (d1 - d0) layers_per_rad;  pen = margin - d
 *   The row is  gain pen,  gain (-gx),  gain (-gy),  gain (-gth).
 *   A pose outside the image sees the clamped border value, with a zero gradient component along each clamped axis.  A pose
 *   with a non-finite component, or with a heading so large that w is not finite, gives four NaNs and reads nothing of sd_dev.
 *   Between two slices the distance is interpolated: a long robot at a heading between them is judged by its neighbours
 *   (choose layers and margin for the robot's length). */
typedef struct nfopp_heading_field {
  const float* sd_dev;        /* [layers, rows, cols]: signed distance in metres of heading slice k = heading k * 2 pi / layers,
                                 free positive, blocked negative, every value finite */
  int32_t layers, rows, cols; /* layers 2..64, rows >= 2, cols >= 2; layers * rows * cols < 2^31 */
  float x0, y0, inv_res;      /* as nfopp_sdf_field */
  float layers_per_rad;       /* float(layers / (2 pi)): formed in double, rounded once */
  float margin, gain;         /* metres, logit per metre */
} nfopp_heading_field;

/* The row above at explicit poses.
 *   points_dev [P, 3] (x, y, theta): a robot without a heading is nfopp_sdf_field's case
 *   out4_dev   [P, 4], 16-byte aligned: all 4 P floats are written and nothing else
 * Added within ABI 6 (no existing entry changed), as are the two entries below.  All three refuse, before any launch and
 * without writing anything: a null field or image, layers outside 2..64, rows or cols below 2, an image beyond a 32-bit index,
 * a non-finite x0, y0, inv_res, layers_per_rad, margin or gain, null pointers with a positive count, an unaligned out4_dev,
 * t_mode outside {0, 1}, fewer than 2 waypoints and counts beyond one launch. */
int nfopp_hdf_eval_points(const nfopp_heading_field* field, const float* points_dev, int64_t n, float* out4_dev, void* stream);

/* The row above at the collision samples of a batch of SE(2) trajectories: nfopp_traj_sdf_collision_eval with the layered
 * field in the disc field's place.  Sample, draw, Philox counter, t_mode, active_dev and traj_index_offset are that entry's
 * (one device function forms the sample for all collision models).
 *   traj_dev [B, N, 3];  t_dev [B, N-1];  out4_dev [B, N-1, 4], 16-byte aligned;  active_dev [B] uint8 or NULL */
int nfopp_traj_hdf_collision_eval(const nfopp_heading_field* field, const float* traj_dev, int64_t batch, int32_t n_waypoints,
                                  float* t_dev, int32_t t_mode, uint64_t seed, uint64_t rng_offset, int64_t traj_index_offset,
                                  float* out4_dev, const uint8_t* active_dev, void* stream);

/* nfopp_traj_steps with nfopp_traj_hdf_collision_eval as each step's first launch (the one loop serves all three entries): n_steps
 * here equal n_steps single-step sequences bit for bit.  buf->dim must be 3; buf->live_ws_dev is not used. */
int nfopp_traj_steps_hdf(const nfopp_heading_field* field, const nfopp_traj_hyper* hp, const nfopp_traj_buffers* buf,
                         const nfopp_step_schedule* sched, int32_t n_steps, const float* t_steps_dev, float* terms_dev,
                         void* stream);

/* The moving-obstacle collision term (csrc/track_field.hip): a pass over the [.., 4] rows one of the three
 * collision entries has written.  Where a moving obstacle penetrates the robot deeper than the row says, the row is replaced by
 * the moving obstacle's: "the deepest disc gives the row" of nfopp_sdf_field, extended over time.
 *   Tracks: tracks_dev [m, k, stride >= 2], x and y first in a row, the positions of m obstacles at t_n = t0 + n dt -- the
 *     tensors nfopp_track_conflicts and nfopp_path_time_sample work on, consumed as they are.  Obstacle i is a disc of radius
 *     radius_dev[i] (NULL: 0).  A track is linear in time between two instants, stands at its first position before t0 and at
 *     its last after t_{k-1}.
 *   Time of a sample: wp_time [B, N] says when the robot is at waypoint i.  The collision sample j is
 *     traj[j+1] + t (traj[j] - traj[j+1]) (it runs backwards in the index), and its time is formed the same way:
 *     tau = T[j+1] + t (T[j] - T[j+1]), one subtraction, one product, one sum.  Times are data: the term has no gradient in tau.
 *   The robot is n_discs discs as in nfopp_sdf_field: the same centres cx, cy, the same rule that a robot of centred discs
 *     takes no sine; poses of 2 components: one centred disc.
 *   All in fp32, every operation rounded on its own (no fused multiply-add):
 *     w = (tau - t0) inv_dt;  w = w > 0 ? w : 0;  w = w < k - 1 ? w : k - 1  (a NaN goes to 0)
 *     n = max(min((int)floor(w), k - 2), 0);  n1 = min(n + 1, k - 1);  s = w - n      (k = 1: n = n1 = 0, s = 0)
 *     per disc d (outer loop) and track i (inner loop), p = tracks[i]:
 *       qx = p[n].x + s (p[n1].x - p[n].x), qy likewise;  ex = cx - qx;  ey = cy - qy
 *       dist = sqrt(ex ex + ey ey), correctly rounded (sqrtf as hipcc compiles it by default; it equals numpy's sqrt on float32)
 *       pen = ((r_d + radius[i]) + margin) - dist
 *     The candidate that counts is the first one with the largest pen (strict >); a candidate whose pen is a NaN (a track with
 *     a coordinate that is not finite) never counts.  For it alone: nx = ex / dist, ny = ey / dist (IEEE division), both 0 when
 *     dist == 0.  The track row is
 *       gain pen,  gain (-nx),  gain (-ny),  gain ((-nx) lx + (-ny) ly)      (0 for poses of 2 components)
 *     with lx = (-ox) s - oy c, ly = ox c - oy s of that disc, as in nfopp_sdf_field.
 *   Combination: the track row replaces the 16 bytes of the row iff track logit > row logit (strict; so a row whose logit is a
 *     NaN or +inf stays, and so does every row when no candidate counts).  Otherwise the row is not written.  A sample with a
 *     pose component or a time that is not finite reads no track and keeps its row. */
typedef struct nfopp_track_field {
  const float* tracks_dev;      /* [m, k, stride]; may be NULL when m == 0 */
  const float* radius_dev;      /* [m] or NULL (= 0) */
  int32_t m, k, stride;         /* m >= 0, k >= 1, stride >= 2; m * k * stride < 2^31 */
  float t0, inv_dt;             /* float(t0), float(1.0 / dt): each rounded once from double; inv_dt > 0 */
  int32_t n_discs;              /* 1..8 */
  float disc[8][3];             /* body-frame centre (ox, oy) and radius */
  float margin, gain;           /* metres, logit per metre */
} nfopp_track_field;

/* The overlay at explicit poses and times.
 *   points_dev [n, dim], dim 3 (x, y, theta) or 2 (x, y: one disc with a zero offset only);  times_dev [n]
 *   out4_dev [n, 4], 16-byte aligned, in-out: read as the rows to beat; only the 16 bytes of a row that a track row beats are
 *     written, nothing else.  (Rows of logit -inf give back the pure track row.)
 * m == 0 is a set of no obstacles: the call returns without a launch.  Added within ABI 6 (no existing entry changed), as are
 * the two entries below.  All three refuse, before any launch and without writing anything: a null field, null tracks with
 * m > 0, null times, m < 0, k < 1, stride < 2, n_discs outside 1..8, an offset disc or several discs with dim 2, a non-finite
 * t0, inv_dt, margin or gain, inv_dt <= 0, m * k * stride beyond a 32-bit index, null pointers with a positive count, an
 * unaligned out4_dev, fewer than 2 waypoints and counts beyond one launch. */
int nfopp_track_field_eval_points(const nfopp_track_field* field, const float* points_dev, const float* times_dev, int64_t n,
                                  int32_t dim, float* out4_dev, void* stream);

/* The overlay at the collision samples of a batch of trajectories, after any of the three collision entries.
 *   traj_dev [B, N, dim], wp_time_dev [B, N]
 *   t_dev [B, N-1]: read only -- the draws the collision entry has just used (or written, in its t_mode 1)
 *   out4_dev [B, N-1, 4], 16-byte aligned, in-out as above
 *   active_dev [B] uint8 or NULL: the rows of trajectories with 0 are neither read nor written */
int nfopp_traj_track_overlay(const nfopp_track_field* field, const float* traj_dev, const float* wp_time_dev, int64_t batch,
                             int32_t n_waypoints, int32_t dim, const float* t_dev, float* out4_dev, const uint8_t* active_dev,
                             void* stream);

/* nfopp_traj_steps / _sdf / _hdf with moving obstacles: the one loop, with the collision entry of `kind` followed by
 * nfopp_traj_track_overlay as each step's collision term, so n_steps here equal n_steps sequences of collision entry,
 * overlay, update (and reparametrisation on its schedule) bit for bit.
 *   kind NFOPP_MODEL_ONF: model = const nfopp_onf_config*, params_dev its parameters;  NFOPP_MODEL_SDF: model = const
 *   nfopp_sdf_field*;  NFOPP_MODEL_HDF: model = const nfopp_heading_field* (buf->dim must be 3);  params_dev is ignored for both
 * Writes what nfopp_traj_steps writes.  An unknown kind, the track field, wp_time_dev and the schedule are checked before the
 * first launch: a call refused for one of them has written nothing. */
#define NFOPP_MODEL_ONF 0
#define NFOPP_MODEL_SDF 1
#define NFOPP_MODEL_HDF 2
int nfopp_traj_steps_moving(int32_t kind, const void* model, const float* params_dev, const nfopp_track_field* field,
                            const float* wp_time_dev, const nfopp_traj_hyper* hp, const nfopp_traj_buffers* buf,
                            const nfopp_step_schedule* sched, int32_t n_steps, const float* t_steps_dev, float* terms_dev,
                            void* stream);

/* ONF fitting step, gradient part: BCE-with-logits (mean over ALL samples of the job) and its gradient w.r.t.
 * every parameter incl. the angle frequencies (nfop/nerf_opt_planner.py:83-89).
 *   samples_dev [P, point_dim], labels_dev [P] (0/1), inv_count = 1 / (global sample count)
 *   grad_dev [n_params + 2]: flat gradient in parameter order, then sum of per-sample losses * inv_count, then P
 *   workspace: nfopp_onf_train_workspace_bytes(cfg, P) bytes of device scratch, exactly that many are enough for every P
 *     (the last, ragged chunk of samples reads and writes no row past P); it needs no initialisation
 *   All n_params + 2 floats of grad_dev are written (stored, not accumulated: the buffer need not be zeroed).
 * Reductions run in a fixed order (no float atomics): results are bitwise reproducible. */
size_t nfopp_onf_train_workspace_bytes(const nfopp_onf_config* cfg, int64_t n_samples);
int nfopp_onf_train_grad(const nfopp_onf_config* cfg, const float* params_dev, const float* samples_dev,
                         const float* labels_dev, int64_t n_samples, float inv_count, float* grad_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* Same, with an explicit implementation path: 0 = automatic (MFMA GEMM path from 2048 samples), 1 = per-sample
 * workgroups + thread-per-parameter reductions, 2 = MFMA forward/backward + split-K weight-gradient GEMMs. */
int nfopp_onf_train_grad_ex(const nfopp_onf_config* cfg, const float* params_dev, const float* samples_dev,
                            const float* labels_dev, int64_t n_samples, float inv_count, float* grad_dev,
                            void* workspace_dev, size_t workspace_bytes, int32_t path, void* stream);

/* ---- continuous ONF learning over a batch: ground truth and sample generation on the device --------------------
 * Ground-truth checkers (labels_dev[p] = 1.0 in collision, 0.0 free); bounds4 (host, may be NULL) = xmin,xmax,ymin,ymax
 * of nfop/collision_checker/collision_checker.py:12-19.  Every one of labels_dev[0 .. n) is written, by all five entries.
 *   circle:    any |pose.xy - obstacle| < radius                 nfop/collision_checker/circle_collision_checker.py:11-14
 *   rectangle: any obstacle inside box4 = (x0,x1,y0,y1) in the robot frame   .../rectangle_collision_checker.py:11-26
 *   grid:      uint8 occupancy image, cell = int((x - origin - cell/2)/cell) in float64 like the reference's numpy
 *              (geometry scalars are doubles since ABI 4); outside the image = collision
 *              (MapCollisionChecker, notebooks/onf_planner_image_map.ipynb cell 2; labels pinned by tests/golden/g16) */
int nfopp_check_collision_circle(const float* poses_dev, int64_t n, int32_t pose_dim, const float* obstacles_dev,
                                 int32_t n_obstacles, float radius, const float* bounds4, float* labels_dev,
                                 void* stream);
/* The circle checker with a uniform cell index over the obstacle points (same labels, far fewer distance tests):
 * obstacles_sorted_dev [n_obstacles, 2] sorted by cell (row-major cells of cell_size >= radius, origin cell_x0 / cell_y0),
 * cell_start_dev [cells_x * cells_y + 1] = first point of each cell. */
int nfopp_check_collision_circle_cells(const float* poses_dev, int64_t n, int32_t pose_dim,
                                       const float* obstacles_sorted_dev, int32_t n_obstacles,
                                       const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y, float cell_x0,
                                       float cell_y0, float cell_size, float radius, const float* bounds4,
                                       float* labels_dev, void* stream);
int nfopp_check_collision_rectangle(const float* poses_dev, int64_t n, const float* obstacles_dev, int32_t n_obstacles,
                                    const float* box4, const float* bounds4, float* labels_dev, void* stream);
/* The rectangle checker over the same cell index (additive under ABI 6): `reach` = the largest distance from the robot
 * origin to a corner of box4 (the box need not contain the origin), formed by the caller; cell_size >= reach, so every
 * point inside the box lies in the 3 x 3 cells around the pose's cell.  The per-point predicate is the one function the
 * brute-force kernel calls: identical labels. */
int nfopp_check_collision_rectangle_cells(const float* poses_dev, int64_t n, const float* obstacles_sorted_dev,
                                          int32_t n_obstacles, const int32_t* cell_start_dev, int32_t cells_x,
                                          int32_t cells_y, float cell_x0, float cell_y0, float cell_size,
                                          const float* box4, float reach, const float* bounds4, float* labels_dev,
                                          void* stream);
int nfopp_check_collision_grid(const float* poses_dev, int64_t n, int32_t pose_dim, const uint8_t* grid_dev,
                               int32_t rows, int32_t cols, double origin_x, double origin_y, double cell_size,
                               float* labels_dev, void* stream);

/* Training-pose generation for every trajectory of a batch (nfop/nerf_opt_planner.py:101-120,135-141,
 * constrained:57-61,173-176).  Per trajectory: N-1 interpolated poses of the PREVIOUS trajectory -> "course" copies
 * (sigma course/angle) written to samples[b][0..N-2], "fine" copies appended to the candidate list behind the
 * retained pool (pool_count = 0 on the first step, pool_cap afterwards), n_field uniform field poses written to
 * samples[b][N-1+pool_cap ...].  Layouts: cand [B, pool_cap+N-1, D], samples [B, N-1+pool_cap+n_field, D].
 * Written: cand / cand_age slots [0, pool_count + N - 1) of every trajectory (with pool_count = 0 the last pool_cap slots are
 * left alone), samples slots [0, N - 1) and [N - 1 + pool_cap, end); the pool_cap slots between them belong to
 * nfopp_resample_pool and are left alone.  pool_dev / pool_age_dev are only read (not at all with pool_count = 0).
 * Draws: Philox4x32-10 keyed by seed, counter (index, stream, trajectory, rng_offset). */
int nfopp_sample_candidates(const float* prev_traj_dev, int64_t batch, int32_t n_waypoints, int32_t dim,
                            int32_t pool_cap, int32_t pool_count, int32_t n_field, float course_sigma, float fine_sigma,
                            float angle_sigma, const float* bounds4, uint64_t seed, uint64_t rng_offset,
                            int64_t traj_index_offset, const float* pool_dev, const float* pool_age_dev,
                            float* cand_dev, float* cand_age_dev, float* samples_dev, void* stream);

/* Retained-pool resampling (nfop/nerf_opt_planner.py:122-133): weights sigmoid(logit)*exp(-0.03 age)+1e-6, pool_cap
 * candidates kept WITHOUT replacement with probability proportional to the weights (exponential race), ages + 1.
 * The first n_candidates of cand_stride (= pool_cap + N - 1) candidate slots per trajectory are valid;
 * onf_out4_dev [B, cand_stride, 4] = nfopp_onf_eval_points on cand_dev.  The new pool is also written to
 * samples[b][sample_offset ...] (sample_stride = poses per trajectory in the samples buffer): all of pool_dev and
 * pool_age_dev is written, of samples_dev the slots [sample_offset, sample_offset + pool_cap) of every trajectory and no
 * other. */
int nfopp_resample_pool(int64_t batch, int32_t n_candidates, int32_t cand_stride, int32_t pool_cap, int32_t dim,
                        int32_t sample_stride,
                        int32_t sample_offset, uint64_t seed, uint64_t rng_offset, int64_t traj_index_offset,
                        const float* cand_dev, const float* cand_age_dev, const float* onf_out4_dev, float* pool_dev,
                        float* pool_age_dev, float* samples_dev, void* stream);

/* ---- path evaluation (the step after the planner step: scripts/run_bench_mr.py:109-132) ---------------------------
 * nfopp_path_interpolate: densifies start -> waypoints -> goal with `sub` poses per segment (theta along the wrapped
 *   difference) into poses_dev [B, (N+1)*sub + 1, D] and writes the xy polyline length to length_dev [B].
 * The caller labels the poses with a ground-truth checker (above), then
 * nfopp_path_select_best: collides[b] = any label set; a collision-free path shorter than best_length[b] replaces
 *   best_traj[b]; a collision-free path that does not improve clears active[b] (the reference's `break`); inactive
 *   trajectories are skipped by nfopp_traj_update / nfopp_reparametrize when active_dev is passed to them.
 * Written: every pose of poses_dev and every length_dev[b]; every collides_dev[b], for inactive trajectories too;
 *   best_traj[b] and best_length[b] only where the path replaces the best one; active[b] only where it is cleared. */
int nfopp_path_interpolate(const float* traj_dev, const float* start_dev, const float* goal_dev, int64_t batch,
                           int32_t n_waypoints, int32_t dim, int32_t sub, float* poses_dev, float* length_dev,
                           void* stream);
int nfopp_path_select_best(const float* labels_dev, const float* length_dev, const float* traj_dev, int64_t batch,
                           int32_t poses_per_path, int32_t n_waypoints, int32_t dim, float* best_traj_dev,
                           float* best_length_dev, uint8_t* collides_dev, uint8_t* active_dev, void* stream);
/* Matrix path of the fused ONF kernels (nfopp_onf_eval_points / _logits / nfopp_traj_collision_eval):
 *   1 (default) = bf16x3 split-precision MFMA: every fp32 operand is split EXACTLY into three bf16 levels and the six
 *       partial products above 2^-24 are accumulated in fp32 on the bf16 matrix pipe -- fp32-faithful (closer to float64
 *       than a sequential fp32 dot product).  Every launch of every ONF shape (F = 100 / 120 / 200 / 220) runs on 32x32x16 tiles
 *       (csrc/onf_x32_impl.h), in two workgroup shapes that are bit-identical per sample: results do not depend on the batch
 *       size or on how a batch is sharded; the training pass of the ONF fit too.
 *   0 = fp32 MFMA (v_mfma_f32_16x16x4_f32, csrc/onf_fused.hip).
 *   2 = bf16x3 split on the round-2 kernels (16x16x32 tiles, csrc/onf_split.hip) at every size: an independent implementation
 *       of path 1's arithmetic, kept as a cross-check.
 *   The environment variable NFOPP_MATRIX_PATH=fp32|0|1|2 selects the path at load time.  Process-wide.
 *   The split paths keep ONE scratch image per (device, stream) (pre-split weights, rebuilt from params_dev by a small
 *   kernel in front of every evaluation on the caller's stream), at most 16 per device: a 17th stream reuses the least
 *   recently used slot after a device synchronisation. */
int nfopp_set_matrix_path(int32_t path);
/* Content version of an ONF parameter buffer on the current device (ABI 5).  The split matrix paths evaluate the field from
 * a pre-split image of the weights that a small kernel rebuilds from params_dev in front of EVERY launch, because the
 * library cannot see whether the caller changed the buffer.  A caller who knows can vouch for it: register a non-zero
 * `version` that it changes whenever the buffer's contents change; while (buffer, version, configuration) stay the same,
 * launches on a stream reuse that stream's image and skip the rebuild (a frozen field: one launch less per planner step).
 * version = 0 withdraws the registration; nfopp_adam_step withdraws it for the buffer it updates.  Versions must be unique
 * per content over the life of the process (a counter), not per buffer. */
int nfopp_onf_params_version(const float* params_dev, uint64_t version);
int nfopp_get_matrix_path(void);
/* Sample count from which matrix path 1 launches its 512-thread workgroup (two waves per SIMD); a launch of fewer samples
 * runs the 256-thread one.  CUs x 256 on the current device.  Results do not depend on the shape; tests that want a launch
 * on either side of the edge read it here.  Added within ABI 6 (no existing entry changed). */
int64_t nfopp_onf_wide_launch_threshold(void);

/* ---- the steps either side of the planner step ----------------------------------------
 * nfopp_init_trajectories: TrajectoryInitializer.initialize_trajectory (+ initialize_angle and, with
 *   angles_with_direction != 0, initialize_angle_with_trajectory_direction; nfop/trajectory_initializer.py:12-45) for
 *   a batch: traj_dev [B, N, D] <- straight line start -> goal with torch.linspace's fp32 rounding, theta along the
 *   wrapped shortest rotation, optionally pulled towards the travel direction by a 0 -> 1 -> 0 ramp.  All B * N * D
 *   floats are written.
 * nfopp_path_postprocess: PathPostprocessor.process (nfop/ros/path_postprocessor.py:13-69) for a batch of fp32 paths
 *   path_dev [B, n_points, 3] (3 <= n_points <= 1026): near-duplicate filter, quadratic-spline re-sampling every
 *   distance_step metres over the chord-length parameter (float64), leading direction flip trimmed.  count_dev[b] =
 *   poses path b produces (may exceed max_out: only the first max_out are written to out_dev [B, max_out, 3] float64;
 *   call with max_out = 0 to size the buffer), -1 when fewer than 3 poses survive the filter or two surviving poses
 *   share a parameter value (a segment rounded away in the fp32 running length): the reference raises for both. */
int nfopp_init_trajectories(const float* start_dev, const float* goal_dev, int64_t batch, int32_t n_waypoints,
                            int32_t dim, int32_t angles_with_direction, float* traj_dev, void* stream);
int nfopp_path_postprocess(const float* path_dev, int64_t batch, int32_t n_points, float minimal_distance,
                           float distance_step, int32_t max_out, double* out_dev, int32_t* count_dev, void* stream);
/* torch.optim.Adam single-tensor update on a flat buffer (used for the ONF weights after the gradient
 * all-reduce): m.lerp_(g, 1-b1); v = b2 v + (1-b2) g^2; p -= step_size * m / (sqrt(v)/bc2_sqrt + eps).  param, m and v are
 * updated in place over [0, n) at every n (a grid-stride loop beyond 2048 * 256 elements); grad_dev is only read. */
int nfopp_adam_step(float* param_dev, const float* grad_dev, float* m_dev, float* v_dev, int64_t n, float beta2,
                    float omb1, float omb2, float eps, float step_size, float bc2_sqrt, void* stream);

/* ---- grid-search (A*) trajectory seeding for whole batches (csrc/grid_search.hip) ----------------------------------
 * Replaces AstarTrajectoryInitializer (nfop/astar/astar_trajectory_initializer.py:15-48) with the search of
 * nfop/astar/jps.py (jps=False: 8-connected, cost 1 / sqrt 2, no corner rule, :99-125) and reparametrize_path
 * (nfop/utils/math.py:57-65), additive under ABI 6.  Costs are integer pairs (a, b) = (straight, diagonal) moves.
 *
 * nfopp_grid_distance_fields (the search, jps.py:56-66 + the expansion loop): occupancy_dev uint8 [rows, cols]
 *   (non-zero = wall), goal_cells_dev int32 [G, 2] (row, col), callers pass each goal cell once.  fields_dev int32
 *   [G, rows, cols, 2] <- exact minimum cost (a, b) from every cell to goal g; the goal cell is forced free
 *   (astar_trajectory_initializer.py:40); walls, cells that cannot reach the goal and every cell of a goal outside the
 *   grid hold the sentinel (-1, -1).  The result is the unique fixed point of the relaxation: bit-identical from run to
 *   run.  Grids whose padded field fits 144 KiB of LDS with 16 + 16-bit counts (at most 65535 cells) are relaxed in
 *   LDS; larger ones, up to 2^21 cells, in `workspace` (nfopp_grid_fields_workspace_bytes, 0 for the LDS form) with
 *   32 + 32-bit counts, so no count can wrap.  The workspace needs no initialisation; all of fields_dev is written.
 * nfopp_grid_trace_paths (find_path's parent walk, jps.py:56-66): problem p starts in start_cells_dev[p], ends in
 *   goal_cells_dev[p] and reads field field_index_dev[p].  From the start cell it steps to the first neighbour, in
 *   the order N, W, S, E, NW, NE, SW, SE of (row, col), whose cost plus the move equals the current cost exactly.
 *   cells_dev int32 [B, max_len, 2] (row, col; first and last cell included), count_dev [B] = cells the path has
 *   (max_len = 0 sizes the buffer), status_dev [B]: 0 ok, 1 goal unreachable from the start, 2 start or goal cell
 *   outside the grid; cost_dev [B, 2] (may be null) = (a, b) of the path, (-1, -1) without one.  The start cell is not
 *   tested for occupancy, as in the reference.
 * nfopp_grid_seed_trajectories (initialize_trajectory :15-25 + reparametrize_path + initialize_angle): the polyline
 *   [start xy, cell centres (col * resolution + resolution / 2 + origin_x, row ... origin_y; fp32), goal xy] is
 *   re-sampled to n_waypoints + 2 points by the quadratic spline over the normalised chord length and the interior
 *   points are stored as fp32 in traj_dev [B, N, D]; headings as nfopp_init_trajectories writes them, the
 *   travel-direction pull along the seeded path.  A problem with status != 0 gets exactly nfopp_init_trajectories'
 *   trajectory.  Paths longer than 64 KiB of LDS allow need `workspace` (nfopp_grid_seed_workspace_bytes, else 0), which
 *   needs no initialisation. */
size_t nfopp_grid_fields_workspace_bytes(int32_t rows, int32_t cols, int64_t n_goals);
int nfopp_grid_distance_fields(const uint8_t* occupancy_dev, int32_t rows, int32_t cols, const int32_t* goal_cells_dev,
                               int64_t n_goals, int32_t* fields_dev, void* workspace_dev, size_t workspace_bytes,
                               void* stream);
int nfopp_grid_trace_paths(const int32_t* fields_dev, int64_t n_fields, int32_t rows, int32_t cols,
                           const int32_t* start_cells_dev, const int32_t* goal_cells_dev, const int32_t* field_index_dev,
                           int64_t batch, int32_t max_len, int32_t* cells_dev, int32_t* count_dev, int32_t* status_dev,
                           int32_t* cost_dev, void* stream);
size_t nfopp_grid_seed_workspace_bytes(int64_t batch, int32_t max_len);
int nfopp_grid_seed_trajectories(const int32_t* cells_dev, const int32_t* count_dev, const int32_t* status_dev,
                                 int64_t batch, int32_t max_len, const float* start_dev, const float* goal_dev,
                                 int32_t n_waypoints, int32_t dim, int32_t angles_with_direction, double origin_x,
                                 double origin_y, double resolution, float* traj_dev, void* workspace_dev,
                                 size_t workspace_bytes, void* stream);


/* ---- the obstacle update of the receding-horizon loop (csrc/obstacle_map.hip), additive under ABI 6 ------------------
 * What every sensor message does in the reference's deployment (nfop/ros/collision_checker_adapter.py:17-27,
 * nfop/ros/map_adapter.py): occupancy grid -> point cloud -> the checker that labels the ONF's training poses.
 *
 * nfopp_grid_to_points: GridMap.as_point_cloud (nfop/ros/grid_map.py:14-20) and, with is_int8 != 0, the unpacking of
 *   from_ros_occupancy_grid (:31-40).  grid_dev [rows, cols] is fp32 (occupied: v > threshold, compared in fp32) or the
 *   raw int8 ROS image (value fp32(v < 0 ? 0 : v) / 100.0f, then the same comparison); at most 2^24 cells.  The occupied
 *   cells leave in row-major order (np.nonzero's).  Cell (row, col) -> p = (col, row) * resolution + resolution / 2,
 *   then the origin pose: (x c - y s + origin_x, x s + y c + origin_y), all in float64 with every operation rounded on
 *   its own; origin_cos / origin_sin are the caller's np.cos / np.sin of the origin angle (no device libm result enters
 *   the output).  points_dev [max_points, 2] <- fp32 rounding of the float64 points (what the checkers read),
 *   points64_dev (may be null) <- the float64 points, count_dev <- occupied cells (may exceed max_points: only the first
 *   max_points are written; call with max_points = 0 to size the buffer).  Compaction: chunk counts by ballot +
 *   popcount, a fixed-order exclusive scan, the predicate again with rank = offset + position in the chunk.
 * nfopp_build_cell_index: obstacles_sorted_dev [n, 2] <- obstacles_dev stably sorted by cell, cell_start_dev
 *   [cells_x * cells_y + 1] <- first sorted point of each cell, bit for bit np.argsort(cell, kind="stable") and
 *   np.searchsorted(cell[order], arange(cells + 1)).  cell = cy * cells_x + cx with cx = floorf((x - cell_x0) /
 *   cell_size) in fp32 clamped to [0, cells_x - 1] (cy alike): CellIndex::cell of csrc/point_cloud.h, the one function
 *   the *_cells check kernels and the nearest-obstacle search form a pose's cell with.
 *   cells_x * cells_y <= 65536: an LSD radix sort over the 16-bit cell id in two 8-bit passes, per-wave digit
 *   histograms in LDS, fixed-order scans, no atomics.  Points outside the index region are clamped into its border
 *   cells, and the 3 x 3 search of the check kernels stays exhaustive: clamping to an interval is monotone and
 *   non-expansive, so a point whose true cell is within one cell of a pose's true cell (in x and in y) is still within
 *   one after both are clamped.  n_obstacles = 0 is valid: cell_start_dev <- zeros, nothing else is touched.
 *   workspace: nfopp_cell_index_workspace_bytes(n_obstacles) bytes of device scratch; it needs no initialisation. */
int nfopp_grid_to_points(const void* grid_dev, int32_t is_int8, int32_t rows, int32_t cols, float threshold,
                         double resolution, double origin_x, double origin_y, double origin_cos, double origin_sin,
                         int32_t max_points, float* points_dev, double* points64_dev, int32_t* count_dev, void* stream);
size_t nfopp_cell_index_workspace_bytes(int32_t n_obstacles);
int nfopp_build_cell_index(const float* obstacles_dev, int32_t n_obstacles, float cell_x0, float cell_y0, float cell_size,
                           int32_t cells_x, int32_t cells_y, float* obstacles_sorted_dev, int32_t* cell_start_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- nearest-obstacle clearance and per-path statistics (csrc/clearance.hip), additive under ABI 6 -------------------
 * What a user who picks among the paths of a batch asks beside `collides` and `length`.  The batch axis is this library's
 * own and so are these definitions (the reference reports a length; bench-mr's metric code is not part of it).
 *
 * nfopp_nearest_obstacle / nfopp_nearest_obstacle_cells: dist_dev[p] <- the minimum over ALL obstacle points k of d(p, k),
 *   index_dev[p] (may be null) <- the smallest k attaining it, an index into the obstacle array passed in (the sorted one
 *   for _cells).  box4 is a host pointer, as in the checkers:
 *     box4 = NULL, disc robot: dx = ox - x, dy = oy - y, d = sqrtf(fmaf(dx, dx, dy * dy)) -- the argument
 *       nfopp_check_collision_circle compares with the radius, through the one function both call.  sqrtf and `<` are
 *       monotone, so dist < radius IS that checker's obstacle term for every pose, bit for bit.
 *     box4 = (x0, x1, y0, y1), box robot, pose_dim must be 3: (rx, ry) as nfopp_check_collision_rectangle forms them
 *       (the same function), ex = max(x0 - rx, rx - x1, 0), ey alike, d = sqrtf(fmaf(ex, ex, ey * ey)): the distance from
 *       the obstacle point to the CLOSED box, 0 inside it.  A point the rectangle checker accepts has d == 0, and d > 0
 *       implies that the checker's obstacle term is false; a point exactly on the rim has d == 0 without being a collision.
 *   n_obstacles = 0: every pose gets +inf and -1.  A pose with a non-finite component gets +inf and -1, and so does a
 *   pose so far away that every fp32 distance overflows.  n = 0 is a no-op.
 *   nfopp_nearest_obstacle tests all pairs with the points staged in LDS: for small clouds, and the independent
 *   cross-check.  nfopp_nearest_obstacle_cells takes the index of nfopp_build_cell_index (any cell size: there is no
 *   "at least the reach" condition here) and searches outward from the pose's clamped cell in rings of growing Chebyshev
 *   radius r, one thread per pose, keeping the lexicographic minimum of (d, k).  It stops after ring r when the visited
 *   rectangle of cells has reached the index's border on all four sides, or when
 *       (r - 1/16) * cell_size * (1 - 2^-18) - reach  >  best distance so far        (strictly: ties go to the smaller k)
 *   with reach = 0 for the disc and the largest corner distance of the box, formed inside the call, otherwise.  The left
 *   side is a lower bound on the computed distance of every unvisited point: a side of the visited rectangle that lies on
 *   the border has nothing beyond it, because the border cells hold every point clamped into them; on the other sides a
 *   point in an unvisited column (row) differs from the pose by more than r - 2.1 * 2^-24 * 2^17 cells, the fp32 rounding
 *   of the two cell numbers, however far outside the region the pose is; the box is contained in the disc of radius reach
 *   about the robot's origin; 2^-18 covers the rounding of the distance itself (csrc/clearance.hip has the full argument).
 *   At most max(cells_x, cells_y) rings, whatever the pose holds.  No atomics; both entries return the same bits, run
 *   after run.
 * nfopp_nearest_obstacle_cells_probe: the measurements behind the work distribution (tools/clearance_timing.py).
 *   what = 0: the same search with one wave per group of 4 poses, the lanes sharing each run of points -- the same bits,
 *   5 % slower at the checkers' cell sizes, kept as a cross-check.  what = 1: index_dev[p] <- the
 *   rings pose p's search takes, dist_dev untouched.
 *
 * nfopp_path_stats: stats_dev [B, NFOPP_NUM_PATH_STATS] float64, one workgroup per path, for the polyline start,
 *   waypoints, goal (N + 2 points p_0 .. p_{N+1}, read as fp32, widened), segments e_i = p_{i+1} - p_i with
 *   n_i = sqrt(ex * ex + ey * ey).  Everything in float64 with every operation rounded on its own; sums in a fixed order
 *   (strided partial sums, a tree inside each wave, then the waves in order), extrema with the first index attaining them.
 *     0 NFOPP_PATH_STAT_LENGTH         sum of n_i
 *     1 NFOPP_PATH_STAT_MAX_CURVATURE  max over interior vertices i = 1..N of the Menger curvature
 *                                      (2 * |ex0 * ey1 - ey0 * ex1|) / ((n0 * n1) * |p_{i+1} - p_{i-1}|), e0 = e_{i-1}, e1 = e_i;
 *                                      a vertex with a zero factor in the denominator is no candidate; 0 without candidates
 *     2 NFOPP_PATH_STAT_CURVATURE_AT   full-trajectory index i of the first vertex attaining it, -1 without candidates
 *     3 NFOPP_PATH_STAT_CUSPS          vertices with n0 > 0, n1 > 0 and ex0 * ex1 + ey0 * ey1 < cos_cusp * (n0 * n1)
 *     4 NFOPP_PATH_STAT_REVERSALS      dim 3 only, else 0: with s_i = cos(theta_i) * ex_i + sin(theta_i) * ey_i (theta_i the
 *                                      heading of p_i; the device's float64 cos / sin), pairs of consecutive NON-ZERO s_i
 *                                      of opposite sign
 *     5 NFOPP_PATH_STAT_MIN_CLEARANCE  min of pose_dist_dev[b, 0 .. poses_per_path)   (+inf when pose_dist_dev is null)
 *     6 NFOPP_PATH_STAT_CLEARANCE_AT   the first pose index attaining it              (-1)
 *     7 NFOPP_PATH_STAT_MEAN_CLEARANCE sum / poses_per_path                           (+inf)
 *   pose_dist_dev [B, poses_per_path] (may be null) is whatever the caller measured along the densified path
 *   (nfopp_path_interpolate, then a nearest-obstacle query).  active_dev (may be null) is accepted for symmetry with the
 *   other per-path calls and NOT consulted: rows with active == 0 are written too, statistics are wanted for retired paths.
 *   A sign byte per segment and the reductions' 64 bytes sit in one workgroup's LDS: N <= 163775, beyond that "path too long". */
#define NFOPP_NUM_PATH_STATS 8
#define NFOPP_PATH_STAT_LENGTH 0
#define NFOPP_PATH_STAT_MAX_CURVATURE 1
#define NFOPP_PATH_STAT_CURVATURE_AT 2
#define NFOPP_PATH_STAT_CUSPS 3
#define NFOPP_PATH_STAT_REVERSALS 4
#define NFOPP_PATH_STAT_MIN_CLEARANCE 5
#define NFOPP_PATH_STAT_CLEARANCE_AT 6
#define NFOPP_PATH_STAT_MEAN_CLEARANCE 7
int nfopp_nearest_obstacle(const float* poses_dev, int64_t n, int32_t pose_dim, const float* obstacles_dev,
                           int32_t n_obstacles, const float* box4, float* dist_dev, int32_t* index_dev, void* stream);
int nfopp_nearest_obstacle_cells(const float* poses_dev, int64_t n, int32_t pose_dim, const float* obstacles_sorted_dev,
                                 int32_t n_obstacles, const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y,
                                 float cell_x0, float cell_y0, float cell_size, const float* box4, float* dist_dev,
                                 int32_t* index_dev, void* stream);
int nfopp_nearest_obstacle_cells_probe(int32_t what, const float* poses_dev, int64_t n, int32_t pose_dim,
                                       const float* obstacles_sorted_dev, int32_t n_obstacles,
                                       const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y, float cell_x0,
                                       float cell_y0, float cell_size, const float* box4, float* dist_dev,
                                       int32_t* index_dev, void* stream);
int nfopp_path_stats(const float* traj_dev, const float* start_dev, const float* goal_dev, int64_t batch,
                     int32_t n_waypoints, int32_t dim, const float* pose_dist_dev, int32_t poses_per_path,
                     double cos_cusp, double* stats_dev, const uint8_t* active_dev, void* stream);

/* ---- swept collision check between consecutive poses (csrc/swept.hip), additive under ABI 6 ---------------------------
 * `collides`, the clearance and the path statistics judge SAMPLED poses.  These entries judge what lies between two of
 * them.  A segment is a pair of poses (a_dev[p], b_dev[p]) of pose_dim 2 or 3; between them x and y are linear and theta
 * is linear along the wrapped shortest difference (wrap_angle, fp32), the motion nfopp_path_interpolate lays its poses on.
 *
 * nfopp_swept_segments / nfopp_swept_segments_cells: value_dev[p] <- one fp32 value per segment, index_dev[p] (may be
 *   null) <- the obstacle point that attains it, the smallest k among equals, an index into the array passed in.
 *     box4 = NULL, disc robot -- exact.  With e = b - a, |e|^2 = fmaf(ex, ex, ey * ey), d = o - a:
 *         value = min over obstacle points o of  min( disc(o - a), disc(o - b), interior ? |cross| / sqrtf(|e|^2) : +inf ),
 *         interior: 0 < fmaf(ex, dx, ey * dy) < |e|^2 (strictly),  cross = fmaf(ex, dy, -(ey * dx)),
 *       disc(dx, dy) = sqrtf(fmaf(dx, dx, dy * dy)), the one expression nfopp_nearest_obstacle and the circle checker
 *       evaluate.  So, bit for bit: value <= min(nearest(a), nearest(b)); either end pose's circle label implies
 *       value < radius; a zero-length segment returns nfopp_nearest_obstacle's distance and index.  The disc swept along
 *       the segment is a capsule: value < radius IS the swept collision test.
 *     box4 = (x0, x1, y0, y1), box robot, pose_dim must be 3 -- a sound certificate.  With d_a(o), d_b(o) the distances from
 *       o to the closed box at either end (nfopp_nearest_obstacle's expression), reach = the box's largest corner distance
 *       (rounded up, formed inside the call) and  delta = fmaf(reach, |wrap_angle(theta_b - theta_a)|, |e|):
 *         value = fl( min over o of fl(d_a(o) + d_b(o))  -  delta ).
 *       On the way from a to the interpolation parameter s no body point travels more than s * delta, and the distance
 *       from a fixed point to the box is 1-Lipschitz in that displacement: an obstacle inside the box at some s needs
 *       d_a <= s delta and d_b <= (1 - s) delta, so d_a + d_b <= delta.  Hence
 *         value > slack = nfopp_swept_slack(box4) = reach * NFOPP_SWEPT_SLACK_REL (2^-16 = 256 * 2^-24)
 *       certifies the whole segment free.  slack bounds the rounding of `value` for every point that can decide it
 *       (d_a + d_b near delta, so |o - a| + |o - b| <= 2 reach + delta), in units of u = 2^-24:
 *         9.5 u (|dx| + |dy|) per distance (cosf / sinf to 2 ulp, the roundings of dx, dy, of the two fmas of the robot
 *           frame and of the distance; derived in tests/test_gpu_clearance.py)  -> 13.5 u (2 reach + delta) for the two,
 *         1 u delta for their sum,
 *         delta itself: 4 u |e|, 2 u delta for its fma, and reach times the error of the wrapped difference, at most
 *           (2.5 |theta_b - theta_a| + 17) u <= 80 u for a raw difference of at most 8 pi,
 *       together (107 reach + 20.5 delta) u: below 189 u reach while delta <= 4 reach.  A segment with delta > 4 reach or
 *       |theta_b - theta_a| > 8 pi (fp32) is outside that derivation and gets value -inf, index -1: not certifiable at
 *       this pose spacing.  A segment with value <= slack whose end poses are free is UNDECIDED: the caller needs more
 *       poses per segment (there is no adaptive subdivision here).
 *   horizon >= 0 (+inf allowed): a segment whose value exceeds it gets +inf and -1, which bounds the indexed search.  Both
 *   entries apply the same cap and write the same bytes, run after run (no atomics).
 *   n = 0 is a no-op.  n_obstacles = 0: every segment gets +inf and -1.  A segment with a non-finite component in either
 *   pose (x, y; theta too for the box) gets +inf and -1; nfopp_path_swept_labels treats it as not certified.  Coordinates
 *   are taken to be below 2^60 in magnitude (squares must not overflow).  box4 with pose_dim != 3, and a negative or NaN
 *   horizon, are argument errors.
 *   nfopp_swept_segments tests all pairs with the points staged in LDS: for small clouds, and the independent cross-check.
 *   nfopp_swept_segments_cells takes the index of nfopp_build_cell_index (any cell size), one thread per segment, and
 *   visits the rows of cells that cover the bounding box of the two end points inflated by R, plus one cell on each side:
 *     disc: R = horizon + 2^-18 (horizon + |e|);   box: R = (reach + delta + horizon)(1 + 2^-18).
 *   Every point whose computed value is <= horizon lies inside (disc: within `value` of the segment; box: d_a <= delta +
 *   horizon, so within reach + delta + horizon of a's origin; 2^-18 covers the fp32 evaluation), the bounds are rounded
 *   outward, and points and bounds get their cells from one monotone function (csrc/swept.hip has the full argument).
 *
 * nfopp_path_swept_labels: for B densified paths of m = poses_per_path poses, value_dev [B, m - 1] (segment j joins poses
 *   j and j + 1) and labels_dev [B * m] as the checker wrote them: labels_dev[b, j] <- 1 where segment j is not certified
 *   -- box == 0: value < threshold (the radius); box != 0: value <= threshold (the slack); a segment with a non-finite
 *   pose component either way.  The last pose keeps its label.  The result is what nfopp_path_select_best reads.
 *   status_dev [B] uint8 (may be null): 0 every segment certified and no pose in collision; 1 a pose, or for the disc a
 *   segment, in collision; 2 (box only) no pose collides but a segment is undecided.
 *   worst_dev [B, 2] fp32 (may be null): the smallest segment value of the path and the first segment index attaining it
 *   (+inf, 0 when every segment is beyond the horizon).  One workgroup per path, reductions in a fixed order. */
#define NFOPP_SWEPT_SLACK_REL 1.52587890625e-05f /* 2^-16 */
float nfopp_swept_slack(const float* box4);
int nfopp_swept_segments(const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim, const float* obstacles_dev,
                         int32_t n_obstacles, const float* box4, float horizon, float* value_dev, int32_t* index_dev,
                         void* stream);
int nfopp_swept_segments_cells(const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                               const float* obstacles_sorted_dev, int32_t n_obstacles, const int32_t* cell_start_dev,
                               int32_t cells_x, int32_t cells_y, float cell_x0, float cell_y0, float cell_size,
                               const float* box4, float horizon, float* value_dev, int32_t* index_dev, void* stream);
int nfopp_path_swept_labels(const float* poses_dev, const float* value_dev, float* labels_dev, int64_t batch,
                            int32_t poses_per_path, int32_t dim, float threshold, int32_t box, uint8_t* status_dev,
                            float* worst_dev, void* stream);

/* ---- box robot: undecided swept segments resolved by bisection (csrc/swept.hip), additive under ABI 6 ------------------
 * nfopp_swept_refine / nfopp_swept_refine_cells: box robot only (box4 required, pose_dim 3).  The certificate above is
 * applied to dyadic pieces of the segment and the rectangle checker's label to their midpoints until every piece is proven
 * free, a colliding pose is found or a limit is reached.
 *
 * Sub-poses.  For a segment (a, b), a depth d and an index i in 0 .. 2^d the parameter is s = i * 2^-d (exact in fp32):
 *   pose(0) = a as loaded, pose(1) = b as loaded, with its raw heading; otherwise
 *   x = fmaf(s, ex, a.x), y = fmaf(s, ey, a.y), theta = fmaf(s, dth, theta_a),
 *   ex = b.x - a.x, ey = b.y - a.y, dth = wrap_angle(theta_b - theta_a): the motion nfopp_path_interpolate lays its poses on.
 * Piece test.  cert(p, q) = the box value nfopp_swept_segments gives the segment (p, q) at horizon = slack, the domain rule
 *   included (delta > 4 reach or |theta_q - theta_p| > 8 pi, raw: not certified).  A piece is certified iff cert > slack; an
 *   empty cloud certifies everything.  hits(p) = the rectangle checker's label over the cloud: a point strictly inside.
 * Decision, refine(a, b; max_depth, node_budget), in this order:
 *   1. a non-finite component in either pose: UNDECIDED, s = -1, depth = 0 (as nfopp_path_swept_labels treats it);
 *   2. hits(a): HIT, s = 0; else hits(b): HIT, s = 1; both at depth 0;
 *   3. a pre-order walk of the dyadic tree from node (d = 0, i = 0); node (d, i) covers [i 2^-d, (i + 1) 2^-d]:
 *        cert certifies the piece: the node is FREE;  else d == max_depth: the node is UNDECIDED;
 *        else the midpoint pose hits: the whole segment is HIT, s = (2 i + 1) 2^-(d + 1), stop;
 *        else the left child, then the right child
 *      (no stack: after finishing (d, i), while i is odd i >>= 1, d -= 1; stop if d == 0; else i += 1);
 *   4. without a HIT the segment is UNDECIDED when any node was, else FREE;
 *   5. node_budget bounds the work: every piece test and every midpoint test is one evaluation of the candidate points,
 *      and each counts one against node_budget.  When node_budget evaluations are spent the walk stops UNDECIDED (a HIT
 *      found before that stands).  The order is fixed, so the outcome is deterministic.  node_budget = 1 pays for the
 *      root piece alone: the max_depth = 0 answer;
 *   6. depth = the deepest level at which a piece was tested.
 * Consequences.  FREE is a proof: the Lipschitz argument above on each certified piece, and the pieces cover [0, 1].  HIT is a
 *   proof: a pose of the motion has an obstacle point strictly inside the box.  depth == 0 && FREE is today's value > slack
 *   (where no end pose hits).  s is the first hit in pre-order, not necessarily the smallest s.  A segment the domain rule
 *   refuses is simply split -- except that the last piece keeps b's RAW heading, so a raw turn above 8 pi stays UNDECIDED
 *   (or becomes a HIT): wrap the headings first.  Termination: if every obstacle point stays at least c from the box along
 *   the whole motion every piece has d_a + d_b >= 2 c, so a piece is certified once its delta is below 2 c - slack, and
 *   the segment is decided by depth ceil(log2(delta / (2 c - slack))) + 1 (the + 1 absorbs the rounding of a piece's delta).
 * Defaults of the Python layer: max_depth = 8 (0 <= max_depth <= 20; at delta = 4 reach, about 2 m, the pieces are 8 mm long:
 *   more than about 4 mm of clearance is decided), node_budget = 1024 (>= 1).
 * status_dev uint8 [n]: 0 free, 1 hit, 2 undecided.  s_dev fp32 [n] (may be null): the parameter of the hit, -1 where there
 *   is none.  depth_dev uint8 [n] (may be null).  status_dev holds the same bytes with and without the other two.  Both
 *   entries write the same bytes, run after run (no atomics; only comparisons leave the reductions over the points, and a
 *   minimum and an OR do not depend on the order).  n = 0 is a no-op.  Null a / b / status, a missing box4, pose_dim != 3,
 *   max_depth outside 0 .. 20 and node_budget < 1 are argument errors.
 * Work shape: one thread per segment decides 1, 2 and the root piece; each remaining segment is walked by one wavefront
 *   over the segment's candidate points staged in LDS (1024 of them; further ones are read from global memory, none is
 *   dropped).  nfopp_swept_refine_cells gathers the candidates ONCE per segment from the rows of cells covering the
 *   bounding box of a and b inflated by (reach + delta_root + slack)(1 + 2^-18), bounds moved outward, one further cell per
 *   side; delta_root is the fp32 delta of the whole segment, inside the certificate's domain or not.  Every sub-pose lies
 *   in that bounding box, a piece's cert <= slack needs a point within reach + delta_piece + slack of a sub-pose, a midpoint
 *   hit a point within reach (csrc/swept.hip has the argument).
 *
 * nfopp_path_refined_labels: for B paths of m = poses_per_path poses, seg_status_dev uint8 [B, m - 1] and seg_s_dev fp32
 *   [B, m - 1] as nfopp_swept_refine wrote them, labels_dev [B * m] as the checker wrote them: labels_dev[b, j] <- 1 where
 *   segment j is not free; the last pose keeps its label.  status_dev [B] uint8 (may be null): 1 if a pose label was set on
 *   entry or a segment is a hit, else 2 if a segment is undecided, else 0.  first_dev [B, 2] fp32 (may be null; needs
 *   seg_s_dev): the first segment that is not free and its s, (-1, -1) if there is none.  One workgroup per path,
 *   reductions in a fixed order.  nfopp_path_select_best reads the labels unchanged. */
#define NFOPP_REFINE_FREE 0
#define NFOPP_REFINE_HIT 1
#define NFOPP_REFINE_UNDECIDED 2
int nfopp_swept_refine(const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim, const float* obstacles_dev,
                       int32_t n_obstacles, const float* box4, int32_t max_depth, int32_t node_budget, uint8_t* status_dev,
                       float* s_dev, uint8_t* depth_dev, void* stream);
int nfopp_swept_refine_cells(const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                             const float* obstacles_sorted_dev, int32_t n_obstacles, const int32_t* cell_start_dev,
                             int32_t cells_x, int32_t cells_y, float cell_x0, float cell_y0, float cell_size,
                             const float* box4, int32_t max_depth, int32_t node_budget, uint8_t* status_dev, float* s_dev,
                             uint8_t* depth_dev, void* stream);
int nfopp_path_refined_labels(const uint8_t* seg_status_dev, const float* seg_s_dev, float* labels_dev, int64_t batch,
                              int32_t poses_per_path, uint8_t* status_dev, float* first_dev, void* stream);

/* ---- exact Euclidean distance transform of an occupancy grid (csrc/grid_edt.hip), additive under ABI 6 ----------------
 * What a clearance margin for the grid-search seeds is decided on (nfopp/grid_search.py: OccupancyGrid.inflated).
 *
 * nfopp_grid_edt: occupancy_dev uint8 [rows, cols], non-zero = occupied (as in nfopp_grid_distance_fields).
 *   dist2_dev int32 [rows, cols] <- the squared Euclidean distance, in cells, from each cell to the nearest occupied
 *   cell: 0 on occupied cells, INT32_MAX everywhere when no cell is occupied.
 *   nearest_dev int32 [rows, cols] (may be null) <- the flat index row * cols + col of the occupied cell that attains
 *   dist2; among equidistant cells the SMALLEST flat index (smallest row, then smallest column); -1 everywhere when no
 *   cell is occupied.  dist2_dev holds the same bytes with and without nearest_dev.
 *   border != 0: cells outside the matrix count as occupied, dist2 <- min(dist2, b * b) with
 *   b = min(row + 1, rows - row, col + 1, cols - col).  nearest still names real cells only: it is what it is without
 *   the border (so dist2 may be smaller than the distance to `nearest`, and nearest stays -1 on an empty grid).
 *   Separable: a column pass keeps, per cell, the nearest occupied row of its column (above and below equally far: the
 *   smaller row), a row pass takes the minimum over col' of ((col - col')^2 + (row - g(row, col'))^2, g, col'), scanning
 *   outward from the cell over a copy of the row of g in LDS until (col - col')^2 alone exceeds the best distance.
 *   Integer arithmetic throughout, no atomics: the same bytes from run to run.
 *   Limits: 1 <= rows, cols <= 4096 and rows * cols <= 2^24 (the limit of nfopp_grid_to_points); larger input is an
 *   argument error.  workspace: nfopp_grid_edt_workspace_bytes(rows, cols) bytes of device scratch (0 = bad shape); it
 *   needs no initialisation. */
size_t nfopp_grid_edt_workspace_bytes(int32_t rows, int32_t cols);
int nfopp_grid_edt(const uint8_t* occupancy_dev, int32_t rows, int32_t cols, int32_t border, int32_t* dist2_dev,
                   int32_t* nearest_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- any-angle shortening of grid-search paths by exact line of sight (csrc/grid_any_angle.hip), additive under ABI 6 --
 * A shortest 8-connected path is a staircase and the spline through every cell centre wiggles with the cell size.  The two
 * entries below skip the cells between path cells that see each other and seed the spline through the shortened polyline
 * (nfopp/grid_search.py: shorten_paths, seed_polylines, grid_search_init(any_angle=True)).  The rule is this library's own.
 *
 * Line of sight.  Cells are unit squares, cell (r, c) the open square (c, c + 1) x (r, r + 1).  A = (r0, c0) sees
 *   B = (r1, c1) iff no BLOCKED cell other than A and B has an open interior met by the segment between the two centres.
 *   Such a segment never lies on a grid line; where it passes exactly through a lattice corner it meets the two diagonal
 *   cells only, not the two beside the corner -- the search's "no corner rule" (a diagonal move between two walls is
 *   legal), so consecutive cells of a traced path always see each other.
 *   The cells are visited by an integer merge of the two crossing sequences: with ar = |r1 - r0|, ac = |c1 - c0|, column
 *   crossing i = 1..ac lies at parameter (2i - 1) / (2 ac), row crossing j = 1..ar at (2j - 1) / (2 ar); compare
 *   (2i - 1) ar with (2j - 1) ac: smaller steps the column, larger the row, equal both at once (only the diagonal cell is
 *   visited).  Every product is at most 2 * 4096 * 4096 = 2^25: int32.  The merge visits exactly the cells whose interior
 *   the segment meets, each once.
 * Blocked.  Cell x is blocked for problem p iff dist2[x] <= cells2[p].  dist2_dev int32 [rows, cols] is the output of
 *   nfopp_grid_edt with border = 0 (one image serves every clearance level; INT32_MAX everywhere on a grid without walls,
 *   where nothing is blocked); cells2_dev int32 [batch] is the threshold of the level problem p was searched on, 0 on the
 *   plain grid (dist2 <= 0 is exactly "wall"), null = all 0.  dist2 >= 0, so a negative threshold blocks nothing; it is
 *   device data and not tested here (the Python wrapper refuses it).  The two end cells of a query are never tested: the
 *   search forces the goal free and leaves the start untested.
 * Anchors.  For a path p[0 .. n - 1]: a_0 = 0; a_{k+1} = the LARGEST j in (a_k, min(a_k + lookahead, n - 1)] such that
 *   p[a_k] sees p[j], or a_k + 1 if there is none (only possible with a caller-made list that is not 8-connected); the
 *   last anchor is n - 1.  Farthest visible, not "the first blocked cell ends the scan": visibility along a path is not
 *   monotone.  lookahead >= 1 bounds the work on maze paths of thousands of cells.
 * Dense points.  Each segment between anchors A -> B is refilled at the cell path's density: with m = max(|dr|, |dc|), for
 *   t = 0 .. m - 1 the point in cell units is u_c = (double)c0 + (double)(dc * t) / (double)m, u_r alike, stored as fp32
 *   metres x = (float)((u_c * resolution + resolution / 2) + origin_x), y from u_r and origin_y, float64 with every
 *   operation rounded on its own; the centre of the last anchor is appended; m = 0 (a repeated cell) emits nothing.  For an
 *   integer u this is bit for bit the centre nfopp_grid_seed_trajectories forms, so a path with nothing to shorten yields
 *   exactly its polyline.  For a traced path the point count never exceeds the cell count.
 *
 * nfopp_grid_shorten_paths: cells_dev / count_dev / status_dev as nfopp_grid_trace_paths wrote them.  A row with
 *   status != 0, count < 1, count > max_len or a cell outside the grid gets anchor_count = point_count = 0 and nothing else
 *   of it is written.  Otherwise anchor_dev int32 [batch, max_len] <- the anchors (indices into the cell path),
 *   anchor_count_dev [batch] their number; point_count_dev [batch] <- the number of dense points the path HAS, of which
 *   the first max_points are written to points_dev fp32 [batch, max_points, 2] (xy; may be null: counts and anchors only).
 *   count = 1 gives one anchor and one point.  One wavefront per problem: the lanes take the candidates j = hi - lane of a
 *   round of 64, farthest first, each walks its own traversal up to its first blocked cell, and the highest visible
 *   candidate of the first round that has one is taken by ballot; no atomics, the same bytes from run to run.
 *   Argument errors: lookahead < 1, a grid beyond the limits of nfopp_grid_edt, resolution <= 0, max_len > 2^21 + 1.
 * nfopp_grid_seed_polylines: nfopp_grid_seed_trajectories with the interior of the polyline read from points_dev fp32
 *   [batch, max_len, 2] (count_dev points per row) instead of formed from cell centres: [start, points, goal] -> spline ->
 *   waypoints, the same arithmetic, fallback rows (status != 0, count < 1, count > max_len) and workspace rule
 *   (nfopp_grid_seed_workspace_bytes). */
int nfopp_grid_shorten_paths(const int32_t* dist2_dev, int32_t rows, int32_t cols, const int32_t* cells_dev,
                             const int32_t* count_dev, const int32_t* status_dev, const int32_t* cells2_dev, int64_t batch,
                             int32_t max_len, int32_t lookahead, int32_t* anchor_dev, int32_t* anchor_count_dev,
                             double origin_x, double origin_y, double resolution, int32_t max_points, float* points_dev,
                             int32_t* point_count_dev, void* stream);
int nfopp_grid_seed_polylines(const float* points_dev, const int32_t* count_dev, const int32_t* status_dev, int64_t batch,
                              int32_t max_len, const float* start_dev, const float* goal_dev, int32_t n_waypoints,
                              int32_t dim, int32_t angles_with_direction, float* traj_dev, void* workspace_dev,
                              size_t workspace_bytes, void* stream);

/* ---- heading-aware lattice search for car-like seeds (csrc/lattice_search.hip), additive under ABI 6 ---------------------
 * A search over (cell, heading) states whose cell paths go through nfopp_grid_seed_trajectories unchanged
 * (nfopp/lattice.py: LatticeGrid, lattice_fields, lattice_search_paths, lattice_search_init).  The rule is this library's
 * own; the reference has no such search.  tests/lattice_ref.py restates it in numpy and the device is compared with ==.
 *
 * State: (cell (row, col), heading h in 0 .. 7); heading h stands for the angle h * pi / 4.
 * Directions dir(h) as (d row, d col), row = y and col = x as in the occupancy grid:
 *   h      0       1       2       3       4        5        6       7
 *   dir  (0,+1)  (+1,+1)  (+1,0)  (+1,-1)  (0,-1)  (-1,-1)  (-1,0)  (-1,+1)
 * Occupancy: layers_dev uint8 [L, rows, cols] with L = 1 or 8, non-zero = blocked.  State (c, h) reads layer h mod L.  Cells
 *   outside the image are blocked.  There is no corner rule between states.
 * Moves are forward only: from (c, h) to (c + dir(h'), h') with h' in {h, h + 1, h - 1} mod 8.  The move is along the heading
 *   the robot has AFTER it; that heading differs from the one before by at most one step.  The target state must be free.
 * Cost: an integer pair (a, b), ordered exactly as a + b * sqrt 2.  A move to an even h' adds (1, 0), a move to an odd h'
 *   adds (0, 1), a move with h' != h adds a further (turn_cost, 0), turn_cost an integer 0 .. 255.  Equal cost means equal
 *   pair, so the field is the unique fixed point of the relaxation: the same bits from run to run, compared with ==.
 * Goal: goal state g = (goal cell, goal heading); with goal heading -1 it is the goal cell at every heading.  Goal states
 *   have cost (0, 0) and are forced free.
 * Field: d_g(c, h) = the minimum cost from (c, h) to g.  The sentinel (-1, -1) marks blocked states, states that cannot
 *   reach g, every state of a goal whose cell is outside the grid and every state of a goal whose heading is outside -1 .. 7.
 * Trace: problem p starts in (start cell, start heading); the start state is NOT tested for occupancy.  At a state with a
 *   cost the next state is the first successor, tried in the order h' = h, h + 1, h - 1, whose cost plus the move equals
 *   the current cost exactly; the trace ends at the first state with cost (0, 0).  At a blocked start state, whose own value
 *   is the sentinel, the first step goes to the successor with the smallest d + move, ties broken by the same order; the
 *   path's cost is that sum; if no successor has a cost the status is 1.
 * Status: 0 ok; 1 unreachable; 2 the start or goal cell is outside the grid, or the start heading is outside 0 .. 7.
 * Refused before launch (argument error, nothing is clamped): turn_cost outside 0 .. 255, L not 1 or 8,
 *   8 * rows * cols * (1 + turn_cost) >= 2^21 (the bound under which the float64 key orders pairs exactly), a short
 *   workspace, null required pointers.
 *
 * nfopp_lattice_distance_fields: goal_states_dev int32 [G, 3] (row, col, heading or -1), callers pass each goal state once;
 *   fields_dev int32 [G, 8, rows, cols, 2] <- d_g.  One workgroup per goal state.  While the padded 8-layer field fits 144 KiB
 *   of LDS and 8 * rows * cols * (1 + turn_cost) <= 65535 the counts are packed 16 + 16 bits in LDS (no count can wrap);
 *   otherwise 32 + 32 bits in `workspace` (nfopp_lattice_fields_workspace_bytes, 0 for the LDS form and for a refused
 *   shape), 8-byte aligned, no initialisation needed.  No float atomics.
 * nfopp_lattice_trace_paths: one thread per problem.  start_states_dev int32 [B, 3] (row, col, heading), goal_states_dev
 *   int32 [B, 3], field_index_dev int32 [B] = the problem's field among n_total; fields_dev holds the n_fields fields
 *   field_first .. field_first + n_fields - 1 of them (a caller that cannot hold all fields at once calls once per chunk).
 *   A field_index outside 0 .. n_total - 1 gives status 2, like an off-grid cell or a bad start heading: all are tested
 *   before anything is indexed by them.  A problem whose field is not among the ones passed is not touched by the call.
 *   cells_dev int32 [B, max_len, 2] (row, col), headings_dev int32 [B, max_len] (first and last state included), count_dev [B]
 *   = states the path has (max_len = 0 sizes the buffers: nothing is written to cells / headings, which may be null),
 *   status_dev [B], cost_dev [B, 2] (may be null) = (a, b) of the path, (-1, -1) and count 0 where status != 0. */
size_t nfopp_lattice_fields_workspace_bytes(int32_t rows, int32_t cols, int32_t turn_cost, int64_t n_goals);
int nfopp_lattice_distance_fields(const uint8_t* layers_dev, int32_t n_layers, int32_t rows, int32_t cols,
                                  const int32_t* goal_states_dev, int64_t n_goals, int32_t turn_cost, int32_t* fields_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream);
int nfopp_lattice_trace_paths(const int32_t* fields_dev, int64_t field_first, int64_t n_fields, int64_t n_total,
                              int32_t rows, int32_t cols, int32_t turn_cost, const int32_t* start_states_dev,
                              const int32_t* goal_states_dev, const int32_t* field_index_dev, int64_t batch, int32_t max_len,
                              int32_t* cells_dev, int32_t* headings_dev, int32_t* count_dev, int32_t* status_dev,
                              int32_t* cost_dev, void* stream);

/* ---- lattice search with reverse moves and gear changes (csrc/lattice_gears.hip), additive under ABI 6 --------------------
 * The search above over (cell, heading, gear) states, so that a seed may back out of a dead end or make a three-point turn,
 * a trace that reports the gear of every move, and a seeding entry that takes the body heading from the lattice states
 * (nfopp/lattice.py: lattice_gear_fields, lattice_gear_search_paths, seed_lattice_trajectories, lattice_gear_search_init,
 * GearLattice).  The rule is this library's own; tests/lattice_gears_ref.py restates it in numpy and the device is compared
 * with ==.  Directions, headings, occupancy layers and the pair order are those of the section above, unchanged.
 *
 * State: (cell c, heading h in 0 .. 7, gear s in {0 forward, 1 reverse}).  s is the gear of the move that entered the state.
 *   Occupancy does not depend on s: state (c, h, s) reads layer h mod L, cells outside the image are blocked, no corner rule.
 * Moves.  Forward, gear 0: from (c, h) to (c + dir(h'), h').  Reverse, gear 1: from (c, h) to (c - dir(h), h'): a forward move
 *   run backwards in time, so the robot backs along the heading it had BEFORE the move.  In both h' in {h, h + 1, h - 1} mod
 *   8, and the target state must be free.
 * Cost: an integer pair (a, b), ordered exactly as a + b * sqrt 2.  A forward move adds (1, 0) for even h' and (0, 1) for odd
 *   h'.  A reverse move adds (1, 0) for even h and (0, 1) for odd h: the parity of the direction it moves along.  Either adds
 *   (turn_cost, 0) where h' != h.  A reverse move adds a further (reverse_cost, 0).  A move whose gear differs from s adds
 *   (cusp_cost, 0).  All three costs are integers 0 .. 255.
 * Goal: (goal cell, goal heading or -1 for every heading), at both gears.  Cost (0, 0), forced free.
 * Field: d_g(s, h, c) = the minimum cost from the state to the goal, int32 [G, 2, 8, rows, cols, 2].  (-1, -1) marks blocked
 *   states, states that cannot reach the goal, and every state of a goal whose cell is outside the grid or whose heading is
 *   outside -1 .. 7.
 * Trace: the start has no gear: its first move is charged no cusp cost.  The start state is NOT tested for occupancy.  A start
 *   that is a goal state gives the one-state path with cost (0, 0).  Otherwise the first move is the one of the six successors
 *   with the smallest d(successor) + move cost without the cusp term.  The order is forward h, h + 1, h - 1, then reverse h,
 *   h + 1, h - 1; ties go to the first in that order; the path's cost is that sum; if no successor has a cost the status is 1.
 *   After the first move the next state is the first successor in the same order whose cost plus the move (with the cusp
 *   term) equals the current cost exactly.  The trace ends at the first state with cost (0, 0).  This one rule covers blocked
 *   starts too.
 * Status: 0 ok; 1 unreachable; 2 the start or goal cell is outside the grid, or the start heading is outside 0 .. 7.
 * Refused before launch (argument error, nothing is clamped): a cost outside 0 .. 255, L not 1 or 8,
 *   16 * rows * cols * (1 + turn_cost + reverse_cost + cusp_cost) >= 2^21 (the bound under which the float64 key orders pairs
 *   exactly, on the largest count a path over 16 * rows * cols states can reach), a short or misaligned workspace, null
 *   required pointers.
 *
 * nfopp_lattice_gear_distance_fields: goal_states_dev int32 [G, 3]; fields_dev int32 [G, 2, 8, rows, cols, 2] <- d_g, every
 *   element written.  One workgroup per goal state.  While the padded 16-layer field fits 144 KiB of LDS and the count above
 *   is <= 65535 the pairs are packed 16 + 16 bits in LDS; otherwise 32 + 32 bits in `workspace`
 *   (nfopp_lattice_gear_fields_workspace_bytes, 0 for the LDS form and for a refused shape), 8-byte aligned, no initialisation
 *   needed; of it only the queried number of bytes is written.  No atomics; the same bits run after run.
 * nfopp_lattice_gear_trace_paths: one thread per problem; arguments as nfopp_lattice_trace_paths, every index tested before
 *   anything is indexed by it, a problem whose field is not among the ones passed is not touched.  Writes count_dev [B],
 *   status_dev [B], cost_dev [B, 2] (may be null) of every other problem; (-1, -1) and count 0 where status != 0.  Of
 *   cells_dev [B, max_len, 2], headings_dev [B, max_len] and gears_dev [B, max_len] it writes the first min(count, max_len)
 *   entries of a problem with status 0 and nothing else (max_len = 0 sizes the buffers; the three may then be null).
 *   gears[k] is the gear of the move into state k; gears[0] is the gear of the first move, or 0 for a one-state path.
 *   fields_dev is the caller's: on a field that is no fixed point of the rule a walk that finds no fitting successor, or
 *   does not end within 16 * rows * cols moves, gives status 1 (entries of its row may then have been written).
 * nfopp_lattice_seed_trajectories: SE(2) only, traj_dev fp32 [B, N, 3], every element written.  xy is bit for bit what
 *   nfopp_grid_seed_trajectories writes for the same cells (one code path).  theta is the body heading of the lattice path,
 *   unwound, interpolated over the parameter the spline already has.  With m = count + 2 knots in float64: A[0] = theta_start;
 *   the first cell knot is a1 = theta_start + wrap(h_0 * (pi / 4) - theta_start); cell knot k is a1 + u_k * (pi / 4) with
 *   u_0 = 0 and u_k = u_(k-1) + the signed heading step ((h_k - h_(k-1) + 4) mod 8) - 4, which is -1, 0 or +1 on a lattice
 *   path; the goal knot is the last cell knot + wrap(theta_goal - it); wrap(x) = x - 2 pi * rint(x / (2 pi)).  Waypoint i has
 *   q = (i + 1) * (1 / (N + 1)), the product the xy spline is evaluated at; k is the largest index in 0 .. m - 2 with
 *   PAR_k <= q, PAR the spline's normalised chord-length parameter; theta = A_k + (A_(k+1) - A_k) * ((q - PAR_k) /
 *   (PAR_(k+1) - PAR_k)), rounded to fp32.  Every operation is rounded on its own; no atan2, sin or cos.  A problem with
 *   status != 0 or a count outside 1 .. max_len gets the trajectory of nfopp_init_trajectories with angles_with_direction = 0.
 *   Workspace as nfopp_grid_seed_workspace_bytes (nfopp_lattice_seed_workspace_bytes returns the same number). */
size_t nfopp_lattice_gear_fields_workspace_bytes(int32_t rows, int32_t cols, int32_t turn_cost, int32_t reverse_cost,
                                                 int32_t cusp_cost, int64_t n_goals);
int nfopp_lattice_gear_distance_fields(const uint8_t* layers_dev, int32_t n_layers, int32_t rows, int32_t cols,
                                       const int32_t* goal_states_dev, int64_t n_goals, int32_t turn_cost, int32_t reverse_cost,
                                       int32_t cusp_cost, int32_t* fields_dev, void* workspace_dev, size_t workspace_bytes,
                                       void* stream);
int nfopp_lattice_gear_trace_paths(const int32_t* fields_dev, int64_t field_first, int64_t n_fields, int64_t n_total,
                                   int32_t rows, int32_t cols, int32_t turn_cost, int32_t reverse_cost, int32_t cusp_cost,
                                   const int32_t* start_states_dev, const int32_t* goal_states_dev,
                                   const int32_t* field_index_dev, int64_t batch, int32_t max_len, int32_t* cells_dev,
                                   int32_t* headings_dev, int32_t* gears_dev, int32_t* count_dev, int32_t* status_dev,
                                   int32_t* cost_dev, void* stream);
size_t nfopp_lattice_seed_workspace_bytes(int64_t batch, int32_t max_len);
int nfopp_lattice_seed_trajectories(const int32_t* cells_dev, const int32_t* headings_dev, const int32_t* count_dev,
                                    const int32_t* status_dev, int64_t batch, int32_t max_len, const float* start_dev,
                                    const float* goal_dev, int32_t n_waypoints, double origin_x, double origin_y,
                                    double resolution, float* traj_dev, void* workspace_dev, size_t workspace_bytes,
                                    void* stream);

/* ---- time parametrisation under motion limits (csrc/time_profile.hip), additive under ABI 6 --------------------------------
 * Everything above is geometry; these two entries say WHEN the robot is where and how fast it may go, for a whole batch,
 * without a host round trip.  Float64 throughout, every operation rounded on its own; the two prefix sums are integers, so
 * a parallel scan and a sequential loop give the same bits (tests/time_profile_ref.py restates the rule in numpy and the
 * device is compared with it bit for bit).  No atomics; the same bits run after run.
 *
 * Polyline p_0 .. p_{N+1} = start, waypoints, goal (read as fp32, widened); segment i = 0..N joins p_i and p_{i+1}, ex, ey its
 * xy difference.  A = 2 * a_max, Dd = 2 * d_max.  v_start_dev / v_goal_dev [B] fp32 >= 0 (null = rest).
 * Arc length.  n_i = sqrt(ex * ex + ey * ey), L_i = llrint(n_i * 2^32), S_i = L_0 + .. + L_{i-1} (integers), s_i = S_i * 2^-32.
 * Gear (dim 3; +1 throughout for dim 2).  The sign of the forward component cos(theta_i) * ex + sin(theta_i) * ey as
 *   NFOPP_PATH_STAT_REVERSALS forms it; a zero takes the last non-zero sign before it, else the first after it, else +1.
 * Vertex caps on v^2.  kappa_i = the Menger curvature of NFOPP_PATH_STAT_MAX_CURVATURE at interior vertex i (same candidate
 *   rule); k_i = min(a_lat / kappa_i, (w_max / kappa_i)^2) where kappa_i exists and is > 0, else +inf; k_0 = k_{N+1} = +inf.
 *   Vertex i is a STOP when it is a cusp by NFOPP_PATH_STAT_CUSPS' rule with limits->cos_cusp (never when cos_cusp == -1) or
 *   when the gears of segments i - 1 and i differ.  c_i = 0 at a stop, else min(v_max^2, k_i); c_0 = v_start^2,
 *   c_{N+1} = v_goal^2.
 * Speeds, the closed form of a forward and a backward sweep (two scans of exact, order-free minima):
 *   fwd_i = min_{j <= i}(c_j - A * s_j) + A * s_i,  bwd_i = min_{j >= i}(c_j + Dd * s_j) - Dd * s_i,
 *   u_i = max(0, min(c_i, fwd_i, bwd_i)),  v_i = sqrt(u_i).
 * Segment i, time-optimal on a straight piece.  ds = L_i * 2^-32, g = min(v_max^2, max(k_i, k_{i+1})),
 *   u_p = max(min(g, (((A * d_max) * ds + d_max * u_i) + a_max * u_{i+1}) / (a_max + d_max)), max(u_i, u_{i+1})), v_p = sqrt(u_p),
 *   t_acc = (v_p - v_i) / a_max, t_dec = (v_p - v_{i+1}) / d_max, l_cruise = max(0, (ds - (u_p - u_i) / A) - (u_p - u_{i+1}) / Dd),
 *   t_cruise = l_cruise > 0 ? l_cruise / v_p : 0, duration = (t_acc + t_cruise) + t_dec, Q_i = llrint(duration * 2^32),
 *   T_i = Q_0 + .. + Q_{i-1} (integers), t_i = T_i * 2^-32.  A segment between two stops takes finite time, and a dense
 *   smooth curve does not bulge above the larger of its two neighbouring caps.
 *
 * nfopp_path_time_profile: one workgroup per path, the path's image in LDS; N + 2 <= 3032 (dim 3) / 3275 (dim 2), beyond
 *   that "path too long".  Writes
 *     profile_dev [B, N + 2, NFOPP_NUM_TIME_SLOTS] float64: s_i, t_i, v_i, and v_p of the segment that STARTS at vertex i
 *                 (the last vertex: its own v)
 *     gear_dev    [B, N + 1] int8 (may be null)
 *     summary_dev [B, NFOPP_NUM_TIME_SUMMARY] float64: total time t_{N+1}, length s_{N+1}, number of stops, status
 *   status bits: NFOPP_TIME_START_TOO_FAST u_0 < v_start^2; NFOPP_TIME_GOAL_UNREACHABLE u_{N+1} < v_goal^2;
 *   NFOPP_TIME_OUT_OF_RANGE (always alone): a non-finite coordinate, a speed not in [0, inf), a segment of 2^20 m or more, a
 *   total of 2^21 m or more, or a duration not below 2^20 s -- the row's profile and its first three summary slots are NaN
 *   and its gear is 0.
 * nfopp_path_time_sample: states_dev [B, count, dim + 1] fp32 <- pose and SIGNED speed (gear * speed) at the instants
 *   t = t0 + k * dt, k = 0 .. count - 1 (k * dt rounded, then the sum); segment_dev [B, count] int32 (may be null).  One
 *   thread per instant, the path's t column in LDS.  profile_dev / gear_dev as written above; a null gear_dev means +1.
 *   Before t_0: start pose, speed 0, segment -1.  At or after t_{N+1}: goal pose, gear_N * v_{N+1}, segment N + 1.  A NaN
 *   profile row: NaN states, segment -1.  Else i = the largest i <= N with t_i <= t (binary search; ties over zero-duration
 *   segments go to the largest i), tau = t - t_i, dur = t_{i+1} - t_i, rem = dur - tau, ds = s_{i+1} - s_i,
 *   t_acc = (v_p - v_i) / a_max, t_dec = (v_p - v_{i+1}) / d_max, ha = 0.5 * a_max, hd = 0.5 * d_max:
 *     tau < t_acc:       dist = v_i * tau + (ha * tau) * tau,                                speed = v_i + a_max * tau
 *     else rem < t_dec:  dist = ds - (v_{i+1} * rem + (hd * rem) * rem),                     speed = v_{i+1} + d_max * rem
 *     else:              dist = (v_i * t_acc + (ha * t_acc) * t_acc) + v_p * (tau - t_acc),  speed = v_p
 *   dist = min(max(dist, 0), ds), speed = min(speed, v_p), frac = ds > 0 ? dist / ds : 0; x = fp32(x_i + frac * (x_{i+1} - x_i)),
 *   y alike, theta = fp32(theta_i + frac * dth) with dth the fp32 wrap_angle(theta_{i+1} - theta_i) that
 *   nfopp_path_interpolate lays its poses on, widened.
 * Argument errors (both): dim, n_waypoints < 1, batch < 0, null limits, v_max / a_max / d_max not positive and finite,
 *   a_lat / w_max not positive (+inf allowed, NaN not), cos_cusp outside [-1, 1]; for the sampler also dt not positive and
 *   finite, t0 not finite, count < 0.  batch == 0 returns 0 with null pointers. */
typedef struct nfopp_motion_limits {
  double v_max;     /* m/s */
  double a_max;     /* acceleration, m/s^2 */
  double d_max;     /* deceleration, m/s^2 */
  double a_lat;     /* lateral acceleration v^2 * kappa, +inf = none */
  double w_max;     /* turn rate v * kappa, +inf = none */
  double cos_cusp;  /* cusp threshold of nfopp_path_stats; -1 = no cusp stops */
} nfopp_motion_limits;
#define NFOPP_NUM_TIME_SLOTS 4
#define NFOPP_TIME_SLOT_S 0
#define NFOPP_TIME_SLOT_T 1
#define NFOPP_TIME_SLOT_V 2
#define NFOPP_TIME_SLOT_V_PEAK 3
#define NFOPP_NUM_TIME_SUMMARY 4
#define NFOPP_TIME_SUMMARY_TIME 0
#define NFOPP_TIME_SUMMARY_LENGTH 1
#define NFOPP_TIME_SUMMARY_STOPS 2
#define NFOPP_TIME_SUMMARY_STATUS 3
#define NFOPP_TIME_START_TOO_FAST 1
#define NFOPP_TIME_GOAL_UNREACHABLE 2
#define NFOPP_TIME_OUT_OF_RANGE 4
int nfopp_path_time_profile(const float* traj_dev, const float* start_dev, const float* goal_dev, int64_t batch,
                            int32_t n_waypoints, int32_t dim, const nfopp_motion_limits* limits, const float* v_start_dev,
                            const float* v_goal_dev, double* profile_dev, int8_t* gear_dev, double* summary_dev, void* stream);
int nfopp_path_time_sample(const float* traj_dev, const float* start_dev, const float* goal_dev, int64_t batch,
                           int32_t n_waypoints, int32_t dim, const nfopp_motion_limits* limits, const double* profile_dev,
                           const int8_t* gear_dev, double t0, double dt, int32_t count, float* states_dev,
                           int32_t* segment_dev, void* stream);

/* ---- conflicts between timed tracks (csrc/track_conflict.hip), additive under ABI 6 -----------------------------------------
 * The entries above compare a path with a static map.  This one compares tracks with tracks: the B paths of a batch as B
 * robots on one floor (self mode), or a set of timed paths against M predicted tracks of moving obstacles -- who comes closer
 * than the radii allow, when first, and with whom, all pairs on the device.  Float64 throughout, every operation rounded on
 * its own; the reductions are lexicographic minima on (value, index) and an integer count, which do not depend on the order:
 * no float atomics, the same bits run after run, and the device is compared bit for bit with the numpy restatement in
 * tests/track_conflict_ref.py.
 *
 * Inputs.  A track is k >= 1 positions at t_n = t0 + n * dt (n * dt rounded, then the sum, as nfopp_path_time_sample forms
 *   its instants), read as fp32 and widened.  tracks_a_dev [ba, k, stride_a] fp32, tracks_b_dev [bb, k, stride_b]: x, y are
 *   the first two floats of a row, stride >= 2 -- the [B, count, dim + 1] states of nfopp_path_time_sample are consumed as
 *   they are.  Between two instants a track is LINEAR IN TIME (this check's own rule; see "what linearity costs").
 *   tracks_b_dev == null is SELF MODE: the partners of track i are all j != i of set A (bb, stride_b, radius_b_dev are not
 *   read).  A non-null tracks_b_dev with bb == 0 is a set of no obstacles.  radius_a_dev [ba], radius_b_dev [bb] fp32, null
 *   = 0; self mode uses radius_a_dev for both sides.  R_ij = (ra_i + rb_j) + margin, R2_ij = R_ij * R_ij (float64; R_ij is
 *   meant to be >= 0: the test below is on squares).  A box robot takes the radius of its circumscribed disc.
 * Pair (i, j), interval n = 0 .. k - 2, componentwise d0 = pa_n - pb_n, d1 = pa_{n+1} - pb_{n+1}, w = d1 - d0:
 *     c = d0x * d0x + d0y * d0y,  a = wx * wx + wy * wy,  b = d0x * wx + d0y * wy
 *     a == 0 or b >= 0:  s = 0,         m = c
 *     else -b >= a:      s = 1,         m = d1x * d1x + d1y * d1y
 *     else:              s = (-b) / a,  p = d0 + s * w,  m = px * px + py * py
 *   and one more term for the last instant: n = k - 1, s = 0, m = |d_{k-1}|^2 (the whole check when k = 1).
 *   M_ij = min_n m_n, attained first at n*;  t*_ij = t_{n*} + s_{n*} * dt;  the gap g_ij = sqrt(M_ij) - R_ij.
 * Conflict.  Pair (i, j) is in conflict when some m_n < R2_ij (strict, like the circle checker's dist < radius).  At the
 *   smallest such n: s_in = 0 when c < R2, else disc = max(b * b - a * (c - R2), 0),
 *   s_in = min(max(((-b) - sqrt(disc)) / a, 0), s);  tc_ij = t_n + s_in * dt.  A pair without conflict has tc_ij = +inf.
 * Bad tracks.  A track with a non-finite coordinate (or radius) is BAD: as a partner it is skipped by everyone, its own
 *   summary row is NaN with status NFOPP_CONFLICT_BAD_TRACK, its pair-matrix rows and columns are NaN (its diagonal entry in
 *   self mode included).
 * summary_dev [ba, NFOPP_NUM_CONFLICT_SLOTS] float64, over the good partners j of track i:
 *     MIN_GAP        min_j g_ij; ties: the smaller j (the lexicographic minimum on (g, j));  +inf without a partner
 *     MIN_PARTNER    j of that minimum, -1 without a partner
 *     MIN_TIME       t* of that pair, NaN without a partner
 *     FIRST_TIME     min_j tc_ij, +inf if none; ties: the smaller j
 *     FIRST_PARTNER  j of that minimum, -1 if none
 *     CONFLICTS      number of partners in conflict
 *     STATUS         0, NFOPP_CONFLICT_BAD_TRACK, or NFOPP_CONFLICT_NO_PARTNER (no good partner: one robot alone, no
 *                    obstacles, or every partner bad)
 *   summary_b_dev [bb, NFOPP_NUM_CONFLICT_SLOTS] (may be null; not read in self mode): the same from set B's side, partners i.
 * pair_gap_dev, pair_first_dev [ba, bb] float64 (each may be null): g_ij and tc_ij; in self mode [ba, ba] with +inf on the
 *   diagonal.  In self mode every quantity above is even in the sign of d: swapping i and j negates d0, d1 and w exactly, and
 *   every product is of two negated factors -- so the matrices are BITWISE SYMMETRIC, and the kernel evaluates the tiles of
 *   the upper triangle only and serves both rows from them.
 * What linearity costs.  A point moving at speed <= v stays within v * dt / 2 of the chord between its positions dt apart:
 *   at time tau into the interval, with lambda = tau / dt, its distance from the chord point is at most
 *   (1 - lambda) * v * tau + lambda * v * (dt - tau) = 2 * v * tau * (dt - tau) / dt <= v * dt / 2.  Two robots timed under
 *   v_max therefore never get closer than gap - v_max * dt; `margin` is where the caller puts (va_max + vb_max) * dt / 2.
 * workspace_dev: nfopp_track_conflicts_workspace_bytes(ba, bb, k) bytes (bb = 0 in self mode), rewritten by every call.
 * Everything runs on `stream`; nothing synchronises.  Argument errors: a negative batch size, k < 1, a stride < 2, dt not
 *   positive and finite, t0 or margin not finite, null tracks_a_dev / summary_dev with ba > 0, more tiles of 32 x 32 pairs than
 *   a grid holds (2^31 - 1), a workspace that is null or too small.  ba == 0 returns 0 with null pointers and writes nothing;
 *   self mode with ba == 1 writes the "no partner" row. */
#define NFOPP_NUM_CONFLICT_SLOTS 7
#define NFOPP_CONFLICT_SLOT_MIN_GAP 0
#define NFOPP_CONFLICT_SLOT_MIN_PARTNER 1
#define NFOPP_CONFLICT_SLOT_MIN_TIME 2
#define NFOPP_CONFLICT_SLOT_FIRST_TIME 3
#define NFOPP_CONFLICT_SLOT_FIRST_PARTNER 4
#define NFOPP_CONFLICT_SLOT_CONFLICTS 5
#define NFOPP_CONFLICT_SLOT_STATUS 6
#define NFOPP_CONFLICT_BAD_TRACK 1
#define NFOPP_CONFLICT_NO_PARTNER 2
size_t nfopp_track_conflicts_workspace_bytes(int64_t ba, int64_t bb, int32_t k);
int nfopp_track_conflicts(const float* tracks_a_dev, int64_t ba, int32_t stride_a, const float* tracks_b_dev, int64_t bb,
                          int32_t stride_b, int32_t k, double t0, double dt, const float* radius_a_dev,
                          const float* radius_b_dev, double margin, double* summary_dev, double* summary_b_dev,
                          double* pair_gap_dev, double* pair_first_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);

/* ---- conflicts between timed SE(2) tracks of oriented boxes (csrc/box_conflict.hip), additive under ABI 6 --------------------
 * nfopp_track_conflicts sees every robot as a disc; a car is a box that drives along its heading, and two of them pass in
 * neighbouring lanes long before their circumscribed discs do.  These entries check box against box over time: the separation
 * of the boxes at the instants, a Lipschitz certificate for what lies between two instants (the form of the static swept
 * check), and bisection of what the certificate leaves undecided.  Float64 with every operation rounded on its own; after the
 * headings pass only +, -, *, /, sqrt and comparisons, so the device is compared bit for bit with the numpy restatement in
 * tests/box_conflict_ref.py when that is given the device's unit vectors.  No float atomics, no float sums: the same bits run
 * after run.
 *
 * nfopp_track_headings.  tracks_dev [batch, k, stride >= 3] fp32, x, y, theta first in a row (the states of
 *   nfopp_path_time_sample for SE(2) as they are) -> heading_dev [batch, k, 2] float64 (cos theta, sin theta) of the widened
 *   theta, NaN for a theta that is not finite.  The only transcendental step of the check; the pair kernel never reads theta.
 * Tracks.  Instants t_n = t0 + n * dt as for nfopp_track_conflicts.  Between two instants the position is LINEAR IN TIME and the
 *   heading turns the shorter way at a constant rate.  tracks_b_dev == null is SELF MODE (heading_b_dev, box_b_dev,
 *   radius_b_dev, bb, stride_b are not read); a non-null tracks_b_dev with bb == 0 is a set of no obstacles.
 * Shape.  box_a_dev [ba, 4], box_b_dev [bb, 4] fp32: x0, x1, y0, y1 of each track's box in its body frame, x0 < x1, y0 < y1 (a
 *   zero-size box is not allowed: a disc is a small box plus a rounding radius, or goes to nfopp_track_conflicts).
 *   radius_a_dev [ba], radius_b_dev [bb] fp32, null = 0: the rounding radius r >= 0.  reach = fl32(fl32(sqrt(mx * mx + my * my))
 *   * 1.000001f) with mx = max(|x0|, |x1|), my = max(|y0|, |y1|) widened to float64: box_reach of the static checkers with
 *   hypotf written as the rounded float64 root.  R_ij = (r_i + r_j) + margin as for nfopp_track_conflicts;
 *   D_ij = (reach_i + reach_j) + R_ij, D2_ij = D_ij * D_ij.
 * Bad tracks.  A non-finite x, y, unit vector, box entry or radius, x0 >= x1, y0 >= y1 or r < 0 make a track BAD: nobody's
 *   partner, its summary row NaN with status NFOPP_CONFLICT_BAD_TRACK, its pair rows and columns NFOPP_BOX_PAIR_BAD / NaN (the
 *   diagonal entry in self mode included).
 * Separation at an instant, poses P_i = (p_i, u_i), P_j = (p_j, u_j), u = (c, s):
 *     d = p_j - p_i;  cr = ci * cj + si * sj,  sr = ci * sj - si * cj
 *     xi = dx * ci + dy * si,  yi = dy * ci - dx * si;  xj = -(dx * cj + dy * sj),  yj = -(dy * cj - dx * sj)
 *     gap(t, box, cx, cy, s0, s1):  a0 = box.x0 * cx, a1 = box.x1 * cx, b0 = box.y0 * cy, b1 = box.y1 * cy,
 *       lo = (t + min(a0, a1)) + min(b0, b1),  hi = (t + max(a0, a1)) + max(b0, b1),  max(lo - s1, s0 - hi)
 *     g1 = gap(xi, box_j, cr, -sr, x0_i, x1_i),  g2 = gap(yi, box_j, sr, cr, y0_i, y1_i)
 *     g3 = gap(xj, box_i, cr, sr, x0_j, x1_j),   g4 = gap(yj, box_i, -sr, cr, y0_j, y1_j)
 *     sep = max(max(g1, g2), max(g3, g4))        with max(a, b) = a > b ? a : b and min(a, b) = a < b ? a : b
 *   -- the largest gap over the four face axes (the separating-axis test): sep < 0 iff the open boxes intersect, and sep never
 *   exceeds the distance between the boxes.
 * A sub-interval [a, b] -- an interval of the grid or a dyadic part of one -- with poses P at a and Q at b.  In this order:
 *     1. d0 = p_i - p_j at a, d1 at b, c = |d0|^2, e = |d1|^2, and (a, b, s, m) the closest approach of nfopp_track_conflicts'
 *        rule on them.  m >= D2: FREE (the discs of radius reach cover the boxes at every heading; this step is part of the
 *        rule: it decides cases step 3 cannot).
 *     2. sa = sep at a.  sa - R < 0: CONFLICT at a (strict).
 *     3. sb = sep at b;  ni = sqrt(|Q_i.u - P_i.u|^2), nj likewise;  mot = sqrt(a) + H * (reach_i * ni + reach_j * nj) with H
 *        the float64 next above pi / 2 (0x1.921fb54442d19p+0).  ((sa + sb) - mot) * 0.5 - R >= 0: FREE.  The certificate: the
 *        distance f between the rounded boxes changes no faster than the relative position moves plus reach times the angle
 *        each box turns; an angle phi <= pi is at most (pi / 2) * 2 sin(phi / 2), its chord; so over the sub-interval
 *        f >= max(f_a - lambda * mot, f_b - (1 - lambda) * mot) >= (f_a + f_b - mot) / 2, and f >= sep.
 *     4. depth < refine, and li = sqrt(|P_i.u + Q_i.u|^2) != 0 and lj != 0: split at the mid pose, p = (p_a + p_b) * 0.5 and
 *        u = (P.u + Q.u) / l (the exact middle of the shorter turn); the left half first, then the right half.  A zero sum is
 *        a turn of exactly pi, whose direction is not defined.
 *     5. Otherwise UNDECIDED at a.
 * A pair.  The intervals in time order, then one term for the last instant: with d = p_i - p_j there, unless |d|^2 >= D2 (the
 *   discs, as in step 1), sep_{k-1} - R < 0 is a CONFLICT at t_{k-1} (the whole check when k = 1).  The walk stops at the first CONFLICT: first_ij is its time, +inf if none; undecided_ij is the
 *   time of the first UNDECIDED met before it, +inf if none.  The node at depth d and position pos of interval n has the time
 *   t_n + (pos / 2^d) * dt, an exact dyadic fraction.  Status: NFOPP_BOX_PAIR_CONFLICT when first < inf, else
 *   NFOPP_BOX_PAIR_UNDECIDED when undecided < inf, else NFOPP_BOX_PAIR_FREE.  Raising `refine` only splits what was UNDECIDED.
 *   FREE says that the rounded boxes stay R apart between the instants under the motion model above; CONFLICT says sep < R at
 *   the reported time; continuous-time exactness beyond the certificate is not claimed.
 * Self mode evaluates i < j with i as the first box and COPIES the result to (j, i): the arithmetic is not even in the order of
 *   the boxes, the matrices are symmetric because they are copied.
 * summary_dev [ba, NFOPP_NUM_BOX_CONFLICT_SLOTS] float64, over the good partners j of track i:
 *     FIRST_TIME, FIRST_PARTNER          the lexicographic minimum on (first_ij, j); +inf, -1 if none
 *     CONFLICTS                          number of partners whose status is CONFLICT
 *     UNDECIDED_TIME, UNDECIDED_PARTNER  the lexicographic minimum on (undecided_ij, j) over all partners; +inf, -1 if none
 *     UNDECIDED                          number of partners whose status is UNDECIDED
 *     STATUS                             0, NFOPP_CONFLICT_BAD_TRACK or NFOPP_CONFLICT_NO_PARTNER
 *   summary_b_dev [bb, ...] (may be null; not read in self mode): the same from set B's side.
 * pair_status_dev [ba, bb] int32, pair_first_dev, pair_undecided_dev [ba, bb] float64 (each may be null; self mode: [ba, ba],
 *   the diagonal FREE, +inf, +inf).
 * What the motion model costs.  For margin: a point of a box at distance <= reach from its origin, on a robot with speed <= v
 *   and turn rate <= w, moves at speed <= v + reach * w, so by the bound of nfopp_track_conflicts it stays within
 *   (v + reach * w) * dt / 2 of where the model puts it: (va + vb) * dt / 2 + (reach_a * wa + reach_b * wb) * dt / 2 in all.
 * workspace_dev: nfopp_box_track_conflicts_workspace_bytes(ba, bb, k) bytes (bb = 0 in self mode), rewritten by every call.
 * Everything runs on `stream`; nothing synchronises.  Argument errors, refused before any launch and never clamped: a negative
 *   batch size or one past 2^31 - 1, k < 1, a stride < 3, refine outside 0 .. NFOPP_BOX_CONFLICT_MAX_REFINE, dt not positive
 *   and finite, t0 or margin not finite, a null tracks / heading / box / summary pointer with tracks to read, more tiles of
 *   32 x 32 pairs than a grid holds, a workspace that is null or too small.  ba == 0 returns 0 and writes nothing. */
#define NFOPP_BOX_CONFLICT_MAX_REFINE 8
#define NFOPP_BOX_PAIR_BAD (-1)
#define NFOPP_BOX_PAIR_FREE 0
#define NFOPP_BOX_PAIR_CONFLICT 1
#define NFOPP_BOX_PAIR_UNDECIDED 2
#define NFOPP_NUM_BOX_CONFLICT_SLOTS 7
#define NFOPP_BOX_CONFLICT_SLOT_FIRST_TIME 0
#define NFOPP_BOX_CONFLICT_SLOT_FIRST_PARTNER 1
#define NFOPP_BOX_CONFLICT_SLOT_CONFLICTS 2
#define NFOPP_BOX_CONFLICT_SLOT_UNDECIDED_TIME 3
#define NFOPP_BOX_CONFLICT_SLOT_UNDECIDED_PARTNER 4
#define NFOPP_BOX_CONFLICT_SLOT_UNDECIDED 5
#define NFOPP_BOX_CONFLICT_SLOT_STATUS 6
int nfopp_track_headings(const float* tracks_dev, int64_t batch, int32_t stride, int32_t k, double* heading_dev, void* stream);
size_t nfopp_box_track_conflicts_workspace_bytes(int64_t ba, int64_t bb, int32_t k);
int nfopp_box_track_conflicts(const float* tracks_a_dev, const double* heading_a_dev, int64_t ba, int32_t stride_a,
                              const float* tracks_b_dev, const double* heading_b_dev, int64_t bb, int32_t stride_b, int32_t k,
                              double t0, double dt, const float* box_a_dev, const float* box_b_dev, const float* radius_a_dev,
                              const float* radius_b_dev, double margin, int32_t refine, double* summary_dev,
                              double* summary_b_dev, int32_t* pair_status_dev, double* pair_first_dev,
                              double* pair_undecided_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- prioritised start-delay scheduling of a fleet (csrc/fleet_schedule.hip), additive under ABI 6 ---------------------------
 * nfopp_track_conflicts tells which robots of a fleet are in conflict.  These two entries are the outer step: every robot
 * keeps its path and only WHEN it leaves changes.  In priority order each robot takes the smallest start delay, in steps of
 * the common time grid, that keeps it clear of every robot scheduled before it and of every predicted obstacle.  Predicates,
 * integer ORs and a count-trailing-zeros: no atomics, the same bits run after run, and the device is compared bit for bit
 * with the numpy restatement in tests/fleet_schedule_ref.py.
 *
 * Tracks.  tracks_dev [b, k, stride] fp32 on a common grid, x, y the first two floats of a row, stride >= 2 -- what
 *   nfopp_path_time_sample writes.  There are D = max_delay + 1 candidate delays 0 .. max_delay grid steps,
 *   0 <= max_delay <= NFOPP_SCHEDULE_MAX_DELAY.
 * A delayed robot.  Robot i delayed by q is at track_i[clamp(h - q, 0, k - 1)] at instant h: it waits at its first sample and
 *   stays parked at its last.  The caller chooses k so that the last sample is the goal.
 * Pair predicate C_ij(r) for a relative shift r = q_i - q_j in [-max_delay, max_delay]: the conflict predicate of
 *   nfopp_track_conflicts -- some m_n < R2_ij (strict), the last-instant term included, R_ij = (r_i + r_j) + margin, the same
 *   float64 arithmetic (one set of device functions, csrc/track_pairs.h, which both kernel files call and which also owns
 *   the map from a workgroup to its tile of pairs) -- applied to robot i delayed by max(r, 0) and robot j delayed by max(-r, 0), over k + |r| instants.
 *   Later instants add nothing: both robots are parked there and the last-instant term already holds that value, so the
 *   definition is independent of any horizon.  One of the two robots is never delayed: the assignment uses bit d - q_j for
 *   robot i at delay d against robot j at delay q_j, and in absolute time that pair only has min(d, q_j) more intervals in
 *   front, in which both wait at |d_0|^2, the c interval 0 starts from -- the predicate depends on the two delays through their
 *   difference
 *   alone.  By the evenness in the sign of d stated above, C_ji(-r) has the same bit as C_ij(r).
 * pair_mask_dev [b, b, 2] uint64, both triangles: the mask of a pair is 128 bits in two little-endian words, bit
 *   r + max_delay is C_ij(r), unused high bits are 0.  The diagonal is 0, a pair with a bad robot is 0, and mask_ji is mask_ij
 *   with its 2 * max_delay + 1 bits reversed (the kernel evaluates the upper triangle only and mirrors it).
 * Obstacles (optional: obstacles_dev null or m == 0).  obstacles_dev [m, k + max_delay, obstacle_stride] fp32 with
 *   obstacle_radius_dev [m] (null = 0), in absolute time, never shifted.  Bit d of base_mask_dev[i] is the same predicate for
 *   robot i delayed by d against obstacle j over all k + max_delay instants, ORed over the good obstacles j.
 * Bad tracks.  A robot or obstacle with a non-finite coordinate or radius is bad.  A bad obstacle is skipped by everyone.  A
 *   bad robot has bad_dev[i] = 1 (else 0), base 0, gets NFOPP_SCHEDULE_BAD_TRACK and delay -1, and is invisible to the others.
 * Assignment (nfopp_fleet_assign_delays, one workgroup).  order_dev [b] int32 (null: 0 .. b - 1) is visited front to back.  An
 *   entry out of range, or a robot already visited, is skipped (any int32 content is safe).  A robot never visited ends with
 *   NFOPP_SCHEDULE_NOT_ORDERED, delay -1, forbidden 0.  For robot i
 *     forbidden_i = (base_i | OR over the robots j scheduled before it of (mask_ij >> (max_delay - q_j))) & (2^D - 1),
 *   q_i = its lowest clear bit, status 0.  No clear bit: NFOPP_SCHEDULE_UNRESOLVED, delay -1; the robot is not on the floor for
 *   those after it and the schedule promises nothing about it (a caller can pass it back as a parked obstacle).
 *   delay_dev [b] int32, status_dev [b] int32, forbidden_dev [b] uint64 (may be null).
 * The two-step form lets a caller retry other priority orders -- the standard cure for an unresolved robot -- on the same
 *   masks at the cost of the assignment pass alone.
 * workspace_dev: nfopp_fleet_shift_masks_workspace_bytes(b, m) bytes (0 without obstacles), rewritten by every call (no
 *   initialisation needed).  All of pair_mask_dev, base_mask_dev and bad_dev is written.
 * Everything runs on `stream`; nothing synchronises.  Argument errors: a negative batch size or one above 2^31 - 1, max_delay
 *   outside 0 .. 63, k < 1 or too large for an index, a stride < 2, margin not finite, a null pointer where one is read or
 *   written, more tiles of 8 x 8 pairs than a grid holds (2^31 - 1), a workspace that is null or too small, more robots than
 *   the assignment pass can keep in one workgroup's LDS (one byte each in 160 KiB).  b == 0 returns 0 with null pointers. */
#define NFOPP_SCHEDULE_MAX_DELAY 63
#define NFOPP_SCHEDULE_BAD_TRACK 1
#define NFOPP_SCHEDULE_UNRESOLVED 2
#define NFOPP_SCHEDULE_NOT_ORDERED 3
size_t nfopp_fleet_shift_masks_workspace_bytes(int64_t b, int64_t m);
int nfopp_fleet_shift_masks(const float* tracks_dev, int64_t b, int32_t stride, int32_t k, const float* radius_dev,
                            double margin, int32_t max_delay, const float* obstacles_dev, int64_t m, int32_t obstacle_stride,
                            const float* obstacle_radius_dev, uint64_t* pair_mask_dev, uint64_t* base_mask_dev,
                            int32_t* bad_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int nfopp_fleet_assign_delays(const uint64_t* pair_mask_dev, const uint64_t* base_mask_dev, const int32_t* bad_dev,
                              const int32_t* order_dev, int64_t b, int32_t max_delay, int32_t* delay_dev, int32_t* status_dev,
                              uint64_t* forbidden_dev, void* stream);

/* ---- shift masks of oriented boxes for the scheduler (csrc/fleet_box_schedule.hip), additive under ABI 6 --------------------
 * nfopp_fleet_shift_masks shifts discs: a fleet of cars that nfopp_box_track_conflicts calls free can still be delayed by it,
 * or left NFOPP_SCHEDULE_UNRESOLVED.  nfopp_fleet_box_shift_masks writes masks of the same layout from the box check's rule;
 * nfopp_fleet_assign_delays reads them as they are.  Everything about tracks, delayed robots, masks, bad robots and obstacles
 * stays as nfopp_fleet_shift_masks states it; the pair predicate changes.  The device is compared bit for bit with the numpy
 * restatement in tests/fleet_box_schedule_ref.py when that is given the device's unit vectors.
 *
 * Tracks.  tracks_dev [b, k, stride >= 3] fp32, x, y, theta first in a row, and heading_dev [b, k, 2] float64 from
 *   nfopp_track_headings.  A robot delayed by q is at track[clamp(h - q, 0, k - 1)] at instant h, and its unit vector is
 *   gathered with the same clamped index.
 * Pair predicate C_ij(r): "the status of the pair is not NFOPP_BOX_PAIR_FREE" (CONFLICT or UNDECIDED) by the rule of
 *   nfopp_box_track_conflicts with the given refine, margin, boxes box_dev [b, 4] and rounding radii radius_dev [b] (null = 0)
 *   -- one set of device functions, csrc/box_pairs.h, which both kernel files call -- applied to robot i delayed by max(r, 0)
 *   and robot j delayed by max(-r, 0), over k + |r| instants.  UNDECIDED counts as forbidden: a schedule built from these masks
 *   is FREE by the box check, not merely free of conflicts.  dt and t0 do not enter (only times depend on them).
 * Order of the boxes.  The box arithmetic is not even in the order of the two boxes.  Only i < j is evaluated, with i as the
 *   first box, for every r; mask_ji is mask_ij with its 2 * max_delay + 1 bits reversed -- a copy, as in the box check's self
 *   mode.
 * Obstacles (optional: obstacles_dev null or m == 0).  obstacles_dev [m, k + max_delay, obstacle_stride >= 3] with
 *   obstacle_heading_dev [m, k + max_delay, 2], obstacle_box_dev [m, 4] and obstacle_radius_dev [m] (null = 0), in absolute
 *   time, never shifted.  Bit d of base_mask_dev[i]: the predicate on robot i delayed by d (the first box) against obstacle j
 *   (the second) over all k + max_delay instants, ORed over the good obstacles.
 * Bad tracks.  The box check's rule: a non-finite x, y, unit vector, box entry or radius, x0 >= x1 or y0 >= y1, or r < 0.  The
 *   consequences are those of nfopp_fleet_shift_masks.
 * Horizon.  In an interval where both robots stand still the poses at its two ends are the same.  Step 1 frees the pair when
 *   |d|^2 >= D2.  Otherwise step 2 reads the same sa that the neighbouring real interval (or the last-instant term) reads, and
 *   if step 2 finds no conflict, step 3 is ((sa + sa) - 0) * 0.5 - R >= 0 with sa - R >= 0: doubling and halving are exact, so
 *   it is FREE.  The waiting intervals in front and the parked intervals behind therefore add neither a CONFLICT nor an
 *   UNDECIDED, and the bit depends on the two delays through their difference alone, as for the discs.
 * pair_mask_dev [b, b, 2], base_mask_dev [b], bad_dev [b]: exactly the layout nfopp_fleet_assign_delays reads; all of the three
 *   is written.  workspace_dev: nfopp_fleet_box_shift_masks_workspace_bytes(b, m, k, max_delay) bytes (shape rows and obstacle
 *   partials; m = 0 without obstacles), rewritten by every call.
 * Everything runs on `stream`; nothing synchronises.  Arguments refused before any launch: a negative batch size or one above
 *   2^31 - 1, max_delay outside 0 .. 63, k < 1 or too large for an index, a stride < 3, refine outside
 *   0 .. NFOPP_BOX_CONFLICT_MAX_REFINE, margin not finite, a null tracks / heading / box / mask / bad pointer, a null obstacle
 *   heading or box pointer with obstacles to read, more tiles of 8 x 8 pairs than a grid holds, a workspace that is null or
 *   too small.  b == 0 returns 0 with null pointers. */
size_t nfopp_fleet_box_shift_masks_workspace_bytes(int64_t b, int64_t m, int32_t k, int32_t max_delay);
int nfopp_fleet_box_shift_masks(const float* tracks_dev, const double* heading_dev, int64_t b, int32_t stride, int32_t k,
                                const float* box_dev, const float* radius_dev, double margin, int32_t refine,
                                int32_t max_delay, const float* obstacles_dev, const double* obstacle_heading_dev, int64_t m,
                                int32_t obstacle_stride, const float* obstacle_box_dev, const float* obstacle_radius_dev,
                                uint64_t* pair_mask_dev, uint64_t* base_mask_dev, int32_t* bad_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream);

/* ---- space-time grid search for the robots a schedule cannot place (csrc/spacetime_search.hip), additive under ABI 6 ---------
 * nfopp_fleet_assign_delays ends with robots it cannot place: a robot placed before them waits on their path, crosses it at the
 * wrong time or parks on it for good, and no re-timing of a fixed path gets round that.  These entries give such a robot
 * another path, chosen with time in it: an earliest-arrival search on an occupancy grid against what is already reserved.
 * Predicates and integer ORs only, the same bits run after run; the device is compared bit for bit with the numpy restatement
 * in tests/spacetime_ref.py.
 *
 * Grid.  occupancy_dev [rows, cols] uint8, non-zero = wall, with the geometry of the grid search above: the float64 centre of
 *   cell (row, col) is  col * res + res / 2 + b0  (x) and  row * res + res / 2 + b2  (y), every operation rounded on its own,
 *   left to right.  The centre used everywhere is that value rounded to fp32: it is what the output tracks hold and, widened,
 *   what the predicate reads.  The caller inflates the image for the robot's footprint.
 * Time.  t >= 1 instants on the callers' common time grid.  dt does not enter: everything is per tick.
 * Moves.  In one tick a robot stays or moves to one of its 8 neighbours (the move set of the grid search with no corner rule;
 *   cells outside the image are walls).  A move takes one tick whatever its length: the caller chooses
 *   dt >= sqrt(2) * res / v_max.  Directions d = 0 .. 8 as (drow, dcol):
 *     (0,+1) (0,-1) (+1,0) (-1,0) (+1,+1) (+1,-1) (-1,+1) (-1,-1) (0,0) -- the wait is last.
 * Movers.  tracks_dev [m, t, stride >= 2] fp32 in absolute time, never shifted, radius_dev [m] (null = 0) and visible_dev [m]
 *   uint8 (null = all visible).  A track with a non-finite coordinate or radius is bad and skipped.
 * Edge predicate.  Edge (u, d, h) is the robot going from cell u at instant h to v = u + d at h + 1.  It is blocked if v is
 *   outside the image or a wall, or if some visible good mover j gives the conflict predicate of nfopp_track_conflicts on this
 *   one interval: d0 = centre(u) - p_j[h], d1 = centre(v) - p_j[h + 1], m the closest approach of the interval, blocked when
 *   m < R2_j (strict), R_j = (robot_radius + r_j) + margin, R2_j = R_j * R_j -- the same float64 arithmetic, the same device
 *   functions (csrc/track_pairs.h).  last[u] is the last-instant term: |centre(u) - p_j[t - 1]|^2 < R2_j for some such j.
 *   There is one robot_radius (an fp32 value) for the whole planned fleet: the reservation then does not depend on which robot
 *   is being planned and can be accumulated.
 * Reservation.  uint64 words, W = (cols + 63) / 64 words a row, bit c % 64 of word c / 64 is column c:
 *     blocked [t - 1][9][rows][W]   bit = edge (u, d, h) is blocked, indexed by the source cell u
 *     last    [rows][W]             follows it
 *   nfopp_spacetime_reservation_bytes(rows, cols, t) bytes in all (0: not an image and t an int32 indexes).  The padding bits of
 *   a row (columns >= cols) are 1 in blocked and 0 in last.  nfopp_spacetime_reservation_init writes the static part (walls,
 *   the image edge, the padding) and clears last -- every word of the reservation is written, for t = 1 (no blocked part)
 *   too, so the buffer needs no initialisation; nfopp_spacetime_reserve ORs the movers' bits in -- OR is order-free, so
 *   reserving a set of tracks in two calls gives the bits of one call.  Its workspace: nfopp_spacetime_reserve_workspace_bytes(m),
 *   no initialisation needed.
 * Search of one robot, start cell s, goal cell g.  reach_0 = {s}; reach_{h+1}[v] = OR over d of (reach_h[v - d] and edge
 *   (v - d, d, h) not blocked).  park[t - 1] = !last[g]; park[h] = park[h + 1] and wait edge (g, 8, h) not blocked.  Arrival
 *   h* = the smallest h with reach_h[g] and park[h].  Path: cell[h] = g for h >= h*; backwards from (g, h*) the predecessor
 *   of (v, h) is v - d for the lowest d with reach_{h-1}[v - d] and edge (v - d, d, h - 1) not blocked; it ends at (s, 0) by
 *   construction.
 * Statuses.  0 planned; NFOPP_SPACETIME_BAD_CELL: start or goal outside the image or on a wall; NFOPP_SPACETIME_UNREACHED: no
 *   such h*; NFOPP_SPACETIME_NOT_ORDERED: never visited.  A robot that is not planned has arrival -1, cells all -1 and NaN track
 *   rows, and reserves nothing: it is not on the floor for those after it, as an unresolved robot of the schedule is not.
 * Fleet (nfopp_spacetime_plan_fleet).  start_cells_dev / goal_cells_dev [robots, 2] int32 (row, col).  order_dev [robots] int32
 *   (null: 0 .. robots - 1) is visited front to back; an entry out of range or a robot already visited is skipped on the
 *   device, before anything is indexed by it (any int32 content is safe).  Each planned robot's output track (fp32 centres,
 *   radius robot_radius) is reserved before the next robot is searched, so robot k's predicate against robot k' < k is the
 *   predicate of nfopp_track_conflicts on the two output tracks, bit for bit: "nobody planned is in conflict, by
 *   nfopp_track_conflicts itself" holds by construction, not by tolerance.  reservation_dev is read and written: the caller
 *   initialises it and reserves the movers first.  Outputs: cells_dev [robots, t] int32 flat index row * cols + col,
 *   arrival_dev [robots], status_dev [robots], tracks_dev [robots, t, 2] fp32.  workspace_dev:
 *   nfopp_spacetime_plan_workspace_bytes(rows, cols, t, robots) bytes (reach of every instant, t * rows * W * 8, and a word
 *   of state per robot; no initialisation needed).  Every element of the four outputs is written.  One search launch (one
 *   workgroup, both frontiers in LDS) and one reserve launch per order position,
 *   all on `stream`; nothing synchronises, no kernel waits on another workgroup.
 * The snap.  A planned track starts at the centre of the robot's start cell, up to res / sqrt(2) from where the robot stands:
 *   the caller adds that to margin.  Grid tracks are seeds and timetables, not smooth trajectories.
 * Argument errors, nothing is clamped: t < 1, an empty image, an image and t whose bitmaps overflow an int32 index, a frontier
 *   larger than one workgroup's LDS (2 * rows * W * 8 + 64 bytes in 160 KiB), a reservation or workspace that is null or too
 *   small, a null pointer where one is read or written, a stride < 2, a negative batch size, a geometry value, robot_radius or
 *   margin that is not finite, a resolution <= 0.  robots == 0 and m == 0 return 0. */
#define NFOPP_SPACETIME_BAD_CELL 1
#define NFOPP_SPACETIME_UNREACHED 2
#define NFOPP_SPACETIME_NOT_ORDERED 3
size_t nfopp_spacetime_reservation_bytes(int32_t rows, int32_t cols, int32_t t);
int nfopp_spacetime_reservation_init(const uint8_t* occupancy_dev, int32_t rows, int32_t cols, int32_t t,
                                     uint64_t* reservation_dev, size_t reservation_bytes, void* stream);
size_t nfopp_spacetime_reserve_workspace_bytes(int64_t m);
int nfopp_spacetime_reserve(int32_t rows, int32_t cols, int32_t t, double b0, double b2, double resolution, float robot_radius,
                            double margin, const float* tracks_dev, int64_t m, int32_t stride, const float* radius_dev,
                            const uint8_t* visible_dev, uint64_t* reservation_dev, size_t reservation_bytes,
                            void* workspace_dev, size_t workspace_bytes, void* stream);
size_t nfopp_spacetime_plan_workspace_bytes(int32_t rows, int32_t cols, int32_t t, int64_t robots);
int nfopp_spacetime_plan_fleet(const uint8_t* occupancy_dev, int32_t rows, int32_t cols, int32_t t, double b0, double b2,
                               double resolution, float robot_radius, double margin, const int32_t* start_cells_dev,
                               const int32_t* goal_cells_dev, const int32_t* order_dev, int64_t robots,
                               uint64_t* reservation_dev, size_t reservation_bytes, int32_t* cells_dev, int32_t* arrival_dev,
                               int32_t* status_dev, float* tracks_dev, void* workspace_dev, size_t workspace_bytes,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NFOPP_HIP_H */
