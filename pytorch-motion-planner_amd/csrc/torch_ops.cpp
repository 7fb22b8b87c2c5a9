// torch.ops.nfopp.* -- the PyTorch-ROCm extension form of the drop-in boundary (last row; BASELINE
// north_star: "exposed as a PyTorch-ROCm extension").  A thin TORCH_LIBRARY shim over the C ABI of include/nfopp_hip.h:
// every op checks device / dtype / contiguity / shapes with TORCH_CHECK at the op boundary, takes the CURRENT HIP stream of
// the tensors' device, and calls the extern "C" entry point -- no arithmetic lives here.  Built as
// nfopp/lib/libnfopp_torch.so (links libnfopp_hip.so from the same directory); loaded with torch.ops.load_library.
//
// Reference side these ops stand in for: the autograd graph of ONF.forward (nfop/onf_model.py:33-50), one
// `_optimize_trajectory` (nfop/nerf_opt_planner.py:143-155, nfop/constrained_nerf_opt_planner.py:63-130), the
// reparametrisation (constrained:132-171, nerf:224-244) and one `_optimize_collision_model` step (nerf:76-91).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>    // PyTorch-ROCm names its HIP devices "cuda": these are the
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>       // guard / stream types that accept that device type
#include <torch/library.h>

#include <limits>

#include "nfopp_hip.h"

namespace {

using at::Tensor;
using OptTensor = std::optional<Tensor>;

void check_tensor(const Tensor& t, const char* name, at::ScalarType dtype = at::kFloat) {
  TORCH_CHECK(t.is_cuda(), "nfopp: ", name, " must live on a HIP device (got ", t.device(), "); there is no CPU path");
  TORCH_CHECK(t.scalar_type() == dtype, "nfopp: ", name, " must be ", dtype, " (got ", t.scalar_type(), ")");
  TORCH_CHECK(t.is_contiguous(), "nfopp: ", name, " must be contiguous");
}
void same_device(const Tensor& a, const Tensor& b, const char* name) {
  TORCH_CHECK(a.device() == b.device(), "nfopp: ", name, " lives on ", b.device(), ", expected ", a.device());
}
// x belongs beside `first`: of `dtype`, contiguous, on its device
void beside(const Tensor& first, const Tensor& x, const char* name, at::ScalarType dtype = at::kFloat) {
  check_tensor(x, name, dtype);
  same_device(first, x, name);
}
// ... and of exactly this shape
void need(const Tensor& first, const Tensor& x, const char* name, at::IntArrayRef shape, at::ScalarType dtype = at::kFloat) {
  beside(first, x, name, dtype);
  TORCH_CHECK(x.sizes() == shape, "nfopp: ", name, " must have shape ", shape, ", got ", x.sizes());
}
void need_if_given(const Tensor& first, const OptTensor& x, const char* name, at::IntArrayRef shape, at::ScalarType dtype = at::kFloat) {
  if (x.has_value()) need(first, *x, name, shape, dtype);
}
// The one statement of "pointer, or null when there is nothing": a tensor that is absent, undefined or empty gives null.  Every
// pointer an entry may receive as null comes from here; a site whose null follows another rule says so ("own condition").
template <class T>
T* ptr(const Tensor& t) { return (t.defined() && t.numel() > 0) ? t.data_ptr<T>() : nullptr; }
template <class T>
T* ptr(const OptTensor& t) { return t.has_value() ? ptr<T>(*t) : nullptr; }
// the uint64 words an int64 tensor holds
uint64_t* words_ptr(const Tensor& t) { return reinterpret_cast<uint64_t*>(ptr<int64_t>(t)); }
// the workspace of an op: `bytes` bytes on the device of `like` (the entries' 8-byte alignment is the device allocator's)
struct Workspace {
  Tensor buffer;
  size_t bytes;
  Workspace(const Tensor& like, size_t n) : buffer(at::empty({(int64_t)n}, like.options().dtype(at::kByte))), bytes(n) {}
  void* ptr() const { return bytes ? buffer.data_ptr() : nullptr; }
};
// what an op holds while it launches: the device of its tensors made current, and the CURRENT HIP stream of that device
struct Launch {
  c10::hip::HIPGuardMasqueradingAsCUDA guard;
  void* stream;
  explicit Launch(const Tensor& t)
      : guard(t.device()), stream((void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.get_device()).stream()) {}
};
void check_status(int rc) { TORCH_CHECK(rc == 0, "nfopp call failed (", rc, "): ", nfopp_last_error()); }

nfopp_onf_config make_cfg(double mean, double sigma, bool use_cos, bool has_bias, int64_t angle_dim) {
  nfopp_onf_config c;
  c.mean = (float)mean; c.sigma = (float)sigma; c.use_cos = use_cos; c.has_bias = has_bias; c.angle_dim = (int32_t)angle_dim;
  return c;
}
void check_params(const Tensor& params, const nfopp_onf_config& c) {
  check_tensor(params, "params");
  const int64_t want = nfopp_onf_param_count(&c);
  TORCH_CHECK(want > 0, "nfopp: bad ONF configuration");
  TORCH_CHECK(params.numel() == want, "nfopp: params has ", params.numel(), " elements, this ONF configuration has ", want);
}
// x is [P, 2] or, for an ONF with angle features, [P, 3]
void check_point_rows(const Tensor& x, const char* name, int64_t angle_dim) {
  const int64_t dim = angle_dim > 0 ? 3 : 2;
  TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "nfopp: ", name, " must be [P, ", dim, "]");
}

// the 18 floats of nfopp_traj_hyper in declaration order
nfopp_traj_hyper make_hyper(at::ArrayRef<double> h) {
  TORCH_CHECK(h.size() == 18, "nfopp: hyper must hold the 18 floats of nfopp_traj_hyper (include/nfopp_hip.h), got ", h.size());
  nfopp_traj_hyper o;
  float* f = reinterpret_cast<float*>(&o);
  static_assert(sizeof(nfopp_traj_hyper) == 18 * sizeof(float), "nfopp_traj_hyper layout");
  for (int k = 0; k < 18; ++k) f[k] = (float)h[k];
  return o;
}

// What onf_fwd_bwd_input and onf_logits share: params and points [P, dim] through `entry` -> its [P, 4] rows
using OnfPointsEntry = int (*)(const nfopp_onf_config*, const float*, const float*, int64_t, float*, void*);
Tensor onf_points(OnfPointsEntry entry, const Tensor& params, const Tensor& points, const nfopp_onf_config& c, int64_t angle_dim) {
  check_params(params, c);
  beside(params, points, "points");
  check_point_rows(points, "points", angle_dim);
  const Launch on(params);
  Tensor out = at::empty({points.size(0), 4}, points.options());
  check_status(entry(&c, params.data_ptr<float>(), points.data_ptr<float>(), points.size(0), out.data_ptr<float>(), on.stream));
  return out;
}

// ONF.forward + autograd w.r.t. the input (nfop/onf_model.py:33-50): out [P, 4] = logit, d/dx, d/dy, d/dtheta
Tensor onf_fwd_bwd_input(const Tensor& params, const Tensor& points, double mean, double sigma, bool use_cos, bool has_bias,
                         int64_t angle_dim) {
  return onf_points(nfopp_onf_eval_points, params, points, make_cfg(mean, sigma, use_cos, has_bias, angle_dim), angle_dim);
}

// forward only (nfop/nerf_opt_planner.py:98-99,122-125): out [P, 1]
Tensor onf_logits(const Tensor& params, const Tensor& points, double mean, double sigma, bool use_cos, bool has_bias,
                  int64_t angle_dim) {
  return onf_points(nfopp_onf_eval_logits, params, points, make_cfg(mean, sigma, use_cos, has_bias, angle_dim), angle_dim)
      .narrow(1, 0, 1);
}

// The state tensors of a batch of B trajectories, stated once for every op that takes them: traj [B, N, D], start / goal
// [B, D], the SE(2) multipliers lam [B, N+1] / cm [B, N] (D == 3: both; D == 2: neither), the reparametrisation grid u [N]
// and a uint8 row mask [B] with the int32 live-list workspace (>= B + 1) the ONF kernel needs beside it.
struct Batch {
  int64_t B = 0, N = 0, D = 0;
  float *traj = nullptr, *start = nullptr, *goal = nullptr, *lam = nullptr, *cm = nullptr, *u = nullptr;
  uint8_t* mask = nullptr;
  int32_t* live_ws = nullptr;
};

// traj, start and goal alone (the grid search seeds a batch that has no multipliers yet)
Batch batch_endpoints(const Tensor& traj, const Tensor& start, const Tensor& goal) {
  check_tensor(traj, "traj");
  TORCH_CHECK(traj.dim() == 3, "nfopp: traj must be [B, N, D]");
  Batch b;
  b.B = traj.size(0); b.N = traj.size(1); b.D = traj.size(2);
  TORCH_CHECK(b.D == 2 || b.D == 3, "nfopp: trajectory dim must be 2 or 3");
  need(traj, start, "start", {b.B, b.D}); need(traj, goal, "goal", {b.B, b.D});
  b.traj = traj.data_ptr<float>(); b.start = start.data_ptr<float>(); b.goal = goal.data_ptr<float>();
  return b;
}

// `u`, `mask` and `live_ws` are null for an op that has no such argument; `mask_name` is the op's name for its row mask
Batch batch_state(const Tensor& traj, const Tensor& start, const Tensor& goal, const OptTensor& lam, const OptTensor& cm,
                  const Tensor* u, const OptTensor* mask, const char* mask_name, const OptTensor* live_ws) {
  Batch b = batch_endpoints(traj, start, goal);
  TORCH_CHECK(b.N >= 2, "nfopp: need at least 2 waypoints");
  if (b.D == 3) {
    TORCH_CHECK(lam.has_value() && cm.has_value(), "nfopp: an SE(2) batch needs the multiplier tensors lam [B, N+1], cm [B, N]");
    need(traj, *lam, "lam", {b.B, b.N + 1}); need(traj, *cm, "cm", {b.B, b.N});
    b.lam = lam->data_ptr<float>(); b.cm = cm->data_ptr<float>();
  } else {
    // a 2-D batch has no multipliers: a tensor passed here would reach the kernel unvalidated
    TORCH_CHECK(!lam.has_value() && !cm.has_value(), "nfopp: a 2-D batch takes no multiplier tensors (lam / cm must be None)");
  }
  if (u) {
    need(traj, *u, "u", {b.N});
    b.u = u->data_ptr<float>();
  }
  const bool masked = mask && mask->has_value();
  if (masked) {
    need(traj, **mask, mask_name, {b.B}, at::kByte);
    b.mask = (*mask)->data_ptr<uint8_t>();
  }
  if (live_ws && masked) {
    TORCH_CHECK(live_ws->has_value(), "nfopp: an active mask needs the live-list workspace (B + 1 int32)");
    beside(traj, **live_ws, "live_ws", at::kInt);
    TORCH_CHECK((*live_ws)->numel() >= b.B + 1, "nfopp: live_ws must hold B + 1 int32");
    b.live_ws = (*live_ws)->data_ptr<int32_t>();
  } else if (live_ws) {
    TORCH_CHECK(!live_ws->has_value(), "nfopp: live_ws without an active mask");
  }
  return b;
}

// what traj_step and traj_steps check beyond the batch: the ONF, the Adam moments, the per-step scratch, the band
Batch step_state(const Tensor& params, const nfopp_onf_config& c, int64_t angle_dim, const Tensor& traj, const Tensor& start,
                 const Tensor& goal, const OptTensor& lam, const OptTensor& cm, const Tensor& adam_m, const Tensor& adam_v,
                 const Tensor& t, const Tensor& onf_out, const Tensor& hinv_band, int64_t half_width, const Tensor* u,
                 const OptTensor& terms, const OptTensor& active, const OptTensor& live_ws) {
  check_params(params, c);
  const Batch b = batch_state(traj, start, goal, lam, cm, u, &active, "active", &live_ws);
  TORCH_CHECK(b.D == (angle_dim > 0 ? 3 : 2), "nfopp: trajectory dim ", b.D, " does not match the ONF point dim");
  same_device(traj, params, "params");
  need(traj, adam_m, "adam_m", {b.B, b.N, b.D}); need(traj, adam_v, "adam_v", {b.B, b.N, b.D});
  need(traj, t, "t", {b.B, b.N - 1}); need(traj, onf_out, "onf_out", {b.B, b.N - 1, 4});
  need(traj, hinv_band, "hinv_band", {2 * half_width + 1, b.N});
  need_if_given(traj, terms, "terms", {b.B, NFOPP_NUM_TERMS});
  return b;
}

// one `_optimize_trajectory` for a batch: collision sampling + ONF (nfopp_traj_collision_eval), then losses, H^-1 g, Adam and
// the multiplier ascent (nfopp_traj_update).  State tensors are updated in place.
void traj_step(const Tensor& params, double mean, double sigma, bool use_cos, bool has_bias, int64_t angle_dim, Tensor traj,
               const Tensor& start, const Tensor& goal, const OptTensor& lam, const OptTensor& cm, Tensor adam_m, Tensor adam_v,
               Tensor t, int64_t t_mode, int64_t seed, int64_t rng_offset, int64_t traj_index_offset, Tensor onf_out,
               const Tensor& hinv_band, int64_t half_width, int64_t interior_lo, int64_t interior_hi, at::ArrayRef<double> hyper,
               const OptTensor& terms, const OptTensor& active, const OptTensor& live_ws) {
  const nfopp_onf_config c = make_cfg(mean, sigma, use_cos, has_bias, angle_dim);
  const Batch b = step_state(params, c, angle_dim, traj, start, goal, lam, cm, adam_m, adam_v, t, onf_out, hinv_band, half_width,
                             nullptr, terms, active, live_ws);
  const nfopp_traj_hyper hp = make_hyper(hyper);
  const Launch on(traj);
  check_status(nfopp_traj_collision_eval(&c, params.data_ptr<float>(), b.traj, b.B, (int32_t)b.N, (int32_t)b.D,
                                         t.data_ptr<float>(), (int32_t)t_mode, (uint64_t)seed, (uint64_t)rng_offset,
                                         traj_index_offset, onf_out.data_ptr<float>(), b.mask, b.live_ws, on.stream));
  check_status(nfopp_traj_update(&hp, b.B, (int32_t)b.N, (int32_t)b.D, b.traj, b.start, b.goal, b.lam, b.cm,
                                 adam_m.data_ptr<float>(), adam_v.data_ptr<float>(), t.data_ptr<float>(),
                                 onf_out.data_ptr<float>(), hinv_band.data_ptr<float>(), (int32_t)half_width,
                                 (int32_t)interior_lo, (int32_t)interior_hi, ptr<float>(terms), b.mask, on.stream));
}

// n frozen-field planner steps from one call (nfopp_traj_steps, ABI 6): the callers' step loops
// (nfop/ros/goal_planner_adapter.py:50-52, scripts/run_planner.py:76-77) without a host round trip per step.
// t_steps: [n_steps, B, N-1] injected draws (t_mode 0) or None (t_mode 1, in-kernel Philox; `t` is the scratch row).
void traj_steps(const Tensor& params, double mean, double sigma, bool use_cos, bool has_bias, int64_t angle_dim, Tensor traj,
                const Tensor& start, const Tensor& goal, const OptTensor& lam, const OptTensor& cm, Tensor adam_m, Tensor adam_v,
                Tensor t, const OptTensor& t_steps, int64_t seed, int64_t rng_offset, int64_t traj_index_offset, Tensor onf_out,
                const Tensor& hinv_band, int64_t half_width, int64_t interior_lo, int64_t interior_hi, const Tensor& u,
                at::ArrayRef<double> hyper, double adam_lr, double adam_beta1, double adam_beta2, int64_t adam_steps_done,
                int64_t step_count, int64_t reparam_freq, int64_t n_steps, const OptTensor& terms, const OptTensor& active,
                const OptTensor& live_ws) {
  const nfopp_onf_config c = make_cfg(mean, sigma, use_cos, has_bias, angle_dim);
  const Batch b = step_state(params, c, angle_dim, traj, start, goal, lam, cm, adam_m, adam_v, t, onf_out, hinv_band, half_width,
                             &u, terms, active, live_ws);
  TORCH_CHECK(n_steps >= 0 && reparam_freq >= 1 && adam_steps_done >= 0 && step_count >= 0, "nfopp: bad step schedule");
  need_if_given(traj, t_steps, "t_steps", {n_steps, b.B, b.N - 1});
  const nfopp_traj_hyper hp = make_hyper(hyper);
  const nfopp_traj_buffers buf = {b.traj, b.start, b.goal, b.lam, b.cm, adam_m.data_ptr<float>(), adam_v.data_ptr<float>(),
                                  t.data_ptr<float>(), onf_out.data_ptr<float>(), hinv_band.data_ptr<float>(), b.u, b.mask,
                                  b.live_ws, b.B, (int32_t)b.N, (int32_t)b.D, (int32_t)half_width, (int32_t)interior_lo,
                                  (int32_t)interior_hi};
  nfopp_step_schedule sc;
  sc.adam_lr = adam_lr; sc.adam_beta1 = adam_beta1; sc.adam_beta2 = adam_beta2;
  sc.adam_steps_done = adam_steps_done; sc.step_count = step_count; sc.traj_index_offset = traj_index_offset;
  sc.seed = (uint64_t)seed; sc.rng_offset = (uint64_t)rng_offset; sc.reparam_freq = (int32_t)reparam_freq;
  sc.t_mode = t_steps.has_value() ? 0 : 1;
  const Launch on(traj);
  check_status(nfopp_traj_steps(&c, params.data_ptr<float>(), &hp, &buf, &sc, (int32_t)n_steps, ptr<float>(t_steps),
                                ptr<float>(terms), on.stream));
}

// arc-length reparametrisation (constrained:132-171 / nerf:224-244), in place
void reparametrize(Tensor traj, const Tensor& start, const Tensor& goal, const OptTensor& lam, const OptTensor& cm,
                   const Tensor& u, const OptTensor& active) {
  const Batch b = batch_state(traj, start, goal, lam, cm, &u, &active, "active", nullptr);
  const Launch on(traj);
  check_status(nfopp_reparametrize(b.B, (int32_t)b.N, (int32_t)b.D, b.traj, b.start, b.goal, b.lam, b.cm, b.u, b.mask, on.stream));
}

// start (which = 0) / goal (which = 1) update of a batch (constrained:178-194 / nerf:202-218), in place: nearest waypoint,
// cut, endpoint write and reparametrisation from one launch.  moved [B] uint8 or None (= all); min_index [B] int32 or None.
void update_endpoints(Tensor traj, Tensor start, Tensor goal, const OptTensor& lam, const OptTensor& cm, const Tensor& u,
                      const Tensor& points, int64_t which, const OptTensor& moved, const OptTensor& min_index) {
  const Batch b = batch_state(traj, start, goal, lam, cm, &u, &moved, "moved", nullptr);
  TORCH_CHECK(which == 0 || which == 1, "nfopp: which must be 0 (start) or 1 (goal)");
  need(traj, points, "points", {b.B, b.D});
  need_if_given(traj, min_index, "min_index", {b.B}, at::kInt);
  const Launch on(traj);
  check_status(nfopp_update_endpoints(b.B, (int32_t)b.N, (int32_t)b.D, (int32_t)which, points.data_ptr<float>(), b.mask, b.traj,
                                      b.start, b.goal, b.lam, b.cm, b.u, ptr<int32_t>(min_index), on.stream));
}

// grid-search (A*) seeding of a batch (astar_trajectory_initializer.py:15-48): traj [B, N, D] in place, returns status [B].
// occupancy uint8 [rows, cols]; start_cells / goal_cells int32 [B, 2] (row, col); unique_goal_cells int32 [G, 2] and
// field_index int32 [B] = the de-duplicated goal cells and each problem's entry in them (nfopp/grid_search.py builds them).
Tensor grid_search_init(Tensor traj, const Tensor& start, const Tensor& goal, const Tensor& occupancy, const Tensor& start_cells,
                        const Tensor& goal_cells, const Tensor& unique_goal_cells, const Tensor& field_index, double origin_x,
                        double origin_y, double resolution, bool angles_with_direction) {
  const Batch b = batch_endpoints(traj, start, goal);
  const int64_t B = b.B, N = b.N, D = b.D;
  beside(traj, occupancy, "occupancy", at::kByte);
  beside(traj, start_cells, "start_cells", at::kInt); beside(traj, goal_cells, "goal_cells", at::kInt);
  beside(traj, unique_goal_cells, "unique_goal_cells", at::kInt); beside(traj, field_index, "field_index", at::kInt);
  TORCH_CHECK(occupancy.dim() == 2, "nfopp: occupancy must be [rows, cols] uint8");
  // the cells and the index are taken by their element counts (a flat [2 B] start_cells passes), so `need` does not state them
  TORCH_CHECK(start_cells.numel() == 2 * B && goal_cells.numel() == 2 * B && field_index.numel() == B,
              "nfopp: start_cells / goal_cells must be [B, 2], field_index [B]");
  TORCH_CHECK(unique_goal_cells.dim() == 2 && unique_goal_cells.size(1) == 2, "nfopp: unique_goal_cells must be [G, 2]");
  const int64_t rows = occupancy.size(0), cols = occupancy.size(1), G = unique_goal_cells.size(0);
  const Launch on(traj);
  const auto i32 = traj.options().dtype(at::kInt);
  Tensor fields = at::empty({G, rows, cols, 2}, i32);
  const Workspace fwork(traj, nfopp_grid_fields_workspace_bytes((int32_t)rows, (int32_t)cols, G));
  check_status(nfopp_grid_distance_fields(occupancy.data_ptr<uint8_t>(), (int32_t)rows, (int32_t)cols,
                                          unique_goal_cells.data_ptr<int32_t>(), G, fields.data_ptr<int32_t>(), fwork.ptr(),
                                          fwork.bytes, on.stream));
  Tensor count = at::empty({B}, i32), status = at::empty({B}, i32);
  auto trace = [&](int32_t max_len, int32_t* cells) {
    check_status(nfopp_grid_trace_paths(ptr<int32_t>(fields), G, (int32_t)rows, (int32_t)cols,
                                        start_cells.data_ptr<int32_t>(), goal_cells.data_ptr<int32_t>(),
                                        field_index.data_ptr<int32_t>(), B, max_len, cells, count.data_ptr<int32_t>(),
                                        status.data_ptr<int32_t>(), nullptr, on.stream));
  };
  trace(0, nullptr);
  const int64_t max_len = B ? std::max<int64_t>(count.max().item<int64_t>(), 1) : 1;
  Tensor cells = at::zeros({B, max_len, 2}, i32);
  trace((int32_t)max_len, cells.data_ptr<int32_t>());
  const Workspace swork(traj, nfopp_grid_seed_workspace_bytes(B, (int32_t)max_len));
  check_status(nfopp_grid_seed_trajectories(cells.data_ptr<int32_t>(), count.data_ptr<int32_t>(), status.data_ptr<int32_t>(), B,
                                            (int32_t)max_len, b.start, b.goal, (int32_t)N, (int32_t)D,
                                            angles_with_direction ? 1 : 0, origin_x, origin_y, resolution, b.traj, swork.ptr(),
                                            swork.bytes, on.stream));
  return status;
}

// gradient of the BCE-with-logits fitting loss w.r.t. every ONF parameter (nerf:83-89): [n_params | loss | count]
Tensor onf_train_grad(const Tensor& params, const Tensor& samples, const Tensor& labels, double inv_count, double mean,
                      double sigma, bool use_cos, bool has_bias, int64_t angle_dim) {
  const nfopp_onf_config c = make_cfg(mean, sigma, use_cos, has_bias, angle_dim);
  check_params(params, c);
  beside(params, samples, "samples"); beside(params, labels, "labels");
  check_point_rows(samples, "samples", angle_dim);
  TORCH_CHECK(labels.numel() == samples.size(0), "nfopp: labels must be [P]");
  const Launch on(params);
  const int64_t P = samples.size(0);
  const size_t ws_bytes = nfopp_onf_train_workspace_bytes(&c, P);
  Tensor ws = at::empty({(int64_t)((ws_bytes + 3) / 4)}, params.options());
  Tensor grad = at::empty({params.numel() + 2}, params.options());
  check_status(nfopp_onf_train_grad(&c, params.data_ptr<float>(), samples.data_ptr<float>(), labels.data_ptr<float>(), P,
                                    (float)inv_count, grad.data_ptr<float>(), ws.data_ptr<float>(), ws_bytes, on.stream));
  return grad;
}

// torch.optim.Adam single-tensor update on the flat parameter buffer (nerf:90), in place
void adam_step(Tensor param, const Tensor& grad, Tensor m, Tensor v, double beta2, double omb1, double omb2, double eps,
               double step_size, double bc2_sqrt) {
  check_tensor(param, "param");
  beside(param, grad, "grad"); beside(param, m, "m"); beside(param, v, "v");
  const int64_t n = param.numel();
  TORCH_CHECK(grad.numel() >= n && m.numel() == n && v.numel() == n, "nfopp: grad / m / v must cover the ", n, " parameters");
  const Launch on(param);
  check_status(nfopp_adam_step(param.data_ptr<float>(), grad.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), n,
                               (float)beta2, (float)omb1, (float)omb2, (float)eps, (float)step_size, (float)bc2_sqrt, on.stream));
}

// one `_optimize_collision_model` step on one GPU: gradient + Adam (multi-GPU callers all-reduce the gradient in between:
// nfopp/batch.py OnfFitter).  Returns the gradient buffer (its [-2] entry is the loss).
Tensor onf_train_step(Tensor params, Tensor m, Tensor v, const Tensor& samples, const Tensor& labels, double mean, double sigma,
                      bool use_cos, bool has_bias, int64_t angle_dim, double beta2, double omb1, double omb2, double eps,
                      double step_size, double bc2_sqrt) {
  TORCH_CHECK(samples.dim() == 2 && samples.size(0) > 0, "nfopp: samples must be [P, D] with P > 0");
  Tensor grad = onf_train_grad(params, samples, labels, 1.0 / (double)samples.size(0), mean, sigma, use_cos, has_bias, angle_dim);
  adam_step(params, grad, m, v, beta2, omb1, omb2, eps, step_size, bc2_sqrt);
  return grad;
}

// the 6 doubles of nfopp_motion_limits in declaration order
nfopp_motion_limits make_limits(at::ArrayRef<double> l) {
  TORCH_CHECK(l.size() == 6, "nfopp: limits must hold the 6 doubles of nfopp_motion_limits (include/nfopp_hip.h), got ", l.size());
  static_assert(sizeof(nfopp_motion_limits) == 6 * sizeof(double), "nfopp_motion_limits layout");
  return nfopp_motion_limits{l[0], l[1], l[2], l[3], l[4], l[5]};
}

// velocity profile of a batch of paths under motion limits (nfopp_path_time_profile): (profile [B, N+2, 4] float64,
// gear [B, N+1] int8, summary [B, 4] float64).  v_start / v_goal: [B] fp32 or None (rest).
std::tuple<Tensor, Tensor, Tensor> path_time_profile(const Tensor& traj, const Tensor& start, const Tensor& goal,
                                                     at::ArrayRef<double> limits, const OptTensor& v_start,
                                                     const OptTensor& v_goal) {
  const Batch b = batch_endpoints(traj, start, goal);
  const nfopp_motion_limits lim = make_limits(limits);
  need_if_given(traj, v_start, "v_start", {b.B});
  need_if_given(traj, v_goal, "v_goal", {b.B});
  const Launch on(traj);
  const auto f64 = traj.options().dtype(at::kDouble);
  Tensor profile = at::empty({b.B, b.N + 2, NFOPP_NUM_TIME_SLOTS}, f64), summary = at::empty({b.B, NFOPP_NUM_TIME_SUMMARY}, f64);
  Tensor gear = at::empty({b.B, b.N + 1}, traj.options().dtype(at::kChar));
  check_status(nfopp_path_time_profile(b.traj, b.start, b.goal, b.B, (int32_t)b.N, (int32_t)b.D, &lim, ptr<float>(v_start),
                                       ptr<float>(v_goal), profile.data_ptr<double>(), gear.data_ptr<int8_t>(),
                                       summary.data_ptr<double>(), on.stream));
  return std::make_tuple(profile, gear, summary);
}

// pose and signed speed at t0 + k * dt (nfopp_path_time_sample): (states [B, count, D+1] fp32, segment [B, count] int32).
// gear: int8 [B, N+1] or None (+1).
std::tuple<Tensor, Tensor> path_time_sample(const Tensor& traj, const Tensor& start, const Tensor& goal,
                                            at::ArrayRef<double> limits, const Tensor& profile, const OptTensor& gear, double t0,
                                            double dt, int64_t count) {
  const Batch b = batch_endpoints(traj, start, goal);
  const nfopp_motion_limits lim = make_limits(limits);
  need(traj, profile, "profile", {b.B, b.N + 2, NFOPP_NUM_TIME_SLOTS}, at::kDouble);
  need_if_given(traj, gear, "gear", {b.B, b.N + 1}, at::kChar);
  TORCH_CHECK(count >= 0 && count <= 0x7fffffffLL, "nfopp: count must lie in [0, 2^31)");
  const Launch on(traj);
  Tensor states = at::empty({b.B, count, b.D + 1}, traj.options());
  Tensor segment = at::empty({b.B, count}, traj.options().dtype(at::kInt));
  check_status(nfopp_path_time_sample(b.traj, b.start, b.goal, b.B, (int32_t)b.N, (int32_t)b.D, &lim, profile.data_ptr<double>(),
                                      ptr<int8_t>(gear), t0, dt, (int32_t)count, ptr<float>(states), ptr<int32_t>(segment), on.stream));
  return std::make_tuple(states, segment);
}

// a tracks tensor of the conflict check and the scheduler: [B, K, S] fp32 with K >= 1 instants and S >= 2 floats per row, K
// and S an int32 -> (B, K, S)
std::tuple<int64_t, int64_t, int32_t> check_tracks(const Tensor& t, const char* name) {
  check_tensor(t, name);
  TORCH_CHECK(t.dim() == 3 && t.size(1) >= 1 && t.size(2) >= 2, "nfopp: ", name, " must be [B, K, >= 2] with K >= 1");
  TORCH_CHECK(t.size(1) <= 0x7fffffffLL && t.size(2) <= 0x7fffffffLL, "nfopp: ", name,
              " must have fewer than 2^31 instants and floats per row");
  return std::make_tuple(t.size(0), t.size(1), (int32_t)t.size(2));
}
// ... of a second set, which lives beside the op's first tensor
std::tuple<int64_t, int64_t, int32_t> check_tracks_beside(const Tensor& first, const Tensor& t, const char* name) {
  const auto shape = check_tracks(t, name);
  same_device(first, t, name);
  return shape;
}

// The two sets of a conflict check, stated once for track_conflicts and box_track_conflicts: tracks_a [Ba, K, Sa] against
// tracks_b [Bb, K, Sb], or against itself when tracks_b is None (self mode: the entries take a null tracks_b for it, and
// Bb = 0 where they count B's rows).  `least_stride` is the S both sets need at least, and what stride_b reads in self mode.
struct TwoSets {
  int64_t ba = 0, bb = 0, k = 0;   // bb = ba in self mode: the width of the pair matrices
  int32_t stride_a = 0, stride_b = 0;
  bool self = true;
  const float *a = nullptr, *b = nullptr, *radius_a = nullptr, *radius_b = nullptr;   // what the entry receives
  at::TensorOptions f64;

  TwoSets(const Tensor& tracks_a, const OptTensor& tracks_b, int32_t least_stride) : f64(tracks_a.options().dtype(at::kDouble)) {
    std::tie(ba, k, stride_a) = check_tracks(tracks_a, "tracks_a");
    self = !tracks_b.has_value();
    bb = ba;
    stride_b = least_stride;
    if (!self) {
      int64_t kb;
      std::tie(bb, kb, stride_b) = check_tracks_beside(tracks_a, *tracks_b, "tracks_b");
      TORCH_CHECK(kb == k, "nfopp: tracks_b must be [Bb, K, >= ", least_stride, "] with the K of tracks_a (", k, ")");
    }
    a = ptr<float>(tracks_a);
    // own condition: null selects self mode, so a set of no obstacles still needs a non-null tracks_b pointer (it is never
    // read), and an empty set A, for which the entries do nothing, gives null on both sides
    b = (self || ba == 0) ? nullptr : (bb > 0 ? tracks_b->data_ptr<float>() : a);
  }
  // radius_a [Ba], radius_b [Bb] fp32 or None (0)
  void radii(const Tensor& tracks_a, const OptTensor& ra, const OptTensor& rb) {
    need_if_given(tracks_a, ra, "radius_a", {ba});
    if (!self) need_if_given(tracks_a, rb, "radius_b", {bb});
    radius_a = ptr<float>(ra);
    radius_b = self ? nullptr : ptr<float>(rb);   // own condition: self mode neither checks nor reads radius_b
  }
  int64_t rows_b() const { return self ? 0 : bb; }   // B's rows as the entries and summary_b count them
  Tensor summary_a(int64_t slots) const { return at::empty({ba, slots}, f64); }
  Tensor summary_b(int64_t slots) const { return at::empty({rows_b(), slots}, f64); }
  Tensor pair_matrix(bool want_pairs, const at::TensorOptions& options) const {
    return at::empty({want_pairs ? ba : 0, want_pairs ? bb : 0}, options);
  }
  // the entries write nothing for an empty set A: every obstacle is without a partner, which reads `row`
  void fill_b_of_empty_a(Tensor& summary_b, at::ArrayRef<double> row) const {
    if (ba == 0 && summary_b.numel()) summary_b.copy_(at::tensor(row, at::kDouble).expand_as(summary_b));
  }
};

// conflicts between timed tracks (nfopp_track_conflicts): tracks_a [Ba, K, Sa], tracks_b [Bb, K, Sb] or None (self mode), radii
// [Ba] / [Bb] fp32 or None (0) -> (summary [Ba, 7], summary_b [Bb, 7], pair_gap, pair_first [Ba, Bb]) float64; summary_b is
// empty in self mode, the pair matrices are empty without want_pairs.
std::tuple<Tensor, Tensor, Tensor, Tensor> track_conflicts(const Tensor& tracks_a, const OptTensor& tracks_b, double dt, double t0,
                                                           const OptTensor& radius_a, const OptTensor& radius_b, double margin,
                                                           bool want_pairs) {
  TwoSets s(tracks_a, tracks_b, 2);
  s.radii(tracks_a, radius_a, radius_b);
  const Launch on(tracks_a);
  Tensor summary = s.summary_a(NFOPP_NUM_CONFLICT_SLOTS), summary_b = s.summary_b(NFOPP_NUM_CONFLICT_SLOTS);
  Tensor pair_gap = s.pair_matrix(want_pairs, s.f64), pair_first = at::empty_like(pair_gap);
  const Workspace work(tracks_a, nfopp_track_conflicts_workspace_bytes(s.ba, s.rows_b(), (int32_t)s.k));
  check_status(nfopp_track_conflicts(s.a, s.ba, s.stride_a, s.b, s.bb, s.stride_b, (int32_t)s.k, t0, dt, s.radius_a, s.radius_b, margin,
                                     ptr<double>(summary), ptr<double>(summary_b), ptr<double>(pair_gap), ptr<double>(pair_first),
                                     work.ptr(), work.bytes, on.stream));
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  s.fill_b_of_empty_a(summary_b, {inf, -1.0, nan, inf, -1.0, 0.0, (double)NFOPP_CONFLICT_NO_PARTNER});
  return std::make_tuple(summary, summary_b, pair_gap, pair_first);
}

// the headings pass of the box check (nfopp_track_headings): tracks [B, K, S >= 3] -> [B, K, 2] float64 (cos theta, sin theta)
Tensor track_headings(const Tensor& tracks) {
  const auto [b, k, stride] = check_tracks(tracks, "tracks");
  TORCH_CHECK(stride >= 3, "nfopp: tracks must be [B, K, >= 3] (x, y, theta)");
  const Launch on(tracks);
  Tensor out = at::empty({b, k, 2}, tracks.options().dtype(at::kDouble));
  check_status(nfopp_track_headings(ptr<float>(tracks), b, stride, (int32_t)k, ptr<double>(out), on.stream));
  return out;
}

// conflicts between timed tracks of oriented boxes (nfopp_track_headings, then nfopp_box_track_conflicts): tracks [B, K, S >= 3],
// box [B, 4] fp32, radius [B] fp32 or None (0) -> (summary [Ba, 7], summary_b [Bb, 7] float64, pair_status [Ba, Bb] int32,
// pair_first, pair_undecided [Ba, Bb] float64); summary_b is empty in self mode, the pair matrices without want_pairs.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> box_track_conflicts(const Tensor& tracks_a, const OptTensor& tracks_b, double dt,
                                                                       double t0, const Tensor& box_a, const OptTensor& box_b,
                                                                       const OptTensor& radius_a, const OptTensor& radius_b,
                                                                       double margin, int64_t refine, bool want_pairs) {
  TwoSets s(tracks_a, tracks_b, 3);
  if (!s.self) {
    TORCH_CHECK(box_b.has_value(), "nfopp: tracks_b needs box_b");
    need(tracks_a, *box_b, "box_b", {s.bb, 4});
  }
  TORCH_CHECK(s.stride_a >= 3 && s.stride_b >= 3, "nfopp: box tracks must be [B, K, >= 3] (x, y, theta)");
  TORCH_CHECK(refine >= 0 && refine <= NFOPP_BOX_CONFLICT_MAX_REFINE, "nfopp: refine must be 0 .. ", NFOPP_BOX_CONFLICT_MAX_REFINE);
  need(tracks_a, box_a, "box_a", {s.ba, 4});
  s.radii(tracks_a, radius_a, radius_b);
  const Launch on(tracks_a);
  Tensor heading_a = track_headings(tracks_a);
  Tensor heading_b = s.self ? at::empty({0, s.k, 2}, s.f64) : track_headings(*tracks_b);
  Tensor summary = s.summary_a(NFOPP_NUM_BOX_CONFLICT_SLOTS), summary_b = s.summary_b(NFOPP_NUM_BOX_CONFLICT_SLOTS);
  Tensor pair_status = s.pair_matrix(want_pairs, tracks_a.options().dtype(at::kInt));
  Tensor pair_first = s.pair_matrix(want_pairs, s.f64), pair_undecided = at::empty_like(pair_first);
  const Workspace work(tracks_a, nfopp_box_track_conflicts_workspace_bytes(s.ba, s.rows_b(), (int32_t)s.k));
  const float* box_b_ptr = s.self ? nullptr : ptr<float>(box_b);   // own condition: self mode neither checks nor reads box_b
  check_status(nfopp_box_track_conflicts(s.a, ptr<double>(heading_a), s.ba, s.stride_a, s.b, ptr<double>(heading_b), s.bb, s.stride_b,
                                         (int32_t)s.k, t0, dt, ptr<float>(box_a), box_b_ptr, s.radius_a, s.radius_b, margin,
                                         (int32_t)refine, ptr<double>(summary), ptr<double>(summary_b), ptr<int32_t>(pair_status),
                                         ptr<double>(pair_first), ptr<double>(pair_undecided), work.ptr(), work.bytes, on.stream));
  const double inf = std::numeric_limits<double>::infinity();
  s.fill_b_of_empty_a(summary_b, {inf, -1.0, 0.0, inf, -1.0, 0.0, (double)NFOPP_CONFLICT_NO_PARTNER});
  return std::make_tuple(summary, summary_b, pair_status, pair_first, pair_undecided);
}

// the shift masks of a fleet (nfopp_fleet_shift_masks): tracks [B, K, S], radius [B] fp32 or None (0), obstacles
// [M, K + max_delay, So] or None with obstacle_radius [M] or None -> (pair [B, B, 2], base [B]) int64 holding the uint64 words,
// bad [B] int32
std::tuple<Tensor, Tensor, Tensor> fleet_shift_masks(const Tensor& tracks, int64_t max_delay, const OptTensor& radius, double margin,
                                                     const OptTensor& obstacles, const OptTensor& obstacle_radius) {
  const auto [b, k, stride] = check_tracks(tracks, "tracks");
  TORCH_CHECK(max_delay >= 0 && max_delay <= NFOPP_SCHEDULE_MAX_DELAY, "nfopp: max_delay must be in 0 .. ", NFOPP_SCHEDULE_MAX_DELAY);
  need_if_given(tracks, radius, "radius", {b});
  int64_t m = 0;
  int32_t obstacle_stride = 2;
  if (obstacles.has_value()) {
    int64_t ko;
    std::tie(m, ko, obstacle_stride) = check_tracks_beside(tracks, *obstacles, "obstacles");
    TORCH_CHECK(ko == k + max_delay, "nfopp: obstacles must be [M, K + max_delay, >= 2] = [M, ", k + max_delay, ", >= 2]");
    need_if_given(tracks, obstacle_radius, "obstacle_radius", {m});
  }
  const Launch on(tracks);
  const auto i64 = tracks.options().dtype(at::kLong);
  Tensor pair = at::empty({b, b, 2}, i64), base = at::empty({b}, i64), bad = at::empty({b}, tracks.options().dtype(at::kInt));
  const Workspace work(tracks, nfopp_fleet_shift_masks_workspace_bytes(b, m));
  // own condition: without obstacles, obstacle_radius is neither checked nor read
  const float* obstacle_radius_ptr = obstacles.has_value() ? ptr<float>(obstacle_radius) : nullptr;
  check_status(nfopp_fleet_shift_masks(ptr<float>(tracks), b, stride, (int32_t)k, ptr<float>(radius), margin, (int32_t)max_delay,
                                       ptr<float>(obstacles), m, obstacle_stride, obstacle_radius_ptr, words_ptr(pair), words_ptr(base),
                                       ptr<int32_t>(bad), work.ptr(), work.bytes, on.stream));
  return std::make_tuple(pair, base, bad);
}

// the assignment pass (nfopp_fleet_assign_delays) on masks as written above; order [B] int32 or None (0 .. B - 1)
// -> (delay [B] int32, status [B] int32, forbidden [B] int64 holding the uint64 word)
std::tuple<Tensor, Tensor, Tensor> fleet_assign_delays(const Tensor& pair, const Tensor& base, const Tensor& bad, const OptTensor& order,
                                                       int64_t max_delay) {
  check_tensor(pair, "pair", at::kLong);
  TORCH_CHECK(pair.dim() == 3 && pair.size(0) == pair.size(1) && pair.size(2) == 2, "nfopp: pair must be [B, B, 2]");
  TORCH_CHECK(max_delay >= 0 && max_delay <= NFOPP_SCHEDULE_MAX_DELAY, "nfopp: max_delay must be in 0 .. ", NFOPP_SCHEDULE_MAX_DELAY);
  const int64_t b = pair.size(0);
  need(pair, base, "base", {b}, at::kLong);
  need(pair, bad, "bad", {b}, at::kInt);
  need_if_given(pair, order, "order", {b}, at::kInt);
  const Launch on(pair);
  const auto i32 = pair.options().dtype(at::kInt);
  Tensor delay = at::empty({b}, i32), status = at::empty({b}, i32), forbidden = at::empty({b}, pair.options());
  if (b > 0)
    check_status(nfopp_fleet_assign_delays(words_ptr(pair), words_ptr(base), bad.data_ptr<int32_t>(), ptr<int32_t>(order), b,
                                           (int32_t)max_delay, delay.data_ptr<int32_t>(), status.data_ptr<int32_t>(),
                                           words_ptr(forbidden), on.stream));
  return std::make_tuple(delay, status, forbidden);
}

// What the two space-time ops share: an occupancy image [rows, cols] uint8 and the instants of a reservation on it -> the
// frame, and the reservation's size in int64 words
struct ImageFrame {
  int32_t rows, cols, count;
  int64_t words;
  size_t bytes() const { return (size_t)words * 8; }
};
ImageFrame image_frame(const Tensor& occupancy, int64_t count) {
  check_tensor(occupancy, "occupancy", at::kByte);
  TORCH_CHECK(occupancy.dim() == 2 && occupancy.numel() > 0, "nfopp: occupancy must be a non-empty [rows, cols] image");
  TORCH_CHECK(count >= 1 && count <= 0x7fffffffLL, "nfopp: count must be >= 1");
  TORCH_CHECK(occupancy.size(0) <= 0x7fffffffLL && occupancy.size(1) <= 0x7fffffffLL, "nfopp: image too large for an index");
  ImageFrame f = {(int32_t)occupancy.size(0), (int32_t)occupancy.size(1), (int32_t)count, 0};
  const size_t bytes = nfopp_spacetime_reservation_bytes(f.rows, f.cols, f.count);
  TORCH_CHECK(bytes > 0, "nfopp: image and count too large for an index");
  f.words = (int64_t)(bytes / 8);
  return f;
}

// a space-time reservation with tracks ORed in (nfopp_spacetime_reservation_init / nfopp_spacetime_reserve): reservation None
// = a fresh one from the occupancy image, else a copy of the given one; tracks [M, count, S] or None with radius [M] fp32 or
// None (0) and visible [M] uint8 or None (all) -> the reservation's words [n] int64 (layout: include/nfopp_hip.h)
Tensor spacetime_reserve(const Tensor& occupancy, int64_t count, double b0, double b2, double resolution, double robot_radius, double margin,
                         const OptTensor& reservation, const OptTensor& tracks, const OptTensor& radius, const OptTensor& visible) {
  const ImageFrame f = image_frame(occupancy, count);
  const Launch on(occupancy);
  Tensor words;
  if (reservation.has_value()) {
    need(occupancy, *reservation, "reservation", {f.words}, at::kLong);
    words = reservation->clone();
  } else {
    words = at::empty({f.words}, occupancy.options().dtype(at::kLong));
    check_status(nfopp_spacetime_reservation_init(occupancy.data_ptr<uint8_t>(), f.rows, f.cols, f.count, words_ptr(words), f.bytes(),
                                                  on.stream));
  }
  if (!tracks.has_value()) {
    TORCH_CHECK(!radius.has_value() && !visible.has_value(), "nfopp: radius and visible belong to tracks");
    return words;
  }
  const auto [m, k, stride] = check_tracks_beside(occupancy, *tracks, "tracks");
  TORCH_CHECK(k == count, "nfopp: tracks must be [M, count, >= 2] = [M, ", count, ", >= 2]");
  need_if_given(occupancy, radius, "radius", {m});
  need_if_given(occupancy, visible, "visible", {m}, at::kByte);
  const Workspace work(occupancy, nfopp_spacetime_reserve_workspace_bytes(m));
  check_status(nfopp_spacetime_reserve(f.rows, f.cols, f.count, b0, b2, resolution, (float)robot_radius, margin, ptr<float>(tracks), m,
                                       stride, ptr<float>(radius), ptr<uint8_t>(visible), words_ptr(words), f.bytes(), work.ptr(),
                                       work.bytes, on.stream));
  return words;
}

// the fleet pass (nfopp_spacetime_plan_fleet): start_cells / goal_cells [R, 2] int32 (row, col), order [R] int32 or None; the
// reservation is read and WRITTEN (every planned robot is reserved) -> (cells [R, count] int32, arrival [R] int32, status [R]
// int32, tracks [R, count, 2] fp32)
std::tuple<Tensor, Tensor, Tensor, Tensor> spacetime_plan_fleet(const Tensor& occupancy, int64_t count, double b0, double b2, double resolution,
                                                                double robot_radius, double margin, const Tensor& start_cells,
                                                                const Tensor& goal_cells, const OptTensor& order, Tensor reservation) {
  const ImageFrame f = image_frame(occupancy, count);
  need(occupancy, reservation, "reservation", {f.words}, at::kLong);
  check_tensor(start_cells, "start_cells", at::kInt);
  TORCH_CHECK(start_cells.dim() == 2 && start_cells.size(1) == 2, "nfopp: start_cells must be [R, 2] (row, col)");
  const int64_t r = start_cells.size(0);
  same_device(occupancy, start_cells, "start_cells");
  need(occupancy, goal_cells, "goal_cells", {r, 2}, at::kInt);
  need_if_given(occupancy, order, "order", {r}, at::kInt);
  const Launch on(occupancy);
  const auto i32 = occupancy.options().dtype(at::kInt);
  Tensor cells = at::empty({r, count}, i32), arrival = at::empty({r}, i32), status = at::empty({r}, i32);
  Tensor tracks = at::empty({r, count, 2}, occupancy.options().dtype(at::kFloat));
  const Workspace work(occupancy, nfopp_spacetime_plan_workspace_bytes(f.rows, f.cols, f.count, r));
  check_status(nfopp_spacetime_plan_fleet(occupancy.data_ptr<uint8_t>(), f.rows, f.cols, f.count, b0, b2, resolution, (float)robot_radius,
                                          margin, ptr<int32_t>(start_cells), ptr<int32_t>(goal_cells), ptr<int32_t>(order), r,
                                          words_ptr(reservation), f.bytes(), ptr<int32_t>(cells), ptr<int32_t>(arrival),
                                          ptr<int32_t>(status), ptr<float>(tracks), work.ptr(), work.bytes, on.stream));
  return std::make_tuple(cells, arrival, status, tracks);
}

static void check_lattice_costs(int64_t turn_cost, int64_t reverse_cost, int64_t cusp_cost) {
  TORCH_CHECK(turn_cost >= 0 && turn_cost <= 255, "nfopp: turn_cost must be 0..255");
  TORCH_CHECK(reverse_cost >= 0 && reverse_cost <= 255, "nfopp: reverse_cost must be 0..255");
  TORCH_CHECK(cusp_cost >= 0 && cusp_cost <= 255, "nfopp: cusp_cost must be 0..255");
}

// What the two lattice field ops share: layers uint8 [L, rows, cols], goal_states int32 [G, 3] (row, col, heading or -1) ->
// fields int32 [G, 8, rows, cols, 2] from nfopp_lattice_distance_fields, with `gears` [G, 2, 8, rows, cols, 2] from
// nfopp_lattice_gear_distance_fields; the forward-only search has reverse_cost = cusp_cost = 0.
static Tensor lattice_fields_impl(const Tensor& layers, const Tensor& goal_states, int64_t turn_cost, int64_t reverse_cost,
                                  int64_t cusp_cost, bool gears) {
  check_tensor(layers, "layers", at::kByte);
  beside(layers, goal_states, "goal_states", at::kInt);
  TORCH_CHECK(layers.dim() == 3, "nfopp: layers must be [L, rows, cols] uint8");
  TORCH_CHECK(goal_states.dim() == 2 && goal_states.size(1) == 3, "nfopp: goal_states must be [G, 3] (row, col, heading)");
  check_lattice_costs(turn_cost, reverse_cost, cusp_cost);
  const int64_t G = goal_states.size(0);
  const int32_t L = (int32_t)layers.size(0), tc = (int32_t)turn_cost, rc = (int32_t)reverse_cost, cc = (int32_t)cusp_cost;
  TORCH_CHECK(layers.size(1) >= 1 && layers.size(2) >= 1 && layers.size(1) <= 32768 && layers.size(2) <= 32768,
              "nfopp: grid must be 1..32768 cells a side");
  const int32_t rows = (int32_t)layers.size(1), cols = (int32_t)layers.size(2);
  const Launch on(layers);
  const auto i32 = layers.options().dtype(at::kInt);
  Tensor fields = gears ? at::empty({G, 2, 8, rows, cols, 2}, i32) : at::empty({G, 8, rows, cols, 2}, i32);
  const Workspace work(layers, gears ? nfopp_lattice_gear_fields_workspace_bytes(rows, cols, tc, rc, cc, G)
                                     : nfopp_lattice_fields_workspace_bytes(rows, cols, tc, G));
  const uint8_t* occ = layers.data_ptr<uint8_t>();
  const int32_t* goals = ptr<int32_t>(goal_states);
  int32_t* out = ptr<int32_t>(fields);
  check_status(gears ? nfopp_lattice_gear_distance_fields(occ, L, rows, cols, goals, G, tc, rc, cc, out, work.ptr(), work.bytes, on.stream)
                     : nfopp_lattice_distance_fields(occ, L, rows, cols, goals, G, tc, out, work.ptr(), work.bytes, on.stream));
  return fields;
}

// What the two lattice trace ops share: the descent through fields [n_fields, 8, rows, cols, 2] (nfopp_lattice_trace_paths), with
// `gears` [n_fields, 2, 8, rows, cols, 2] (nfopp_lattice_gear_trace_paths), = the fields field_first .. of n_total; start_states /
// goal_states int32 [B, 3], field_index int32 [B] -> {cells [B, max_len, 2], headings [B, max_len], gears [B, max_len] (with
// `gears` only), count [B], status [B], cost [B, 2]} int32.  Outputs start as zeros, so a problem of another chunk reads count
// 0, status 0.
static std::vector<Tensor> lattice_trace_impl(const Tensor& fields, int64_t field_first, int64_t n_total, const Tensor& start_states,
                                              const Tensor& goal_states, const Tensor& field_index, int64_t turn_cost,
                                              int64_t reverse_cost, int64_t cusp_cost, int64_t max_len, bool gears) {
  check_tensor(fields, "fields", at::kInt);
  if (gears) {
    TORCH_CHECK(fields.dim() == 6 && fields.size(1) == 2 && fields.size(2) == 8 && fields.size(5) == 2,
                "nfopp: fields must be [G, 2, 8, rows, cols, 2]");
  } else {
    TORCH_CHECK(fields.dim() == 5 && fields.size(1) == 8 && fields.size(4) == 2, "nfopp: fields must be [G, 8, rows, cols, 2]");
  }
  check_tensor(start_states, "start_states", at::kInt);
  TORCH_CHECK(start_states.dim() == 2 && start_states.size(1) == 3, "nfopp: start_states must be [B, 3] (row, col, heading)");
  same_device(fields, start_states, "start_states");
  const int64_t B = start_states.size(0), G = fields.size(0), rows = fields.size(gears ? 3 : 2), cols = fields.size(gears ? 4 : 3);
  need(fields, goal_states, "goal_states", {B, 3}, at::kInt);
  need(fields, field_index, "field_index", {B}, at::kInt);
  TORCH_CHECK(max_len >= 0 && max_len <= std::numeric_limits<int32_t>::max(), "nfopp: bad max_len");
  check_lattice_costs(turn_cost, reverse_cost, cusp_cost);
  TORCH_CHECK(rows >= 1 && cols >= 1, "nfopp: fields of an empty grid");
  const Launch on(fields);
  const auto i32 = fields.options().dtype(at::kInt);
  Tensor cells = at::zeros({B, max_len, 2}, i32), headings = at::zeros({B, max_len}, i32), gear = at::zeros({gears ? B : 0, max_len}, i32);
  Tensor count = at::zeros({B}, i32), status = at::zeros({B}, i32), cost = at::zeros({B, 2}, i32);
  const int32_t r = (int32_t)rows, c = (int32_t)cols, tc = (int32_t)turn_cost, ml = (int32_t)max_len;
  const auto p = [](const Tensor& t) { return ptr<int32_t>(t); };
  check_status(gears ? nfopp_lattice_gear_trace_paths(p(fields), field_first, G, n_total, r, c, tc, (int32_t)reverse_cost,
                                                      (int32_t)cusp_cost, p(start_states), p(goal_states), p(field_index), B, ml,
                                                      p(cells), p(headings), p(gear), p(count), p(status), p(cost), on.stream)
                     : nfopp_lattice_trace_paths(p(fields), field_first, G, n_total, r, c, tc, p(start_states), p(goal_states),
                                                 p(field_index), B, ml, p(cells), p(headings), p(count), p(status), p(cost),
                                                 on.stream));
  return {cells, headings, gear, count, status, cost};
}

Tensor lattice_fields(const Tensor& layers, const Tensor& goal_states, int64_t turn_cost) {
  return lattice_fields_impl(layers, goal_states, turn_cost, 0, 0, false);
}

Tensor lattice_gear_fields(const Tensor& layers, const Tensor& goal_states, int64_t turn_cost, int64_t reverse_cost, int64_t cusp_cost) {
  return lattice_fields_impl(layers, goal_states, turn_cost, reverse_cost, cusp_cost, true);
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> lattice_trace_paths(const Tensor& fields, int64_t field_first, int64_t n_total,
                                                                       const Tensor& start_states, const Tensor& goal_states,
                                                                       const Tensor& field_index, int64_t turn_cost, int64_t max_len) {
  const auto t = lattice_trace_impl(fields, field_first, n_total, start_states, goal_states, field_index, turn_cost, 0, 0, max_len, false);
  return std::make_tuple(t[0], t[1], t[3], t[4], t[5]);
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> lattice_gear_trace_paths(
    const Tensor& fields, int64_t field_first, int64_t n_total, const Tensor& start_states, const Tensor& goal_states,
    const Tensor& field_index, int64_t turn_cost, int64_t reverse_cost, int64_t cusp_cost, int64_t max_len) {
  const auto t = lattice_trace_impl(fields, field_first, n_total, start_states, goal_states, field_index, turn_cost, reverse_cost,
                                    cusp_cost, max_len, true);
  return std::make_tuple(t[0], t[1], t[2], t[3], t[4], t[5]);
}

// nfopp_lattice_seed_trajectories: cells int32 [B, max_len, 2], headings int32 [B, max_len], count / status int32 [B], start /
// goal fp32 [B, 3] -> traj fp32 [B, n_waypoints, 3]
Tensor lattice_seed_trajectories(const Tensor& cells, const Tensor& headings, const Tensor& count, const Tensor& status,
                                 const Tensor& start, const Tensor& goal, int64_t n_waypoints, double origin_x, double origin_y,
                                 double resolution) {
  check_tensor(cells, "cells", at::kInt);
  TORCH_CHECK(cells.dim() == 3 && cells.size(2) == 2, "nfopp: cells must be [B, max_len, 2] (row, col)");
  const int64_t B = cells.size(0), max_len = cells.size(1);
  need(cells, headings, "headings", {B, max_len}, at::kInt);
  need(cells, count, "count", {B}, at::kInt);
  need(cells, status, "status", {B}, at::kInt);
  need(cells, start, "start", {B, 3}, at::kFloat);
  need(cells, goal, "goal", {B, 3}, at::kFloat);
  TORCH_CHECK(n_waypoints >= 1 && n_waypoints <= std::numeric_limits<int32_t>::max(), "nfopp: bad n_waypoints");
  TORCH_CHECK(resolution > 0.0, "nfopp: bad resolution");
  const Launch on(cells);
  Tensor traj = at::empty({B, n_waypoints, 3}, cells.options().dtype(at::kFloat));
  const Workspace work(cells, nfopp_lattice_seed_workspace_bytes(B, (int32_t)max_len));
  check_status(nfopp_lattice_seed_trajectories(ptr<int32_t>(cells), ptr<int32_t>(headings), ptr<int32_t>(count), ptr<int32_t>(status), B,
                                               (int32_t)max_len, ptr<float>(start), ptr<float>(goal), (int32_t)n_waypoints, origin_x,
                                               origin_y, resolution, ptr<float>(traj), work.ptr(), work.bytes, on.stream));
  return traj;
}

}  // namespace

// One list: the schema of every op and its function.  The ops validate their arguments themselves (device included: a CPU tensor
// gets the "no CPU path" message instead of a dispatcher "no kernel" error), so each is registered for every dispatch key.
TORCH_LIBRARY(nfopp, lib) {
  const auto op = [&lib](const char* schema, auto* fn) {
    lib.def(schema, torch::dispatch(c10::DispatchKey::CompositeExplicitAutograd, fn));
  };
  op("onf_fwd_bwd_input(Tensor params, Tensor points, float mean, float sigma, bool use_cos, bool has_bias, int angle_dim) -> Tensor", &onf_fwd_bwd_input);
  op("onf_logits(Tensor params, Tensor points, float mean, float sigma, bool use_cos, bool has_bias, int angle_dim) -> Tensor", &onf_logits);
  op("traj_step(Tensor params, float mean, float sigma, bool use_cos, bool has_bias, int angle_dim, Tensor(a!) traj, Tensor start, "
     "Tensor goal, Tensor(b!)? lam, Tensor(c!)? cm, Tensor(d!) adam_m, Tensor(e!) adam_v, Tensor(f!) t, int t_mode, int seed, "
     "int rng_offset, int traj_index_offset, Tensor(g!) onf_out, Tensor hinv_band, int half_width, int interior_lo, int interior_hi, "
     "float[] hyper, Tensor(h!)? terms, Tensor? active, Tensor(i!)? live_ws) -> ()", &traj_step);
  op("traj_steps(Tensor params, float mean, float sigma, bool use_cos, bool has_bias, int angle_dim, Tensor(a!) traj, Tensor start, "
     "Tensor goal, Tensor(b!)? lam, Tensor(c!)? cm, Tensor(d!) adam_m, Tensor(e!) adam_v, Tensor(f!) t, Tensor? t_steps, int seed, "
     "int rng_offset, int traj_index_offset, Tensor(g!) onf_out, Tensor hinv_band, int half_width, int interior_lo, int interior_hi, "
     "Tensor u, float[] hyper, float adam_lr, float adam_beta1, float adam_beta2, int adam_steps_done, int step_count, "
     "int reparam_freq, int n_steps, Tensor(h!)? terms, Tensor? active, Tensor(i!)? live_ws) -> ()", &traj_steps);
  op("reparametrize(Tensor(a!) traj, Tensor start, Tensor goal, Tensor(b!)? lam, Tensor(c!)? cm, Tensor u, Tensor? active) -> ()", &reparametrize);
  op("update_endpoints(Tensor(a!) traj, Tensor(b!) start, Tensor(c!) goal, Tensor(d!)? lam, Tensor(e!)? cm, Tensor u, "
     "Tensor points, int which, Tensor? moved, Tensor(f!)? min_index) -> ()", &update_endpoints);
  op("onf_train_grad(Tensor params, Tensor samples, Tensor labels, float inv_count, float mean, float sigma, bool use_cos, "
     "bool has_bias, int angle_dim) -> Tensor", &onf_train_grad);
  op("adam_step(Tensor(a!) param, Tensor grad, Tensor(b!) m, Tensor(c!) v, float beta2, float omb1, float omb2, float eps, "
     "float step_size, float bc2_sqrt) -> ()", &adam_step);
  op("onf_train_step(Tensor(a!) params, Tensor(b!) m, Tensor(c!) v, Tensor samples, Tensor labels, float mean, float sigma, "
     "bool use_cos, bool has_bias, int angle_dim, float beta2, float omb1, float omb2, float eps, float step_size, "
     "float bc2_sqrt) -> Tensor", &onf_train_step);
  op("grid_search_init(Tensor(a!) traj, Tensor start, Tensor goal, Tensor occupancy, Tensor start_cells, Tensor goal_cells, "
     "Tensor unique_goal_cells, Tensor field_index, float origin_x, float origin_y, float resolution, "
     "bool angles_with_direction) -> Tensor", &grid_search_init);
  op("path_time_profile(Tensor traj, Tensor start, Tensor goal, float[] limits, Tensor? v_start, Tensor? v_goal) -> "
     "(Tensor, Tensor, Tensor)", &path_time_profile);
  op("path_time_sample(Tensor traj, Tensor start, Tensor goal, float[] limits, Tensor profile, Tensor? gear, float t0, "
     "float dt, int count) -> (Tensor, Tensor)", &path_time_sample);
  op("track_conflicts(Tensor tracks_a, Tensor? tracks_b, float dt, float t0, Tensor? radius_a, Tensor? radius_b, float margin, "
     "bool want_pairs) -> (Tensor, Tensor, Tensor, Tensor)", &track_conflicts);
  op("track_headings(Tensor tracks) -> Tensor", &track_headings);
  op("box_track_conflicts(Tensor tracks_a, Tensor? tracks_b, float dt, float t0, Tensor box_a, Tensor? box_b, Tensor? radius_a, "
     "Tensor? radius_b, float margin, int refine, bool want_pairs) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", &box_track_conflicts);
  op("fleet_shift_masks(Tensor tracks, int max_delay, Tensor? radius, float margin, Tensor? obstacles, Tensor? obstacle_radius) -> "
     "(Tensor, Tensor, Tensor)", &fleet_shift_masks);
  op("fleet_assign_delays(Tensor pair, Tensor base, Tensor bad, Tensor? order, int max_delay) -> (Tensor, Tensor, Tensor)", &fleet_assign_delays);
  op("spacetime_reserve(Tensor occupancy, int count, float b0, float b2, float resolution, float robot_radius, float margin, "
     "Tensor? reservation, Tensor? tracks, Tensor? radius, Tensor? visible) -> Tensor", &spacetime_reserve);
  op("spacetime_plan_fleet(Tensor occupancy, int count, float b0, float b2, float resolution, float robot_radius, float margin, "
     "Tensor start_cells, Tensor goal_cells, Tensor? order, Tensor(a!) reservation) -> (Tensor, Tensor, Tensor, Tensor)", &spacetime_plan_fleet);
  op("lattice_fields(Tensor layers, Tensor goal_states, int turn_cost) -> Tensor", &lattice_fields);
  op("lattice_trace_paths(Tensor fields, int field_first, int n_total, Tensor start_states, Tensor goal_states, "
     "Tensor field_index, int turn_cost, int max_len) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", &lattice_trace_paths);
  op("lattice_gear_fields(Tensor layers, Tensor goal_states, int turn_cost, int reverse_cost, int cusp_cost) -> Tensor", &lattice_gear_fields);
  op("lattice_gear_trace_paths(Tensor fields, int field_first, int n_total, Tensor start_states, Tensor goal_states, "
     "Tensor field_index, int turn_cost, int reverse_cost, int cusp_cost, int max_len) -> "
     "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", &lattice_gear_trace_paths);
  op("lattice_seed_trajectories(Tensor cells, Tensor headings, Tensor count, Tensor status, Tensor start, Tensor goal, "
     "int n_waypoints, float origin_x, float origin_y, float resolution) -> Tensor", &lattice_seed_trajectories);
}
