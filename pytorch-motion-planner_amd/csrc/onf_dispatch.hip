// The matrix-path switch and the ONF entry points: which kernel family and tile count every ONF launch runs on.
//
// Matrix path 0: fp32 MFMA (csrc/onf_fused.hip).  1 (default): bf16x3 split on 32x32x16 tiles (csrc/onf_x32.hip) at EVERY
// launch size -- results must not depend on how a batch is sharded -- and on 16x16x32 tiles (csrc/onf_split.hip) for the
// feature dimensions the 32x32 kernel does not cover.  2: bf16x3 split on 16x16x32 tiles everywhere.  The switch is read
// once per C-ABI call: the route it gives serves every launch of that call (the ONF fit's weight-gradient pass reads the
// factor order the training pass wrote).
#include <stdlib.h>

#include <atomic>

#include "block_collectives.h"
#include "onf_kernel.h"

namespace nfopp {

static std::atomic<int> g_matrix_path{-1};   // -1: NFOPP_MATRIX_PATH not read yet

static int matrix_path() {
  int path = g_matrix_path.load(std::memory_order_relaxed);
  if (path >= 0) return path;
  const char* e = getenv("NFOPP_MATRIX_PATH");
  path = !e ? 1 : (e[0] == 'f' || e[0] == '0') ? 0 : e[0] == '2' ? 2 : 1;
  int unset = -1;   // an nfopp_set_matrix_path that came first wins
  return g_matrix_path.compare_exchange_strong(unset, path) ? path : unset;
}

int onf_unsupported(const OnfGeom& g) {
  set_error("unsupported ONF feature dimension %d", g.fin);
  return NFOPP_ERR_ARG;
}

int onf_route(const OnfGeom& g, OnfRoute* r) {
  const int path = matrix_path();
  // the 32x32 kernel needs one free pad position for its ones feature
  const int nkb = (g.fin + 16) >> 4;
  if (path == 1 && ((g.n_enc == 200 && (nkb == 14 || nkb == 13)) || (g.n_enc == 100 && (nkb == 8 || nkb == 7)))) {
    *r = {ONF_X32, nkb};
    return NFOPP_OK;
  }
  const int nkt = layout_p_tiles(g.fin);
  if (nkt != 14 && nkt != 13 && nkt != 8 && nkt != 7) return onf_unsupported(g);
  *r = {path == 0 ? ONF_FP32 : ONF_SPLIT16, nkt};
  return NFOPP_OK;
}

// ---- early stop: stable compaction of the live trajectory indices (one workgroup; B is a few thousand per GPU) ------
// live[0] = count, live[1 + k] = index of the k-th trajectory with active[b] != 0, ascending.
constexpr int CP_THREADS = 1024;
__global__ __launch_bounds__(CP_THREADS) void compact_live_kernel(const unsigned char* active, long long batch, int* live) {
  __shared__ int wave_sum[CP_THREADS / 64];
  const int tid = threadIdx.x;
  const long long per = (batch + CP_THREADS - 1) / CP_THREADS;
  const long long lo = tid * per, hi = lo + per < batch ? lo + per : batch;
  int mine = 0;
  for (long long b = lo; b < hi; ++b) mine += active[b] != 0;
  int count;
  int pos = block_exclusive_scan<CP_THREADS / 64>(mine, 0, Plus(), wave_sum, &count);
  if (tid == 0) live[0] = count;
  for (long long b = lo; b < hi; ++b)
    if (active[b] != 0) live[1 + pos++] = (int)b;
}

// nfopp_onf_eval_points (mode ONF_EVAL) / nfopp_onf_eval_logits (ONF_LOGITS)
static int eval_points(int mode, const nfopp_onf_config* cfg, const float* params_dev, const float* points_dev,
                       int64_t n_points, float* out4_dev, hipStream_t stream) {
  OnfKernelArgs a = {};
  NFOPP_REQUIRE(make_geom(cfg, &a.geom), "bad ONF configuration");
  NFOPP_REQUIRE(n_points >= 0, "negative point count");
  NFOPP_REQUIRE(n_points == 0 || (params_dev && points_dev && out4_dev), "null device pointer");
  if (n_points == 0) return NFOPP_OK;
  OnfRoute r;
  const int rc = onf_route(a.geom, &r);
  if (rc != NFOPP_OK) return rc;
  a.params = params_dev;
  a.points = points_dev;
  a.n_points = n_points;
  a.out4 = out4_dev;
  return launch_onf(r, mode, a, stream);
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_set_matrix_path(int32_t path) {
  NFOPP_REQUIRE(path >= 0 && path <= 2,
                "matrix path must be 0 (fp32 MFMA), 1 (bf16x3 split MFMA) or 2 (bf16x3 split MFMA, 16x16x32 kernels only)");
  g_matrix_path.store(path, std::memory_order_relaxed);
  return NFOPP_OK;
}

extern "C" int nfopp_get_matrix_path(void) { return matrix_path(); }

extern "C" int nfopp_onf_eval_points(const nfopp_onf_config* cfg, const float* params_dev, const float* points_dev,
                                     int64_t n_points, float* out4_dev, void* stream) {
  return eval_points(ONF_EVAL, cfg, params_dev, points_dev, n_points, out4_dev, (hipStream_t)stream);
}

extern "C" int nfopp_onf_eval_logits(const nfopp_onf_config* cfg, const float* params_dev, const float* points_dev,
                                     int64_t n_points, float* out4_dev, void* stream) {
  return eval_points(ONF_LOGITS, cfg, params_dev, points_dev, n_points, out4_dev, (hipStream_t)stream);
}

extern "C" int nfopp_traj_collision_eval(const nfopp_onf_config* cfg, const float* params_dev, const float* traj_dev,
                                         int64_t batch, int32_t n_waypoints, int32_t dim, float* t_dev,
                                         int32_t t_mode, uint64_t seed, uint64_t rng_offset,
                                         int64_t traj_index_offset, float* out4_dev, const uint8_t* active_dev,
                                         int32_t* live_ws_dev, void* stream) {
  OnfKernelArgs a = {};
  NFOPP_REQUIRE(make_geom(cfg, &a.geom), "bad ONF configuration");
  NFOPP_REQUIRE(batch >= 0 && n_waypoints >= 2, "need batch >= 0 and at least 2 waypoints");
  NFOPP_REQUIRE(batch == 0 || (params_dev && traj_dev && t_dev && out4_dev), "null device pointer");
  NFOPP_REQUIRE(dim == a.geom.point_dim, "trajectory dim %d does not match the ONF point dim %d", dim,
                a.geom.point_dim);
  NFOPP_REQUIRE(t_mode == 0 || t_mode == 1, "t_mode must be 0 (read) or 1 (Philox)");
  NFOPP_REQUIRE(batch <= 0x7fffffffLL, "batch too large for one launch");
  NFOPP_REQUIRE(!active_dev || live_ws_dev, "an active mask needs the live-list workspace (batch + 1 int32)");
  if (batch == 0) return NFOPP_OK;
  OnfRoute r;
  const int rc = onf_route(a.geom, &r);
  if (rc != NFOPP_OK) return rc;
  if (active_dev) {
    hipLaunchKernelGGL(compact_live_kernel, dim3(1), dim3(CP_THREADS), 0, (hipStream_t)stream, active_dev,
                       (long long)batch, live_ws_dev);
    NFOPP_HIP(hipGetLastError());
    a.live = live_ws_dev;
  }
  a.params = params_dev;
  a.traj = traj_dev;
  a.n_way = n_waypoints;
  a.dim = dim;
  a.t = t_dev;
  a.t_mode = t_mode;
  a.seed = seed;
  a.rng_offset = rng_offset;
  a.traj_index_offset = traj_index_offset;
  a.n_points = batch * (int64_t)(n_waypoints - 1);
  a.out4 = out4_dev;
  return launch_onf(r, ONF_EVAL, a, (hipStream_t)stream);
}
