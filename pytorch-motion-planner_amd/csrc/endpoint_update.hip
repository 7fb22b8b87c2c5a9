// Start / goal update of a batch (HBM-bound; one workgroup per trajectory): the receding-horizon re-rooting of
// nfop/constrained_nerf_opt_planner.py:178-194 (SE(2)) and nfop/nerf_opt_planner.py:202-218 (2-D) in ONE launch --
//   delta = sum((traj[:, :2] - point[:, :2]) ** 2, dim=1);  min_index = argmin(delta) [+ 1, capped at N, for SE(2)]
//   traj[min_index:] = goal   or   traj[:min_index] = start;   reparametrize_trajectory()
// The trajectory is edited in the LDS image the reparametrisation (csrc/reparam.h) then works on, so the overwritten
// rows never travel to HBM.
//
// argmin is INDEX work: a delta that differs in the last bit flips a near-tie and with it every output.  So each delta
// is rn(rn(dx*dx) + rn(dy*dy)) -- torch's separate `** 2` and two-element `sum`, no contraction to fma -- and the
// order is torch's: a NaN is smaller than every number, equal keys (and NaNs among themselves) go to the lower index.
// The +1 of the SE(2) class and its absence in the 2-D class are the reference's own and are kept.
#include <limits.h>

#include "reparam.h"

namespace nfopp {

__device__ __forceinline__ float sq_dist_unfused(float dx, float dy) {
#pragma clang fp contract(off)
  const float xx = dx * dx;
  const float yy = dy * dy;
  return xx + yy;
}

// torch.argmin's order on (key, index) pairs (ATen LessOrNan): is pair a in front of pair b?
__device__ __forceinline__ bool argmin_before(float ka, int ia, float kb, int ib) {
  if (ka != ka) return (kb != kb) ? ia < ib : true;
  return ka == kb ? ia < ib : ka < kb;
}
struct ArgminFirst {
  __device__ __forceinline__ Indexed<float> operator()(Indexed<float> a, Indexed<float> b) const {
    return argmin_before(b.v, b.i, a.v, a.i) ? b : a;
  }
};

struct EndpointArgs {
  int n, which;                 // which: 0 = start, 1 = goal
  const float* points;          // [B, D] new endpoints
  const unsigned char* moved;   // [B] or NULL (= all)
  float* traj;
  float* start;
  float* goal;
  float* lam;
  float* cm;
  const float* u;
  int* min_index;               // [B] or NULL
};

template <int D>
__global__ __launch_bounds__(RP_THREADS) void endpoint_update_kernel(const EndpointArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int N = a.n, tid = threadIdx.x;
  const long long b = blockIdx.x;
  if (a.moved && !a.moved[b]) return;  // this trajectory keeps its endpoint: nothing of it is touched
  const bool is_goal = a.which == 1;
  const ReparamLds L = reparam_lds<D>(sm, N);
  float* traj = a.traj + b * N * D;
  float* lam = D == 3 ? a.lam + b * (N + 1) : nullptr;
  float* cm = D == 3 ? a.cm + b * N : nullptr;
  const float* point = a.points + b * D;
  reparam_load<D>(L, N, tid, traj, is_goal ? a.start + b * D : point, is_goal ? point : a.goal + b * D, lam, cm);
  if (tid < D) (is_goal ? a.goal : a.start)[b * D + tid] = point[tid];
  __syncthreads();

  // nearest waypoint: per-thread scan in rising index order, then the workgroup's reduction under the same order
  float* Q = L.Q;
  const float* P = Q + (is_goal ? (N + 1) * D : 0);   // the new endpoint's row of the image
  const float px = P[0], py = P[1];
  const Indexed<float> none = {__builtin_inff(), INT_MAX};   // loses to every waypoint, inf keys included
  Indexed<float> nearest = none;
  for (int w = tid; w < N; w += RP_THREADS)
    nearest = ArgminFirst()(nearest, {sq_dist_unfused(Q[(w + 1) * D] - px, Q[(w + 1) * D + 1] - py), w});
  constexpr int WAVES = RP_THREADS / 64;
  const IndexedScratch<float> wred = {L.red, reinterpret_cast<int*>(L.red + WAVES)};   // idle until the reparametrisation's sum
  const int idx = block_reduce<WAVES>(nearest, none, ArgminFirst(), wred).i;
  const int m = D == 3 ? min(idx + 1, N) : idx;       // constrained:182,190 vs nerf:206,214
  if (tid == 0 && a.min_index) a.min_index[b] = m;

  // traj[m:] = goal / traj[:m] = start (all D columns), on the image; the multipliers are interpolated, not overwritten
  float p[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = P[k];
  for (int w = tid; w < N; w += RP_THREADS) {
    if (is_goal ? w >= m : w < m) {
#pragma unroll
      for (int k = 0; k < D; ++k) Q[(w + 1) * D + k] = p[k];
    }
  }
  __syncthreads();
  reparam_from_lds<D>(L, N, tid, traj, lam, cm, a.u);
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_update_endpoints(int64_t batch, int32_t n_waypoints, int32_t dim, int32_t which,
                                      const float* new_points_dev, const uint8_t* moved_dev, float* traj_dev,
                                      float* start_dev, float* goal_dev, float* lam_dev, float* cm_dev, const float* u_dev,
                                      int32_t* min_index_out_dev, void* stream) {
  NFOPP_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  NFOPP_REQUIRE(which == 0 || which == 1, "which must be 0 (start) or 1 (goal)");
  NFOPP_REQUIRE(batch >= 0 && n_waypoints >= 2, "need batch >= 0 and at least 2 waypoints");
  NFOPP_REQUIRE(batch <= 0x7fffffffLL, "batch too large for one launch");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(new_points_dev && traj_dev && start_dev && goal_dev && u_dev, "null device pointer");
  NFOPP_REQUIRE(dim == 2 || (lam_dev && cm_dev), "the SE(2) endpoint update needs the multiplier arrays");
  EndpointArgs a;
  a.n = n_waypoints; a.which = which; a.points = new_points_dev; a.moved = moved_dev; a.traj = traj_dev;
  a.start = start_dev; a.goal = goal_dev; a.lam = lam_dev; a.cm = cm_dev; a.u = u_dev; a.min_index = min_index_out_dev;
  return launch_dynamic_lds(dim == 3 ? endpoint_update_kernel<3> : endpoint_update_kernel<2>, batch, RP_THREADS,
                            reparam_lds_bytes(n_waypoints, dim), stream, a, "trajectory too long");
}
