// Arc-length reparametrisation kernel (HBM-bound; one workgroup per trajectory; runs every
// `reparametrize_trajectory_freq` steps).  The body -- and the account of the torch-CPU roundings it restates -- is in
// csrc/reparam.h, shared with the endpoint update (csrc/endpoint_update.hip).
#include "reparam.h"

namespace nfopp {

struct ReparamArgs {
  int n, dim;
  float* traj;
  const float* start;
  const float* goal;
  float* lam;
  float* cm;
  const float* u;
  const unsigned char* active;
};

template <int D>
__global__ __launch_bounds__(RP_THREADS) void reparam_kernel(const ReparamArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int N = a.n, tid = threadIdx.x;
  const long long b = blockIdx.x;
  if (a.active && !a.active[b]) return;  // retired trajectory
  const ReparamLds L = reparam_lds<D>(sm, N);
  float* traj = a.traj + b * N * D;
  float* lam = D == 3 ? a.lam + b * (N + 1) : nullptr;
  float* cm = D == 3 ? a.cm + b * N : nullptr;
  reparam_load<D>(L, N, tid, traj, a.start + b * D, a.goal + b * D, lam, cm);
  __syncthreads();
  reparam_from_lds<D>(L, N, tid, traj, lam, cm, a.u);
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_reparametrize(int64_t batch, int32_t n_waypoints, int32_t dim, float* traj_dev,
                                   const float* start_dev, const float* goal_dev, float* lam_dev, float* cm_dev,
                                   const float* u_dev, const uint8_t* active_dev, void* stream) {
  NFOPP_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  NFOPP_REQUIRE(batch >= 0 && n_waypoints >= 2, "need batch >= 0 and at least 2 waypoints");
  NFOPP_REQUIRE(batch <= 0x7fffffffLL, "batch too large for one launch");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(traj_dev && start_dev && goal_dev && u_dev, "null device pointer");
  NFOPP_REQUIRE(dim == 2 || (lam_dev && cm_dev), "SE(2) reparametrisation needs the multiplier arrays");
  ReparamArgs a;
  a.n = n_waypoints; a.dim = dim; a.traj = traj_dev; a.start = start_dev; a.goal = goal_dev;
  a.lam = lam_dev; a.cm = cm_dev; a.u = u_dev; a.active = active_dev;
  return launch_dynamic_lds(dim == 3 ? reparam_kernel<3> : reparam_kernel<2>, batch, RP_THREADS,
                            reparam_lds_bytes(n_waypoints, dim), stream, a, "trajectory too long");
}
