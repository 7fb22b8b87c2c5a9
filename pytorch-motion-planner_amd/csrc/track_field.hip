// The moving-obstacle collision term: a pass over the four floats per collision sample that one of the
// collision entries (the ONF, csrc/sdf_field.hip, csrc/heading_field.hip) has just written.  The obstacles are discs on
// predicted tracks [M, K, stride], linear in time between the instants of a uniform grid; every sample has a time, formed from
// the waypoint times with the sample's own draw.  Where a moving obstacle penetrates the robot's discs deeper than the row
// says, the row is replaced by the moving obstacle's: "the deepest disc gives the row" of DESIGN.md 24, extended over time.
//
// One lane per sample, 256-lane workgroups, one 16-byte load of the row and at most one 16-byte store.  The inner loop reads
// two positions per track from the plain tensor (64 tracks x 256 instants are 128 KB: L2, and the lanes of a wave, which are
// neighbouring samples of one trajectory, read neighbouring instants).  No LDS, no scratch.  The layouts that were tried
// against this one: tools/micro/track_layouts.hip.
//
// Arithmetic: fp32, every operation rounded on its own (contraction is off for this whole file), so that a float32 numpy
// restatement (tests/track_field_ref.py) reproduces the kernel bit for bit wherever no sine or cosine is involved.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "track_eval.h"
#include "track_field.h"

namespace nfopp {

struct TrackArgs {
  nfopp_track_field f;
  const float* points;       // explicit mode: [n, dim]; NULL in trajectory mode
  const float* times;        // explicit mode: [n]
  int dim;
  const float* traj;         // trajectory mode: [B, N, dim]
  const float* wp_time;      // [B, N]
  int n_way;
  const float* t;            // [B, N-1], read only
  const unsigned char* active;
  long long n;               // samples: points, or B * (N - 1)
  float* out4;               // [n, 4], 16-byte aligned, in-out
};

// The row of sample p against the tracks, stored over the row in out4 iff its logit is strictly larger.  A sample with a
// component or a time that is not finite reads no track and keeps its row.
template <bool PAIR>
__device__ __forceinline__ void track_overlay(const TrackArgs& a, long long p, float x, float y, float th, float tau) {
  if (!(isfinite(x) && isfinite(y) && (a.dim == 2 || isfinite(th)) && isfinite(tau))) return;
  float4* const row = reinterpret_cast<float4*>(a.out4) + p;
  const float4 base = *row;
  const TrackGather<PAIR> fetch{a.f.tracks_dev, a.f.k, a.f.stride};
  const float4 r = track_eval_pose(a.f, fetch, a.dim, track_any_offset(a.f), x, y, th, tau);
  if (r.x > base.x) *row = r;
}

constexpr int TRACK_THREADS = 256;

template <bool PAIR>
__global__ __launch_bounds__(TRACK_THREADS) void track_points_kernel(const TrackArgs a) {
  const long long p = (long long)blockIdx.x * TRACK_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const float* q = a.points + p * a.dim;
  track_overlay<PAIR>(a, p, q[0], q[1], a.dim == 3 ? q[2] : 0.0f, a.times[p]);
}

// Sample j of trajectory b, as in sdf_traj_kernel (csrc/sdf_field.hip), at the draw the collision entry used; its time is
// formed from the two waypoint times as the heading-free sample is formed from the two waypoints.
template <bool PAIR>
__global__ __launch_bounds__(TRACK_THREADS) void track_traj_kernel(const TrackArgs a) {
  const long long p = (long long)blockIdx.x * TRACK_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const int nseg = a.n_way - 1;
  const long long b = p / nseg;
  const int j = (int)(p - b * nseg);
  if (a.active && a.active[b] == 0) return;
  const int dim = a.dim;
  const float* pa = a.traj + (b * a.n_way + j) * dim;   // traj[:-1]
  const float* pb = pa + dim;                            // traj[1:]
  const float qa[3] = {pa[0], pa[1], dim == 3 ? pa[2] : 0.0f}, qb[3] = {pb[0], pb[1], dim == 3 ? pb[2] : 0.0f};
  const float tt = a.t[p];
  const SamplePose s = collision_sample(dim, qa, qb, tt);
  const float* w = a.wp_time + b * a.n_way + j;
  const float tau = w[1] + tt * (w[0] - w[1]);
  track_overlay<PAIR>(a, p, s.x, s.y, s.ang, tau);
}

template <bool PAIR>
static int launch_track(bool traj_mode, const TrackArgs& a, void* stream) {
  return launch_per_item<TRACK_THREADS>(traj_mode ? track_traj_kernel<PAIR> : track_points_kernel<PAIR>, a.n, stream, a);
}

static int launch_track(bool traj_mode, const TrackArgs& a, void* stream) {
  const bool pair = a.f.stride % 2 == 0 && ((uintptr_t)a.f.tracks_dev & 7) == 0;
  return pair ? launch_track<true>(traj_mode, a, stream) : launch_track<false>(traj_mode, a, stream);
}

int check_track_field(const nfopp_track_field* f, int32_t dim) {
  NFOPP_REQUIRE(f, "null track field");
  NFOPP_REQUIRE(dim == 2 || dim == 3, "poses have 2 or 3 components, not %d", dim);
  NFOPP_REQUIRE(f->m >= 0 && f->k >= 1 && f->stride >= 2, "tracks are [M >= 0, K >= 1, stride >= 2], not [%d, %d, %d]", f->m,
                f->k, f->stride);
  NFOPP_REQUIRE(f->m == 0 || f->tracks_dev, "null tracks");
  NFOPP_REQUIRE((int64_t)f->m * f->k * f->stride <= 0x7fffffffLL, "M x K x stride must fit a 32-bit index");
  NFOPP_REQUIRE(f->n_discs >= 1 && f->n_discs <= 8, "a robot has 1 to 8 discs, not %d", f->n_discs);
  NFOPP_REQUIRE(dim == 3 || (f->n_discs == 1 && f->disc[0][0] == 0.0f && f->disc[0][1] == 0.0f),
                "a robot without a heading (dim 2) is one disc with a zero offset");
  NFOPP_REQUIRE(std::isfinite(f->t0) && std::isfinite(f->inv_dt) && std::isfinite(f->margin) && std::isfinite(f->gain),
                "t0, inv_dt, margin and gain must be finite");
  NFOPP_REQUIRE(f->inv_dt > 0.0f, "inv_dt must be positive");
  return NFOPP_OK;
}

int check_track_overlay(const nfopp_track_field* f, const float* wp_time_dev, int64_t batch, int32_t n_waypoints, int32_t dim,
                        const float* out4_dev) {
  const int rc = check_track_field(f, dim);
  if (rc != NFOPP_OK) return rc;
  NFOPP_REQUIRE(batch >= 0 && n_waypoints >= 2, "need batch >= 0 and at least 2 waypoints");
  NFOPP_REQUIRE(batch == 0 || wp_time_dev, "null waypoint times");
  NFOPP_REQUIRE(batch <= 0x7fffffffLL, "batch too large for one launch");
  NFOPP_REQUIRE(((uintptr_t)out4_dev & 15) == 0, "out4_dev must be 16-byte aligned");
  NFOPP_REQUIRE(batch * (int64_t)(n_waypoints - 1) <= (int64_t)0x7fffffff * TRACK_THREADS, "too many samples for one launch");
  return NFOPP_OK;
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_track_field_eval_points(const nfopp_track_field* field, const float* points_dev, const float* times_dev,
                                             int64_t n, int32_t dim, float* out4_dev, void* stream) {
  const int rc = check_track_field(field, dim);
  if (rc != NFOPP_OK) return rc;
  NFOPP_REQUIRE(n >= 0, "negative point count");
  NFOPP_REQUIRE(n == 0 || (points_dev && times_dev && out4_dev), "null device pointer");
  NFOPP_REQUIRE(((uintptr_t)out4_dev & 15) == 0, "out4_dev must be 16-byte aligned");
  NFOPP_REQUIRE(n <= (int64_t)0x7fffffff * TRACK_THREADS, "too many samples for one launch");
  if (field->m == 0) return NFOPP_OK;
  TrackArgs a = {};
  a.f = *field;
  a.points = points_dev;
  a.times = times_dev;
  a.dim = dim;
  a.n = n;
  a.out4 = out4_dev;
  return launch_track(false, a, stream);
}

extern "C" int nfopp_traj_track_overlay(const nfopp_track_field* field, const float* traj_dev, const float* wp_time_dev,
                                        int64_t batch, int32_t n_waypoints, int32_t dim, const float* t_dev, float* out4_dev,
                                        const uint8_t* active_dev, void* stream) {
  const int rc = check_track_overlay(field, wp_time_dev, batch, n_waypoints, dim, out4_dev);
  if (rc != NFOPP_OK) return rc;
  NFOPP_REQUIRE(batch == 0 || (traj_dev && t_dev && out4_dev), "null device pointer");
  if (field->m == 0) return NFOPP_OK;
  TrackArgs a = {};
  a.f = *field;
  a.dim = dim;
  a.traj = traj_dev;
  a.wp_time = wp_time_dev;
  a.n_way = n_waypoints;
  a.t = t_dev;
  a.active = active_dev;
  a.n = batch * (int64_t)(n_waypoints - 1);
  a.out4 = out4_dev;
  return launch_track(true, a, stream);
}
