// The distance-field collision term: a second producer of the four floats per collision sample that
// nfopp_traj_update reads -- a logit and its gradient in x, y and theta -- from the signed distance image of an occupancy
// grid (OccupancyGrid.signed_distance_field) instead of the occupancy network.  The robot is a handful of discs in the body
// frame; per disc one bilinear tap of the image; the disc that penetrates deepest gives the row.  This is the obstacle
// cost of CHOMP / GPMP2 (the reference compares itself against it in scripts/run_gpmp2.py).
//
// One lane per sample, a loop over the discs, four dword gathers per disc from the plain image.  The image of a planning
// map (590 KB at 384 x 384) stays in L2; the kernel's HBM traffic is the poses in and 16 bytes per sample out.
//
// Arithmetic: fp32, every operation rounded on its own (contraction is off for this whole file), so that a float32 numpy
// restatement (tests/sdf_ref.py) reproduces the kernel bit for bit wherever no sine or cosine is involved.
#include "common.h"

#pragma clang fp contract(off)

#include "sdf_axis.h"

namespace nfopp {

struct SdfArgs {
  nfopp_sdf_field f;
  const float* points;       // explicit mode: [n, point_dim]; NULL in trajectory mode
  int point_dim;
  const float* traj;         // trajectory mode: [B, N, dim]
  int n_way;
  float* t;                  // [B, N-1]
  int t_mode;
  unsigned long long seed, rng_offset;
  long long traj_index_offset;
  const unsigned char* active;
  long long n;               // samples: points, or B * (N - 1)
  float* out4;               // [n, 4], 16-byte aligned
};

// One pose -> the row (logit, dlogit/dx, dlogit/dy, dlogit/dtheta).  `dim` 2: no heading, dlogit/dtheta = 0.
__device__ __forceinline__ float4 sdf_eval_pose(const nfopp_sdf_field& f, int dim, bool any_offset, float x, float y,
                                                float th) {
  const float nan = __int_as_float(0x7fc00000);
  if (!(isfinite(x) && isfinite(y) && (dim == 2 || isfinite(th)))) return make_float4(nan, nan, nan, nan);
  // robots of centred discs never evaluate a sine: (c, s) = (1, 0) stands in, and every lever below is a zero
  float c = 1.0f, s = 0.0f;
  if (any_offset) { c = cosf(th); s = sinf(th); }
  float pen = 0.0f, gx = 0.0f, gy = 0.0f, lx = 0.0f, ly = 0.0f;
  for (int k = 0; k < f.n_discs; ++k) {
    const float ox = f.disc[k][0], oy = f.disc[k][1];
    const bool centred = ox == 0.0f && oy == 0.0f;
    const float cx = centred ? x : (x + ox * c) - oy * s;
    const float cy = centred ? y : (y + ox * s) + oy * c;
    const float u = (cx - f.x0) * f.inv_res - 0.5f;
    const float v = (cy - f.y0) * f.inv_res - 0.5f;
    int i, j;
    float fu, fv;
    bool in_x, in_y;
    sdf_axis(u, f.cols, i, fu, in_x);
    sdf_axis(v, f.rows, j, fv, in_y);
    const float* row0 = f.sd_dev + (long long)j * f.cols + i;
    const float s00 = row0[0], s01 = row0[1], s10 = row0[f.cols], s11 = row0[f.cols + 1];
    const float a = s01 - s00, b = s11 - s10;
    const float top = s00 + fu * a, bot = s10 + fu * b;
    const float d = top + fv * (bot - top);
    const float pk = (f.disc[k][2] + f.margin) - d;
    if (k == 0 || pk > pen) {
      pen = pk;
      gx = in_x ? (a + fv * (b - a)) * f.inv_res : 0.0f;
      gy = in_y ? (bot - top) * f.inv_res : 0.0f;
      lx = (-ox) * s - oy * c;   // d cx / d theta
      ly = ox * c - oy * s;      // d cy / d theta
    }
  }
  const float ngx = -gx, ngy = -gy;
  return make_float4(f.gain * pen, f.gain * ngx, f.gain * ngy, dim == 2 ? 0.0f : f.gain * (ngx * lx + ngy * ly));
}

__device__ __forceinline__ bool sdf_any_offset(const nfopp_sdf_field& f) {
  bool any = false;
  for (int k = 0; k < f.n_discs; ++k) any = any || f.disc[k][0] != 0.0f || f.disc[k][1] != 0.0f;
  return any;
}

constexpr int SDF_THREADS = 256;

__global__ __launch_bounds__(SDF_THREADS) void sdf_points_kernel(const SdfArgs a) {
  const long long p = (long long)blockIdx.x * SDF_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const float* q = a.points + p * a.point_dim;
  const float th = a.point_dim == 3 ? q[2] : 0.0f;
  reinterpret_cast<float4*>(a.out4)[p] = sdf_eval_pose(a.f, a.point_dim, sdf_any_offset(a.f), q[0], q[1], th);
}

// Sample j of trajectory b, draw and Philox counter as in the ONF kernels (csrc/onf_layout.h: point_fetch / point_finish).
// A lane whose trajectory is retired returns: its t and out4 rows keep their bytes.
__global__ __launch_bounds__(SDF_THREADS) void sdf_traj_kernel(const SdfArgs a) {
  const long long p = (long long)blockIdx.x * SDF_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const int nseg = a.n_way - 1;
  const long long b = p / nseg;
  const int j = (int)(p - b * nseg);
  if (a.active && a.active[b] == 0) return;
  const int dim = a.point_dim;
  const float* pa = a.traj + (b * a.n_way + j) * dim;   // traj[:-1]
  const float* pb = pa + dim;                            // traj[1:]
  const float qa[3] = {pa[0], pa[1], dim == 3 ? pa[2] : 0.0f}, qb[3] = {pb[0], pb[1], dim == 3 ? pb[2] : 0.0f};
  float tt;
  if (a.t_mode == 0) {
    tt = a.t[p];
  } else {
    tt = philox_uniform(a.seed, (unsigned long long)((a.traj_index_offset + b) * nseg + j), a.rng_offset);
    a.t[p] = tt;
  }
  const SamplePose s = collision_sample(dim, qa, qb, tt);
  reinterpret_cast<float4*>(a.out4)[p] = sdf_eval_pose(a.f, dim, sdf_any_offset(a.f), s.x, s.y, s.ang);
}

// What both entries ask of the field and of the robot for poses of `dim` components.
static int check_field(const nfopp_sdf_field* f, int32_t dim) {
  NFOPP_REQUIRE(f, "null field");
  NFOPP_REQUIRE(dim == 2 || dim == 3, "poses have 2 or 3 components, not %d", dim);
  NFOPP_REQUIRE(f->sd_dev, "null distance image");
  NFOPP_REQUIRE(f->rows >= 2 && f->cols >= 2, "a distance image needs at least 2 x 2 cells, not %d x %d", f->rows, f->cols);
  NFOPP_REQUIRE(f->n_discs >= 1 && f->n_discs <= 8, "a robot has 1 to 8 discs, not %d", f->n_discs);
  NFOPP_REQUIRE(dim == 3 || (f->n_discs == 1 && f->disc[0][0] == 0.0f && f->disc[0][1] == 0.0f),
                "a robot without a heading (dim 2) is one disc with a zero offset");
  return NFOPP_OK;
}

static int check_out(const float* out4_dev, int64_t n) {
  NFOPP_REQUIRE(((uintptr_t)out4_dev & 15) == 0, "out4_dev must be 16-byte aligned");
  NFOPP_REQUIRE(n <= (int64_t)0x7fffffff * SDF_THREADS, "too many samples for one launch");
  return NFOPP_OK;
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_sdf_eval_points(const nfopp_sdf_field* field, const float* points_dev, int64_t n, int32_t point_dim,
                                     float* out4_dev, void* stream) {
  int rc = check_field(field, point_dim);
  if (rc != NFOPP_OK) return rc;
  NFOPP_REQUIRE(n >= 0, "negative point count");
  NFOPP_REQUIRE(n == 0 || (points_dev && out4_dev), "null device pointer");
  rc = check_out(out4_dev, n);
  if (rc != NFOPP_OK) return rc;
  SdfArgs a = {};
  a.f = *field;
  a.points = points_dev;
  a.point_dim = point_dim;
  a.n = n;
  a.out4 = out4_dev;
  return launch_per_item<SDF_THREADS>(sdf_points_kernel, n, stream, a);
}

extern "C" int nfopp_traj_sdf_collision_eval(const nfopp_sdf_field* field, const float* traj_dev, int64_t batch,
                                             int32_t n_waypoints, int32_t dim, float* t_dev, int32_t t_mode, uint64_t seed,
                                             uint64_t rng_offset, int64_t traj_index_offset, float* out4_dev,
                                             const uint8_t* active_dev, void* stream) {
  int rc = check_field(field, dim);
  if (rc != NFOPP_OK) return rc;
  NFOPP_REQUIRE(batch >= 0 && n_waypoints >= 2, "need batch >= 0 and at least 2 waypoints");
  NFOPP_REQUIRE(batch == 0 || (traj_dev && t_dev && out4_dev), "null device pointer");
  NFOPP_REQUIRE(t_mode == 0 || t_mode == 1, "t_mode must be 0 (read) or 1 (Philox)");
  NFOPP_REQUIRE(batch <= 0x7fffffffLL, "batch too large for one launch");
  const int64_t n = batch * (int64_t)(n_waypoints - 1);
  rc = check_out(out4_dev, n);
  if (rc != NFOPP_OK) return rc;
  SdfArgs a = {};
  a.f = *field;
  a.point_dim = dim;
  a.traj = traj_dev;
  a.n_way = n_waypoints;
  a.t = t_dev;
  a.t_mode = t_mode;
  a.seed = seed;
  a.rng_offset = rng_offset;
  a.traj_index_offset = traj_index_offset;
  a.active = active_dev;
  a.n = n;
  a.out4 = out4_dev;
  return launch_per_item<SDF_THREADS>(sdf_traj_kernel, n, stream, a);
}
