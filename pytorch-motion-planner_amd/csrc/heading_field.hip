// The heading-layered distance field: a third producer of the four floats per collision sample that
// nfopp_traj_update reads.  The image holds `layers` signed distance slices, slice k for the heading k * 2 pi / layers: how far
// the robot's centre may move at that heading before the footprint the slice was made from meets a wall.  It is the signed
// distance of the robot's configuration space, sampled in theta; a collision sample is one trilinear tap of it, whatever the
// robot's shape, and no sine or cosine is taken.
//
// One lane per sample, eight dword gathers from the plain [layers, rows, cols] image (two neighbouring slices, the four taps of
// sdf_field.hip in each), one 16-byte store.  No LDS, no scratch.  The image of a planning map stays in L2 / MALL; the
// kernel's HBM traffic is the poses in and 16 bytes per sample out.
//
// Arithmetic: fp32, every operation rounded on its own (contraction is off for this whole file); floorf and fmodf are exact.
// A float32 numpy restatement (tests/heading_field_ref.py) reproduces the kernel bit for bit for every robot.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "sdf_axis.h"

namespace nfopp {

struct HdfArgs {
  nfopp_heading_field f;
  const float* points;       // explicit mode: [n, 3]; NULL in trajectory mode
  const float* traj;         // trajectory mode: [B, N, 3]
  int n_way;
  float* t;                  // [B, N-1]
  int t_mode;
  unsigned long long seed, rng_offset;
  long long traj_index_offset;
  const unsigned char* active;
  long long n;               // samples: points, or B * (N - 1)
  float* out4;               // [n, 4], 16-byte aligned
};

// The bilinear tap of one slice at cell (j, i): distance and its slope in x and y (the latter two still without in_x / in_y).
struct SliceTap { float d, gx, gy; };
__device__ __forceinline__ SliceTap hdf_slice(const float* row0, int cols, float fu, float fv, float inv_res) {
  const float s00 = row0[0], s01 = row0[1], s10 = row0[cols], s11 = row0[cols + 1];
  const float a = s01 - s00, b = s11 - s10;
  const float top = s00 + fu * a, bot = s10 + fu * b;
  const float dv = bot - top;
  return SliceTap{top + fv * dv, (a + fv * (b - a)) * inv_res, dv * inv_res};
}

// One pose -> the row (logit, dlogit/dx, dlogit/dy, dlogit/dtheta).
__device__ __forceinline__ float4 hdf_eval_pose(const nfopp_heading_field& f, float x, float y, float th) {
  const float nan = __int_as_float(0x7fc00000);
  const float w = th * f.layers_per_rad;
  // x, y, th not finite, or th so large that w overflows: four NaNs, and nothing of the image is read
  if (!(isfinite(x) && isfinite(y) && isfinite(w))) return make_float4(nan, nan, nan, nan);
  const float kf = floorf(w);
  const float fw = w - kf;
  const int r = (int)fmodf(kf, (float)f.layers);       // exact, |r| < layers
  const int k0 = r < 0 ? r + f.layers : r;
  const int k1 = k0 + 1 == f.layers ? 0 : k0 + 1;
  const float u = (x - f.x0) * f.inv_res - 0.5f;
  const float v = (y - f.y0) * f.inv_res - 0.5f;
  int i, j;
  float fu, fv;
  bool in_x, in_y;
  sdf_axis(u, f.cols, i, fu, in_x);
  sdf_axis(v, f.rows, j, fv, in_y);
  // layers * rows * cols fits an int32 (checked on the host), so every index below does
  const int cell = j * f.cols + i, slice = f.rows * f.cols;
  const SliceTap t0 = hdf_slice(f.sd_dev + (k0 * slice + cell), f.cols, fu, fv, f.inv_res);
  const SliceTap t1 = hdf_slice(f.sd_dev + (k1 * slice + cell), f.cols, fu, fv, f.inv_res);
  const float dd = t1.d - t0.d;
  const float d = t0.d + fw * dd;
  const float gx = in_x ? t0.gx + fw * (t1.gx - t0.gx) : 0.0f;
  const float gy = in_y ? t0.gy + fw * (t1.gy - t0.gy) : 0.0f;
  const float gth = dd * f.layers_per_rad;
  const float pen = f.margin - d;
  return make_float4(f.gain * pen, f.gain * (-gx), f.gain * (-gy), f.gain * (-gth));
}

constexpr int HDF_THREADS = 256;

__global__ __launch_bounds__(HDF_THREADS) void hdf_points_kernel(const HdfArgs a) {
  const long long p = (long long)blockIdx.x * HDF_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const float* q = a.points + p * 3;
  reinterpret_cast<float4*>(a.out4)[p] = hdf_eval_pose(a.f, q[0], q[1], q[2]);
}

// Sample j of trajectory b: sample, draw and Philox counter as in sdf_traj_kernel (csrc/sdf_field.hip) and the ONF kernels.
// A lane whose trajectory is retired returns: its t and out4 rows keep their bytes.
__global__ __launch_bounds__(HDF_THREADS) void hdf_traj_kernel(const HdfArgs a) {
  const long long p = (long long)blockIdx.x * HDF_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const int nseg = a.n_way - 1;
  const long long b = p / nseg;
  const int j = (int)(p - b * nseg);
  if (a.active && a.active[b] == 0) return;
  const float* pa = a.traj + (b * a.n_way + j) * 3;   // traj[:-1]
  const float* pb = pa + 3;                            // traj[1:]
  const float qa[3] = {pa[0], pa[1], pa[2]}, qb[3] = {pb[0], pb[1], pb[2]};
  float tt;
  if (a.t_mode == 0) {
    tt = a.t[p];
  } else {
    tt = philox_uniform(a.seed, (unsigned long long)((a.traj_index_offset + b) * nseg + j), a.rng_offset);
    a.t[p] = tt;
  }
  const SamplePose s = collision_sample(3, qa, qb, tt);
  reinterpret_cast<float4*>(a.out4)[p] = hdf_eval_pose(a.f, s.x, s.y, s.ang);
}

// What every entry asks of the field.
static int check_heading_field(const nfopp_heading_field* f) {
  NFOPP_REQUIRE(f, "null field");
  NFOPP_REQUIRE(f->sd_dev, "null distance image");
  NFOPP_REQUIRE(f->layers >= 2 && f->layers <= 64, "a heading field has 2 to 64 layers, not %d", f->layers);
  NFOPP_REQUIRE(f->rows >= 2 && f->cols >= 2, "a distance image needs at least 2 x 2 cells, not %d x %d", f->rows, f->cols);
  NFOPP_REQUIRE((int64_t)f->layers * f->rows * f->cols <= 0x7fffffffLL, "layers x rows x cols must fit a 32-bit index");
  NFOPP_REQUIRE(std::isfinite(f->x0) && std::isfinite(f->y0) && std::isfinite(f->inv_res) && std::isfinite(f->layers_per_rad) &&
                    std::isfinite(f->margin) && std::isfinite(f->gain),
                "x0, y0, inv_res, layers_per_rad, margin and gain must be finite");
  return NFOPP_OK;
}

static int check_heading_out(const float* out4_dev, int64_t n) {
  NFOPP_REQUIRE(((uintptr_t)out4_dev & 15) == 0, "out4_dev must be 16-byte aligned");
  NFOPP_REQUIRE(n <= (int64_t)0x7fffffff * HDF_THREADS, "too many samples for one launch");
  return NFOPP_OK;
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_hdf_eval_points(const nfopp_heading_field* field, const float* points_dev, int64_t n, float* out4_dev,
                                     void* stream) {
  int rc = check_heading_field(field);
  if (rc != NFOPP_OK) return rc;
  NFOPP_REQUIRE(n >= 0, "negative point count");
  NFOPP_REQUIRE(n == 0 || (points_dev && out4_dev), "null device pointer");
  rc = check_heading_out(out4_dev, n);
  if (rc != NFOPP_OK) return rc;
  HdfArgs a = {};
  a.f = *field;
  a.points = points_dev;
  a.n = n;
  a.out4 = out4_dev;
  return launch_per_item<HDF_THREADS>(hdf_points_kernel, n, stream, a);
}

extern "C" int nfopp_traj_hdf_collision_eval(const nfopp_heading_field* field, const float* traj_dev, int64_t batch,
                                             int32_t n_waypoints, float* t_dev, int32_t t_mode, uint64_t seed,
                                             uint64_t rng_offset, int64_t traj_index_offset, float* out4_dev,
                                             const uint8_t* active_dev, void* stream) {
  int rc = check_heading_field(field);
  if (rc != NFOPP_OK) return rc;
  NFOPP_REQUIRE(batch >= 0 && n_waypoints >= 2, "need batch >= 0 and at least 2 waypoints");
  NFOPP_REQUIRE(batch == 0 || (traj_dev && t_dev && out4_dev), "null device pointer");
  NFOPP_REQUIRE(t_mode == 0 || t_mode == 1, "t_mode must be 0 (read) or 1 (Philox)");
  NFOPP_REQUIRE(batch <= 0x7fffffffLL, "batch too large for one launch");
  const int64_t n = batch * (int64_t)(n_waypoints - 1);
  rc = check_heading_out(out4_dev, n);
  if (rc != NFOPP_OK) return rc;
  HdfArgs a = {};
  a.f = *field;
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
  return launch_per_item<HDF_THREADS>(hdf_traj_kernel, n, stream, a);
}
