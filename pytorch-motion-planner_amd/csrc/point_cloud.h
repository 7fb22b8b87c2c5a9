// What every kernel over the obstacle point cloud shares: the uniform cell index (built by csrc/obstacle_map.hip, searched
// by the *_cells checkers of csrc/sampling.hip, the nearest-obstacle query of csrc/clearance.hip and the swept check of
// csrc/swept.hip), the robot's shape and
// the all-pairs visit.  The index is sound only if all three form a cell number the same way, and `dist < radius` of the
// query is the circle checker's obstacle term only if both evaluate one expression: each is written once, here.
//
// RULE for the fp32 arithmetic of this header: csrc/clearance.hip compiles under `#pragma clang fp contract(off)`,
// csrc/sampling.hip does not, so a product feeding a plain add or subtract would be one fma in one file and two roundings in
// the other.  Every multiply-add is an explicit __builtin_fmaf; everything else is one operation per statement.
#pragma once
#include "block_collectives.h"
#include "common.h"

namespace nfopp {

constexpr int MAX_INDEX_CELLS = 65536;   // cell numbers are the build's 16-bit sort key and enter the ring search's bound

// cells_x * cells_y cells of `size` from (x0, y0), row-major; cell_start[c] .. cell_start[c + 1]: the sorted points of cell c
struct CellIndex {
  const int* cell_start; int cells_x, cells_y; float x0, y0, size;

  // cell of a coordinate along an axis of n cells: fp32 subtract, divide, floor, clamp.  Clamped as a float, so no value out
  // of int's range is ever converted: anything outside, +-inf included, lands in a border cell, a NaN in cell 0.
  __device__ __forceinline__ static int axis_cell(float v, float v0, float size, int n) {
    return (int)fminf(fmaxf(floorf((v - v0) / size), 0.f), (float)(n - 1));
  }
  __device__ __forceinline__ void cell(float x, float y, int* cx, int* cy) const {
    *cx = axis_cell(x, x0, size, cells_x);
    *cy = axis_cell(y, y0, size, cells_y);
  }
  // [*k0, *k1): the sorted points of cells x_lo..x_hi of row yy (consecutive cell numbers, so one contiguous run)
  __device__ __forceinline__ void row_range(int yy, int x_lo, int x_hi, int* k0, int* k1) const {
    *k0 = cell_start[yy * cells_x + x_lo];
    *k1 = cell_start[yy * cells_x + x_hi + 1];
  }
};

struct PointCloud { const float* points; int n; CellIndex index; };   // [n, 2]; cell-sorted where the index is used

// |obstacle - pose| for an obstacle (dx, dy) away from the pose
__device__ __forceinline__ float disc_distance(float dx, float dy) { return sqrtf(__builtin_fmaf(dx, dx, dy * dy)); }

// the obstacle (dx, dy away from the pose) in the frame of a robot heading (c, s) = (cos, sin): the form the brute-force
// rectangle kernel has always compiled to
__device__ __forceinline__ void robot_frame(float dx, float dy, float c, float s, float* rx, float* ry) {
  *rx = __builtin_fmaf(c, dx, s * dy);
  *ry = __builtin_fmaf(c, dy, -(s * dx));
}

struct Pose { float x, y, c, s; bool finite; };

// MODE 0: disc robot (circle_collision_checker.py:11-14), heading unused.  MODE 1: box robot, obstacle points moved into
// the robot frame (rectangle_collision_checker.py:11-26).  `finite` is false for a pose with a NaN or infinite component:
// it has no distance (fmaxf would drop a NaN of the box arithmetic and report 0).  The labels do not consult it.
template <int MODE>
__device__ __forceinline__ Pose load_pose(const float* poses, int dim, long long p) {
  Pose q = {poses[p * dim], poses[p * dim + 1], 1.f, 0.f, false};
  q.finite = isfinite(q.x) && isfinite(q.y);
  if (MODE == 1) {
    const float th = poses[p * dim + 2];
    q.finite = q.finite && isfinite(th);
    q.c = cosf(th); q.s = sinf(th);
  }
  return q;
}

struct Robot {
  float radius;   // MODE 0
  float box[4];   // MODE 1: x0, x1, y0, y1 in the robot's frame
  float reach;    // MODE 1: box_reach(box), what the ring search allows for the box's extent; 0 for the disc

  // the checkers' predicate: obstacle point strictly inside the disc / the box of the robot at pose q
  template <int MODE>
  __device__ __forceinline__ bool hits(const Pose& q, float ox, float oy) const {
    const float dx = ox - q.x, dy = oy - q.y;
    if (MODE == 0) return disc_distance(dx, dy) < radius;
    float rx, ry;
    robot_frame(dx, dy, q.c, q.s, &rx, &ry);
    return (rx > box[0]) & (rx < box[1]) & (ry > box[2]) & (ry < box[3]);
  }

  // distance from the point to the robot: the left side of the disc's comparison / to the closed box (0 inside, 0 on the rim)
  template <int MODE>
  __device__ __forceinline__ float point_distance(const Pose& q, float ox, float oy) const {
    const float dx = ox - q.x, dy = oy - q.y;
    if (MODE == 0) return disc_distance(dx, dy);
    float rx, ry;
    robot_frame(dx, dy, q.c, q.s, &rx, &ry);
    const float ex = fmaxf(fmaxf(box[0] - rx, rx - box[1]), 0.f);
    const float ey = fmaxf(fmaxf(box[2] - ry, ry - box[3]), 0.f);
    return disc_distance(ex, ey);
  }
};

// (best, bestk) <- lexicographic minimum with (d, k): what "the nearest point, the smallest index among equals" means in
// csrc/clearance.hip and csrc/swept.hip.  A NaN or +inf distance never enters: the initial (+inf, -1) stays.
__device__ __forceinline__ void take_min(float d, int k, float* best, int* bestk) {
  if (d < *best || (d == *best && k < *bestk)) { *best = d; *bestk = k; }
}
struct TakeMin {   // take_min as the op of a reduction over (distance, index) pairs
  __device__ __forceinline__ Indexed<float> operator()(Indexed<float> a, Indexed<float> b) const {
    take_min(b.v, b.i, &a.v, &a.i);
    return a;
  }
};

// All pairs: f(ox, oy, k) for every point k of the cloud in ascending k.  The points pass through the workgroup's LDS arrays
// ox, oy [THREADS] a tile at a time between two barriers, so every thread has to call this, one without a pose included.
template <int THREADS, class F>
__device__ __forceinline__ void for_all_points(const PointCloud& cloud, float* ox, float* oy, F&& f) {
  for (int base = 0; base < cloud.n; base += THREADS) {
    __syncthreads();
    if (base + (int)threadIdx.x < cloud.n) {
      ox[threadIdx.x] = cloud.points[2 * (long long)(base + threadIdx.x)];
      oy[threadIdx.x] = cloud.points[2 * (long long)(base + threadIdx.x) + 1];
    }
    __syncthreads();
    const int m = min(THREADS, cloud.n - base);
    for (int k = 0; k < m; ++k) f(ox[k], oy[k], base + k);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// The six index arguments of the C ABI with the checks every indexed entry makes; `cell_start_dev` may be null only where
// the caller says that nothing will read it (an index over no points).
static inline int fill_cell_index(CellIndex* ix, const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y,
                                  float cell_x0, float cell_y0, float cell_size, bool needs_cell_start = true) {
  NFOPP_REQUIRE(cells_x > 0 && cells_y > 0, "the cell index needs at least one cell along each axis");
  NFOPP_REQUIRE(cell_size > 0.f, "the cell size must be positive");   // false for a NaN too
  NFOPP_REQUIRE(cell_start_dev || !needs_cell_start, "null cell index");
  *ix = {cell_start_dev, cells_x, cells_y, cell_x0, cell_y0, cell_size};
  return NFOPP_OK;
}

// largest distance from the robot's origin to a corner of its box (the box need not contain the origin) ...
static inline float box_corner(const float* box4) {
  return hypotf(fmaxf(fabsf(box4[0]), fabsf(box4[1])), fmaxf(fabsf(box4[2]), fabsf(box4[3])));
}
// ... rounded up, so the box lies inside the disc of this radius whatever hypotf's last bit is
// (DeviceRectangleChecker._reach of nfopp/learning.py is the Python statement)
static inline float box_reach(const float* box4) { return box_corner(box4) * 1.000001f; }
static inline void set_box(Robot* r, const float* box4) {
  for (int k = 0; k < 4; ++k) r->box[k] = box4[k];
  r->reach = box_reach(box4);
}

}  // namespace nfopp
