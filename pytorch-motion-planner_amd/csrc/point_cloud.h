// What every kernel over the obstacle point cloud shares: the uniform cell index, the robot's shape, the visits of the points
// (all pairs; the sorted points of a window of cells) and the host's side of an entry that takes a cloud and a robot.
// Users: csrc/obstacle_map.hip builds the index (CellIndex::cell); the checkers of csrc/sampling.hip, the nearest-obstacle
// query of csrc/clearance.hip and the swept check and its refinement of csrc/swept.hip search it (for_row_points,
// for_window_points), visit every point (for_all_points) and open their entries with fill_scene.  The index is sound only
// if all of them form a cell number the same way, `dist < radius` of the query is the circle checker's obstacle term only
// if both evaluate one expression, and an indexed entry writes its all-pairs partner's bytes only if each visit is one loop:
// every one of these is written once, here.
//
// RULE for the fp32 arithmetic of this header: csrc/clearance.hip compiles under `#pragma clang fp contract(off)`,
// csrc/sampling.hip does not, so a product feeding a plain add or subtract would be one fma in one file and two roundings in
// the other.  Every multiply-add is an explicit __builtin_fmaf; everything else is one operation per statement.
#pragma once
#include "block_collectives.h"
#include "common.h"

namespace nfopp {

constexpr int MAX_INDEX_CELLS = 65536;   // cell numbers are the build's 16-bit sort key and enter the ring search's bound

struct CellWindow { int x_lo, y_lo, x_hi, y_hi; };   // a rectangle of cells, both ends included, inside the index

__device__ __forceinline__ float outward(float w, float sign) {   // w moved by 4 * 2^-24 |w| towards sign * inf
  return __builtin_fmaf(fabsf(w), sign * 2.384185791015625e-07f, w);
}

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
  // the cell of (x, y) grown by r cells per side
  __device__ __forceinline__ CellWindow window_around(float x, float y, int r) const {
    int cx, cy;
    cell(x, y, &cx, &cy);
    return {max(cx - r, 0), max(cy - r, 0), min(cx + r, cells_x - 1), min(cy + r, cells_y - 1)};
  }
  // The cells of the bounding box of (ax, ay) and (bx, by) inflated by r, and one further cell per side: every cell that can
  // hold a point within r of the segment between the two.  From coordinates to cells: each bound w = min - r or max + r is
  // formed in fp32 and then moved outward by 4 * 2^-24 |w|, more than the rounding of its own two operations, so the fp32
  // bound encloses the exact one.  axis_cell is a chain of monotone operations (correctly rounded subtraction and division,
  // floor, clamp), and points and bounds go through that one function: lo <= ox <= hi implies
  // cell(lo) <= cell(ox) <= cell(hi), for a point clamped into a border cell too.  One further cell is visited on each side:
  // it costs a few points per segment and keeps the coverage from resting on the last bit of this argument and of the one
  // that gave r (csrc/swept.hip, (1) and (2)).
  __device__ __forceinline__ CellWindow window_of_box(float ax, float ay, float bx, float by, float r) const {
    const float lox = outward(fminf(ax, bx) - r, -1.f), hix = outward(fmaxf(ax, bx) + r, 1.f);
    const float loy = outward(fminf(ay, by) - r, -1.f), hiy = outward(fmaxf(ay, by) + r, 1.f);
    int x_lo, y_lo, x_hi, y_hi;
    cell(lox, loy, &x_lo, &y_lo);
    cell(hix, hiy, &x_hi, &y_hi);
    return {max(x_lo - 1, 0), max(y_lo - 1, 0), min(x_hi + 1, cells_x - 1), min(y_hi + 1, cells_y - 1)};
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

// The two visits of the points.  Both call f(ox, oy, k, j): point k of the cloud, the jth the visit comes to.  A query passes
// one functor to either, so its all-pairs and its indexed kernel differ in the visit alone.
// All pairs: every point k of the cloud in ascending k (j = k).  The points pass through the workgroup's LDS arrays
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
    for (int k = 0; k < m; ++k) f(ox[k], oy[k], base + k, base + k);
  }
}

// The index: the sorted points k of cells x_lo..x_hi of row yy in ascending k, j = before, before + 1, ... counting along
// the run, only those with FIRST <= j < LAST; -> the run's length.  WAVE = false: the calling thread visits every point.
// WAVE = true: the 64 lanes of a wave call this with the same arguments and split the points, the first going to lane 0.
// Cells are formed only through CellIndex::cell and read only through row_range, here.
template <bool WAVE, int FIRST = 0, int LAST = 0x7fffffff, class F>
__device__ __forceinline__ int for_row_points(const PointCloud& cloud, int yy, int x_lo, int x_hi, F&& f, int before = 0) {
  int k0, k1;
  cloud.index.row_range(yy, x_lo, x_hi, &k0, &k1);
  const int from = FIRST > 0 ? min(max(FIRST - before, 0), k1 - k0) : 0;
  const int to = LAST < 0x7fffffff ? min(max(LAST - before, 0), k1 - k0) : k1 - k0;
  for (int k = k0 + from + (WAVE ? (int)(threadIdx.x & 63) : 0); k < k0 + to; k += WAVE ? 64 : 1)
    f(cloud.points[2 * (long long)k], cloud.points[2 * (long long)k + 1], k, before + (k - k0));
  return k1 - k0;
}

// ... and the points of a window, row after row: j is the point's ordinal among the window's; -> their number.  The loop
// runs over at most cells_y rows of the index.
template <bool WAVE, int FIRST = 0, int LAST = 0x7fffffff, class F>
__device__ __forceinline__ int for_window_points(const PointCloud& cloud, const CellWindow& w, F&& f) {
  int total = 0;
  for (int yy = w.y_lo; yy <= w.y_hi; ++yy) total += for_row_points<WAVE, FIRST, LAST>(cloud, yy, w.x_lo, w.x_hi, f, total);
  return total;
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

struct Scene { PointCloud cloud; Robot robot; };   // what an entry judges its poses against: in every argument struct

enum SceneLookup {      // how an entry finds the points of a pose, as far as its arguments are concerned
  SCENE_ALL_PAIRS,      // no index: the six index arguments are not looked at
  SCENE_CELLS,          // an index of at most MAX_INDEX_CELLS cells; without points nothing reads it and cell_start may be null
  SCENE_CELLS_ALWAYS,   // the same, read even without points (the ring counts of csrc/clearance.hip)
  SCENE_CHECKER_CELLS,  // the *_cells checkers: at least one point, any number of cells (they search 3 x 3 cells, no rings)
};

// The part of every entry's prologue that is about the scene, in the order the requirements have always fired in; then
// *scene is filled (box4 null: the disc of `radius`) and *all_pairs says which kernel to launch -- the all-pairs one also
// where an indexed entry has no points, so that nothing reads an index over nothing.  What only some entries ask (a cell no
// smaller than the reach, a box at all) and what is about their own arrays (counts, null pointers) stays with them.
static inline int fill_scene(Scene* scene, bool* all_pairs, SceneLookup lookup, const float* obstacles_dev,
                             int32_t n_obstacles, const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y,
                             float cell_x0, float cell_y0, float cell_size, const float* box4, float radius,
                             int32_t pose_dim) {
  NFOPP_REQUIRE(!box4 || pose_dim == 3, "the box robot needs poses with a heading (pose_dim 3)");
  if (lookup == SCENE_CHECKER_CELLS) NFOPP_REQUIRE(n_obstacles > 0 && obstacles_dev, "bad obstacle index");
  else NFOPP_REQUIRE(n_obstacles >= 0 && (n_obstacles == 0 || obstacles_dev), "bad obstacle array");
  if (lookup != SCENE_ALL_PAIRS) {
    const int rc = fill_cell_index(&scene->cloud.index, cell_start_dev, cells_x, cells_y, cell_x0, cell_y0, cell_size,
                                   n_obstacles > 0 || lookup == SCENE_CELLS_ALWAYS);
    if (rc) return rc;
    NFOPP_REQUIRE(lookup == SCENE_CHECKER_CELLS || (long long)cells_x * cells_y <= MAX_INDEX_CELLS,
                  "the index holds between 1 and 65536 cells");
  }
  scene->cloud.points = obstacles_dev; scene->cloud.n = n_obstacles;
  if (box4) set_box(&scene->robot, box4);
  else scene->robot.radius = radius;
  *all_pairs = lookup == SCENE_ALL_PAIRS || (n_obstacles == 0 && lookup != SCENE_CELLS_ALWAYS);
  return NFOPP_OK;
}

}  // namespace nfopp
