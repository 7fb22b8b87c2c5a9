// Nearest-obstacle distance for a set of poses, and per-path statistics for a batch of trajectories: what a user who picks
// among the paths of a batch asks beside `collides` and `length` (csrc/path_eval.hip) -- how far a path stays from the
// obstacles, how sharply it turns, whether it reverses.  The batch axis and these statistics are this library's own (the
// reference plans one path and reports its length); the definitions are stated in include/nfopp_hip.h.
//
//   * nfopp_nearest_obstacle        all pairs, obstacle points staged in LDS (for_all_points, as in check_points_kernel)
//   * nfopp_nearest_obstacle_cells  the same minimum over the checkers' cell index, searched ring by ring (below)
//   * nfopp_path_stats              one workgroup per path, float64, fixed-order reductions
// The per-point distance is the fp32 expression of csrc/point_cloud.h that the ground-truth checkers compare, so the
// query and the checkers cannot disagree about a pose.  No atomics; every minimum is the lexicographic minimum of
// (distance, index), which does not depend on the order the points are visited in: the two entries, the two work
// distributions of the indexed one and any two runs give the same bits.
#include "block_collectives.h"
#include "common.h"
#include "point_cloud.h"

// nfopp_path_stats is compared with numpy bit for bit: every float64 operation rounded on its own.  (The fp32 expressions
// of point_cloud.h hold their fmas explicitly and are unaffected.)
#pragma clang fp contract(off)

namespace nfopp {

constexpr int NR_THREADS = 256;
constexpr int NR_WAVE_POSES = 4;              // poses one wave searches one after the other in the wave form

struct NearArgs {   // a pose that load_pose flags as not finite is answered +inf / -1
  const float* poses; long long n; int dim;
  Scene scene;
  float* dist; int* index;
};

__device__ __forceinline__ void store_result(const NearArgs& a, long long p, bool finite, float best, int bestk) {
  a.dist[p] = finite ? best : __builtin_inff();
  if (a.index) a.index[p] = finite ? bestk : -1;
}

// what every form does with a point: the nearest one to the robot at pose q so far, the smallest index among equals
template <int MODE>
struct Nearest {
  const Robot& robot; const Pose& q; float best; int bestk;
  __device__ __forceinline__ void operator()(float px, float py, int k, int) {
    take_min(robot.point_distance<MODE>(q, px, py), k, &best, &bestk);
  }
};

// ---- all pairs ------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(NR_THREADS) void nearest_kernel(const NearArgs a) {
  __shared__ float ox[NR_THREADS], oy[NR_THREADS];
  const long long p = blockIdx.x * (long long)NR_THREADS + threadIdx.x;
  const bool valid = p < a.n;
  Pose q = {0.f, 0.f, 1.f, 0.f, false};
  if (valid) q = load_pose<MODE>(a.poses, a.dim, p);
  Nearest<MODE> near = {a.scene.robot, q, __builtin_inff(), -1};
  for_all_points<NR_THREADS>(a.scene.cloud, ox, oy, near);
  if (valid) store_result(a, p, q.finite, near.best, near.bestk);
}

// ---- cell index: search in rings, and when it may stop -----------------------------------------------------------------
// Ring r holds the cells at Chebyshev distance exactly r from the pose's cell (cx, cy), clipped to the index; after ring r
// the rectangle [cx - r, cx + r] x [cy - r, cy + r] of cells has been visited.  A side of it that has reached the index's
// border has nothing beyond it: the border cells hold every point that was clamped into them, so that side extends to
// infinity.  The search stops after ring r when all four sides are at the border (at r = max(cells_x, cells_y) - 1 at the
// latest, which bounds the loop whatever the pose holds) or when
//     L(r) = (r - 1/16) * size * (1 - 2^-18) - reach  >  best        (reach: Robot::reach, 0 for the disc).
// Why L(r) is a lower bound on the COMPUTED distance of every unvisited point, say one whose cell column qx exceeds
// cx + r (the other three cases mirror it):
//  (1) Pose and points get their cells from one function, CellIndex::cell: u(v) = fl(fl(v - x0) / size), floor, clamp.
//      qx >= cx + r + 1 >= 1 is clamped, so the point's own u >= cx + r + 1.  Unvisited columns to the right exist only if
//      cx + r < cells_x - 1; then cx was not clamped from above and u(pose) < cx + 1 -- also for a pose left of the
//      region, whose negative floor was clamped to 0.  A pose outside the region needs no case of its own.
//  (2) u(v) = t(v) (1 + e), t(v) = (v - x0) / size exactly, |e| <= 2.1 * 2^-24 (one subtraction, one correctly rounded
//      division).  From (1): t(point) >= (cx + r + 1)(1 - |e|), and t(pose) < (cx + 1)(1 + |e|) or t(pose) <= 0, so
//      t(point) - t(pose) > r - |e| (2 cx + r + 2) >= r - 2.1 * 2^-24 * 2^17 > r - 1/16   (cx + r + 1 < MAX_INDEX_CELLS).
//      Only cell numbers enter, never the pose's own magnitude: the bound holds for a pose 10^6 cells away.
//  (3) The point is therefore more than A = (r - 1/16) * size away along x, exactly.  Disc: dx = fl(ox - x) >= A (1 - 2^-24),
//      and sqrtf(fma(dx, dx, dy * dy)) >= |dx| (1 - 2^-23) as rounding and sqrtf are monotone and dy * dy >= 0.
//      Box: the box lies inside the disc of radius `reach` about the robot's origin, so the exact distance to it is at
//      least |point - pose| - reach >= A - reach; the fp32 evaluation (cosf / sinf within 2 ulp, five roundings for rx, ry,
//      three for the distance) is below the exact one by less than 10 * 2^-24 (|dx| + |dy|) <= 15 * 2^-24 |point - pose|,
//      and a bound of the form |point - pose| (1 - k 2^-24) - reach grows with |point - pose|, so it holds at A.
//      The factor 1 - 2^-18 (64 * 2^-24) covers both cases and the roundings of forming L(r) itself.
//  (4) Ties: a point at exactly the best distance with a smaller index must still be found, hence the strict L(r) > best.
// L(0) < 0: ring 1 is always searched, unless the index is a single cell.
// WAVE = false: the calling thread visits every point.  WAVE = true: the 64 lanes of a wave hold the same pose, split each
// run of points among them (for_row_points) and combine their minima after every ring.  *rings (may be null) <- rings
// searched.  The minimum lives in a functor of this function's own and leaves through the pointers: carried in from the
// kernels, across their `if (q.finite)` and the wave form's loop over poses, it cost that kernel 23 instructions more.
template <int MODE, bool WAVE>
__device__ __forceinline__ void nearest_in_cells(const Scene& scene, const Pose& q, float* best, int* bestk, int* rings) {
  const PointCloud& cloud = scene.cloud;
  Nearest<MODE> near = {scene.robot, q, __builtin_inff(), -1};
  const int nx = cloud.index.cells_x, ny = cloud.index.cells_y;
  int cx, cy;
  cloud.index.cell(q.x, q.y, &cx, &cy);
  int r = 0;
  const int r_end = max(nx, ny);
  for (; r < r_end; ++r) {
    const int x_lo = max(cx - r, 0), x_hi = min(cx + r, nx - 1);
    // the two rows of the ring
    if (cy - r >= 0) for_row_points<WAVE>(cloud, cy - r, x_lo, x_hi, near);
    if (r > 0 && cy + r <= ny - 1) for_row_points<WAVE>(cloud, cy + r, x_lo, x_hi, near);
    // the two columns between them, a cell at a time
    for (int yy = max(cy - r + 1, 0); yy <= min(cy + r - 1, ny - 1); ++yy) {
      if (cx - r >= 0) for_row_points<WAVE>(cloud, yy, cx - r, cx - r, near);
      if (cx + r <= nx - 1) for_row_points<WAVE>(cloud, yy, cx + r, cx + r, near);
    }
    if (WAVE) {
      const Indexed<float> m = wave_reduce(Indexed<float>{near.best, near.bestk}, TakeMin());
      near.best = m.v; near.bestk = m.i;
    }
    const bool closed = cx - r <= 0 && cx + r >= nx - 1 && cy - r <= 0 && cy + r >= ny - 1;
    const float lower = __builtin_fmaf(((float)r - 0.0625f) * cloud.index.size, 1.0f - 3.814697265625e-06f, -scene.robot.reach);
    if (closed || lower > near.best) { ++r; break; }
  }
  *best = near.best;
  *bestk = near.bestk;
  if (rings) *rings = r;
}

template <int MODE>
__global__ __launch_bounds__(NR_THREADS) void nearest_cells_kernel(const NearArgs a) {
  const long long p = blockIdx.x * (long long)NR_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const Pose q = load_pose<MODE>(a.poses, a.dim, p);
  float best = __builtin_inff();
  int bestk = -1;
  if (q.finite) nearest_in_cells<MODE, false>(a.scene, q, &best, &bestk, nullptr);
  store_result(a, p, q.finite, best, bestk);
}

// the other work distribution: a wave searches NR_WAVE_POSES poses one after the other, 64 points at a time
template <int MODE>
__global__ __launch_bounds__(NR_THREADS) void nearest_cells_wave_kernel(const NearArgs a) {
  const long long wave = blockIdx.x * (long long)(NR_THREADS / 64) + (threadIdx.x >> 6);
  for (int j = 0; j < NR_WAVE_POSES; ++j) {
    const long long p = wave * NR_WAVE_POSES + j;
    if (p >= a.n) return;   // the same for every lane of the wave
    const Pose q = load_pose<MODE>(a.poses, a.dim, p);
    float best = __builtin_inff();
    int bestk = -1;
    if (q.finite) nearest_in_cells<MODE, true>(a.scene, q, &best, &bestk, nullptr);
    if ((threadIdx.x & 63) == 0) store_result(a, p, q.finite, best, bestk);
  }
}

// rings each pose's search takes (tools/clearance_timing.py reports their distribution)
template <int MODE>
__global__ __launch_bounds__(NR_THREADS) void nearest_rings_kernel(const NearArgs a) {
  const long long p = blockIdx.x * (long long)NR_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const Pose q = load_pose<MODE>(a.poses, a.dim, p);
  float best;
  int bestk, rings = 0;
  if (q.finite) nearest_in_cells<MODE, false>(a.scene, q, &best, &bestk, &rings);
  a.index[p] = rings;
}

// ---- per-path statistics ------------------------------------------------------------------------------------------------
struct StatsArgs {
  const float* traj; const float* start; const float* goal;
  int n, dim;
  const float* pose_dist; int poses;
  double cos_cusp;
  double* stats;
};

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_HEAD = 64;                   // bytes in front of the sign array: the reductions' scratch
static_assert(PS_WAVES * 8 + PS_WAVES * 4 <= PS_HEAD, "the reductions' scratch fits its head");

// LDS of one path of N waypoints: the head and a sign byte per segment, every byte of it dynamic (a static array would come
// off the 160 KiB without launch_dynamic_lds seeing it, as block_collectives.h notes).  The longest path served is the largest
// N with ps_lds_bytes(N) <= 160 KiB: N = 163775.
inline size_t ps_lds_bytes(long long n) { return (size_t)PS_HEAD + (size_t)((n + 1 + 15) & ~15LL); }

// extremum with the first index attaining it: SIGN = +1 maximum, -1 minimum; index -1 = no candidate
template <int SIGN>
__device__ __forceinline__ bool better(double v, int i, double o, int oi) {
  if (i < 0) return false;
  if (oi < 0) return true;
  return (SIGN > 0 ? v > o : v < o) || (v == o && i < oi);
}
template <int SIGN>
struct Better {
  __device__ __forceinline__ Indexed<double> operator()(Indexed<double> a, Indexed<double> b) const {
    return better<SIGN>(b.v, b.i, a.v, a.i) ? b : a;
  }
};

template <int D>
__global__ __launch_bounds__(PS_THREADS) void path_stats_kernel(const StatsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ps_smem[];
  double* red = reinterpret_cast<double*>(ps_smem);                    // [PS_WAVES]
  int* redi = reinterpret_cast<int*>(ps_smem + PS_WAVES * 8);          // [PS_WAVES]
  signed char* sgn = reinterpret_cast<signed char*>(ps_smem + PS_HEAD);   // [N + 1]: sign of each segment's forward component (dim 3)
  const long long b = blockIdx.x;
  const int N = a.n;
  auto point = [&](int f, int d) { return (double)path_entry<D>(a.traj, a.start, a.goal, N, b, f * D + d); };
  // the collectives of this kernel: sums from 0, extrema from "no candidate" (which loses to every candidate)
  auto block_sum = [&](double v) { return block_reduce<PS_WAVES>(v, 0.0, Plus(), red); };
  const Indexed<double> none = {0.0, -1};
  const IndexedScratch<double> red2 = {red, redi};
  // segments i = 0..N: length, forward sign
  double len = 0.0;
  for (int i = threadIdx.x; i <= N; i += PS_THREADS) {
    const double ex = point(i + 1, 0) - point(i, 0), ey = point(i + 1, 1) - point(i, 1);
    len = len + sqrt(ex * ex + ey * ey);
    if (D == 3) {
      const double th = point(i, 2);
      const double fwd = cos(th) * ex + sin(th) * ey;
      sgn[i] = fwd > 0.0 ? 1 : (fwd < 0.0 ? -1 : 0);
    }
  }
  len = block_sum(len);   // its barriers also publish sgn[]
  // interior vertices i = 1..N between segments i - 1 and i
  double kmax = 0.0;
  int kidx = -1, cusps = 0, reversals = 0;
  for (int i = 1 + threadIdx.x; i <= N; i += PS_THREADS) {
    const double x0 = point(i - 1, 0), y0 = point(i - 1, 1), x1 = point(i, 0), y1 = point(i, 1);
    const double x2 = point(i + 1, 0), y2 = point(i + 1, 1);
    const double ex0 = x1 - x0, ey0 = y1 - y0, ex1 = x2 - x1, ey1 = y2 - y1, cx = x2 - x0, cy = y2 - y0;
    const double n0 = sqrt(ex0 * ex0 + ey0 * ey0), n1 = sqrt(ex1 * ex1 + ey1 * ey1), ch = sqrt(cx * cx + cy * cy);
    if (n0 > 0.0 && n1 > 0.0) {
      if (ch > 0.0) {
        const double k = (2.0 * fabs(ex0 * ey1 - ey0 * ex1)) / ((n0 * n1) * ch);
        if (kidx < 0 || k > kmax) { kmax = k; kidx = i; }
      }
      if (ex0 * ex1 + ey0 * ey1 < a.cos_cusp * (n0 * n1)) ++cusps;
    }
    if (D == 3 && sgn[i] != 0) {   // against the last non-zero sign before it
      int j = i - 1;
      while (j >= 0 && sgn[j] == 0) --j;
      if (j >= 0 && sgn[j] != sgn[i]) ++reversals;
    }
  }
  const Indexed<double> sharpest = block_reduce<PS_WAVES>(Indexed<double>{kmax, kidx}, none, Better<+1>(), red2);
  const double n_cusps = block_sum((double)cusps), n_rev = block_sum((double)reversals);   // integers: exact
  // clearance along the densified path
  double dmin = (double)__builtin_inff(), dmean = (double)__builtin_inff();
  int didx = -1;
  if (a.pose_dist) {
    const float* pd = a.pose_dist + b * a.poses;
    double sum = 0.0, m = 0.0;
    int mi = -1;
    for (int k = threadIdx.x; k < a.poses; k += PS_THREADS) {
      const double v = (double)pd[k];
      sum = sum + v;
      if (mi < 0 || v < m) { m = v; mi = k; }
    }
    const Indexed<double> nearest = block_reduce<PS_WAVES>(Indexed<double>{m, mi}, none, Better<-1>(), red2);
    sum = block_sum(sum);
    dmin = nearest.v; didx = nearest.i; dmean = sum / (double)a.poses;
  }
  if (threadIdx.x == 0) {
    double* o = a.stats + b * NFOPP_NUM_PATH_STATS;
    o[0] = len; o[1] = sharpest.i < 0 ? 0.0 : sharpest.v; o[2] = (double)sharpest.i; o[3] = n_cusps; o[4] = n_rev;
    o[5] = dmin; o[6] = (double)didx; o[7] = dmean;
  }
}

template <int MODE>
static void launch_nearest(const NearArgs& a, void* stream) {   // the wave form: the one launch with a grid of its own
  const long long per_group = (long long)(NR_THREADS / 64) * NR_WAVE_POSES;
  hipLaunchKernelGGL(nearest_cells_wave_kernel<MODE>, dim3((unsigned)((a.n + per_group - 1) / per_group)), dim3(NR_THREADS),
                     0, (hipStream_t)stream, a);
}

template <int MODE>
static int launch_form(const NearArgs& a, int form, void* stream) {
  const auto per_pose = form == 0 ? nearest_kernel<MODE> : (form == 1 ? nearest_cells_kernel<MODE> : nearest_rings_kernel<MODE>);
  if (form != 2) return launch_per_item<NR_THREADS>(per_pose, a.n, stream, a);
  launch_nearest<MODE>(a, stream);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

// form: 0 all pairs, 1 cell index with one thread per pose, 2 cell index with one wave per group of poses, 3 ring counts
static int nearest(int form, const float* poses_dev, int64_t n, int32_t pose_dim, const float* obstacles_dev,
                   int32_t n_obstacles, const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y, float cell_x0,
                   float cell_y0, float cell_size, const float* box4, float* dist_dev, int32_t* index_dev, void* stream) {
  NFOPP_REQUIRE(n >= 0 && (pose_dim == 2 || pose_dim == 3), "need n >= 0 and pose_dim 2 or 3");
  NFOPP_REQUIRE(n <= (int64_t)0x7fffffff * NR_WAVE_POSES, "too many poses for one call");
  NearArgs a = {};
  bool all_pairs;
  const int rc = fill_scene(&a.scene, &all_pairs, form == 0 ? SCENE_ALL_PAIRS : (form == 3 ? SCENE_CELLS_ALWAYS : SCENE_CELLS),
                            obstacles_dev, n_obstacles, cell_start_dev, cells_x, cells_y, cell_x0, cell_y0, cell_size, box4,
                            0.f, pose_dim);
  if (rc) return rc;
  if (n == 0) return NFOPP_OK;
  NFOPP_REQUIRE(poses_dev && dist_dev && (form != 3 || index_dev), "null device pointer");
  a.poses = poses_dev; a.n = n; a.dim = pose_dim; a.dist = dist_dev; a.index = index_dev;
  if (all_pairs) form = 0;   // nothing to search: the all-pairs kernel writes +inf / -1
  return box4 ? launch_form<1>(a, form, stream) : launch_form<0>(a, form, stream);
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_nearest_obstacle(const float* poses_dev, int64_t n, int32_t pose_dim, const float* obstacles_dev,
                                      int32_t n_obstacles, const float* box4, float* dist_dev, int32_t* index_dev,
                                      void* stream) {
  return nearest(0, poses_dev, n, pose_dim, obstacles_dev, n_obstacles, nullptr, 0, 0, 0.f, 0.f, 0.f, box4, dist_dev,
                 index_dev, stream);
}

extern "C" int nfopp_nearest_obstacle_cells(const float* poses_dev, int64_t n, int32_t pose_dim,
                                            const float* obstacles_sorted_dev, int32_t n_obstacles,
                                            const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y, float cell_x0,
                                            float cell_y0, float cell_size, const float* box4, float* dist_dev,
                                            int32_t* index_dev, void* stream) {
  return nearest(1, poses_dev, n, pose_dim, obstacles_sorted_dev, n_obstacles, cell_start_dev, cells_x, cells_y, cell_x0,
                 cell_y0, cell_size, box4, dist_dev, index_dev, stream);
}

extern "C" int nfopp_nearest_obstacle_cells_probe(int32_t what, const float* poses_dev, int64_t n, int32_t pose_dim,
                                                  const float* obstacles_sorted_dev, int32_t n_obstacles,
                                                  const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y,
                                                  float cell_x0, float cell_y0, float cell_size, const float* box4,
                                                  float* dist_dev, int32_t* index_dev, void* stream) {
  NFOPP_REQUIRE(what == 0 || what == 1, "what: 0 = the wave form, 1 = ring counts");
  return nearest(what == 0 ? 2 : 3, poses_dev, n, pose_dim, obstacles_sorted_dev, n_obstacles, cell_start_dev, cells_x,
                 cells_y, cell_x0, cell_y0, cell_size, box4, dist_dev, index_dev, stream);
}

extern "C" int nfopp_path_stats(const float* traj_dev, const float* start_dev, const float* goal_dev, int64_t batch,
                                int32_t n_waypoints, int32_t dim, const float* pose_dist_dev, int32_t poses_per_path,
                                double cos_cusp, double* stats_dev, const uint8_t* active_dev, void* stream) {
  (void)active_dev;   // statistics are wanted for retired paths too: every row is written
  NFOPP_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL && n_waypoints >= 1, "bad batch / waypoint count");
  NFOPP_REQUIRE(poses_per_path >= (pose_dist_dev ? 1 : 0), "bad pose count");
  NFOPP_REQUIRE(cos_cusp == cos_cusp, "cos_cusp is not a number");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(traj_dev && start_dev && goal_dev && stats_dev, "null device pointer");
  StatsArgs a;
  a.traj = traj_dev; a.start = start_dev; a.goal = goal_dev; a.n = n_waypoints; a.dim = dim;
  a.pose_dist = pose_dist_dev; a.poses = poses_per_path; a.cos_cusp = cos_cusp; a.stats = stats_dev;
  return launch_dynamic_lds(dim == 3 ? path_stats_kernel<3> : path_stats_kernel<2>, batch, PS_THREADS,
                            ps_lds_bytes(n_waypoints), stream, a, "path too long");
}
