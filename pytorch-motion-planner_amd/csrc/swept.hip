// Swept collision check between consecutive poses of a path: what `collides` (csrc/path_eval.hip) and the clearance of
// csrc/clearance.hip do not see.  Both judge SAMPLED poses; a robot whose dense poses lie either side of a one-cell wall is
// reported free by both.  Here the unit is the segment (a, b) between two poses -- x and y linear, theta linear along the
// wrapped shortest difference, the motion nfopp_path_interpolate lays its poses on.  Definitions: include/nfopp_hip.h.
//
//   * nfopp_swept_segments        all pairs, obstacle points staged in LDS (for_all_points)
//   * nfopp_swept_segments_cells  the same minimum over the rows of cells that cover the segment (below)
//   * nfopp_path_swept_labels     one workgroup per path: segment values -> the labels nfopp_path_select_best reads
//   * nfopp_swept_refine[_cells]  box robot: the certificate on dyadic pieces, the rectangle label at their midpoints
//   * nfopp_path_refined_labels   the path reduction over the refined segments' free / hit / undecided
// The per-point terms are the fp32 expressions of csrc/point_cloud.h that the checkers and the nearest-obstacle query
// evaluate.  No atomics; every minimum is the lexicographic minimum of (value, index), which does not depend on the order
// the points are visited in: both entries and any two runs give the same bits.
#include "block_collectives.h"
#include "common.h"
#include "point_cloud.h"

// the arithmetic rule of point_cloud.h holds here too: explicit fmas, one operation per statement
#pragma clang fp contract(off)

namespace nfopp {

constexpr int SW_THREADS = 256;
constexpr float SW_COVER = 1.0f + 3.814697265625e-06f;   // 1 + 2^-18: what the cell coverage allows for rounding (below)
constexpr float SW_MAX_TURN = 25.1327419f;                // 8 pi: the largest |theta_b - theta_a| the box certificate takes

struct Segment {
  Pose a, b;
  float ex, ey, len2, len;   // e = b - a, |e|^2, |e|
  float delta;               // box: NFOPP_SWEPT delta, the bound on any body point's travel; 0 for the disc
  bool finite;               // both poses finite
  bool in_domain;            // box: delta <= 4 reach and |theta_b - theta_a| <= 8 pi (what `slack` was derived for)
};

struct SweptArgs {
  const float* a; const float* b; long long n; int dim;
  Scene scene;
  float horizon;
  float* value; int* index;
};

template <int MODE>
__device__ __forceinline__ Segment load_segment(const SweptArgs& g, long long p) {
  Segment s;
  s.a = load_pose<MODE>(g.a, g.dim, p);
  s.b = load_pose<MODE>(g.b, g.dim, p);
  s.finite = s.a.finite && s.b.finite;
  s.ex = s.b.x - s.a.x;
  s.ey = s.b.y - s.a.y;
  const float eyey = s.ey * s.ey;
  s.len2 = __builtin_fmaf(s.ex, s.ex, eyey);
  s.len = sqrtf(s.len2);          // disc_distance(ex, ey)
  s.delta = 0.f;
  s.in_domain = true;
  if (MODE == 1) {
    const float turn = g.b[p * g.dim + 2] - g.a[p * g.dim + 2];
    const float dth = fabsf(wrap_angle(turn));
    s.delta = __builtin_fmaf(g.scene.robot.reach, dth, s.len);
    const float limit = 4.f * g.scene.robot.reach;
    s.in_domain = s.delta <= limit && fabsf(turn) <= SW_MAX_TURN;
  }
  return s;
}

// MODE 0: the distance from the obstacle to the segment [a, b].  The end terms are the disc_distance the circle checker
// compares; the perpendicular term enters only where the obstacle projects strictly inside the segment.
// MODE 1: d_a + d_b, the two distances from the obstacle to the closed box at either end (delta is taken off once, at the end:
// one subtraction of a per-segment constant is monotone, so it does not change which point wins).
template <int MODE>
__device__ __forceinline__ float segment_term(const SweptArgs& g, const Segment& s, float ox, float oy) {
  if (MODE == 1) return g.scene.robot.point_distance<1>(s.a, ox, oy) + g.scene.robot.point_distance<1>(s.b, ox, oy);
  const float ax = ox - s.a.x, ay = oy - s.a.y;
  const float bx = ox - s.b.x, by = oy - s.b.y;
  float v = fminf(disc_distance(ax, ay), disc_distance(bx, by));
  const float eyay = s.ey * ay;
  const float t = __builtin_fmaf(s.ex, ax, eyay);
  if (t > 0.f && t < s.len2) {     // never for a zero-length segment: t == len2 == 0
    const float eyax = s.ey * ax;
    const float cross = __builtin_fmaf(s.ex, ay, -eyax);
    v = fminf(v, fabsf(cross) / s.len);
  }
  return v;
}

// One rule for both entries, so that they write the same bytes: a non-finite segment and an empty cloud give +inf / -1, a
// box segment outside the certificate's domain -inf / -1, a value above the horizon +inf / -1.
template <int MODE>
__device__ __forceinline__ void store_segment(const SweptArgs& g, long long p, const Segment& s, float best, int bestk) {
  float v = best;
  int k = bestk;
  if (MODE == 1 && bestk >= 0) v = best - s.delta;
  if (!s.finite || g.scene.cloud.n == 0) { v = __builtin_inff(); k = -1; }
  else if (!s.in_domain) { v = -__builtin_inff(); k = -1; }
  else if (!(v <= g.horizon)) { v = __builtin_inff(); k = -1; }
  g.value[p] = v;
  if (g.index) g.index[p] = k;
}

// what both entries do with a point: the smallest term of segment s so far, the smallest index among equals
template <int MODE>
struct SegmentMin {
  const SweptArgs& g; const Segment& s; float best; int bestk;
  __device__ __forceinline__ void operator()(float px, float py, int k, int) {
    take_min(segment_term<MODE>(g, s, px, py), k, &best, &bestk);
  }
};

// ---- all pairs ------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(SW_THREADS) void swept_kernel(const SweptArgs g) {
  __shared__ float ox[SW_THREADS], oy[SW_THREADS];
  const long long p = blockIdx.x * (long long)SW_THREADS + threadIdx.x;
  const bool valid = p < g.n;
  Segment s = {};
  if (valid) s = load_segment<MODE>(g, p);
  SegmentMin<MODE> least = {g, s, __builtin_inff(), -1};
  for_all_points<SW_THREADS>(g.scene.cloud, ox, oy, least);
  if (valid) store_segment<MODE>(g, p, s, least.best, least.bestk);
}

// ---- cell index: which cells a segment has to look at --------------------------------------------------------------------
// The indexed entry must write what the all-pairs entry writes.  That one takes the minimum over every point and then
// discards it when it exceeds the horizon, so it is enough to visit every point k whose COMPUTED value is <= horizon: the
// winner and everything tied with it are among them, and if there is none both entries write +inf / -1.
//  (1) Disc.  The computed value of a point is min(da, db, perp).  Each of the three is a lower bound, up to rounding, on
//      a true distance from the point to a point of the segment: da and db within 3 * 2^-24 relative (test_gpu_clearance's
//      count), perp = |cross| / |e| within 12 * 2^-24 (|o - a| + |e|) of the true distance to the line (cross: four
//      roundings of products of two rounded differences, |e|: three; the count is in tests/test_gpu_swept.py).  So a
//      point with computed value <= h lies within h + 12 * 2^-24 (2 h + 2 |e|) of the segment, hence inside the bounding
//      box of a and b inflated by  R = h + 2^-18 (h + |e|)   (2^-18 = 64 * 2^-24).
//  (2) Box.  value <= h means fl(fl(da + db) - delta) <= h with db >= 0, so da <= (delta + h)(1 + 2 * 2^-24).  The box lies in
//      the disc of radius `reach` about the robot's origin and the fp32 distance is below the exact one by less than
//      15 * 2^-24 |o - a| (csrc/clearance.hip, (3)), so |o - a| (1 - 15 * 2^-24) <= reach + (delta + h)(1 + 2 * 2^-24): the point
//      lies within  R = (reach + delta + h)(1 + 2^-18)  of a's origin, a fortiori inside the bounding box of a and b
//      inflated by R (the same holds about b; one rectangle serves both shapes).
//  (3) From coordinates to cells: CellIndex::window_of_box of csrc/point_cloud.h, where the rectangle is formed and the
//      argument stands -- bounds moved outward, monotone cell numbers, one further cell per side.
template <int MODE>
__device__ __forceinline__ float cover_radius(const SweptArgs& g, const Segment& s) {
  if (MODE == 0) return __builtin_fmaf(3.814697265625e-06f, g.horizon + s.len, g.horizon);
  const float reach_delta = g.scene.robot.reach + s.delta;
  const float r = reach_delta + g.horizon;
  return r * SW_COVER;
}

template <int MODE>
__device__ __forceinline__ CellWindow cover_window(const SweptArgs& g, const Segment& s) {
  return g.scene.cloud.index.window_of_box(s.a.x, s.a.y, s.b.x, s.b.y, cover_radius<MODE>(g, s));
}

template <int MODE>
__global__ __launch_bounds__(SW_THREADS) void swept_cells_kernel(const SweptArgs g) {
  const long long p = blockIdx.x * (long long)SW_THREADS + threadIdx.x;
  if (p >= g.n) return;
  const Segment s = load_segment<MODE>(g, p);
  SegmentMin<MODE> least = {g, s, __builtin_inff(), -1};
  if (s.finite && s.in_domain) for_window_points<false>(g.scene.cloud, cover_window<MODE>(g, s), least);
  store_segment<MODE>(g, p, s, least.best, least.bestk);
}

// ---- path reduction -------------------------------------------------------------------------------------------------
struct SweptLabelArgs {
  const float* poses;   // [B, m, D]
  const float* value;   // [B, m - 1]
  float* labels;        // [B * m] in / out
  int m, dim, box;
  float threshold;      // radius (disc) or slack (box)
  unsigned char* status; float* worst;
};

constexpr int SL_THREADS = 256;
constexpr int SL_WAVES = SL_THREADS / 64;

// what a path's threads reduce: the smallest (value, segment) under take_min's order, and the OR of their flags
struct WorstSegment { Indexed<float> seg; int flags; };
__device__ __forceinline__ WorstSegment lane_xor(WorstSegment a, int o) { return {lane_xor(a.seg, o), lane_xor(a.flags, o)}; }
struct WorstOp {
  __device__ __forceinline__ WorstSegment operator()(WorstSegment a, WorstSegment b) const {
    return {TakeMin()(a.seg, b.seg), a.flags | b.flags};
  }
};

__global__ __launch_bounds__(SL_THREADS) void path_swept_labels_kernel(const SweptLabelArgs g) {
  __shared__ WorstSegment red[SL_WAVES];
  const long long b = blockIdx.x;
  const int m = g.m, D = g.dim;
  const float* poses = g.poses + b * m * D;
  const float* value = g.value + b * (m - 1);
  float* labels = g.labels + b * m;
  const int used = g.box ? 3 : 2;   // the components the segment kernels' `finite` looks at
  const WorstSegment none = {{__builtin_inff(), 0x7fffffff}, 0};
  WorstSegment mine = none;   // flags bit 0: a pose in collision, bit 1: a segment not certified
  for (int j = threadIdx.x; j < m; j += SL_THREADS) {
    if (labels[j] != 0.0f) mine.flags |= 1;
    if (j == m - 1) break;            // the last pose keeps its label
    const float v = value[j];
    bool finite = true;
    for (int d = 0; d < used; ++d) finite = finite && isfinite(poses[j * D + d]) && isfinite(poses[(j + 1) * D + d]);
    const bool certified = finite && (g.box ? v > g.threshold : v >= g.threshold);
    if (!certified) { mine.flags |= 2; labels[j] = 1.0f; }
    take_min(v, j, &mine.seg.v, &mine.seg.i);
  }
  const WorstSegment all = block_reduce<SL_WAVES>(mine, none, WorstOp(), red);
  if (threadIdx.x == 0) {
    // a disc segment that is not certified IS a collision; a box segment is only undecided
    if (g.status) g.status[b] = (all.flags & 1) || (!g.box && (all.flags & 2)) ? 1 : ((all.flags & 2) ? 2 : 0);
    if (g.worst) { g.worst[2 * b] = all.seg.v; g.worst[2 * b + 1] = (float)all.seg.i; }
  }
}

// ---- box robot: undecided segments resolved by bisection ---------------------------------------------------------------
// nfopp_swept_refine[_cells] (definition: include/nfopp_hip.h).  The certificate above is applied to dyadic pieces of the
// segment and the rectangle checker's label to their midpoints, in pre-order, until every piece is certified (FREE), a
// midpoint has an obstacle point strictly inside the box (HIT) or the depth / evaluation limits are reached (UNDECIDED).
// A piece (p, q) goes through load_segment<1>, segment_term<1> and the comparison of store_segment<1>; a midpoint through
// load_pose<1> and Robot::hits<1>: the sub-poses are laid into three floats each and read as any other pose array.
//
//   pass 1  refine_root_kernel / refine_root_cells_kernel: one thread per segment.  Steps 1 and 2 of the definition and
//           the root piece, in one visit of the points.  Final for every segment decided there; the others get PENDING.
//   pass 2  refine_walk_kernel: one wavefront (a workgroup of 64) per PENDING segment.  The segment's candidate points are
//           staged in LDS once (those beyond RF_STAGE are read from global memory in the same loop, none is dropped); for
//           every piece and every midpoint the 64 lanes split the points and reduce with an xor tree, so the tree walk is
//           wave-uniform.  Wave w owns the segments p = w (mod waves) and finds the PENDING ones by reading their `status`
//           64 at a time: no list, no atomics, only the owner writes a segment, and consecutive segments of a path -- hard
//           together, where they pass the same obstacle -- are walked by different waves.
// Only comparisons leave the reductions (a minimum against slack + delta, an OR), and minimum and OR do not depend on the
// order of the points: both entries and any two runs write the same bytes.
//
// Which points the indexed entry gathers, ONCE per segment: the rectangle of (2) above with the root's delta and
// horizon = slack, i.e. the bounding box of a and b inflated by (reach + delta_root + slack)(1 + 2^-18), bounds moved outward,
// one further cell per side.
//   Only comparisons matter: a point that cannot turn `cert > slack` false or a `hits` true may be left out.
//   A piece's cert <= slack needs a point with d_p <= delta_piece + slack, so within reach + delta_piece + slack of the
//     sub-pose p, and delta_piece <= delta_root (a piece of depth d >= 1 has half the root's or less; pieces outside the
//     certificate's domain are refused whatever the points are).
//   A midpoint `hits` needs a point inside the box, so within reach of that sub-pose.
//   Every sub-pose lies in the bounding box of a and b (its fmas can leave it by an ulp of a coordinate: the 2^-18 and the
//     further cell hold far more).
// For a segment outside the certificate's domain delta_root is still the fp32 delta of load_segment.
constexpr int RF_STAGE = 1024;                // candidate points a wave keeps in LDS (8 KiB); the 5 x 5 cells of DESIGN 14's
                                              // workload hold about a hundred
constexpr unsigned char RF_FREE = 0, RF_HIT = 1, RF_UNDECIDED = 2, RF_PENDING = 3;

struct RefineArgs {
  SweptArgs seg;            // a, b, n, dim = 3, cloud, robot, horizon = slack; value / index unused
  int max_depth, budget;
  unsigned char* status; float* s; unsigned char* depth;
};

// the comparison store_segment<1> leaves to its reader: the written value is > slack.  `best` = +inf without a point.
__device__ __forceinline__ bool piece_certified(const SweptArgs& g, const Segment& s, float best) {
  if (!s.finite) return false;              // not reached below: sub-poses of finite ends are finite (|coordinates| < 2^60)
  if (g.scene.cloud.n == 0) return true;
  if (!s.in_domain) return false;
  const float v = best - s.delta;
  return v > g.horizon;
}

__device__ __forceinline__ void store_root(const RefineArgs& g, long long p, const Segment& s, bool hit_a, bool hit_b, float best) {
  unsigned char st;
  float at = -1.f;
  if (!s.finite) st = RF_UNDECIDED;
  else if (hit_a) { st = RF_HIT; at = 0.f; }
  else if (hit_b) { st = RF_HIT; at = 1.f; }
  else if (piece_certified(g.seg, s, best)) st = RF_FREE;
  else st = (g.max_depth == 0 || g.budget == 1) ? RF_UNDECIDED : RF_PENDING;
  g.status[p] = st;
  if (g.s) g.s[p] = at;
  if (g.depth) g.depth[p] = 0;
}

// what both root kernels do with a point: steps 1 and 2 of the definition and the root piece's minimum
struct RootTerms {
  const SweptArgs& g; const Segment& s; float best; bool hit_a, hit_b;
  __device__ __forceinline__ void operator()(float px, float py, int, int) {
    best = fminf(best, segment_term<1>(g, s, px, py));
    hit_a |= g.scene.robot.hits<1>(s.a, px, py);
    hit_b |= g.scene.robot.hits<1>(s.b, px, py);
  }
};

__global__ __launch_bounds__(SW_THREADS) void refine_root_kernel(const RefineArgs g) {
  __shared__ float ox[SW_THREADS], oy[SW_THREADS];
  const long long p = blockIdx.x * (long long)SW_THREADS + threadIdx.x;
  const bool valid = p < g.seg.n;
  Segment s = {};
  if (valid) s = load_segment<1>(g.seg, p);
  RootTerms root = {g.seg, s, __builtin_inff(), false, false};
  for_all_points<SW_THREADS>(g.seg.scene.cloud, ox, oy, root);
  if (valid) store_root(g, p, s, root.hit_a, root.hit_b, root.best);
}

__global__ __launch_bounds__(SW_THREADS) void refine_root_cells_kernel(const RefineArgs g) {
  const long long p = blockIdx.x * (long long)SW_THREADS + threadIdx.x;
  if (p >= g.seg.n) return;
  const Segment s = load_segment<1>(g.seg, p);
  RootTerms root = {g.seg, s, __builtin_inff(), false, false};
  if (s.finite) for_window_points<false>(g.seg.scene.cloud, cover_window<1>(g.seg, s), root);
  store_root(g, p, s, root.hit_a, root.hit_b, root.best);
}

// The candidate points of one segment as a wave sees them.  CELLS: candidate j is the jth point for_window_points comes to
// in the segment's window; else it is point j of the cloud.  Candidates j < RF_STAGE are kept in LDS, the others are read
// from global memory at every visit.
struct Candidates {
  const float* lx; const float* ly;   // the first min(total, RF_STAGE) of them
  int total;
  CellWindow window;      // CELLS
};

// f(ox, oy) for each candidate, the 64 lanes taking them in turn
template <bool CELLS, class F>
__device__ __forceinline__ void for_candidates(const PointCloud& cloud, const Candidates& c, int lane, F&& f) {
  for (int k = lane; k < min(c.total, RF_STAGE); k += 64) f(c.lx[k], c.ly[k]);
  if (c.total <= RF_STAGE) return;
  const float* pt = cloud.points;
  if (CELLS) for_window_points<true, RF_STAGE>(cloud, c.window, [&](float px, float py, int, int) { f(px, py); });
  else for (int k = RF_STAGE + lane; k < c.total; k += 64) f(pt[2 * (long long)k], pt[2 * (long long)k + 1]);
}

// sub-pose i * 2^-d of the motion from a to b, as three floats: the ends as loaded, the others by one fma per component
__device__ __forceinline__ void sub_pose(const float* a3, const float* b3, float ex, float ey, float dth, unsigned i, int d,
                                         float* out3) {
  if (i == 0) { out3[0] = a3[0]; out3[1] = a3[1]; out3[2] = a3[2]; return; }
  if (i == (1u << d)) { out3[0] = b3[0]; out3[1] = b3[1]; out3[2] = b3[2]; return; }
  const float s = (float)i * __int_as_float((127 - d) << 23);   // i * 2^-d, exact
  out3[0] = __builtin_fmaf(s, ex, a3[0]);
  out3[1] = __builtin_fmaf(s, ey, a3[1]);
  out3[2] = __builtin_fmaf(s, dth, a3[2]);
}

template <bool CELLS>
__global__ __launch_bounds__(64) void refine_walk_kernel(const RefineArgs g) {
  __shared__ float lx[RF_STAGE], ly[RF_STAGE];
  const int lane = threadIdx.x;
  const long long waves = gridDim.x;
  const PointCloud& cloud = g.seg.scene.cloud;
  // wave w owns the segments p = w (mod waves): neighbours along a path, which tend to be hard together, go to different waves
  for (long long base = blockIdx.x; base < g.seg.n; base += 64 * waves) {
    const long long mine = base + lane * waves;
    unsigned long long pending = __ballot(mine < g.seg.n && g.status[mine] == RF_PENDING);
    while (pending) {
      const long long p = base + (__ffsll((long long)pending) - 1) * waves;
      pending &= pending - 1;
      float a3[3], b3[3];
      for (int k = 0; k < 3; ++k) { a3[k] = g.seg.a[p * 3 + k]; b3[k] = g.seg.b[p * 3 + k]; }
      const Segment root = load_segment<1>(g.seg, p);
      const float dth = wrap_angle(b3[2] - a3[2]);
      Candidates c = {lx, ly, cloud.n, {}};
      if (CELLS) c.window = cover_window<1>(g.seg, root);
      const auto keep = [&](float px, float py, int, int j) { lx[j] = px; ly[j] = py; };
      __syncthreads();                 // the previous segment's reads of lx, ly are done (one wave: a wait, no stall)
      if (CELLS) c.total = for_window_points<true, 0, RF_STAGE>(cloud, c.window, keep);
      else for (int k = lane; k < min(c.total, RF_STAGE); k += 64) keep(cloud.points[2 * k], cloud.points[2 * k + 1], k, k);
      __syncthreads();
      // the pre-order walk; the root piece was evaluated, and found wanting, in pass 1
      int d = 0, deepest = 0, evals = 1;
      unsigned i = 0;
      bool undecided = false, hit = false, root_node = true;
      float at = -1.f;
      for (;;) {
        bool certified = false;
        if (!root_node) {
          if (evals == g.budget) { undecided = true; break; }
          ++evals;
          deepest = max(deepest, d);
          float pa[3], pb[3];
          sub_pose(a3, b3, root.ex, root.ey, dth, i, d, pa);
          sub_pose(a3, b3, root.ex, root.ey, dth, i + 1, d, pb);
          SweptArgs h = g.seg;
          h.a = pa; h.b = pb;
          const Segment piece = load_segment<1>(h, 0);
          float best = __builtin_inff();
          for_candidates<CELLS>(cloud, c, lane, [&](float px, float py) {
            best = fminf(best, segment_term<1>(g.seg, piece, px, py));
          });
          best = wave_reduce(best, [](float x, float y) { return fminf(x, y); });
          certified = piece_certified(g.seg, piece, best);
        }
        root_node = false;
        if (!certified) {
          if (d == g.max_depth) undecided = true;
          else {
            if (evals == g.budget) { undecided = true; break; }
            ++evals;
            float pm[3];
            sub_pose(a3, b3, root.ex, root.ey, dth, 2 * i + 1, d + 1, pm);
            const Pose mid = load_pose<1>(pm, 3, 0);
            bool inside = false;
            for_candidates<CELLS>(cloud, c, lane, [&](float px, float py) { inside |= g.seg.scene.robot.hits<1>(mid, px, py); });
            if (__ballot(inside)) {
              hit = true;
              at = (float)(2 * i + 1) * __int_as_float((127 - (d + 1)) << 23);
              break;
            }
            ++d;
            i <<= 1;
            continue;
          }
        }
        while (i & 1) { i >>= 1; --d; }   // (d, i) is finished: up while it was a right child, then its right sibling
        if (d == 0) break;
        ++i;
      }
      if (lane == 0) {
        g.status[p] = hit ? RF_HIT : (undecided ? RF_UNDECIDED : RF_FREE);
        if (g.s) g.s[p] = at;
        if (g.depth) g.depth[p] = (unsigned char)deepest;
      }
    }
  }
}

// ---- path reduction over refined segments -----------------------------------------------------------------------------
struct RefinedLabelArgs {
  const unsigned char* seg_status;   // [B, m - 1]
  const float* seg_s;                // [B, m - 1]
  float* labels;                     // [B * m] in / out
  int m;
  unsigned char* status; float* first;
};

// the first segment that is not free, and the OR of the flags
struct FirstSegment { int j, flags; };
__device__ __forceinline__ FirstSegment lane_xor(FirstSegment a, int o) { return {lane_xor(a.j, o), lane_xor(a.flags, o)}; }
struct FirstOp {
  __device__ __forceinline__ FirstSegment operator()(FirstSegment a, FirstSegment b) const {
    return {min(a.j, b.j), a.flags | b.flags};
  }
};

__global__ __launch_bounds__(SL_THREADS) void path_refined_labels_kernel(const RefinedLabelArgs g) {
  __shared__ FirstSegment red[SL_WAVES];
  const long long b = blockIdx.x;
  const int m = g.m;
  const unsigned char* seg = g.seg_status + b * (m - 1);
  float* labels = g.labels + b * m;
  const FirstSegment none = {0x7fffffff, 0};
  FirstSegment mine = none;   // flags bit 0: a pose or a segment in collision, bit 1: a segment undecided
  for (int j = threadIdx.x; j < m; j += SL_THREADS) {
    if (labels[j] != 0.0f) mine.flags |= 1;
    if (j == m - 1) break;            // the last pose keeps its label
    const unsigned char st = seg[j];
    if (st == RF_FREE) continue;
    mine.flags |= st == RF_HIT ? 1 : 2;
    labels[j] = 1.0f;
    mine.j = min(mine.j, j);
  }
  const FirstSegment all = block_reduce<SL_WAVES>(mine, none, FirstOp(), red);
  const int firstj = all.j, flags = all.flags;
  if (threadIdx.x == 0) {
    if (g.status) g.status[b] = (flags & 1) ? 1 : ((flags & 2) ? 2 : 0);
    if (g.first) {
      const bool any = firstj != 0x7fffffff;
      g.first[2 * b] = any ? (float)firstj : -1.f;
      g.first[2 * b + 1] = any ? g.seg_s[b * (m - 1) + firstj] : -1.f;
    }
  }
}

static int swept_refine(bool cells, const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                        const float* obstacles_dev, int32_t n_obstacles, const int32_t* cell_start_dev, int32_t cells_x,
                        int32_t cells_y, float cell_x0, float cell_y0, float cell_size, const float* box4, int32_t max_depth,
                        int32_t node_budget, uint8_t* status_dev, float* s_dev, uint8_t* depth_dev, void* stream) {
  NFOPP_REQUIRE(box4, "the refinement is the box robot's: box4 is required (the disc's swept test is exact)");
  NFOPP_REQUIRE(n >= 0 && pose_dim == 3, "need n >= 0 and poses with a heading (pose_dim 3)");
  NFOPP_REQUIRE(n <= (int64_t)0x7fffffff * SW_THREADS, "too many segments for one call");
  NFOPP_REQUIRE(max_depth >= 0 && max_depth <= 20, "max_depth must be between 0 and 20");
  NFOPP_REQUIRE(node_budget >= 1, "node_budget must be >= 1");
  RefineArgs g = {};
  bool all_pairs;   // also where there is nothing to search: every finite segment is certified at its root
  int rc = fill_scene(&g.seg.scene, &all_pairs, cells ? SCENE_CELLS : SCENE_ALL_PAIRS, obstacles_dev, n_obstacles,
                      cell_start_dev, cells_x, cells_y, cell_x0, cell_y0, cell_size, box4, 0.f, pose_dim);
  if (rc) return rc;
  if (n == 0) return NFOPP_OK;
  NFOPP_REQUIRE(a_dev && b_dev && status_dev, "null device pointer");
  g.seg.a = a_dev; g.seg.b = b_dev; g.seg.n = n; g.seg.dim = 3;
  g.seg.horizon = nfopp_swept_slack(box4);
  g.max_depth = max_depth; g.budget = node_budget;
  g.status = status_dev; g.s = s_dev; g.depth = depth_dev;
  rc = launch_per_item<SW_THREADS>(all_pairs ? refine_root_kernel : refine_root_cells_kernel, n, stream, g);
  if (rc) return rc;
  if (max_depth == 0 || node_budget == 1 || n_obstacles == 0) return NFOPP_OK;   // pass 1 left nothing PENDING
  const long long groups = (n + 63) / 64;
  const long long waves = (long long)query_cus() * 16;
  const unsigned wgrid = (unsigned)(groups < waves ? groups : waves);
  if (all_pairs) hipLaunchKernelGGL(refine_walk_kernel<false>, dim3(wgrid), dim3(64), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(refine_walk_kernel<true>, dim3(wgrid), dim3(64), 0, (hipStream_t)stream, g);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

static int swept(bool cells, const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                 const float* obstacles_dev, int32_t n_obstacles, const int32_t* cell_start_dev, int32_t cells_x,
                 int32_t cells_y, float cell_x0, float cell_y0, float cell_size, const float* box4, float horizon,
                 float* value_dev, int32_t* index_dev, void* stream) {
  NFOPP_REQUIRE(n >= 0 && (pose_dim == 2 || pose_dim == 3), "need n >= 0 and pose_dim 2 or 3");
  NFOPP_REQUIRE(n <= (int64_t)0x7fffffff * SW_THREADS, "too many segments for one call");
  // fill_scene asks this too; here it has always been asked in front of the horizon, and stays there
  NFOPP_REQUIRE(!box4 || pose_dim == 3, "the box robot needs poses with a heading (pose_dim 3)");
  NFOPP_REQUIRE(horizon >= 0.f, "the horizon must be >= 0");   // false for a NaN too
  SweptArgs g = {};
  bool all_pairs;   // also where there is nothing to search: the all-pairs kernel writes +inf / -1
  const int rc = fill_scene(&g.scene, &all_pairs, cells ? SCENE_CELLS : SCENE_ALL_PAIRS, obstacles_dev, n_obstacles,
                            cell_start_dev, cells_x, cells_y, cell_x0, cell_y0, cell_size, box4, 0.f, pose_dim);
  if (rc) return rc;
  if (n == 0) return NFOPP_OK;
  NFOPP_REQUIRE(a_dev && b_dev && value_dev, "null device pointer");
  g.a = a_dev; g.b = b_dev; g.n = n; g.dim = pose_dim; g.horizon = horizon; g.value = value_dev; g.index = index_dev;
  if (box4) return launch_per_item<SW_THREADS>(all_pairs ? swept_kernel<1> : swept_cells_kernel<1>, n, stream, g);
  return launch_per_item<SW_THREADS>(all_pairs ? swept_kernel<0> : swept_cells_kernel<0>, n, stream, g);
}

}  // namespace nfopp

using namespace nfopp;

extern "C" float nfopp_swept_slack(const float* box4) {
  return box4 ? box_reach(box4) * NFOPP_SWEPT_SLACK_REL : 0.f;
}

extern "C" int nfopp_swept_segments(const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                                    const float* obstacles_dev, int32_t n_obstacles, const float* box4, float horizon,
                                    float* value_dev, int32_t* index_dev, void* stream) {
  return swept(false, a_dev, b_dev, n, pose_dim, obstacles_dev, n_obstacles, nullptr, 0, 0, 0.f, 0.f, 0.f, box4, horizon,
               value_dev, index_dev, stream);
}

extern "C" int nfopp_swept_segments_cells(const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                                          const float* obstacles_sorted_dev, int32_t n_obstacles,
                                          const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y, float cell_x0,
                                          float cell_y0, float cell_size, const float* box4, float horizon,
                                          float* value_dev, int32_t* index_dev, void* stream) {
  return swept(true, a_dev, b_dev, n, pose_dim, obstacles_sorted_dev, n_obstacles, cell_start_dev, cells_x, cells_y, cell_x0,
               cell_y0, cell_size, box4, horizon, value_dev, index_dev, stream);
}

extern "C" int nfopp_swept_refine(const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                                  const float* obstacles_dev, int32_t n_obstacles, const float* box4, int32_t max_depth,
                                  int32_t node_budget, uint8_t* status_dev, float* s_dev, uint8_t* depth_dev, void* stream) {
  return swept_refine(false, a_dev, b_dev, n, pose_dim, obstacles_dev, n_obstacles, nullptr, 0, 0, 0.f, 0.f, 0.f, box4,
                      max_depth, node_budget, status_dev, s_dev, depth_dev, stream);
}

extern "C" int nfopp_swept_refine_cells(const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                                        const float* obstacles_sorted_dev, int32_t n_obstacles,
                                        const int32_t* cell_start_dev, int32_t cells_x, int32_t cells_y, float cell_x0,
                                        float cell_y0, float cell_size, const float* box4, int32_t max_depth,
                                        int32_t node_budget, uint8_t* status_dev, float* s_dev, uint8_t* depth_dev,
                                        void* stream) {
  return swept_refine(true, a_dev, b_dev, n, pose_dim, obstacles_sorted_dev, n_obstacles, cell_start_dev, cells_x, cells_y,
                      cell_x0, cell_y0, cell_size, box4, max_depth, node_budget, status_dev, s_dev, depth_dev, stream);
}

extern "C" int nfopp_path_refined_labels(const uint8_t* seg_status_dev, const float* seg_s_dev, float* labels_dev,
                                         int64_t batch, int32_t poses_per_path, uint8_t* status_dev, float* first_dev,
                                         void* stream) {
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL && poses_per_path >= 2, "bad batch / pose count");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(seg_status_dev && labels_dev, "null device pointer");
  NFOPP_REQUIRE(seg_s_dev || !first_dev, "first_dev needs the segments' s");
  RefinedLabelArgs g;
  g.seg_status = seg_status_dev; g.seg_s = seg_s_dev; g.labels = labels_dev; g.m = poses_per_path;
  g.status = status_dev; g.first = first_dev;
  hipLaunchKernelGGL(path_refined_labels_kernel, dim3((unsigned)batch), dim3(SL_THREADS), 0, (hipStream_t)stream, g);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" int nfopp_path_swept_labels(const float* poses_dev, const float* value_dev, float* labels_dev, int64_t batch,
                                       int32_t poses_per_path, int32_t dim, float threshold, int32_t box,
                                       uint8_t* status_dev, float* worst_dev, void* stream) {
  NFOPP_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  NFOPP_REQUIRE(!box || dim == 3, "the box robot needs poses with a heading (dim 3)");
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL && poses_per_path >= 2, "bad batch / pose count");
  NFOPP_REQUIRE(threshold >= 0.f, "the radius / slack must be >= 0");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(poses_dev && value_dev && labels_dev, "null device pointer");
  SweptLabelArgs g;
  g.poses = poses_dev; g.value = value_dev; g.labels = labels_dev; g.m = poses_per_path; g.dim = dim; g.box = box != 0;
  g.threshold = threshold; g.status = status_dev; g.worst = worst_dev;
  hipLaunchKernelGGL(path_swept_labels_kernel, dim3((unsigned)batch), dim3(SL_THREADS), 0, (hipStream_t)stream, g);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}
