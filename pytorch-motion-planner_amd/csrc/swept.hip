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
  PointCloud cloud; Robot robot;
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
    s.delta = __builtin_fmaf(g.robot.reach, dth, s.len);
    const float limit = 4.f * g.robot.reach;
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
  if (MODE == 1) return g.robot.point_distance<1>(s.a, ox, oy) + g.robot.point_distance<1>(s.b, ox, oy);
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
  if (!s.finite || g.cloud.n == 0) { v = __builtin_inff(); k = -1; }
  else if (!s.in_domain) { v = -__builtin_inff(); k = -1; }
  else if (!(v <= g.horizon)) { v = __builtin_inff(); k = -1; }
  g.value[p] = v;
  if (g.index) g.index[p] = k;
}

// ---- all pairs ------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(SW_THREADS) void swept_kernel(const SweptArgs g) {
  __shared__ float ox[SW_THREADS], oy[SW_THREADS];
  const long long p = blockIdx.x * (long long)SW_THREADS + threadIdx.x;
  const bool valid = p < g.n;
  Segment s = {};
  if (valid) s = load_segment<MODE>(g, p);
  float best = __builtin_inff();
  int bestk = -1;
  for_all_points<SW_THREADS>(g.cloud, ox, oy, [&](float px, float py, int k) {
    take_min(segment_term<MODE>(g, s, px, py), k, &best, &bestk);
  });
  if (valid) store_segment<MODE>(g, p, s, best, bestk);
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
//  (3) From coordinates to cells.  Each bound w = min - R or max + R is formed in fp32 and then moved outward by
//      4 * 2^-24 |w|, more than the rounding of its own two operations, so the fp32 bound encloses the exact one.
//      CellIndex::axis_cell is a chain of monotone operations (correctly rounded subtraction and division, floor, clamp),
//      and points and bounds go through that one function: lo <= ox <= hi implies cell(lo) <= cell(ox) <= cell(hi), for a
//      point clamped into a border cell too.  One further cell is visited on each side: it costs a few points per segment
//      and keeps the coverage from resting on the last bit of (1) to (3).
//  Cells are formed only through CellIndex::cell and row_range; the loops run over at most cells_y rows of the index.
template <int MODE>
__device__ __forceinline__ float cover_radius(const SweptArgs& g, const Segment& s) {
  if (MODE == 0) return __builtin_fmaf(3.814697265625e-06f, g.horizon + s.len, g.horizon);
  const float reach_delta = g.robot.reach + s.delta;
  const float r = reach_delta + g.horizon;
  return r * SW_COVER;
}

__device__ __forceinline__ float outward(float w, float sign) {   // w moved by 4 * 2^-24 |w| towards sign * inf
  return __builtin_fmaf(fabsf(w), sign * 2.384185791015625e-07f, w);
}

template <int MODE>
__global__ __launch_bounds__(SW_THREADS) void swept_cells_kernel(const SweptArgs g) {
  const long long p = blockIdx.x * (long long)SW_THREADS + threadIdx.x;
  if (p >= g.n) return;
  const Segment s = load_segment<MODE>(g, p);
  float best = __builtin_inff();
  int bestk = -1;
  if (s.finite && s.in_domain) {
    const float r = cover_radius<MODE>(g, s);
    const float lox = outward(fminf(s.a.x, s.b.x) - r, -1.f), hix = outward(fmaxf(s.a.x, s.b.x) + r, 1.f);
    const float loy = outward(fminf(s.a.y, s.b.y) - r, -1.f), hiy = outward(fmaxf(s.a.y, s.b.y) + r, 1.f);
    int x_lo, y_lo, x_hi, y_hi;
    g.cloud.index.cell(lox, loy, &x_lo, &y_lo);
    g.cloud.index.cell(hix, hiy, &x_hi, &y_hi);
    x_lo = max(x_lo - 1, 0); x_hi = min(x_hi + 1, g.cloud.index.cells_x - 1);
    y_lo = max(y_lo - 1, 0); y_hi = min(y_hi + 1, g.cloud.index.cells_y - 1);
    const float* pt = g.cloud.points;
    for (int yy = y_lo; yy <= y_hi; ++yy) {
      int k, k1;
      g.cloud.index.row_range(yy, x_lo, x_hi, &k, &k1);
      for (; k < k1; ++k)
        take_min(segment_term<MODE>(g, s, pt[2 * (long long)k], pt[2 * (long long)k + 1]), k, &best, &bestk);
    }
  }
  store_segment<MODE>(g, p, s, best, bestk);
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
  if (g.cloud.n == 0) return true;
  if (!s.in_domain) return false;
  const float v = best - s.delta;
  return v > g.horizon;
}

__device__ __forceinline__ void cover_cells(const SweptArgs& g, const Segment& s, int* x_lo, int* y_lo, int* x_hi, int* y_hi) {
  const float r = cover_radius<1>(g, s);
  const float lox = outward(fminf(s.a.x, s.b.x) - r, -1.f), hix = outward(fmaxf(s.a.x, s.b.x) + r, 1.f);
  const float loy = outward(fminf(s.a.y, s.b.y) - r, -1.f), hiy = outward(fmaxf(s.a.y, s.b.y) + r, 1.f);
  g.cloud.index.cell(lox, loy, x_lo, y_lo);
  g.cloud.index.cell(hix, hiy, x_hi, y_hi);
  *x_lo = max(*x_lo - 1, 0); *x_hi = min(*x_hi + 1, g.cloud.index.cells_x - 1);
  *y_lo = max(*y_lo - 1, 0); *y_hi = min(*y_hi + 1, g.cloud.index.cells_y - 1);
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

__global__ __launch_bounds__(SW_THREADS) void refine_root_kernel(const RefineArgs g) {
  __shared__ float ox[SW_THREADS], oy[SW_THREADS];
  const long long p = blockIdx.x * (long long)SW_THREADS + threadIdx.x;
  const bool valid = p < g.seg.n;
  Segment s = {};
  if (valid) s = load_segment<1>(g.seg, p);
  float best = __builtin_inff();
  bool hit_a = false, hit_b = false;
  for_all_points<SW_THREADS>(g.seg.cloud, ox, oy, [&](float px, float py, int) {
    best = fminf(best, segment_term<1>(g.seg, s, px, py));
    hit_a |= g.seg.robot.hits<1>(s.a, px, py);
    hit_b |= g.seg.robot.hits<1>(s.b, px, py);
  });
  if (valid) store_root(g, p, s, hit_a, hit_b, best);
}

__global__ __launch_bounds__(SW_THREADS) void refine_root_cells_kernel(const RefineArgs g) {
  const long long p = blockIdx.x * (long long)SW_THREADS + threadIdx.x;
  if (p >= g.seg.n) return;
  const Segment s = load_segment<1>(g.seg, p);
  float best = __builtin_inff();
  bool hit_a = false, hit_b = false;
  if (s.finite) {
    int x_lo, y_lo, x_hi, y_hi;
    cover_cells(g.seg, s, &x_lo, &y_lo, &x_hi, &y_hi);
    const float* pt = g.seg.cloud.points;
    for (int yy = y_lo; yy <= y_hi; ++yy) {
      int k, k1;
      g.seg.cloud.index.row_range(yy, x_lo, x_hi, &k, &k1);
      for (; k < k1; ++k) {
        const float px = pt[2 * (long long)k], py = pt[2 * (long long)k + 1];
        best = fminf(best, segment_term<1>(g.seg, s, px, py));
        hit_a |= g.seg.robot.hits<1>(s.a, px, py);
        hit_b |= g.seg.robot.hits<1>(s.b, px, py);
      }
    }
  }
  store_root(g, p, s, hit_a, hit_b, best);
}

// the candidate points of one segment as a wave sees them: f(ox, oy) for each, the 64 lanes taking them in turn
struct Candidates {
  const float* lx; const float* ly;   // the first min(total, RF_STAGE) of them, in LDS
  int total;
  int x_lo, y_lo, x_hi, y_hi;         // CELLS: the rows they come from
};

template <bool CELLS, class F>
__device__ __forceinline__ void for_candidates(const PointCloud& cloud, const Candidates& c, int lane, F&& f) {
  const int staged = min(c.total, RF_STAGE);
  for (int k = lane; k < staged; k += 64) f(c.lx[k], c.ly[k]);
  if (c.total <= RF_STAGE) return;
  const float* pt = cloud.points;
  if (!CELLS) {
    for (int k = RF_STAGE + lane; k < c.total; k += 64) f(pt[2 * (long long)k], pt[2 * (long long)k + 1]);
    return;
  }
  int base = 0;                        // candidates in front of this row
  for (int yy = c.y_lo; yy <= c.y_hi; ++yy) {
    int k0, k1;
    cloud.index.row_range(yy, c.x_lo, c.x_hi, &k0, &k1);
    const int skip = min(max(RF_STAGE - base, 0), k1 - k0);   // of this row, already visited in LDS
    for (int k = k0 + skip + lane; k < k1; k += 64) f(pt[2 * (long long)k], pt[2 * (long long)k + 1]);
    base += k1 - k0;
  }
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
  const PointCloud& cloud = g.seg.cloud;
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
      Candidates c = {lx, ly, cloud.n, 0, 0, 0, 0};
      __syncthreads();                 // the previous segment's reads of lx, ly are done (one wave: a wait, no stall)
      if (CELLS) {
        cover_cells(g.seg, root, &c.x_lo, &c.y_lo, &c.x_hi, &c.y_hi);
        c.total = 0;
        for (int yy = c.y_lo; yy <= c.y_hi; ++yy) {
          int k0, k1;
          cloud.index.row_range(yy, c.x_lo, c.x_hi, &k0, &k1);
          for (int k = k0 + lane; k < k1 && c.total + (k - k0) < RF_STAGE; k += 64) {
            lx[c.total + (k - k0)] = cloud.points[2 * (long long)k];
            ly[c.total + (k - k0)] = cloud.points[2 * (long long)k + 1];
          }
          c.total += k1 - k0;
        }
      } else {
        for (int k = lane; k < min(c.total, RF_STAGE); k += 64) {
          lx[k] = cloud.points[2 * (long long)k];
          ly[k] = cloud.points[2 * (long long)k + 1];
        }
      }
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
            for_candidates<CELLS>(cloud, c, lane, [&](float px, float py) { inside |= g.seg.robot.hits<1>(mid, px, py); });
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
  NFOPP_REQUIRE(n_obstacles >= 0 && (n_obstacles == 0 || obstacles_dev), "bad obstacle array");
  RefineArgs g = {};
  if (cells) {
    const int rc = fill_cell_index(&g.seg.cloud.index, cell_start_dev, cells_x, cells_y, cell_x0, cell_y0, cell_size,
                                   n_obstacles > 0);
    if (rc) return rc;
    NFOPP_REQUIRE((long long)cells_x * cells_y <= MAX_INDEX_CELLS, "the index holds between 1 and 65536 cells");
  }
  if (n == 0) return NFOPP_OK;
  NFOPP_REQUIRE(a_dev && b_dev && status_dev, "null device pointer");
  g.seg.a = a_dev; g.seg.b = b_dev; g.seg.n = n; g.seg.dim = 3; g.seg.cloud.points = obstacles_dev; g.seg.cloud.n = n_obstacles;
  set_box(&g.seg.robot, box4);
  g.seg.horizon = nfopp_swept_slack(box4);
  g.max_depth = max_depth; g.budget = node_budget;
  g.status = status_dev; g.s = s_dev; g.depth = depth_dev;
  if (n_obstacles == 0) cells = false;   // nothing to search: every finite segment is certified at its root
  const hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((n + SW_THREADS - 1) / SW_THREADS);
  if (cells) hipLaunchKernelGGL(refine_root_cells_kernel, dim3(grid), dim3(SW_THREADS), 0, st, g);
  else hipLaunchKernelGGL(refine_root_kernel, dim3(grid), dim3(SW_THREADS), 0, st, g);
  NFOPP_HIP(hipGetLastError());
  if (max_depth == 0 || node_budget == 1 || n_obstacles == 0) return NFOPP_OK;   // pass 1 left nothing PENDING
  const long long groups = (n + 63) / 64;
  const long long waves = (long long)query_cus() * 16;
  const unsigned wgrid = (unsigned)(groups < waves ? groups : waves);
  if (cells) hipLaunchKernelGGL(refine_walk_kernel<true>, dim3(wgrid), dim3(64), 0, st, g);
  else hipLaunchKernelGGL(refine_walk_kernel<false>, dim3(wgrid), dim3(64), 0, st, g);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

template <int MODE>
static void launch_swept(const SweptArgs& g, bool cells, hipStream_t st) {
  const unsigned grid = (unsigned)((g.n + SW_THREADS - 1) / SW_THREADS);
  if (cells) hipLaunchKernelGGL(swept_cells_kernel<MODE>, dim3(grid), dim3(SW_THREADS), 0, st, g);
  else hipLaunchKernelGGL(swept_kernel<MODE>, dim3(grid), dim3(SW_THREADS), 0, st, g);
}

static int swept(bool cells, const float* a_dev, const float* b_dev, int64_t n, int32_t pose_dim,
                 const float* obstacles_dev, int32_t n_obstacles, const int32_t* cell_start_dev, int32_t cells_x,
                 int32_t cells_y, float cell_x0, float cell_y0, float cell_size, const float* box4, float horizon,
                 float* value_dev, int32_t* index_dev, void* stream) {
  NFOPP_REQUIRE(n >= 0 && (pose_dim == 2 || pose_dim == 3), "need n >= 0 and pose_dim 2 or 3");
  NFOPP_REQUIRE(n <= (int64_t)0x7fffffff * SW_THREADS, "too many segments for one call");
  NFOPP_REQUIRE(!box4 || pose_dim == 3, "the box robot needs poses with a heading (pose_dim 3)");
  NFOPP_REQUIRE(horizon >= 0.f, "the horizon must be >= 0");   // false for a NaN too
  NFOPP_REQUIRE(n_obstacles >= 0 && (n_obstacles == 0 || obstacles_dev), "bad obstacle array");
  SweptArgs g = {};
  if (cells) {
    const int rc = fill_cell_index(&g.cloud.index, cell_start_dev, cells_x, cells_y, cell_x0, cell_y0, cell_size,
                                   n_obstacles > 0);
    if (rc) return rc;
    NFOPP_REQUIRE((long long)cells_x * cells_y <= MAX_INDEX_CELLS, "the index holds between 1 and 65536 cells");
  }
  if (n == 0) return NFOPP_OK;
  NFOPP_REQUIRE(a_dev && b_dev && value_dev, "null device pointer");
  g.a = a_dev; g.b = b_dev; g.n = n; g.dim = pose_dim; g.cloud.points = obstacles_dev; g.cloud.n = n_obstacles;
  g.horizon = horizon; g.value = value_dev; g.index = index_dev;
  if (box4) set_box(&g.robot, box4);
  if (n_obstacles == 0) cells = false;   // nothing to search: the all-pairs kernel writes +inf / -1
  if (box4) launch_swept<1>(g, cells, (hipStream_t)stream);
  else launch_swept<0>(g, cells, (hipStream_t)stream);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
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
