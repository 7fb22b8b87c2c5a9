// The arithmetic of a pair of timed SE(2) tracks of oriented boxes -- the separation of two boxes at an instant, steps 1 .. 5 on
// a sub-interval, the walk of an interval's dyadic tree, the last-instant term and a track's shape row -- for box_conflict.hip
// and fleet_box_schedule.hip.  This header is its only owner: "a schedule built from box masks is FREE by the box check" holds
// because both kernel files call these functions.  The rule is stated at the top of box_conflict.hip (restated in numpy in
// tests/box_conflict_ref.py; include/nfopp_hip.h repeats it for callers).
// CONTRACTION.  The including files switch contraction off after their includes, so every function here that does float
// arithmetic carries the pragma in its own body, as the functions of track_pairs.h do.
#pragma once
#include <hip/hip_runtime.h>

#include "nfopp_hip.h"
#include "track_pairs.h"

namespace nfopp {

constexpr int BC_SHAPE = 8;       // doubles of a shape row: x0, x1, y0, y1, reach, r, bad, unused
constexpr int BC_MAX_REFINE = NFOPP_BOX_CONFLICT_MAX_REFINE;
constexpr double BC_HALF_PI_UP = 0x1.921fb54442d19p+0;   // the float64 next above pi / 2

struct Pose2 { double x, y, c, s; };

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < (double)__builtin_inff(); }
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }

__device__ __forceinline__ double axis_gap(double t, const double* box, double cx, double cy, double s0, double s1) {
#pragma clang fp contract(off)
  const double a0 = box[0] * cx, a1 = box[1] * cx, b0 = box[2] * cy, b1 = box[3] * cy;
  const double lo = (t + dmin(a0, a1)) + dmin(b0, b1);
  const double hi = (t + dmax(a0, a1)) + dmax(b0, b1);
  return dmax(lo - s1, s0 - hi);
}

__device__ __forceinline__ double box_separation(const Pose2& pi, const Pose2& pj, const double* bi, const double* bj) {
#pragma clang fp contract(off)
  const double dx = pj.x - pi.x, dy = pj.y - pi.y;
  const double cr = pi.c * pj.c + pi.s * pj.s;
  const double sr = pi.c * pj.s - pi.s * pj.c;
  const double xi = dx * pi.c + dy * pi.s;
  const double yi = dy * pi.c - dx * pi.s;
  const double xj = -(dx * pj.c + dy * pj.s);
  const double yj = -(dy * pj.c - dx * pj.s);
  const double g1 = axis_gap(xi, bj, cr, -sr, bi[0], bi[1]);
  const double g2 = axis_gap(yi, bj, sr, cr, bi[2], bi[3]);
  const double g3 = axis_gap(xj, bi, cr, sr, bj[0], bj[1]);
  const double g4 = axis_gap(yj, bi, -sr, cr, bj[2], bj[3]);
  return dmax(dmax(g1, g2), dmax(g3, g4));
}

// |u + v| and |v - u| of two unit vectors
__device__ __forceinline__ double unit_sum_norm(const Pose2& p, const Pose2& q) {
#pragma clang fp contract(off)
  const double sx = p.c + q.c, sy = p.s + q.s;
  return sqrt(sx * sx + sy * sy);
}
__device__ __forceinline__ double unit_chord(const Pose2& p, const Pose2& q) {
#pragma clang fp contract(off)
  const double ex = q.c - p.c, ey = q.s - p.s;
  return sqrt(ex * ex + ey * ey);
}
__device__ __forceinline__ Pose2 mid_pose(const Pose2& p, const Pose2& q, double l) {
#pragma clang fp contract(off)
  Pose2 m;
  m.x = (p.x + q.x) * 0.5; m.y = (p.y + q.y) * 0.5;
  m.c = (p.c + q.c) / l; m.s = (p.s + q.s) / l;
  return m;
}

enum NodeClass { NODE_FREE = 0, NODE_CONFLICT = 1, NODE_SPLIT = 2, NODE_UNDECIDED = 3 };

// steps 1 .. 5 on one sub-interval
__device__ __forceinline__ int classify_node(const Pose2& ia, const Pose2& ja, const Pose2& ib, const Pose2& jb, const double* bi,
                                             const double* bj, double reach_i, double reach_j, double R, double D2, bool may_split) {
#pragma clang fp contract(off)
  const double d0x = ia.x - ja.x, d0y = ia.y - ja.y, d1x = ib.x - jb.x, d1y = ib.y - jb.y;
  const double cc = d0x * d0x + d0y * d0y, e = d1x * d1x + d1y * d1y;
  const Approach q = closest_approach(d0x, d0y, cc, d1x, d1y, e);
  if (q.m >= D2) return NODE_FREE;
  const double sa = box_separation(ia, ja, bi, bj);
  if (sa - R < 0.0) return NODE_CONFLICT;
  const double sb = box_separation(ib, jb, bi, bj);
  const double rot = reach_i * unit_chord(ia, ib) + reach_j * unit_chord(ja, jb);
  const double mot = sqrt(q.a) + BC_HALF_PI_UP * rot;
  if (((sa + sb) - mot) * 0.5 - R >= 0.0) return NODE_FREE;
  if (may_split && unit_sum_norm(ia, ib) != 0.0 && unit_sum_norm(ja, jb) != 0.0) return NODE_SPLIT;
  return NODE_UNDECIDED;
}

// The dyadic tree of one interval with end poses (ia0, ja0) and (ib0, jb0), depth first and left first, without a stack: node
// (depth, pos) is found from the interval's end points in `depth` halvings.  on_node(cls, depth, pos) is called at every node
// that is a CONFLICT or UNDECIDED, in the order of the rule; it returns true to end the walk.
template <class OnNode>
__device__ __forceinline__ void walk_interval(const Pose2& ia0, const Pose2& ja0, const Pose2& ib0, const Pose2& jb0, const double* bi,
                                              const double* bj, double reach_i, double reach_j, double R, double D2, int refine,
                                              OnNode on_node) {
  int depth = 0, pos = 0;
  for (int visit = 0; visit < (2 << BC_MAX_REFINE); ++visit) {
    Pose2 ia = ia0, ja = ja0, ib = ib0, jb = jb0;
    for (int l = depth - 1; l >= 0; --l) {
      const Pose2 mi = mid_pose(ia, ib, unit_sum_norm(ia, ib)), mj = mid_pose(ja, jb, unit_sum_norm(ja, jb));
      if ((pos >> l) & 1) { ia = mi; ja = mj; } else { ib = mi; jb = mj; }
    }
    const int cls = classify_node(ia, ja, ib, jb, bi, bj, reach_i, reach_j, R, D2, depth < refine);
    if (cls == NODE_SPLIT) { ++depth; pos <<= 1; continue; }
    if (cls != NODE_FREE && on_node(cls, depth, pos)) break;
    while (depth > 0 && (pos & 1)) { pos >>= 1; --depth; }
    if (depth == 0) break;
    ++pos;
  }
}

// the term of the last instant: unless the discs are clear of each other, sep - R < 0 is a CONFLICT there
__device__ __forceinline__ bool last_instant_conflict(const Pose2& il, const Pose2& jl, const double* bi, const double* bj, double R,
                                                      double D2) {
#pragma clang fp contract(off)
  const double lx = il.x - jl.x, ly = il.y - jl.y;
  const double cl = lx * lx + ly * ly;
  return !(cl >= D2) && box_separation(il, jl, bi, bj) - R < 0.0;
}

// The shape row of track g, by a workgroup of 64 threads: `row` its k instants, `u` its unit vectors.  -> the BAD flag, in
// thread 0 alone (it wrote the row).
__device__ __forceinline__ int box_shape_row(const float* row, const double* u, const float* box, const float* radius, long long g,
                                             int stride, int k, double* shape) {
#pragma clang fp contract(off)
  int bad = 0;
  for (int n = threadIdx.x; n < k; n += 64) {
    const float x = row[(long long)n * stride], y = row[(long long)n * stride + 1];
    if (!(finite32(x) && finite32(y) && finite64(u[2 * n]) && finite64(u[2 * n + 1]))) bad = 1;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x != 0) return 0;
  const float x0 = box[4 * g], x1 = box[4 * g + 1], y0 = box[4 * g + 2], y1 = box[4 * g + 3];
  const float r = radius ? radius[g] : 0.f;
  if (!(finite32(x0) && finite32(x1) && finite32(y0) && finite32(y1) && finite32(r) && x0 < x1 && y0 < y1 && r >= 0.f)) bad = 1;
  const double mx = (double)fmaxf(fabsf(x0), fabsf(x1)), my = (double)fmaxf(fabsf(y0), fabsf(y1));
  const float corner = (float)sqrt(mx * mx + my * my);
  const float reach = corner * 1.000001f;
  double* o = shape + g * BC_SHAPE;
  o[0] = (double)x0; o[1] = (double)x1; o[2] = (double)y0; o[3] = (double)y1;
  o[4] = (double)reach; o[5] = (double)r; o[6] = bad ? 1.0 : 0.0; o[7] = 0.0;
  return bad;
}

}  // namespace nfopp
