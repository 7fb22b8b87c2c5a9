// The arithmetic of a pair of timed tracks -- how close two points come that move linearly between the instants of a common
// grid, whether that is a conflict, which tile of pairs a workgroup takes -- for track_conflict.hip and fleet_schedule.hip.
// This header is its only owner: "the schedule is clear by the conflict check" holds because both kernels call these functions.
//
// The rule (restated in numpy in tests/track_conflict_ref.py; include/nfopp_hip.h repeats it for callers).  Everything is
// float64 with every operation rounded on its own.  A track is K >= 1 positions at t_k = t0 + k * dt (k * dt rounded, then
// the sum, as nfopp_path_time_sample forms its instants), read as fp32 and widened; x, y are the first two floats of a row
// of `stride` floats.  Between two instants a track is linear in time.  R_ij = (ra_i + rb_j) + margin, R2_ij = R_ij * R_ij.
//  Pair (i, j), interval k = 0 .. K - 2, componentwise d0 = pa_k - pb_k, d1 = pa_{k+1} - pb_{k+1}, w = d1 - d0:
//    c = d0x * d0x + d0y * d0y,  a = wx * wx + wy * wy,  b = d0x * wx + d0y * wy
//    a == 0 or b >= 0:  s = 0,         m = c
//    else -b >= a:      s = 1,         m = d1x * d1x + d1y * d1y
//    else:              s = (-b) / a,  p = d0 + s * w,  m = px * px + py * py
//  and one more term for the last instant: k = K - 1, s = 0, m = |d_{K-1}|^2 (the whole check when K = 1).
//  M_ij = min_k m_k, attained first at k*;  t*_ij = t_{k*} + s_{k*} * dt;  gap g_ij = sqrt(M_ij) - R_ij.
//  Conflict: some m_k < R2_ij (strict, like the circle checker's dist < radius).  At the smallest such k: s_in = 0 when
//    c < R2, else disc = max(b * b - a * (c - R2), 0), s_in = min(max(((-b) - sqrt(disc)) / a, 0), s);  tc_ij = t_k + s_in * dt
//    (the last-instant term: tc = t_{K-1} + 0 * dt).  No conflict: tc_ij = +inf.
//  A track with a non-finite coordinate or radius is BAD and nobody's partner; its outputs are each kernel's own rule.
// CONTRACTION.  The including files switch contraction off after their includes, so every function here that does float
// arithmetic carries the pragma in its own body, as add_mul_unfused of common.h does.
#pragma once
#include <hip/hip_runtime.h>

namespace nfopp {

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __builtin_inff(); }

// Tile `t` of the upper triangle of n x n tiles, row by row: row r starts at r * n - r * (r - 1) / 2.  The closed form
// gives r up to the rounding of the square root; the two loops correct it.
__device__ __forceinline__ void upper_triangle_tile(long long t, long long n, long long* ta, long long* tb) {
  const long long q = 2 * n + 1;
  long long r = (long long)(((double)q - sqrt((double)(q * q - 8 * t))) * 0.5);
  if (r < 0) r = 0;
  if (r > n - 1) r = n - 1;
  while (r > 0 && r * n - r * (r - 1) / 2 > t) --r;
  while (r + 1 < n && (r + 1) * n - (r + 1) * r / 2 <= t) ++r;
  *ta = r;
  *tb = r + (t - (r * n - r * (r - 1) / 2));
}

// Tile `t` of a rectangle of tiles with ntb columns, row by row: set A against set B
__device__ __forceinline__ void pair_tile(long long t, long long ntb, long long* ta, long long* tb) {
  *ta = t / ntb;
  *tb = t % ntb;
}

// R = (ra + rb) + margin, R2 = R * R
__device__ __forceinline__ void pair_radius(double ra, double rb, double margin, double* R, double* R2) {
#pragma clang fp contract(off)
  *R = (ra + rb) + margin;
  *R2 = *R * *R;
}

// One interval: d0 = (x0, y0) with c = |d0|^2 = cc, d1 = (d1x, d1y) with |d1|^2 = e -> a, b, the fraction s of the closest
// approach and its squared distance m.
struct Approach { double a, b, s, m; };
__device__ __forceinline__ Approach closest_approach(double x0, double y0, double cc, double d1x, double d1y, double e) {
#pragma clang fp contract(off)
  const double wx = d1x - x0, wy = d1y - y0;
  Approach r;
  r.a = wx * wx + wy * wy; r.b = x0 * wx + y0 * wy;
  if (r.a == 0.0 || r.b >= 0.0) { r.s = 0.0; r.m = cc; }
  else if (-r.b >= r.a) { r.s = 1.0; r.m = e; }
  else {
    r.s = (-r.b) / r.a;
    const double px = x0 + r.s * wx, py = y0 + r.s * wy;
    r.m = px * px + py * py;
  }
  return r;
}

// s_in of an interval in conflict (m < R2): the fraction at which the distance first falls to R
__device__ __forceinline__ double entry_fraction(double a, double b, double cc, double R2, double s) {
#pragma clang fp contract(off)
  double s_in = 0.0;
  if (!(cc < R2)) {
    const double bb = b * b, cr = cc - R2, acr = a * cr;
    double disc = bb - acr;
    disc = disc > 0.0 ? disc : 0.0;
    s_in = ((-b) - sqrt(disc)) / a;
    s_in = s_in > 0.0 ? s_in : 0.0;
    s_in = s_in < s ? s_in : s;
  }
  return s_in;
}

}  // namespace nfopp
