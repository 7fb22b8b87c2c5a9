// Quadratic interpolating spline with midpoint knots (scipy interp1d(kind="quadratic") = make_interp_spline(k=2)):
// the one fit and evaluation of the follower's path post-processing (path_post.hip, 3 columns over the filtered poses) and of
// the grid-search seeder (grid_search.hip, 2 columns over start | cells or points | goal).  Knots t[0..m+2] (ends tripled), D
// coefficients per knot interval; everything behind the fp32 chord lengths is float64.
#pragma once
#include <cstddef>
#include <type_traits>
#include "common.h"

// numpy / scipy evaluate every float64 operation separately: no fused multiply-adds in these functions
#pragma clang fp contract(off)

namespace nfopp {

// the three quadratic B-spline basis values B_{ell-2..ell}(x) on knots t, t[ell] <= x < t[ell+1] (de Boor-Cox)
__device__ __forceinline__ void basis2(const double* t, int ell, double x, double h[3]) {
  h[0] = 1.0; h[1] = 0.0; h[2] = 0.0;
#pragma unroll
  for (int j = 1; j <= 2; ++j) {
    double hh[2] = {h[0], h[1]};
    h[0] = 0.0;
#pragma unroll
    for (int n = 1; n <= j; ++n) {
      const double xb = t[ell + n], xa = t[ell + n - j];
      if (xb == xa) { h[n] = 0.0; continue; }
      const double w = hh[n - 1] / (xb - xa);
      h[n - 1] += w * (xb - x);
      h[n] = w * (x - xa);
    }
  }
}

template <int D>
__device__ __forceinline__ void spline_at(const double* t, const double* c, int m, double x, double p[D]) {
  int lo = 2, hi = m - 1;   // largest ell in [2, m-1] with t[ell] <= x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid] <= x) lo = mid; else hi = mid - 1;
  }
  double h[3];
  basis2(t, lo, x, h);
#pragma unroll
  for (int d = 0; d < D; ++d) p[d] = h[0] * c[(lo - 2) * D + d] + h[1] * c[(lo - 1) * D + d] + h[2] * c[lo * D + d];
}

// Row j (1 <= j <= m-2) of the collocation matrix of m data sites `par` on knots t: with midpoint knots site j lies in
// knot interval j+1 and only coefficients j-1..j+1 are non-zero there, so the system is tridiagonal.
__device__ __forceinline__ void collocation_row(const double* t, const double* par, int m, int j, double h[3]) {
  const int ell = j + 1 > m - 1 ? m - 1 : j + 1;
  basis2(t, ell, par[j], h);
}

// Doubles of the area for at most `cap` sites of D columns: knots cap + 3, coefficients D * cap, parameter, pivots and
// super-diagonal cap each.  What a caller keeps behind it (its fp32 sites) is the caller's to add.
constexpr long long spline_doubles(long long cap, int D) { return (4 + D) * cap + 3; }

struct SplineArea {
  double *T, *C, *PAR, *DD, *UP, *end;   // knots | coefficients (sites in) | parameter | pivots | super-diagonal | what follows
};
template <int D>
__device__ __forceinline__ SplineArea spline_carve(double* base, int cap) {
  double *C = base + (cap + 3), *PAR = C + D * cap;
  return {base, C, PAR, PAR + cap, PAR + 2 * cap, PAR + 3 * cap};
}

// numpy's chord parameter of m >= 2 fp32 sites P[STRIDE * i + {0, 1}] (utils/math.py:58-61, path_postprocessor.py:27-33): fp32
// segment lengths + 1e-6 (kept in dist[0 .. m-2] if `dist` is a float*, not if it is a literal nullptr: told apart by type, as a
// run-time null test of an LDS pointer does not fold), their fp32 running sum, widened and divided by its last value in float64
// -> PAR[0 .. m-1].  Returns whether all sites are distinct: from 1e-6 * 2^24 = 16.8 m of path on a segment can round away in the
// running sum; the collocation matrix is then singular, and scipy refuses the sites.  One lane.
template <int STRIDE, class Dist>
__device__ __forceinline__ bool chord_parameter(const float* P, int m, double* PAR, Dist dist) {
  float acc = 0.f;
  PAR[0] = 0.0;
  for (int i = 0; i < m - 1; ++i) {
    const float dx = P[STRIDE * (i + 1)] - P[STRIDE * i], dy = P[STRIDE * (i + 1) + 1] - P[STRIDE * i + 1];
    const float d = sqrtf((dx * dx) + (dy * dy)) + 1e-6f;
    if constexpr (!std::is_same_v<Dist, std::nullptr_t>) dist[i] = d;
    acc = (acc + d);
    PAR[i + 1] = (double)acc;
  }
  const double last = PAR[m - 1];
  for (int i = 0; i < m; ++i) PAR[i] = PAR[i] / last;
  bool distinct = true;
  for (int i = 1; i < m; ++i)
    if (PAR[i] == PAR[i - 1]) distinct = false;
  return distinct;
}

// The interpolating spline through m >= 3 sites: s.PAR[0 .. m-1] the parameter, s.C[D * i + d] the sites in float64 on entry and
// the coefficients on return, s.T[0 .. m+2] the knots (site midpoints, ends tripled).  The tridiagonal collocation system is
// eliminated without pivoting by the one calling lane (scipy: LAPACK gbsv; agreement to rounding); the previous row stays in
// registers, so the serial chain does not wait for LDS.  s.DD and s.UP are scratch: after the fit they, and s.PAR, are the
// caller's again (the seeder keeps its heading knots in DD and searches PAR).  Two equal sites give a zero pivot: ask
// chord_parameter first.
template <int D>
__device__ __forceinline__ void spline_fit(const SplineArea& s, int m) {
  double *T = s.T, *C = s.C, *DD = s.DD, *UP = s.UP;
  const double* PAR = s.PAR;
  T[0] = T[1] = T[2] = PAR[0];
  for (int i = 1; i <= m - 3; ++i) T[2 + i] = (PAR[i + 1] + PAR[i]) / 2.0;
  T[m] = T[m + 1] = T[m + 2] = PAR[m - 1];
  DD[0] = 1.0; UP[0] = 0.0;
  double dd_prev = 1.0, up_prev = 0.0, c_prev[D];
  for (int d = 0; d < D; ++d) c_prev[d] = C[d];
  for (int j = 1; j < m; ++j) {
    double lowj = 0.0, diagj = 1.0, upj = 0.0;   // the last row is the identity: the end coefficient is the end site
    if (j < m - 1) {
      double h[3];
      collocation_row(T, PAR, m, j, h);
      lowj = h[0]; diagj = h[1]; upj = h[2];
    }
    const double wgt = lowj / dd_prev;
    dd_prev = diagj - wgt * up_prev;
    up_prev = upj;
    DD[j] = dd_prev; UP[j] = upj;
    for (int d = 0; d < D; ++d) { c_prev[d] = C[D * j + d] - wgt * c_prev[d]; C[D * j + d] = c_prev[d]; }
  }
  for (int d = 0; d < D; ++d) { c_prev[d] = c_prev[d] / dd_prev; C[D * (m - 1) + d] = c_prev[d]; }
  for (int j = m - 2; j >= 0; --j)
    for (int d = 0; d < D; ++d) { c_prev[d] = (C[D * j + d] - UP[j] * c_prev[d]) / DD[j]; C[D * j + d] = c_prev[d]; }
}

}  // namespace nfopp
