// Quadratic interpolating spline with midpoint knots (scipy interp1d(kind="quadratic") = make_interp_spline(k=2)):
// the device functions shared by the follower's path post-processing (path_post.hip) and the grid-search seeder
// (grid_search.hip).  Knots t[0..m+2] (ends tripled), D coefficients per knot interval; everything float64.
#pragma once
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

}  // namespace nfopp
