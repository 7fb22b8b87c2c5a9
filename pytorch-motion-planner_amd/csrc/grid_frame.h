// The frame of an occupancy grid on the device: the one cell-centre function of the seeding stage (grid_search.hip), the
// any-angle shortening (grid_any_angle.hip) and the space-time search (spacetime_search.hip).  nfopp/_grid.py (GridFrame) is the
// host side; obstacle_map.hip's cell_point is another frame (rotated origin, float64 out).
#pragma once

#include <hip/hip_runtime.h>

namespace nfopp {

// The fp32 centre, in metres, of the (possibly fractional) column or row u of a grid of resolution `res` that begins at `origin`:
// (u * res + res / 2) + origin in float64 (astar_trajectory_initializer.py:35-37), every operation rounded on its own -- no
// fused multiply-add -- and the sum rounded to fp32 once.  An integer caller widens.  Because all three stages call this, a
// path with nothing to shorten gives the seeding stage's polyline, and a planned track its cells' seeding points, bit for bit.
__host__ __device__ __forceinline__ float grid_cell_centre(double u, double res, double origin) {
#pragma clang fp contract(off)
  const double scaled = u * res;
  const double half = res / 2.0;
  const double mid = scaled + half;
  return (float)(mid + origin);
}

}  // namespace nfopp
