// The axis rule of the distance-image taps (csrc/sdf_field.hip, csrc/heading_field.hip; include/nfopp_hip.h: nfopp_sdf_field).
#pragma once

namespace nfopp {

// u -> (cell, fraction, strictly inside) on an axis of `count` cell centres.  NaN-safe: the two selects send a NaN to 0,
// so the cell is in [0, count - 2] for every input.
__device__ __forceinline__ void sdf_axis(float u, int count, int& cell, float& frac, bool& inside) {
  const float last = (float)(count - 1);
  inside = u > 0.0f && u < last;
  float c = u > 0.0f ? u : 0.0f;
  c = c < last ? c : last;
  int i = (int)floorf(c);
  cell = i < count - 2 ? i : count - 2;
  frac = c - (float)cell;
}

}  // namespace nfopp
