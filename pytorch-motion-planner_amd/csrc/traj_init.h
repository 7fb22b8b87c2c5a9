// torch.linspace's fp32 rounding and the straight-line initialiser built on it, shared by traj_init.hip and
// grid_search.hip (see traj_init.hip for the reference lines).
#pragma once
#include "common.h"

namespace nfopp {

__device__ __forceinline__ float linspace_at(float s, float e, int steps, int i) {
  if (steps <= 1) return s;
  const float step = (e - s) / (float)(steps - 1);   // IEEE division (hipcc default)
  return i < steps / 2 ? fmaf(step, (float)i, s) : fmaf(-step, (float)(steps - 1 - i), e);
}

// Waypoints i = first, first + stride, ... of ONE straight-line trajectory (trajectory_initializer.py:12-45): the
// body of traj_init_kernel, shared with the grid-search seeder for the problems it cannot seed.
template <int D>
__device__ __forceinline__ void straight_line_fill(const float* s, const float* g, int N, int directed, float* out,
                                                   int first, int stride) {
  const int steps = N + 2;
  float goal_angle = 0.f;
  if (D == 3) goal_angle = wrap_angle(g[2] - s[2]) + s[2];
  for (int i = first; i < N; i += stride) {
    out[i * D + 0] = linspace_at(s[0], g[0], steps, i + 1);
    out[i * D + 1] = linspace_at(s[1], g[1], steps, i + 1);
    if (D == 3) {
      float th = linspace_at(s[2], goal_angle, steps, i + 1);
      if (directed) {
        // central difference over the FULL path (start, waypoints, goal): neighbours i and i+2 of the full index
        const float x0 = i == 0 ? s[0] : linspace_at(s[0], g[0], steps, i);
        const float y0 = i == 0 ? s[1] : linspace_at(s[1], g[1], steps, i);
        const float x1 = i == N - 1 ? g[0] : linspace_at(s[0], g[0], steps, i + 2);
        const float y1 = i == N - 1 ? g[1] : linspace_at(s[1], g[1], steps, i + 2);
        const float heading = atan2f(y1 - y0, x1 - x0);
        const int h = N / 2;
        const float w = i < h ? linspace_at(0.f, 1.f, h, i) : linspace_at(1.f, 0.f, (N + 1) / 2, i - h);
        th = add_mul_unfused(th, wrap_angle(heading - th), w);
      }
      out[i * D + 2] = th;
    }
  }
}

}  // namespace nfopp
