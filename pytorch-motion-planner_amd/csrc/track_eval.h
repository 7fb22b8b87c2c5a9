// The moving-obstacle row of one collision sample (the model is stated at nfopp_track_field in
// include/nfopp_hip.h): shared by csrc/track_field.hip and the layout experiment tools/micro/track_layouts.hip, which differ
// only in where a track position comes from (`Fetch`).
//
// Arithmetic: fp32, every operation rounded on its own; the including file switches contraction off for the whole file in
// front of this header, and the pragma below holds for what is defined here.  The root is sqrtf and the division the
// language's `/`: hipcc rounds both correctly by default, so they equal numpy's on float32.  (__fsqrt_rn is NOT that: hipcc
// 7.2 lowers it to a bare v_sqrt_f32, one ulp off in places -- the first run of tests/test_gpu_track_field.py found it.)
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace nfopp {

struct TrackXY { float x, y; };

// The [M, K, stride] tensor as the caller holds it, x and y first in a row.  m * k * stride fits an int32 (checked on the host).
// PAIR: stride is even and the base 8-byte aligned, so x and y come in one 8-byte load.
template <bool PAIR>
struct TrackGather {
  const float* tracks;
  int k, stride;
  __device__ __forceinline__ TrackXY at(int m, int n) const {
    const float* p = tracks + (m * k + n) * stride;
    if (PAIR) {
      const float2 v = *reinterpret_cast<const float2*>(p);
      return TrackXY{v.x, v.y};
    }
    return TrackXY{p[0], p[1]};
  }
};

// The interval of the track grid a time falls into: positions n and n1 (= n + 1, or n itself when K = 1) and the weight s.
struct TrackTime { int n, n1; float s; };
__device__ __forceinline__ TrackTime track_time(const nfopp_track_field& f, float tau) {
  const float last = (float)(f.k - 1);
  float w = (tau - f.t0) * f.inv_dt;
  w = w > 0.0f ? w : 0.0f;      // a NaN goes to 0
  w = w < last ? w : last;
  const int n = max(min((int)floorf(w), f.k - 2), 0);
  return TrackTime{n, min(n + 1, f.k - 1), w - (float)n};
}

// One finite pose at one finite time -> the track row (logit, dlogit/dx, dlogit/dy, dlogit/dtheta); four NaNs when no
// candidate has a penetration that is a number.  `dim` 2: no heading, dlogit/dtheta = 0.
template <class Fetch>
__device__ __forceinline__ float4 track_eval_pose(const nfopp_track_field& f, const Fetch& fetch, int dim, bool any_offset,
                                                  float x, float y, float th, float tau) {
  const TrackTime tt = track_time(f, tau);
  // robots of centred discs never evaluate a sine, as in csrc/sdf_field.hip
  float c = 1.0f, s = 0.0f;
  if (any_offset) { c = cosf(th); s = sinf(th); }
  float pen = __int_as_float(0x7fc00000), ex = 0.0f, ey = 0.0f, dist = 0.0f, lx = 0.0f, ly = 0.0f;
  for (int d = 0; d < f.n_discs; ++d) {
    const float ox = f.disc[d][0], oy = f.disc[d][1];
    const bool centred = ox == 0.0f && oy == 0.0f;
    const float cx = centred ? x : (x + ox * c) - oy * s;
    const float cy = centred ? y : (y + ox * s) + oy * c;
    for (int m = 0; m < f.m; ++m) {
      const TrackXY a = fetch.at(m, tt.n), b = fetch.at(m, tt.n1);
      const float qx = a.x + tt.s * (b.x - a.x), qy = a.y + tt.s * (b.y - a.y);
      const float dx = cx - qx, dy = cy - qy;
      const float dk = sqrtf(dx * dx + dy * dy);
      const float rho = f.radius_dev ? f.radius_dev[m] : 0.0f;
      const float pk = ((f.disc[d][2] + rho) + f.margin) - dk;
      if (pk > pen || (pen != pen && pk == pk)) {      // the first of the largest; a NaN never wins
        pen = pk; ex = dx; ey = dy; dist = dk;
        lx = (-ox) * s - oy * c;   // d cx / d theta
        ly = ox * c - oy * s;      // d cy / d theta
      }
    }
  }
  const float nx = dist == 0.0f ? 0.0f : ex / dist, ny = dist == 0.0f ? 0.0f : ey / dist;
  const float nnx = -nx, nny = -ny;
  return make_float4(f.gain * pen, f.gain * nnx, f.gain * nny, dim == 2 ? 0.0f : f.gain * (nnx * lx + nny * ly));
}

__device__ __forceinline__ bool track_any_offset(const nfopp_track_field& f) {
  bool any = false;
  for (int d = 0; d < f.n_discs; ++d) any = any || f.disc[d][0] != 0.0f || f.disc[d][1] != 0.0f;
  return any;
}

}  // namespace nfopp
