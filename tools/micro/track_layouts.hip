// Micro-experiment (dev tool): where the moving-obstacle kernel (csrc/track_field.hip) takes a track position
// from.  The arithmetic behind the fetch is the product's own (csrc/track_eval.h).
//   plain:  the product's [M, K, stride] tensor, x and y as two 4-byte loads (what an odd stride or base needs)
//   pair:   the same tensor, x and y in one 8-byte load (even stride, 8-byte aligned base: what the product launches then)
//   major:  a derived time-major copy [K, M] of (x, y): the inner loop over the tracks walks two contiguous rows per lane
// The samples are those of a planner batch: 4096 straight trajectories of 255 samples whose times run over the track grid, so
// the lanes of a wave read neighbouring instants.  Prints microseconds per launch for M = 8, 64, 256 at K = 256, alternating
// the forms round by round, and whether all forms gave the same bits.
// Build: hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize -Iinclude -Ipytorch-motion-planner_amd/csrc tools/micro/track_layouts.hip -o tools/micro/track_layouts
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)

#include "track_eval.h"

using namespace nfopp;

struct TrackMajor {
  const float2* xy;   // [K, M]
  int m_count;
  __device__ __forceinline__ TrackXY at(int m, int n) const {
    const float2 v = xy[n * m_count + m];
    return TrackXY{v.x, v.y};
  }
};

// pose = (x, y, theta, tau); out4 in-out as in the product: the row is replaced iff the track row's logit is larger
template <class Fetch>
__global__ __launch_bounds__(256) void overlay(const nfopp_track_field f, const Fetch fetch, const float4* pose, long long n,
                                               float4* out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float4 q = pose[p];
  const float4 base = out[p];
  const float4 r = track_eval_pose(f, fetch, 3, track_any_offset(f), q.x, q.y, q.z, q.w);
  if (r.x > base.x) out[p] = r;
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main() {
  const int B = 4096, S = 255, K = 256, FORMS = 3;
  const long long n = (long long)B * S;
  const float extent = 100.f, dt = 0.25f;
  srand(11);
  auto uni = [] { return (float)rand() / (float)RAND_MAX; };
  std::vector<float4> pose(n);
  for (int b = 0; b < B; ++b) {
    const float x0 = extent * uni(), y0 = extent * uni(), x1 = extent * uni(), y1 = extent * uni();
    const float th0 = 6.28f * uni() - 3.14f, th1 = th0 + 2.f * uni() - 1.f;
    for (int s = 0; s < S; ++s) {
      const float t = (s + uni()) / S;
      pose[(size_t)b * S + s] = make_float4(x0 + t * (x1 - x0), y0 + t * (y1 - y0), th0 + t * (th1 - th0), t * (K - 1) * dt);
    }
  }
  float4* d_pose; float4* d_out[FORMS];
  CK(hipMalloc(&d_pose, n * sizeof(float4)));
  for (auto& o : d_out) CK(hipMalloc(&o, n * sizeof(float4)));
  CK(hipMemcpy(d_pose, pose.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  const std::vector<float4> zero_rows(n, make_float4(0.f, 0.f, 0.f, 0.f));
  for (int discs : {1, 3})
    for (int M : {8, 64, 256}) {
      // constant-velocity tracks across the floor, radius 0.5 m
      std::vector<float> plain((size_t)M * K * 2), major((size_t)K * M * 2), radius(M, 0.5f);
      for (int m = 0; m < M; ++m) {
        const float px = extent * uni(), py = extent * uni(), vx = 2.f * uni() - 1.f, vy = 2.f * uni() - 1.f;
        for (int k = 0; k < K; ++k) {
          const float x = px + vx * k * dt, y = py + vy * k * dt;
          plain[((size_t)m * K + k) * 2] = x; plain[((size_t)m * K + k) * 2 + 1] = y;
          major[((size_t)k * M + m) * 2] = x; major[((size_t)k * M + m) * 2 + 1] = y;
        }
      }
      float *d_plain, *d_major, *d_radius;
      CK(hipMalloc(&d_plain, plain.size() * 4)); CK(hipMalloc(&d_major, major.size() * 4)); CK(hipMalloc(&d_radius, M * 4));
      CK(hipMemcpy(d_plain, plain.data(), plain.size() * 4, hipMemcpyHostToDevice));
      CK(hipMemcpy(d_major, major.data(), major.size() * 4, hipMemcpyHostToDevice));
      CK(hipMemcpy(d_radius, radius.data(), M * 4, hipMemcpyHostToDevice));
      nfopp_track_field f = {};
      f.tracks_dev = d_plain; f.radius_dev = d_radius;
      f.m = M; f.k = K; f.stride = 2;
      f.t0 = 0.f; f.inv_dt = 1.f / dt;
      f.n_discs = discs;
      const float three[3][3] = {{-0.2f, 0.f, 0.15f}, {0.f, 0.f, 0.15f}, {0.25f, 0.05f, 0.15f}};
      for (int d = 0; d < discs; ++d)
        for (int c = 0; c < 3; ++c) f.disc[d][c] = discs == 1 ? (c == 2 ? 0.3f : 0.f) : three[d][c];
      f.margin = 0.5f; f.gain = 10.f;
      for (auto& o : d_out) CK(hipMemcpy(o, zero_rows.data(), n * 16, hipMemcpyHostToDevice));
      const dim3 grid((unsigned)((n + 255) / 256)), block(256);
      auto launch = [&](int form) {
        if (form == 0) hipLaunchKernelGGL(overlay<TrackGather<false>>, grid, block, 0, 0, f, TrackGather<false>{d_plain, K, 2}, d_pose, n, d_out[0]);
        if (form == 1) hipLaunchKernelGGL(overlay<TrackGather<true>>, grid, block, 0, 0, f, TrackGather<true>{d_plain, K, 2}, d_pose, n, d_out[1]);
        if (form == 2) hipLaunchKernelGGL(overlay<TrackMajor>, grid, block, 0, 0, f, TrackMajor{(const float2*)d_major, M}, d_pose, n, d_out[2]);
      };
      std::vector<float> us[FORMS];
      hipEvent_t e0, e1;
      CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
      const int rounds = 7, reps = 20;
      for (int r = 0; r < rounds; ++r)
        for (int turn = 0; turn < FORMS; ++turn) {
          const int form = (r + turn) % FORMS;          // the order rotates round by round
          for (int w = 0; w < 3; ++w) launch(form);
          CK(hipEventRecord(e0, 0));
          for (int w = 0; w < reps; ++w) launch(form);
          CK(hipEventRecord(e1, 0));
          CK(hipEventSynchronize(e1));
          float ms;
          CK(hipEventElapsedTime(&ms, e0, e1));
          us[form].push_back(ms * 1000.f / reps);
        }
      CK(hipGetLastError());
      std::vector<float4> got[FORMS];
      long long replaced = 0;
      for (int k = 0; k < FORMS; ++k) {
        got[k].resize(n);
        CK(hipMemcpy(got[k].data(), d_out[k], n * 16, hipMemcpyDeviceToHost));
      }
      for (long long p = 0; p < n; ++p) replaced += got[0][p].x != 0.f;
      const bool same = memcmp(got[0].data(), got[1].data(), n * 16) == 0 && memcmp(got[0].data(), got[2].data(), n * 16) == 0;
      for (auto& v : us) std::sort(v.begin(), v.end());
      printf("discs %d, M = %3d, K = %d (%6.1f KB of tracks): plain %8.2f us (min %.2f max %.2f)   pair %8.2f us (min %.2f max %.2f)   "
             "major %8.2f us (min %.2f max %.2f)   same bits: %s   rows replaced: %lld of %lld\n",
             discs, M, K, plain.size() * 4 / 1e3, us[0][rounds / 2], us[0].front(), us[0].back(), us[1][rounds / 2], us[1].front(),
             us[1].back(), us[2][rounds / 2], us[2].front(), us[2].back(), same ? "yes" : "NO", replaced, n);
      fflush(stdout);
      CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
      CK(hipFree(d_plain)); CK(hipFree(d_major)); CK(hipFree(d_radius));
    }
  return 0;
}
