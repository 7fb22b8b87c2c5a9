// Micro-experiment (dev tool): the two tap layouts of the distance-field collision kernel (csrc/sdf_field.hip).
//   plain: the four taps of a bilinear cell gathered from the [rows, cols] image (hipcc pairs them into two 8-byte loads)
//   quad:  one 16-byte load from a derived [rows - 1, cols - 1, 4] image that holds (s00, s01, s10, s11) per cell
// Same arithmetic behind the taps as the product kernel (per disc: cell, fraction, bilinear value and gradient; the disc with
// the largest penetration gives the row), no trigonometry: the disc offsets are added in the world frame, which leaves the
// memory behaviour as it is.  The samples are those of a planner batch: 4096 straight trajectories of 255 samples between
// random end points, so that the lanes of a wave walk along a line about half a cell apart, as collision samples do.
// Prints microseconds per launch for both layouts, 1 and 3 discs, a 100 x 100 and a 384 x 384 image, alternating the layouts
// round by round, and whether the two layouts gave the same bits.
// Build: hipcc --offload-arch=gfx950 -O3 tools/micro/sdf_taps.hip -o tools/micro/sdf_taps
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

struct Robot { int n; float disc[3][3]; };

template <bool QUAD>
__global__ __launch_bounds__(256) void taps(const float* sd, const float4* quad, int rows, int cols, float inv_res, Robot rb,
                                            const float2* pose, long long n, float4* out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float2 q = pose[p];
  float pen = 0.f, gx = 0.f, gy = 0.f;
  for (int k = 0; k < rb.n; ++k) {
    const float u = (q.x + rb.disc[k][0]) * inv_res - 0.5f, v = (q.y + rb.disc[k][1]) * inv_res - 0.5f;
    const float lu = (float)(cols - 1), lv = (float)(rows - 1);
    const bool in_x = u > 0.f && u < lu, in_y = v > 0.f && v < lv;
    float cu = u > 0.f ? u : 0.f, cv = v > 0.f ? v : 0.f;
    cu = cu < lu ? cu : lu; cv = cv < lv ? cv : lv;
    const int i = min((int)floorf(cu), cols - 2), j = min((int)floorf(cv), rows - 2);
    const float fu = cu - (float)i, fv = cv - (float)j;
    float s00, s01, s10, s11;
    if (QUAD) {
      const float4 c = quad[(long long)j * (cols - 1) + i];
      s00 = c.x; s01 = c.y; s10 = c.z; s11 = c.w;
    } else {
      const float* r0 = sd + (long long)j * cols + i;
      s00 = r0[0]; s01 = r0[1]; s10 = r0[cols]; s11 = r0[cols + 1];
    }
    const float a = s01 - s00, b = s11 - s10, top = s00 + fu * a, bot = s10 + fu * b;
    const float pk = rb.disc[k][2] - (top + fv * (bot - top));
    if (k == 0 || pk > pen) {
      pen = pk;
      gx = in_x ? (a + fv * (b - a)) * inv_res : 0.f;
      gy = in_y ? (bot - top) * inv_res : 0.f;
    }
  }
  out[p] = make_float4(pen, -gx, -gy, 0.f);
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main() {
  const int B = 4096, S = 255;
  const long long n = (long long)B * S;
  srand(11);
  auto uni = [] { return (float)rand() / (float)RAND_MAX; };
  const Robot robots[2] = {{1, {{0.f, 0.f, 0.5f}}}, {3, {{-0.5f, 0.f, 0.6f}, {0.5f, 0.1f, 0.6f}, {1.5f, -0.1f, 0.6f}}}};
  float2* d_pose; float4 *d_out[2];
  CK(hipMalloc(&d_pose, n * sizeof(float2)));
  for (auto& o : d_out) CK(hipMalloc(&o, n * sizeof(float4)));
  for (int side : {100, 384}) {
    const int rows = side, cols = side;
    const float extent = 100.f, inv_res = side / extent;
    // an image with structure: distance to a few random discs, in metres
    std::vector<float> sd((size_t)rows * cols);
    float cxs[40], cys[40];
    for (int k = 0; k < 40; ++k) { cxs[k] = extent * uni(); cys[k] = extent * uni(); }
    for (int j = 0; j < rows; ++j)
      for (int i = 0; i < cols; ++i) {
        float best = 1e9f;
        for (int k = 0; k < 40; ++k) best = std::min(best, hypotf((i + 0.5f) / inv_res - cxs[k], (j + 0.5f) / inv_res - cys[k]) - 3.f);
        sd[(size_t)j * cols + i] = best;
      }
    std::vector<float4> quad((size_t)(rows - 1) * (cols - 1));
    for (int j = 0; j < rows - 1; ++j)
      for (int i = 0; i < cols - 1; ++i)
        quad[(size_t)j * (cols - 1) + i] = make_float4(sd[(size_t)j * cols + i], sd[(size_t)j * cols + i + 1], sd[(size_t)(j + 1) * cols + i],
                                                       sd[(size_t)(j + 1) * cols + i + 1]);
    std::vector<float2> pose(n);
    for (int b = 0; b < B; ++b) {
      const float x0 = extent * uni(), y0 = extent * uni(), x1 = extent * uni(), y1 = extent * uni();
      for (int s = 0; s < S; ++s) {
        const float t = (s + uni()) / S;
        pose[(size_t)b * S + s] = make_float2(x0 + t * (x1 - x0), y0 + t * (y1 - y0));
      }
    }
    float* d_sd; float4* d_quad;
    CK(hipMalloc(&d_sd, sd.size() * 4)); CK(hipMalloc(&d_quad, quad.size() * 16));
    CK(hipMemcpy(d_sd, sd.data(), sd.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_quad, quad.data(), quad.size() * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_pose, pose.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    for (const Robot& rb : robots) {
      const dim3 grid((unsigned)((n + 255) / 256)), block(256);
      auto launch = [&](int layout) {
        if (layout) hipLaunchKernelGGL(taps<true>, grid, block, 0, 0, d_sd, d_quad, rows, cols, inv_res, rb, d_pose, n, d_out[1]);
        else hipLaunchKernelGGL(taps<false>, grid, block, 0, 0, d_sd, d_quad, rows, cols, inv_res, rb, d_pose, n, d_out[0]);
      };
      std::vector<float> us[2];
      hipEvent_t e0, e1;
      CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
      const int rounds = 8, reps = 50;
      for (int r = 0; r < rounds; ++r)
        for (int side2 = 0; side2 < 2; ++side2) {
          const int layout = (r + side2) & 1;          // the order alternates round by round
          for (int w = 0; w < 5; ++w) launch(layout);
          CK(hipEventRecord(e0, 0));
          for (int w = 0; w < reps; ++w) launch(layout);
          CK(hipEventRecord(e1, 0));
          CK(hipEventSynchronize(e1));
          float ms;
          CK(hipEventElapsedTime(&ms, e0, e1));
          us[layout].push_back(ms * 1000.f / reps);
        }
      CK(hipGetLastError());
      std::vector<float4> a(n), b(n);
      CK(hipMemcpy(a.data(), d_out[0], n * 16, hipMemcpyDeviceToHost));
      CK(hipMemcpy(b.data(), d_out[1], n * 16, hipMemcpyDeviceToHost));
      for (auto& v : us) std::sort(v.begin(), v.end());
      printf("image %3d x %3d, %d disc%s: plain %.2f us (min %.2f max %.2f)   quad %.2f us (min %.2f max %.2f)   same bits: %s\n",
             side, side, rb.n, rb.n > 1 ? "s" : " ", us[0][rounds / 2], us[0].front(), us[0].back(), us[1][rounds / 2], us[1].front(),
             us[1].back(), memcmp(a.data(), b.data(), n * 16) == 0 ? "yes" : "NO");
    }
    CK(hipFree(d_sd)); CK(hipFree(d_quad));
  }
  printf("%lld samples per launch: %.1f MB of poses read and rows written\n", n, n * 24 / 1e6);
  return 0;
}
