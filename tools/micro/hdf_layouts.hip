// Micro-experiment (dev tool): two image layouts of the heading-layered distance field kernel (csrc/heading_field.hip,
// DESIGN.md 26).
//   plain:  the product's [L, rows, cols]: per slice the four taps of a bilinear cell (hipcc pairs the x-neighbours), the two
//           slices rows * cols floats apart
//   inner:  a derived [rows, cols, L + 1] image, layers innermost, with slice 0 copied behind slice L - 1 (the wrap): the two
//           slices of a corner in one 8-byte load, four such loads per sample
// Same arithmetic behind the taps as the product kernel.  The samples are those of a planner batch: 4096 straight
// trajectories of 255 samples between random end points with a heading that turns along the way.  Prints microseconds per
// launch for both layouts at L = 8 and 64 on a 100 x 100 and a 384 x 384 image, alternating the layouts round by round, and
// whether the two layouts gave the same bits.
// Build: hipcc --offload-arch=gfx950 -O3 tools/micro/hdf_layouts.hip -o tools/micro/hdf_layouts
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

struct Tap { float d, gx, gy; };
__device__ __forceinline__ Tap blend(float s00, float s01, float s10, float s11, float fu, float fv, float inv_res) {
  const float a = s01 - s00, b = s11 - s10, top = s00 + fu * a, bot = s10 + fu * b, dv = bot - top;
  return Tap{top + fv * dv, (a + fv * (b - a)) * inv_res, dv * inv_res};
}

// layers 2..64, rows, cols >= 2: i in [0, cols - 2], j in [0, rows - 2], k0, k1 in [0, layers - 1] for every finite pose
template <bool INNER>
__global__ __launch_bounds__(256) void taps(const float* img, int layers, int rows, int cols, float inv_res, float lpr,
                                            const float4* pose, long long n, float4* out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float4 q = pose[p];
  const float w = q.z * lpr, kf = floorf(w), fw = w - kf;
  const int r = (int)fmodf(kf, (float)layers);
  const int k0 = r < 0 ? r + layers : r, k1 = k0 + 1 == layers ? 0 : k0 + 1;
  const float u = q.x * inv_res - 0.5f, v = q.y * inv_res - 0.5f;
  const float lu = (float)(cols - 1), lv = (float)(rows - 1);
  const bool in_x = u > 0.f && u < lu, in_y = v > 0.f && v < lv;
  float cu = u > 0.f ? u : 0.f, cv = v > 0.f ? v : 0.f;
  cu = cu < lu ? cu : lu; cv = cv < lv ? cv : lv;
  const int i = min((int)floorf(cu), cols - 2), j = min((int)floorf(cv), rows - 2);
  const float fu = cu - (float)i, fv = cv - (float)j;
  Tap t0, t1;
  if (INNER) {
    const int stride = layers + 1;                       // slice `layers` is the copy of slice 0, so k0 + 1 never wraps
    const float* c = img + ((long long)j * cols + i) * stride + k0;
    const float s00a = c[0], s00b = c[1], s01a = c[stride], s01b = c[stride + 1];
    const float* c1 = c + (long long)cols * stride;
    const float s10a = c1[0], s10b = c1[1], s11a = c1[stride], s11b = c1[stride + 1];
    t0 = blend(s00a, s01a, s10a, s11a, fu, fv, inv_res);
    t1 = blend(s00b, s01b, s10b, s11b, fu, fv, inv_res);
  } else {
    const long long slice = (long long)rows * cols, cell = (long long)j * cols + i;
    const float* a = img + k0 * slice + cell;
    const float* b = img + k1 * slice + cell;
    t0 = blend(a[0], a[1], a[cols], a[cols + 1], fu, fv, inv_res);
    t1 = blend(b[0], b[1], b[cols], b[cols + 1], fu, fv, inv_res);
  }
  const float dd = t1.d - t0.d;
  const float gx = in_x ? t0.gx + fw * (t1.gx - t0.gx) : 0.f, gy = in_y ? t0.gy + fw * (t1.gy - t0.gy) : 0.f;
  out[p] = make_float4(0.1f - (t0.d + fw * dd), -gx, -gy, -(dd * lpr));
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main() {
  const int B = 4096, S = 255;
  const long long n = (long long)B * S;
  srand(11);
  auto uni = [] { return (float)rand() / (float)RAND_MAX; };
  float4* d_pose; float4* d_out[2];
  CK(hipMalloc(&d_pose, n * sizeof(float4)));
  for (auto& o : d_out) CK(hipMalloc(&o, n * sizeof(float4)));
  const float extent = 100.f;
  std::vector<float4> pose(n);
  for (int b = 0; b < B; ++b) {
    const float x0 = extent * uni(), y0 = extent * uni(), x1 = extent * uni(), y1 = extent * uni();
    const float th0 = 6.28f * uni() - 3.14f, th1 = th0 + 2.f * uni() - 1.f;
    for (int s = 0; s < S; ++s) {
      const float t = (s + uni()) / S;
      pose[(size_t)b * S + s] = make_float4(x0 + t * (x1 - x0), y0 + t * (y1 - y0), th0 + t * (th1 - th0), 0.f);
    }
  }
  CK(hipMemcpy(d_pose, pose.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  for (int side : {100, 384})
    for (int layers : {8, 64}) {
      const int rows = side, cols = side;
      const float inv_res = side / extent, lpr = (float)(layers / (2 * M_PI));
      const size_t cells = (size_t)rows * cols;
      // an image with structure: per slice the distance to a few random discs, in metres
      std::vector<float> plain(cells * layers), inner(cells * (layers + 1));
      for (int k = 0; k < layers; ++k) {
        float cxs[20], cys[20];
        for (int m = 0; m < 20; ++m) { cxs[m] = extent * uni(); cys[m] = extent * uni(); }
        for (int j = 0; j < rows; ++j)
          for (int i = 0; i < cols; ++i) {
            float best = 1e9f;
            for (int m = 0; m < 20; ++m) best = std::min(best, hypotf((i + 0.5f) / inv_res - cxs[m], (j + 0.5f) / inv_res - cys[m]) - 3.f);
            plain[k * cells + (size_t)j * cols + i] = best;
          }
      }
      for (size_t c = 0; c < cells; ++c)
        for (int k = 0; k <= layers; ++k) inner[c * (layers + 1) + k] = plain[(size_t)(k % layers) * cells + c];
      float *d_plain, *d_inner;
      CK(hipMalloc(&d_plain, plain.size() * 4)); CK(hipMalloc(&d_inner, inner.size() * 4));
      CK(hipMemcpy(d_plain, plain.data(), plain.size() * 4, hipMemcpyHostToDevice));
      CK(hipMemcpy(d_inner, inner.data(), inner.size() * 4, hipMemcpyHostToDevice));
      const dim3 grid((unsigned)((n + 255) / 256)), block(256);
      auto launch = [&](int layout) {
        if (layout) hipLaunchKernelGGL(taps<true>, grid, block, 0, 0, d_inner, layers, rows, cols, inv_res, lpr, d_pose, n, d_out[1]);
        else hipLaunchKernelGGL(taps<false>, grid, block, 0, 0, d_plain, layers, rows, cols, inv_res, lpr, d_pose, n, d_out[0]);
      };
      std::vector<float> us[2];
      hipEvent_t e0, e1;
      CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
      const int rounds = 8, reps = 50;
      for (int r = 0; r < rounds; ++r)
        for (int half = 0; half < 2; ++half) {
          const int layout = (r + half) & 1;          // the order alternates round by round
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
      printf("image %3d x %3d, L = %2d (%5.1f MB): plain %.2f us (min %.2f max %.2f)   inner %.2f us (min %.2f max %.2f)   same bits: %s\n",
             side, side, layers, plain.size() * 4 / 1e6, us[0][rounds / 2], us[0].front(), us[0].back(), us[1][rounds / 2],
             us[1].front(), us[1].back(), memcmp(a.data(), b.data(), n * 16) == 0 ? "yes" : "NO");
      CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
      CK(hipFree(d_plain)); CK(hipFree(d_inner));
    }
  printf("%lld samples per launch: %.1f MB of poses read and rows written\n", n, n * 32 / 1e6);
  return 0;
}
