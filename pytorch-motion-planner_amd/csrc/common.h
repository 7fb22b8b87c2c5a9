// Shared host/device helpers of libnfopp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <mutex>

#include "nfopp_hip.h"

namespace nfopp {

// ---- error plumbing (host) -------------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define NFOPP_REQUIRE(cond, ...)          \
  do {                                    \
    if (!(cond)) {                        \
      ::nfopp::set_error(__VA_ARGS__);    \
      return NFOPP_ERR_ARG;               \
    }                                     \
  } while (0)

#define NFOPP_HIP(call)                                          \
  do {                                                           \
    hipError_t e__ = (call);                                     \
    if (e__ != hipSuccess) return ::nfopp::hip_fail(e__, #call); \
  } while (0)

// ---- per-device launch state (host) ------------------------------------------------------------------------------
// One process may drive several GPUs: the dynamic-LDS attribute of a kernel and the CU count belong to the CURRENT
// device's copy of the code object, so "already set" flags are kept per device (csrc/runtime.hip).
constexpr int MAX_DEVICES = 64;
int current_device();   // hipGetDevice, -1 on failure (error string set)
int query_cus();        // CU count of the current device (cached), 256 if it cannot be queried
// Samples from which the 32x32 ONF kernels launch 512 threads per workgroup (nfopp_onf_wide_launch_threshold): CUs x 256.
inline long long onf_wide_launch_threshold() { return (long long)query_cus() * 256; }
// Raises the dynamic-LDS limit of `kernel` on the current device the first time it is launched there.
// `flags` is the caller's static bool[MAX_DEVICES] for that kernel instantiation.
int ensure_dynamic_lds(const void* kernel, size_t bytes, bool* flags);
// Content version the caller registered for a parameter buffer on the current device (nfopp_onf_params_version), 0 = none.
unsigned long long onf_params_version_of(const float* params_dev);
void onf_params_invalidate(const float* params_dev);

// Persistent launch of KERNEL: one workgroup of `threads` per CU, fewer when there are only `n_chunks` pieces of work,
// with `lds` bytes of dynamic LDS; *grid_out (if given) receives the workgroup count.
template <auto KERNEL, class... Args>
int launch_persistent(size_t lds, int threads, long long n_chunks, hipStream_t stream, int* grid_out, const Args&... args) {
  static bool attr_set[MAX_DEVICES] = {};
  const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(KERNEL), lds, attr_set);
  if (rc != NFOPP_OK) return rc;
  long long grid = query_cus();
  if (grid > n_chunks) grid = n_chunks;
  if (grid_out) *grid_out = (int)grid;
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(threads), lds, stream, args...);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

// Launch of KERNEL(args) on `grid` workgroups of `threads` with `lds` bytes of dynamic LDS that follow the problem size
// (trajectory length, candidate count): the 160 KiB a gfx950 workgroup can hold (`what` opens the message of a request
// beyond it), the attribute that lifts HIP's 64 KiB default, the launch and its status.  The attribute is set in front of
// every launch above 64 KiB with that launch's own size.  ensure_dynamic_lds (above) sets it once per device instead and
// stays with launch_persistent and the grid search: their kernels have ONE LDS size each, so a flag is enough there and
// saves the call; here a flag would pin the first -- possibly smaller -- size.
template <class Args>
int launch_dynamic_lds(void (*kernel)(Args), long long grid, int threads, size_t lds, void* stream, const Args& args,
                       const char* what) {
  NFOPP_REQUIRE(lds <= 160 * 1024, "%s for one workgroup's LDS (%zu bytes)", what, lds);
  if (lds > 64 * 1024)
    NFOPP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, (hipStream_t)stream, args);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

// kernel(args) with one thread per item: ceil(n / THREADS) workgroups of THREADS, no launch for n == 0; -> the launch's status
template <int THREADS, class Args>
int launch_per_item(void (*kernel)(Args), long long n, void* stream, const Args& args) {
  if (n == 0) return NFOPP_OK;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, args);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

// A scratch device buffer per (device, stream), for kernels that rewrite their scratch on the launch stream in front of
// every launch: launches of one stream are ordered by the stream itself, and two streams (two planners with different
// fields) never share a buffer.  16 buffers per device -- a handful of streams is the realistic case, though PyTorch's
// pool alone hands out 32 per priority -- and once all are taken the least recently used one is reused after one
// hipDeviceSynchronize (its stream may still be running on it).  Buffers grow on demand.  `Tag` is what the caller
// records about a buffer's content (csrc/onf_x32.hip: what its weight image was built from); it is kept under the pool's
// lock and reset to Tag{} whenever the buffer changes stream or is reallocated.
struct NoTag {};
template <class Tag = NoTag>
class StreamScratch {
 public:
  // *buf = a buffer of at least `bytes` for `stream` on the current device, *tag = its record, *slot = its handle
  int acquire(size_t bytes, hipStream_t stream, void** buf, Tag* tag = nullptr, int* slot = nullptr) {
    const int dev = current_device();
    if (dev < 0) return NFOPP_ERR_HIP;
    std::lock_guard<std::mutex> lock(mutex_);
    Slot* const row = slots_ + dev * SLOTS;
    Slot* s = nullptr;
    for (int k = 0; k < SLOTS && !s; ++k)
      if (row[k].used && row[k].stream == stream) s = &row[k];
    for (int k = 0; k < SLOTS && !s; ++k)
      if (!row[k].used) { s = &row[k]; s->used = true; }
    if (!s) {
      s = &row[0];
      for (int k = 1; k < SLOTS; ++k)
        if (row[k].stamp < s->stamp) s = &row[k];
      NFOPP_HIP(hipDeviceSynchronize());
    }
    if (s->stream != stream) s->tag = Tag{};
    s->stream = stream;
    s->stamp = ++stamp_;
    if (s->bytes < bytes) {
      if (s->ptr) NFOPP_HIP(hipFree(s->ptr));
      s->ptr = nullptr; s->bytes = 0; s->tag = Tag{};
      NFOPP_HIP(hipMalloc(&s->ptr, bytes));
      s->bytes = bytes;
    }
    *buf = s->ptr;
    if (tag) *tag = s->tag;
    if (slot) *slot = (int)(s - slots_);
    return NFOPP_OK;
  }
  // records what the buffer of `slot` now holds, unless another stream has taken it over meanwhile
  void set_tag(int slot, hipStream_t stream, const Tag& tag) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (slots_[slot].stream == stream) slots_[slot].tag = tag;
  }

 private:
  static constexpr int SLOTS = 16;
  struct Slot { hipStream_t stream; void* ptr; size_t bytes; bool used; unsigned long long stamp; Tag tag; };
  Slot slots_[MAX_DEVICES * SLOTS] = {};
  unsigned long long stamp_ = 0;
  std::mutex mutex_;
};

// ---- ONF parameter buffer geometry (state_dict order, include/nfopp_hip.h) --------------------------------------
struct OnfGeom {
  int n_enc, n_sin, ang_dim, n_ang, fin, point_dim;
  int off_ang_b, off_ang_f, off_w1, off_b1, off_w2, off_b2, off_w3, off_b3, off_we, off_be;  // -1 = absent
  int n_params;
  float mean, sigma;
};

inline bool make_geom(const nfopp_onf_config* c, OnfGeom* g) {
  if (!c) return false;
  if (c->angle_dim < 0 || c->angle_dim > 16 || !(c->sigma != 0.0f)) return false;
  g->n_enc = c->use_cos ? 200 : 100;
  g->n_sin = 100;
  g->ang_dim = c->angle_dim;
  g->n_ang = 2 * c->angle_dim;
  g->fin = g->n_enc + g->n_ang;
  g->point_dim = c->angle_dim > 0 ? 3 : 2;
  g->mean = c->mean;
  g->sigma = c->sigma;
  int o = 0;
  g->off_ang_b = g->off_ang_f = -1;
  if (g->n_ang) {
    g->off_ang_b = o; o += g->n_ang;
    g->off_ang_f = o; o += g->n_ang;
  }
  g->off_w1 = o; o += NFOPP_HIDDEN * g->fin;
  g->off_b1 = o; o += NFOPP_HIDDEN;
  g->off_w2 = o; o += NFOPP_HIDDEN * NFOPP_HIDDEN;
  g->off_b2 = o; o += NFOPP_HIDDEN;
  g->off_w3 = o; o += NFOPP_HIDDEN + g->fin;
  g->off_b3 = o; o += 1;
  g->off_we = o; o += 2 * g->n_enc;
  g->off_be = -1;
  if (c->has_bias) { g->off_be = o; o += g->n_enc; }
  g->n_params = o;
  return true;
}

// ---- device math shared by the kernels ---------------------------------------------------------------------------
#define NFOPP_PI_F 3.14159274101257324f      /* fp32(pi)   */
#define NFOPP_PI_D 3.14159265358979323846    /* float64 pi (path post-processing) */
#define NFOPP_TWO_PI_F 6.28318548202514648f  /* fp32(2 pi) */

// nfop/torch_math.py:5-7: (a + pi) % (2 pi) - pi, remainder with the divisor's sign, all in fp32.
// r = x - floor(x / 2pi) * 2pi through one fma: the true remainder is exactly representable, so the fma returns the
// same correctly rounded value torch's fmod-then-adjust produces; the two fix-ups only fire when x / 2pi rounds
// across an integer (remainder within 1 ulp of 0 or 2 pi).
__device__ __forceinline__ float wrap_angle(float a) {
  const float x = a + NFOPP_PI_F;
  const float k = floorf(x * 0.159154943f);
  float r = fmaf(-k, NFOPP_TWO_PI_F, x);
  if (r < 0.0f) r += NFOPP_TWO_PI_F;
  if (r >= NFOPP_TWO_PI_F) r -= NFOPP_TWO_PI_F;
  return r - NFOPP_PI_F;
}

// Entry k = f * D + d of the polyline  start | traj | goal  of batch row b: component d of vertex f, where vertex 0 is the
// start, 1 .. N the waypoints and N + 1 the goal (start, goal [B, D]; traj [B, N, D]).  fp32 as stored: the caller widens.
template <int D>
__device__ __forceinline__ float path_entry(const float* traj, const float* start, const float* goal, int N, long long b,
                                            int k) {
  if (k < D) return start[b * D + k];
  if (k >= (N + 1) * D) return goal[b * D + (k - (N + 1) * D)];
  return traj[b * N * D + (k - D)];
}

// a + b * c and p * a + q * b with every product and sum rounded on its own, as a chain of separate torch ops is on the
// CPU (hipcc would contract the plain expressions to fused multiply-adds)
// (HIP's __fmul_rn / __fadd_rn are plain * and + and contract like them: the pragma is what holds)
__device__ __forceinline__ float add_mul_unfused(float a, float b, float c) {
#pragma clang fp contract(off)
  const float p = b * c;
  return a + p;
}
__device__ __forceinline__ float mix_unfused(float p, float a, float q, float b) {
#pragma clang fp contract(off)
  const float pa = p * a;
  const float qb = q * b;
  return pa + qb;
}

// The collision sample between two consecutive interior waypoints qa = traj[:-1][j] and qb = traj[1:][j] at the draw tt:
// what every collision model (the ONF kernels, csrc/sdf_field.hip) is evaluated at.
// Every product and sum rounded on its own, as the reference's separate torch ops do (no fused multiply-add): the
// sample is then bit-identical to the oracle's for the same t, and K1 sees the reference's inputs.
struct SamplePose { float x, y, ang; };   // ang = 0 without a heading
__device__ __forceinline__ SamplePose collision_sample(int dim, const float* qa, const float* qb, float tt) {
  float x, y, ang = 0.0f;
  if (dim == 3) {
    // constrained:79-81  p = traj[1:] + t * wrap-theta(traj[:-1] - traj[1:])
    float dx = qa[0] - qb[0], dy = qa[1] - qb[1], dth = wrap_angle(qa[2] - qb[2]);
    x = add_mul_unfused(qb[0], tt, dx); y = add_mul_unfused(qb[1], tt, dy); ang = add_mul_unfused(qb[2], tt, dth);
  } else {
    // nerf:117  p = traj[1:] * (1 - t) + traj[:-1] * t
    float omt = 1.0f - tt;
    x = mix_unfused(qb[0], omt, qa[0], tt); y = mix_unfused(qb[1], omt, qa[1], tt);
  }
  return SamplePose{x, y, ang};
}

// sin(x + q*pi/2) for q in Z: 3-term Cody-Waite reduction to [-pi/4, pi/4] + minimax polynomials
// (<= 1.5 ulp for |x| < 1e5; checked against float64 in tests/test_host_logic.py through an fp32 emulation).
__device__ __forceinline__ float sin_quadrant(float x, int q) {
  float j = rintf(x * 0.636619772f);
  float r = fmaf(j, -1.57079601e+00f, x);
  r = fmaf(j, -3.13916473e-07f, r);
  r = fmaf(j, -5.39030253e-15f, r);
  int n = (int)j + q;
  float s = r * r;
  float ps = 2.86567956e-6f;
  ps = fmaf(ps, s, -1.98559923e-4f);
  ps = fmaf(ps, s, 8.33338592e-3f);
  ps = fmaf(ps, s, -1.66666672e-1f);
  float sv = fmaf(ps, r * s, r);
  float pc = 2.44677067e-5f;
  pc = fmaf(pc, s, -1.38877297e-3f);
  pc = fmaf(pc, s, 4.16666567e-2f);
  pc = fmaf(pc, s, -5.0e-1f);
  float cv = fmaf(pc, s, 1.0f);
  float res = (n & 1) ? cv : sv;
  return __int_as_float(__float_as_int(res) ^ ((n & 2) << 30));
}

// Packed-math pairs: the feature evaluation of the fused ONF kernels (onf_layout.h: features2) is written on 2-vectors
// so that hipcc emits v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32.
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 splat2(float v) { return f32x2{v, v}; }

// Hardware path: Cody-Waite reduction of x modulo 2 pi (fma with a hi/lo split of 2 pi), then v_sin_f32 on the remainder
// expressed in revolutions plus the offset qq: |r / 2 pi| <= 0.5006, so |f| reaches 0.5006 / 0.7506 / 1.0006 for qq = 0 /
// 0.25 / 0.5 (a sine kind, a cosine kind or the derivative of a sine kind, the derivative of a cosine kind).  5 VALU + 1
// transcendental op instead of 15 VALU.  Absolute error for any |x| < 1e5 (profiles/feature_probe.txt,
// tests/test_gpu_feature_probe.py), per offset 0 / 0.25 / 0.5:
//   the chain alone (an exact sine in v_sin_f32's place)   4.3e-7 / 3.5e-7 / 6.2e-7: the fp32 rounding of f, whose spacing
//                                                          is 6e-8 revolutions = 3.7e-7 rad from |f| = 0.5 on
//   on gfx950, worst over the feature probes               3.2e-7 / 3.3e-7 / 3.6e-7
// v_sin_f32 itself: max |v_sin_f32(f) - sin(2 pi f)| = 1.25e-7 on the 4 M-point grid of tools/micro/vsin_accuracy.hip; the
// probes see up to 1.35e-7 between the device and the chain with an exact sine.
__device__ __forceinline__ float sin_halfturns_hw(float x, float qq) {  // qq = offset in REVOLUTIONS (q/4)
  const float jm = fmaf(x, 0.159154943f, 12582912.0f);  // 1.5*2^23 + x/2pi: the add rounds to the nearest turn
  const float j = jm - 12582912.0f;                      // whole turns, exact
  float r = fmaf(j, -6.28318548202514648f, x);           // x - j * 2pi  in [-pi, pi] (product exact in the fma)
  r = fmaf(j, 1.74845553e-07f, r);
  return __builtin_amdgcn_sinf(fmaf(r, 0.159154943f, qq));  // |revolutions| <= 1.0006 (qq = 0.5)
}

// sin_halfturns2(x, q * NFOPP_Q_UNIT) = sin(x + q*pi/2): the quadrant offset is pre-scaled to revolutions, the unit
// v_sin_f32 works in
#define NFOPP_Q_UNIT 0.25f

__device__ __forceinline__ f32x2 sin_halfturns2(f32x2 x, f32x2 qh) {
  return f32x2{sin_halfturns_hw(x.x, qh.x), sin_halfturns_hw(x.y, qh.y)};
}

// Philox4x32-10, first output word -> uniform [0,1) with 24 random bits (the same u32->float map torch uses).
__device__ __forceinline__ float philox_uniform(unsigned long long seed, unsigned long long ctr_lo,
                                                unsigned long long ctr_hi) {
  unsigned int c0 = (unsigned int)ctr_lo, c1 = (unsigned int)(ctr_lo >> 32);
  unsigned int c2 = (unsigned int)ctr_hi, c3 = (unsigned int)(ctr_hi >> 32);
  unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    unsigned int hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    unsigned int hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * 5.9604644775390625e-08f;  // 2^-24
}

}  // namespace nfopp
