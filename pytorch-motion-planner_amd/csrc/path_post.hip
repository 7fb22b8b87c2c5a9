// Path post-processing for the follower, one workgroup per path.
//
// Replaces PathPostprocessor.process (nfop/ros/path_postprocessor.py:13-69): drop interior poses closer than
// `minimal_distance` to the previously kept one (walking from the goal), re-sample the path every `distance_step`
// metres along a QUADRATIC interpolating spline over the normalised chord-length parameter (scipy
// interp1d(kind="quadratic") = make_interp_spline(k=2): knots at the data-site midpoints, end knots tripled), headings
// unfolded first, and trim the leading poses that are driven in the opposite direction to the first one.
//
// Precision follows numpy on the fp32 path the planner returns: filter, segment lengths, their running sum and the
// unfolded headings in fp32; parametrisation, spline and output in float64.  The parameter and the fit are spline2.h's
// (chord_parameter, spline_fit; agreement with scipy to rounding, checked against its output in tests/golden/g12); this
// file keeps the filter, the pairwise length, the heading unfold and the trim.  The sequential parts (filter, sums,
// elimination: O(n)) run on lane 0; evaluation of the `count` output poses is spread over the workgroup.
#include "common.h"
#include "spline2.h"

// numpy evaluates every fp32 / float64 operation separately: no fused multiply-adds anywhere in this file
// (hipcc's `__fmul_rn` / `__fadd_rn` are plain operators and would still be contracted)
#pragma clang fp contract(off)

namespace nfopp {

constexpr int PP_THREADS = 256;

struct PostArgs {
  const float* path;   // [B, n, 3]
  int n, max_out;
  float min_dist, dist_step;
  double* out;         // [B, max_out, 3]
  int* count;          // [B]: poses the path needs (after trimming); -1 = no spline through the path: fewer than 3 poses
                       // survive the filter, or two of them share a parameter value
};

// numpy's pairwise float summation order (8 partial sums per block of <= 128, halves split at a multiple of 8);
// the recursion is unrolled at compile time: 4 levels cover the 1025 segments of the longest path
template <int LEVELS>
__device__ __forceinline__ float pairwise_sum(const float* a, int n) {
  if (n < 8) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s = s + a[i];
    return s;
  }
  if constexpr (LEVELS > 0) {
    if (n > 128) {
      int n2 = n / 2;
      n2 -= n2 % 8;
      return pairwise_sum<LEVELS - 1>(a, n2) + pairwise_sum<LEVELS - 1>(a + n2, n - n2);
    }
  }
  float r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
  float s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) s = s + a[i];
  return s;
}

// np.remainder(x, 2 pi) for fp32 (result takes the sign of the divisor)
__device__ __forceinline__ float remainder_two_pi(float x) {
  float r = fmodf(x, NFOPP_TWO_PI_F);
  if (r != 0.f && r < 0.f) r = (r + NFOPP_TWO_PI_F);
  return r;
}

__global__ __launch_bounds__(PP_THREADS) void path_post_kernel(const PostArgs a) {
  extern __shared__ double lds[];
  const int n = a.n;
  const SplineArea sp = spline_carve<3>(lds, n);
  const double *T = sp.T, *C = sp.C;             // knots and coefficients, once lane 0 has fitted the spline
  float* P = reinterpret_cast<float*>(sp.end);   // 3n filtered poses
  float* DIST = P + 3 * n;      // n segment lengths
  __shared__ int s_m, s_count, s_first;
  const long long b = blockIdx.x;
  const float* src = a.path + b * (long long)n * 3;
  for (int k = threadIdx.x; k < 3 * n; k += PP_THREADS) P[k] = src[k];
  __syncthreads();

  if (threadIdx.x == 0) {
    // ---- filter (:35-44), in place from the back: kept poses end up in P[w..n-1]
    int w = n - 1;
    float px = P[3 * (n - 1)], py = P[3 * (n - 1) + 1];
    for (int i = n - 2; i >= 1; --i) {
      const float dx = px - P[3 * i], dy = py - P[3 * i + 1];
      const float dist = sqrtf(((dx * dx) + (dy * dy)));
      if (dist > a.min_dist) {
        --w;
        P[3 * w] = P[3 * i]; P[3 * w + 1] = P[3 * i + 1]; P[3 * w + 2] = P[3 * i + 2];
        px = P[3 * i]; py = P[3 * i + 1];
      }
    }
    --w;
    const float x0 = P[0], y0 = P[1], a0 = P[2];
    P[3 * w] = x0; P[3 * w + 1] = y0; P[3 * w + 2] = a0;
    const int m = n - w;
    float* Q = P + 3 * w;
    int count = -1;
    // ---- parametrisation (:27-33).  scipy refuses duplicate sites ("Expect x to not have duplicates"): with minimal_distance
    // below 1e-6 * 2^24 a segment can round away in the fp32 running sum; no spline goes through such a path
    if (m >= 3 && chord_parameter<3>(Q, m, sp.PAR, DIST)) {
      const float total = pairwise_sum<4>(DIST, m - 1);   // total length (:21-25)
      count = (int)(total / a.dist_step);
      // ---- unfold headings (utils/math.py:38-43)
      float prev = remainder_two_pi(Q[2] + NFOPP_PI_F) - NFOPP_PI_F;
      const float first_angle = prev;
      float run = 0.f;
      Q[2] = (float)((double)first_angle);
      for (int i = 1; i < m; ++i) {
        const float cur = remainder_two_pi(Q[3 * i + 2] + NFOPP_PI_F) - NFOPP_PI_F;
        float d = (cur + -prev);
        if (d > NFOPP_PI_F) d = (d + -NFOPP_TWO_PI_F);
        if (d < -NFOPP_PI_F) d = (d + NFOPP_TWO_PI_F);
        run = (run + d);
        prev = cur;
        Q[3 * i + 2] = (float)((double)first_angle + (double)run);
      }
      // ---- the spline through the kept poses (spline2.h)
      for (int i = 0; i < m; ++i)
        for (int d = 0; d < 3; ++d) sp.C[3 * i + d] = (double)Q[3 * i + d];
      spline_fit<3>(sp, m);
      // ---- direction of the first segments (:54-69): only the first 7 poses matter
      int first = 1;
      if (count >= 2) {
        const double step = 1.0 / (double)(count - 1);
        const int lim = count < 8 ? count : 8;
        double prevp[3];
        bool fwd0 = false;
        for (int q = 0; q < lim; ++q) {
          const double x = q == count - 1 ? 1.0 : (double)q * step;
          double p[3];
          spline_at<3>(T, C, m, x, p);
          if (q > 0) {
            double dth = fmod(p[2] - prevp[2] + NFOPP_PI_D, 2.0 * NFOPP_PI_D);
            if (dth != 0.0 && dth < 0.0) dth += 2.0 * NFOPP_PI_D;
            dth -= NFOPP_PI_D;
            const double mean = prevp[2] + dth / 2.0;
            const bool fwd = cos(mean) * (p[0] - prevp[0]) + sin(mean) * (p[1] - prevp[1]) > 0.0;
            if (q == 1) fwd0 = fwd;
            else if (fwd != fwd0) {
              const int other = q - 1;
              if (other < 6) first = other > 1 ? other : 1;
              break;
            }
          }
          prevp[0] = p[0]; prevp[1] = p[1]; prevp[2] = p[2];
        }
      }
      if (count < 0) count = 0;
      s_first = first;
    }
    s_m = m;
    s_count = count;
  }
  __syncthreads();
  const int count = s_count;
  if (count < 0) {
    if (threadIdx.x == 0) a.count[b] = -1;
    return;
  }
  const int first = count > 0 ? s_first : 0;
  const int kept = count - first > 0 ? count - first : 0;
  if (threadIdx.x == 0) a.count[b] = kept;
  const int m = s_m;
  const double step = count > 1 ? 1.0 / (double)(count - 1) : 0.0;
  double* out = a.out + b * (long long)a.max_out * 3;
  for (int q = first + threadIdx.x; q < count && q - first < a.max_out; q += PP_THREADS) {
    const double x = (q == count - 1 && count > 1) ? 1.0 : (double)q * step;
    double p[3];
    spline_at<3>(T, C, m, x, p);
    out[(q - first) * 3 + 0] = p[0];
    out[(q - first) * 3 + 1] = p[1];
    out[(q - first) * 3 + 2] = p[2];
  }
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_path_postprocess(const float* path_dev, int64_t batch, int32_t n_points, float minimal_distance,
                                      float distance_step, int32_t max_out, double* out_dev, int32_t* count_dev,
                                      void* stream) {
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL, "bad batch");
  NFOPP_REQUIRE(n_points >= 3 && n_points <= 1026, "path length must be 3..1026 poses (shorter paths pass through unchanged)");
  NFOPP_REQUIRE(distance_step > 0.f && minimal_distance >= 0.f && max_out >= 0, "bad distances");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(path_dev && count_dev && (out_dev || max_out == 0), "null device pointer");
  PostArgs a;
  a.path = path_dev; a.n = n_points; a.max_out = max_out; a.min_dist = minimal_distance; a.dist_step = distance_step;
  a.out = out_dev; a.count = count_dev;
  // the spline's area for n poses of (x, y, heading); floats behind it: poses 3n, lengths n
  const size_t lds = (size_t)spline_doubles(n_points, 3) * 8 + (size_t)(4 * n_points) * 4;
  return launch_dynamic_lds(path_post_kernel, batch, PP_THREADS, lds, stream, a, "path too long");   // 1026 poses: 72 KiB
}
