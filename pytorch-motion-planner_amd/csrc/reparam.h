// Arc-length reparametrisation of ONE trajectory held in LDS, as device functions (one workgroup of RP_THREADS per
// trajectory).  Shared by reparam_kernel (csrc/reparam.hip) and endpoint_update_kernel (csrc/endpoint_update.hip), which
// edits the LDS image between `reparam_load` and `reparam_from_lds`.
//
// Replaces nfop/constrained_nerf_opt_planner.py:132-171 (SE(2): waypoints + both multiplier arrays) and
// nfop/nerf_opt_planner.py:224-244 (2-D): xy segment lengths -> normalised cumulative distribution ->
// searchsorted(left) of the uniform grid -> linear interpolation (theta along the wrapped difference).
//
// searchsorted is INDEX work: the cdf must equal torch's bit for bit or a grid value that ties with a cdf entry lands
// on the other side of a flat run.  So the three roundings that build the cdf are torch-CPU's (each checked against
// torch in tests/test_oracle_golden.py::test_torch_reduction_orders and pinned by tests/golden/g4_reparam[clamp]):
//   * torch.norm(dim=1) of an (dx, dy) row = sqrt(fma(dy, dy, rn(dx*dx)))   (NormTwoOps `acc + data*data`, contracted)
//   * torch.sum of N+1 floats = ATen's cascade sum (SumKernel.cpp, the 8-float-vector build): 8 lane columns, four
//     interleaved accumulator chains per lane folded every 16 rows, then the scalar tail, then the lanes in order
//   * torch.cumsum accumulates in float64 (at::acc_type<float, false>) and rounds every partial sum to fp32
#pragma once
#include "block_collectives.h"
#include "common.h"

namespace nfopp {

constexpr int RP_THREADS = 256;

// ATen row_sum (native/cpu/SumKernel.cpp): element i = a[i * stride]; ilp_factor 4, cascade levels of 16 rows.
// level_power = max(4, ceil_log2(size / 4) / 4) = 4 for every size below 2^21 elements (LDS bounds N far below that).
__device__ __forceinline__ float torch_row_sum(const float* a, int stride, int size) {
  float acc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[j][k] = 0.f;
  const int rows = size / 4;
  int i = 0;
  while (i + 16 <= rows) {
    for (int j = 0; j < 16; ++j, ++i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[0][k] += a[(i * 4 + k) * stride];
    }
    bool more = true;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      if (more) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { acc[j][k] += acc[j - 1][k]; acc[j - 1][k] = 0.f; }
        if ((i & (15 << (4 * j))) != 0) more = false;
      }
    }
  }
  for (; i < rows; ++i) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[0][k] += a[(i * 4 + k) * stride];
  }
#pragma unroll
  for (int j = 1; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[0][k] += acc[j][k];
  for (int r = rows * 4; r < size; ++r) acc[0][0] += a[r * stride];
  return ((acc[0][0] + acc[0][1]) + acc[0][2]) + acc[0][3];
}

// The workgroup's LDS image of one trajectory (dynamic LDS, `reparam_lds_bytes`).
struct ReparamLds {
  float* Q;     // (N+2)*D  [start, waypoints, goal]
  float* cdf;   // N+2
  float* cmf;   // N+2      [0, cm, 0]
  float* lf;    // N+2      [l0, mid-averages, lN]
  float* li;    // N        interpolated multipliers
  float* red;   // 8 lane sums of the torch-order reduction, the total, 4 wave sums (float64)
};

template <int D>
__device__ __forceinline__ ReparamLds reparam_lds(float* sm, int N) {
  ReparamLds L;
  L.Q = sm;
  L.cdf = L.Q + (N + 2) * D;
  L.cmf = L.cdf + (N + 2);
  L.lf = L.cmf + (N + 2);
  L.li = L.lf + (N + 2);
  L.red = L.li + N;
  return L;
}

inline size_t reparam_lds_bytes(int n_waypoints, int dim) {
  return (size_t)((n_waypoints + 2) * dim + 3 * (n_waypoints + 2) + n_waypoints + 8 + 12) * 4;
}

// Fills Q, cmf and lf from one trajectory's rows (`lam` / `cm` are read for D = 3 only).  The caller synchronises.
template <int D>
__device__ __forceinline__ void reparam_load(const ReparamLds& L, int N, int tid, const float* traj, const float* start,
                                             const float* goal, const float* lam, const float* cm) {
  float* Q = L.Q;
  for (int k = tid; k < N * D; k += RP_THREADS) Q[D + k] = traj[k];
  if (tid < D) {
    Q[tid] = start[tid];
    Q[(N + 1) * D + tid] = goal[tid];
  }
  if (D == 3) {
    float* cmf = L.cmf;
    float* lf = L.lf;
    for (int k = tid; k < N + 2; k += RP_THREADS) {
      cmf[k] = (k == 0 || k == N + 1) ? 0.0f : cm[k - 1];
      lf[k] = k == 0 ? lam[0] : (k == N + 1 ? lam[N] : (lam[k - 1] + lam[k]) / 2.0f);
    }
  }
}

// Reparametrises the loaded (and synchronised) image and writes the trajectory's rows of traj [N, D], cm [N], lam [N+1].
template <int D>
__device__ __forceinline__ void reparam_from_lds(const ReparamLds& L, int N, int tid, float* traj, float* lam_out,
                                                 float* cm_out, const float* u_grid) {
  float* Q = L.Q;
  float* cdf = L.cdf;
  float* cmf = L.cmf;
  float* lf = L.lf;
  float* li = L.li;
  float* red = L.red;

  // segment lengths (xy only, constrained:45-47), torch.norm rounding
  for (int s = tid; s <= N; s += RP_THREADS) {
    const float dx = Q[(s + 1) * D] - Q[s * D], dy = Q[(s + 1) * D + 1] - Q[s * D + 1];
    cdf[s + 1] = sqrtf(__builtin_fmaf(dy, dy, dx * dx));
  }
  __syncthreads();
  // torch.sum(distances): vectorized_inner_sum with 8-float vectors when there are at least 8 elements
  const int n_el = N + 1, n_vec = n_el >= 8 ? n_el / 8 : 0;
  if (tid < 8 && n_vec > 0) red[tid] = torch_row_sum(cdf + 1 + tid, 8, n_vec);
  __syncthreads();
  if (tid == 0) {
    float total;
    if (n_vec > 0) {
      total = 0.f;
      for (int k = n_vec * 8; k < n_el; ++k) total += cdf[1 + k];
      for (int l = 0; l < 8; ++l) total += red[l];
    } else {
      total = torch_row_sum(cdf + 1, 1, n_el);   // scalar_inner_sum
    }
    red[8] = total;
    cdf[0] = 0.f;
  }
  __syncthreads();
  // torch.cumsum on CPU: a float64 accumulator walks the fp32 quotients in order and every partial sum is rounded to fp32.
  // The quotients are multiples of 2^(e-23) with e their smallest exponent and every partial sum stays below 2, so if the
  // smallest non-zero quotient is at least 2^-29 EVERY sum of a subset of them is exactly representable in float64: the
  // additions are exact, their order does not matter, and a parallel scan returns the sequential loop's partial sums bit
  // for bit.  Otherwise (a segment 2^-29 of the path length, or a degenerate path) one lane walks the sequence as torch does.
  const float total = red[8];
  const int per = (n_el + RP_THREADS - 1) / RP_THREADS, lo_s = 1 + tid * per, hi_s = min(lo_s + per, n_el + 1);
  float qmin = 1.0f;
  bool ok = total > 0.0f && total < 3.0e38f;
  for (int s2 = lo_s; s2 < hi_s; ++s2) {
    const float q = cdf[s2] / total;
    cdf[s2] = q;
    if (q != 0.0f) qmin = fminf(qmin, q);
    ok = ok && (q >= 0.0f) && (q <= 1.0f);    // (false for NaN)
  }
  ok = ok && qmin >= 1.862645149230957e-09f;   // 2^-29
  // Block-wide AND: a wave vote, then the four wave flags through `red` (its lane sums were consumed before the last
  // barrier).  Not __syncthreads_and: that builtin brings a 256-byte STATIC LDS array, which comes off the 160 KB a
  // workgroup can hold, so the longest trajectories that pass reparam_lds_bytes' limit could not be launched.
  const bool wave_ok = __all(ok);
  if ((tid & 63) == 0) red[tid >> 6] = wave_ok ? 1.0f : 0.0f;
  __syncthreads();
  const bool exact = red[0] != 0.0f && red[1] != 0.0f && red[2] != 0.0f && red[3] != 0.0f;
  if (exact) {
    double part = 0.0;
    for (int s2 = lo_s; s2 < hi_s; ++s2) part += (double)cdf[s2];
    // exclusive offsets of the per-thread sums (exact, like every sum here); the wave totals go through `red2`
    float* r8 = red + 9;
    if (reinterpret_cast<size_t>(r8) & 7) r8 += 1;        // 8-byte aligned slot for the four wave sums
    double* red2 = reinterpret_cast<double*>(r8);
    double run = block_exclusive_scan<RP_THREADS / 64>(part, 0.0, Plus(), red2);
    for (int s2 = lo_s; s2 < hi_s; ++s2) {
      run += (double)cdf[s2];
      cdf[s2] = (float)run;
    }
  } else if (tid == 0) {
    double run = 0.0;
    for (int s2 = 1; s2 <= N + 1; ++s2) {
      run += (double)cdf[s2];
      cdf[s2] = (float)run;
    }
  }
  __syncthreads();

  for (int w = tid; w < N; w += RP_THREADS) {
    const float u = u_grid[w];
    int lo = 0, hi = N + 2;  // first index with cdf[idx] >= u (torch.searchsorted, right=False)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] < u) lo = mid + 1; else hi = mid;
    }
    const int ia = lo > N + 1 ? N + 1 : lo;
    const int ib = lo - 1 < 0 ? 0 : lo - 1;
    const float cb = cdf[ib];
    float den = cdf[ia] - cb;
    if (den < 1e-5f) den = 1e-5f;
    const float tau = (u - cb) / den;
    const float omt = 1.0f - tau;
    // products and sums rounded one by one, as the reference's separate torch ops are (no contraction to fma)
    traj[w * D] = mix_unfused(omt, Q[ib * D], tau, Q[ia * D]);
    traj[w * D + 1] = mix_unfused(omt, Q[ib * D + 1], tau, Q[ia * D + 1]);
    if (D == 3) {
      const float thb = Q[ib * 3 + 2];
      traj[w * 3 + 2] = add_mul_unfused(thb, tau, wrap_angle(Q[ia * 3 + 2] - thb));
      cm_out[w] = mix_unfused(omt, cmf[ib], tau, cmf[ia]);
      li[w] = mix_unfused(omt, lf[ib], tau, lf[ia]);
    }
  }
  if (D == 3) {
    __syncthreads();
    for (int k = tid; k <= N; k += RP_THREADS)
      lam_out[k] = k == 0 ? li[0] : (k == N ? li[N - 1] : (li[k - 1] + li[k]) / 2.0f);
  }
}

}  // namespace nfopp
