// Time parametrisation of planned paths under motion limits: when the robot is where, and how fast it may go.  The
// planner's other outputs are geometry (poses, length, curvature, cusps, clearance); these two entries add the velocity
// profile and the timed trajectory of a whole batch on the device.  The batch axis and the rule are this library's own
// (the reference plans one path and hands its poses to a follower).
//
//   * nfopp_path_time_profile   one workgroup per path, the path's image in LDS, float64 + two integer prefix sums
//   * nfopp_path_time_sample    one thread per instant, the path's time column in LDS
//
// The rule (restated in numpy in tests/time_profile_ref.py; include/nfopp_hip.h repeats it for callers).  Everything is
// float64 with every operation rounded on its own.  Polyline p_0 .. p_{N+1} = start, waypoints, goal, read as fp32, widened;
// segment i = 0..N joins p_i and p_{i+1}: ex, ey its xy difference.  A = 2 * a_max, Dd = 2 * d_max.
//  Arc length, fixed point.  n_i = sqrt(ex * ex + ey * ey), L_i = llrint(n_i * 2^32), S_i = L_0 + .. + L_{i-1} in integers,
//    s_i = S_i * 2^-32.  Integer sums are exact in any order: the parallel scan here and a sequential loop give the same
//    bits, which no float sum of 2000 terms does.
//  Gear (dim 3; all +1 for dim 2).  The sign of cos(theta_i) * ex + sin(theta_i) * ey as nfopp_path_stats forms it; a zero
//    sign takes the last non-zero sign before it, else the first non-zero sign after it, else +1.
//  Vertex caps on v^2.  kappa_i = the Menger curvature of nfopp_path_stats at interior vertex i (same candidate rule);
//    k_i = min(a_lat / kappa_i, (w_max / kappa_i)^2) where kappa_i exists and is > 0, else +inf; k_0 = k_{N+1} = +inf.
//    Vertex i is a STOP when it is a cusp by nfopp_path_stats' rule with limits.cos_cusp (never when cos_cusp == -1), or
//    when the gears of segments i - 1 and i differ.  c_i = 0 at a stop, else min(v_max^2, k_i); c_0 = v_start^2,
//    c_{N+1} = v_goal^2.
//  Speeds, closed form of the forward and the backward sweep:
//    fwd_i = min_{j <= i}(c_j - A * s_j) + A * s_i,   bwd_i = min_{j >= i}(c_j + Dd * s_j) - Dd * s_i,
//    u_i = max(0, min(c_i, fwd_i, bwd_i)),  v_i = sqrt(u_i).  Minima are exact and order-free: two scans, not two loops.
//  Segment i, time-optimal on a straight piece.  ds = L_i * 2^-32, g = min(v_max^2, max(k_i, k_{i+1})),
//    u_p = max(min(g, (((A * d_max) * ds + d_max * u_i) + a_max * u_{i+1}) / (a_max + d_max)), max(u_i, u_{i+1})),
//    v_p = sqrt(u_p), t_acc = (v_p - v_i) / a_max, t_dec = (v_p - v_{i+1}) / d_max,
//    l_cruise = max(0, (ds - (u_p - u_i) / A) - (u_p - u_{i+1}) / Dd), t_cruise = l_cruise > 0 ? l_cruise / v_p : 0,
//    duration = (t_acc + t_cruise) + t_dec, Q_i = llrint(duration * 2^32), T_i its integer prefix sum, t_i = T_i * 2^-32.
//  Status.  1: u_0 < v_start^2.  2: u_{N+1} < v_goal^2.  4 (alone): a non-finite coordinate, a speed that is not in
//    [0, inf), a segment of 2^20 m or more, a total of 2^21 m or more, or a duration that is not below 2^20 s; the row's
//    profile and the first three summary slots are then NaN and its gear is 0.
//  Sampling at t = t0 + k * dt (k * dt rounded, then the sum).  Before t_0: start pose, speed 0, segment -1.  At or after
//    t_{N+1}: goal pose, gear_N * v_{N+1}, segment N + 1.  A NaN profile row: NaN states, segment -1.  Else i = the largest
//    i <= N with t_i <= t (binary search), tau = t - t_i, dur = t_{i+1} - t_i, rem = dur - tau, ds = s_{i+1} - s_i,
//    t_acc = (v_p - v_i) / a_max, t_dec = (v_p - v_{i+1}) / d_max, ha = 0.5 * a_max, hd = 0.5 * d_max:
//      tau < t_acc:        dist = v_i * tau + (ha * tau) * tau,                                speed = v_i + a_max * tau
//      else rem < t_dec:   dist = ds - (v_{i+1} * rem + (hd * rem) * rem),                     speed = v_{i+1} + d_max * rem
//      else:               dist = (v_i * t_acc + (ha * t_acc) * t_acc) + v_p * (tau - t_acc),  speed = v_p
//    dist = min(max(dist, 0), ds), speed = min(speed, v_p), frac = ds > 0 ? dist / ds : 0;
//    x = fp32(x_i + frac * (x_{i+1} - x_i)), y alike, theta = fp32(theta_i + frac * dth) with dth the fp32
//    wrap_angle(theta_{i+1} - theta_i) of nfopp_path_interpolate, widened; signed speed = fp32(gear_i * speed).
//
// No atomics, no static LDS (every byte of LDS is dynamic and follows the path length; a static array would come off the
// 160 KiB as reparam.h notes for __syncthreads_and).  The same bits run after run.
#include "block_collectives.h"
#include "common.h"

#pragma clang fp contract(off)

namespace nfopp {

constexpr int TP_THREADS = 256;
constexpr int TP_WAVES = TP_THREADS / 64;
constexpr double TP_TWO32 = 4294967296.0, TP_INV32 = 1.0 / 4294967296.0;
constexpr double TP_SEG_LIMIT = 1048576.0, TP_TOTAL_LIMIT = 2097152.0, TP_TIME_LIMIT = 1048576.0;
typedef unsigned long long u64;

struct ProfileArgs {
  const float* traj; const float* start; const float* goal;
  int n, dim;
  nfopp_motion_limits lim;
  const float* v_start; const float* v_goal;
  double* profile; signed char* gear; double* summary;
};

// LDS image of one path of m = N + 2 vertices: 16 bytes of scan scratch per wave, five 8-byte columns, the fp32 poses, two
// int8 columns.  The longest path served is the largest m with tp_lds_bytes(m, dim) <= 160 KiB: N + 2 <= 3032 for dim 3,
// 3275 for dim 2.
inline size_t tp_lds_bytes(long long m, int dim) {
  return (size_t)(TP_WAVES * 16 + m * 40 + ((m * dim * 4 + 7) & ~7LL) + ((2 * m + 15) & ~15LL));
}

struct MinOp {
  __device__ __forceinline__ double operator()(double a, double b) const { return b < a ? b : a; }
};

template <int D>
__global__ __launch_bounds__(TP_THREADS) void time_profile_kernel(const ProfileArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
  const int N = a.n, M = N + 2, tid = threadIdx.x;
  u64* redu = reinterpret_cast<u64*>(tp_smem);                   // [TP_WAVES]
  double* redd = reinterpret_cast<double*>(tp_smem) + TP_WAVES;  // [TP_WAVES]
  u64* S = reinterpret_cast<u64*>(tp_smem + TP_WAVES * 16);      // [M] L_i, then the exclusive prefix S_i
  u64* T = S + M;                                                // [M] Q_i, then T_i
  double* K = reinterpret_cast<double*>(T + M);                  // [M] k_i
  double* C = K + M;                                             // [M] c_i
  double* U = C + M;                                             // [M] u_i
  float* P = reinterpret_cast<float*>(U + M);                    // [M, D]
  signed char* sg = reinterpret_cast<signed char*>(tp_smem + TP_WAVES * 16 + (size_t)M * 40 + (((size_t)M * D * 4 + 7) & ~(size_t)7));
  signed char* gr = sg + M;                                      // [M] gear of segment i
  const long long b = blockIdx.x;
  const nfopp_motion_limits lim = a.lim;
  const double A = 2.0 * lim.a_max, Dd = 2.0 * lim.d_max, vmax2 = lim.v_max * lim.v_max;
  const double inf = (double)__builtin_inff(), qnan = (double)__builtin_nanf("");

  // the path's image
  int bad = 0;
  for (int k = tid; k < M * D; k += TP_THREADS) {
    const float v = path_entry<D>(a.traj, a.start, a.goal, N, b, k);
    P[k] = v;
    if (!(fabsf(v) < __builtin_inff())) bad = 1;
  }
  const double vs = a.v_start ? (double)a.v_start[b] : 0.0, vg = a.v_goal ? (double)a.v_goal[b] : 0.0;
  if (!(vs >= 0.0 && vs < inf && vg >= 0.0 && vg < inf)) bad = 1;
  __syncthreads();
  auto px = [&](int i) { return (double)P[i * D]; };
  auto py = [&](int i) { return (double)P[i * D + 1]; };

  // segments: fixed-point length, raw forward sign
  for (int i = tid; i < M; i += TP_THREADS) {
    u64 l = 0;
    signed char s = 1;
    if (i <= N) {
      const double ex = px(i + 1) - px(i), ey = py(i + 1) - py(i);
      const double n = sqrt(ex * ex + ey * ey);
      if (n < TP_SEG_LIMIT) l = (u64)llrint(n * TP_TWO32); else bad = 1;
      if (D == 3) {
        const double th = (double)P[i * D + 2];
        const double fwd = cos(th) * ex + sin(th) * ey;
        s = fwd > 0.0 ? 1 : (fwd < 0.0 ? -1 : 0);
      }
    }
    S[i] = l;
    sg[i] = s;
  }
  __syncthreads();

  // S_i: every thread owns a run of `per` consecutive entries
  const int per = (M + TP_THREADS - 1) / TP_THREADS, lo = min(tid * per, M), hi = min(lo + per, M);
  {
    u64 part = 0;
    for (int i = lo; i < hi; ++i) part += S[i];
    u64 run = block_exclusive_scan<TP_WAVES>(part, (u64)0, Plus(), redu);
    for (int i = lo; i < hi; ++i) { const u64 l = S[i]; S[i] = run; run += l; }
  }
  // gear of each segment (S and gr are published by the barriers of the next scan)
  for (int i = tid; i <= N; i += TP_THREADS) {
    signed char s = sg[i];
    if (D == 3 && s == 0) {
      int j = i - 1;
      while (j >= 0 && sg[j] == 0) --j;
      if (j < 0) { j = i + 1; while (j <= N && sg[j] == 0) ++j; }
      s = (j >= 0 && j <= N) ? sg[j] : 1;
    }
    gr[i] = s;
  }
  __syncthreads();
  if ((double)S[N + 1] >= TP_TOTAL_LIMIT * TP_TWO32) bad = 1;
  auto s_of = [&](int i) { return (double)S[i] * TP_INV32; };

  // vertex caps
  int stops = 0;
  for (int i = tid; i < M; i += TP_THREADS) {
    double k = inf, c;
    if (i == 0) c = vs * vs;
    else if (i == N + 1) c = vg * vg;
    else {
      const double x0 = px(i - 1), y0 = py(i - 1), x1 = px(i), y1 = py(i), x2 = px(i + 1), y2 = py(i + 1);
      const double ex0 = x1 - x0, ey0 = y1 - y0, ex1 = x2 - x1, ey1 = y2 - y1, cx = x2 - x0, cy = y2 - y0;
      const double n0 = sqrt(ex0 * ex0 + ey0 * ey0), n1 = sqrt(ex1 * ex1 + ey1 * ey1), ch = sqrt(cx * cx + cy * cy);
      bool stop = gr[i - 1] != gr[i];
      if (n0 > 0.0 && n1 > 0.0) {
        if (ch > 0.0) {
          const double kappa = (2.0 * fabs(ex0 * ey1 - ey0 * ex1)) / ((n0 * n1) * ch);
          if (kappa > 0.0) {
            const double q = lim.w_max / kappa, kl = lim.a_lat / kappa, kw = q * q;
            k = kw < kl ? kw : kl;
          }
        }
        if (lim.cos_cusp > -1.0 && ex0 * ex1 + ey0 * ey1 < lim.cos_cusp * (n0 * n1)) stop = true;
      }
      c = stop ? 0.0 : (k < vmax2 ? k : vmax2);
      stops += stop ? 1 : 0;
    }
    K[i] = k;
    C[i] = c;
  }
  __syncthreads();

  // u_i = max(0, min(c_i, fwd_i, bwd_i)): a prefix minimum and a suffix minimum
  {
    double part = inf;
    for (int i = lo; i < hi; ++i) { const double v = C[i] - A * s_of(i); part = v < part ? v : part; }
    double run = block_exclusive_scan<TP_WAVES>(part, inf, MinOp(), redd);
    for (int i = lo; i < hi; ++i) {
      const double As = A * s_of(i), v = C[i] - As;
      run = v < run ? v : run;
      const double fwd = run + As;
      U[i] = fwd < C[i] ? fwd : C[i];
    }
  }
  {
    // the same run of entries, counted from the far end: thread order = descending index
    const int rlo = M - hi, rhi = M - lo;   // this thread owns indices M - 1 - r for r in [lo, hi) = [rlo, rhi)
    double part = inf;
    for (int i = rhi - 1; i >= rlo; --i) { const double v = C[i] + Dd * s_of(i); part = v < part ? v : part; }
    double run = block_exclusive_scan<TP_WAVES>(part, inf, MinOp(), redd);
    for (int i = rhi - 1; i >= rlo; --i) {
      const double Ds = Dd * s_of(i), v = C[i] + Ds;
      run = v < run ? v : run;
      const double bwd = run - Ds;
      double u = U[i];      // written by the thread that owns i in ascending order: published by the scan's barriers
      u = bwd < u ? bwd : u;
      U[i] = u > 0.0 ? u : 0.0;
    }
  }
  __syncthreads();

  // segments: peak speed and duration; v_p goes straight to slot 3
  double* prof = a.profile + b * M * 4;
  for (int i = tid; i < M; i += TP_THREADS) {
    u64 q = 0;
    if (i <= N) {
      const double ds = (double)(S[i + 1] - S[i]) * TP_INV32;
      const double u0 = U[i], u1 = U[i + 1], v0 = sqrt(u0), v1 = sqrt(u1);
      const double km = K[i] > K[i + 1] ? K[i] : K[i + 1], g = km < vmax2 ? km : vmax2;
      const double reach = (((A * lim.d_max) * ds + lim.d_max * u0) + lim.a_max * u1) / (lim.a_max + lim.d_max);
      double up = reach < g ? reach : g;
      const double ue = u0 > u1 ? u0 : u1;
      up = up > ue ? up : ue;
      const double vp = sqrt(up);
      const double t_acc = (vp - v0) / lim.a_max, t_dec = (vp - v1) / lim.d_max;
      double lc = (ds - (up - u0) / A) - (up - u1) / Dd;
      lc = lc > 0.0 ? lc : 0.0;
      const double t_cruise = lc > 0.0 ? lc / vp : 0.0;
      const double dur = (t_acc + t_cruise) + t_dec;
      if (dur < TP_TIME_LIMIT) q = (u64)llrint(dur * TP_TWO32); else bad = 1;
      prof[i * 4 + 3] = vp;
    }
    T[i] = q;
  }
  __syncthreads();
  {
    u64 part = 0;
    for (int i = lo; i < hi; ++i) part += T[i];
    u64 run = block_exclusive_scan<TP_WAVES>(part, (u64)0, Plus(), redu);
    for (int i = lo; i < hi; ++i) { const u64 q = T[i]; T[i] = run; run += q; }
  }
  // workgroup totals of small integer counts (exact in any order); their barriers publish T
  const u64 n_stops = block_reduce<TP_WAVES>((u64)stops, (u64)0, Plus(), redu);
  const bool out_of_range = block_reduce<TP_WAVES>((u64)bad, (u64)0, Plus(), redu) != 0;

  for (int i = tid; i < M; i += TP_THREADS) {
    double* o = prof + i * 4;
    if (out_of_range) { o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = qnan; continue; }
    const double v = sqrt(U[i]);
    o[0] = s_of(i); o[1] = (double)T[i] * TP_INV32; o[2] = v;
    if (i == N + 1) o[3] = v;
  }
  if (a.gear)
    for (int i = tid; i <= N; i += TP_THREADS) a.gear[b * (N + 1) + i] = out_of_range ? 0 : gr[i];
  if (tid == 0) {
    double* o = a.summary + b * 4;
    if (out_of_range) { o[0] = qnan; o[1] = qnan; o[2] = qnan; o[3] = 4.0; }
    else {
      o[0] = (double)T[N + 1] * TP_INV32; o[1] = s_of(N + 1); o[2] = (double)n_stops;
      o[3] = (double)((U[0] < vs * vs ? 1 : 0) | (U[N + 1] < vg * vg ? 2 : 0));
    }
  }
}

struct SampleArgs {
  const float* traj; const float* start; const float* goal;
  int n, dim;
  nfopp_motion_limits lim;
  const double* profile; const signed char* gear;
  double t0, dt;
  int count, chunks;   // chunks = workgroups per path
  float* states; int* segment;
};

template <int D>
__global__ __launch_bounds__(TP_THREADS) void time_sample_kernel(const SampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
  double* tc = reinterpret_cast<double*>(tp_smem);   // [N + 2] the path's t column
  const int N = a.n, M = N + 2;
  const long long b = blockIdx.x / a.chunks;
  const int k = (int)(blockIdx.x % a.chunks) * TP_THREADS + threadIdx.x;
  const double* prof = a.profile + b * M * 4;
  for (int i = threadIdx.x; i < M; i += TP_THREADS) tc[i] = prof[i * 4 + 1];
  __syncthreads();
  if (k >= a.count) return;
  auto pose = [&](int f, int d) { return path_entry<D>(a.traj, a.start, a.goal, N, b, f * D + d); };
  float* o = a.states + (b * a.count + k) * (D + 1);
  const double t = a.t0 + (double)k * a.dt;
  const double t_end = tc[N + 1];
  int seg = -1;
  if (t_end != t_end) {
#pragma unroll
    for (int d = 0; d <= D; ++d) o[d] = __builtin_nanf("");
  } else if (t < tc[0]) {
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] = pose(0, d);
    o[D] = 0.f;
  } else if (t >= t_end) {
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] = pose(N + 1, d);
    const double g = a.gear ? (double)a.gear[b * (N + 1) + N] : 1.0;
    o[D] = (float)(g * prof[(N + 1) * 4 + 2]);
    seg = N + 1;
  } else {
    int lo = 0, hi = N;   // the largest i in [0, N] with t_i <= t: t_0 <= t holds
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tc[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int i = lo;
    seg = i;
    const nfopp_motion_limits lim = a.lim;
    const double tau = t - tc[i], dur = tc[i + 1] - tc[i], rem = dur - tau;
    const double ds = prof[(i + 1) * 4] - prof[i * 4];
    const double v0 = prof[i * 4 + 2], v1 = prof[(i + 1) * 4 + 2], vp = prof[i * 4 + 3];
    const double t_acc = (vp - v0) / lim.a_max, t_dec = (vp - v1) / lim.d_max;
    const double ha = 0.5 * lim.a_max, hd = 0.5 * lim.d_max;
    double dist, speed;
    if (tau < t_acc) {
      dist = v0 * tau + (ha * tau) * tau;
      speed = v0 + lim.a_max * tau;
    } else if (rem < t_dec) {
      dist = ds - (v1 * rem + (hd * rem) * rem);
      speed = v1 + lim.d_max * rem;
    } else {
      dist = (v0 * t_acc + (ha * t_acc) * t_acc) + vp * (tau - t_acc);
      speed = vp;
    }
    dist = dist > 0.0 ? dist : 0.0;
    dist = dist < ds ? dist : ds;
    speed = speed < vp ? speed : vp;
    const double frac = ds > 0.0 ? dist / ds : 0.0;
    const double x0 = (double)pose(i, 0), y0 = (double)pose(i, 1);
    o[0] = (float)(x0 + frac * ((double)pose(i + 1, 0) - x0));
    o[1] = (float)(y0 + frac * ((double)pose(i + 1, 1) - y0));
    if (D == 3) {
      const float th0 = pose(i, 2);
      const double dth = (double)wrap_angle(pose(i + 1, 2) - th0);
      o[2] = (float)((double)th0 + frac * dth);
    }
    const double g = a.gear ? (double)a.gear[b * (N + 1) + i] : 1.0;
    o[D] = (float)(g * speed);
  }
  if (a.segment) a.segment[b * a.count + k] = seg;
}

static int check_common(int64_t batch, int32_t n_waypoints, int32_t dim, const nfopp_motion_limits* limits) {
  NFOPP_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL && n_waypoints >= 1, "bad batch / waypoint count");
  NFOPP_REQUIRE(limits, "null motion limits");
  const double inf = (double)__builtin_inff();
  NFOPP_REQUIRE(limits->v_max > 0.0 && limits->v_max < inf, "v_max must be positive and finite");
  NFOPP_REQUIRE(limits->a_max > 0.0 && limits->a_max < inf, "a_max must be positive and finite");
  NFOPP_REQUIRE(limits->d_max > 0.0 && limits->d_max < inf, "d_max must be positive and finite");
  NFOPP_REQUIRE(limits->a_lat > 0.0, "a_lat must be positive (+inf = no lateral limit)");
  NFOPP_REQUIRE(limits->w_max > 0.0, "w_max must be positive (+inf = no turn-rate limit)");
  NFOPP_REQUIRE(limits->cos_cusp >= -1.0 && limits->cos_cusp <= 1.0, "cos_cusp must lie in [-1, 1]");
  return NFOPP_OK;
}

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_path_time_profile(const float* traj_dev, const float* start_dev, const float* goal_dev, int64_t batch,
                                       int32_t n_waypoints, int32_t dim, const nfopp_motion_limits* limits,
                                       const float* v_start_dev, const float* v_goal_dev, double* profile_dev,
                                       int8_t* gear_dev, double* summary_dev, void* stream) {
  const int rc = check_common(batch, n_waypoints, dim, limits);
  if (rc) return rc;
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(traj_dev && start_dev && goal_dev && profile_dev && summary_dev, "null device pointer");
  ProfileArgs a;
  a.traj = traj_dev; a.start = start_dev; a.goal = goal_dev; a.n = n_waypoints; a.dim = dim; a.lim = *limits;
  a.v_start = v_start_dev; a.v_goal = v_goal_dev;
  a.profile = profile_dev; a.gear = reinterpret_cast<signed char*>(gear_dev); a.summary = summary_dev;
  return launch_dynamic_lds(dim == 3 ? time_profile_kernel<3> : time_profile_kernel<2>, batch, TP_THREADS,
                            tp_lds_bytes((long long)n_waypoints + 2, dim), stream, a, "path too long");
}

extern "C" int nfopp_path_time_sample(const float* traj_dev, const float* start_dev, const float* goal_dev, int64_t batch,
                                      int32_t n_waypoints, int32_t dim, const nfopp_motion_limits* limits,
                                      const double* profile_dev, const int8_t* gear_dev, double t0, double dt, int32_t count,
                                      float* states_dev, int32_t* segment_dev, void* stream) {
  const int rc = check_common(batch, n_waypoints, dim, limits);
  if (rc) return rc;
  NFOPP_REQUIRE(dt > 0.0 && dt < (double)__builtin_inff(), "dt must be positive and finite");
  NFOPP_REQUIRE(t0 == t0 && fabs(t0) < (double)__builtin_inff(), "t0 must be finite");
  NFOPP_REQUIRE(count >= 0, "count must not be negative");
  if (batch == 0 || count == 0) return NFOPP_OK;
  NFOPP_REQUIRE(traj_dev && start_dev && goal_dev && profile_dev && states_dev, "null device pointer");
  const long long chunks = ((long long)count + TP_THREADS - 1) / TP_THREADS;
  NFOPP_REQUIRE(batch * chunks <= 0x7fffffffLL, "too many instants for one call");
  SampleArgs a;
  a.traj = traj_dev; a.start = start_dev; a.goal = goal_dev; a.n = n_waypoints; a.dim = dim; a.lim = *limits;
  a.profile = profile_dev; a.gear = reinterpret_cast<const signed char*>(gear_dev); a.t0 = t0; a.dt = dt;
  a.count = count; a.chunks = (int)chunks; a.states = states_dev; a.segment = segment_dev;
  return launch_dynamic_lds(dim == 3 ? time_sample_kernel<3> : time_sample_kernel<2>, batch * chunks, TP_THREADS,
                            ((size_t)n_waypoints + 2) * 8, stream, a, "path too long");
}
