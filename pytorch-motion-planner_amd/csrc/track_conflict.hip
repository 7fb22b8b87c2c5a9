// Conflict detection between timed tracks: which robots of a fleet come closer than their radii allow, when first, and with
// whom -- and the same for a batch of timed paths against predicted tracks of moving obstacles.  Every other collision
// facility of the library compares a path with a static map; this one compares tracks with tracks, all pairs, on the device.
// The rule is this library's own (the reference plans one robot on a static floor).
//
//   * track_conflict_tile_kernel    one workgroup per TC_TILE_A x TC_TILE_B tile of pairs, TC_CHUNK instants of both sides
//                                   staged in LDS per trip, 2 x 2 pairs per thread; per-tile partials of every row (and column)
//   * track_conflict_reduce_kernel  one thread per track: the lexicographic minima and the count over its tiles' partials
//
// The pair rule -- the closest approach of an interval, R and R2, the strict conflict test, the first-contact fraction -- and
// the map from a workgroup to its tile of pairs are those of track_pairs.h, which states them.  What is this file's own:
//  A track with a non-finite coordinate or radius is BAD: skipped as a partner by everyone, its own summary row NaN with
//    status NFOPP_CONFLICT_BAD_TRACK, its pair-matrix rows and columns NaN (the diagonal entry included).
//  Summary row of track i: lexicographic minima over the good partners j on (g_ij, j) and on (tc_ij, j) -- the smaller j wins
//    a tie -- and the number of partners in conflict.
//  Self mode (no set B): partners are all j != i.  Swapping i and j negates d0, d1 and w exactly, and every product of the
//    rule is of two negated factors, so every quantity is even in the sign of d: the pair matrices are bitwise symmetric.
//    The kernel evaluates the tiles of the upper triangle only and serves both rows from them.
//
// No atomics and no float sums: minima are order-free and the count is an integer, so two runs give the same bits.
#include "common.h"
#include "track_pairs.h"

#pragma clang fp contract(off)

namespace nfopp {

constexpr int TC_TILE_A = 32;    // A-tracks of a tile
constexpr int TC_TILE_B = 32;    // B-tracks of a tile
constexpr int TC_CHUNK = 32;     // instants staged per trip
constexpr int TC_THREADS = 256;  // 16 x 16 threads, 2 x 2 pairs each
constexpr int TC_PITCH = TC_TILE_B + 1;
constexpr int TC_PART = 6;       // doubles of a partial: min gap, its partner, its time, first time, its partner, conflicts (-1: bad)
static_assert(TC_TILE_A == 32 && TC_TILE_B == 32 && TC_THREADS == 256, "the thread map below is 16 x 16 threads on 32 x 32 pairs");
static_assert(TC_CHUNK * TC_PITCH * 8 * 2 <= 3 * TC_TILE_A * TC_PITCH * 8, "the staging area fits the result area");

struct ConflictArgs {
  const float* a; const float* b;      // b == a in self mode
  const float* ra; const float* rb;    // rb == ra in self mode
  long long ba, bb;
  int stride_a, stride_b, k, self;
  double t0, dt, margin;
  double* pair_gap; double* pair_first;
  double* part_a; double* part_b;      // [ba, ntb, TC_PART], [bb, nta, TC_PART] (null: not wanted; self mode: part_a alone)
  long long nta, ntb;
};

// (value, index) partial of one row over one tile's partners, in ascending partner order: strict < keeps the smaller index
struct RowMin {
  double g, j, t, tc, jc, n;
  __device__ __forceinline__ void init() {
    g = (double)__builtin_inff(); j = -1.0; t = (double)__builtin_nanf(""); tc = (double)__builtin_inff(); jc = -1.0; n = 0.0;
  }
  __device__ __forceinline__ void take(double pg, double pt, double ptc, double idx) {
    if (pg != pg) return;   // not a partner: a bad track, the track itself, or past the end
    if (pg < g) { g = pg; j = idx; t = pt; }
    if (ptc < tc) { tc = ptc; jc = idx; }
    if (ptc < (double)__builtin_inff()) n += 1.0;
  }
};

__global__ __launch_bounds__(TC_THREADS) void track_conflict_tile_kernel(const ConflictArgs p) {
  __shared__ __attribute__((aligned(16))) double tc_smem[3 * TC_TILE_A * TC_PITCH];
  __shared__ int sbad[TC_TILE_A + TC_TILE_B];
  float2* sA = reinterpret_cast<float2*>(tc_smem);   // [TC_CHUNK][TC_PITCH]
  float2* sB = sA + TC_CHUNK * TC_PITCH;             // [TC_CHUNK][TC_PITCH]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const double inf = (double)__builtin_inff(), qnan = (double)__builtin_nanf("");

  long long ta, tb;
  if (p.self) upper_triangle_tile(blockIdx.x, p.nta, &ta, &tb);
  else pair_tile(blockIdx.x, p.ntb, &ta, &tb);
  const long long a0 = ta * TC_TILE_A, b0 = tb * TC_TILE_B;

  // radii; a non-finite one makes the track bad, as a non-finite coordinate does below
  if (tid < TC_TILE_A + TC_TILE_B) {
    const bool is_a = tid < TC_TILE_A;
    const long long g = is_a ? a0 + tid : b0 + (tid - TC_TILE_A);
    const float* rad = is_a ? p.ra : p.rb;
    const float r = (rad && g < (is_a ? p.ba : p.bb)) ? rad[g] : 0.f;
    sbad[tid] = finite32(r) ? 0 : 1;
  }
  double R[2][2], R2[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const long long gi = a0 + ty + 16 * r, gj = b0 + tx + 16 * c;
      const double ra = (p.ra && gi < p.ba) ? (double)p.ra[gi] : 0.0, rb = (p.rb && gj < p.bb) ? (double)p.rb[gj] : 0.0;
      pair_radius(ra, rb, p.margin, &R[r][c], &R2[r][c]);
    }

  double M[2][2], ss[2][2], tc[2][2], d0x[2][2], d0y[2][2], c0[2][2];
  int ks[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) { M[r][c] = inf; ss[r][c] = 0.0; tc[r][c] = inf; ks[r][c] = 0; d0x[r][c] = d0y[r][c] = c0[r][c] = 0.0; }

  const long long row_a = (long long)p.k * p.stride_a, row_b = (long long)p.k * p.stride_b;
  for (int k0 = 0; k0 < p.k; k0 += TC_CHUNK) {
    const int n = min(TC_CHUNK, p.k - k0);
    __syncthreads();   // the previous trip's reads; sbad's initial values
    for (int idx = tid; idx < (TC_TILE_A + TC_TILE_B) * TC_CHUNK; idx += TC_THREADS) {
      const int kk = idx & (TC_CHUNK - 1), tr = idx / TC_CHUNK;
      if (kk >= n) continue;
      const bool is_a = tr < TC_TILE_A;
      const int lt = is_a ? tr : tr - TC_TILE_A;
      const long long g = (is_a ? a0 : b0) + lt;
      float2 v = make_float2(0.f, 0.f);
      if (g < (is_a ? p.ba : p.bb)) {
        const float* src = is_a ? p.a + g * row_a + (long long)(k0 + kk) * p.stride_a
                                : p.b + g * row_b + (long long)(k0 + kk) * p.stride_b;
        v.x = src[0]; v.y = src[1];
        if (!(finite32(v.x) && finite32(v.y))) sbad[tr] = 1;   // every writer writes 1
      }
      (is_a ? sA : sB)[kk * TC_PITCH + lt] = v;
    }
    __syncthreads();
    for (int kk = 0; kk < n; ++kk) {
      const int k = k0 + kk;
      float2 pa[2], pb[2];
      pa[0] = sA[kk * TC_PITCH + ty]; pa[1] = sA[kk * TC_PITCH + ty + 16];
      pb[0] = sB[kk * TC_PITCH + tx]; pb[1] = sB[kk * TC_PITCH + tx + 16];
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const double d1x = (double)pa[r].x - (double)pb[c].x, d1y = (double)pa[r].y - (double)pb[c].y;
          const double e = d1x * d1x + d1y * d1y;
          if (k > 0) {   // interval k - 1: d1 of the previous instant is d0 of this one, across chunk boundaries too
            const Approach q = closest_approach(d0x[r][c], d0y[r][c], c0[r][c], d1x, d1y, e);
            if (q.m < M[r][c]) { M[r][c] = q.m; ks[r][c] = k - 1; ss[r][c] = q.s; }
            if (q.m < R2[r][c] && !(tc[r][c] < inf))
              tc[r][c] = (p.t0 + (double)(k - 1) * p.dt) + entry_fraction(q.a, q.b, c0[r][c], R2[r][c], q.s) * p.dt;
          }
          d0x[r][c] = d1x; d0y[r][c] = d1y; c0[r][c] = e;
        }
    }
  }
  __syncthreads();   // the last trip's reads: the staging area becomes the result area

  double* resG = tc_smem;                           // [TC_TILE_A][TC_PITCH] gap, NaN = not a partner
  double* resT = resG + TC_TILE_A * TC_PITCH;       // time of the closest approach
  double* resC = resT + TC_TILE_A * TC_PITCH;       // time of the first conflict
  const bool mirror = p.self && ta != tb;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int li = ty + 16 * r, lj = tx + 16 * c;
      const long long gi = a0 + li, gj = b0 + lj;
      // the last-instant term: s = 0, m = |d_{K-1}|^2
      const double m = c0[r][c];
      if (m < M[r][c]) { M[r][c] = m; ks[r][c] = p.k - 1; ss[r][c] = 0.0; }
      if (m < R2[r][c] && !(tc[r][c] < inf)) tc[r][c] = (p.t0 + (double)(p.k - 1) * p.dt) + 0.0 * p.dt;
      const bool inside = gi < p.ba && gj < p.bb, bad = sbad[li] != 0 || sbad[TC_TILE_A + lj] != 0;
      const bool same = p.self && gi == gj;
      const double g = sqrt(M[r][c]) - R[r][c];
      const double ts = (p.t0 + (double)ks[r][c] * p.dt) + ss[r][c] * p.dt;
      const bool partner = inside && !bad && !same;
      resG[li * TC_PITCH + lj] = partner ? g : qnan;
      resT[li * TC_PITCH + lj] = ts;
      resC[li * TC_PITCH + lj] = tc[r][c];
      if (inside) {
        const double og = bad ? qnan : (same ? inf : g), oc = bad ? qnan : (same ? inf : tc[r][c]);
        if (p.pair_gap) {
          p.pair_gap[gi * p.bb + gj] = og;
          if (mirror) p.pair_gap[gj * p.bb + gi] = og;
        }
        if (p.pair_first) {
          p.pair_first[gi * p.bb + gj] = oc;
          if (mirror) p.pair_first[gj * p.bb + gi] = oc;
        }
      }
    }
  __syncthreads();

  // per-tile partials: wave 0 takes the rows, wave 1 the columns
  if (tid < TC_TILE_A) {
    const long long gi = a0 + tid;
    if (gi < p.ba) {
      RowMin q; q.init();
      for (int lj = 0; lj < TC_TILE_B; ++lj)
        q.take(resG[tid * TC_PITCH + lj], resT[tid * TC_PITCH + lj], resC[tid * TC_PITCH + lj], (double)(b0 + lj));
      double* o = p.part_a + (gi * p.ntb + tb) * TC_PART;
      o[0] = q.g; o[1] = q.j; o[2] = q.t; o[3] = q.tc; o[4] = q.jc; o[5] = sbad[tid] ? -1.0 : q.n;
    }
  } else if (tid >= 64 && tid < 64 + TC_TILE_B) {
    const int lj = tid - 64;
    const long long gj = b0 + lj;
    double* part = p.self ? (mirror ? p.part_a : nullptr) : p.part_b;
    if (part && gj < p.bb) {
      RowMin q; q.init();
      for (int li = 0; li < TC_TILE_A; ++li)
        q.take(resG[li * TC_PITCH + lj], resT[li * TC_PITCH + lj], resC[li * TC_PITCH + lj], (double)(a0 + li));
      double* o = part + (gj * p.nta + ta) * TC_PART;   // self mode: nta == ntb, the row of track gj, tile column ta
      o[0] = q.g; o[1] = q.j; o[2] = q.t; o[3] = q.tc; o[4] = q.jc; o[5] = sbad[TC_TILE_A + lj] ? -1.0 : q.n;
    }
  }
}

// summary [n_tracks, NFOPP_NUM_CONFLICT_SLOTS] from part [n_tracks, n_tiles, TC_PART], tiles in ascending partner order
__global__ __launch_bounds__(TC_THREADS) void track_conflict_reduce_kernel(const double* part, long long n_tracks, long long n_tiles,
                                                                           double* summary) {
  const long long i = (long long)blockIdx.x * TC_THREADS + threadIdx.x;
  if (i >= n_tracks) return;
  const double qnan = (double)__builtin_nanf("");
  RowMin q; q.init();
  bool bad = false;
  const double* row = part + i * n_tiles * TC_PART;
  for (long long t = 0; t < n_tiles; ++t) {
    const double* o = row + t * TC_PART;
    if (o[5] < 0.0) bad = true;
    if (o[0] < q.g) { q.g = o[0]; q.j = o[1]; q.t = o[2]; }
    if (o[3] < q.tc) { q.tc = o[3]; q.jc = o[4]; }
    q.n += o[5];
  }
  double* s = summary + i * NFOPP_NUM_CONFLICT_SLOTS;
  if (bad) {
    for (int k = 0; k < NFOPP_CONFLICT_SLOT_STATUS; ++k) s[k] = qnan;
    s[NFOPP_CONFLICT_SLOT_STATUS] = (double)NFOPP_CONFLICT_BAD_TRACK;
    return;
  }
  s[NFOPP_CONFLICT_SLOT_MIN_GAP] = q.g;
  s[NFOPP_CONFLICT_SLOT_MIN_PARTNER] = q.j;
  s[NFOPP_CONFLICT_SLOT_MIN_TIME] = q.t;
  s[NFOPP_CONFLICT_SLOT_FIRST_TIME] = q.tc;
  s[NFOPP_CONFLICT_SLOT_FIRST_PARTNER] = q.jc;
  s[NFOPP_CONFLICT_SLOT_CONFLICTS] = q.n;
  s[NFOPP_CONFLICT_SLOT_STATUS] = q.j < 0.0 ? (double)NFOPP_CONFLICT_NO_PARTNER : 0.0;
}

static long long tc_tiles(long long n, int tile) { return n > 0 ? (n + tile - 1) / tile : 1; }

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_track_conflicts_workspace_bytes(int64_t ba, int64_t bb, int32_t k) {
  (void)k;
  if (ba <= 0 || bb < 0) return 0;
  const long long nta = tc_tiles(ba, TC_TILE_A), ntb = tc_tiles(bb, TC_TILE_B);
  // self mode (bb == 0): [ba, nta]; A against B: [ba, ntb] and [bb, nta]
  return (size_t)(ba * (bb > 0 ? ntb : nta) + bb * nta) * TC_PART * sizeof(double);
}

extern "C" int nfopp_track_conflicts(const float* tracks_a_dev, int64_t ba, int32_t stride_a, const float* tracks_b_dev,
                                     int64_t bb, int32_t stride_b, int32_t k, double t0, double dt, const float* radius_a_dev,
                                     const float* radius_b_dev, double margin, double* summary_dev, double* summary_b_dev,
                                     double* pair_gap_dev, double* pair_first_dev, void* workspace_dev, size_t workspace_bytes,
                                     void* stream) {
  const bool self = tracks_b_dev == nullptr;
  const double inf = (double)__builtin_inff();
  NFOPP_REQUIRE(ba >= 0 && ba <= 0x7fffffffLL && (self || (bb >= 0 && bb <= 0x7fffffffLL)), "bad batch size");
  NFOPP_REQUIRE(k >= 1, "a track needs at least one instant (k >= 1)");
  NFOPP_REQUIRE(stride_a >= 2 && (self || stride_b >= 2), "a track row holds x and y: stride must be >= 2");
  NFOPP_REQUIRE(dt > 0.0 && dt < inf, "dt must be positive and finite");
  NFOPP_REQUIRE(t0 == t0 && fabs(t0) < inf, "t0 must be finite");
  NFOPP_REQUIRE(margin == margin && fabs(margin) < inf, "margin must be finite");
  if (ba == 0) return NFOPP_OK;
  NFOPP_REQUIRE(tracks_a_dev && summary_dev, "null device pointer");
  ConflictArgs p;
  p.a = tracks_a_dev; p.b = self ? tracks_a_dev : tracks_b_dev;
  p.ra = radius_a_dev; p.rb = self ? radius_a_dev : radius_b_dev;
  p.ba = ba; p.bb = self ? ba : bb;
  p.stride_a = stride_a; p.stride_b = self ? stride_a : stride_b; p.k = k; p.self = self ? 1 : 0;
  p.t0 = t0; p.dt = dt; p.margin = margin;
  p.pair_gap = pair_gap_dev; p.pair_first = pair_first_dev;
  p.nta = tc_tiles(p.ba, TC_TILE_A); p.ntb = tc_tiles(p.bb, TC_TILE_B);
  const long long grid = self ? p.nta * (p.nta + 1) / 2 : p.nta * p.ntb;
  NFOPP_REQUIRE(grid <= 0x7fffffffLL, "too many track pairs for one call (%lld tiles)", grid);
  const bool want_b = !self && summary_b_dev && p.bb > 0;
  const size_t bytes_a = (size_t)(p.ba * p.ntb) * TC_PART * sizeof(double);
  const size_t bytes_b = want_b ? (size_t)(p.bb * p.nta) * TC_PART * sizeof(double) : 0;
  NFOPP_REQUIRE(workspace_dev && workspace_bytes >= bytes_a + bytes_b, "workspace too small or null (%zu bytes, %zu needed)",
                workspace_dev ? workspace_bytes : (size_t)0, bytes_a + bytes_b);
  p.part_a = reinterpret_cast<double*>(workspace_dev);
  p.part_b = want_b ? p.part_a + p.ba * p.ntb * TC_PART : nullptr;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(track_conflict_tile_kernel, dim3((unsigned)grid), dim3(TC_THREADS), 0, s, p);
  NFOPP_HIP(hipGetLastError());
  hipLaunchKernelGGL(track_conflict_reduce_kernel, dim3((unsigned)((p.ba + TC_THREADS - 1) / TC_THREADS)), dim3(TC_THREADS), 0, s,
                     (const double*)p.part_a, p.ba, p.ntb, summary_dev);
  NFOPP_HIP(hipGetLastError());
  if (want_b) {
    hipLaunchKernelGGL(track_conflict_reduce_kernel, dim3((unsigned)((p.bb + TC_THREADS - 1) / TC_THREADS)), dim3(TC_THREADS), 0, s,
                       (const double*)p.part_b, p.bb, p.nta, summary_b_dev);
    NFOPP_HIP(hipGetLastError());
  }
  return NFOPP_OK;
}
