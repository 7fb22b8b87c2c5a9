// Conflict detection between timed SE(2) tracks of oriented boxes: which car-like robots of a fleet touch, when first, and
// with whom -- where track_conflict.hip sees every robot as its circumscribed disc.  The rule is this library's own.
//
//   * track_heading_kernel       (cos, sin) of every heading, float64: the only transcendental step, a pass of its own
//   * box_shape_kernel           one workgroup per track: box, reach, rounding radius and the BAD flag into the workspace
//   * box_conflict_tile_kernel   one workgroup per BC_TILE x BC_TILE tile of pairs, BC_CHUNK intervals of both sides staged in
//                                LDS per trip, 4 pairs per thread; per-tile partials of every row (and column)
//   * box_conflict_reduce_kernel one thread per track: merges its tiles' partials in tile order
//
// THE RULE (restated in numpy in tests/box_conflict_ref.py; include/nfopp_hip.h repeats it for callers).  Float64 with every
// operation rounded on its own (contraction off); only +, -, *, /, sqrt and comparisons after the headings pass.
//  Tracks.  [B, K, stride >= 3] fp32 on the grid t_k = t0 + k * dt of track_pairs.h: x, y, theta first in a row.  Position is
//    linear in time between two instants; the heading turns the shorter way at a constant rate.  The pair kernel reads x, y
//    and the unit vectors u = (cos theta, sin theta) of the headings pass, never theta.
//  Shape of track i: box (x0, x1, y0, y1) in the body frame (fp32, widened), rounding radius r_i >= 0,
//    reach_i = fl32(fl32(sqrt(mx * mx + my * my)) * 1.000001f) with mx = max(|x0|, |x1|), my = max(|y0|, |y1|) widened to
//    float64 -- box_reach of point_cloud.h with hypotf written as the rounded float64 root.  R_ij, R2_ij = pair_radius(r_i,
//    r_j, margin);  D_ij = (reach_i + reach_j) + R_ij,  D2_ij = D_ij * D_ij.
//  BAD: a track with a non-finite x, y, unit vector, box entry or radius, with x0 >= x1 or y0 >= y1, or with r < 0.  It is
//    nobody's partner; its summary row is NaN with status NFOPP_CONFLICT_BAD_TRACK, its pair rows and columns are
//    NFOPP_BOX_PAIR_BAD / NaN (the diagonal entry included).
//  sep(P_i, P_j) at an instant, P = (p, u):  d = p_j - p_i;  cr = ci * cj + si * sj,  sr = ci * sj - si * cj;
//    xi = dx * ci + dy * si,  yi = dy * ci - dx * si;  xj = -(dx * cj + dy * sj),  yj = -(dy * cj - dx * sj);
//    gap(t, box, cx, cy, s0, s1):  a0 = box.x0 * cx, a1 = box.x1 * cx, b0 = box.y0 * cy, b1 = box.y1 * cy,
//      lo = (t + min(a0, a1)) + min(b0, b1),  hi = (t + max(a0, a1)) + max(b0, b1),  max(lo - s1, s0 - hi);
//    g1 = gap(xi, box_j, cr, -sr, x0_i, x1_i),  g2 = gap(yi, box_j, sr, cr, y0_i, y1_i),
//    g3 = gap(xj, box_i, cr, sr, x0_j, x1_j),   g4 = gap(yj, box_i, -sr, cr, y0_j, y1_j);  sep = max(max(g1, g2), max(g3, g4))
//    (max(a, b) = a > b ? a : b, min(a, b) = a < b ? a : b).  The largest gap over the four face axes: negative iff the open
//    boxes intersect, never more than the distance between the boxes.
//  A sub-interval [a, b] (an interval, or a dyadic part of one) with poses P_i, P_j at a and Q_i, Q_j at b, in this order:
//    1. d0 = p_i - p_j at a, d1 at b, c = |d0|^2, e = |d1|^2;  q = closest_approach(d0, c, d1, e).  q.m >= D2: FREE.
//    2. sa = sep at a;  sa - R < 0: CONFLICT at a.
//    3. sb = sep at b;  ni = sqrt(|Q_i.u - P_i.u|^2), nj likewise;  mot = sqrt(q.a) + H * (reach_i * ni + reach_j * nj) with
//       H the float64 next above pi / 2;  ((sa + sb) - mot) * 0.5 - R >= 0: FREE.
//    4. depth < refine and both li = sqrt(|P_i.u + Q_i.u|^2), lj != 0: split at the mid pose, p = (p_a + p_b) * 0.5,
//       u = (P.u + Q.u) / l;  the left half, then the right half.
//    5. otherwise UNDECIDED at a.
//  A pair: the intervals in time order, then the last instant (d = p_i - p_j at K - 1: unless |d|^2 >= D2, sep_{K-1} - R < 0 is a
//    CONFLICT; the whole check when K = 1).  The walk stops at the first CONFLICT; tc = its time, +inf if none;  tu = the time
//    of the first UNDECIDED met before, +inf if none.  The time of the node at depth d, position pos of interval k is
//    t_k + (pos / 2^d) * dt.  Status: CONFLICT when tc < inf, else UNDECIDED when tu < inf, else FREE.
//  Self mode evaluates i < j with i as the first box and copies the result to (j, i): the arithmetic is not even in the order
//    of the boxes; the matrices are symmetric because they are copied.
//  Summary row of track i over its good partners j: the lexicographic minima on (tc_ij, j) and on (tu_ij, j) -- the smaller j
//    wins a tie -- and the numbers of partners whose status is CONFLICT and UNDECIDED.
//
// The device functions of the rule -- sep, steps 1 .. 5, the walk of an interval's tree, the last-instant term, the shape row --
// live in box_pairs.h, which fleet_box_schedule.hip includes too; H above is box_pairs.h's BC_HALF_PI_UP = 0x1.921fb54442d19p+0;
//
// Loops: a pair visits at most 2^(refine + 1) - 1 nodes per interval, each found from the interval's end points in at most
// `refine` halvings (no stack, so no scratch).  Nothing waits on another workgroup; no atomics and no float sums.
#include "box_pairs.h"
#include "common.h"
#include "track_pairs.h"

#pragma clang fp contract(off)

namespace nfopp {

constexpr int BC_TILE = 32;       // tracks of a tile, on either side
constexpr int BC_CHUNK = 16;      // intervals staged per trip (BC_CHUNK + 1 instants)
constexpr int BC_THREADS = 256;   // 32 x 8 threads, 4 pairs each
constexpr int BC_PITCH = BC_TILE + 1;
constexpr int BC_PART = 7;        // doubles of a partial: tc, its partner, conflicts, tu, its partner, undecided, good partners (-1: bad)
static_assert(BC_TILE == 32 && BC_THREADS == 256, "the thread map below is 32 x 8 threads on 32 x 32 pairs");

struct BoxConflictArgs {
  const float* a; const float* b;            // b == a in self mode
  const double* ua; const double* ub;
  const double* shape_a; const double* shape_b;
  long long ba, bb;
  int stride_a, stride_b, k, self, refine;
  double t0, dt, margin;
  int* pair_status; double* pair_first; double* pair_undecided;
  double* part_a; double* part_b;            // [ba, ntb, BC_PART], [bb, nta, BC_PART] (self mode: part_a alone)
  long long nta, ntb;
};

// (cos, sin) of every heading: heading_dev [b, k, 2]
__global__ __launch_bounds__(BC_THREADS) void track_heading_kernel(const float* tracks, long long n, int stride, double* out) {
  const long long i = (long long)blockIdx.x * BC_THREADS + threadIdx.x;
  if (i >= n) return;
  const float th = tracks[i * stride + 2];
  const double qnan = (double)__builtin_nanf("");
  double c = qnan, s = qnan;
  if (finite32(th)) { c = cos((double)th); s = sin((double)th); }
  out[2 * i] = c; out[2 * i + 1] = s;
}

// shape row of every track: one workgroup of 64 threads per track
__global__ __launch_bounds__(64) void box_shape_kernel(const float* tracks, const double* units, const float* box, const float* radius,
                                                       int stride, int k, double* shape) {
  const long long g = blockIdx.x;
  box_shape_row(tracks + g * (long long)k * stride, units + g * (long long)k * 2, box, radius, g, stride, k, shape);
}

// (time, index) partial of one row over one tile's partners, in ascending partner order: strict < keeps the smaller index
struct BoxRowMin {
  double tc, jc, nc, tu, ju, nu, np;
  __device__ __forceinline__ void init() {
    tc = tu = (double)__builtin_inff(); jc = ju = -1.0; nc = nu = np = 0.0;
  }
  __device__ __forceinline__ void take(int st, double ptc, double ptu, double idx) {
    if (st < 0) return;   // not a partner: a bad track, the track itself, or past the end
    if (ptc < tc) { tc = ptc; jc = idx; }
    if (ptu < tu) { tu = ptu; ju = idx; }
    nc += st == NFOPP_BOX_PAIR_CONFLICT ? 1.0 : 0.0;     // counts of small integers: exact
    nu += st == NFOPP_BOX_PAIR_UNDECIDED ? 1.0 : 0.0;
    np += 1.0;
  }
  __device__ __forceinline__ void store(double* o, bool bad) const {
    o[0] = tc; o[1] = jc; o[2] = nc; o[3] = tu; o[4] = ju; o[5] = nu; o[6] = bad ? -1.0 : np;
  }
};

__global__ __launch_bounds__(BC_THREADS) void box_conflict_tile_kernel(const BoxConflictArgs p) {
  // staging: [BC_CHUNK + 1][2 * BC_TILE] poses; afterwards the result area: tc, tu [BC_TILE][BC_PITCH], status
  __shared__ __attribute__((aligned(16))) double bc_smem[(BC_CHUNK + 1) * 2 * BC_TILE * 4];
  __shared__ double sshape[2 * BC_TILE][BC_SHAPE];
  static_assert((2 * 8 + 4) * BC_TILE * BC_PITCH <= (int)sizeof(bc_smem), "the result area fits the staging area");
  Pose2* sP = reinterpret_cast<Pose2*>(bc_smem);
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const double inf = (double)__builtin_inff(), qnan = (double)__builtin_nanf("");

  long long ta, tb;
  if (p.self) upper_triangle_tile(blockIdx.x, p.nta, &ta, &tb);
  else pair_tile(blockIdx.x, p.ntb, &ta, &tb);
  const long long a0 = ta * BC_TILE, b0 = tb * BC_TILE;

  // shapes; a track past the end counts as bad
  for (int idx = tid; idx < 2 * BC_TILE * BC_SHAPE; idx += BC_THREADS) {
    const int tr = idx / BC_SHAPE, f = idx % BC_SHAPE;
    const bool is_a = tr < BC_TILE;
    const long long g = (is_a ? a0 : b0) + (is_a ? tr : tr - BC_TILE);
    const bool in = g < (is_a ? p.ba : p.bb);
    sshape[tr][f] = in ? (is_a ? p.shape_a : p.shape_b)[g * BC_SHAPE + f] : (f == 6 ? 1.0 : 0.0);
  }
  __syncthreads();

  // the pairs of this thread: (ty + 8 * q, tx), q = 0 .. 3
  double tc[4], tu[4];
  bool live[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int li = ty + 8 * q, lj = tx;
    const long long gi = a0 + li, gj = b0 + lj;
    tc[q] = inf; tu[q] = inf;
    live[q] = sshape[li][6] == 0.0 && sshape[BC_TILE + lj][6] == 0.0 && !(p.self && gi >= gj);
  }

  const long long row_a = (long long)p.k * p.stride_a, row_b = (long long)p.k * p.stride_b;
  for (long long k0 = 0; k0 == 0 || k0 < p.k - 1; k0 += BC_CHUNK) {
    const int n_int = (int)min((long long)BC_CHUNK, p.k - 1 - k0);    // intervals of this trip (0: K = 1, the last instant alone)
    const int n_inst = n_int + 1;
    __syncthreads();   // the previous trip's reads
    for (int idx = tid; idx < 2 * BC_TILE * (BC_CHUNK + 1); idx += BC_THREADS) {
      const int tr = idx % (2 * BC_TILE), kk = idx / (2 * BC_TILE);
      if (kk >= n_inst) continue;
      const bool is_a = tr < BC_TILE;
      const long long g = (is_a ? a0 : b0) + (is_a ? tr : tr - BC_TILE);
      Pose2 v; v.x = v.y = v.c = v.s = 0.0;
      if (g < (is_a ? p.ba : p.bb) && sshape[tr][6] == 0.0) {
        const long long inst = k0 + kk;
        const float* src = is_a ? p.a + g * row_a + inst * p.stride_a : p.b + g * row_b + inst * p.stride_b;
        const double* us = (is_a ? p.ua : p.ub) + (g * (long long)p.k + inst) * 2;
        v.x = (double)src[0]; v.y = (double)src[1]; v.c = us[0]; v.s = us[1];
      }
      sP[kk * 2 * BC_TILE + tr] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      if (!live[q] || tc[q] < inf) continue;
      const int li = ty + 8 * q, lj = tx;
      const double* bi = sshape[li];
      const double* bj = sshape[BC_TILE + lj];
      const double reach_i = bi[4], reach_j = bj[4];
      double R, R2;
      pair_radius(bi[5], bj[5], p.margin, &R, &R2);
      const double D = (reach_i + reach_j) + R, D2 = D * D;
      double ptc = inf, ptu = tu[q];
      for (int kk = 0; kk < n_int && !(ptc < inf); ++kk) {
        const Pose2 ia0 = sP[kk * 2 * BC_TILE + li], ja0 = sP[kk * 2 * BC_TILE + BC_TILE + lj];
        const Pose2 ib0 = sP[(kk + 1) * 2 * BC_TILE + li], jb0 = sP[(kk + 1) * 2 * BC_TILE + BC_TILE + lj];
        const double tk = p.t0 + (double)(k0 + kk) * p.dt;
        walk_interval(ia0, ja0, ib0, jb0, bi, bj, reach_i, reach_j, R, D2, p.refine, [&](int cls, int depth, int pos) {
          const double t = tk + ((double)pos / (double)(1 << depth)) * p.dt;
          if (cls == NODE_CONFLICT) { ptc = t; return true; }
          if (!(ptu < inf)) ptu = t;
          return false;
        });
      }
      if (k0 + n_int == p.k - 1 && !(ptc < inf)) {   // the last instant
        const Pose2 il = sP[n_int * 2 * BC_TILE + li], jl = sP[n_int * 2 * BC_TILE + BC_TILE + lj];
        if (last_instant_conflict(il, jl, bi, bj, R, D2)) ptc = (p.t0 + (double)(p.k - 1) * p.dt) + (0.0 / 1.0) * p.dt;
      }
      tc[q] = ptc; tu[q] = ptu;
    }
  }
  __syncthreads();   // the last trip's reads: the staging area becomes the result area

  double* resC = bc_smem;                           // [BC_TILE][BC_PITCH] first conflict
  double* resU = resC + BC_TILE * BC_PITCH;         // first undecided
  int* resS = reinterpret_cast<int*>(resU + BC_TILE * BC_PITCH);   // status, -1 = not a partner
  const bool mirror = p.self && ta != tb;
  const bool diagonal = p.self && ta == tb;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int li = ty + 8 * q, lj = tx;
    const long long gi = a0 + li, gj = b0 + lj;
    const bool inside = gi < p.ba && gj < p.bb;
    const bool bad = sshape[li][6] != 0.0 || sshape[BC_TILE + lj][6] != 0.0;
    const bool same = p.self && gi == gj;
    const int st = tc[q] < inf ? NFOPP_BOX_PAIR_CONFLICT : (tu[q] < inf ? NFOPP_BOX_PAIR_UNDECIDED : NFOPP_BOX_PAIR_FREE);
    const bool upper = !(p.self && gi > gj);        // the lower triangle of a diagonal tile is filled from the upper below
    if (upper) {
      const bool partner = inside && !bad && !same;
      resC[li * BC_PITCH + lj] = tc[q]; resU[li * BC_PITCH + lj] = tu[q]; resS[li * BC_PITCH + lj] = partner ? st : -1;
      if (diagonal && li != lj) {
        resC[lj * BC_PITCH + li] = tc[q]; resU[lj * BC_PITCH + li] = tu[q]; resS[lj * BC_PITCH + li] = partner ? st : -1;
      }
      if (inside) {
        const int os = bad ? NFOPP_BOX_PAIR_BAD : st;
        const double oc = bad ? qnan : tc[q], ou = bad ? qnan : tu[q];
        const bool both = (mirror || diagonal) && !same;
        if (p.pair_status) {
          p.pair_status[gi * p.bb + gj] = os;
          if (both) p.pair_status[gj * p.bb + gi] = os;
        }
        if (p.pair_first) {
          p.pair_first[gi * p.bb + gj] = oc;
          if (both) p.pair_first[gj * p.bb + gi] = oc;
        }
        if (p.pair_undecided) {
          p.pair_undecided[gi * p.bb + gj] = ou;
          if (both) p.pair_undecided[gj * p.bb + gi] = ou;
        }
      }
    }
  }
  __syncthreads();

  // per-tile partials: wave 0 takes the rows, wave 1 the columns
  if (tid < BC_TILE) {
    const long long gi = a0 + tid;
    if (gi < p.ba) {
      BoxRowMin m; m.init();
      for (int lj = 0; lj < BC_TILE; ++lj)
        m.take(resS[tid * BC_PITCH + lj], resC[tid * BC_PITCH + lj], resU[tid * BC_PITCH + lj], (double)(b0 + lj));
      m.store(p.part_a + (gi * p.ntb + tb) * BC_PART, sshape[tid][6] != 0.0);
    }
  } else if (tid >= 64 && tid < 64 + BC_TILE) {
    const int lj = tid - 64;
    const long long gj = b0 + lj;
    double* part = p.self ? (mirror ? p.part_a : nullptr) : p.part_b;
    if (part && gj < p.bb) {
      BoxRowMin m; m.init();
      for (int li = 0; li < BC_TILE; ++li)
        m.take(resS[li * BC_PITCH + lj], resC[li * BC_PITCH + lj], resU[li * BC_PITCH + lj], (double)(a0 + li));
      m.store(part + (gj * p.nta + ta) * BC_PART, sshape[BC_TILE + lj][6] != 0.0);   // self mode: the row of track gj, tile column ta
    }
  }
}

// summary [n_tracks, NFOPP_NUM_BOX_CONFLICT_SLOTS] from part [n_tracks, n_tiles, BC_PART], tiles in ascending partner order
__global__ __launch_bounds__(BC_THREADS) void box_conflict_reduce_kernel(const double* part, long long n_tracks, long long n_tiles,
                                                                         double* summary) {
  const long long i = (long long)blockIdx.x * BC_THREADS + threadIdx.x;
  if (i >= n_tracks) return;
  BoxRowMin m; m.init();
  bool bad = false;
  const double* row = part + i * n_tiles * BC_PART;
  for (long long t = 0; t < n_tiles; ++t) {
    const double* o = row + t * BC_PART;
    if (o[6] < 0.0) { bad = true; continue; }
    if (o[0] < m.tc) { m.tc = o[0]; m.jc = o[1]; }
    if (o[3] < m.tu) { m.tu = o[3]; m.ju = o[4]; }
    m.nc += o[2]; m.nu += o[5]; m.np += o[6];
  }
  double* s = summary + i * NFOPP_NUM_BOX_CONFLICT_SLOTS;
  if (bad) {
    for (int k = 0; k < NFOPP_BOX_CONFLICT_SLOT_STATUS; ++k) s[k] = (double)__builtin_nanf("");
    s[NFOPP_BOX_CONFLICT_SLOT_STATUS] = (double)NFOPP_CONFLICT_BAD_TRACK;
    return;
  }
  s[NFOPP_BOX_CONFLICT_SLOT_FIRST_TIME] = m.tc;
  s[NFOPP_BOX_CONFLICT_SLOT_FIRST_PARTNER] = m.jc;
  s[NFOPP_BOX_CONFLICT_SLOT_CONFLICTS] = m.nc;
  s[NFOPP_BOX_CONFLICT_SLOT_UNDECIDED_TIME] = m.tu;
  s[NFOPP_BOX_CONFLICT_SLOT_UNDECIDED_PARTNER] = m.ju;
  s[NFOPP_BOX_CONFLICT_SLOT_UNDECIDED] = m.nu;
  s[NFOPP_BOX_CONFLICT_SLOT_STATUS] = m.np > 0.0 ? 0.0 : (double)NFOPP_CONFLICT_NO_PARTNER;
}

static long long bc_tiles(long long n) { return n > 0 ? (n + BC_TILE - 1) / BC_TILE : 1; }

}  // namespace nfopp

using namespace nfopp;

extern "C" int nfopp_track_headings(const float* tracks_dev, int64_t batch, int32_t stride, int32_t k, double* heading_dev,
                                    void* stream) {
  NFOPP_REQUIRE(batch >= 0 && batch <= 0x7fffffffLL, "bad batch size");
  NFOPP_REQUIRE(k >= 1, "a track needs at least one instant (k >= 1)");
  NFOPP_REQUIRE(stride >= 3, "a track row holds x, y and theta: stride must be >= 3");
  if (batch == 0) return NFOPP_OK;
  NFOPP_REQUIRE(tracks_dev && heading_dev, "null device pointer");
  const long long n = (long long)batch * k;
  const long long grid = (n + BC_THREADS - 1) / BC_THREADS;
  NFOPP_REQUIRE(grid <= 0x7fffffffLL, "too many instants for one call (%lld)", n);
  hipLaunchKernelGGL(track_heading_kernel, dim3((unsigned)grid), dim3(BC_THREADS), 0, (hipStream_t)stream, tracks_dev, n, (int)stride,
                     heading_dev);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" size_t nfopp_box_track_conflicts_workspace_bytes(int64_t ba, int64_t bb, int32_t k) {
  (void)k;
  if (ba <= 0 || bb < 0) return 0;
  const long long nta = bc_tiles(ba), ntb = bc_tiles(bb);
  // shape rows of both sides; partials: self mode (bb == 0) [ba, nta]; A against B [ba, ntb] and [bb, nta]
  return (size_t)((ba + bb) * BC_SHAPE + (ba * (bb > 0 ? ntb : nta) + bb * nta) * BC_PART) * sizeof(double);
}

extern "C" int nfopp_box_track_conflicts(const float* tracks_a_dev, const double* heading_a_dev, int64_t ba, int32_t stride_a,
                                         const float* tracks_b_dev, const double* heading_b_dev, int64_t bb, int32_t stride_b,
                                         int32_t k, double t0, double dt, const float* box_a_dev, const float* box_b_dev,
                                         const float* radius_a_dev, const float* radius_b_dev, double margin, int32_t refine,
                                         double* summary_dev, double* summary_b_dev, int32_t* pair_status_dev,
                                         double* pair_first_dev, double* pair_undecided_dev, void* workspace_dev,
                                         size_t workspace_bytes, void* stream) {
  const bool self = tracks_b_dev == nullptr;
  const double inf = (double)__builtin_inff();
  NFOPP_REQUIRE(ba >= 0 && ba <= 0x7fffffffLL && (self || (bb >= 0 && bb <= 0x7fffffffLL)), "bad batch size");
  NFOPP_REQUIRE(k >= 1, "a track needs at least one instant (k >= 1)");
  NFOPP_REQUIRE(stride_a >= 3 && (self || stride_b >= 3), "a track row holds x, y and theta: stride must be >= 3");
  NFOPP_REQUIRE(refine >= 0 && refine <= BC_MAX_REFINE, "refine must be 0 .. %d, got %d", BC_MAX_REFINE, (int)refine);
  NFOPP_REQUIRE(dt > 0.0 && dt < inf, "dt must be positive and finite");
  NFOPP_REQUIRE(t0 == t0 && fabs(t0) < inf, "t0 must be finite");
  NFOPP_REQUIRE(margin == margin && fabs(margin) < inf, "margin must be finite");
  if (ba == 0) return NFOPP_OK;
  NFOPP_REQUIRE(tracks_a_dev && heading_a_dev && box_a_dev && summary_dev, "null device pointer");
  const long long nb = self ? ba : bb;
  NFOPP_REQUIRE(self || nb == 0 || (heading_b_dev && box_b_dev), "null device pointer (set B)");
  BoxConflictArgs p;
  p.a = tracks_a_dev; p.b = self ? tracks_a_dev : tracks_b_dev;
  p.ua = heading_a_dev; p.ub = self ? heading_a_dev : heading_b_dev;
  p.ba = ba; p.bb = nb;
  p.stride_a = stride_a; p.stride_b = self ? stride_a : stride_b; p.k = k; p.self = self ? 1 : 0; p.refine = refine;
  p.t0 = t0; p.dt = dt; p.margin = margin;
  p.pair_status = pair_status_dev; p.pair_first = pair_first_dev; p.pair_undecided = pair_undecided_dev;
  p.nta = bc_tiles(p.ba); p.ntb = bc_tiles(p.bb);
  const long long grid = self ? p.nta * (p.nta + 1) / 2 : p.nta * p.ntb;
  NFOPP_REQUIRE(grid <= 0x7fffffffLL, "too many track pairs for one call (%lld tiles)", grid);
  const bool want_b = !self && summary_b_dev && p.bb > 0;
  const size_t bytes_shape = (size_t)(p.ba + (self ? 0 : p.bb)) * BC_SHAPE * sizeof(double);
  const size_t bytes_a = (size_t)(p.ba * p.ntb) * BC_PART * sizeof(double);
  const size_t bytes_b = want_b ? (size_t)(p.bb * p.nta) * BC_PART * sizeof(double) : 0;
  const size_t need = bytes_shape + bytes_a + bytes_b;
  NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small or null (%zu bytes, %zu needed)",
                workspace_dev ? workspace_bytes : (size_t)0, need);
  double* shape_a = reinterpret_cast<double*>(workspace_dev);
  double* shape_b = self ? shape_a : shape_a + p.ba * BC_SHAPE;
  p.shape_a = shape_a; p.shape_b = shape_b;
  p.part_a = shape_a + (p.ba + (self ? 0 : p.bb)) * BC_SHAPE;
  p.part_b = want_b ? p.part_a + p.ba * p.ntb * BC_PART : nullptr;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(box_shape_kernel, dim3((unsigned)p.ba), dim3(64), 0, s, p.a, p.ua, box_a_dev, radius_a_dev, (int)p.stride_a, (int)k,
                     shape_a);
  NFOPP_HIP(hipGetLastError());
  if (!self && p.bb > 0) {
    hipLaunchKernelGGL(box_shape_kernel, dim3((unsigned)p.bb), dim3(64), 0, s, p.b, p.ub, box_b_dev, radius_b_dev, (int)p.stride_b, (int)k,
                       shape_b);
    NFOPP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(box_conflict_tile_kernel, dim3((unsigned)grid), dim3(BC_THREADS), 0, s, p);
  NFOPP_HIP(hipGetLastError());
  hipLaunchKernelGGL(box_conflict_reduce_kernel, dim3((unsigned)((p.ba + BC_THREADS - 1) / BC_THREADS)), dim3(BC_THREADS), 0, s,
                     (const double*)p.part_a, p.ba, p.ntb, summary_dev);
  NFOPP_HIP(hipGetLastError());
  if (want_b) {
    hipLaunchKernelGGL(box_conflict_reduce_kernel, dim3((unsigned)((p.bb + BC_THREADS - 1) / BC_THREADS)), dim3(BC_THREADS), 0, s,
                       (const double*)p.part_b, p.bb, p.nta, summary_b_dev);
    NFOPP_HIP(hipGetLastError());
  }
  return NFOPP_OK;
}
