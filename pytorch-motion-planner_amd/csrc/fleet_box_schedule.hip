// Shift masks of oriented boxes for the fleet scheduler: fleet_schedule.hip shifts the circumscribed discs of car-like robots,
// so two cars that pass in neighbouring lanes are delayed, or left unresolved, though box_conflict.hip calls them free.  This
// file writes the masks of nfopp_fleet_shift_masks' layout from the box check's pair rule; nfopp_fleet_assign_delays reads them
// unchanged.
//
//   * fleet_box_shape_kernel   one workgroup per robot / obstacle track: the shape row of box_pairs.h (box, reach, rounding
//                              radius, BAD flag) into the workspace; the robots' flags also into bad_dev
//   * fleet_box_mask_kernel    one workgroup per FS_TILE x FS_TILE tile of pairs; work items are (pair, relative shift); a window
//                              of both sides' poses (x, y, cos, sin as float64) staged in LDS per FB_CHUNK instants; the bits of
//                              a pair are collected by wave ballots (fleet_masks.h).  Self mode: tiles of the upper triangle,
//                              mirrored by a bit reversal.  Obstacle mode: robots x obstacles, per-tile ORs of every robot's bits
//   * fleet_box_base_kernel    one thread per robot: the OR of its obstacle tiles' partials
//
// The rule (restated in numpy in tests/fleet_box_schedule_ref.py from tests/box_conflict_ref.py and
// tests/fleet_schedule_ref.py; include/nfopp_hip.h repeats it for callers).  Tracks, delayed robots, masks, bad robots and
// obstacles are fleet_schedule.hip's; the pair predicate is another.
//  Tracks.  [B, K, stride >= 3] fp32, x, y, theta first in a row, with the unit vectors [B, K, 2] float64 of the headings pass.
//    Robot i delayed by q is at track_i[clamp(h - q, 0, K - 1)] at instant h; its unit vector is gathered with the same index.
//  Pair predicate C_ij(r), r = q_i - q_j: "the status of the pair is not NFOPP_BOX_PAIR_FREE" by box_conflict.hip's rule (the
//    given refine, margin, boxes and rounding radii) on robot i delayed by max(r, 0) and robot j delayed by max(-r, 0), over
//    K + |r| instants.  UNDECIDED counts as forbidden, so a schedule built from these masks is FREE by the box check.
//  Order of the boxes.  The box arithmetic is not even in the order of the boxes: only i < j is evaluated, with i as the first
//    box, for every r; mask_ji is mask_ij with its 2 * max_delay + 1 bits reversed -- a copy, as in the box check's self mode.
//  Obstacles.  [M, K + max_delay, stride >= 3] with their own unit vectors, boxes and radii, in absolute time, never shifted;
//    the robot is the first box and the obstacle the second, over all K + max_delay instants.
//  Bad.  The box check's rule: a non-finite x, y, unit vector, box entry or radius, x0 >= x1, y0 >= y1 or r < 0.  The
//    consequences are fleet_schedule.hip's.
//  Horizon.  In an interval where both robots stand still the poses at its two ends are the same.  Step 1 frees the pair when
//    |d|^2 >= D2.  Otherwise step 2 reads the sa that the neighbouring real interval (or the last-instant term) reads, and if
//    that is no conflict, step 3 is ((sa + sa) - 0) * 0.5 - R >= 0 with sa - R >= 0: sa + sa and its half are exact, so it is
//    FREE.  The waiting intervals in front and the parked intervals behind add neither a CONFLICT nor an UNDECIDED that the
//    pair does not have already: the bit depends on the two delays through their difference alone.
//
// An item stops at its first node that is not FREE (the bit is an OR); the last-instant term, the same for every shift, opens
// every item.  Predicates, integer ORs: no atomics, nothing depends on an order, two runs give the same bits.
#include "box_pairs.h"
#include "common.h"
#include "fleet_masks.h"
#include "track_pairs.h"

#pragma clang fp contract(off)

namespace nfopp {

constexpr int FB_CHUNK = 16;                                          // instants walked per trip
constexpr int FB_WINDOW = FB_CHUNK + NFOPP_SCHEDULE_MAX_DELAY + 1;    // staged per track and trip: the chunk, max_delay before it, one more for the start pose

struct BoxMaskArgs {
  const float* a; const float* b;        // robots; self mode: b == a, else the obstacles
  const double* ua; const double* ub;    // unit vectors [ba, k, 2], [bb, kb, 2]
  const double* shape_a; const double* shape_b;   // shape rows, written by fleet_box_shape_kernel on the same stream
  long long ba, bb;
  int stride_a, stride_b, k, kb;         // kb: instants of side B (self: k; obstacles: k + max_delay)
  int max_delay, self, refine;
  int ns_log2;                           // item index = pair << ns_log2 | shift index; 1 << ns_log2 >= the number of shifts
  double margin;
  unsigned long long* pair;              // self: [ba, ba, 2]
  unsigned long long* part;              // obstacles: [ba, ntb]
  long long nta, ntb;
};

// shape row of every track, one workgroup of 64 threads per track; flags (robots: bad_dev; obstacles: null) <- the BAD flag
__global__ __launch_bounds__(64) void fleet_box_shape_kernel(const float* tracks, const double* units, const float* box,
                                                             const float* radius, int stride, int k, double* shape, int* flags) {
  const long long g = blockIdx.x;
  const int bad = box_shape_row(tracks + g * (long long)k * stride, units + g * (long long)k * 2, box, radius, g, stride, k, shape);
  if (threadIdx.x == 0 && flags) flags[g] = bad ? 1 : 0;
}

__global__ __launch_bounds__(FS_THREADS) void fleet_box_mask_kernel(const BoxMaskArgs p) {
  __shared__ Pose2 sA[FS_TILE * FB_WINDOW], sB[FS_TILE * FB_WINDOW];   // [track][slot]
  __shared__ Pose2 sLast[2 * FS_TILE];                                 // both sides' last poses
  __shared__ double sShape[2 * FS_TILE][BC_SHAPE];                     // a track past the end of its side counts as bad
  __shared__ unsigned long long sMask[FS_PAIRS * 2];
  const int tid = threadIdx.x;

  long long ta, tb;
  if (p.self) upper_triangle_tile(blockIdx.x, p.nta, &ta, &tb);
  else pair_tile(blockIdx.x, p.ntb, &ta, &tb);
  const long long a0 = ta * FS_TILE, b0 = tb * FS_TILE;
  const long long row_a = (long long)p.k * p.stride_a, row_b = (long long)p.kb * p.stride_b;

  if (tid < 2 * FS_TILE * BC_SHAPE) {
    const int tr = tid / BC_SHAPE, f = tid % BC_SHAPE;
    const bool is_a = tr < FS_TILE;
    const long long g = is_a ? a0 + tr : b0 + (tr - FS_TILE);
    const bool in = g < (is_a ? p.ba : p.bb);
    sShape[tr][f] = in ? (is_a ? p.shape_a : p.shape_b)[g * BC_SHAPE + f] : (f == 6 ? 1.0 : 0.0);
  } else if (tid < 2 * FS_TILE * BC_SHAPE + 2 * FS_TILE) {
    const int tr = tid - 2 * FS_TILE * BC_SHAPE;
    const bool is_a = tr < FS_TILE;
    const long long g = is_a ? a0 + tr : b0 + (tr - FS_TILE);
    Pose2 v; v.x = v.y = v.c = v.s = 0.0;
    if (g < (is_a ? p.ba : p.bb)) {
      const int last = (is_a ? p.k : p.kb) - 1;
      const float* src = is_a ? p.a + g * row_a + (long long)last * p.stride_a : p.b + g * row_b + (long long)last * p.stride_b;
      const double* us = (is_a ? p.ua + g * (long long)p.k * 2 : p.ub + g * (long long)p.kb * 2) + (long long)last * 2;
      v.x = (double)src[0]; v.y = (double)src[1]; v.c = us[0]; v.s = us[1];
    }
    sLast[tr] = v;
  }
  static_assert(2 * FS_TILE * BC_SHAPE + 2 * FS_TILE <= FS_THREADS, "one thread per shape entry and per last pose");
  if (tid < FS_PAIRS * 2) sMask[tid] = 0ull;
  __syncthreads();

  const int ns = 1 << p.ns_log2, n_shift = p.self ? 2 * p.max_delay + 1 : p.max_delay + 1;
  const int n_items = FS_PAIRS << p.ns_log2;   // a multiple of 64: a wave is inside the item loops as a whole or not at all
  const bool diagonal = p.self && ta == tb;

  // the last-instant term is the same for every shift (both sides stand at their last samples): it opens every item's bit
  unsigned done = 0u, live = 0u;   // bit s: item tid + s * FS_THREADS is not FREE / is evaluated at all
  for (int s = 0, q = tid; q < n_items; ++s, q += FS_THREADS) {
    const int pair = q >> p.ns_log2, sidx = q & (ns - 1), li = pair >> 3, lj = pair & 7;
    const double* bi = sShape[li];
    const double* bj = sShape[FS_TILE + lj];
    const bool on = sidx < n_shift && bi[6] == 0.0 && bj[6] == 0.0 && (!diagonal || li < lj);
    if (!on) continue;
    live |= 1u << s;
    double R, R2;
    pair_radius(bi[5], bj[5], p.margin, &R, &R2);
    const double D = (bi[4] + bj[4]) + R, D2 = D * D;
    if (last_instant_conflict(sLast[li], sLast[FS_TILE + lj], bi, bj, R, D2)) done |= 1u << s;
  }

  const int h_all = p.k + p.max_delay;   // no item has an instant at or past this
  for (int h0 = 0; h0 < h_all; h0 += FB_CHUNK) {
    const int wbase = h0 - 1 - p.max_delay;   // slot w holds track[clamp(wbase + w)]: the clamp of a delayed robot is made here
    const int width = min(FB_CHUNK, h_all - h0) + p.max_delay + 1;
    __syncthreads();   // the previous trip's reads
    for (int idx = tid; idx < 2 * FS_TILE * FB_WINDOW; idx += FS_THREADS) {
      const int w = idx % FB_WINDOW, tr = idx / FB_WINDOW;
      if (w >= width) continue;
      const bool is_a = tr < FS_TILE;
      const int lt = is_a ? tr : tr - FS_TILE;
      const long long g = (is_a ? a0 : b0) + lt;
      Pose2 v; v.x = v.y = v.c = v.s = 0.0;
      if (g < (is_a ? p.ba : p.bb)) {
        const int kk = min(max(wbase + w, 0), (is_a ? p.k : p.kb) - 1);
        const float* src = is_a ? p.a + g * row_a + (long long)kk * p.stride_a : p.b + g * row_b + (long long)kk * p.stride_b;
        const double* us = (is_a ? p.ua + g * (long long)p.k * 2 : p.ub + g * (long long)p.kb * 2) + (long long)kk * 2;
        v.x = (double)src[0]; v.y = (double)src[1]; v.c = us[0]; v.s = us[1];
      }
      (is_a ? sA : sB)[lt * FB_WINDOW + w] = v;
    }
    __syncthreads();
    for (int s = 0, q = tid; q < n_items; ++s, q += FS_THREADS) {
      if (!((live & ~done) >> s & 1u)) continue;
      const int pair = q >> p.ns_log2, sidx = q & (ns - 1), li = pair >> 3, lj = pair & 7;
      const int r = p.self ? sidx - p.max_delay : sidx;
      const int da = r > 0 ? r : 0, db = r < 0 ? -r : 0;
      const int n_inst = p.self ? p.k + (r < 0 ? -r : r) : h_all;
      const int lo = h0 > 1 ? h0 : 1, hi = min(h0 + FB_CHUNK - 1, n_inst - 1);   // intervals h - 1 -> h of this trip
      if (lo > hi) continue;
      const double* bi = sShape[li];
      const double* bj = sShape[FS_TILE + lj];
      const double reach_i = bi[4], reach_j = bj[4];
      double R, R2;
      pair_radius(bi[5], bj[5], p.margin, &R, &R2);
      const double D = (reach_i + reach_j) + R, D2 = D * D;
      const Pose2* rowA = sA + li * FB_WINDOW + (lo - 1 - da - wbase);
      const Pose2* rowB = sB + lj * FB_WINDOW + (lo - 1 - db - wbase);
      bool hit = false;
      for (int n = 1; n <= hi - lo + 1 && !hit; ++n) {
        const Pose2 ia0 = rowA[n - 1], ja0 = rowB[n - 1], ib0 = rowA[n], jb0 = rowB[n];
        // an OR: the first node that is not FREE decides the bit
        walk_interval(ia0, ja0, ib0, jb0, bi, bj, reach_i, reach_j, R, D2, p.refine, [&](int, int, int) { hit = true; return true; });
      }
      if (hit) done |= 1u << s;
    }
  }

  collect_item_bits(done, n_items, p.ns_log2, sMask);
  __syncthreads();

  if (p.self) store_pair_masks(sMask, diagonal, a0, b0, p.ba, p.max_delay, p.pair);
  else store_obstacle_part(sMask, a0, p.ba, tb, p.ntb, p.part);
}

// base[i] <- the OR of robot i's obstacle partials (none: 0); 0 for a bad robot
__global__ __launch_bounds__(FS_THREADS) void fleet_box_base_kernel(const unsigned long long* part, const int* bad, long long n,
                                                                     long long n_tiles, unsigned long long* base) {
  base_from_parts(part, bad, n, n_tiles, base);
}

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_fleet_box_shift_masks_workspace_bytes(int64_t b, int64_t m, int32_t k, int32_t max_delay) {
  (void)k; (void)max_delay;
  if (b <= 0 || m < 0) return 0;
  // shape rows of the robots and the obstacles; one partial per robot and tile of obstacles
  return (size_t)((b + m) * BC_SHAPE + b * fs_tiles(m)) * sizeof(double);
}

extern "C" int nfopp_fleet_box_shift_masks(const float* tracks_dev, const double* heading_dev, int64_t b, int32_t stride, int32_t k,
                                           const float* box_dev, const float* radius_dev, double margin, int32_t refine,
                                           int32_t max_delay, const float* obstacles_dev, const double* obstacle_heading_dev,
                                           int64_t m, int32_t obstacle_stride, const float* obstacle_box_dev,
                                           const float* obstacle_radius_dev, uint64_t* pair_mask_dev, uint64_t* base_mask_dev,
                                           int32_t* bad_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  static_assert(sizeof(double) == sizeof(unsigned long long), "shape rows and partials share the workspace's unit");
  const double inf = (double)__builtin_inff();
  NFOPP_REQUIRE(b >= 0 && b <= 0x7fffffffLL && m >= 0 && m <= 0x7fffffffLL, "bad batch size");
  NFOPP_REQUIRE(max_delay >= 0 && max_delay <= NFOPP_SCHEDULE_MAX_DELAY, "max_delay must be in 0 .. %d", NFOPP_SCHEDULE_MAX_DELAY);
  NFOPP_REQUIRE(k >= 1, "a track needs at least one instant (k >= 1)");
  NFOPP_REQUIRE(k <= 0x7fffffff - 2 * (NFOPP_SCHEDULE_MAX_DELAY + 1) - FB_CHUNK, "too many instants for an index (k = %d)", k);
  NFOPP_REQUIRE(stride >= 3 && (m == 0 || !obstacles_dev || obstacle_stride >= 3),
                "a track row holds x, y and theta: stride must be >= 3");
  NFOPP_REQUIRE(refine >= 0 && refine <= BC_MAX_REFINE, "refine must be 0 .. %d, got %d", BC_MAX_REFINE, (int)refine);
  NFOPP_REQUIRE(margin == margin && fabs(margin) < inf, "margin must be finite");
  if (b == 0) return NFOPP_OK;
  if (!obstacles_dev) m = 0;   // no obstacles
  NFOPP_REQUIRE(tracks_dev && heading_dev && box_dev && pair_mask_dev && base_mask_dev && bad_dev, "null device pointer");
  NFOPP_REQUIRE(m == 0 || (obstacle_heading_dev && obstacle_box_dev), "null device pointer (obstacles)");
  BoxMaskArgs p;
  p.a = tracks_dev; p.ua = heading_dev; p.ba = b; p.stride_a = stride; p.k = k; p.max_delay = max_delay; p.refine = refine;
  p.margin = margin;
  p.nta = fs_tiles(b);
  const long long grid_self = p.nta * (p.nta + 1) / 2, ntm = fs_tiles(m);
  NFOPP_REQUIRE(grid_self <= 0x7fffffffLL && p.nta * ntm <= 0x7fffffffLL, "too many track pairs for one call (%lld tiles)",
                grid_self > p.nta * ntm ? grid_self : p.nta * ntm);
  const size_t need = nfopp_fleet_box_shift_masks_workspace_bytes(b, m, k, max_delay);
  NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small or null (%zu bytes, %zu needed)",
                workspace_dev ? workspace_bytes : (size_t)0, need);
  double* shape_a = reinterpret_cast<double*>(workspace_dev);
  double* shape_b = shape_a + b * BC_SHAPE;
  unsigned long long* part = reinterpret_cast<unsigned long long*>(shape_b + m * BC_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fleet_box_shape_kernel, dim3((unsigned)b), dim3(64), 0, s, tracks_dev, heading_dev, box_dev, radius_dev, (int)stride,
                     (int)k, shape_a, (int*)bad_dev);
  NFOPP_HIP(hipGetLastError());
  // the fleet against itself
  p.b = tracks_dev; p.ub = heading_dev; p.shape_a = shape_a; p.shape_b = shape_a; p.bb = b; p.stride_b = stride; p.kb = k; p.self = 1;
  p.ns_log2 = fs_log2_ceil(2 * max_delay + 1);
  p.pair = reinterpret_cast<unsigned long long*>(pair_mask_dev); p.part = nullptr; p.ntb = p.nta;
  hipLaunchKernelGGL(fleet_box_mask_kernel, dim3((unsigned)grid_self), dim3(FS_THREADS), 0, s, p);
  NFOPP_HIP(hipGetLastError());
  if (m > 0) {   // the fleet against the obstacles
    hipLaunchKernelGGL(fleet_box_shape_kernel, dim3((unsigned)m), dim3(64), 0, s, obstacles_dev, obstacle_heading_dev, obstacle_box_dev,
                       obstacle_radius_dev, (int)obstacle_stride, (int)(k + max_delay), shape_b, (int*)nullptr);
    NFOPP_HIP(hipGetLastError());
    p.b = obstacles_dev; p.ub = obstacle_heading_dev; p.shape_b = shape_b; p.bb = m; p.stride_b = obstacle_stride; p.kb = k + max_delay;
    p.self = 0;
    p.ns_log2 = fs_log2_ceil(max_delay + 1);
    p.pair = nullptr; p.part = part; p.ntb = ntm;
    hipLaunchKernelGGL(fleet_box_mask_kernel, dim3((unsigned)(p.nta * ntm)), dim3(FS_THREADS), 0, s, p);
    NFOPP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(fleet_box_base_kernel, dim3((unsigned)((b + FS_THREADS - 1) / FS_THREADS)), dim3(FS_THREADS), 0, s,
                     (const unsigned long long*)part, (const int*)bad_dev, (long long)b, m > 0 ? ntm : 0LL,
                     reinterpret_cast<unsigned long long*>(base_mask_dev));
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}
