// Prioritised start-delay scheduling of a fleet: every robot keeps its path and only WHEN it leaves changes.  In priority order
// each robot takes the smallest start delay, in steps of the common time grid, that keeps it clear of every robot scheduled
// before it and of every predicted obstacle.  track_conflict.hip answers "who is in conflict"; this file is the outer step that
// turns the answer into a fleet that can drive.  The rule is this library's own (the reference plans one robot).
//
//   * fleet_bad_kernel           one wave per robot / obstacle track: the bad flags
//   * fleet_shift_mask_kernel    one workgroup per FS_TILE x FS_TILE tile of pairs; work items are (pair, relative shift); a
//                                window of both sides' tracks staged in LDS per FS_CHUNK instants; the bits of a pair are
//                                collected by wave ballots.  Self mode: tiles of the upper triangle, mirrored by a bit reversal.
//                                Obstacle mode: robots x obstacles, per-tile ORs of every robot's bits.  The write-out is
//                                fleet_masks.h's, which fleet_box_schedule.hip shares
//   * fleet_base_kernel          one thread per robot: the OR of its obstacle tiles' partials
//   * fleet_assign_kernel        ONE workgroup: the sequential pass over the priority order, ORs and a count-trailing-zeros
//
// The rule (restated in numpy in tests/fleet_schedule_ref.py; include/nfopp_hip.h repeats it for callers).
//  Tracks.  B robot tracks [B, K, stride >= 2] fp32 on a common grid (x, y the first two floats of a row), D = max_delay + 1
//    candidate delays 0 .. max_delay grid steps, 0 <= max_delay <= 63.
//  A delayed robot.  Robot i delayed by q is at track_i[clamp(h - q, 0, K - 1)] at instant h: it waits at its first sample and
//    stays parked at its last.
//  Pair predicate C_ij(r), r = q_i - q_j in [-max_delay, max_delay]: the conflict predicate of track_conflict.hip -- some
//    m_k < R2_ij (strict), over the intervals k = 0 .. n - 2 and the last-instant term m = |d_{n-1}|^2, the predicate of
//    track_pairs.h, R_ij = (r_i + r_j) + margin, R2_ij = R_ij * R_ij -- on robot i delayed by max(r, 0) and robot j delayed by
//    max(-r, 0), over n = K + |r| instants.  Later instants add nothing: both robots are parked there, every further interval has
//    a == 0 and m = c = the last-instant term.  So the predicate does not depend on a horizon.  One of the two robots is never
//    delayed: the assignment uses bit d - q_j for robot i at delay d against robot j at delay q_j, and in absolute time that
//    pair only has min(d, q_j) more intervals in front, in which both wait (a == 0, m = c = |d_0|^2, the c interval 0 starts from).
//    Every quantity is even in the sign of d (track_conflict.hip), so C_ji(-r) has the same bit as C_ij(r).
//  Pair mask.  128 bits, two little-endian uint64 words: bit r + max_delay is C_ij(r); unused high bits 0.  The diagonal is 0; a
//    pair with a bad robot is 0.  mask_ji is mask_ij with its 2 * max_delay + 1 bits reversed.
//  Obstacles (optional).  M tracks [M, K + max_delay, stride >= 2] with radii, in absolute time, never shifted.  Bit d of base_i:
//    the same predicate on robot i delayed by d against obstacle j over all K + max_delay instants, ORed over the good obstacles.
//  Bad.  A robot or obstacle with a non-finite coordinate or radius is bad.  A bad obstacle is skipped by everyone; a bad robot
//    gets NFOPP_SCHEDULE_BAD_TRACK, delay -1, base 0, and is invisible to the others.
//  Assignment.  order [B] int32 (null: 0 .. B - 1), visited front to back; an entry out of range or a robot already visited is
//    skipped; a robot never visited ends with NFOPP_SCHEDULE_NOT_ORDERED, delay -1, forbidden 0.  For robot i
//      forbidden_i = (base_i | OR over the robots j scheduled before it of (mask_ij >> (max_delay - q_j))) & (2^D - 1)
//    (bit d of the shifted mask is C_ij(d - q_j)); q_i = the lowest clear bit, status 0.  No clear bit: status
//    NFOPP_SCHEDULE_UNRESOLVED, delay -1, and the robot is NOT on the floor for those after it.
//
// Predicates, integer ORs and a count-trailing-zeros: no atomics, nothing depends on an order, two runs give the same bits.
#include "block_collectives.h"
#include "common.h"
#include "fleet_masks.h"
#include "track_pairs.h"

#pragma clang fp contract(off)

namespace nfopp {

constexpr int FS_CHUNK = 64;                                 // instants walked per trip
constexpr int FS_WINDOW = FS_CHUNK + NFOPP_SCHEDULE_MAX_DELAY + 1;   // staged per track and trip: the chunk, max_delay before it, one more for d0
constexpr int FS_ASSIGN_THREADS = 256;
constexpr int FS_ASSIGN_WAVES = FS_ASSIGN_THREADS / 64;
constexpr int FS_ASSIGN_HEAD = 64;                           // bytes in front of the state array: the reduction's scratch
static_assert((FS_WINDOW & (FS_WINDOW - 1)) == 0, "the staging loop splits its index by a mask");
static_assert(FS_ASSIGN_WAVES * 8 <= FS_ASSIGN_HEAD, "the reduction's scratch fits its head");

struct ShiftMaskArgs {
  const float* a; const float* b;        // robots; self mode: b == a, else the obstacles
  const float* ra; const float* rb;
  const int* bad_a; const int* bad_b;    // written by fleet_bad_kernel on the same stream
  long long ba, bb;
  int stride_a, stride_b, k, kb;         // kb: instants of side B (self: k; obstacles: k + max_delay)
  int max_delay, self;
  int ns_log2;                           // item index = pair << ns_log2 | shift index; 1 << ns_log2 >= the number of shifts
  double margin;
  unsigned long long* pair;              // self: [ba, ba, 2]
  unsigned long long* part;              // obstacles: [ba, ntb]
  long long nta, ntb;
};

// flags[t] <- 1 when track t has a non-finite x or y at any instant, or a non-finite radius; one wave per track
__global__ __launch_bounds__(FS_THREADS) void fleet_bad_kernel(const float* tracks, const float* radius, long long n, int k, int stride,
                                                                int* flags) {
  const long long t = (long long)blockIdx.x * (FS_THREADS / 64) + (threadIdx.x >> 6);
  if (t >= n) return;   // a whole wave
  const int lane = threadIdx.x & 63;
  const float* row = tracks + t * (long long)k * stride;
  bool bad = false;
  for (int h = lane; h < k; h += 64) {
    const float* s = row + (long long)h * stride;
    bad |= !(finite32(s[0]) && finite32(s[1]));
  }
  const bool any = __ballot(bad) != 0ull;
  if (lane == 0) flags[t] = (any || (radius && !finite32(radius[t]))) ? 1 : 0;
}

__global__ __launch_bounds__(FS_THREADS) void fleet_shift_mask_kernel(const ShiftMaskArgs p) {
  __shared__ float2 sA[FS_TILE * FS_WINDOW], sB[FS_TILE * FS_WINDOW];   // [track][slot]
  __shared__ float2 sLast[2 * FS_TILE];                                 // both sides' last samples
  __shared__ double sRad[2 * FS_TILE];
  __shared__ int sBad[2 * FS_TILE];                                     // bad, or past the end of its side
  __shared__ unsigned long long sMask[FS_PAIRS * 2];
  const int tid = threadIdx.x;

  long long ta, tb;
  if (p.self) upper_triangle_tile(blockIdx.x, p.nta, &ta, &tb);
  else pair_tile(blockIdx.x, p.ntb, &ta, &tb);
  const long long a0 = ta * FS_TILE, b0 = tb * FS_TILE;
  const long long row_a = (long long)p.k * p.stride_a, row_b = (long long)p.kb * p.stride_b;

  if (tid < 2 * FS_TILE) {
    const bool is_a = tid < FS_TILE;
    const long long g = is_a ? a0 + tid : b0 + (tid - FS_TILE);
    const bool in = g < (is_a ? p.ba : p.bb);
    const float* rad = is_a ? p.ra : p.rb;
    sRad[tid] = (rad && in) ? (double)rad[g] : 0.0;
    sBad[tid] = in ? (is_a ? p.bad_a : p.bad_b)[g] : 1;
    float2 v = make_float2(0.f, 0.f);
    if (in) {
      const float* src = is_a ? p.a + g * row_a + (long long)(p.k - 1) * p.stride_a : p.b + g * row_b + (long long)(p.kb - 1) * p.stride_b;
      v.x = src[0]; v.y = src[1];
    }
    sLast[tid] = v;
  }
  if (tid < FS_PAIRS * 2) sMask[tid] = 0ull;
  __syncthreads();

  const int ns = 1 << p.ns_log2, n_shift = p.self ? 2 * p.max_delay + 1 : p.max_delay + 1;
  const int n_items = FS_PAIRS << p.ns_log2;   // a multiple of 64: a wave is inside the item loops as a whole or not at all
  const bool diagonal = p.self && ta == tb;

  // the last-instant term is the same for every shift (both sides stand at their last samples): it opens every item's bit
  unsigned done = 0u, live = 0u;   // bit s: item tid + s * FS_THREADS is in conflict / is evaluated at all
  for (int s = 0, q = tid; q < n_items; ++s, q += FS_THREADS) {
    const int pair = q >> p.ns_log2, sidx = q & (ns - 1), li = pair >> 3, lj = pair & 7;
    const bool on = sidx < n_shift && !sBad[li] && !sBad[FS_TILE + lj] && (!diagonal || li < lj);
    if (!on) continue;
    live |= 1u << s;
    double R, R2;
    pair_radius(sRad[li], sRad[FS_TILE + lj], p.margin, &R, &R2);
    const double x = (double)sLast[li].x - (double)sLast[FS_TILE + lj].x, y = (double)sLast[li].y - (double)sLast[FS_TILE + lj].y;
    const double m = x * x + y * y;
    if (m < R2) done |= 1u << s;
  }

  const int h_all = p.k + p.max_delay;   // no item has an instant at or past this
  for (int h0 = 0; h0 < h_all; h0 += FS_CHUNK) {
    const int wbase = h0 - 1 - p.max_delay;   // slot w holds track[clamp(wbase + w)]: the clamp of a delayed robot is made here
    const int width = min(FS_CHUNK, h_all - h0) + p.max_delay + 1;
    __syncthreads();   // the previous trip's reads
    for (int idx = tid; idx < 2 * FS_TILE * FS_WINDOW; idx += FS_THREADS) {
      const int w = idx & (FS_WINDOW - 1), tr = idx / FS_WINDOW;
      if (w >= width) continue;
      const bool is_a = tr < FS_TILE;
      const int lt = is_a ? tr : tr - FS_TILE;
      const long long g = (is_a ? a0 : b0) + lt;
      float2 v = make_float2(0.f, 0.f);
      if (g < (is_a ? p.ba : p.bb)) {
        const int kk = min(max(wbase + w, 0), (is_a ? p.k : p.kb) - 1);
        const float* src = is_a ? p.a + g * row_a + (long long)kk * p.stride_a : p.b + g * row_b + (long long)kk * p.stride_b;
        v.x = src[0]; v.y = src[1];
      }
      (is_a ? sA : sB)[lt * FS_WINDOW + w] = v;
    }
    __syncthreads();
    for (int s = 0, q = tid; q < n_items; ++s, q += FS_THREADS) {
      if (!((live & ~done) >> s & 1u)) continue;
      const int pair = q >> p.ns_log2, sidx = q & (ns - 1), li = pair >> 3, lj = pair & 7;
      const int r = p.self ? sidx - p.max_delay : sidx;
      const int da = r > 0 ? r : 0, db = r < 0 ? -r : 0;
      const int n_inst = p.self ? p.k + (r < 0 ? -r : r) : h_all;
      const int lo = h0 > 1 ? h0 : 1, hi = min(h0 + FS_CHUNK - 1, n_inst - 1);   // intervals h - 1 -> h of this trip
      if (lo > hi) continue;
      double R, R2;
      pair_radius(sRad[li], sRad[FS_TILE + lj], p.margin, &R, &R2);
      const float2* rowA = sA + li * FS_WINDOW + (lo - 1 - da - wbase);
      const float2* rowB = sB + lj * FS_WINDOW + (lo - 1 - db - wbase);
      float2 pa = rowA[0], pb = rowB[0];
      double x0 = (double)pa.x - (double)pb.x, y0 = (double)pa.y - (double)pb.y;
      double cc = x0 * x0 + y0 * y0;
      bool hit = false;
      for (int n = 1; n <= hi - lo + 1; ++n) {
        pa = rowA[n]; pb = rowB[n];
        const double d1x = (double)pa.x - (double)pb.x, d1y = (double)pa.y - (double)pb.y;
        const double e = d1x * d1x + d1y * d1y;
        const double m = closest_approach(x0, y0, cc, d1x, d1y, e).m;
        if (m < R2) { hit = true; break; }   // an OR: the remaining intervals cannot change the bit
        x0 = d1x; y0 = d1y; cc = e;          // d1 of this interval is d0 of the next
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
__global__ __launch_bounds__(FS_THREADS) void fleet_base_kernel(const unsigned long long* part, const int* bad, long long n, long long n_tiles,
                                                                 unsigned long long* base) {
  base_from_parts(part, bad, n, n_tiles, base);
}

struct AssignArgs {
  const unsigned long long* pair; const unsigned long long* base;
  const int* bad; const int* order;
  long long b;
  int max_delay;
  int* delay; int* status; unsigned long long* forbidden;
};

// One workgroup.  state[j]: -2 not visited yet, -1 visited and not on the floor (bad or unresolved), >= 0 its delay.
__global__ __launch_bounds__(FS_ASSIGN_THREADS) void fleet_assign_kernel(const AssignArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fs_assign_smem[];
  unsigned long long* red = reinterpret_cast<unsigned long long*>(fs_assign_smem);
  signed char* state = reinterpret_cast<signed char*>(fs_assign_smem + FS_ASSIGN_HEAD);
  const int tid = threadIdx.x;
  const int D = p.max_delay + 1;
  const unsigned long long low = D >= 64 ? ~0ull : ((1ull << D) - 1ull);
  for (long long j = tid; j < p.b; j += FS_ASSIGN_THREADS) state[j] = -2;
  __syncthreads();
  for (long long pos = 0; pos < p.b; ++pos) {
    // everything up to the reduction is the same in every thread: one global word, one LDS byte
    const long long i = p.order ? (long long)p.order[pos] : pos;
    if (i < 0 || i >= p.b) continue;
    if (state[i] != -2) continue;
    if (p.bad[i]) {
      __syncthreads();   // every thread has read state[i]
      if (tid == 0) {
        state[i] = -1; p.delay[i] = -1; p.status[i] = NFOPP_SCHEDULE_BAD_TRACK;
        if (p.forbidden) p.forbidden[i] = 0ull;
      }
      __syncthreads();
      continue;
    }
    unsigned long long acc = 0ull;
    const unsigned long long* row = p.pair + i * p.b * 2;
    for (long long j = tid; j < p.b; j += FS_ASSIGN_THREADS) {
      const int q = state[j];
      if (q < 0) continue;
      const unsigned long long lo = row[j * 2], hi = row[j * 2 + 1];
      const int s = p.max_delay - q;   // 0 .. 63; bit d of the shifted mask is C_ij(d - q)
      acc |= s ? (lo >> s) | (hi << (64 - s)) : lo;
    }
    acc = block_reduce<FS_ASSIGN_WAVES>(acc, 0ull, BitOr(), red);
    const unsigned long long forbidden = (acc | p.base[i]) & low, open = ~forbidden & low;
    if (tid == 0) {
      const int q = open ? (int)__builtin_ctzll(open) : -1;
      state[i] = (signed char)q;
      p.delay[i] = q;
      p.status[i] = open ? 0 : NFOPP_SCHEDULE_UNRESOLVED;
      if (p.forbidden) p.forbidden[i] = forbidden;
    }
    __syncthreads();
  }
  for (long long j = tid; j < p.b; j += FS_ASSIGN_THREADS)
    if (state[j] == -2) {
      p.delay[j] = -1; p.status[j] = NFOPP_SCHEDULE_NOT_ORDERED;
      if (p.forbidden) p.forbidden[j] = 0ull;
    }
}

static size_t fs_flag_bytes(long long m) { return (size_t)((m + 1) / 2 * 2) * sizeof(int); }

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_fleet_shift_masks_workspace_bytes(int64_t b, int64_t m) {
  if (b <= 0 || m <= 0) return 0;
  return (size_t)(b * fs_tiles(m)) * sizeof(unsigned long long) + fs_flag_bytes(m);
}

extern "C" int nfopp_fleet_shift_masks(const float* tracks_dev, int64_t b, int32_t stride, int32_t k, const float* radius_dev,
                                       double margin, int32_t max_delay, const float* obstacles_dev, int64_t m,
                                       int32_t obstacle_stride, const float* obstacle_radius_dev, uint64_t* pair_mask_dev,
                                       uint64_t* base_mask_dev, int32_t* bad_dev, void* workspace_dev, size_t workspace_bytes,
                                       void* stream) {
  const double inf = (double)__builtin_inff();
  NFOPP_REQUIRE(b >= 0 && b <= 0x7fffffffLL && m >= 0 && m <= 0x7fffffffLL, "bad batch size");
  NFOPP_REQUIRE(max_delay >= 0 && max_delay <= NFOPP_SCHEDULE_MAX_DELAY, "max_delay must be in 0 .. %d", NFOPP_SCHEDULE_MAX_DELAY);
  NFOPP_REQUIRE(k >= 1, "a track needs at least one instant (k >= 1)");
  NFOPP_REQUIRE(k <= 0x7fffffff - 2 * (NFOPP_SCHEDULE_MAX_DELAY + 1) - FS_CHUNK, "too many instants for an index (k = %d)", k);
  NFOPP_REQUIRE(stride >= 2 && (m == 0 || !obstacles_dev || obstacle_stride >= 2), "a track row holds x and y: stride must be >= 2");
  NFOPP_REQUIRE(margin == margin && fabs(margin) < inf, "margin must be finite");
  if (b == 0) return NFOPP_OK;
  if (!obstacles_dev) m = 0;   // no obstacles
  NFOPP_REQUIRE(tracks_dev && pair_mask_dev && base_mask_dev && bad_dev, "null device pointer");
  ShiftMaskArgs p;
  p.a = tracks_dev; p.ra = radius_dev; p.ba = b; p.stride_a = stride; p.k = k; p.max_delay = max_delay; p.margin = margin;
  p.bad_a = bad_dev;
  p.nta = fs_tiles(b);
  const long long grid_self = p.nta * (p.nta + 1) / 2, ntm = fs_tiles(m);
  NFOPP_REQUIRE(grid_self <= 0x7fffffffLL && p.nta * ntm <= 0x7fffffffLL, "too many track pairs for one call (%lld tiles)",
                grid_self > p.nta * ntm ? grid_self : p.nta * ntm);
  const size_t need = nfopp_fleet_shift_masks_workspace_bytes(b, m);
  NFOPP_REQUIRE(need == 0 || (workspace_dev && workspace_bytes >= need), "workspace too small or null (%zu bytes, %zu needed)",
                workspace_dev ? workspace_bytes : (size_t)0, need);
  unsigned long long* part = reinterpret_cast<unsigned long long*>(workspace_dev);
  int* bad_obstacle = m > 0 ? reinterpret_cast<int*>(part + b * ntm) : nullptr;
  hipStream_t s = (hipStream_t)stream;
  const int per_block = FS_THREADS / 64;
  hipLaunchKernelGGL(fleet_bad_kernel, dim3((unsigned)((b + per_block - 1) / per_block)), dim3(FS_THREADS), 0, s, tracks_dev, radius_dev,
                     (long long)b, (int)k, (int)stride, (int*)bad_dev);
  NFOPP_HIP(hipGetLastError());
  // the fleet against itself
  p.b = tracks_dev; p.rb = radius_dev; p.bb = b; p.stride_b = stride; p.kb = k; p.bad_b = bad_dev; p.self = 1;
  p.ns_log2 = fs_log2_ceil(2 * max_delay + 1);
  p.pair = reinterpret_cast<unsigned long long*>(pair_mask_dev); p.part = nullptr; p.ntb = p.nta;
  hipLaunchKernelGGL(fleet_shift_mask_kernel, dim3((unsigned)grid_self), dim3(FS_THREADS), 0, s, p);
  NFOPP_HIP(hipGetLastError());
  if (m > 0) {   // the fleet against the obstacles
    hipLaunchKernelGGL(fleet_bad_kernel, dim3((unsigned)((m + per_block - 1) / per_block)), dim3(FS_THREADS), 0, s, obstacles_dev,
                       obstacle_radius_dev, (long long)m, (int)(k + max_delay), (int)obstacle_stride, bad_obstacle);
    NFOPP_HIP(hipGetLastError());
    p.b = obstacles_dev; p.rb = obstacle_radius_dev; p.bb = m; p.stride_b = obstacle_stride; p.kb = k + max_delay;
    p.bad_b = bad_obstacle; p.self = 0;
    p.ns_log2 = fs_log2_ceil(max_delay + 1);
    p.pair = nullptr; p.part = part; p.ntb = ntm;
    hipLaunchKernelGGL(fleet_shift_mask_kernel, dim3((unsigned)(p.nta * ntm)), dim3(FS_THREADS), 0, s, p);
    NFOPP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(fleet_base_kernel, dim3((unsigned)((b + FS_THREADS - 1) / FS_THREADS)), dim3(FS_THREADS), 0, s,
                     (const unsigned long long*)part, (const int*)bad_dev, (long long)b, m > 0 ? ntm : 0LL,
                     reinterpret_cast<unsigned long long*>(base_mask_dev));
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" int nfopp_fleet_assign_delays(const uint64_t* pair_mask_dev, const uint64_t* base_mask_dev, const int32_t* bad_dev,
                                         const int32_t* order_dev, int64_t b, int32_t max_delay, int32_t* delay_dev,
                                         int32_t* status_dev, uint64_t* forbidden_dev, void* stream) {
  NFOPP_REQUIRE(b >= 0 && b <= 0x7fffffffLL, "bad batch size");
  NFOPP_REQUIRE(max_delay >= 0 && max_delay <= NFOPP_SCHEDULE_MAX_DELAY, "max_delay must be in 0 .. %d", NFOPP_SCHEDULE_MAX_DELAY);
  if (b == 0) return NFOPP_OK;
  NFOPP_REQUIRE(pair_mask_dev && base_mask_dev && bad_dev && delay_dev && status_dev, "null device pointer");
  AssignArgs p;
  p.pair = reinterpret_cast<const unsigned long long*>(pair_mask_dev);
  p.base = reinterpret_cast<const unsigned long long*>(base_mask_dev);
  p.bad = bad_dev; p.order = order_dev; p.b = b; p.max_delay = max_delay;
  p.delay = delay_dev; p.status = status_dev; p.forbidden = reinterpret_cast<unsigned long long*>(forbidden_dev);
  const size_t lds = (size_t)FS_ASSIGN_HEAD + (size_t)((b + 15) / 16 * 16);   // one byte of state per robot
  return launch_dynamic_lds(fleet_assign_kernel, 1, FS_ASSIGN_THREADS, lds, stream, p, "too many robots");
}
