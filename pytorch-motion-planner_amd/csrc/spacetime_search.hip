// Space-time grid search for the robots a fleet schedule cannot place: a robot that fleet_schedule.hip leaves unresolved gets
// ANOTHER PATH, chosen with time in it -- an earliest-arrival search on an occupancy grid against what is already reserved
// (cooperative A* without the heuristic: the frontier of an instant is a bitmap, a tick is nine shifted ANDs and an OR).
// The rule is this library's own (the reference plans one robot).
//
//   * st_reservation_init_kernel   the static part of a reservation: walls and the image edge, once per reservation
//   * st_bad_kernel                one wave per mover track: the bad flags
//   * st_reserve_kernel            THE HOT PATH.  One wave per (instant, row, word of 64 cells), one lane per cell, nine
//                                  directions per lane; the tracks pass through LDS in tiles of ST_TRACKS; a ballot per
//                                  direction is the word, and each word has one owner per launch: plain ORs, no atomics
//   * st_plan_init_kernel          the outputs of a fleet call before anyone is planned
//   * st_search_kernel             ONE workgroup per search: the frontier of the current and the next instant in LDS, reach of
//                                  every instant in the workspace, arrival by two workgroup reductions, the backward pass by one
//                                  wave (lane d tries direction d, a ballot and a count-trailing-zeros take the lowest)
//
// The rule (restated in numpy in tests/spacetime_ref.py; include/nfopp_hip.h repeats it for callers).
//  Grid.  An occupancy image [rows, cols] uint8, non-zero = wall, with OccupancyGrid's geometry: the float64 centre of cell
//    (row, col) is  col * res + res / 2 + b0  (x) and  row * res + res / 2 + b2  (y), every operation rounded on its own, left
//    to right.  The centre used EVERYWHERE is that value rounded to fp32: it is what the output tracks hold and, widened, what
//    the predicate reads.  The caller inflates the image for the robot's footprint.
//  Time.  T >= 1 instants on the callers' common grid; dt does not enter, everything is per tick.
//  Moves.  In one tick a robot stays or moves to one of its 8 neighbours (no corner rule; cells outside the image are walls); a
//    move takes one tick whatever its length.  Directions d = 0 .. 8 as (drow, dcol):
//      (0,+1) (0,-1) (+1,0) (-1,0) (+1,+1) (+1,-1) (-1,+1) (-1,-1) (0,0) -- the wait is last.
//  Movers.  M tracks [M, T, stride >= 2] fp32 in absolute time, never shifted, a radius each (null: 0) and a visible flag each
//    (null: all visible).  A track with a non-finite coordinate or radius is bad and skipped.
//  Edge (u, d, h): the robot goes from cell u at instant h to v = u + d at h + 1.  It is BLOCKED if v is outside the image or a
//    wall, or if some visible good mover j gives the conflict predicate of track_pairs.h on this one interval:
//      d0 = centre(u) - p_j[h],  d1 = centre(v) - p_j[h + 1],  m = closest_approach(d0, |d0|^2, d1, |d1|^2).m,  blocked when
//      m < R2_j (strict),  R_j = (robot_radius + r_j) + margin,  R2_j = R_j * R_j  (pair_radius).
//    last[u]: |centre(u) - p_j[T - 1]|^2 < R2_j for some such j -- the last-instant term.
//    One robot_radius (an fp32 value) for the whole planned fleet, so a reservation does not depend on who is planned.
//  Search of one robot, start cell s, goal cell g:
//    reach_0 = {s};  reach_{h+1}[v] = OR over d of (reach_h[v - d] and edge (v - d, d, h) not blocked)
//    park[T - 1] = !last[g];  park[h] = park[h + 1] and wait edge (g, 8, h) not blocked
//    arrival h* = the smallest h with reach_h[g] and park[h]
//    path: cell[h] = g for h >= h*; backwards from (g, h*) the predecessor of (v, h) is v - d for the LOWEST d with
//    reach_{h-1}[v - d] and edge (v - d, d, h - 1) not blocked.  It ends at (s, 0) by construction.
//  Statuses.  0 planned; NFOPP_SPACETIME_BAD_CELL start or goal outside the image or on a wall; _UNREACHED no such h*;
//    _NOT_ORDERED never visited.  A robot that is not planned has arrival -1, cells all -1, NaN track rows and reserves nothing.
//  Fleet.  order [R] int32 (null: 0 .. R - 1) is visited front to back; an entry out of range or a robot already visited is
//    skipped, on the device, before anything is indexed by it.  Each planned robot's output track (fp32 centres, radius
//    robot_radius) is reserved before the next robot is searched, so robot k's predicate against robot k' < k is the
//    predicate of track_conflict.hip on the two OUTPUT tracks, bit for bit: nobody planned is in conflict by
//    nfopp_track_conflicts itself, by construction.
//
// LAYOUT of a reservation: uint64 words, W = (cols + 63) / 64 words a row, bit c % 64 of word c / 64 is column c.
//    blocked [T - 1][9][rows][W]   bit = edge (u, d, h) is blocked, indexed by the SOURCE cell u
//    last    [rows][W]             follows it
//  The padding bits of a row (columns >= cols) are 1 in `blocked` -- no edge leaves a cell that does not exist, which is what
//  keeps a frontier from leaking across a row end -- and 0 in `last`.
//
// Predicates and integer ORs; a word of the reservation has exactly one writing wave per launch and launches are ordered by the
// stream: no atomics, nothing depends on an order, two runs give the same bits.  No kernel waits on another workgroup or
// spins on memory; every loop is bounded by T, by the cell count or by M.
#include <limits.h>
#include <math.h>

#include "block_collectives.h"
#include "common.h"
#include "grid_frame.h"
#include "track_pairs.h"

#pragma clang fp contract(off)

namespace nfopp {

constexpr int ST_DIRS = 9;
constexpr int ST_WAIT = 8;
constexpr int ST_THREADS = 256;                 // reserve, init: four waves, four words of 64 cells
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int ST_TRACKS = 16;                   // tracks staged in LDS per trip of the reserve kernel
constexpr int ST_INIT_CHUNK = 16;               // instants one thread of the init kernel writes its static word to
constexpr int ST_SEARCH_THREADS = 1024;
constexpr int ST_SEARCH_WAVES = ST_SEARCH_THREADS / 64;
constexpr int ST_SEARCH_HEAD = 64;              // bytes in front of the frontiers: the reductions' scratch
static_assert(ST_SEARCH_WAVES * 4 <= ST_SEARCH_HEAD, "the reductions' scratch fits its head");
static_assert(ST_TRACKS <= ST_THREADS, "one thread stages one track");

// (drow, dcol) + 1 of direction d in two bits each: a table in a register
constexpr unsigned st_pack(const int (&v)[ST_DIRS]) {
  unsigned r = 0;
  for (int d = 0; d < ST_DIRS; ++d) r |= (unsigned)(v[d] + 1) << (2 * d);
  return r;
}
constexpr int ST_DROW[ST_DIRS] = {0, 0, 1, -1, 1, 1, -1, -1, 0};
constexpr int ST_DCOL[ST_DIRS] = {1, -1, 0, 0, 1, -1, 1, -1, 0};
constexpr unsigned ST_DROW_BITS = st_pack(ST_DROW), ST_DCOL_BITS = st_pack(ST_DCOL);
__host__ __device__ __forceinline__ int st_drow(int d) { return (int)((ST_DROW_BITS >> (2 * d)) & 3u) - 1; }
__host__ __device__ __forceinline__ int st_dcol(int d) { return (int)((ST_DCOL_BITS >> (2 * d)) & 3u) - 1; }

struct IntMax { __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct IntMin { __device__ __forceinline__ int operator()(int a, int b) const { return a < b ? a : b; } };

__device__ __forceinline__ bool st_wall(const unsigned char* occ, int rows, int cols, int r, int c) {
  return r < 0 || r >= rows || c < 0 || c >= cols || occ[(long long)r * cols + c] != 0;
}

// ---- the static part -------------------------------------------------------------------------------------------------------
// thread (direction d, word q) forms its static word once and writes it to ST_INIT_CHUNK instants; `last` is cleared
__global__ __launch_bounds__(ST_THREADS) void st_reservation_init_kernel(const unsigned char* occ, int rows, int cols, int words, int T,
                                                                         unsigned long long* blocked, unsigned long long* last) {
  const int rw = rows * words;
  const int n = ST_DIRS * rw;
  const int idx = blockIdx.x * ST_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int d = idx / rw, q = idx % rw, r = q / words, w = q % words;
  if (blockIdx.y == 0 && d == 0) last[q] = 0ull;
  const int h0 = blockIdx.y * ST_INIT_CHUNK, h1 = min(h0 + ST_INIT_CHUNK, T - 1);
  if (h0 >= h1) return;
  const int dr = st_drow(d), dc = st_dcol(d);
  unsigned long long word = 0ull;
  for (int b = 0; b < 64; ++b) {
    const int c = w * 64 + b;
    const bool block = c >= cols || st_wall(occ, rows, cols, r + dr, c + dc);
    word |= (unsigned long long)block << b;
  }
  for (int h = h0; h < h1; ++h) blocked[(long long)(h * ST_DIRS + d) * rw + q] = word;
}

// flags[t] <- 1 when track t has a non-finite x or y at any instant, or a non-finite radius; one wave per track
__global__ __launch_bounds__(ST_THREADS) void st_bad_kernel(const float* tracks, const float* radius, long long n, int T, int stride, int* flags) {
  const long long t = (long long)blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
  if (t >= n) return;   // a whole wave
  const int lane = threadIdx.x & 63;
  const float* row = tracks + t * (long long)T * stride;
  bool bad = false;
  for (int h = lane; h < T; h += 64) {
    const float* s = row + (long long)h * stride;
    bad |= !(finite32(s[0]) && finite32(s[1]));
  }
  const bool any = __ballot(bad) != 0ull;
  if (lane == 0) flags[t] = (any || (radius && !finite32(radius[t]))) ? 1 : 0;
}

// ---- the hot path ----------------------------------------------------------------------------------------------------------
struct ReserveArgs {
  const float* tracks; const float* radius;       // [m, T, stride]; radius null: default_radius
  const unsigned char* visible; const int* bad;    // null: all visible / nobody bad
  long long m;
  int stride, T, rows, cols, words, blocks_per_instant;
  float robot_radius, default_radius;
  double margin, b0, b2, res;
  unsigned long long* blocked; unsigned long long* last;
  // fleet mode (state non-null): the one track is the output track of robot order[pos], if that robot was planned at pos
  const int* order; const int* state; const int* status;
  long long robots; int pos;
};

__global__ __launch_bounds__(ST_THREADS) void st_reserve_kernel(const ReserveArgs p) {
  __shared__ float2 sP0[ST_TRACKS], sP1[ST_TRACKS];
  __shared__ double sR2[ST_TRACKS];   // < 0: the track is skipped
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long first = 0;
  if (p.state) {   // the same in every thread of the grid
    const long long i = p.order ? (long long)p.order[p.pos] : (long long)p.pos;
    if (i < 0 || i >= p.robots) return;
    if (p.state[i] != p.pos + 1 || p.status[i] != 0) return;   // a repeat, or not planned: it reserves nothing
    first = i;
  }
  const int rw = p.rows * p.words;
  const int h = blockIdx.x / p.blocks_per_instant;             // T - 1: the last-instant term
  const int q = (blockIdx.x % p.blocks_per_instant) * ST_WAVES + wave;
  const bool valid = q < rw;                                    // a whole wave
  const bool last_term = h == p.T - 1;
  const int r = valid ? q / p.words : 0, col = (valid ? q % p.words : 0) * 64 + lane;
  double xs[3], ys[3];   // the centres of the columns col - 1 .. col + 1 and the rows r - 1 .. r + 1, widened
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    xs[k] = (double)grid_cell_centre((double)(col + k - 1), p.res, p.b0);
    ys[k] = (double)grid_cell_centre((double)(r + k - 1), p.res, p.b2);
  }
  unsigned bits = 0u;   // bit d: edge (this cell, d, h) meets a mover; bit 0 alone for the last-instant term
  for (long long j0 = 0; j0 < p.m; j0 += ST_TRACKS) {
    __syncthreads();   // the previous trip's reads
    if (tid < ST_TRACKS) {
      const long long j = j0 + tid;
      float2 a = make_float2(0.f, 0.f), b = a;
      double R2 = -1.0;
      if (j < p.m && (!p.visible || p.visible[j]) && !(p.bad && p.bad[j])) {
        const float* row = p.tracks + (first + j) * (long long)p.T * p.stride;
        const float* s0 = row + (long long)h * p.stride;
        a.x = s0[0]; a.y = s0[1];
        b = a;
        if (!last_term) { b.x = s0[p.stride]; b.y = s0[p.stride + 1]; }
        double R;
        pair_radius((double)p.robot_radius, (double)(p.radius ? p.radius[j] : p.default_radius), p.margin, &R, &R2);
      }
      sP0[tid] = a; sP1[tid] = b; sR2[tid] = R2;
    }
    __syncthreads();
    if (!valid) continue;
    const int n = (int)min((long long)ST_TRACKS, p.m - j0);
    for (int t = 0; t < n; ++t) {
      const double R2 = sR2[t];
      if (!(R2 >= 0.0)) continue;   // skipped (the same in every lane)
      const float2 a = sP0[t], b = sP1[t];
      const double x0 = xs[1] - (double)a.x, y0 = ys[1] - (double)a.y;
      const double cc = x0 * x0 + y0 * y0;
      if (last_term) {
        if (cc < R2) bits |= 1u;
        continue;
      }
#pragma unroll
      for (int d = 0; d < ST_DIRS; ++d) {
        const double d1x = xs[1 + st_dcol(d)] - (double)b.x, d1y = ys[1 + st_drow(d)] - (double)b.y;
        const double e = d1x * d1x + d1y * d1y;
        const double m = closest_approach(x0, y0, cc, d1x, d1y, e).m;
        if (m < R2) bits |= 1u << d;
      }
    }
  }
  if (!valid) return;
  // the cells of a word sit in the lanes of a wave: a ballot is the word.  Padding lanes may carry anything: their bits are
  // already 1 in `blocked` and are masked off for `last`
  if (last_term) {
    const unsigned long long bal = __ballot((bits & 1u) != 0u);
    const int n_in = p.cols - (q % p.words) * 64;   // >= 1
    const unsigned long long in = n_in >= 64 ? ~0ull : ((1ull << n_in) - 1ull);
    if (lane == 0 && (bal & in)) p.last[q] |= bal & in;
    return;
  }
#pragma unroll
  for (int d = 0; d < ST_DIRS; ++d) {
    const unsigned long long bal = __ballot((bits >> d & 1u) != 0u);
    if (lane == d && bal) p.blocked[(long long)(h * ST_DIRS + d) * rw + q] |= bal;
  }
}

// ---- the fleet -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void st_plan_init_kernel(long long robots, int T, int* state, int* cells, int* arrival, int* status,
                                                                  float* tracks) {
  const long long n = robots * T;
  const float nan = __builtin_nanf("");
  for (long long k = (long long)blockIdx.x * ST_THREADS + threadIdx.x; k < n; k += (long long)gridDim.x * ST_THREADS) {
    cells[k] = -1; tracks[2 * k] = nan; tracks[2 * k + 1] = nan;
    if (k < robots) { state[k] = 0; arrival[k] = -1; status[k] = NFOPP_SPACETIME_NOT_ORDERED; }
  }
}

struct SearchArgs {
  const unsigned char* occ;
  int rows, cols, words, T;
  double b0, b2, res;
  const int* start; const int* goal;       // [robots, 2] (row, col)
  const int* order; long long robots; int pos;
  const unsigned long long* blocked; const unsigned long long* last;
  unsigned long long* reach;               // [T][rows][words]
  int* state;                              // 0: not visited yet; pos + 1: visited at position pos
  int* cells; int* arrival; int* status; float* tracks;
};

__device__ __forceinline__ bool st_bit(const unsigned long long* words, long long q, int c) { return (words[q] >> (c & 63) & 1ull) != 0ull; }

__global__ __launch_bounds__(ST_SEARCH_THREADS) void st_search_kernel(const SearchArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char st_smem[];
  int* red = reinterpret_cast<int*>(st_smem);
  const int rw = p.rows * p.words, W = p.words;
  unsigned long long* cur = reinterpret_cast<unsigned long long*>(st_smem + ST_SEARCH_HEAD);
  unsigned long long* nxt = cur + rw;
  const int tid = threadIdx.x, lane = tid & 63;

  // everything up to the search is the same in every thread
  const long long i = p.order ? (long long)p.order[p.pos] : (long long)p.pos;
  if (i < 0 || i >= p.robots) return;
  if (p.state[i] != 0) return;   // visited before
  __syncthreads();               // every thread has read state[i]
  if (tid == 0) p.state[i] = p.pos + 1;
  const int sr = p.start[2 * i], sc = p.start[2 * i + 1], gr = p.goal[2 * i], gc = p.goal[2 * i + 1];
  if (st_wall(p.occ, p.rows, p.cols, sr, sc) || st_wall(p.occ, p.rows, p.cols, gr, gc)) {
    if (tid == 0) p.status[i] = NFOPP_SPACETIME_BAD_CELL;
    return;
  }
  const int sq = sr * W + (sc >> 6), gq = gr * W + (gc >> 6);

  // forward: reach_0 = {s}; one tick is nine shifted ANDs and an OR
  for (int q = tid; q < rw; q += ST_SEARCH_THREADS) {
    const unsigned long long v = q == sq ? 1ull << (sc & 63) : 0ull;
    cur[q] = v; p.reach[q] = v;
  }
  for (int h = 0; h + 1 < p.T; ++h) {
    __syncthreads();   // cur is written, nxt is no longer read
    const unsigned long long* blk = p.blocked + (long long)h * ST_DIRS * rw;
    for (int q = tid; q < rw; q += ST_SEARCH_THREADS) {
      const int r = q / W, w = q % W;
      unsigned long long acc = 0ull;
#pragma unroll
      for (int d = 0; d < ST_DIRS; ++d) {
        const int ur = r - st_drow(d);
        if (ur < 0 || ur >= p.rows) continue;
        const int uq = ur * W + w;
        const unsigned long long* bd = blk + (long long)d * rw;
        // the sources of this word's cells: the same word, and one bit of its neighbour across the word boundary
        unsigned long long open = cur[uq];
        if (open) open &= ~bd[uq];
        if (st_dcol(d) == 0) acc |= open;
        else if (st_dcol(d) > 0) {
          acc |= open << 1;
          if (w > 0) { unsigned long long o = cur[uq - 1] >> 63; if (o) o &= ~(bd[uq - 1] >> 63); acc |= o; }
        } else {
          acc |= open >> 1;
          if (w + 1 < W) { unsigned long long o = cur[uq + 1] & 1ull; if (o) o &= ~bd[uq + 1]; acc |= o << 63; }
        }
      }
      nxt[q] = acc; p.reach[(long long)(h + 1) * rw + q] = acc;
    }
    unsigned long long* t = cur; cur = nxt; nxt = t;
  }
  __threadfence_block();   // reach is read back below by other threads of this workgroup (the reductions hold the barriers)

  // park[h] holds from one past the last blocked wait edge at g on, if last[g] is clear
  int hb = -1;
  for (int h = tid; h + 1 < p.T; h += ST_SEARCH_THREADS)
    if (st_bit(p.blocked + (long long)(h * ST_DIRS + ST_WAIT) * rw, gq, gc)) hb = h;   // ascending in a thread
  hb = block_reduce<ST_SEARCH_WAVES>(hb, -1, IntMax(), red);
  int ha = INT_MAX;
  for (int h = tid; h < p.T; h += ST_SEARCH_THREADS)
    if (h > hb && h < ha && st_bit(p.reach + (long long)h * rw, gq, gc)) ha = h;
  ha = block_reduce<ST_SEARCH_WAVES>(ha, INT_MAX, IntMin(), red);
  if (ha == INT_MAX || st_bit(p.last, gq, gc)) {
    if (tid == 0) p.status[i] = NFOPP_SPACETIME_UNREACHED;
    return;
  }

  // backward, one wave: lane d tries direction d, the lowest that holds is taken
  int* cells = p.cells + i * p.T;
  if (tid < 64) {
    int vr = gr, vc = gc;
    const int dr = lane < ST_DIRS ? st_drow(lane) : 0, dc = lane < ST_DIRS ? st_dcol(lane) : 0;
    for (int h = ha; h >= 1; --h) {
      const int ur = vr - dr, uc = vc - dc;
      bool ok = lane < ST_DIRS && ur >= 0 && ur < p.rows && uc >= 0 && uc < p.cols;
      if (ok) {
        const long long uq = (long long)ur * W + (uc >> 6);
        ok = st_bit(p.reach + (long long)(h - 1) * rw, uq, uc) && !st_bit(p.blocked + (long long)((h - 1) * ST_DIRS + lane) * rw, uq, uc);
      }
      const unsigned long long bal = __ballot(ok);
      if (bal == 0ull) break;   // cannot happen: (v, h) was reached through some edge
      const int d = (int)__builtin_ctzll(bal);
      if (lane == 0) cells[h] = vr * p.cols + vc;
      vr -= st_drow(d); vc -= st_dcol(d);
    }
    if (lane == 0) cells[0] = vr * p.cols + vc;
  }
  __threadfence_block();
  __syncthreads();
  float* track = p.tracks + i * (long long)p.T * 2;
  for (int h = tid; h < p.T; h += ST_SEARCH_THREADS) {
    const int cell = h >= ha ? gr * p.cols + gc : cells[h];
    if (h > ha) cells[h] = cell;
    track[2 * h] = grid_cell_centre((double)(cell % p.cols), p.res, p.b0);
    track[2 * h + 1] = grid_cell_centre((double)(cell / p.cols), p.res, p.b2);
  }
  if (tid == 0) { p.arrival[i] = ha; p.status[i] = 0; }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static long long st_words(long long cols) { return (cols + 63) / 64; }
static size_t st_round8(size_t n) { return (n + 7) / 8 * 8; }
// words of a reservation, or -1 when the image and T are not ones an int32 indexes
static long long st_reservation_words(int32_t rows, int32_t cols, int32_t T) {
  if (rows < 1 || cols < 1 || T < 1) return -1;
  const long long rw = (long long)rows * st_words(cols);
  if (rw > 0x7fffffffLL / ST_DIRS) return -1;
  const long long n = ((long long)(T - 1) * ST_DIRS + 1) * rw;
  return n <= 0x7fffffffLL && (long long)rows * cols <= 0x7fffffffLL ? n : -1;
}

#define ST_REQUIRE_IMAGE(rows, cols, T)                                                                            \
  do {                                                                                                             \
    NFOPP_REQUIRE((T) >= 1, "a reservation needs at least one instant (T >= 1)");                                 \
    NFOPP_REQUIRE((rows) >= 1 && (cols) >= 1, "the image must have at least one cell");                           \
    NFOPP_REQUIRE(st_reservation_words(rows, cols, T) >= 0, "image and T too large for an index (%d x %d x %d)", \
                  (int)(rows), (int)(cols), (int)(T));                                                            \
  } while (0)

static bool st_finite(double v) { return v == v && fabs(v) < (double)__builtin_inff(); }

#define ST_REQUIRE_GEOMETRY(b0, b2, res, robot_radius, margin)                                                              \
  do {                                                                                                                      \
    NFOPP_REQUIRE(st_finite(b0) && st_finite(b2) && st_finite(res) && (res) > 0.0, "grid origin and resolution must be finite, resolution > 0"); \
    NFOPP_REQUIRE(st_finite((double)(robot_radius)), "robot_radius must be finite");                                        \
    NFOPP_REQUIRE(st_finite(margin), "margin must be finite");                                                              \
  } while (0)

static int st_launch_reserve(ReserveArgs& p, void* reservation_dev, hipStream_t s) {
  const long long rw = (long long)p.rows * p.words;
  p.blocked = reinterpret_cast<unsigned long long*>(reservation_dev);
  p.last = p.blocked + (long long)(p.T - 1) * ST_DIRS * rw;
  p.blocks_per_instant = (int)((rw + ST_WAVES - 1) / ST_WAVES);
  const long long grid = (long long)p.blocks_per_instant * p.T;
  NFOPP_REQUIRE(grid <= 0x7fffffffLL, "image and T too large for one launch (%lld workgroups)", grid);
  hipLaunchKernelGGL(st_reserve_kernel, dim3((unsigned)grid), dim3(ST_THREADS), 0, s, p);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

}  // namespace nfopp

using namespace nfopp;

extern "C" size_t nfopp_spacetime_reservation_bytes(int32_t rows, int32_t cols, int32_t t) {
  const long long n = st_reservation_words(rows, cols, t);
  return n < 0 ? 0 : (size_t)n * sizeof(unsigned long long);
}

extern "C" int nfopp_spacetime_reservation_init(const uint8_t* occupancy_dev, int32_t rows, int32_t cols, int32_t t,
                                                uint64_t* reservation_dev, size_t reservation_bytes, void* stream) {
  ST_REQUIRE_IMAGE(rows, cols, t);
  NFOPP_REQUIRE(occupancy_dev && reservation_dev, "null device pointer");
  NFOPP_REQUIRE(reservation_bytes >= nfopp_spacetime_reservation_bytes(rows, cols, t), "reservation too small (%zu bytes, %zu needed)",
                reservation_bytes, nfopp_spacetime_reservation_bytes(rows, cols, t));
  const int words = (int)st_words(cols);
  const long long rw = (long long)rows * words;
  unsigned long long* blocked = reinterpret_cast<unsigned long long*>(reservation_dev);
  const unsigned gx = (unsigned)((ST_DIRS * rw + ST_THREADS - 1) / ST_THREADS);
  const unsigned gy = (unsigned)((t - 1 + ST_INIT_CHUNK - 1) / ST_INIT_CHUNK);
  NFOPP_REQUIRE(gy <= 65535u, "too many instants for one launch (T = %d)", (int)t);
  hipLaunchKernelGGL(st_reservation_init_kernel, dim3(gx, gy > 0 ? gy : 1u), dim3(ST_THREADS), 0, (hipStream_t)stream, occupancy_dev,
                     (int)rows, (int)cols, words, (int)t, blocked, blocked + (long long)(t - 1) * ST_DIRS * rw);
  NFOPP_HIP(hipGetLastError());
  return NFOPP_OK;
}

extern "C" size_t nfopp_spacetime_reserve_workspace_bytes(int64_t m) { return m > 0 ? st_round8((size_t)m * sizeof(int)) : 0; }

extern "C" int nfopp_spacetime_reserve(int32_t rows, int32_t cols, int32_t t, double b0, double b2, double resolution,
                                       float robot_radius, double margin, const float* tracks_dev, int64_t m, int32_t stride,
                                       const float* radius_dev, const uint8_t* visible_dev, uint64_t* reservation_dev,
                                       size_t reservation_bytes, void* workspace_dev, size_t workspace_bytes, void* stream) {
  ST_REQUIRE_IMAGE(rows, cols, t);
  ST_REQUIRE_GEOMETRY(b0, b2, resolution, robot_radius, margin);
  NFOPP_REQUIRE(m >= 0 && m <= 0x7fffffffLL, "bad batch size");
  NFOPP_REQUIRE(stride >= 2, "a track row holds x and y: stride must be >= 2");
  NFOPP_REQUIRE((long long)t * stride <= 0x7fffffffLL, "image and T too large for an index (T * stride)");
  NFOPP_REQUIRE(reservation_dev, "null device pointer");
  NFOPP_REQUIRE(reservation_bytes >= nfopp_spacetime_reservation_bytes(rows, cols, t), "reservation too small (%zu bytes, %zu needed)",
                reservation_bytes, nfopp_spacetime_reservation_bytes(rows, cols, t));
  if (m == 0) return NFOPP_OK;
  NFOPP_REQUIRE(tracks_dev, "null device pointer");
  const size_t need = nfopp_spacetime_reserve_workspace_bytes(m);
  NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small or null (%zu bytes, %zu needed)",
                workspace_dev ? workspace_bytes : (size_t)0, need);
  hipStream_t s = (hipStream_t)stream;
  int* bad = reinterpret_cast<int*>(workspace_dev);
  hipLaunchKernelGGL(st_bad_kernel, dim3((unsigned)((m + ST_WAVES - 1) / ST_WAVES)), dim3(ST_THREADS), 0, s, tracks_dev, radius_dev,
                     (long long)m, (int)t, (int)stride, bad);
  NFOPP_HIP(hipGetLastError());
  ReserveArgs p = {};
  p.tracks = tracks_dev; p.radius = radius_dev; p.visible = visible_dev; p.bad = bad; p.m = m;
  p.stride = stride; p.T = t; p.rows = rows; p.cols = cols; p.words = (int)st_words(cols);
  p.robot_radius = robot_radius; p.default_radius = 0.0f; p.margin = margin; p.b0 = b0; p.b2 = b2; p.res = resolution;
  return st_launch_reserve(p, reservation_dev, s);
}

extern "C" size_t nfopp_spacetime_plan_workspace_bytes(int32_t rows, int32_t cols, int32_t t, int64_t robots) {
  if (st_reservation_words(rows, cols, t) < 0 || robots <= 0) return 0;
  return (size_t)t * (size_t)rows * (size_t)st_words(cols) * sizeof(unsigned long long) + st_round8((size_t)robots * sizeof(int));
}

extern "C" int nfopp_spacetime_plan_fleet(const uint8_t* occupancy_dev, int32_t rows, int32_t cols, int32_t t, double b0, double b2,
                                          double resolution, float robot_radius, double margin, const int32_t* start_cells_dev,
                                          const int32_t* goal_cells_dev, const int32_t* order_dev, int64_t robots,
                                          uint64_t* reservation_dev, size_t reservation_bytes, int32_t* cells_dev,
                                          int32_t* arrival_dev, int32_t* status_dev, float* tracks_dev, void* workspace_dev,
                                          size_t workspace_bytes, void* stream) {
  ST_REQUIRE_IMAGE(rows, cols, t);
  ST_REQUIRE_GEOMETRY(b0, b2, resolution, robot_radius, margin);
  NFOPP_REQUIRE(robots >= 0 && robots <= 0x7fffffffLL, "bad batch size");
  const long long rw = (long long)rows * st_words(cols);
  NFOPP_REQUIRE((long long)t * rw <= 0x7fffffffLL && robots * t <= 0x7fffffffLL / 2, "image and T too large for an index (%d x %d x %d)",
                (int)rows, (int)cols, (int)t);
  const size_t lds = (size_t)ST_SEARCH_HEAD + 2 * (size_t)rw * sizeof(unsigned long long);
  NFOPP_REQUIRE(lds <= 160 * 1024, "frontier too large for one workgroup's LDS (%zu bytes)", lds);
  if (robots == 0) return NFOPP_OK;
  NFOPP_REQUIRE(occupancy_dev && start_cells_dev && goal_cells_dev && reservation_dev && cells_dev && arrival_dev && status_dev && tracks_dev,
                "null device pointer");
  NFOPP_REQUIRE(reservation_bytes >= nfopp_spacetime_reservation_bytes(rows, cols, t), "reservation too small (%zu bytes, %zu needed)",
                reservation_bytes, nfopp_spacetime_reservation_bytes(rows, cols, t));
  const size_t need = nfopp_spacetime_plan_workspace_bytes(rows, cols, t, robots);
  NFOPP_REQUIRE(workspace_dev && workspace_bytes >= need, "workspace too small or null (%zu bytes, %zu needed)",
                workspace_dev ? workspace_bytes : (size_t)0, need);
  hipStream_t s = (hipStream_t)stream;
  SearchArgs q = {};
  q.occ = occupancy_dev; q.rows = rows; q.cols = cols; q.words = (int)st_words(cols); q.T = t;
  q.b0 = b0; q.b2 = b2; q.res = resolution; q.start = start_cells_dev; q.goal = goal_cells_dev; q.order = order_dev; q.robots = robots;
  q.blocked = reinterpret_cast<const unsigned long long*>(reservation_dev);
  q.last = q.blocked + (long long)(t - 1) * ST_DIRS * rw;
  q.reach = reinterpret_cast<unsigned long long*>(workspace_dev);
  q.state = reinterpret_cast<int*>(q.reach + (long long)t * rw);
  q.cells = cells_dev; q.arrival = arrival_dev; q.status = status_dev; q.tracks = tracks_dev;
  ReserveArgs p = {};
  p.tracks = tracks_dev; p.m = 1; p.stride = 2; p.T = t; p.rows = rows; p.cols = cols; p.words = q.words;
  p.robot_radius = robot_radius; p.default_radius = robot_radius; p.margin = margin; p.b0 = b0; p.b2 = b2; p.res = resolution;
  p.order = order_dev; p.state = q.state; p.status = status_dev; p.robots = robots;
  const long long cells_n = robots * t;
  const long long init_blocks = (cells_n + ST_THREADS - 1) / ST_THREADS;
  const unsigned init_grid = (unsigned)(init_blocks < 2048 ? init_blocks : 2048);
  hipLaunchKernelGGL(st_plan_init_kernel, dim3(init_grid), dim3(ST_THREADS), 0, s, (long long)robots, (int)t, q.state, cells_dev, arrival_dev,
                     status_dev, tracks_dev);
  NFOPP_HIP(hipGetLastError());
  for (long long pos = 0; pos < robots; ++pos) {   // a search and the reservation of what it wrote: 2 launches a position
    q.pos = p.pos = (int)pos;
    const int rc = launch_dynamic_lds(st_search_kernel, 1, ST_SEARCH_THREADS, lds, stream, q, "frontier too large");
    if (rc != NFOPP_OK) return rc;
    const int rr = st_launch_reserve(p, reservation_dev, s);
    if (rr != NFOPP_OK) return rr;
  }
  return NFOPP_OK;
}
