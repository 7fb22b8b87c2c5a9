// How the shift-mask kernels of the fleet scheduler lay their work out and write their bits -- the tile of 8 x 8 pairs, the
// item index (pair, relative shift), the wave ballots that turn items into mask words, the mirror of the self-mode triangle by
// a bit reversal, the per-tile OR of the obstacle mode and the OR over a robot's obstacle tiles -- for fleet_schedule.hip
// (discs) and fleet_box_schedule.hip (oriented boxes).  Both write pair [b, b, 2], base [b] and bad [b] in the layout
// fleet_assign_kernel reads.  Integers only: nothing here rounds.
#pragma once
#include <hip/hip_runtime.h>

#include "nfopp_hip.h"

namespace nfopp {

constexpr int FS_TILE = 8;                                   // a tile is 8 x 8 pairs
constexpr int FS_PAIRS = FS_TILE * FS_TILE;
constexpr int FS_THREADS = 256;
static_assert(FS_PAIRS == 64 && FS_THREADS == 256, "the write-out below is one wave on 64 pairs");
static_assert(FS_PAIRS * 128 / FS_THREADS <= 32, "one bit per item of a thread in a 32-bit register");

// the low 2 * max_delay + 1 bits of (lo, hi) reversed: bit p -> bit 2 * max_delay - p
__device__ __forceinline__ void reverse_mask(unsigned long long lo, unsigned long long hi, int max_delay, unsigned long long* rlo,
                                             unsigned long long* rhi) {
  const unsigned long long flo = __brevll(hi), fhi = __brevll(lo);   // bit p -> bit 127 - p
  const int s = 127 - 2 * max_delay;                                 // 1 .. 127
  if (s >= 64) { *rlo = fhi >> (s - 64); *rhi = 0ull; }
  else { *rlo = (flo >> s) | (fhi << (64 - s)); *rhi = fhi >> s; }
}

// Item q = pair << ns_log2 | shift index of thread tid is q = tid + s * FS_THREADS, its bit is bit s of `done`.  The bits of a
// pair sit in consecutive lanes: a ballot is the mask word.  mask [FS_PAIRS * 2], zeroed by the caller; n_items is a multiple
// of 64, so a wave is inside the loop as a whole or not at all.
__device__ __forceinline__ void collect_item_bits(unsigned done, int n_items, int ns_log2, unsigned long long* mask) {
  const int tid = threadIdx.x, lane = tid & 63, ns = 1 << ns_log2;
  for (int s = 0, q = tid; q < n_items; ++s, q += FS_THREADS) {
    const unsigned long long bal = __ballot((done >> s & 1u) != 0u);
    if (ns_log2 >= 6) {
      if (lane == 0) mask[(q >> ns_log2) * 2 + ((q & (ns - 1)) >> 6)] = bal;
    } else if ((lane & (ns - 1)) == 0) {
      mask[(q >> ns_log2) * 2] = (bal >> lane) & ((1ull << ns) - 1ull);
    }
  }
}

// Self mode: the masks of the tile (ta, tb) of the upper triangle and their mirrors -> pair [b, b, 2]; the diagonal is 0.
__device__ __forceinline__ void store_pair_masks(const unsigned long long* mask, bool diagonal, long long a0, long long b0, long long b,
                                                 int max_delay, unsigned long long* pair) {
  const int tid = threadIdx.x;
  if (tid >= FS_PAIRS) return;
  const int li = tid >> 3, lj = tid & 7;
  const long long gi = a0 + li, gj = b0 + lj;
  if (!(gi < b && gj < b)) return;
  const unsigned long long lo = mask[tid * 2], hi = mask[tid * 2 + 1];
  if (diagonal && li == lj) {
    pair[(gi * b + gj) * 2] = 0ull; pair[(gi * b + gj) * 2 + 1] = 0ull;
  } else if (!diagonal || li < lj) {   // the lower half of a diagonal tile is written by its mirror
    unsigned long long rlo, rhi;
    reverse_mask(lo, hi, max_delay, &rlo, &rhi);
    pair[(gi * b + gj) * 2] = lo; pair[(gi * b + gj) * 2 + 1] = hi;
    pair[(gj * b + gi) * 2] = rlo; pair[(gj * b + gi) * 2 + 1] = rhi;
  }
}

// Obstacle mode: the OR of every robot's bits over the obstacles of tile tb -> part [ba, ntb]
__device__ __forceinline__ void store_obstacle_part(const unsigned long long* mask, long long a0, long long ba, long long tb, long long ntb,
                                                    unsigned long long* part) {
  const int tid = threadIdx.x;
  if (tid >= FS_TILE) return;
  const long long gi = a0 + tid;
  if (gi >= ba) return;
  unsigned long long m = 0ull;
  for (int lj = 0; lj < FS_TILE; ++lj) m |= mask[(tid * FS_TILE + lj) * 2];
  part[gi * ntb + tb] = m;
}

// base[i] <- the OR of robot i's obstacle partials (none: 0); 0 for a bad robot.  One thread per robot.
__device__ __forceinline__ void base_from_parts(const unsigned long long* part, const int* bad, long long n, long long n_tiles,
                                                unsigned long long* base) {
  const long long i = (long long)blockIdx.x * FS_THREADS + threadIdx.x;
  if (i >= n) return;
  unsigned long long m = 0ull;
  for (long long t = 0; t < n_tiles; ++t) m |= part[i * n_tiles + t];
  base[i] = bad[i] ? 0ull : m;
}

static inline long long fs_tiles(long long n) { return (n + FS_TILE - 1) / FS_TILE; }
static inline int fs_log2_ceil(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

}  // namespace nfopp
