// Wave and workgroup collectives of the path, map and obstacle kernels: one reduce, one exclusive scan, one (value, index)
// pair.  Every bit-for-bit pin these kernels have rests on the order stated here, and this header is its only owner.
//
// ORDER.  A wave is 64 lanes; a workgroup is WAVES waves of consecutive threads (threadIdx.x only).
//   * reduce: inside a wave an xor butterfly over the offsets 32, 16, .., 1, every lane combining op(own, other); then all
//     threads fold  identity, red[0], red[1], .., red[WAVES - 1]  from the left, in that order.
//   * scan: inside a wave __shfl_up over the offsets 1, 2, .., 32, a lane >= offset combining op(from_below, own); then
//     thread t's exclusive result is  op(fold(identity, red[0], .., red[wave - 1]), exclusive value inside its wave).
// BARRIERS.  block_reduce and block_exclusive_scan hold two __syncthreads each: the first so that `red` may still be read
//   by whatever the caller did before (a previous collective included), the second to publish it.  They must be called
//   from workgroup-uniform control flow, by every thread of the workgroup.  After the call `red` is being read: a caller
//   that writes it by hand needs a barrier of its own first.
// SCRATCH.  `red` is always the caller's: no __shared__ array and no __syncthreads_and / _or / _count in here, which bring
//   static LDS that comes off the 160 KiB the kernels with a path image in LDS size their longest path by (reparam.h).
// ARITHMETIC.  Only op(a, b) is evaluated.  An identity must be one for op (for an arg-extremum: lose to every candidate).
#pragma once
#include <hip/hip_runtime.h>

namespace nfopp {

constexpr int WAVES_FROM_BLOCKDIM = 0;   // WAVES argument: blockDim.x / 64, for a kernel launched at more than one size

// a + b, never half of a fused multiply-add whatever the including file's contraction mode is
struct Plus {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const {
#pragma clang fp contract(off)
    return a + b;
  }
};

// a | b on integers: the union of bit sets, which no order can change
struct BitOr {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a | b; }
};

// ---- what moves between lanes: scalars, and (value, index) pairs for "the extremum and where it is" -----------------
// The order on pairs (ties, NaN, "no candidate") is the caller's op and stays beside its kernel.
template <class V>
struct Indexed { V v; int i; };

template <class T>
__device__ __forceinline__ T lane_xor(T v, int o) { return __shfl_xor(v, o); }
template <class T>
__device__ __forceinline__ T lane_up(T v, int o) { return __shfl_up(v, o); }
template <class V>
__device__ __forceinline__ Indexed<V> lane_xor(Indexed<V> p, int o) { return {lane_xor(p.v, o), lane_xor(p.i, o)}; }

// Scratch of a reduction: T* for any T; for pairs two arrays, which pack tighter than an array of padded structs.
template <class V>
struct IndexedScratch { V* v; int* i; };
template <class T>
__device__ __forceinline__ void scratch_put(T* red, int k, T x) { red[k] = x; }
template <class T>
__device__ __forceinline__ T scratch_get(const T* red, int k) { return red[k]; }
template <class V>
__device__ __forceinline__ void scratch_put(IndexedScratch<V> red, int k, Indexed<V> x) { red.v[k] = x.v; red.i[k] = x.i; }
template <class V>
__device__ __forceinline__ Indexed<V> scratch_get(IndexedScratch<V> red, int k) { return {red.v[k], red.i[k]}; }

// ---- wave ---------------------------------------------------------------------------------------------------------
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {   // every lane gets the result
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, lane_xor(v, o));
  return v;
}

template <class T, class Op>
__device__ __forceinline__ T wave_inclusive_scan(T v, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = lane_up(v, o);
    if (lane >= o) v = op(up, v);
  }
  return v;
}

// ---- workgroup ------------------------------------------------------------------------------------------------------
// K values at once through one pair of barriers: v[k] <- the workgroup's reduction of v[k], in every thread.
// `red` holds WAVES * K entries.
template <int WAVES, int K, class T, class Op, class Red>
__device__ __forceinline__ void block_reduce(T (&v)[K], T identity, Op op, Red red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int waves = WAVES != WAVES_FROM_BLOCKDIM ? WAVES : (int)(blockDim.x >> 6);
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_reduce(v[k], op);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) scratch_put(red, wave * K + k, v[k]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T s = identity;
    for (int w = 0; w < waves; ++w) s = op(s, scratch_get(red, w * K + k));
    v[k] = s;
  }
}

template <int WAVES, class T, class Op, class Red>
__device__ __forceinline__ T block_reduce(T v, T identity, Op op, Red red) {
  T one[1] = {v};
  block_reduce<WAVES>(one, identity, op, red);
  return one[0];
}

// Exclusive scan of one value per thread in thread order; *total (if asked for) <- the fold of all wave totals, in every
// thread.  `red` holds WAVES entries.
template <int WAVES, class T, class Op>
__device__ __forceinline__ T block_exclusive_scan(T v, T identity, Op op, T* red, T* total = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_inclusive_scan(v, op);
  T excl = lane_up(incl, 1);
  if (lane == 0) excl = identity;
  __syncthreads();
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  T off = identity;
  for (int w = 0; w < wave; ++w) off = op(off, red[w]);
  if (total) {
    T all = identity;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) all = op(all, red[w]);
    *total = all;
  }
  return op(off, excl);
}

}  // namespace nfopp
