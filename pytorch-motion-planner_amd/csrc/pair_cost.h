// Integer-pair path costs of the grid searches (grid_search.hip, lattice_search.hip): a cost is (a, b), ordered exactly as
// a + b * sqrt 2.  For counts below 2^21 two different pairs differ by more than 1 / (2^21 * 2.42) = 2e-7 while the rounding
// of the float64 key stays below 3e-9, so the order of DIFFERENT pairs is exact; equal pairs are recognised on the integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nfopp {

constexpr double GS_SQRT2 = 1.4142135623730951;

// Field cell in flight: the pair packed into one word, the two largest values reserved.  A wall is never relaxed; an
// unreached cell is.  Both read as "infinitely far" from a neighbour.
template <class T> struct Packed;
template <> struct Packed<uint32_t> {   // 16 + 16 bits: grids of at most 65535 cells (a path has fewer moves than that)
  static constexpr uint32_t WALL = 0xfffffffeu, UNREACHED = 0xffffffffu, STRAIGHT = 0x10000u, DIAGONAL = 1u;
  static __device__ __forceinline__ int a(uint32_t v) { return (int)(v >> 16); }
  static __device__ __forceinline__ int b(uint32_t v) { return (int)(v & 0xffffu); }
};
template <> struct Packed<uint64_t> {   // 32 + 32 bits
  static constexpr uint64_t WALL = 0xfffffffffffffffeull, UNREACHED = 0xffffffffffffffffull, STRAIGHT = 1ull << 32,
                            DIAGONAL = 1ull;
  static __device__ __forceinline__ int a(uint64_t v) { return (int)(v >> 32); }
  static __device__ __forceinline__ int b(uint64_t v) { return (int)(v & 0xffffffffull); }
};

template <class T>
__device__ __forceinline__ double pair_key(T v) {
  if (v >= Packed<T>::WALL) return INFINITY;
  return fma((double)Packed<T>::b(v), GS_SQRT2, (double)Packed<T>::a(v));
}
__device__ __forceinline__ double pair_key(int a, int b) { return fma((double)b, GS_SQRT2, (double)a); }

}  // namespace nfopp
