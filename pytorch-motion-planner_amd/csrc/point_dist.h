// The two per-point fp32 expressions every point-cloud kernel shares: the ground-truth checkers of csrc/sampling.hip
// compare them with the robot's shape, the nearest-obstacle query of csrc/clearance.hip delivers them.  ONE arithmetic
// each, with explicit fmas, so that no two kernels can be contracted differently: `dist < radius` of the query is the
// circle checker's obstacle term bit for bit, and a point the rectangle checker accepts is at distance 0 from the box.
#pragma once
#include "common.h"

namespace nfopp {

// |obstacle - pose| for an obstacle (dx, dy) away from the pose
__device__ __forceinline__ float disc_distance(float dx, float dy) {
  return sqrtf(__builtin_fmaf(dx, dx, dy * dy));
}

// the obstacle (dx, dy away from the pose) in the frame of a robot heading (c, s) = (cos, sin): the form the brute-force
// rectangle kernel has always compiled to
__device__ __forceinline__ void robot_frame(float dx, float dy, float c, float s, float* rx, float* ry) {
  *rx = __builtin_fmaf(c, dx, s * dy);
  *ry = __builtin_fmaf(c, dy, -(s * dx));
}

}  // namespace nfopp
