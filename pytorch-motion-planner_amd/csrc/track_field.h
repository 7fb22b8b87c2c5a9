// What the step loop (csrc/traj_steps.hip) asks of csrc/track_field.hip before its first launch.
#pragma once
#include "common.h"

namespace nfopp {

// Every refusal of nfopp_traj_track_overlay that does not depend on the trajectory, draw and mask pointers: the field, the
// robot for poses of `dim` components, the waypoint times, the counts and out4's alignment.  -> NFOPP_OK or NFOPP_ERR_ARG.
int check_track_overlay(const nfopp_track_field* f, const float* wp_time_dev, int64_t batch, int32_t n_waypoints, int32_t dim,
                        const float* out4_dev);

}  // namespace nfopp
