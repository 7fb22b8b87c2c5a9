// Instances of csrc/onf_x32_impl.h for 7 input blocks of 16 (its own translation unit: the build compiles the feature
// dimensions in parallel).
#include "onf_x32_impl.h"

namespace nfopp {
namespace x32 {
template int launch_nkb<7>(const OnfKernelArgs&, hipStream_t, int, int*);
}  // namespace x32
}  // namespace nfopp
