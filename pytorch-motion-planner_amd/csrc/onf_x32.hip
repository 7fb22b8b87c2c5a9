// K1 on 32x32x16 tiles (csrc/onf_x32_impl.h): per-stream weight images and the family's launcher.  The kernels themselves are
// instantiated per feature dimension in csrc/onf_x32_k{14,13,8,7}.hip.
#include "onf_x32_impl.h"

namespace nfopp {
namespace x32 {

// a pool of its own: an x32 image is never evicted or invalidated by a split16 blob of the same stream
StreamScratch<ImageTag> g_images;

}  // namespace x32

int launch_x32(int nkt, int mode, const OnfKernelArgs& a, hipStream_t stream, int* grid_out) {
  return dispatch_nkt(nkt, a.geom, [&](auto k) { return x32::launch_nkb<decltype(k)::value>(a, stream, mode, grid_out); });
}

}  // namespace nfopp
