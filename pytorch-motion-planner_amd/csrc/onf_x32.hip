// K1 on 32x32x16 tiles (csrc/onf_x32_impl.h): per-stream weight images and the family's launcher.  The kernels themselves are
// instantiated per feature dimension in csrc/onf_x32_k{14,13,8,7}.hip.
#include "onf_x32_impl.h"

namespace nfopp {
namespace x32 {

// a pool of its own: an x32 image is never evicted or invalidated by a split16 blob of the same stream
StreamScratch<ImageTag> g_images;

}  // namespace x32

int launch_x32(int nkt, int mode, const OnfKernelArgs& a, hipStream_t stream, int* grid_out) {
  return dispatch_nkt(nkt, a.geom, [&](auto k) -> int {
    // the kernels of a block count are written for ONE geometry: the kinds of their last input blocks are compile-time
    // constants (x32::Cfg::group_kind), so another angle dimension in the same number of blocks is refused, not computed
    using C = x32::Cfg<decltype(k)::value>;
    NFOPP_REQUIRE(C::geometry_ok(a.geom.n_enc, a.geom.fin, a.geom.ang_dim),
                  "the 32x32 ONF kernel for %d input blocks is built for n_enc %d, fin %d, angle_dim %d: got n_enc %d, fin %d, angle_dim %d",
                  decltype(k)::value, C::N_ENC, C::FIN, C::ANG_DIM, a.geom.n_enc, a.geom.fin, a.geom.ang_dim);
    return x32::launch_nkb<decltype(k)::value>(a, stream, mode, grid_out);
  });
}

}  // namespace nfopp
