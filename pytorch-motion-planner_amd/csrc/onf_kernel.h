// Argument block, matrix-path route and launchers of the fused ONF kernels, shared by the dispatcher
// (csrc/onf_dispatch.hip) and the weight-gradient path (csrc/onf_wgrad.hip).
#pragma once
#include <type_traits>

#include "common.h"

namespace nfopp {

struct OnfKernelArgs {
  OnfGeom geom;
  const float* params;
  // explicit-point mode
  const float* points;
  // trajectory mode (points == nullptr)
  const float* traj;
  int n_way, dim;
  float* t;
  int t_mode;
  unsigned long long seed, rng_offset;
  long long traj_index_offset;
  long long n_points;
  // early stop (trajectory mode): live[0] = number of live trajectories, live[1 + k] = index of the k-th one (ascending).
  // The kernel then walks live[0] * (n_way - 1) samples; t / out4 rows keep their place (trajectory * (n_way-1) + j).
  const int* live;
  float* out4;
  // training mode (TRAIN kernels only): labels, BCE normalisation, the per-sample factors the weight-gradient GEMMs
  // (csrc/onf_wgrad.hip) cannot rebuild cheaply, per-wave loss and dW3[:100] partials.  NOT stored (rebuilt in pass 2
  // from the 48-byte record): the input features `in` (a function of u) and dh2 (= rho * W3a * [a2 > 0]); h2 never
  // leaves the kernel (its only use, dW3[:100] = sum_p rho_p h2_p, is accumulated here).
  const float* labels;
  float inv_count;
  int aug_feature;   // zero-weight pad feature evaluated as cos(0) = 1: the "ones" column of the input matrix
  // (slot orders below: the 16x16 kernels'; csrc/onf_x32.hip stores by index -- ones unit 101, rho row 100, ones feature fin,
  //  rows of 16 * ((fin + 16) / 16) floats in ws_de, no g4 partials: csrc/onf_wgrad.hip, onf_wgrad_split_kernel<NKT, XO>)
  float* ws_h1;      // [P, 112]      relu(a1) in slot order (layout Q), ones at slot 16*6 + 1
  float* ws_dh1;     // [P, 112]      d loss / d a1, rho at slot 16*6 + 1
  float* ws_de;      // [P, 16*NKT]   d loss / d (encoding argument)
  float* ws_u;       // [P, 12]       (ux, uy, 1, theta | rho, 0, 0, 0 | 4 words: bit 4*tile + r of word g = [a2 > 0])
  float* g4_partial; // [grid * WAVES, 112]  per-wave sum_p rho_p * relu(a2_p) in h2 slot order (layout P)
  float* loss_partial;  // [grid * WAVES]
};

// The kernel family a launch runs on, one per matrix path (csrc/onf_dispatch.hip: onf_route), and the family's count of
// 16-wide input tiles.
enum OnfFamily { ONF_FP32, ONF_SPLIT16, ONF_X32 };
struct OnfRoute { OnfFamily family; int nkt; };
// Input tiles of 16 a 16x16 kernel has to visit for `fin` features.  Layout P (csrc/onf_layout.h: slot_layout_p) deals the
// features of a block of 32 to a PAIR of tiles -- 0..7 and 16..23 to the even one, 8..15 and 24..31 to the odd one -- so the
// odd tile is in use from the block's 9th feature on: fin = 105..112 needs 8 tiles and 201..208 needs 14, where
// (fin + 15) / 16 says 7 and 13.
inline int layout_p_tiles(int fin) { return 2 * ((fin - 1) >> 5) + (((fin - 1) & 31) >= 8 ? 2 : 1); }
// Reads the matrix path once; sets "unsupported ONF feature dimension" and fails if the family has no kernel for g.
int onf_route(const OnfGeom& g, OnfRoute* r);

// Kernel modes: forward + input gradient (planner step), training pass (pass 1 of csrc/onf_wgrad.hip: factors for the
// weight-gradient GEMMs, *grid_out = workgroups launched), forward only (logits)
enum OnfMode { ONF_EVAL = 0, ONF_TRAIN = 1, ONF_LOGITS = 2 };
// one launcher per family; a.n_points > 0
int launch_fp32(int nkt, int mode, const OnfKernelArgs& a, hipStream_t stream, int* grid_out);     // csrc/onf_fused.hip
int launch_split16(int nkt, int mode, const OnfKernelArgs& a, hipStream_t stream, int* grid_out);  // csrc/onf_split.hip
int launch_x32(int nkt, int mode, const OnfKernelArgs& a, hipStream_t stream, int* grid_out);      // csrc/onf_x32.hip
int onf_unsupported(const OnfGeom& g);   // the error of a feature dimension without a kernel

// The ladders of every family's launcher: f(std::integral_constant) for the tile counts that have kernels / the three modes,
// so that a generic lambda can name its launcher template with decltype(k)::value.
template <class F>
int dispatch_nkt(int nkt, const OnfGeom& g, F&& f) {
  switch (nkt) {
    case 14: return f(std::integral_constant<int, 14>{});
    case 13: return f(std::integral_constant<int, 13>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return onf_unsupported(g);
  }
}
template <class F>
int dispatch_mode(int mode, F&& f) {
  return mode == ONF_EVAL ? f(std::integral_constant<int, ONF_EVAL>{})
         : mode == ONF_TRAIN ? f(std::integral_constant<int, ONF_TRAIN>{})
                             : f(std::integral_constant<int, ONF_LOGITS>{});
}

inline int launch_onf(const OnfRoute& r, int mode, const OnfKernelArgs& a, hipStream_t stream, int* grid_out = nullptr) {
  switch (r.family) {
    case ONF_FP32: return launch_fp32(r.nkt, mode, a, stream, grid_out);
    case ONF_SPLIT16: return launch_split16(r.nkt, mode, a, stream, grid_out);
    default: return launch_x32(r.nkt, mode, a, stream, grid_out);
  }
}

// csrc/onf_wgrad.hip: MFMA weight-gradient path of the ONF fitting step
size_t wgrad_workspace_bytes(const OnfGeom& g, long long n_samples);
// (pass 1 on the route of csrc/onf_dispatch.hip, pass 2 on the weight-gradient kernel that reads its factor order)
int onf_train_grad_mfma(const OnfGeom& g, const float* params, const float* samples, const float* labels,
                        long long n_samples, float inv_count, float* grad, float* ws, hipStream_t st);

}  // namespace nfopp
