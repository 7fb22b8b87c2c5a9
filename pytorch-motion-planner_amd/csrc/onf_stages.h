// The stages of K1 on 16-point tiles around the four GEMMs that csrc/onf_fused.hip (fp32 MFMA) and csrc/onf_split.hip
// (bf16x3 on 16x16x32 tiles) BOTH call; everything here has exactly these two callers.  In the order a chunk runs them:
//   l1_features   [L1]   store_factor_row (h1)   [L2]   store_logits   [L2T]   store_factor_row (dh1)   [L1T]
//   chain_rule_tile   store_de_tile   store_out4
// They define the slot order of the factor matrices that pass 2 (csrc/onf_wgrad.hip) reads, and the contract of out4.
// NOT here, but written out once in each of the two .hip files, so a change to one needs the same change in the other:
//  * the point load with record words 0..3 (ux, uy, 1, theta), and the logit / BCE loss / rho / record words 4..11 block.
//    As shared functions they raise SGPR spills under hipcc 7.2: fp32 training kernels 80 -> 82..88, fp32 planner kernels
//    0 -> 2 (<13,1,0>) and 2 -> 3 (<13,2,0>), VGPR spills of fp32 <7,1,1> 39 -> 41;
//  * the L1 bias init with the skip reset, the w1a / w1b / w1c / ftl / isl lane bases, and the per-wave loss and dW3[:100]
//    partials after the loop.  As shared functions: SGPR spills 0 -> 8 in onf_split_kernel<13|14,1,2>, VGPR spills
//    119 -> 124 in onf_split_kernel<14,2,1>.
//
// State is passed by reference to the callers' register arrays; every function is inlined.  Lane constants (header
// comment of onf_fused.hip): i = lane & 15 the point column, g = lane >> 4 the lane group, colP / colQ the group's column
// base in layouts P / Q.
#pragma once
#include "onf_layout.h"

namespace nfopp {

// ---- a lane's four input features (table rows fte + FTS r, angle flags isa[r]) of NT point tiles; skip += W3b . f -----
// NT == 2: packed pair = the two point tiles;  NT == 1: packed pair = two consecutive k-steps of the single tile
template <int NKT, int NT, bool ANG>
__device__ __forceinline__ void l1_features(const float* fte, const float* isa, const float (&ux)[NT], const float (&uy)[NT],
                                            const float (&th)[NT], float (&skip)[NT], float (&fv)[4][NT]) {
  constexpr int FTS = Lds<NKT>::FTS;
  if (NT == 2) {
    const f32x2 ux2 = {ux[0], ux[NT - 1]}, uy2 = {uy[0], uy[NT - 1]}, th2 = {th[0], th[NT - 1]};
    f32x2 sk = {skip[0], skip[NT - 1]};
    f32x4 isa4 = {0.f, 0.f, 0.f, 0.f};
    if (ANG) isa4 = *reinterpret_cast<const f32x4*>(isa);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x4 e0 = *reinterpret_cast<const f32x4*>(fte + FTS * r);      // wx wx wy wy
      const f32x4 e1 = *reinterpret_cast<const f32x4*>(fte + FTS * r + 4);  // b b fr fr
      const f32x4 e2 = *reinterpret_cast<const f32x4*>(fte + FTS * r + 8);  // qh qh w3b w3b
      const f32x2 wx = {e0.x, e0.y}, wy = {e0.z, e0.w}, bb = {e1.x, e1.y}, fr = {e1.z, e1.w};
      const f32x2 qh = {e2.x, e2.y}, w3 = {e2.z, e2.w};
      const f32x2 v = features2<ANG, false>(wx, wy, bb, fr, qh, splat2(isa4[r]), ux2, uy2, th2);
      sk = fma2(w3, v, sk);
      fv[r][0] = v.x; fv[r][NT - 1] = v.y;
    }
    skip[0] = sk.x; skip[NT - 1] = sk.y;
  } else {
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const float* ea = fte + FTS * r;
      const float* eb = ea + FTS;
      const f32x2 ux2 = splat2(ux[0]), uy2 = splat2(uy[0]), th2 = splat2(th[0]);
      const f32x2 wx = {ea[0], eb[0]}, wy = {ea[2], eb[2]}, bb = {ea[4], eb[4]}, fr = {ea[6], eb[6]};
      const f32x2 qh = {ea[8], eb[8]}, isa2 = {isa[r], isa[r + 1]};
      const f32x2 v = features2<ANG, false>(wx, wy, bb, fr, qh, isa2, ux2, uy2, th2);
      skip[0] = fmaf(ea[10], v.x, skip[0]);
      skip[0] = fmaf(eb[10], v.y, skip[0]);
      fv[r][0] = v.x; fv[r + 1][0] = v.y;
    }
  }
}

// ---- TRAIN: a point's 112-float row of a hidden-side factor matrix (layout Q slots): v = relu(a1) with slot6 = 1 (the ones
// column of h1), or v = dh1 with slot6 = rho;  slot6 sits at (tile 6, g = 0, r = 1) = AUG_HIDDEN_SLOT, the rest of tile 6
// past unit 96 + g is 0
__device__ __forceinline__ void store_factor_row(float* row, int g, const f32x4 (&acc)[HT], float slot6) {
#pragma unroll
  for (int t = 0; t < HT; ++t) {
    f32x4 v = acc[t];
    if (t == 6) v = f32x4{v[0], g == 0 ? slot6 : 0.0f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(row + 16 * t + 4 * g) = v;
  }
}

// ---- forward only: out4 = (logit, 0, 0, 0) ---------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ void store_logits(const OnfKernelArgs& a, int g, const long long (&pidx)[NT],
                                             const float (&logit)[NT]) {
#pragma unroll
  for (int tl = 0; tl < NT; ++tl)
    if (g == 0 && pidx[tl] < a.n_points)
      *reinterpret_cast<f32x4*>(a.out4 + pidx[tl] * 4) = f32x4{logit[tl], 0.f, 0.f, 0.f};
}

// ---- chain rule through the encodings for one input tile: acc holds din = W1^T dh1 + W3b of the lane's four features
// (rows (g, r) <-> table rows fte + FTS r, angle flags isa[r]);  de = din * d feature / d arg, the derivative being the
// next quadrant of the same argument, sin(arg + (qh + 0.5) pi).  !TRAIN: d logit / d pose += de * d arg / d (x, y, theta)
// (spatial features have no theta dependence: fr = 0);  TRAIN: acc <- de, all the fit needs.  Pairs as in l1_features
template <int NKT, int NT, bool TRAIN, bool ANG>
__device__ __forceinline__ void chain_rule_tile(const float* fte, const float* isa, const float (&ux)[NT],
                                                const float (&uy)[NT], const float (&th)[NT], f32x4 (&acc)[NT],
                                                float (&gx)[NT], float (&gy)[NT], float (&gt)[NT]) {
  constexpr int FTS = Lds<NKT>::FTS;
  if (NT == 2) {
    const f32x2 ux2 = {ux[0], ux[NT - 1]}, uy2 = {uy[0], uy[NT - 1]}, th2 = {th[0], th[NT - 1]};
    f32x2 gx2 = {gx[0], gx[NT - 1]}, gy2 = {gy[0], gy[NT - 1]}, gt2 = {gt[0], gt[NT - 1]};
    f32x4 isa4 = {0.f, 0.f, 0.f, 0.f};
    if (ANG) isa4 = *reinterpret_cast<const f32x4*>(isa);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x4 e0 = *reinterpret_cast<const f32x4*>(fte + FTS * r);
      const f32x4 e1 = *reinterpret_cast<const f32x4*>(fte + FTS * r + 4);
      const f32x2 qh = *reinterpret_cast<const f32x2*>(fte + FTS * r + 8);
      const f32x2 wx = {e0.x, e0.y}, wy = {e0.z, e0.w}, bb = {e1.x, e1.y}, fr = {e1.z, e1.w};
      const f32x2 cof = features2<ANG, true>(wx, wy, bb, fr, qh, splat2(isa4[r]), ux2, uy2, th2);
      const f32x2 de = f32x2{acc[0][r], acc[NT - 1][r]} * cof;
      if (TRAIN) {
        acc[0][r] = de.x; acc[NT - 1][r] = de.y;
      } else {
        gx2 = fma2(de, wx, gx2);
        gy2 = fma2(de, wy, gy2);
        if (ANG) gt2 = fma2(de, fr, gt2);
      }
    }
    gx[0] = gx2.x; gx[NT - 1] = gx2.y; gy[0] = gy2.x; gy[NT - 1] = gy2.y; gt[0] = gt2.x; gt[NT - 1] = gt2.y;
  } else {
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const float* ea = fte + FTS * r;
      const float* eb = ea + FTS;
      const f32x2 wx = {ea[0], eb[0]}, wy = {ea[2], eb[2]}, bb = {ea[4], eb[4]}, fr = {ea[6], eb[6]};
      const f32x2 qh = {ea[8], eb[8]}, isa2 = {isa[r], isa[r + 1]};
      const f32x2 ux2 = splat2(ux[0]), uy2 = splat2(uy[0]), th2 = splat2(th[0]);
      const f32x2 cof = features2<ANG, true>(wx, wy, bb, fr, qh, isa2, ux2, uy2, th2);
      const f32x2 de = f32x2{acc[0][r], acc[0][r + 1]} * cof;
      if (TRAIN) {
        acc[0][r] = de.x; acc[0][r + 1] = de.y;
      } else {
        gx[0] = fmaf(de.x, wx.x, gx[0]); gx[0] = fmaf(de.y, wx.y, gx[0]);
        gy[0] = fmaf(de.x, wy.x, gy[0]); gy[0] = fmaf(de.y, wy.y, gy[0]);
        if (ANG) { gt[0] = fmaf(de.x, fr.x, gt[0]); gt[0] = fmaf(de.y, fr.y, gt[0]); }
      }
    }
  }
}

// ---- TRAIN: de of input tile mt into the input-side factor matrix (rows of 16 NKT floats) ----------------------------
template <int NKT, int NT>
__device__ __forceinline__ void store_de_tile(const OnfKernelArgs& a, const long long (&pidx)[NT], int mt, int g,
                                              const f32x4 (&de)[NT]) {
#pragma unroll
  for (int tl = 0; tl < NT; ++tl)
    if (pidx[tl] < a.n_points) *reinterpret_cast<f32x4*>(a.ws_de + pidx[tl] * (16 * NKT) + 16 * mt + 4 * g) = de[tl];
}

// ---- sum the pose gradient over the four lane groups; out4 = (logit, d/dx, d/dy, d/dtheta) in world units -----------
template <int NT>
__device__ __forceinline__ void store_out4(const OnfKernelArgs& a, int g, const long long (&pidx)[NT],
                                           const float (&logit)[NT], float (&gx)[NT], float (&gy)[NT], float (&gt)[NT]) {
#pragma unroll
  for (int tl = 0; tl < NT; ++tl) {
    gx[tl] += __shfl_xor(gx[tl], 16); gx[tl] += __shfl_xor(gx[tl], 32);
    gy[tl] += __shfl_xor(gy[tl], 16); gy[tl] += __shfl_xor(gy[tl], 32);
    gt[tl] += __shfl_xor(gt[tl], 16); gt[tl] += __shfl_xor(gt[tl], 32);
    if (a.out4 && g == 0 && pidx[tl] < a.n_points) {
      f32x4 o = {logit[tl], gx[tl] / a.geom.sigma, gy[tl] / a.geom.sigma, gt[tl]};
      *reinterpret_cast<f32x4*>(a.out4 + pidx[tl] * 4) = o;
    }
  }
}

}  // namespace nfopp
