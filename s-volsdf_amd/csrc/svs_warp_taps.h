// The projection of a reference-view voxel into a source view, shared by the cost-volume builders: the variance volume of
// CasMVSNet / UCSNet (csrc/svs_costvol.hip) and the similarity volume of TransMVSNet (csrc/svs_transmvs.hip).  One struct for
// the per-source launch arguments, the host function that fills it, the device function that turns a voxel into its four
// bilinear corners, and the dispatch over the number of source views.
#pragma once
#include "svs_common.h"
#include <type_traits>

namespace svs {
namespace warp {

constexpr int kMaxSrc = 4;

struct SourceViews {
  const float* src_hwc[kMaxSrc];  // (H,W,C) source-view features
  float rot[kMaxSrc][9];          // src_proj @ inv(ref_proj), rows
  float trans[kMaxSrc][3];
};

// rot_trans: a HOST array, 9 rot + 3 trans floats per source.  Entries beyond n_src repeat source 0 (never read by a kernel
// instantiated for n_src sources, but never uninitialised either).
inline int fill_sources(const char* what, SourceViews& sv, const float* const* src_features_hwc, const float* rot_trans, int n_src) {
  if (!src_features_hwc || !rot_trans) { set_error("%s: null argument", what); return SVS_EINVAL; }
  if (n_src < 1 || n_src > kMaxSrc) { set_error("%s: bad sizes", what); return SVS_ESHAPE; }
  for (int v = 0; v < kMaxSrc; ++v) {
    const int u = v < n_src ? v : 0;
    if (!src_features_hwc[u]) { set_error("%s: null source %d", what, u); return SVS_EINVAL; }
    sv.src_hwc[v] = src_features_hwc[u];
    for (int k = 0; k < 9; ++k) sv.rot[v][k] = rot_trans[12 * u + k];
    for (int k = 0; k < 3; ++k) sv.trans[v][k] = rot_trans[12 * u + 9 + k];
  }
  return SVS_OK;
}

// f(std::integral_constant<int, NS>) for NS = n in 1..kMaxSrc: the kernels are instantiated per number of source views
template <class F>
inline void dispatch_n_src(int n, F&& f) {
  switch (n) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

// How the normalised grid coordinate g becomes a pixel coordinate:
//   kHalfPixel     ((g + 1) * size - 1) / 2      CasMVSNet (models/CasMVSNet.py:305-312: normalised with the (W-1)/2 formula,
//                                                sampled with align_corners=False)
//   kAlignCorners  ((g + 1) / 2) * (size - 1)    TransMVSNet (models/module.py:296-321, align_corners=True)
enum Sampling { kHalfPixel, kAlignCorners };

// The four bilinear corners of voxel (x, y, depth) in source view v: weights w4 (0: outside) and BYTE offsets o4 into the
// (H,W,C) feature map.  rot @ [x,y,1] * depth + trans (CasMVSNet.py:300-303), then correctly rounded divisions in the
// reference's operation order: at |coordinate| ~ 300 px one ulp of the quotient already moves a sample by 3e-5 px (once per
// voxel and source: not what bounds the kernels).  Zeros padding: a corner outside contributes nothing (NaN coordinates
// compare false).  Z_GUARD: a hypothesis whose projected z is below 1e-6 (the reference sets its grid coordinates to -99
// there) or is not a number samples nothing.
template <int C, Sampling SAMPLING, bool Z_GUARD>
__device__ __forceinline__ void bilinear_taps(const SourceViews& sv, int v, int x, int y, int H, int W, float depth, f32x4& w4,
                                              i32x4& o4) {
  w4 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  o4 = i32x4{0, 0, 0, 0};
  const float fx = (float)x, fy = (float)y;
  const float* R = sv.rot[v];
  const float qx = ((R[0] * fx + R[1] * fy) + R[2]) * depth + sv.trans[v][0];
  const float qy = ((R[3] * fx + R[4] * fy) + R[5]) * depth + sv.trans[v][1];
  const float qz = ((R[6] * fx + R[7] * fy) + R[8]) * depth + sv.trans[v][2];
  if (Z_GUARD && !(qz >= 1e-6f)) return;
  const float px = qx / qz, py = qy / qz;
  const float gx = px / ((float)(W - 1) / 2.0f) - 1.0f, gy = py / ((float)(H - 1) / 2.0f) - 1.0f;
  const float ix = SAMPLING == kHalfPixel ? ((gx + 1.0f) * (float)W - 1.0f) / 2.0f : ((gx + 1.0f) / 2.0f) * (float)(W - 1);
  const float iy = SAMPLING == kHalfPixel ? ((gy + 1.0f) * (float)H - 1.0f) / 2.0f : ((gy + 1.0f) / 2.0f) * (float)(H - 1);
  const float x0 = __builtin_floorf(ix), y0 = __builtin_floorf(iy);
  const float tx = ix - x0, ty = iy - y0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float xx = x0 + (float)(k & 1), yy = y0 + (float)(k >> 1);
    if (xx >= 0.0f && xx <= (float)(W - 1) && yy >= 0.0f && yy <= (float)(H - 1)) {
      w4[k] = ((k & 1) ? tx : 1.0f - tx) * ((k >> 1) ? ty : 1.0f - ty);
      o4[k] = ((int)yy * W + (int)xx) * (C * 4);
    }
  }
}

}  // namespace warp
}  // namespace svs
