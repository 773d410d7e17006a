// Image-index helpers and argument checks shared by the evaluation-side kernels (svs_scene.hip, svs_mvsout.hip,
// svs_ibr.hip, svs_mvsdata.hip): only index computation and validation live here, every kernel keeps its own arithmetic
// -- but for the cubic resize, which both scan loaders run and svs_resize.h holds once.
#pragma once
#include "svs_common.h"

namespace svs {
namespace image {

constexpr long long kMaxPixels = 1LL << 26;             // per image: pixel offsets times a few channels stay in 32 bits
constexpr int kMaxGridDim = 65535;                      // blockIdx.y / blockIdx.z

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), two forms.
// One reflection: right for -n < v < 2n - 1 only, i.e. for a halo smaller than the image.  The caller guarantees it.
__device__ __forceinline__ int reflect101_once(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }
// Any index and any length >= 1: reflects until the index is inside.
__device__ __forceinline__ int reflect101_any(int p, int len) {
  if (len == 1) return 0;
  while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// One axis of a 2-tap (INTER_LINEAR) resize as the host builds it (svs_hip/images.py::linear_table): the first tap's
// index, which may lie outside the source, and the two float32 weights per destination coordinate.
struct Axis2 {
  const int* ofs;                                       // (dst)
  const float* coef;                                    // (dst,2)
};
struct Taps2 { int i0, i1; float w0, w1; };

// the two source indices of destination coordinate d, each clamped on its own to a source of `len`, and their weights
__device__ __forceinline__ Taps2 taps2(const Axis2& t, int d, int len) {
  const int s = t.ofs[d];
  return {clampi(s, len - 1), clampi(s + 1, len - 1), t.coef[2 * d], t.coef[2 * d + 1]};
}

// One axis of a 4-tap (INTER_CUBIC) resize as the host builds it (svs_hip/images.py::cubic_table): the first tap's
// index (s - 1, it may lie outside the source) and Keys' four float32 weights per destination coordinate.
struct Axis4 {
  const int* ofs;                                       // (dst)
  const float* coef;                                    // (dst,4)
};
struct Taps4 { int i[4]; float w[4]; };

// the four source indices of destination coordinate d, each clamped on its own to a source of `len`, and their weights
__device__ __forceinline__ Taps4 taps4(const Axis4& t, int d, int len) {
  const int s = t.ofs[d];
  Taps4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r.i[k] = clampi(s + k, len - 1);
    r.w[k] = t.coef[4 * d + k];
  }
  return r;
}

// ---- host-side argument checks: each sets the error string, prefixed with the entry point's name ------------------
// both sizes >= min_size and at most 2^26 pixels
inline int check_image(const char* what, const char* names, int H, int W, int min_size = 1) {
  if (H < min_size || W < min_size || (long long)H * W > kMaxPixels) {
    set_error("%s: %s must be >= %d with at most 2^26 pixels", what, names, min_size); return SVS_ESHAPE;
  }
  return SVS_OK;
}

// a size that becomes blockIdx.y or blockIdx.z
inline int check_grid_dim(const char* what, const char* name, int n) {
  if (n > kMaxGridDim) { set_error("%s: %s must be <= 65535 (the launch grid)", what, name); return SVS_ESHAPE; }
  return SVS_OK;
}

// a number of views / sources
inline int check_count(const char* what, const char* name, int n, int hi) {
  if (n < 1 || n > hi) { set_error("%s: %s must be in 1..%d", what, name, hi); return SVS_EINVAL; }
  return SVS_OK;
}

}  // namespace image
}  // namespace svs
