// Steps 1 to 7 of svs_mesh_paint (include/svolsdf_hip.h) for one world-space point: what the photographs of a launch's views
// add to the point's four accumulators.  svs_meshpaint.hip calls it per vertex, svs_meshtexture.hip per texel of an atlas:
// one definition, one order of operations, the same bits in both.  The point and its normal are float64 (a vertex's are its
// float32 values widened).  Also here, for the same reason: the bilinear RGB tap (step 6, and the atlas renderer's) and the
// rule that turns four accumulators into codes (both finish kernels).  The units that include this are compiled with
// -ffp-contract=off.
#pragma once
#include "svs_common.h"
#include "svs_views.h"

namespace svs {
namespace paintgather {

using namespace views;

constexpr int kMaxPower = 8;

struct GatherArgs {
  const double* mats;
  const float* depth;
  const uint8_t* image[kMaxViews];
  const uint8_t* mask[kMaxViews];
  double near, rel, abs_tol, cos_min;
  int n_views, H, W, power, flags;
};

// eye = -R^T t, once per view and workgroup (at least kMaxViews threads); ends with a barrier
__device__ __forceinline__ void load_eyes(const double* __restrict__ mats, int n_views, double (*eye)[3]) {
  if (threadIdx.x < (unsigned)n_views) {
    const double* __restrict__ E = mats + (size_t)threadIdx.x * kMatsPerView + 9;
#pragma unroll
    for (int k = 0; k < 3; ++k) eye[threadIdx.x][k] = -(E[k] * E[3] + E[4 + k] * E[7] + E[8 + k] * E[11]);
  }
  __syncthreads();
}

// the bilinear tap of an (H, W, 3) image at (x, y), 0 <= x <= W - 1 and 0 <= y <= H - 1; the taps past the last column and
// row are the last column and row (their weight is 0 there)
__device__ __forceinline__ void bilinear_rgb(const uint8_t* __restrict__ img, int W, int H, double x, double y, double (&col)[3]) {
  const double x0 = __builtin_floor(x), y0 = __builtin_floor(y);
  const double fx = x - x0, fy = y - y0;
  const int ix0 = (int)x0, iy0 = (int)y0;
  const int ix1 = ix0 + 1 < W ? ix0 + 1 : W - 1, iy1 = iy0 + 1 < H ? iy0 + 1 : H - 1;
  const uint8_t* __restrict__ t00 = img + ((size_t)iy0 * W + ix0) * 3;
  const uint8_t* __restrict__ t01 = img + ((size_t)iy0 * W + ix1) * 3;
  const uint8_t* __restrict__ t10 = img + ((size_t)iy1 * W + ix0) * 3;
  const uint8_t* __restrict__ t11 = img + ((size_t)iy1 * W + ix1) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    col[ch] = ((1.0 - fx) * (double)t00[ch] + fx * (double)t01[ch]) * (1.0 - fy) +
              ((1.0 - fx) * (double)t10[ch] + fx * (double)t11[ch]) * fy;
}

// accumulators with w > 0 -> codes: the best view's colour as it is, the blend's sum over its weight
__device__ __forceinline__ void acc_codes(double r, double g, double b, double w, int flags, uint8_t* __restrict__ code) {
  const bool best = flags & SVS_PAINT_BEST;
  code[0] = code_u8(best ? r : r / w); code[1] = code_u8(best ? g : g / w); code[2] = code_u8(best ? b : b / w);
}

// n: the point's normal when use_normals (the caller has shown it finite and not zero); (r, g, b, wsum): the accumulators
__device__ __forceinline__ void gather(const GatherArgs& a, const double (*eye)[3], double px, double py, double pz, const double* n,
                                       bool use_normals, double& r, double& g, double& b, double& wsum) {
  const bool best = a.flags & SVS_PAINT_BEST;
  const size_t hw = (size_t)a.H * (size_t)a.W;
  for (int view = 0; view < a.n_views; ++view) {
    Corner c; size_t pix;
    if (!project(a.mats + (size_t)view * kMatsPerView, px, py, pz, a.near, c)) continue;             // 1
    if (!(c.x >= 0.0 && c.x <= (double)(a.W - 1) && c.y >= 0.0 && c.y <= (double)(a.H - 1))) continue;   // 2
    if (!nearest_pixel(c, a.H, a.W, pix, true) || masked_out(a.mask[view], pix)) continue;           // 3 (inside after 2)
    if (!not_hidden((double)a.depth[(size_t)view * hw + pix], c.cz, a.rel, a.abs_tol)) continue;     // 4
    double w = 1.0;
    if (use_normals) {                                                                               // 5
      const double tx = eye[view][0] - px, ty = eye[view][1] - py, tz = eye[view][2] - pz;
      double cs = (n[0] * tx + n[1] * ty + n[2] * tz) / __builtin_sqrt(tx * tx + ty * ty + tz * tz);
      if (!(a.flags & SVS_PAINT_ONE_SIDED)) cs = __builtin_fabs(cs);
      if (!(cs >= a.cos_min)) continue;                      // NaN too
      for (int k = 0; k < a.power; ++k) w = w * cs;
    }
    double col[3];
    bilinear_rgb(a.image[view], a.W, a.H, c.x, c.y, col);                                            // 6
    if (best) {                                                                                      // 7
      if (w > wsum) { r = col[0]; g = col[1]; b = col[2]; wsum = w; }
    } else {
      r = r + w * col[0]; g = g + w * col[1]; b = b + w * col[2]; wsum = wsum + w;
    }
  }
}

// the checks of the rules svs_mesh_paint and svs_mesh_atlas_bake share, in svs_mesh_paint's order; SVS_OK or the code
inline int check_rules(const char* name, int n_views, int H, int W, double near, double rel, double abs_tol, double cos_min,
                       int power, int flags) {
  if (int rc = check_views(name, n_views, H, W)) return rc;
  if (!(near > 0.0) || !(rel >= 0.0) || !(abs_tol >= 0.0)) {
    set_error("%s: near must be positive, rel and abs_tol not negative", name); return SVS_EINVAL;
  }
  if (!(cos_min >= 0.0 && cos_min <= 1.0) || power < 0 || power > kMaxPower) {
    set_error("%s: cos_min in [0,1] and power in [0,%d], got %g and %d", name, kMaxPower, cos_min, power); return SVS_EINVAL;
  }
  if (flags & ~(SVS_PAINT_BEST | SVS_PAINT_ONE_SIDED)) { set_error("%s: unknown flags %d", name, flags); return SVS_EINVAL; }
  return SVS_OK;
}

// the kernel argument from checked rules and a non-null `images`; SVS_EINVAL for a view without an image
inline int fill_gather_args(const char* name, GatherArgs& a, const double* mats, int n_views, int H, int W, double near,
                            const float* depth, const uint8_t* const* images, const uint8_t* const* masks, double rel,
                            double abs_tol, double cos_min, int power, int flags) {
  view_pointers(images, n_views, a.image);
  view_pointers(masks, n_views, a.mask);
  for (int v = 0; v < n_views; ++v)
    if (!a.image[v]) { set_error("%s: view %d has no image", name, v); return SVS_EINVAL; }
  a.mats = mats; a.depth = depth;
  a.near = near; a.rel = rel; a.abs_tol = abs_tol; a.cos_min = cos_min;
  a.n_views = n_views; a.H = H; a.W = W; a.power = power; a.flags = flags;
  return SVS_OK;
}

}  // namespace paintgather
}  // namespace svs
