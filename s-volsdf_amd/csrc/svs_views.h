// World-space geometry seen from a scan's cameras: one definition of each step svs_tsdf.hip, svs_meshview.hip and
// svs_meshpaint.hip must agree on, so that a point lands on the same pixel with the same bits in all of them
// (tests/test_gpu_views.py).  All arithmetic is float64; the units that include this are compiled with -ffp-contract=off.
#pragma once
#include "svs_common.h"

namespace svs {
namespace views {

constexpr int kMaxViews = 16;
constexpr int kMatsPerView = 21;     // K(9) row-major, then rows 0..2 of E(12), float64
constexpr double kBig = 1.7976931348623157e308;      // the largest finite double

__device__ __forceinline__ bool finite(double a) { return __builtin_fabs(a) <= kBig; }               // NaN fails
__device__ __forceinline__ bool finite3(double a, double b, double c) { return finite(a) && finite(b) && finite(c); }
struct Corner { double cx, cy, cz, x, y; };

// cam = E (p,1); pix = K cam; x = pix.x / pix.z, y = pix.y / pix.z.  false: z <= near or something is not finite.
// The volume calls this with near = 0.0, which skips exactly the voxels that `!(cz > 0.0)` followed by nearest_pixel's range
// test skips: a cz, x or y that is not finite cannot pass that range test either (floor keeps an infinity or a NaN, and
// neither lies in [0,W) or [0,H)), and every term of K cam that holds an infinite cz is infinite or NaN, so the quotients are
// NaN and x and y fail with it.  (Its inner loop pays twelve compares for it; profiles/views_refactor.txt has the cost.)
__device__ __forceinline__ bool project(const double* __restrict__ M, double px, double py, double pz, double near, Corner& c) {
  const double* __restrict__ E = M + 9;
  c.cx = E[0] * px + E[1] * py + E[2] * pz + E[3];
  c.cy = E[4] * px + E[5] * py + E[6] * pz + E[7];
  c.cz = E[8] * px + E[9] * py + E[10] * pz + E[11];
  const double qx = M[0] * c.cx + M[1] * c.cy + M[2] * c.cz;
  const double qy = M[3] * c.cx + M[4] * c.cy + M[5] * c.cz;
  const double qz = M[6] * c.cx + M[7] * c.cy + M[8] * c.cz;
  c.x = qx / qz;
  c.y = qy / qz;
  return c.cz > near && finite(c.cz) && finite(c.x) && finite(c.y);     // one flat chain: NaN fails every link
}
__device__ __forceinline__ bool project(const double* __restrict__ M, const float* __restrict__ p, double near, Corner& c) {
  return project(M, (double)p[0], (double)p[1], (double)p[2], near, c);
}

// the pixel a projection falls on: (floor(x + 0.5), floor(y + 0.5)); false outside [0,W) x [0,H) (NaN fails too).
// in_image: the caller has shown 0 <= x <= W-1 and 0 <= y <= H-1 (the painter's step 2), so the test is left out.
__device__ __forceinline__ bool nearest_pixel(const Corner& c, int H, int W, size_t& pix, bool in_image = false) {
  const double fu = __builtin_floor(c.x + 0.5), fv = __builtin_floor(c.y + 0.5);
  if (!in_image && !(fu >= 0.0 && fu < (double)W && fv >= 0.0 && fv < (double)H)) return false;
  pix = (size_t)(int)fv * (size_t)W + (size_t)(int)fu;
  return true;
}
__device__ __forceinline__ bool masked_out(const uint8_t* __restrict__ mask, size_t pix) { return mask && mask[pix] == 0; }
__device__ __forceinline__ bool not_hidden(double d, double z, double rel, double abs_tol) {
  return d == 0.0 || z <= d * (1.0 + rel) + abs_tol;
}

// the three vertex indices of face f; false when one lies outside [0, n_verts)
__device__ __forceinline__ bool face_indices(const int* __restrict__ faces, long long f, int n_verts, int* idx) {
  const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) return false;
  idx[0] = i0; idx[1] = i1; idx[2] = i2;
  return true;
}

// rules 6-7 of svs_mesh_raster at pixel centre (ix, iy): b_k = e_k / A, the float64 depth zc -> is the centre covered?
__device__ __forceinline__ bool barycentrics(const double* x, const double* y, const double* z, double A, int ix, int iy,
                                             double* b, double& zc) {
  const double cx = (double)ix, cy = (double)iy;
  const double e0 = (x[2] - x[1]) * (cy - y[1]) - (y[2] - y[1]) * (cx - x[1]);
  const double e1 = (x[0] - x[2]) * (cy - y[2]) - (y[0] - y[2]) * (cx - x[2]);
  const double e2 = (x[1] - x[0]) * (cy - y[0]) - (y[1] - y[0]) * (cx - x[0]);
  b[0] = e0 / A; b[1] = e1 / A; b[2] = e2 / A;
  zc = 1.0 / (b[0] / z[0] + b[1] / z[1] + b[2] / z[2]);
  return A > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
}

// floor(v + 0.5) as a colour code: NaN and negatives to 0, above 255 to 255
__device__ __forceinline__ uint8_t code_u8(double v) {
  double code = __builtin_floor(v + 0.5);
  code = code >= 0.0 ? code : 0.0;
  code = code > 255.0 ? 255.0 : code;
  return (uint8_t)(int)code;
}
inline int check_views(const char* name, int n_views, int H, int W) {
  if (n_views < 0 || n_views > kMaxViews) {
    set_error("%s: %d views in one launch (at most %d)", name, n_views, kMaxViews); return SVS_ESHAPE;
  }
  if (H < 0 || W < 0 || (long long)H * W == 0 || (long long)H * W > 0x7fffffffLL) {
    set_error("%s: bad view size %d x %d", name, H, W); return SVS_ESHAPE;
  }
  return SVS_OK;
}
// a kernel argument's per-view pointers from a host array that may be NULL or hold NULL entries
template <typename T>
inline void view_pointers(const T* const* src, int n_views, const T** dst) {
  for (int v = 0; v < kMaxViews; ++v) dst[v] = (src && v < n_views) ? src[v] : nullptr;
}

}  // namespace views
}  // namespace svs
