// The cameras of the mesh units (svs_meshview.hip, svs_meshpaint.hip): the per-view matrices, the projection of a vertex and
// the check of a launch's view count and size.  One home, so that a vertex lands on the same pixel with the same bits in the
// rasteriser, the visibility test and the painter.  All arithmetic is float64; the units that include this are compiled
// with -ffp-contract=off.
#pragma once
#include "svs_common.h"

namespace svs {
namespace meshview {

constexpr int kMaxViews = 16;
constexpr int kMatsPerView = 21;     // K(9) row-major, then rows 0..2 of E(12), float64

struct Corner { double cx, cy, cz, x, y; };

// cam = E (p,1); pix = K cam; x = pix.x / pix.z, y = pix.y / pix.z.  false: z <= near or something is not finite.
__device__ __forceinline__ bool project(const double* __restrict__ M, const float* __restrict__ p, double near, Corner& c) {
  const double* __restrict__ E = M + 9;
  const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
  c.cx = E[0] * px + E[1] * py + E[2] * pz + E[3];
  c.cy = E[4] * px + E[5] * py + E[6] * pz + E[7];
  c.cz = E[8] * px + E[9] * py + E[10] * pz + E[11];
  const double qx = M[0] * c.cx + M[1] * c.cy + M[2] * c.cz;
  const double qy = M[3] * c.cx + M[4] * c.cy + M[5] * c.cz;
  const double qz = M[6] * c.cx + M[7] * c.cy + M[8] * c.cz;
  c.x = qx / qz;
  c.y = qy / qz;
  const double big = 1.7976931348623157e308;
  return c.cz > near && __builtin_fabs(c.cz) <= big && __builtin_fabs(c.x) <= big && __builtin_fabs(c.y) <= big;   // NaN fails
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

}  // namespace meshview
}  // namespace svs
