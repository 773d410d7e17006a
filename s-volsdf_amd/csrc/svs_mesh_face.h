// The triangle rule of the mesh units that reshape a mesh (svs_meshsimplify.hip, svs_meshsmooth.hip): a face is valid when
// its three indices lie in [0, n_verts), its nine coordinates are finite and the length of cross(P1 - P0, P2 - P0), in
// float64 of the widened float32 corners, is finite and not zero.  The arithmetic stands here once, in one order; the units
// that include it are compiled with -ffp-contract=off.  (svs_meshpaint.hip, svs_mesh.hip, svs_meshview.hip and svs_tsdf.hip
// have rules of their own.)
#pragma once
#include "svs_common.h"

namespace svs {
namespace meshface {

struct Face {
  int i[3];
  double p[3][3];                                           // corners, float32 widened
  double n[3], L;                                           // cross(P1 - P0, P2 - P0) and its length
};

// face f -> t; false when it is not valid (nothing is read through an index outside [0, n_verts))
__device__ __forceinline__ bool load_face(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces, int f, Face& t) {
#pragma unroll
  for (int k = 0; k < 3; ++k) t.i[k] = faces[3 * (size_t)f + k];
  if ((unsigned)t.i[0] >= (unsigned)n_verts || (unsigned)t.i[1] >= (unsigned)n_verts || (unsigned)t.i[2] >= (unsigned)n_verts) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t.p[k][a] = (double)verts[3 * (size_t)t.i[k] + a];
      ok = ok && finite_f64(t.p[k][a]);
    }
  if (!ok) return false;
  const double ux = t.p[1][0] - t.p[0][0], uy = t.p[1][1] - t.p[0][1], uz = t.p[1][2] - t.p[0][2];
  const double vx = t.p[2][0] - t.p[0][0], vy = t.p[2][1] - t.p[0][1], vz = t.p[2][2] - t.p[0][2];
  t.n[0] = uy * vz - uz * vy;
  t.n[1] = uz * vx - ux * vz;
  t.n[2] = ux * vy - uy * vx;
  t.L = __builtin_sqrt(t.n[0] * t.n[0] + t.n[1] * t.n[1] + t.n[2] * t.n[2]);
  return finite_f64(t.L) && t.L > 0.0;
}

}  // namespace meshface
}  // namespace svs
