// Truncated signed distance (TSDF) fusion of filtered depth maps for gfx950 (svs_hip.tsdf): the volume between
// fusion.fuse_view's per-view depth and svs_hip.mesh.marching_cubes.  The reference has no such step; the arithmetic is
// this project's, fixed in include/svolsdf_hip.h and restated in tests/tsdf_oracle.py.
//
// svs_tsdf_integrate is the hot kernel: one read-modify-write pass over the volume per launch, the view loop inside
// the thread, the sums of a launch in float64 registers, one rounding to float32 per launch.  The volume is walked as a
// flat array, four consecutive voxels of the last axis per lane: 16 B loads and stores wherever the arrays allow it
// (a group may run over a row end; every voxel carries its own (i,j,k)), a scalar group at the end.  The camera matrices
// are read with a view index that is uniform over the wave (scalar loads), the depth maps and images are gathers that
// neighbouring voxels share.  40 B of volume traffic per observed voxel with colours, 16 B without; no LDS, no atomics.
// All camera arithmetic is float64 without contraction; the projection and the pixel rule are those of svs_views.h.
#include "svs_common.h"
#include "svs_views.h"

namespace svs {
namespace tsdf {

using namespace views;
constexpr int kGroup = 4;            // voxels per lane

struct IntegrateArgs {
  float* tsdf;                       // (n0,n1,n2)
  float* weight;                     // (n0,n1,n2)
  float* rgb;                        // (3,n0,n1,n2) planar, or nullptr
  const float* depth[kMaxViews];     // (H,W) each
  const uint8_t* mask[kMaxViews];    // (H,W) each or nullptr
  const float* img[kMaxViews];       // (H,W,3) each; all given when rgb is
  const double* mats;                // device, n_views * kMatsPerView
  long long n1, n2, total;
  int n_views, H, W;
  int vec_tw, vec_rgb;               // 16 B accesses allowed on tsdf / weight, on the colour planes
  double ox, oy, oz, voxel, trunc;
};

__device__ __forceinline__ void load4(const float* p, bool vec, int count, float* o) {
  if (vec && count == kGroup) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < kGroup; ++e) o[e] = e < count ? p[e] : 0.0f;
  }
}

__device__ __forceinline__ void store4(float* p, bool vec, int count, const float* o, const bool* wr) {
  if (vec && count == kGroup && wr[0] && wr[1] && wr[2] && wr[3]) {
    f32x4 v; v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
#pragma unroll
    for (int e = 0; e < kGroup; ++e)
      if (e < count && wr[e]) p[e] = o[e];
  }
}

template <bool kColor>
__global__ __launch_bounds__(256) void integrate_kernel(IntegrateArgs a) {
  const long long first = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * kGroup;
  if (first >= a.total) return;
  const long long left = a.total - first;
  const int count = left < kGroup ? (int)left : kGroup;
  // (i,j,k) of the group's first voxel; the others step along the last axis and carry over
  const long long row = first / a.n2;
  long long k = first - row * a.n2;
  long long i = row / a.n1;
  long long j = row - i * a.n1;

  double px[kGroup], py[kGroup], pz[kGroup];
#pragma unroll
  for (int e = 0; e < kGroup; ++e) {
    px[e] = a.ox + (double)i * a.voxel;
    py[e] = a.oy + (double)j * a.voxel;
    pz[e] = a.oz + (double)k * a.voxel;
    if (++k == a.n2) { k = 0; if (++j == a.n1) { j = 0; ++i; } }
  }

  double st[kGroup], sn[kGroup], sc[kGroup][3];
#pragma unroll
  for (int e = 0; e < kGroup; ++e) { st[e] = 0.0; sn[e] = 0.0; sc[e][0] = sc[e][1] = sc[e][2] = 0.0; }

  for (int v = 0; v < a.n_views; ++v) {
    const double* __restrict__ M = a.mats + (size_t)v * kMatsPerView;      // uniform over the wave
    const float* __restrict__ depth = a.depth[v];
    const uint8_t* __restrict__ mask = a.mask[v];
    const float* __restrict__ img = a.img[v];
#pragma unroll
    for (int e = 0; e < kGroup; ++e) {
      if (e >= count) continue;
      Corner c; size_t pix;
      if (!project(M, px[e], py[e], pz[e], 0.0, c) || !nearest_pixel(c, a.H, a.W, pix) || masked_out(mask, pix)) continue;
      const float d = depth[pix];
      if (!(d > 0.0f) || d == __builtin_inff()) continue;                                     // NaN, <= 0, inf
      const double sdf = (double)d - c.cz;
      if (sdf < -a.trunc) continue;
      const double t = sdf / a.trunc;
      st[e] += t < 1.0 ? t : 1.0;
      sn[e] += 1.0;
      if (kColor) {
#pragma unroll
        for (int c = 0; c < 3; ++c) sc[e][c] += (double)img[pix * 3 + c];
      }
    }
  }

  bool wr[kGroup];
  bool any = false;
#pragma unroll
  for (int e = 0; e < kGroup; ++e) { wr[e] = sn[e] > 0.0; any = any || wr[e]; }
  if (!any) return;                                       // an unobserved group is neither read nor written

  float t_old[kGroup], w_old[kGroup], out[kGroup];
  double wn[kGroup];
  load4(a.tsdf + first, a.vec_tw, count, t_old);
  load4(a.weight + first, a.vec_tw, count, w_old);
#pragma unroll
  for (int e = 0; e < kGroup; ++e) {
    wn[e] = (double)w_old[e] + sn[e];
    out[e] = wr[e] ? (float)(((double)w_old[e] * (double)t_old[e] + st[e]) / wn[e]) : t_old[e];
  }
  store4(a.tsdf + first, a.vec_tw, count, out, wr);
  if (kColor) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* plane = a.rgb + (size_t)c * (size_t)a.total + first;
      float c_old[kGroup];
      load4(plane, a.vec_rgb, count, c_old);
#pragma unroll
      for (int e = 0; e < kGroup; ++e)
        out[e] = wr[e] ? (float)(((double)w_old[e] * (double)c_old[e] + sc[e][c]) / wn[e]) : c_old[e];
      store4(plane, a.vec_rgb, count, out, wr);
    }
  }
#pragma unroll
  for (int e = 0; e < kGroup; ++e) out[e] = wr[e] ? (float)wn[e] : w_old[e];
  store4(a.weight + first, a.vec_tw, count, out, wr);
}

// keep[f] = every one of the eight nodes of the face's cell has weight >= min_weight
__global__ __launch_bounds__(256) void face_keep_kernel(const float* __restrict__ weight, long long n0, long long n1, long long n2,
                                                        const int* __restrict__ cells, int n_faces, float min_weight,
                                                        uint8_t* __restrict__ keep) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  const long long node = cells[f];
  bool ok = node >= 0 && node < n0 * n1 * n2;
  if (ok) {
    const long long row = node / n2, k = node - row * n2, i = row / n1, j = row - i * n1;
    ok = i + 1 < n0 && j + 1 < n1 && k + 1 < n2;          // a node on an upper face stands for no cell
    if (ok) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const long long at = ((i + (c >> 2)) * n1 + (j + ((c >> 1) & 1))) * n2 + (k + (c & 1));
        ok = ok && weight[at] >= min_weight;              // NaN weights fail
      }
    }
  }
  keep[f] = ok ? 1 : 0;
}

// trilinear colour of a vertex given in index units, over the nodes that were observed
__global__ __launch_bounds__(256) void vertex_colors_kernel(const float* __restrict__ rgb, const float* __restrict__ weight,
                                                            long long n0, long long n1, long long n2,
                                                            const float* __restrict__ verts, int n_verts, float* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_verts) return;
  const double x[3] = {(double)verts[(size_t)v * 3], (double)verts[(size_t)v * 3 + 1], (double)verts[(size_t)v * 3 + 2]};
  const long long n[3] = {n0, n1, n2};
  long long b[3];
  double f[3];
  bool finite = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    finite = finite && __builtin_fabs(x[d]) < 4.0e18;     // NaN and infinities fail
    double fl = finite ? __builtin_floor(x[d]) : 0.0;
    fl = fl < 0.0 ? 0.0 : (fl > (double)(n[d] - 2) ? (double)(n[d] - 2) : fl);
    b[d] = (long long)fl;
    f[d] = x[d] - fl;
  }
  double acc[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
  if (finite) {
    const size_t total = (size_t)n0 * (size_t)n1 * (size_t)n2;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int d0 = c >> 2, d1 = (c >> 1) & 1, d2 = c & 1;
      const size_t at = (size_t)(((b[0] + d0) * n1 + (b[1] + d1)) * n2 + (b[2] + d2));
      if (!(weight[at] > 0.0f)) continue;
      const double w = (d0 ? f[0] : 1.0 - f[0]) * (d1 ? f[1] : 1.0 - f[1]) * (d2 ? f[2] : 1.0 - f[2]);
      wsum += w;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] += w * (double)rgb[(size_t)ch * total + at];
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[(size_t)v * 3 + ch] = wsum != 0.0 ? (float)(acc[ch] / wsum) : 0.0f;
}

}  // namespace tsdf
}  // namespace svs

using namespace svs;
using namespace svs::tsdf;

extern "C" {

int svs_tsdf_integrate(float* tsdf_vol, float* weight, float* rgb, int n0, int n1, int n2, const double* origin, double voxel,
                       double trunc, const float* const* depths, const uint8_t* const* masks, const float* const* images,
                       const double* mats, int n_views, int H, int W, void* hip_stream) {
  if (!tsdf_vol || !weight || !origin || (n_views > 0 && (!depths || !mats)) || (n_views > 0 && rgb && !images)) {
    set_error("svs_tsdf_integrate: null argument"); return SVS_EINVAL;
  }
  if (n_views < 0 || n_views > kMaxViews) {
    set_error("svs_tsdf_integrate: %d views in one launch (at most %d)", n_views, kMaxViews); return SVS_ESHAPE;
  }
  if (n0 < 1 || n1 < 1 || n2 < 1 || H < 0 || W < 0 || (long long)H * W == 0) {
    set_error("svs_tsdf_integrate: bad sizes (volume %d x %d x %d, views %d x %d)", n0, n1, n2, H, W); return SVS_ESHAPE;
  }
  if (!(voxel > 0.0) || !(trunc > 0.0)) { set_error("svs_tsdf_integrate: voxel and trunc must be positive"); return SVS_EINVAL; }
  if (n_views == 0) return SVS_OK;
  IntegrateArgs a;
  a.tsdf = tsdf_vol; a.weight = weight; a.rgb = rgb; a.mats = mats;
  view_pointers(depths, n_views, a.depth);
  view_pointers(masks, n_views, a.mask);
  view_pointers(rgb ? images : nullptr, n_views, a.img);
  for (int v = 0; v < n_views; ++v)
    if (!a.depth[v] || (rgb && !a.img[v])) { set_error("svs_tsdf_integrate: null depth map or image of view %d", v); return SVS_EINVAL; }
  a.n1 = n1; a.n2 = n2; a.total = (long long)n0 * n1 * n2;
  a.n_views = n_views; a.H = H; a.W = W;
  a.vec_tw = (((uintptr_t)tsdf_vol | (uintptr_t)weight) & 15u) == 0;
  a.vec_rgb = rgb && ((uintptr_t)rgb & 15u) == 0 && (a.total & 3) == 0;      // the planes start total floats apart
  a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2]; a.voxel = voxel; a.trunc = trunc;
  const long long groups = (a.total + kGroup - 1) / kGroup;
  const long long blocks = (groups + 255) / 256;
  if (blocks > 0x7fffffffLL) { set_error("svs_tsdf_integrate: volume too large for one launch"); return SVS_ESHAPE; }
  hipStream_t s = (hipStream_t)hip_stream;
  if (rgb) integrate_kernel<true><<<(unsigned)blocks, 256, 0, s>>>(a);
  else integrate_kernel<false><<<(unsigned)blocks, 256, 0, s>>>(a);
  return check_launch("svs_tsdf_integrate");
}

int svs_tsdf_face_keep(const float* weight, int n0, int n1, int n2, const int* cells, int n_faces, float min_weight,
                       uint8_t* keep, void* hip_stream) {
  if (n_faces == 0) return SVS_OK;
  if (!weight || !cells || !keep) { set_error("svs_tsdf_face_keep: null argument"); return SVS_EINVAL; }
  if (n_faces < 0 || n0 < 2 || n1 < 2 || n2 < 2 || (long long)n0 * n1 * n2 > 0x7fffffffLL) {
    set_error("svs_tsdf_face_keep: bad sizes (two nodes along every axis, int32 node indices)"); return SVS_ESHAPE;
  }
  face_keep_kernel<<<(n_faces + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(weight, n0, n1, n2, cells, n_faces, min_weight, keep);
  return check_launch("svs_tsdf_face_keep");
}

int svs_tsdf_vertex_colors(const float* rgb, const float* weight, int n0, int n1, int n2, const float* verts, int n_verts,
                           float* out, void* hip_stream) {
  if (n_verts == 0) return SVS_OK;
  if (!rgb || !weight || !verts || !out) { set_error("svs_tsdf_vertex_colors: null argument"); return SVS_EINVAL; }
  if (n_verts < 0 || n0 < 2 || n1 < 2 || n2 < 2) {
    set_error("svs_tsdf_vertex_colors: bad sizes (two nodes along every axis)"); return SVS_ESHAPE;
  }
  vertex_colors_kernel<<<(n_verts + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(rgb, weight, n0, n1, n2, verts, n_verts, out);
  return check_launch("svs_tsdf_vertex_colors");
}

}  // extern "C"
