// A mesh's vertices coloured from a scan's photographs, for gfx950 (svs_hip.meshpaint): area-weighted vertex normals, the
// per-vertex blend (or best view) of the photographs' bilinear taps behind the occlusion test of svs_mesh_vertex_visibility,
// the conversion to codes, and the hole filling over the mesh's edges.  The reference has no such step; the arithmetic is
// this project's, fixed in include/svolsdf_hip.h and restated in tests/meshpaint_oracle.py.
//
// paint_kernel is a gather (svs_paint_gather.h, shared with svs_meshtexture.hip, with the tap and the code rule): one lane per vertex walks the launch's
// views in index order with its four accumulators in registers, so the sum has one fixed order and needs no atomics; two
// runs give the same bits.  The per-view eye (-R^T t) is worked out once per workgroup into LDS.  The normals are a scatter of float64 atomic adds (their last bits
// depend on arrival order: they only weight the views); the hole filling is a scatter of integer atomic adds, which is exact
// in any order.  All camera arithmetic is float64 without contraction; its rules are those of svs_views.h.
#include "svs_common.h"
#include "svs_paint_gather.h"
#include "svs_views.h"

namespace svs {
namespace meshpaint {

using namespace views;
using namespace paintgather;

// ---- normals ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void normal_accumulate_kernel(const float* __restrict__ verts, int n_verts,
                                                                const int* __restrict__ faces, int n_faces, double* accum) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int idx[3];
  if (!face_indices(faces, f, n_verts, idx)) return;
  double p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[k][c] = (double)verts[(size_t)idx[k] * 3 + c];
    if (!finite3(p[k][0], p[k][1], p[k][2])) return;
  }
  const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
  const double vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
  const double n[3] = {uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd(accum + (size_t)idx[k] * 3 + c, n[c]);
}

__global__ __launch_bounds__(256) void normal_finish_kernel(const double* __restrict__ accum, int n_verts,
                                                            float* __restrict__ normals) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_verts) return;
  const double x = accum[(size_t)v * 3], y = accum[(size_t)v * 3 + 1], z = accum[(size_t)v * 3 + 2];
  const double len = __builtin_sqrt(x * x + y * y + z * z);
  const bool unit = finite3(x, y, z) && len > 0.0 && len <= kBig;
  normals[(size_t)v * 3] = unit ? (float)(x / len) : 0.0f;
  normals[(size_t)v * 3 + 1] = unit ? (float)(y / len) : 0.0f;
  normals[(size_t)v * 3 + 2] = unit ? (float)(z / len) : 0.0f;
}

// ---- paint -----------------------------------------------------------------------------------------------------------
struct PaintArgs {
  GatherArgs g;
  const float* verts;
  const float* normals;
  double* acc;
  int n_verts;
};

__global__ __launch_bounds__(256) void paint_kernel(PaintArgs a) {
  __shared__ double eye[kMaxViews][3];
  load_eyes(a.g.mats, a.g.n_views, eye);
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= a.n_verts) return;
  const float* __restrict__ p = a.verts + (size_t)v * 3;
  double n[3] = {0.0, 0.0, 0.0};
  bool lit = true;
  if (a.normals) {
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (double)a.normals[(size_t)v * 3 + k];
    lit = finite3(n[0], n[1], n[2]) && !(n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0);
  }
  double r = a.acc[(size_t)v * 4], g = a.acc[(size_t)v * 4 + 1], b = a.acc[(size_t)v * 4 + 2], wsum = a.acc[(size_t)v * 4 + 3];
  if (lit) gather(a.g, eye, (double)p[0], (double)p[1], (double)p[2], n, a.normals != nullptr, r, g, b, wsum);   // steps 1 to 7
  a.acc[(size_t)v * 4] = r; a.acc[(size_t)v * 4 + 1] = g; a.acc[(size_t)v * 4 + 2] = b; a.acc[(size_t)v * 4 + 3] = wsum;
}

__global__ __launch_bounds__(256) void paint_finish_kernel(const double* __restrict__ acc, int n_verts, int flags,
                                                           uint8_t* __restrict__ rgb, int* __restrict__ painted) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_verts) return;
  const double w = acc[(size_t)v * 4 + 3];
  if (!(w > 0.0)) { painted[v] = 0; return; }
  acc_codes(acc[(size_t)v * 4], acc[(size_t)v * 4 + 1], acc[(size_t)v * 4 + 2], w, flags, rgb + (size_t)v * 3);
  painted[v] = 1;
}

// ---- spread ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spread_gather_kernel(const int* __restrict__ faces, int n_faces, int n_verts, int round,
                                                            const uint8_t* __restrict__ rgb, const int* __restrict__ painted,
                                                            int* work) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  int idx[3];
  if (!face_indices(faces, f, n_verts, idx)) return;
  const int state[3] = {painted[idx[0]], painted[idx[1]], painted[idx[2]]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (!(state[i] > 0 && state[i] <= round)) continue;
    const uint8_t* __restrict__ c = rgb + (size_t)idx[i] * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j == i || state[j] != 0) continue;
      int* at = work + (size_t)idx[j] * 4;
      atomicAdd(at, (int)c[0]); atomicAdd(at + 1, (int)c[1]); atomicAdd(at + 2, (int)c[2]); atomicAdd(at + 3, 1);
    }
  }
}

__global__ __launch_bounds__(256) void spread_apply_kernel(const int* __restrict__ work, int n_verts, int round,
                                                           uint8_t* __restrict__ rgb, int* __restrict__ painted, int* changed) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool filled = false;
  if (v < n_verts) {
    const int count = work[(size_t)v * 4 + 3];
    if (count > 0) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) rgb[(size_t)v * 3 + ch] = (uint8_t)((2 * work[(size_t)v * 4 + ch] + count) / (2 * count));
      painted[v] = round + 1;
      filled = true;
    }
  }
  if (__ballot(filled) && (threadIdx.x & 63) == 0) *changed = 1;          // every writer stores the same value
}

}  // namespace meshpaint
}  // namespace svs

using namespace svs;
using namespace svs::meshpaint;

extern "C" {

int svs_mesh_vertex_normals(const float* verts, int n_verts, const int* faces, int n_faces, double* accum, float* normals,
                            void* hip_stream) {
  if (n_verts < 0 || n_faces < 0) { set_error("svs_mesh_vertex_normals: negative count"); return SVS_ESHAPE; }
  if (n_verts == 0) return SVS_OK;
  if (!verts || !accum || (n_faces > 0 && !faces)) { set_error("svs_mesh_vertex_normals: null argument"); return SVS_EINVAL; }
  hipStream_t s = (hipStream_t)hip_stream;
  if (n_faces > 0) normal_accumulate_kernel<<<(unsigned)((n_faces + 255) / 256), 256, 0, s>>>(verts, n_verts, faces, n_faces, accum);
  if (normals) normal_finish_kernel<<<(unsigned)((n_verts + 255) / 256), 256, 0, s>>>(accum, n_verts, normals);
  return check_launch("svs_mesh_vertex_normals");
}

int svs_mesh_paint(const float* verts, int n_verts, const float* normals, const double* mats, int n_views, int H, int W,
                   double near, const float* depth, const uint8_t* const* images, const uint8_t* const* masks, double rel,
                   double abs_tol, double cos_min, int power, int flags, double* acc, void* hip_stream) {
  if (int rc = check_rules("svs_mesh_paint", n_views, H, W, near, rel, abs_tol, cos_min, power, flags)) return rc;
  if (n_verts < 0) { set_error("svs_mesh_paint: negative count"); return SVS_ESHAPE; }
  if (!images) { set_error("svs_mesh_paint: null argument (images)"); return SVS_EINVAL; }
  if (n_verts == 0 || n_views == 0) return SVS_OK;
  if (!verts || !mats || !depth || !acc) { set_error("svs_mesh_paint: null argument"); return SVS_EINVAL; }
  PaintArgs a;
  if (int rc = fill_gather_args("svs_mesh_paint", a.g, mats, n_views, H, W, near, depth, images, masks, rel, abs_tol, cos_min,
                                power, flags)) return rc;
  a.verts = verts; a.normals = normals; a.acc = acc; a.n_verts = n_verts;
  paint_kernel<<<(n_verts + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch("svs_mesh_paint");
}

int svs_mesh_paint_finish(const double* acc, int n_verts, int flags, uint8_t* rgb, int* painted, void* hip_stream) {
  if (n_verts < 0) { set_error("svs_mesh_paint_finish: negative count"); return SVS_ESHAPE; }
  if (flags & ~(SVS_PAINT_BEST | SVS_PAINT_ONE_SIDED)) { set_error("svs_mesh_paint_finish: unknown flags %d", flags); return SVS_EINVAL; }
  if (n_verts == 0) return SVS_OK;
  if (!acc || !rgb || !painted) { set_error("svs_mesh_paint_finish: null argument"); return SVS_EINVAL; }
  paint_finish_kernel<<<(n_verts + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(acc, n_verts, flags, rgb, painted);
  return check_launch("svs_mesh_paint_finish");
}

int svs_mesh_paint_spread(const int* faces, int n_faces, int n_verts, int round, uint8_t* rgb, int* painted, int* work,
                          int* changed, void* hip_stream) {
  if (n_verts < 0 || n_faces < 0) { set_error("svs_mesh_paint_spread: negative count"); return SVS_ESHAPE; }
  if (round < 1 || round > 0x7ffffffe) { set_error("svs_mesh_paint_spread: round %d (rounds count from 1)", round); return SVS_EINVAL; }
  if (n_verts == 0 || n_faces == 0) return SVS_OK;          // nothing is touched, changed included
  if (!faces || !rgb || !painted || !work || !changed) { set_error("svs_mesh_paint_spread: null argument"); return SVS_EINVAL; }
  hipStream_t s = (hipStream_t)hip_stream;
  if (hipMemsetAsync(changed, 0, sizeof(int), s) != hipSuccess || hipMemsetAsync(work, 0, (size_t)n_verts * 4 * sizeof(int), s) != hipSuccess)
    return check_launch("svs_mesh_paint_spread");
  spread_gather_kernel<<<(unsigned)((n_faces + 255) / 256), 256, 0, s>>>(faces, n_faces, n_verts, round, rgb, painted, work);
  spread_apply_kernel<<<(unsigned)((n_verts + 255) / 256), 256, 0, s>>>(work, n_verts, round, rgb, painted, changed);
  return check_launch("svs_mesh_paint_spread");
}

}  // extern "C"
