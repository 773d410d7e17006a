// What the Chamfer evaluators do before and after the neighbour searches, for gfx950.
//
// Reference: evals/eval_bmvs.py:127-134,196-197 -- the float32 bookkeeping of the BlendedMVS clouds (`astype('float32')`,
// scan 5's scale_mat, the in-place division by the relative scale) -- and the colour step of the error clouds that both
// scripts share, evals/eval_bmvs.py:232-246 and evals/eval_dtu.py:173-187.  The searches themselves are csrc/svs_cloud.hip.
//
// Both kernels are one lane per point, a few flops per 24 to 48 bytes: HBM-bound streams, no shared memory, no matrix
// cores.  Built with -ffp-contract=off: every product and sum below rounds on its own, as numpy's do.
#include "svs_common.h"

namespace svs {
namespace chamfer {

struct Mat34 { double m[12]; };                   // rows 0..2 of the homogeneous (4,4) matrix

// data_pcd.astype('float32') then `/= relative_scale` (a float32 array divided in place by a Python float stays float32:
// one IEEE float32 division by (float)scale); the kd-tree then reads the result as float64.
template <typename T>
__global__ void prepare_scale_kernel(const T* __restrict__ pts, size_t n3, float scale, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  out[i] = (double)__fdiv_rn((float)pts[i], scale);
}

// scan 5: transform_points promotes the float32 cloud to float64, t = M [p;1] row by row, then `/= relative_scale` in
// float64.  The sums run left to right; the reference's order is its BLAS's.
template <typename T>
__global__ void prepare_matrix_kernel(const T* __restrict__ pts, size_t n, Mat34 M, double scale, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double p0 = (double)(float)pts[3 * i], p1 = (double)(float)pts[3 * i + 1], p2 = (double)(float)pts[3 * i + 2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t = ((M.m[4 * a] * p0 + M.m[4 * a + 1] * p1) + M.m[4 * a + 2] * p2) + M.m[4 * a + 3];
    out[3 * i + a] = t / scale;
  }
}

// R * a + W * (1 - a) with R = (1,0,0), W = (1,1,1) as numpy evaluates it: (a + (1 - a), 1 - a, 1 - a); rows the
// evaluation left out stay blue, distances >= max_dist (inf included) turn green.
__global__ void error_colors_kernel(const double* __restrict__ dist, const uint8_t* __restrict__ select, const int* __restrict__ rank,
                                    size_t n_dist, size_t n_full, double max_dist, double vis_dist, double* __restrict__ rgb_f64,
                                    uint8_t* __restrict__ rgb_u8) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_full) return;
  double r, g, b;
  const size_t j = !select ? i : (select[i] ? (size_t)rank[i] : n_dist);
  if (j >= n_dist) {                              // not evaluated (or a rank that does not belong to dist: never read)
    r = 0.0; g = 0.0; b = 1.0;
  } else {
    const double d = dist[j];
    if (d >= max_dist) {
      r = 0.0; g = 1.0; b = 0.0;
    } else {
      const double a = (d < vis_dist ? d : vis_dist) / vis_dist;
      const double w = 1.0 - a;
      r = a + w; g = w; b = w;
    }
  }
  if (rgb_f64) { rgb_f64[3 * i] = r; rgb_f64[3 * i + 1] = g; rgb_f64[3 * i + 2] = b; }
  if (rgb_u8) {
    const double c[3] = {r, g, b};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = c[k] < 0.0 ? 0.0 : (c[k] > 1.0 ? 1.0 : c[k]);
      rgb_u8[3 * i + k] = (uint8_t)__builtin_rint(v * 255.0);
    }
  }
}

}  // namespace chamfer
}  // namespace svs

using namespace svs;
using namespace svs::chamfer;

extern "C" {

int svs_cloud_prepare(const void* pts, int is_f64, int n, const double* matrix, double scale, double* out, void* hip_stream) {
  if (n < 0 || !(scale > 0.0) || (n > 0 && (!pts || !out))) { set_error("svs_cloud_prepare: bad argument (need scale > 0)"); return SVS_EINVAL; }
  if (n == 0) return SVS_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  if (!matrix) {
    const size_t n3 = 3 * (size_t)n;
    const unsigned blocks = (unsigned)((n3 + 255) / 256);
    if (is_f64) prepare_scale_kernel<double><<<blocks, 256, 0, s>>>((const double*)pts, n3, (float)scale, out);
    else prepare_scale_kernel<float><<<blocks, 256, 0, s>>>((const float*)pts, n3, (float)scale, out);
  } else {
    Mat34 M;
    for (int k = 0; k < 12; ++k) M.m[k] = matrix[k];          // HOST double[16], row-major; the last row is not used
    const unsigned blocks = (unsigned)(((size_t)n + 255) / 256);
    if (is_f64) prepare_matrix_kernel<double><<<blocks, 256, 0, s>>>((const double*)pts, (size_t)n, M, scale, out);
    else prepare_matrix_kernel<float><<<blocks, 256, 0, s>>>((const float*)pts, (size_t)n, M, scale, out);
  }
  return check_launch("svs_cloud_prepare");
}

int svs_cloud_error_colors(const double* dist, int n_dist, const uint8_t* select, const int* rank, int n_full, double max_dist,
                           double vis_dist, double* rgb_f64, uint8_t* rgb_u8, void* hip_stream) {
  if (n_dist < 0 || n_full < 0 || n_dist > n_full || (n_dist > 0 && !dist) || !(vis_dist > 0.0) || !(max_dist == max_dist)) {
    set_error("svs_cloud_error_colors: bad argument (need 0 <= n_dist <= n_full, vis_dist > 0)"); return SVS_EINVAL;
  }
  if (select ? !rank : n_full != n_dist) { set_error("svs_cloud_error_colors: select needs rank; without select n_full == n_dist"); return SVS_EINVAL; }
  if (n_full == 0 || (!rgb_f64 && !rgb_u8)) return SVS_OK;
  const unsigned blocks = (unsigned)(((size_t)n_full + 255) / 256);
  error_colors_kernel<<<blocks, 256, 0, (hipStream_t)hip_stream>>>(dist, select, rank, (size_t)n_dist, (size_t)n_full, max_dist, vis_dist, rgb_f64, rgb_u8);
  return check_launch("svs_cloud_error_colors");
}

}  // extern "C"
