// Scene loading for gfx950 (volsdf/datasets/scene_dataset.py:163-206): the image work SceneDataset does per view with
// OpenCV -- the bicubic resize of the image, its Gaussian-smoothed copy and the resize of the mask -- for a batch of V
// views of one size per call.  Restated in float64 in tests/scene_oracle.py.
//
// svs_scene_resize_cubic = cv2.resize(code * (1/255), (W,H), interpolation=cv2.INTER_CUBIC) of 8-bit RGB codes: the
//   shared 4x4 gather of svs_resize.h (coordinates, clamping, order of operations: there) with ScaledCode as its
//   code-to-float rule.  load_rgb's img_as_float32 MULTIPLIES the code by float32 (1/255) (it does not divide; the two
//   differ by one ulp at some codes): so does this.  Equal sizes: code * (1/255) alone (the reference skips the resize).
// svs_scene_smooth = cv2.GaussianBlur(img, (31,31), 90): separable, 31 float32 weights (exp(-(i-15)^2 / (2 90^2))
//   normalised in float64, rounded to float32: 0.03197 .. 0.03242), BORDER_REFLECT_101 on both axes, rows first, then
//   columns, float32 intermediate (the workspace).  Each pass sums as OpenCV's symmetric filters do: w15 x0 +
//   sum_k w(15+k) (x(+k) + x(-k)), k = 1..15 in order.  One LDS tile with a 15-pixel halo per workgroup and axis.
//   H, W >= 16: a single reflection covers the halo (svs_image.h::reflect101_once).
// svs_scene_mask = the reference's cv2.resize(mask, (W,H), cv2.INTER_NEAREST) followed by > 0.5.  The third POSITIONAL
//   parameter of cv2.resize is dst, not interpolation, so the interpolation that runs is the default INTER_LINEAR
//   (UNPINNED: no OpenCV at hand to confirm it): 2 taps per axis, the same coordinate rule, indices
//   clamped, tables of the first index and two float32 weights from the host (svs_hip/images.py::linear_table).  The
//   8-bit single-channel input is divided by `divisor` in float32 first (1 for a 0/1 mask, 255 for the BlendedMVS alpha
//   channel, which the reference interpolates before it thresholds); the 0/1 result goes to all three channels.
//
// All three are bandwidth-trivial (about 20 MB of traffic per 576x768 view); plain vector loads and stores.
#include "svs_resize.h"

namespace svs {
namespace scene {

using namespace svs::image;

constexpr int kThreads = 256;
constexpr int kR = 15;                                  // Gaussian radius: ksize 31
constexpr int kTaps = 2 * kR + 1;
constexpr int kMinSize = kR + 1;                        // one REFLECT_101 reflection covers the halo
// rows pass: a tile of kRowW consecutive floats (channel-interleaved, so the halo is 3 * kR floats) of kRowH rows
constexpr int kRowW = 256, kRowH = 8, kRowHalo = 3 * kR;
// columns pass: kColW consecutive floats of kColH rows, kR rows of halo above and below
constexpr int kColW = 64, kColH = 64, kColPer = kColH / (kThreads / kColW);

struct Weights { float w[kR + 1]; };                    // w[k]: the weight at distance k from the centre

struct MaskArgs {
  const uint8_t* src;                                   // (V,Hs,Ws)
  Axis2 x, y;                                           // (W), (H)
  float* dst;                                           // (V,H,W,3)
  int Hs, Ws, H, W;
  float divisor;
};

__global__ __launch_bounds__(kThreads) void mask_kernel(MaskArgs a) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y, v = blockIdx.z;
  if (x >= a.W) return;
  const Taps2 tx = taps2(a.x, x, a.Ws), ty = taps2(a.y, y, a.Hs);
  const uint8_t* img = a.src + (size_t)v * a.Hs * a.Ws;
  const uint8_t* r0 = img + (size_t)ty.i0 * a.Ws;
  const uint8_t* r1 = img + (size_t)ty.i1 * a.Ws;
  const float h0 = ((float)r0[tx.i0] / a.divisor) * tx.w0 + ((float)r0[tx.i1] / a.divisor) * tx.w1;
  const float h1 = ((float)r1[tx.i0] / a.divisor) * tx.w0 + ((float)r1[tx.i1] / a.divisor) * tx.w1;
  const float m = (h0 * ty.w0 + h1 * ty.w1) > 0.5f ? 1.0f : 0.0f;
  float* out = a.dst + (((size_t)v * a.H + y) * a.W + x) * 3;
  out[0] = m; out[1] = m; out[2] = m;
}

// rows pass.  grid: (ceil(3W / kRowW), ceil(H / kRowH), V)
__global__ __launch_bounds__(kThreads) void smooth_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int H,
                                                              int W, Weights wt) {
  __shared__ float tile[kRowH][kRowW + 2 * kRowHalo];
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * kRowW, y0 = blockIdx.y * kRowH;
  const size_t img = (size_t)blockIdx.z * H * W * 3;
  const int WF = 3 * W;
  for (int i = tid; i < kRowH * (kRowW + 2 * kRowHalo); i += kThreads) {
    const int r = i / (kRowW + 2 * kRowHalo), j = i - r * (kRowW + 2 * kRowHalo);
    const int e = e0 - kRowHalo + j;                    // >= -45
    const int px = (e + 3 * kR) / 3 - kR, ch = e - 3 * px;
    const int y = y0 + r;
    float val = 0.0f;                                   // beyond what any pixel of the image reads
    if (y < H && px < W + kR) val = src[img + (size_t)y * WF + reflect101_once(px, W) * 3 + ch];
    tile[r][j] = val;
  }
  __syncthreads();
  const int e = e0 + tid;
  if (e >= WF) return;
#pragma unroll 1
  for (int r = 0; r < kRowH; ++r) {
    if (y0 + r >= H) break;
    const float* t = &tile[r][tid + kRowHalo];
    float acc = wt.w[0] * t[0];
#pragma unroll
    for (int k = 1; k <= kR; ++k) acc += wt.w[k] * (t[3 * k] + t[-3 * k]);
    dst[img + (size_t)(y0 + r) * WF + e] = acc;
  }
}

// columns pass.  grid: (ceil(3W / kColW), ceil(H / kColH), V)
__global__ __launch_bounds__(kThreads) void smooth_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, int H,
                                                              int W, Weights wt) {
  __shared__ float tile[kColH + 2 * kR][kColW];
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * kColW, y0 = blockIdx.y * kColH;
  const size_t img = (size_t)blockIdx.z * H * W * 3;
  const int WF = 3 * W;
  for (int i = tid; i < (kColH + 2 * kR) * kColW; i += kThreads) {
    const int r = i / kColW, c = i - r * kColW;
    const int y = y0 - kR + r, e = e0 + c;
    float val = 0.0f;
    if (e < WF && y < H + kR) val = src[img + (size_t)reflect101_once(y, H) * WF + e];
    tile[r][c] = val;
  }
  __syncthreads();
  const int c = tid & (kColW - 1), e = e0 + c;
  if (e >= WF) return;
  const int rb = (tid / kColW) * kColPer;
#pragma unroll 1
  for (int q = 0; q < kColPer; ++q) {
    const int r = rb + q, y = y0 + r;
    if (y >= H) break;
    float acc = wt.w[0] * tile[r + kR][c];
#pragma unroll
    for (int k = 1; k <= kR; ++k) acc += wt.w[k] * (tile[r + kR + k][c] + tile[r + kR - k][c]);
    dst[img + (size_t)y * WF + e] = acc;
  }
}

inline Weights gaussian_weights() {
  // cv2.getGaussianKernel(31, 90, CV_32F): exp(-(i-15)^2 / (2 sigma^2)) in float64, times 1 / their sum, then float32
  double g[kTaps], sum = 0.0;
  for (int i = 0; i < kTaps; ++i) { const double d = i - kR; g[i] = std::exp(-(d * d) / (2.0 * 90.0 * 90.0)); sum += g[i]; }
  const double scale = 1.0 / sum;
  Weights w;
  for (int k = 0; k <= kR; ++k) w.w[k] = (float)(g[kR + k] * scale);
  return w;
}

// V views of (H,W): H, W >= 16 (the 31-tap filter reflects once); V and H are launch-grid dimensions
inline int check_dst(const char* what, int V, int H, int W) {
  if (V < 1) { set_error("%s: V must be >= 1", what); return SVS_EINVAL; }
  int rc = check_image(what, "H and W", H, W, kMinSize);
  if (rc || (rc = check_grid_dim(what, "V", V))) return rc;
  return check_grid_dim(what, "H", H);
}

}  // namespace scene
}  // namespace svs

using namespace svs;
using namespace svs::scene;

extern "C" {

size_t svs_scene_workspace_bytes(int V, int H, int W) {
  if (V < 1 || H < kMinSize || W < kMinSize) return 0;
  return (size_t)V * (size_t)H * (size_t)W * 3 * sizeof(float);
}

int svs_scene_resize_cubic(const uint8_t* codes, int V, int Hs, int Ws, int H, int W, const int* xofs, const float* xcoef,
                           const int* yofs, const float* ycoef, float* out, void* hip_stream) {
  const char* what = "svs_scene_resize_cubic";
  if (!codes || !out) { set_error("%s: null argument", what); return SVS_EINVAL; }
  int rc = check_dst(what, V, H, W);
  if (rc || (rc = check_image(what, "Hs and Ws", Hs, Ws))) return rc;
  return launch_resize<ScaledCode, 3, false>(what, codes, nullptr, V, Hs, Ws, H, W, xofs, xcoef, yofs, ycoef, out, nullptr,
                                             hip_stream);
}

int svs_scene_smooth(const float* img, int V, int H, int W, void* workspace, float* out, void* hip_stream) {
  const char* what = "svs_scene_smooth";
  if (!img || !workspace || !out) { set_error("%s: null argument", what); return SVS_EINVAL; }
  int rc = check_dst(what, V, H, W);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const Weights w = gaussian_weights();
  float* tmp = (float*)workspace;
  const int WF = 3 * W;
  smooth_rows_kernel<<<dim3((WF + kRowW - 1) / kRowW, (H + kRowH - 1) / kRowH, V), kThreads, 0, s>>>(img, tmp, H, W, w);
  if ((rc = check_launch("svs_scene_smooth(rows)"))) return rc;
  smooth_cols_kernel<<<dim3((WF + kColW - 1) / kColW, (H + kColH - 1) / kColH, V), kThreads, 0, s>>>(tmp, out, H, W, w);
  return check_launch("svs_scene_smooth(columns)");
}

int svs_scene_mask(const uint8_t* mask, float divisor, int V, int Hs, int Ws, int H, int W, const int* xofs,
                   const float* xcoef, const int* yofs, const float* ycoef, float* out, void* hip_stream) {
  const char* what = "svs_scene_mask";
  if (!mask || !xofs || !xcoef || !yofs || !ycoef || !out) { set_error("%s: null argument", what); return SVS_EINVAL; }
  if (!(divisor > 0.0f)) { set_error("%s: divisor must be positive", what); return SVS_EINVAL; }
  int rc = check_dst(what, V, H, W);
  if (rc || (rc = check_image(what, "Hs and Ws", Hs, Ws))) return rc;
  MaskArgs a{mask, {xofs, xcoef}, {yofs, ycoef}, out, Hs, Ws, H, W, divisor};
  mask_kernel<<<dim3((W + kThreads - 1) / kThreads, H, V), kThreads, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch(what);
}

}  // extern "C"
