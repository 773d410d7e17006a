// The image work of the MVS loader for gfx950 (datasets/general_eval.py:157-176, 220-232, 254, 267-268 and
// runner.py:106): read_img's code / 255, scale_mvs_input's cv2.resize(img, (W,H), interpolation=cv2.INTER_CUBIC) once or
// twice, the transpose to planes and the alpha split, for V views of one size per call.  Restated in float64 in
// tests/mvsdata_oracle.py.
//
// A source is either 8-bit codes or float32 (the second pass of the x2_mvsres chain reads what the first wrote).  A
// code's value is read_img's np.float32(code) / 255. -- a float32 DIVISION, where svs_scene.hip multiplies by
// float32(1/255): the two differ by one ulp at some codes.  The 256 values come from the host as a device table
// (numpy's own division), so nothing here depends on how the device divides; each workgroup keeps the table in LDS.
//
// svs_mvs_resize_cubic: the resize alone, channel-last, C = 3 or 4.  Coordinates, tap clamping, Keys' weights (A = -0.75,
//   host tables: svs_hip/images.py::cubic_table) and the order of operations are svs_scene_resize_cubic's: rows first,
//   h_r = ((p0 c0 + p1 c1) + p2 c2) + p3 c3 for the four source rows, then the same sum down the rows, float32, no fma
//   contraction.  Equal sizes: a copy of the values (cv2.resize to the same size copies).
// svs_mvs_resize_pack: the same resize with the sample's layout as its output: planes imgs (V,3,H,W) and masks
//   (V,1,H,W); C = 4: rgb times the resized alpha and the resized alpha itself -- the product AFTER the resize, as
//   imgs[:,:3]*imgs[:,3:] is -- C = 3: rgb and ones.  The channel-last result is never written.
// svs_mvs_codes: np.clip(img * 255, 0, 255).astype(np.uint8) of planes (3,H,W) to (H,W,3): a float32 multiply, the
//   clip, truncation toward zero (NaN, which numpy leaves to the platform's cast: 0).
//
// All three are memory-bound: one pass over the input (the 16 taps of neighbouring pixels overlap in cache), one thread
// per destination pixel, consecutive threads along W, so every plane is written in full wavefront-wide runs.
#include "svs_image.h"

namespace svs {
namespace mvsdata {

using namespace svs::image;

constexpr int kThreads = 256;
constexpr int kCodes = 256;

struct ResizeArgs {
  const void* src;                                      // (V,Hs,Ws,C) uint8 or float32
  const float* table;                                   // (256): the value of every code (uint8 source)
  Axis4 x, y;                                           // (W), (H)
  float* out;                                           // resize: (V,H,W,C).  pack: imgs (V,3,H,W)
  float* masks;                                         // pack: (V,1,H,W)
  int Hs, Ws, H, W;
  int same;                                             // equal sizes: no taps
};

template <typename T> struct Value;
template <> struct Value<uint8_t> {
  const float* lut;
  __device__ __forceinline__ float operator()(uint8_t c) const { return lut[c]; }
};
template <> struct Value<float> {
  __device__ __forceinline__ float operator()(float v) const { return v; }
};

// the C channels of destination pixel (x, y) of view v
template <typename T, int C>
__device__ __forceinline__ void resize_pixel(const ResizeArgs& a, const Value<T>& val, int v, int y, int x, float* px) {
  const T* img = (const T*)a.src + (size_t)v * a.Hs * a.Ws * C;
  if (a.same) {
    const T* p = img + ((size_t)y * a.Ws + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) px[c] = val(p[c]);
    return;
  }
  const Taps4 tx = taps4(a.x, x, a.Ws), ty = taps4(a.y, y, a.Hs);
  float h[4][C];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const T* row = img + (size_t)ty.i[r] * a.Ws * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float p0 = val(row[tx.i[0] * C + c]), p1 = val(row[tx.i[1] * C + c]);
      const float p2 = val(row[tx.i[2] * C + c]), p3 = val(row[tx.i[3] * C + c]);
      h[r][c] = ((p0 * tx.w[0] + p1 * tx.w[1]) + p2 * tx.w[2]) + p3 * tx.w[3];
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) px[c] = ((h[0][c] * ty.w[0] + h[1][c] * ty.w[1]) + h[2][c] * ty.w[2]) + h[3][c] * ty.w[3];
}

template <typename T> __device__ __forceinline__ Value<T> make_value(const float* table, float* lds);
template <> __device__ __forceinline__ Value<uint8_t> make_value<uint8_t>(const float* table, float* lds) {
  static_assert(kThreads == kCodes, "one table entry per thread");
  lds[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  return Value<uint8_t>{lds};
}
template <> __device__ __forceinline__ Value<float> make_value<float>(const float*, float*) { return Value<float>{}; }

// grid: (ceil(W / kThreads), H, V).  PACK: planes and the alpha split; otherwise channel-last
template <typename T, int C, bool PACK>
__global__ __launch_bounds__(kThreads) void resize_kernel(ResizeArgs a) {
  __shared__ float lut[kCodes];
  const Value<T> val = make_value<T>(a.table, lut);     // (every thread of the block reaches the barrier in it)
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y, v = blockIdx.z;
  if (x >= a.W) return;
  float px[C];
  resize_pixel<T, C>(a, val, v, y, x, px);
  if (PACK) {
    const size_t plane = (size_t)a.H * a.W, at = (size_t)y * a.W + x;
    float* img = a.out + (size_t)v * 3 * plane + at;
    const float alpha = C == 4 ? px[C - 1] : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) img[c * plane] = C == 4 ? px[c] * alpha : px[c];
    a.masks[(size_t)v * plane + at] = alpha;
  } else {
    float* out = a.out + (((size_t)v * a.H + y) * a.W + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = px[c];
  }
}

// grid: (ceil(W / kThreads), H)
__global__ __launch_bounds__(kThreads) void codes_kernel(const float* __restrict__ img, uint8_t* __restrict__ codes, int H,
                                                        int W) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const size_t plane = (size_t)H * W, at = (size_t)y * W + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = img[c * plane + at] * 255.0f;
    // np.clip keeps NaN; the comparisons below are false for it and it becomes code 0
    codes[at * 3 + c] = s >= 255.0f ? (uint8_t)255 : (s > 0.0f ? (uint8_t)(int)s : (uint8_t)0);
  }
}

template <bool PACK>
int launch(const char* what, const void* src, int src_is_float, const float* table, int V, int Hs, int Ws, int C, int H,
           int W, const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* out, float* masks,
           void* hip_stream) {
  if (!src || !out || (PACK && !masks)) { set_error("%s: null argument", what); return SVS_EINVAL; }
  if (src_is_float != 0 && src_is_float != 1) { set_error("%s: src_is_float must be 0 or 1", what); return SVS_EINVAL; }
  if (!src_is_float && !table) { set_error("%s: null code table for a source of codes", what); return SVS_EINVAL; }
  if (C != 3 && C != 4) { set_error("%s: C must be 3 or 4", what); return SVS_EINVAL; }
  if (V < 1) { set_error("%s: V must be >= 1", what); return SVS_EINVAL; }
  int rc = check_image(what, "H and W", H, W);
  if (rc || (rc = check_image(what, "Hs and Ws", Hs, Ws)) || (rc = check_grid_dim(what, "V", V)) ||
      (rc = check_grid_dim(what, "H", H)))
    return rc;
  const int same = Hs == H && Ws == W;
  if (!same && (!xofs || !xcoef || !yofs || !ycoef)) { set_error("%s: null table", what); return SVS_EINVAL; }
  ResizeArgs a{src, table, {xofs, xcoef}, {yofs, ycoef}, out, masks, Hs, Ws, H, W, same};
  const dim3 grid((W + kThreads - 1) / kThreads, H, V);
  hipStream_t s = (hipStream_t)hip_stream;
  if (src_is_float) {
    if (C == 3) resize_kernel<float, 3, PACK><<<grid, kThreads, 0, s>>>(a);
    else resize_kernel<float, 4, PACK><<<grid, kThreads, 0, s>>>(a);
  } else {
    if (C == 3) resize_kernel<uint8_t, 3, PACK><<<grid, kThreads, 0, s>>>(a);
    else resize_kernel<uint8_t, 4, PACK><<<grid, kThreads, 0, s>>>(a);
  }
  return check_launch(what);
}

}  // namespace mvsdata
}  // namespace svs

using namespace svs;
using namespace svs::mvsdata;

extern "C" {

int svs_mvs_resize_cubic(const void* src, int src_is_float, const float* code_table, int V, int Hs, int Ws, int C, int H,
                         int W, const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* out,
                         void* hip_stream) {
  return launch<false>("svs_mvs_resize_cubic", src, src_is_float, code_table, V, Hs, Ws, C, H, W, xofs, xcoef, yofs, ycoef,
                       out, nullptr, hip_stream);
}

int svs_mvs_resize_pack(const void* src, int src_is_float, const float* code_table, int V, int Hs, int Ws, int C, int H,
                        int W, const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* imgs,
                        float* masks, void* hip_stream) {
  return launch<true>("svs_mvs_resize_pack", src, src_is_float, code_table, V, Hs, Ws, C, H, W, xofs, xcoef, yofs, ycoef,
                      imgs, masks, hip_stream);
}

int svs_mvs_codes(const float* img, int H, int W, uint8_t* codes, void* hip_stream) {
  const char* what = "svs_mvs_codes";
  if (!img || !codes) { set_error("%s: null argument", what); return SVS_EINVAL; }
  int rc = check_image(what, "H and W", H, W);
  if (rc || (rc = check_grid_dim(what, "H", H))) return rc;
  codes_kernel<<<dim3((W + kThreads - 1) / kThreads, H), kThreads, 0, (hipStream_t)hip_stream>>>(img, codes, H, W);
  return check_launch(what);
}

}  // extern "C"
