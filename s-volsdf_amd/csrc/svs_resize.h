// The 4x4 cubic gather of both scan loaders (svs_scene.hip, svs_mvsdata.hip): cv2.resize(img, (W,H),
// interpolation=cv2.INTER_CUBIC) of V channel-last views of one size.  The one place where the arithmetic lives.
//
// A separable 4-tap filter (Keys' cubic, A = -0.75), source coordinate (d + 0.5) * scale - 0.5, every tap index clamped
// to the image on its own, no prefilter when shrinking.  As OpenCV does, the HOST builds one table per axis (the first
// tap's index and four float32 coefficients per destination column / row: svs_hip/images.py::cubic_table) and the kernel
// only gathers: rows first, h_r = ((p0 c0 + p1 c1) + p2 c2) + p3 c3 for the four source rows, then the same sum down the
// rows, float32, no fma contraction (both translation units are built with -ffp-contract=off).  Equal sizes: the values
// alone, no taps (cv2.resize to the same size copies; the scene loader's reference skips the call).
//
// What differs between the loaders is how a source element becomes a float, a functor:
//   TableCode   uint8 -> table[code], the 256 values from the host; each workgroup keeps them in LDS.  The MVS loader's
//               read_img divides, np.float32(code) / 255., and numpy's own quotients are what the table holds.
//   Identity    float32 as it is: the second pass of the MVS loader's x2_mvsres chain reads what the first wrote.
//   ScaledCode  uint8 -> (float)code * (1.0f / 255.0f), no table: the scene loader's load_rgb (img_as_float32) multiplies.
//               The product and the quotient differ by one ulp at 126 of the 256 codes.
//
// Memory-bound: one pass over the input (the 16 taps of neighbouring pixels overlap in cache), one thread per destination
// pixel and all its channels, consecutive threads along W, so every plane is written in full wavefront-wide runs.
#pragma once
#include "svs_image.h"

namespace svs {
namespace image {

constexpr int kResizeThreads = 256;
constexpr int kCodes = 256;

struct ResizeArgs {
  const void* src;                                      // (V,Hs,Ws,C) uint8 or float32
  const float* table;                                   // (256): the value of every code (TableCode)
  Axis4 x, y;                                           // (W), (H): first tap = ofs[d] (may lie outside: clamped)
  float* out;                                           // resize: (V,H,W,C).  pack: imgs (V,3,H,W)
  float* masks;                                         // pack: (V,1,H,W)
  int Hs, Ws, H, W;
};

// ---- how a source element becomes a float.  make() runs once per thread before any early return ---------------------
struct TableCode {
  typedef uint8_t Src;
  const float* lut;
  __device__ __forceinline__ float operator()(uint8_t c) const { return lut[c]; }
  static __device__ __forceinline__ TableCode make(const float* table) {
    static_assert(kResizeThreads == kCodes, "one table entry per thread");
    __shared__ float lds[kCodes];
    lds[threadIdx.x] = table[threadIdx.x];
    __syncthreads();                                    // every thread of the block reaches it
    return TableCode{lds};
  }
};
struct Identity {
  typedef float Src;
  __device__ __forceinline__ float operator()(float v) const { return v; }
  static __device__ __forceinline__ Identity make(const float*) { return Identity{}; }
};
struct ScaledCode {
  typedef uint8_t Src;
  __device__ __forceinline__ float operator()(uint8_t c) const { return (float)c * (1.0f / 255.0f); }
  static __device__ __forceinline__ ScaledCode make(const float*) { return ScaledCode{}; }
};

// the C channels of destination pixel (x, y) of view v.  SAME: equal sizes, no taps
template <typename Val, int C, bool SAME>
__device__ __forceinline__ void resize_pixel(const ResizeArgs& a, const Val& val, int v, int y, int x, float* px) {
  typedef typename Val::Src T;
  const T* img = (const T*)a.src + (size_t)v * a.Hs * a.Ws * C;
  if (SAME) {
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

// grid: (ceil(W / kResizeThreads), H, V).  PACK: planes imgs (V,3,H,W) and masks (V,1,H,W) -- C = 4: rgb times the
// resized alpha and the resized alpha itself, C = 3: rgb and ones; otherwise channel-last (V,H,W,C)
template <typename Val, int C, bool PACK, bool SAME>
__global__ __launch_bounds__(kResizeThreads) void resize_kernel(ResizeArgs a) {
  const Val val = Val::make(a.table);
  const int x = blockIdx.x * kResizeThreads + threadIdx.x, y = blockIdx.y, v = blockIdx.z;
  if (x >= a.W) return;
  float px[C];
  resize_pixel<Val, C, SAME>(a, val, v, y, x, px);
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

// The launch, once the entry point has checked sizes, grid dimensions and pointers; null axis tables: equal sizes only.
template <typename Val, int C, bool PACK>
int launch_resize(const char* what, const void* src, const float* table, int V, int Hs, int Ws, int H, int W,
                  const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* out, float* masks,
                  void* hip_stream) {
  const bool same = Hs == H && Ws == W;
  if (!same && (!xofs || !xcoef || !yofs || !ycoef)) { set_error("%s: null table", what); return SVS_EINVAL; }
  ResizeArgs a{src, table, {xofs, xcoef}, {yofs, ycoef}, out, masks, Hs, Ws, H, W};
  const dim3 grid((W + kResizeThreads - 1) / kResizeThreads, H, V);
  hipStream_t s = (hipStream_t)hip_stream;
  if (same) resize_kernel<Val, C, PACK, true><<<grid, kResizeThreads, 0, s>>>(a);
  else resize_kernel<Val, C, PACK, false><<<grid, kResizeThreads, 0, s>>>(a);
  return check_launch(what);
}

}  // namespace image
}  // namespace svs
