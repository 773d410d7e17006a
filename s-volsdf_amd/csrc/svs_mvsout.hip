// What the reference's runner does with OpenCV / scikit-image between the MVS network and the point cloud, for gfx950:
// the evaluation mask of filter_depth (runner.py:362-368) and the confidence map that filter_depth thresholds
// (runner.py:267-271).  Restated in numpy / scipy in tests/mvsout_oracle.py.
//
// svs_mask_dilate_disk = skimage.morphology.binary_dilation(mask, disk(radius)) (runner.py:365) =
//   scipy.ndimage.binary_dilation(mask != 0, structure=disk(radius)), border value 0.  disk(r) is x^2 + y^2 <= r^2 on the
//   integer grid: row dy of the footprint is the span |dx| <= isqrt(r^2 - dy^2), and, the disc being symmetric, column dx
//   is the span |dy| <= isqrt(r^2 - dx^2).  The kernel works on BIT-PACKED rows (one 64-bit word per 64 pixels, bit = x mod
//   64): with B_k = the OR of the rows y - h(k) .. y + h(k), h(k) = isqrt(r^2 - k^2), the result row is
//   OR_{k = -r..r} (B_|k| shifted by k).  k runs from r down to 0, h(k) only grows, so B is one running OR: 2r + 1 row
//   reads of three words (the word and its two neighbours; r <= 32 < 64) and 2r + 1 double-word shifts per 64 pixels,
//   against (2r+1)^2-ish taps per pixel of the direct form.  Three launches: pack (one wave-64 ballot per word), dilate
//   (one thread per word), unpack.  A pure boolean function of the input: bit-exact.
// svs_mask_resize_any = cv2.resize(mask * 1., (W,H)) > 0. (runner.py:366-368; float64 INTER_LINEAR).  Inputs and weights
//   are non-negative, so nothing cancels: a destination pixel is set iff one of its 2x2 taps is set and that tap's row
//   weight and column weight are both non-zero.  Taps and weights: svs_hip/images.py::linear_table (tap indices clamped one
//   by one).  Equal sizes: mask != 0.
// svs_mvs_confidence = conf_1 * conf_2 * photometric_confidence of the three maps resized to (H,W) with cv2.resize
//   (INTER_LINEAR, float32; runner.py:267-271): per map the horizontal pass S[x0] a0 + S[x1] a1 on the two source rows,
//   then R0 b0 + R1 b1, every product and sum rounded to float32 on its own (__fmul_rn / __fadd_rn: no fma), a map that
//   already has the size (H,W) taken as it is; out = (r1 * r2) * r3.  One launch.  UNPINNED against OpenCV, whose float32
//   path may contract to fma depending on its build (INTEGRATION.md gives the cv2 call to check it against).
//
// All of it is bandwidth-trivial (2 MB per 1200x1600 mask; the packed rows of a mask are 240 KB and stay in L2).
#include "svs_image.h"

namespace svs {
namespace mvsout {

using namespace svs::image;

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxRadius = 32;                          // < 64: a shifted word needs its direct neighbours only

struct Disk { unsigned char h[kMaxRadius + 1]; };       // h[k] = isqrt(r^2 - k^2), k = 0..r

// one wave per word: lane l holds pixel 64 q + l.  grid: (ceil(Wq / 4), Hs, V)
__global__ __launch_bounds__(kThreads) void pack_kernel(const uint8_t* __restrict__ mask, unsigned long long* __restrict__ bits,
                                                       int Hs, int Ws, int Wq) {
  const int q = blockIdx.x * (kThreads / kWave) + (threadIdx.x / kWave);
  if (q >= Wq) return;                                  // the whole wave leaves
  const int lane = threadIdx.x & (kWave - 1), x = q * kWave + lane;
  const size_t row = (size_t)blockIdx.z * Hs + blockIdx.y;
  const bool set = x < Ws && mask[row * Ws + x] != 0;
  const unsigned long long word = __ballot(set);        // bits beyond Ws stay 0: the border value
  if (lane == 0) bits[row * Wq + q] = word;
}

// one thread per destination word
__global__ __launch_bounds__(kThreads) void dilate_kernel(const unsigned long long* __restrict__ src,
                                                         unsigned long long* __restrict__ dst, int V, int Hs, int Wq,
                                                         int radius, Disk disk) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)V * Hs * Wq) return;
  const int q = (int)(i % Wq), y = (int)((i / Wq) % Hs);
  const unsigned long long* img = src + (i / ((size_t)Wq * Hs)) * (size_t)Hs * Wq;
  unsigned long long L = 0, C = 0, R = 0, res = 0;      // the running OR of the rows y - have .. y + have
  int have = -1;
  for (int k = radius; k >= 0; --k) {
    const int h = disk.h[k];
    while (have < h) {
      ++have;
      for (int side = 0; side < (have ? 2 : 1); ++side) {
        const int yy = side ? y + have : y - have;
        if (yy < 0 || yy >= Hs) continue;
        const unsigned long long* row = img + (size_t)yy * Wq;
        C |= row[q];
        if (q > 0) L |= row[q - 1];
        if (q + 1 < Wq) R |= row[q + 1];
      }
    }
    if (k == 0) res |= C;
    else res |= (C << k) | (L >> (64 - k)) | (C >> k) | (R << (64 - k));
  }
  dst[i] = res;
}

// grid: (ceil(Ws / kThreads), Hs, V)
__global__ __launch_bounds__(kThreads) void unpack_kernel(const unsigned long long* __restrict__ bits, uint8_t* __restrict__ out,
                                                         int Hs, int Ws, int Wq) {
  const int x = blockIdx.x * kThreads + threadIdx.x;
  if (x >= Ws) return;
  const size_t row = (size_t)blockIdx.z * Hs + blockIdx.y;
  out[row * Ws + x] = (uint8_t)((bits[row * Wq + (x >> 6)] >> (x & 63)) & 1ull);
}

struct ResizeArgs {
  const uint8_t* src;                                   // (V,Hs,Ws)
  Axis2 x, y;                                           // (W), (H)
  uint8_t* dst;                                         // (V,H,W)
  int Hs, Ws, H, W;
};

// grid: (ceil(W / kThreads), H, V)
__global__ __launch_bounds__(kThreads) void resize_any_kernel(ResizeArgs a) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y, v = blockIdx.z;
  if (x >= a.W) return;
  const Taps2 tx = taps2(a.x, x, a.Ws), ty = taps2(a.y, y, a.Hs);
  const uint8_t* img = a.src + (size_t)v * a.Hs * a.Ws;
  const uint8_t* r0 = img + (size_t)ty.i0 * a.Ws;
  const uint8_t* r1 = img + (size_t)ty.i1 * a.Ws;
  const bool cx0 = tx.w0 != 0.0f, cx1 = tx.w1 != 0.0f, cy0 = ty.w0 != 0.0f, cy1 = ty.w1 != 0.0f;
  const bool h0 = (cx0 && r0[tx.i0] != 0) || (cx1 && r0[tx.i1] != 0);
  const bool h1 = (cx0 && r1[tx.i0] != 0) || (cx1 && r1[tx.i1] != 0);
  a.dst[((size_t)v * a.H + y) * a.W + x] = (uint8_t)((cy0 && h0) || (cy1 && h1));
}

__global__ __launch_bounds__(kThreads) void nonzero_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) dst[i] = (uint8_t)(src[i] != 0);
}

struct ConfMap {
  const float* src;                                     // (Hk,Wk)
  Axis2 x, y;                                           // (W), (H); unused when the map has the size (H,W)
  int Hk, Wk;
};
struct ConfArgs { ConfMap m[3]; float* dst; int H, W; };

__device__ __forceinline__ float resized(const ConfMap& m, int x, int y, int H, int W) {
  if (m.Hk == H && m.Wk == W) return m.src[(size_t)y * W + x];
  const Taps2 tx = taps2(m.x, x, m.Wk), ty = taps2(m.y, y, m.Hk);
  const float* r0 = m.src + (size_t)ty.i0 * m.Wk;
  const float* r1 = m.src + (size_t)ty.i1 * m.Wk;
  const float h0 = __fadd_rn(__fmul_rn(r0[tx.i0], tx.w0), __fmul_rn(r0[tx.i1], tx.w1));
  const float h1 = __fadd_rn(__fmul_rn(r1[tx.i0], tx.w0), __fmul_rn(r1[tx.i1], tx.w1));
  return __fadd_rn(__fmul_rn(h0, ty.w0), __fmul_rn(h1, ty.w1));
}

// grid: (ceil(W / kThreads), H)
__global__ __launch_bounds__(kThreads) void confidence_kernel(ConfArgs a) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
  if (x >= a.W) return;
  const float c1 = resized(a.m[0], x, y, a.H, a.W), c2 = resized(a.m[1], x, y, a.H, a.W);
  const float c3 = resized(a.m[2], x, y, a.H, a.W);
  a.dst[(size_t)y * a.W + x] = __fmul_rn(__fmul_rn(c1, c2), c3);
}

inline int isqrt_int(int n) {
  int s = 0;
  while ((s + 1) * (s + 1) <= n) ++s;
  return s;
}

// an image whose rows are a launch-grid dimension
inline int check_rows(const char* what, const char* names, int H, int W) {
  const int rc = check_image(what, names, H, W);
  return rc ? rc : check_grid_dim(what, "the number of rows", H);
}

inline size_t words_per_row(int Ws) { return ((size_t)Ws + kWave - 1) / kWave; }

}  // namespace mvsout
}  // namespace svs

using namespace svs;
using namespace svs::mvsout;

extern "C" {

size_t svs_mask_dilate_workspace_bytes(int V, int Hs, int Ws) {
  if (V < 1 || Hs < 1 || Ws < 1) return 0;
  return 2 * (size_t)V * (size_t)Hs * words_per_row(Ws) * sizeof(unsigned long long);
}

int svs_mask_dilate_disk(const uint8_t* mask, int V, int Hs, int Ws, int radius, void* workspace, uint8_t* out,
                         void* hip_stream) {
  const char* what = "svs_mask_dilate_disk";
  if (!mask || !workspace || !out) { set_error("%s: null argument", what); return SVS_EINVAL; }
  if (((uintptr_t)workspace & 7) != 0) { set_error("%s: workspace must be 8-byte aligned", what); return SVS_EINVAL; }
  if (radius < 0 || radius > kMaxRadius) { set_error("%s: radius must be in 0..%d", what, kMaxRadius); return SVS_EINVAL; }
  int rc = check_count(what, "V", V, kMaxGridDim);
  if (rc || (rc = check_rows(what, "Hs and Ws", Hs, Ws))) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const int Wq = (int)words_per_row(Ws);
  const size_t n_words = (size_t)V * Hs * Wq;
  if ((n_words + kThreads - 1) / kThreads > 0x7fffffffull) { set_error("%s: V*Hs*Ws too large", what); return SVS_ESHAPE; }
  unsigned long long* packed = (unsigned long long*)workspace;
  unsigned long long* dilated = packed + n_words;
  Disk disk{};
  for (int k = 0; k <= radius; ++k) disk.h[k] = (unsigned char)isqrt_int(radius * radius - k * k);
  const int per_block = kThreads / kWave;
  pack_kernel<<<dim3((Wq + per_block - 1) / per_block, Hs, V), kThreads, 0, s>>>(mask, packed, Hs, Ws, Wq);
  if ((rc = check_launch("svs_mask_dilate_disk(pack)"))) return rc;
  dilate_kernel<<<(unsigned)((n_words + kThreads - 1) / kThreads), kThreads, 0, s>>>(packed, dilated, V, Hs, Wq, radius, disk);
  if ((rc = check_launch("svs_mask_dilate_disk(dilate)"))) return rc;
  unpack_kernel<<<dim3((Ws + kThreads - 1) / kThreads, Hs, V), kThreads, 0, s>>>(dilated, out, Hs, Ws, Wq);
  return check_launch("svs_mask_dilate_disk(unpack)");
}

int svs_mask_resize_any(const uint8_t* mask, int V, int Hs, int Ws, int H, int W, const int* xofs, const float* xcoef,
                        const int* yofs, const float* ycoef, uint8_t* out, void* hip_stream) {
  const char* what = "svs_mask_resize_any";
  if (!mask || !out) { set_error("%s: null argument", what); return SVS_EINVAL; }
  int rc = check_count(what, "V", V, kMaxGridDim);
  if (rc || (rc = check_rows(what, "Hs and Ws", Hs, Ws)) || (rc = check_rows(what, "H and W", H, W))) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  if (Hs == H && Ws == W) {
    const size_t n = (size_t)V * H * W;
    if ((n + kThreads - 1) / kThreads > 0x7fffffffull) { set_error("%s: V*H*W too large", what); return SVS_ESHAPE; }
    nonzero_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(mask, out, n);
    return check_launch(what);
  }
  if (!xofs || !xcoef || !yofs || !ycoef) { set_error("%s: null table", what); return SVS_EINVAL; }
  ResizeArgs a{mask, {xofs, xcoef}, {yofs, ycoef}, out, Hs, Ws, H, W};
  resize_any_kernel<<<dim3((W + kThreads - 1) / kThreads, H, V), kThreads, 0, s>>>(a);
  return check_launch(what);
}

int svs_mvs_confidence(const float* conf1, int H1, int W1, const int* xofs1, const float* xcoef1, const int* yofs1,
                       const float* ycoef1, const float* conf2, int H2, int W2, const int* xofs2, const float* xcoef2,
                       const int* yofs2, const float* ycoef2, const float* conf3, int H3, int W3, const int* xofs3,
                       const float* xcoef3, const int* yofs3, const float* ycoef3, int H, int W, float* out,
                       void* hip_stream) {
  const char* what = "svs_mvs_confidence";
  ConfArgs a{{{conf1, {xofs1, xcoef1}, {yofs1, ycoef1}, H1, W1}, {conf2, {xofs2, xcoef2}, {yofs2, ycoef2}, H2, W2},
              {conf3, {xofs3, xcoef3}, {yofs3, ycoef3}, H3, W3}}, out, H, W};
  if (!conf1 || !conf2 || !conf3 || !out) { set_error("%s: null argument", what); return SVS_EINVAL; }
  int rc = check_rows(what, "H and W", H, W);
  if (rc) return rc;
  for (const ConfMap& m : a.m) {
    if ((rc = check_rows(what, "every map's size", m.Hk, m.Wk))) return rc;
    if ((m.Hk != H || m.Wk != W) && (!m.x.ofs || !m.x.coef || !m.y.ofs || !m.y.coef)) {
      set_error("%s: null table of a map that is resized", what); return SVS_EINVAL;
    }
  }
  confidence_kernel<<<dim3((W + kThreads - 1) / kThreads, H), kThreads, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch(what);
}

}  // extern "C"
