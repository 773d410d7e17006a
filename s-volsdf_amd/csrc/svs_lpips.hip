// LPIPS (model net-lin, net vgg, version 0.1) for gfx950: the reference's third novel-view score (eval_vsdf.py:178,
// 208-209 -> lpips_tf.py:29-90, which runs a downloaded frozen graph; the network is restated here from the published
// model, svs_hip/lpips.py holds the definition and its UNPINNED statement).
//
// Convolution: every VGG-16 layer is 3x3 / padding 1 / stride 1, an implicit GEMM on v_mfma_f32_16x16x32_f16 with
// two-piece fp16 operands (fp16x2: hi * hi + hi * mid + mid * hi, float32 accumulation; the scheme of svs_conv2d_mfma.hip):
//   D[cout][pixel] = sum_k W[cout][k] P[k][pixel],  M = 64 output channels per workgroup (4 M tiles), N = an 8 (y) x 16 (x)
//   output window (8 N tiles of 16 consecutive x), K walked in slices of CS input channels x 9 taps.
// Per slice the workgroup (4 waves) stages the 10 x 18 halo window of the slice's channels (channel last, hi and mid piece)
// and the slice's weight fragments (KS k-steps x 4 M tiles x 2 pieces, 1 KiB each) in LDS, then every wave computes two
// output rows x four M tiles: per k-step 8 A and 4 B fragment reads (16 bytes per lane) for 24 MFMAs.  CS = 32: one tap per
// k-step (K = 32 = 4 lane groups x 8 channels), pixel pitch 80 bytes (an odd multiple of 16: conflict-free 16-byte reads at
// pixel stride 1).  CS = 8 (the first layer, 3 channels padded to 8): four taps per k-step, 3 k-steps, pitch 16.
//
// Operand ranges: VGG weights are around 1e-2, so the mid piece of an unscaled weight is an fp16 subnormal.  The
// pack multiplies every output channel by the power of two that brings its largest |w| into [2^13, 2^14) and stores the
// inverse behind the fragments; the epilogue multiplies by it (exact), then adds the bias and applies ReLU.  Activations are
// used unscaled: their hi piece holds up to 65504 and their mid piece is normal down to |x| = 0.125.  An operand that would
// not fit -- a weight, an input value or a layer's output that is the next layer's operand, |v| > 65504 or not a number --
// is replaced by 0 and raises a device flag the entry points read back: SVS_EOVERFLOW, never inf or NaN.
//
// Between layers an activation is "packed": channel last, hi[(y W + x) C + c] as fp16 followed by the mid plane of the same
// shape (4 bytes per value, as float32), written by the epilogue and copied to LDS unconverted by the next layer.  The public
// single-layer entry reads and writes float32 (C,H,W); it converts while it stages.
//
// Head: per pixel one wave forms both channel norms, the weighted squared difference of the unit vectors and adds it to the
// wave's float64 sum; workgroups write partial sums, one finishing launch adds them in a fixed order.  No atomics anywhere:
// a run is bit-identical to the next.
#include "svs_conv_frag.h"
#include <mutex>

namespace svs {
namespace lpips {

using frag::f16x8;
using frag::f16x4;
using frag::f32x4v;
using frag::split;

constexpr int kTY = 8, kTX = 16;                         // output window of a workgroup
constexpr int kHY = kTY + 2, kHX = kTX + 2, kHP = kHY * kHX;
constexpr int kMB = 64;                                  // output channels of a workgroup
constexpr float kF16Max = 65504.0f;
constexpr int kLayers = 13, kTaps = 5;
constexpr int kHeadGrid = 256;                           // most workgroups (partial sums) of one head launch
constexpr int kHeadWaves = 4;

template <int CS> constexpr int k_steps() { return CS == 32 ? 9 : 3; }
template <int CS> constexpr int pitch() { return CS == 32 ? 80 : 16; }
template <int CS> constexpr int slice_frags() { return k_steps<CS>() * 4 * 2 * 64; }       // 16-byte fragments per slice
template <int CS> constexpr int lds_bytes() { return 2 * kHP * pitch<CS>() + slice_frags<CS>() * 16; }

inline int slice_channels(int Cin) { return Cin == 3 ? 8 : 32; }
inline int padded_channels(int Cin) { return Cin == 3 ? 8 : Cin; }
inline bool supported(int Cin, int Cout) {
  const bool ci = Cin == 3 || Cin == 64 || Cin == 128 || Cin == 256 || Cin == 512;
  const bool co = Cout == 64 || Cout == 128 || Cout == 256 || Cout == 512;
  return ci && co;
}
inline size_t frag_bytes(int Cin, int Cout) {
  const int cs = slice_channels(Cin), slices = padded_channels(Cin) / cs;
  return (size_t)(Cout / kMB) * slices * (cs == 32 ? slice_frags<32>() : slice_frags<8>()) * 16;
}

struct ConvArgs {
  const void* in;        // float32 (Cin,H,W), or packed (Cp,H,W)
  const uint4* wfrag;    // [Cout / 64][slices][KS][4 M tiles][2 pieces][64 lanes] 16-byte A fragments
  const float* unscale;  // [Cout] the inverse of the pack's power of two per output channel (behind the fragments)
  const float* bias;     // [Cout] or nullptr
  void* out;             // float32 (Cout,H,W), or packed (Cout,H,W)
  int Cin, Cp, Cout, H, W, relu, tiles_x;
  size_t in_stride, out_stride;   // bytes between the images of a launch (blockIdx.z)
  int* status;           // raised when an operand does not fit fp16
};

template <int CS, bool IN_F32, bool OUT_F32>
__global__ __launch_bounds__(256) void conv3x3_kernel(ConvArgs a) {
  constexpr int KS = k_steps<CS>(), PITCH = pitch<CS>(), PIECE = kHP * PITCH, C8 = CS / 8, WSL = slice_frags<CS>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sx = smem;                                       // [2 pieces][kHP pixels][PITCH]
  uint4* sw = reinterpret_cast<uint4*>(smem + 2 * PIECE);         // [KS][4][2][64]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int vox = lane & 15, kg = lane >> 4;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * kTY, x0 = tx * kTX, cb = blockIdx.y;
  const size_t HW = (size_t)a.H * a.W;
  const int slices = a.Cp / CS;
  const unsigned char* in_b = static_cast<const unsigned char*>(a.in) + blockIdx.z * a.in_stride;
  unsigned char* out_b = static_cast<unsigned char*>(a.out) + blockIdx.z * a.out_stride;

  // the B-fragment address of k-step s inside the halo window: the (tap, channel group) of this lane's 8 elements
  int boff[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    int tap = CS == 32 ? s : 4 * s + kg;
    if (tap > 8) tap = 8;                                         // padded k: the weights are zero there
    const int kh = tap / 3, kw = tap - 3 * kh;
    boff[s] = ((2 * wave + kh) * kHX + (vox + kw)) * PITCH + (CS == 32 ? 16 * kg : 0);
  }

  // Accumulation: with all three products of every k-step chained into one accumulator (216 MFMAs at K = 2304) the result
  // was 1.7e-7 of sum |w||x| off float64, 4.8x what float32 conv2d loses and ten times what the operand split loses: the
  // matrix cores' own additions into a long-running sum dominate (a float32 emulation with round-to-nearest additions in
  // that order gives 0.7e-7, one with truncating additions 8e-7).  So the hi * hi products of one slice (9 MFMAs at most)
  // get a fresh accumulator, which the vector ALU adds to the running sum (round to nearest), and the two cross terms,
  // 2^-11 of the sum, keep a chain of their own for the whole layer (the same emulations: 0.45e-7 even when truncating).
  f32x4v acc[4][2], accs[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) { acc[mt][nt] = (f32x4v)(0.0f); accs[mt][nt] = (f32x4v)(0.0f); }
  bool bad = false;

#pragma unroll 1
  for (int sl = 0; sl < slices; ++sl) {
    // ---- the halo window of this slice's channels -> LDS, zero outside the image
    if (IN_F32) {
      const float* g = reinterpret_cast<const float*>(in_b);
#pragma unroll 1
      for (int i = tid; i < kHP * C8; i += 256) {
        const int c8 = i / kHP, p = i - c8 * kHP;                 // consecutive lanes: consecutive x
        const int ly = p / kHX, lx = p - ly * kHX;
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        const bool ok = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        const size_t o = ok ? (size_t)gy * a.W + gx : 0;
        f16x8 h, m;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = sl * CS + c8 * 8 + j;
          float v = (ok && c < a.Cin) ? g[(size_t)c * HW + o] : 0.0f;
          if (!(__builtin_fabsf(v) <= kF16Max)) { bad = true; v = 0.0f; }
          _Float16 hh, mm;
          split(v, hh, mm);
          h[j] = hh; m[j] = mm;
        }
        *reinterpret_cast<f16x8*>(sx + p * PITCH + 16 * c8) = h;
        *reinterpret_cast<f16x8*>(sx + PIECE + p * PITCH + 16 * c8) = m;
      }
    } else {
      const size_t plane = HW * a.Cp * 2;                         // bytes of the hi plane
#pragma unroll 1
      for (int i = tid; i < 2 * kHP * C8; i += 256) {
        const int piece = i / (kHP * C8), r = i - piece * (kHP * C8);
        const int p = r / C8, c8 = r - p * C8;                    // consecutive lanes: consecutive 16 bytes of a pixel
        const int ly = p / kHX, lx = p - ly * kHX;
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
          v = *reinterpret_cast<const uint4*>(in_b + piece * plane + (((size_t)gy * a.W + gx) * a.Cp + sl * CS + c8 * 8) * 2);
        *reinterpret_cast<uint4*>(sx + piece * PIECE + p * PITCH + 16 * c8) = v;
      }
    }
    // ---- this slice's weight fragments -> LDS
    {
      const uint4* src = a.wfrag + ((size_t)cb * slices + sl) * WSL;
#pragma unroll 1
      for (int i = tid; i < WSL; i += 256) sw[i] = src[i];
    }
    __syncthreads();
    f32x4v acch[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { acch[mt][0] = (f32x4v)(0.0f); acch[mt][1] = (f32x4v)(0.0f); }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      f16x8 bh[2], bm[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const unsigned char* p = sx + boff[s] + nt * kHX * PITCH;
        bh[nt] = *reinterpret_cast<const f16x8*>(p);
        bm[nt] = *reinterpret_cast<const f16x8*>(p + PIECE);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const f16x8 wh = __builtin_bit_cast(f16x8, sw[((s * 4 + mt) * 2) * 64 + lane]);
        const f16x8 wm = __builtin_bit_cast(f16x8, sw[((s * 4 + mt) * 2 + 1) * 64 + lane]);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          accs[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wm, bh[nt], accs[mt][nt], 0, 0, 0);
          accs[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, bm[nt], accs[mt][nt], 0, 0, 0);
          acch[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, bh[nt], acch[mt][nt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { acc[mt][0] += acch[mt][0]; acc[mt][1] += acch[mt][1]; }
    __syncthreads();                                              // everyone is done reading before the next slice lands
  }

  // ---- epilogue.  accumulator: row = 4 kg + r (output channel of the M tile), column = vox
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) { acc[mt][0] += accs[mt][0]; acc[mt][1] += accs[mt][1]; }
  const int xo = x0 + vox;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int yo = y0 + 2 * wave + nt;
    if (yo >= a.H || xo >= a.W) continue;
    const size_t pix = (size_t)yo * a.W + xo;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int co = kMB * cb + 16 * mt + 4 * kg;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = acc[mt][nt][r] * a.unscale[co + r] + (a.bias ? a.bias[co + r] : 0.0f);
        if (a.relu) v[r] = __builtin_fmaxf(v[r], 0.0f);
      }
      if (OUT_F32) {
        float* o = reinterpret_cast<float*>(out_b);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(size_t)(co + r) * HW + pix] = v[r];
      } else {
        f16x4 h, m;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (!(__builtin_fabsf(v[r]) <= kF16Max)) { bad = true; v[r] = 0.0f; }
          _Float16 hh, mm;
          split(v[r], hh, mm);
          h[r] = hh; m[r] = mm;
        }
        _Float16* o = reinterpret_cast<_Float16*>(out_b);
        *reinterpret_cast<f16x4*>(o + pix * a.Cout + co) = h;
        *reinterpret_cast<f16x4*>(o + HW * a.Cout + pix * a.Cout + co) = m;
      }
    }
  }
  if (bad) *a.status = 1;
}

// ---- pack.  One wave per output channel: the power of two that brings max |w| into [2^13, 2^14), stored as its inverse
__global__ __launch_bounds__(64) void pack_scale_kernel(const float* __restrict__ w, int n_per, float* __restrict__ unscale,
                                                        int* __restrict__ status) {
  const int co = blockIdx.x, lane = threadIdx.x;
  float mx = 0.0f;
  bool bad = false;
  for (int i = lane; i < n_per; i += 64) {
    const float v = __builtin_fabsf(w[(size_t)co * n_per + i]);
    if (!(v <= 3.0e38f)) bad = true; else mx = __builtin_fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = __builtin_fmaxf(mx, __shfl_xor(mx, o, 64));
    bad = bad || __shfl_xor((int)bad, o, 64);
  }
  if (lane == 0) {
    int e = 0;
    if (mx > 0.0f) {
      int ex;
      frexpf(mx, &ex);                                            // mx = f * 2^ex, f in [0.5, 1): floor(log2 mx) = ex - 1
      e = 13 - (ex - 1);
      e = e > 100 ? 100 : (e < -100 ? -100 : e);
    }
    unscale[co] = ldexpf(1.0f, -e);
    if (bad) *status = 1;
  }
}

// (Cout, Cin, 3, 3) float32 -> A fragments: element j of fragment [cb][sl][s][mt][piece][lane] is the hi / mid part of the
// scaled W[64 cb + 16 mt + (lane & 15)][ci][tap] with (CS = 32) tap = s, ci = 32 sl + 8 (lane >> 4) + j or (CS = 8)
// tap = 4 s + (lane >> 4), ci = j; zero beyond the 9 taps and the Cin channels
__global__ void pack_frag_kernel(const float* __restrict__ w, int Cin, int Cout, int cs, int slices, int KS,
                                 const float* __restrict__ unscale, _Float16* __restrict__ frag, int* __restrict__ status) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)(Cout / kMB) * slices * KS * 4 * 64 * 8;
  if (e >= n) return;
  const int j = e & 7, lane = (e >> 3) & 63, mt = (e >> 9) & 3;
  size_t q = e >> 11;
  const int s = q % KS; q /= KS;
  const int sl = q % slices, cb = q / slices;
  const int co = kMB * cb + 16 * mt + (lane & 15);
  const int tap = cs == 32 ? s : 4 * s + (lane >> 4);
  const int ci = cs == 32 ? 32 * sl + 8 * (lane >> 4) + j : j;
  float v = 0.0f;
  if (tap < 9 && ci < Cin) v = w[((size_t)co * Cin + ci) * 9 + tap] / unscale[co];      // a power of two: exact
  if (!(__builtin_fabsf(v) <= kF16Max)) { *status = 1; v = 0.0f; }
  _Float16 h, m;
  split(v, h, m);
  const size_t base = ((((((size_t)cb * slices + sl) * KS + s) * 4 + mt) * 2) * 64 + lane) * 8 + j;
  frag[base] = h;
  frag[base + 64 * 8] = m;
}

// ---- 2x2 max-pool, floor mode
__global__ void maxpool2_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int H, int W) {
  const int Ho = H >> 1, Wo = W >> 1;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)C * Ho * Wo) return;
  const int x = i % Wo, y = (i / Wo) % Ho, c = i / ((size_t)Wo * Ho);
  const float* p = in + ((size_t)c * H + 2 * y) * W + 2 * x;
  out[i] = __builtin_fmaxf(__builtin_fmaxf(p[0], p[1]), __builtin_fmaxf(p[W], p[W + 1]));
}

// packed (C,H,W) -> packed (C,H/2,W/2): the pair of the largest hi + mid (the sum is the float32 value the pair was split from)
__global__ void maxpool2_packed_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out, int C, int H, int W,
                                       size_t in_stride, size_t out_stride) {
  const int Ho = H >> 1, Wo = W >> 1, C8 = C >> 3;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)Ho * Wo * C8) return;
  const int c8 = i % C8;
  const size_t po = i / C8;
  const int x = po % Wo, y = po / Wo;
  const _Float16* ih = in + blockIdx.y * (in_stride / 2);
  _Float16* oh = out + blockIdx.y * (out_stride / 2);
  const size_t plane_i = (size_t)H * W * C, plane_o = (size_t)Ho * Wo * C;
  f16x8 bh, bm;
  float best[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t o = ((size_t)(2 * y + (k >> 1)) * W + 2 * x + (k & 1)) * C + 8 * c8;
    const f16x8 h = *reinterpret_cast<const f16x8*>(ih + o), m = *reinterpret_cast<const f16x8*>(ih + plane_i + o);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = (float)h[j] + (float)m[j];
      if (k == 0 || v > best[j]) { best[j] = v; bh[j] = h[j]; bm[j] = m[j]; }
    }
  }
  *reinterpret_cast<f16x8*>(oh + po * C + 8 * c8) = bh;
  *reinterpret_cast<f16x8*>(oh + plane_o + po * C + 8 * c8) = bm;
}

// ---- prologue: codes -> the scaled network input of the prediction (image 0) and the ground truth (image 1), packed with
// 8 channels (5 of them zero).  The composite is svs_nvs.hip's: the code where the mask is set, 255 elsewhere
// (eval_vsdf.py:199-204 on 0/1 masks), then code / 255 (float32), x * 2 - 1 (lpips_tf.py:55-56), (x - shift) / scale
__global__ void prologue_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, const uint8_t* __restrict__ mask,
                                size_t HW, _Float16* __restrict__ out, size_t out_stride) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= HW) return;
  const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
  const uint8_t* src = blockIdx.y ? gt : pred;
  _Float16* o = out + blockIdx.y * (out_stride / 2);
  f16x8 h = (f16x8)((_Float16)0.0f), m = (f16x8)((_Float16)0.0f);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int code = mask[3 * p + c] ? src[3 * p + c] : 255;
    const float x = (float)code / 255.0f;
    const float v = ((x * 2.0f - 1.0f) - shift[c]) / scale[c];
    _Float16 hh, mm;
    split(v, hh, mm);
    h[c] = hh; m[c] = mm;
  }
  *reinterpret_cast<f16x8*>(o + p * 8) = h;
  *reinterpret_cast<f16x8*>(o + HW * 8 + p * 8) = m;
}

// ---- head.  One wave per pixel, lane l holds the channels l, l + 64, ...; float64 throughout:
//   n(f) = f / (sqrt(sum_c f_c^2) + 1e-10),  d = sum_c w[c] (n(f0)_c - n(f1)_c)^2
// The butterfly leaves the same bits in every lane.  The wave adds its pixels' d in pixel order, the workgroup its four
// waves in order: partial[blockIdx.x], or (mean: a launch of one workgroup) the spatial mean itself.
__device__ __forceinline__ double wave_sum_all(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool PACKED>
__global__ __launch_bounds__(64 * kHeadWaves) void head_kernel(const void* f0, const void* f1, const float* __restrict__ w, int C,
                                                               size_t HW, double* __restrict__ partial, int mean) {
  __shared__ double red[kHeadWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nq = C >> 6;                                          // <= 8
  double wq[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) wq[q] = q < nq ? (double)w[lane + 64 * q] : 0.0;
  double total = 0.0;
  for (size_t p = (size_t)blockIdx.x * kHeadWaves + wave; p < HW; p += (size_t)gridDim.x * kHeadWaves) {
    double a[8], b[8], sa = 0.0, sb = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      a[q] = 0.0; b[q] = 0.0;
      if (q < nq) {
        const int c = lane + 64 * q;
        if (PACKED) {
          const _Float16* h0 = static_cast<const _Float16*>(f0);
          const _Float16* h1 = static_cast<const _Float16*>(f1);
          const size_t o = p * C + c, plane = HW * C;
          a[q] = (double)((float)h0[o] + (float)h0[plane + o]);
          b[q] = (double)((float)h1[o] + (float)h1[plane + o]);
        } else {
          a[q] = (double)static_cast<const float*>(f0)[(size_t)c * HW + p];
          b[q] = (double)static_cast<const float*>(f1)[(size_t)c * HW + p];
        }
        sa += a[q] * a[q]; sb += b[q] * b[q];
      }
    }
    const double na = __builtin_sqrt(wave_sum_all(sa)) + 1e-10, nb = __builtin_sqrt(wave_sum_all(sb)) + 1e-10;
    double d = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double t = a[q] / na - b[q] / nb;
      d += wq[q] * (t * t);
    }
    total += wave_sum_all(d);
  }
  if (lane == 0) red[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
    for (int k = 1; k < kHeadWaves; ++k) s += red[k];
    partial[blockIdx.x] = mean ? s / (double)HW : s;
  }
}

struct FinishArgs {
  int grid[kTaps];
  double hw[kTaps];
};

// out[v] = sum over the taps, in order, of (the tap's partial sums in order) / its pixels
__global__ void finish_kernel(const double* __restrict__ partial, FinishArgs f, int V, double* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  double r = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    const double* p = partial + ((size_t)v * kTaps + k) * kHeadGrid;
    double s = 0.0;
    for (int g = 0; g < f.grid[k]; ++g) s += p[g];
    r += s / f.hw[k];
  }
  out[v] = r;
}

// ---- host side
template <int CS, bool IN_F32, bool OUT_F32>
int launch_conv(const ConvArgs& a, int images, hipStream_t s) {
  constexpr int lds = lds_bytes<CS>();
  if (const int rc = frag::opt_in_lds<conv3x3_kernel<CS, IN_F32, OUT_F32>>(lds, "svs_conv3x3_mfma")) return rc;
  const dim3 grid((unsigned)(a.tiles_x * ((a.H + kTY - 1) / kTY)), (unsigned)(a.Cout / kMB), (unsigned)images);
  conv3x3_kernel<CS, IN_F32, OUT_F32><<<grid, 256, lds, s>>>(a);
  return check_launch("svs_conv3x3_mfma");
}

inline ConvArgs conv_args(const void* in, const void* wfrag, const float* bias, void* out, int Cin, int Cout, int H, int W, int relu,
                          int* status) {
  ConvArgs a;
  a.in = in; a.wfrag = static_cast<const uint4*>(wfrag);
  a.unscale = reinterpret_cast<const float*>(static_cast<const unsigned char*>(wfrag) + frag_bytes(Cin, Cout));
  a.bias = bias; a.out = out; a.Cin = Cin; a.Cp = padded_channels(Cin); a.Cout = Cout; a.H = H; a.W = W; a.relu = relu ? 1 : 0;
  a.tiles_x = (W + kTX - 1) / kTX; a.in_stride = 0; a.out_stride = 0; a.status = status;
  return a;
}

// the flag of the entries that have no workspace: one device word per process, made at the first use
int* process_status() {
  static int* word = nullptr;
  static std::once_flag once;
  std::call_once(once, [] { if (hipMalloc(&word, sizeof(int)) != hipSuccess) word = nullptr; });
  return word;
}

// reads the flag back (synchronises the stream)
int read_status(const char* what, const int* status, hipStream_t s) {
  int h = 0;
  hipError_t e = hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return (int)e; }
  if (h) { set_error("%s: an operand does not fit fp16 (|v| > 65504 or not a number)", what); return SVS_EOVERFLOW; }
  return SVS_OK;
}

inline bool size_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W <= (1LL << 26); }

// VGG-16 features up to relu5_3: (Cin, Cout) per convolution, the group it belongs to, the taps' channels
const int kCin[kLayers] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int kCout[kLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int kGroup[kLayers] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
const int kTapC[kTaps] = {64, 128, 256, 512, 512};

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// packed_net: per convolution its fragments + inverse scales, then its bias; then the lin weights of the five taps
struct NetLayout {
  size_t wfrag[kLayers], bias[kLayers], lin[kTaps], bytes;
  NetLayout() {
    size_t o = 0;
    for (int i = 0; i < kLayers; ++i) {
      wfrag[i] = o; o += align256(frag_bytes(kCin[i], kCout[i]) + (size_t)kCout[i] * 4);
      bias[i] = o; o += align256((size_t)kCout[i] * 4);
    }
    for (int k = 0; k < kTaps; ++k) { lin[k] = o; o += align256((size_t)kTapC[k] * 4); }
    bytes = o;
  }
};

struct Workspace {
  size_t status, partial, buf[2], buf_bytes, bytes;
  Workspace(int V, int H, int W) {
    status = 0;
    partial = 256;
    buf_bytes = align256((size_t)2 * 64 * H * W * 4);            // both images of the widest activation (64, H, W), packed
    buf[0] = align256(partial + (size_t)V * kTaps * kHeadGrid * sizeof(double));
    buf[1] = buf[0] + buf_bytes;
    bytes = buf[1] + buf_bytes;
  }
};

inline int score_sizes(const char* what, int V, int H, int W) {
  if (V < 1) { set_error("%s: V must be >= 1", what); return SVS_EINVAL; }
  if (H < 16 || W < 16 || (long long)H * W > (1LL << 24)) {
    set_error("%s: H and W must be >= 16 (relu5_3 needs one pixel) with H*W <= 2^24", what); return SVS_ESHAPE;
  }
  return SVS_OK;
}

}  // namespace lpips
}  // namespace svs

using namespace svs;
using namespace svs::lpips;

extern "C" {

int svs_conv3x3_mfma_supported(int Cin, int Cout) { return supported(Cin, Cout) ? 1 : 0; }

// bytes of a layer's packed weights: the A fragments and the per-channel inverse scales behind them; 0 when unsupported
size_t svs_conv3x3_mfma_wfrag_bytes(int Cin, int Cout) {
  if (!supported(Cin, Cout)) return 0;
  return frag_bytes(Cin, Cout) + (size_t)Cout * 4;
}

int svs_conv3x3_mfma_pack(const float* weight, int Cin, int Cout, void* wfrag, void* hip_stream) {
  if (!weight || !wfrag) { set_error("svs_conv3x3_mfma_pack: null argument"); return SVS_EINVAL; }
  if (!supported(Cin, Cout)) { set_error("svs_conv3x3_mfma_pack: unsupported (Cin, Cout) = (%d, %d)", Cin, Cout); return SVS_ESHAPE; }
  int* status = process_status();
  if (!status) { set_error("svs_conv3x3_mfma_pack: no device word for the status flag"); return (int)hipErrorOutOfMemory; }
  hipStream_t s = (hipStream_t)hip_stream;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int), s);
  if (e != hipSuccess) { set_error("svs_conv3x3_mfma_pack: %s", hipGetErrorString(e)); return (int)e; }
  float* unscale = reinterpret_cast<float*>(static_cast<unsigned char*>(wfrag) + frag_bytes(Cin, Cout));
  pack_scale_kernel<<<Cout, 64, 0, s>>>(weight, Cin * 9, unscale, status);
  int rc = check_launch("svs_conv3x3_mfma_pack(scale)");
  if (rc) return rc;
  const int cs = slice_channels(Cin), slices = padded_channels(Cin) / cs, KS = cs == 32 ? 9 : 3;
  const size_t n = (size_t)(Cout / kMB) * slices * KS * 4 * 64 * 8;
  pack_frag_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(weight, Cin, Cout, cs, slices, KS, unscale,
                                                               static_cast<_Float16*>(wfrag), status);
  if ((rc = check_launch("svs_conv3x3_mfma_pack(fragments)"))) return rc;
  return read_status("svs_conv3x3_mfma_pack", status, s);
}

int svs_conv3x3_mfma(const float* in, const void* wfrag, const float* bias, float* out, int Cin, int Cout, int H, int W, int relu,
                     void* hip_stream) {
  if (!in || !wfrag || !out) { set_error("svs_conv3x3_mfma: null argument"); return SVS_EINVAL; }
  if (!supported(Cin, Cout)) { set_error("svs_conv3x3_mfma: unsupported (Cin, Cout) = (%d, %d)", Cin, Cout); return SVS_ESHAPE; }
  if (!size_ok(H, W)) { set_error("svs_conv3x3_mfma: H and W must be >= 1 with H*W <= 2^26"); return SVS_ESHAPE; }
  int* status = process_status();
  if (!status) { set_error("svs_conv3x3_mfma: no device word for the status flag"); return (int)hipErrorOutOfMemory; }
  hipStream_t s = (hipStream_t)hip_stream;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int), s);
  if (e != hipSuccess) { set_error("svs_conv3x3_mfma: %s", hipGetErrorString(e)); return (int)e; }
  const ConvArgs a = conv_args(in, wfrag, bias, out, Cin, Cout, H, W, relu, status);
  const int rc = Cin == 3 ? launch_conv<8, true, true>(a, 1, s) : launch_conv<32, true, true>(a, 1, s);
  if (rc) return rc;
  return read_status("svs_conv3x3_mfma", status, s);
}

int svs_maxpool2(const float* in, float* out, int C, int H, int W, void* hip_stream) {
  if (!in || !out) { set_error("svs_maxpool2: null argument"); return SVS_EINVAL; }
  if (C < 1 || C > 65536 || H < 2 || W < 2 || (long long)H * W > (1LL << 26)) {
    set_error("svs_maxpool2: C in 1..65536, H and W >= 2 with H*W <= 2^26"); return SVS_ESHAPE;
  }
  const size_t n = (size_t)C * (H >> 1) * (W >> 1);
  maxpool2_f32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(in, out, C, H, W);
  return check_launch("svs_maxpool2");
}

int svs_lpips_head(const float* f0, const float* f1, const float* w, int C, int H, int W, double* out, void* hip_stream) {
  if (!f0 || !f1 || !w || !out) { set_error("svs_lpips_head: null argument"); return SVS_EINVAL; }
  if (C < 64 || C > 512 || (C & 63) || !size_ok(H, W)) {
    set_error("svs_lpips_head: C a multiple of 64 in 64..512, H and W >= 1 with H*W <= 2^26"); return SVS_ESHAPE;
  }
  head_kernel<false><<<1, 64 * kHeadWaves, 0, (hipStream_t)hip_stream>>>(f0, f1, w, C, (size_t)H * W, out, 1);
  return check_launch("svs_lpips_head");
}

size_t svs_lpips_net_bytes(void) { return NetLayout().bytes; }

// byte offset inside packed_net: what = 0 the packed weights of convolution `index` (0..12), 1 its bias, 2 the lin weights
// of tap `index` (0..4); (size_t)-1 for anything else
size_t svs_lpips_net_offset(int what, int index) {
  const NetLayout n;
  if (what == 0 && index >= 0 && index < kLayers) return n.wfrag[index];
  if (what == 1 && index >= 0 && index < kLayers) return n.bias[index];
  if (what == 2 && index >= 0 && index < kTaps) return n.lin[index];
  return (size_t)-1;
}

size_t svs_lpips_workspace_bytes(int V, int H, int W) {
  if (V < 1 || H < 16 || W < 16 || (long long)H * W > (1LL << 24)) return 0;
  return Workspace(V, H, W).bytes;
}

int svs_lpips_score(const uint8_t* pred, const uint8_t* gt, const uint8_t* mask, int V, int H, int W, const void* packed_net,
                    void* workspace, double* out, void* hip_stream) {
  if (!pred || !gt || !mask || !packed_net || !workspace || !out) { set_error("svs_lpips_score: null argument"); return SVS_EINVAL; }
  if (((uintptr_t)packed_net | (uintptr_t)workspace) & 15) { set_error("svs_lpips_score: packed_net and workspace must be 16-byte aligned"); return SVS_EINVAL; }
  int rc = score_sizes("svs_lpips_score", V, H, W);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const NetLayout net;
  const Workspace ws(V, H, W);
  unsigned char* wsb = static_cast<unsigned char*>(workspace);
  const unsigned char* nb = static_cast<const unsigned char*>(packed_net);
  int* status = reinterpret_cast<int*>(wsb + ws.status);
  double* partial = reinterpret_cast<double*>(wsb + ws.partial);
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int), s);
  if (e != hipSuccess) { set_error("svs_lpips_score: %s", hipGetErrorString(e)); return (int)e; }

  FinishArgs fin;
  {
    int h = H, w = W;
    for (int k = 0; k < kTaps; ++k) {
      const size_t hw = (size_t)h * w;
      const size_t g = (hw + kHeadWaves - 1) / kHeadWaves;
      fin.grid[k] = (int)(g < (size_t)kHeadGrid ? g : (size_t)kHeadGrid);
      fin.hw[k] = (double)hw;
      h >>= 1; w >>= 1;
    }
  }
  const size_t img_in = (size_t)H * W * 3;
  for (int v = 0; v < V; ++v) {
    int h = H, w = W, cur = 0;                                    // the buffer that holds the current activation
    size_t hw = (size_t)h * w;
    size_t stride = hw * 8 * 4;                                   // bytes of one image of the current activation
    prologue_kernel<<<dim3((unsigned)((hw + 255) / 256), 2), 256, 0, s>>>(pred + v * img_in, gt + v * img_in, mask + v * img_in, hw,
                                                                         reinterpret_cast<_Float16*>(wsb + ws.buf[cur]), stride);
    if ((rc = check_launch("svs_lpips_score(prologue)"))) return rc;
    for (int i = 0; i < kLayers; ++i) {
      const int Cin = kCin[i], Cout = kCout[i];
      if (i > 0 && kGroup[i] != kGroup[i - 1]) {                  // a pool precedes each group except the first
        const int C = Cin, ho = h >> 1, wo = w >> 1;
        const size_t n = (size_t)ho * wo * (C >> 3), ostride = (size_t)ho * wo * C * 4;
        maxpool2_packed_kernel<<<dim3((unsigned)((n + 255) / 256), 2), 256, 0, s>>>(
            reinterpret_cast<const _Float16*>(wsb + ws.buf[cur]), reinterpret_cast<_Float16*>(wsb + ws.buf[cur ^ 1]), C, h, w, stride, ostride);
        if ((rc = check_launch("svs_lpips_score(pool)"))) return rc;
        h = ho; w = wo; hw = (size_t)h * w; stride = ostride; cur ^= 1;
      }
      ConvArgs a = conv_args(wsb + ws.buf[cur], nb + net.wfrag[i], reinterpret_cast<const float*>(nb + net.bias[i]),
                             wsb + ws.buf[cur ^ 1], Cin, Cout, h, w, 1, status);
      a.in_stride = stride;
      a.out_stride = hw * Cout * 4;
      rc = Cin == 3 ? launch_conv<8, false, false>(a, 2, s) : launch_conv<32, false, false>(a, 2, s);
      if (rc) return rc;
      stride = a.out_stride; cur ^= 1;
      if (i + 1 == kLayers || kGroup[i + 1] != kGroup[i]) {       // the group's last ReLU is a tap
        const int k = kGroup[i];
        head_kernel<true><<<fin.grid[k], 64 * kHeadWaves, 0, s>>>(wsb + ws.buf[cur], wsb + ws.buf[cur] + stride,
                                                                 reinterpret_cast<const float*>(nb + net.lin[k]), Cout, hw,
                                                                 partial + ((size_t)v * kTaps + k) * kHeadGrid, 0);
        if ((rc = check_launch("svs_lpips_score(head)"))) return rc;
      }
    }
  }
  finish_kernel<<<(V + 63) / 64, 64, 0, s>>>(partial, fin, V, out);
  if ((rc = check_launch("svs_lpips_score(finish)"))) return rc;
  return read_status("svs_lpips_score", status, s);
}

}  // extern "C"
