// UCSNet's parts that CasMVSNet has no counterpart for (models/ucsnet.py): the 2-D transposed convolutions of the "unet"
// feature extractor FeatExtNet (:114-149, 220-235), the whole extractor from one call (:237-302), and the
// uncertainty-aware depth hypotheses of stages 2 and 3 (:44-72, 443-452).  The per-pixel uncertainty itself (:393-394) is a
// second reduction of the cost volume's tail and lives beside it (csrc/svs_costvol.hip: svs_prob_depth_conf_var).
//
// ConvTranspose2d(k3, s2, p1, output_padding 1):  out[co][oy][ox] = sum_ci sum_(ky,kx) in[ci][(oy+1-ky)/2][(ox+1-kx)/2] *
// w[ci][co][ky][kx] over the taps for which oy+1-ky and ox+1-kx are even and the input position is in range.  With
// oy = 2 y + py, ox = 2 x + px that is four stride-1 convolutions, one per output parity class (py, px), over the 2 x 2 input
// neighbourhood in[y + dy][x + dx], dy <= py, dx <= px:   ky = (py ? (dy ? 0 : 2) : 1),  kx likewise:  1, 2, 2 and 4 taps.
//
// svs_deconv2d_mfma runs the four classes as implicit GEMMs on v_mfma_f32_16x16x32_f16 with two-piece fp16 operands (hi + mid:
// hi * hi + hi * mid + mid * hi, float32 accumulation), the scheme of csrc/svs_conv2d_mfma.hip:
//   D[cout][pixel] = sum_k W_class[cout][k] * P[k][pixel],  k = t * Cin + ci  (t = tdy * (1 + px) + tdx),  M = 16 >= Cout,
//   N = 16 consecutive x, K = 32 (the 1-tap class at Cin 16 is zero-padded to one k-step).
// A workgroup (4 waves) owns 8 (y) x 32 (x) input positions = 16 x 64 outputs and walks over its share of the windows with
// the A fragments of all classes in registers; per window it converts the 9 x 33 input halo (float32, channel first) into
// channel-last fp16 hi / mid pieces in LDS (pixel pitch an odd multiple of 16 bytes), then every wave computes two input
// rows: per row and py both px classes, so that a lane holds out[2 x] and out[2 x + 1] and stores them as one 8-byte word.
// OPERAND RANGE (the split is not scaled): |value| < 65504 for activations and folded weights, or the hi piece is inf (and inf
// times the zero weights of the padded k-step is NaN); a mid piece below 2^-14 (|value| < 0.125) is an fp16 subnormal, good to
// 3e-8 absolute: weights of 1e-2 carry 3e-6 relative instead of 2e-7.  Within [0.125, 65504) both operands have 22 bits.
#include "svs_conv_frag.h"
#include "svs_conv2d_api.h"
#include <cstdint>

namespace svs {
namespace ucsnet {

using frag::f16x8;
using frag::f32x4v;
using frag::f32x2v;
using frag::pitch;

constexpr int kWaves = 4, kRW = 2, kTX = 32, kTY = kWaves * kRW;      // a window: 8 x 32 input positions
constexpr int kHY = kTY + 1, kHX = kTX + 1;                           // + the row below and the column to the right

struct DeconvArgs {
  const float* in;      // (Cin, H, W)
  const uint4* wfrag;   // [class][k-step][2 pieces][64 lanes] 16-byte A fragments (svs_deconv2d_mfma_pack)
  const float* w;       // float32 path: (Cin, Cout, 3, 3)
  const float* bias;    // [Cout] or nullptr
  float* out;           // channel c at out + c * cstride: (2H, 2W) contiguous
  long long cstride;
  int Cin, Cout, H, W, relu;
  int tiles_x, tiles;
};

__host__ __device__ constexpr int class_taps(int c) { return (1 + (c >> 1)) * (1 + (c & 1)); }
template <int CIN> constexpr int class_ks(int c) { return (class_taps(c) * CIN + 31) / 32; }
template <int CIN> constexpr int class_s0(int c) { int o = 0; for (int i = 0; i < c; ++i) o += class_ks<CIN>(i); return o; }
template <int CIN> constexpr int total_ks() { return class_s0<CIN>(4); }
template <int CIN> constexpr int lds_bytes() { return 2 * kHY * kHX * pitch<CIN>(); }

// the weight tap (ky or kx) that output parity p takes from the input at offset d (d <= p)
__host__ __device__ constexpr int tap_of(int p, int d) { return p ? (d ? 0 : 2) : 1; }

// The A fragments of deconv2d_mfma_kernel (svs_deconv2d_mfma_pack) from (Cin, Cout, 3, 3) float32: fragment pairs [class c =
// 2 py + px][k-step s of the class]; lane l holds output channel l & 15 and, for j = 0..7, k = 32 s + 8 (l >> 4) + j =
// t * Cin + ci with t = tdy * (1 + px) + tdx the input offset (the kernel's `boff`): W[ci][co][tap_of(py, tdy)][tap_of(px, tdx)].
// Zero beyond the class's taps and beyond Cout.
struct DeconvMap {
  int Cin, Cout;
  __host__ __device__ int class_ks(int c) const { return (class_taps(c) * Cin + 31) / 32; }
  __host__ __device__ int n_fragments() const { return class_ks(0) + class_ks(1) + class_ks(2) + class_ks(3); }
  __device__ float source(const float* w, int si, int lane, int j) const {
    int c = 0, s = si;
    while (s >= class_ks(c)) s -= class_ks(c++);
    const int py = c >> 1, px = c & 1;
    const int co = lane & 15, k = 32 * s + 8 * (lane >> 4) + j;
    const int t = k / Cin, ci = k - t * Cin;
    if (t >= class_taps(c) || co >= Cout) return 0.0f;
    const int tdy = t / (1 + px), tdx = t - tdy * (1 + px);
    return w[(((size_t)ci * Cout + co) * 3 + tap_of(py, tdy)) * 3 + tap_of(px, tdx)];
  }
};

template <int CIN>
__global__ __launch_bounds__(256, 2) void deconv2d_mfma_kernel(DeconvArgs a) {
  constexpr int PITCH = pitch<CIN>(), PIECE = kHY * kHX * PITCH, TKS = total_ks<CIN>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int vox = lane & 15, kg = lane >> 4;
  const size_t HW = (size_t)a.H * a.W;
  const int Wo = 2 * a.W;

  // ---- weights: the A fragments of every class, for the whole kernel
  f16x8 wh[TKS], wm[TKS];
#pragma unroll
  for (int s = 0; s < TKS; ++s) {
    wh[s] = __builtin_bit_cast(f16x8, a.wfrag[(s * 2) * 64 + lane]);
    wm[s] = __builtin_bit_cast(f16x8, a.wfrag[(s * 2 + 1) * 64 + lane]);
  }
  // ---- the B-fragment address of each (class, k-step) inside the halo window, relative to (row of the wave, column vox)
  int boff[TKS];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int s = 0; s < class_ks<CIN>(c); ++s) {
      const int kk = 32 * s + 8 * kg;
      int t = kk / CIN;
      const int ci0 = kk % CIN;
      if (t > class_taps(c) - 1) t = class_taps(c) - 1;      // padded k: the weights are zero there
      const int nx = 1 + (c & 1), tdy = t / nx, tdx = t - tdy * nx;
      boff[class_s0<CIN>(c) + s] = (tdy * kHX + tdx) * PITCH + 2 * ci0;
    }

  for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * kTX, y0 = ty * kTY;
    // ---- the input halo window -> channel-last fp16 hi / mid pieces (zero below and to the right of the image)
#pragma unroll 1
    for (int p = tid; p < kHY * kHX; p += 256) {
      const int ly = p / kHX, lx = p - ly * kHX;
      const int gy = y0 + ly, gx = x0 + lx;
      const bool ok = gy < a.H && gx < a.W;
      const float* g = a.in + (ok ? (size_t)gy * a.W + gx : 0);
      unsigned char* ph = smem + p * PITCH;
      float v[CIN];
#pragma unroll
      for (int c = 0; c < CIN; ++c) v[c] = ok ? g[(size_t)c * HW] : 0.0f;
#pragma unroll
      for (int c8 = 0; c8 < CIN / 8; ++c8) {
        f16x8 h, m;
        frag::split(v + 8 * c8, h, m);
        *reinterpret_cast<f16x8*>(ph + 16 * c8) = h;
        *reinterpret_cast<f16x8*>(ph + PIECE + 16 * c8) = m;
      }
    }
    __syncthreads();
#pragma unroll
    for (int rw = 0; rw < kRW; ++rw) {
      const int ly = wave * kRW + rw;
      const int y = y0 + ly;
      const unsigned char* rowp = smem + (ly * kHX + vox) * PITCH;
#pragma unroll
      for (int py = 0; py < 2; ++py) {
        f32x4v acc[2][2];
#pragma unroll
        for (int px = 0; px < 2; ++px) {
          acc[px][0] = (f32x4v)(0.0f); acc[px][1] = (f32x4v)(0.0f);
          const int c = 2 * py + px;
#pragma unroll
          for (int s = 0; s < class_ks<CIN>(c); ++s) {
            const int si = class_s0<CIN>(c) + s;
#pragma unroll
            for (int xt = 0; xt < 2; ++xt) {
              const unsigned char* p = rowp + boff[si] + xt * 16 * PITCH;
              const f16x8 bh = *reinterpret_cast<const f16x8*>(p);
              const f16x8 bm = *reinterpret_cast<const f16x8*>(p + PIECE);
              acc[px][xt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wm[si], bh, acc[px][xt], 0, 0, 0);
              acc[px][xt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[si], bm, acc[px][xt], 0, 0, 0);
              acc[px][xt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[si], bh, acc[px][xt], 0, 0, 0);
            }
          }
        }
        // accumulator: row = 4 kg + r (output channel), column = vox (input x); out[2 x], out[2 x + 1] as one word
        if (y < a.H) {
          const int oy = 2 * y + py;
#pragma unroll
          for (int xt = 0; xt < 2; ++xt) {
            const int x = x0 + 16 * xt + vox;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int co = 4 * kg + r;
              if (co < a.Cout && x < a.W) {
                const float b = a.bias ? a.bias[co] : 0.0f;
                float v0 = acc[0][xt][r] + b, v1 = acc[1][xt][r] + b;
                if (a.relu) { v0 = __builtin_fmaxf(v0, 0.0f); v1 = __builtin_fmaxf(v1, 0.0f); }
                *reinterpret_cast<f32x2v*>(a.out + (size_t)co * a.cstride + (size_t)oy * Wo + 2 * x) = f32x2v{v0, v1};
              }
            }
          }
        }
      }
    }
    __syncthreads();                  // everyone is done reading the window before the next one is converted
  }
}

// ---- the float32 vector path: one thread = one input position = a 2 x 2 output quad x 8 output channels; the weights of a
// tap are the same for the whole wave (scalar loads)
constexpr int kF32Threads = 128;

__global__ __launch_bounds__(kF32Threads) void deconv2d_f32_kernel(DeconvArgs a) {
  const int co0 = blockIdx.y * 8;
  const int g = blockIdx.x * kF32Threads + threadIdx.x;
  if (g >= a.H * a.W) return;
  const int y = g / a.W, x = g - y * a.W;
  const bool xr = x + 1 < a.W, yb = y + 1 < a.H;
  const size_t HW = (size_t)a.H * a.W;
  float acc[4][8];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[c][k] = 0.0f;
  for (int ci = 0; ci < a.Cin; ++ci) {
    const float* ip = a.in + ci * HW + (size_t)y * a.W + x;
    const float v00 = ip[0], v01 = xr ? ip[1] : 0.0f, v10 = yb ? ip[a.W] : 0.0f, v11 = (xr && yb) ? ip[a.W + 1] : 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int co = co0 + k < a.Cout ? co0 + k : a.Cout - 1;           // (the surplus channels are not stored)
      const float* wp = a.w + ((size_t)ci * a.Cout + co) * 9;             // [ky][kx]
      acc[0][k] = __builtin_fmaf(wp[4], v00, acc[0][k]);
      acc[1][k] = __builtin_fmaf(wp[3], v01, __builtin_fmaf(wp[5], v00, acc[1][k]));
      acc[2][k] = __builtin_fmaf(wp[1], v10, __builtin_fmaf(wp[7], v00, acc[2][k]));
      acc[3][k] = __builtin_fmaf(wp[0], v11, __builtin_fmaf(wp[2], v10, __builtin_fmaf(wp[6], v01, __builtin_fmaf(wp[8], v00, acc[3][k]))));
    }
  }
  const int Wo = 2 * a.W;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int co = co0 + k;
    if (co >= a.Cout) break;
    const float b = a.bias ? a.bias[co] : 0.0f;
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { r[c] = acc[c][k] + b; if (a.relu) r[c] = __builtin_fmaxf(r[c], 0.0f); }
    float* op = a.out + (size_t)co * a.cstride + (size_t)(2 * y) * Wo + 2 * x;
    *reinterpret_cast<f32x2v*>(op) = f32x2v{r[0], r[1]};
    *reinterpret_cast<f32x2v*>(op + Wo) = f32x2v{r[2], r[3]};
  }
}

bool deconv_supported(int Cin, int Cout) { return (Cin == 16 || Cin == 32) && Cout >= 1 && Cout <= 16; }

bool deconv_args(DeconvArgs& a, const char* what, const float* in, const float* bias, float* out, long long cstride, int Cin, int Cout,
                 int H, int W, int relu) {
  if (!in || !out || Cin < 1 || Cout < 1 || H < 1 || W < 1) { set_error("%s: bad argument", what); return false; }
  if (cstride < 4ll * H * W || (cstride & 1) || (reinterpret_cast<uintptr_t>(out) & 7)) {
    set_error("%s: the output's channel stride must be even and >= 4 H W floats, its address 8-byte aligned", what); return false;
  }
  a.in = in; a.wfrag = nullptr; a.w = nullptr; a.bias = bias; a.out = out; a.cstride = cstride; a.Cin = Cin; a.Cout = Cout;
  a.H = H; a.W = W; a.relu = relu; a.tiles_x = (W + kTX - 1) / kTX; a.tiles = a.tiles_x * ((H + kTY - 1) / kTY);
  return true;
}

template <int CIN>
int launch_mfma(const DeconvArgs& a, hipStream_t s) {
  constexpr int lds = lds_bytes<CIN>();
  if (const int rc = frag::opt_in_lds<deconv2d_mfma_kernel<CIN>>(lds, "svs_deconv2d_mfma")) return rc;
  const int grid = a.tiles < 512 ? a.tiles : 512;
  deconv2d_mfma_kernel<CIN><<<grid, 256, lds, s>>>(a);
  return check_launch("svs_deconv2d_mfma");
}

int run_mfma(const float* in, const void* wfrag, const float* bias, float* out, long long cstride, int Cin, int Cout, int H, int W,
             int relu, hipStream_t s) {
  DeconvArgs a;
  if (!wfrag) { set_error("svs_deconv2d_mfma: bad argument"); return SVS_EINVAL; }
  if (!deconv_supported(Cin, Cout)) { set_error("svs_deconv2d_mfma: unsupported shape (Cin in {16,32}, Cout <= 16)"); return SVS_ESHAPE; }
  if (!deconv_args(a, "svs_deconv2d_mfma", in, bias, out, cstride, Cin, Cout, H, W, relu)) return SVS_EINVAL;
  a.wfrag = reinterpret_cast<const uint4*>(wfrag);
  return Cin == 16 ? launch_mfma<16>(a, s) : launch_mfma<32>(a, s);
}

int run_f32(const float* in, const float* weight, const float* bias, float* out, long long cstride, int Cin, int Cout, int H, int W,
            int relu, hipStream_t s) {
  DeconvArgs a;
  if (!weight) { set_error("svs_deconv2d: bad argument"); return SVS_EINVAL; }
  if (!deconv_args(a, "svs_deconv2d", in, bias, out, cstride, Cin, Cout, H, W, relu)) return SVS_EINVAL;
  a.w = weight;
  const long long n = (long long)H * W;
  dim3 grid((unsigned)((n + kF32Threads - 1) / kF32Threads), (Cout + 7) / 8);
  deconv2d_f32_kernel<<<grid, kF32Threads, 0, s>>>(a);
  return check_launch("svs_deconv2d");
}

// workspace layout of svs_featurenet_unet (floats), P = H * W, b = base channels.  cat1 / cat2 are the two concatenations
// (models/ucsnet.py:233, torch.cat((x, x_pre))): the transposed layer writes channels [0, C), the encoder level [C, 2C)
struct UnetBuffers {
  size_t c0a, cat2, c1a, c1b, cat1, c2a, c2b, c2, d1, d2, total;
  UnetBuffers(int b, int H, int W) {
    const size_t P = (size_t)H * W;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += (n + 63) & ~(size_t)63; return at; };
    c0a = take(b * P); cat2 = take(2 * b * P);
    c1a = take(2 * b * P / 4); c1b = take(2 * b * P / 4); cat1 = take(4 * b * P / 4);
    c2a = take(4 * b * P / 16); c2b = take(4 * b * P / 16); c2 = take(4 * b * P / 16);
    d1 = take(2 * b * P / 4); d2 = take(b * P);
    total = o;
  }
};

// ---- uncertainty-aware hypotheses of stages 2 and 3 (models/ucsnet.py:450-452, 59-70) ----------------------------------
struct UHypoArgs {
  const float* depth;   // (Hp, Wp)
  const float* var;     // (Hp, Wp)
  int Hp, Wp, Hs, Ws, D;
  float* out;           // (D, Hs, Ws)
};

// F.interpolate(mode='bilinear', align_corners=False): source index (o + 0.5) * (n_in / n_out) - 0.5, clamped at 0
__device__ __forceinline__ void lin_src(int o, int n_in, int n_out, int& i0, int& i1, float& t) {
  const float scale = (float)n_in / (float)n_out;
  float src = ((float)o + 0.5f) * scale - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src; if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
  t = src - (float)i0;
}

__global__ void uncertainty_hypotheses_kernel(UHypoArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.Hs * a.Ws) return;
  const int x = idx % a.Ws, y = idx / a.Ws;
  int y0, y1, x0, x1; float ty, tx;
  lin_src(y, a.Hp, a.Hs, y0, y1, ty);
  lin_src(x, a.Wp, a.Ws, x0, x1, tx);
  auto resized = [&](const float* p) {
    const float top = (1.0f - tx) * p[y0 * a.Wp + x0] + tx * p[y0 * a.Wp + x1];
    const float bot = (1.0f - tx) * p[y1 * a.Wp + x0] + tx * p[y1 * a.Wp + x1];
    return (1.0f - ty) * top + ty * bot;
  };
  const float cur = resized(a.depth), var = resized(a.var);
  const float low = -__builtin_fminf(cur, var), high = var;
  const float step = (high - low) / ((float)a.D - 1.0f);
  const float base = cur + low;
  const size_t plane = (size_t)a.Hs * a.Ws;
  for (int d = 0; d < a.D; ++d) a.out[d * plane + idx] = (base + step * (float)d) + 1e-12f;
}

}  // namespace ucsnet
}  // namespace svs

using namespace svs;
using namespace svs::ucsnet;

extern "C" {

int svs_deconv2d_mfma_supported(int Cin, int Cout) { return deconv_supported(Cin, Cout) ? 1 : 0; }

// bytes of the packed A fragments: [sum over the four classes of ceil(taps Cin / 32)][2][64][16 B]
size_t svs_deconv2d_mfma_wfrag_bytes(int Cin, int Cout) {
  if (!deconv_supported(Cin, Cout)) return 0;
  return (size_t)DeconvMap{Cin, Cout}.n_fragments() * 2 * 64 * 16;
}

int svs_deconv2d_mfma_pack(const float* weight, int Cin, int Cout, void* wfrag, void* hip_stream) {
  if (!weight || !wfrag || !deconv_supported(Cin, Cout)) { set_error("svs_deconv2d_mfma_pack: bad argument"); return SVS_EINVAL; }
  return frag::pack_fragments(weight, DeconvMap{Cin, Cout}, wfrag, (hipStream_t)hip_stream, "svs_deconv2d_mfma_pack");
}

int svs_deconv2d_mfma(const float* in, const void* wfrag, const float* bias, float* out, long long out_channel_stride, int Cin,
                      int Cout, int H, int W, int relu, void* hip_stream) {
  return run_mfma(in, wfrag, bias, out, out_channel_stride, Cin, Cout, H, W, relu, (hipStream_t)hip_stream);
}

int svs_deconv2d(const float* in, const float* weight, const float* bias, float* out, long long out_channel_stride, int Cin,
                 int Cout, int H, int W, int relu, void* hip_stream) {
  return run_f32(in, weight, bias, out, out_channel_stride, Cin, Cout, H, W, relu, (hipStream_t)hip_stream);
}

size_t svs_featurenet_unet_workspace_bytes(int base_channels, int H, int W) {
  if (base_channels < 1 || H < 4 || W < 4) return 0;
  return UnetBuffers(base_channels, H, W).total * sizeof(float);
}

int svs_featurenet_unet(const float* image, int H, int W, int base_channels, const float* const* weights, const float* const* biases,
                        const void* const* wfrags, float* workspace, float* stage1, float* stage2, float* stage3, void* hip_stream) {
  if (!image || !weights || !biases || !workspace || !stage1 || !stage2 || !stage3 || base_channels < 1) {
    set_error("svs_featurenet_unet: null argument"); return SVS_EINVAL;
  }
  if (H < 4 || W < 4 || (H & 3) || (W & 3)) { set_error("svs_featurenet_unet: image height and width must be multiples of 4"); return SVS_ESHAPE; }
  for (int i = 0; i < 15; ++i) if (!weights[i]) { set_error("svs_featurenet_unet: weights[%d] is null", i); return SVS_EINVAL; }
  const int b = base_channels, H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4;
  const size_t P = (size_t)H * W, P2 = P / 4;
  const UnetBuffers B(b, H, W);
  float* ws = workspace;
  hipStream_t s = (hipStream_t)hip_stream;
  int rc;
  // layer i on the matrix cores where the caller handed in its fragments, else on the float32 kernels
  auto conv = [&](int i, const float* in, float* out, int Cin, int Cout, int h, int w, int k, int stride, int relu) -> int {
    if (wfrags && wfrags[i] && svs::conv2dmfma::supported(Cin, Cout, k, stride))
      return svs::conv2dmfma::run(in, wfrags[i], biases[i], out, Cin, Cout, h, w, k, stride, relu, s);
    return svs::conv2d::run_conv(in, weights[i], biases[i], nullptr, 0, out, Cin, Cout, h, w, k, stride, relu, s);
  };
  auto deconv = [&](int i, const float* in, float* out, int Cin, int Cout, int h, int w) -> int {
    if (wfrags && wfrags[i] && deconv_supported(Cin, Cout))
      return run_mfma(in, wfrags[i], biases[i], out, 4ll * h * w, Cin, Cout, h, w, 1, s);
    return run_f32(in, weights[i], biases[i], out, 4ll * h * w, Cin, Cout, h, w, 1, s);
  };
#define SVS_UNET(call) if ((rc = (call)) != SVS_OK) return rc
  // encoder (models/ucsnet.py:244-259, 280-282): the last layer of levels 0 and 1 lands in the upper half of its concatenation
  SVS_UNET(svs::conv2d::run_encoder(image, H, W, b, weights, biases, wfrags,
                                    {ws + B.c0a, ws + B.cat2 + b * P, ws + B.c1a, ws + B.c1b, ws + B.cat1 + 2 * b * P2,
                                     ws + B.c2a, ws + B.c2b, ws + B.c2}, s));
  SVS_UNET(conv(8, ws + B.c2, stage1, 4 * b, 4 * b, H4, W4, 1, 1, 0));                    // out1
  // decoder (:289-295): transposed layer into channels [0, C), 3x3 over the concatenation, 1x1 head
  SVS_UNET(deconv(9, ws + B.c2, ws + B.cat1, 4 * b, 2 * b, H4, W4));                      // deconv1.deconv
  SVS_UNET(conv(10, ws + B.cat1, ws + B.d1, 4 * b, 2 * b, H2, W2, 3, 1, 1));              // deconv1.conv
  SVS_UNET(conv(11, ws + B.d1, stage2, 2 * b, 2 * b, H2, W2, 1, 1, 0));                   // out2
  SVS_UNET(deconv(12, ws + B.d1, ws + B.cat2, 2 * b, b, H2, W2));                         // deconv2.deconv
  SVS_UNET(conv(13, ws + B.cat2, ws + B.d2, 2 * b, b, H, W, 3, 1, 1));                    // deconv2.conv
  SVS_UNET(conv(14, ws + B.d2, stage3, b, b, H, W, 1, 1, 0));                             // out3
#undef SVS_UNET
  return SVS_OK;
}

int svs_uncertainty_hypotheses(const float* prev_depth, int Hd, int Wd, const float* prev_var, int Hv, int Wv, int Hs, int Ws,
                               int D, float* out, void* hip_stream) {
  if (!prev_depth || !prev_var || !out || D < 2 || Hd < 1 || Wd < 1 || Hs < 1 || Ws < 1) {
    set_error("svs_uncertainty_hypotheses: bad argument (D >= 2)"); return SVS_EINVAL;
  }
  if (Hd != Hv || Wd != Wv) { set_error("svs_uncertainty_hypotheses: the depth and the uncertainty map differ in size"); return SVS_ESHAPE; }
  UHypoArgs a{prev_depth, prev_var, Hd, Wd, Hs, Ws, D, out};
  const int n = Hs * Ws;
  uncertainty_hypotheses_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch("svs_uncertainty_hypotheses");
}

}  // extern "C"
