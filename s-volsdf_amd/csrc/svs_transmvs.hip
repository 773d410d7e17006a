// TransMVSNet, the third MVS backbone, for gfx950: what it does that CasMVSNet and UCSNet have no kernel for.
//
// Reference: models/dcn.py:66-80 (modulated deformable 3x3 convolution, torchvision.ops.deform_conv2d), models/FMT.py:16-111
// (linear attention encoder layer), :196-223 (the pathway's up-sample-and-add), models/position_encoding.py:23-60,
// models/TransMVSNet.py:52-91 (similarity cost volume with per-pixel view weights) and models/module.py:285-324 (its
// homo_warping: align_corners=True, hypotheses behind the source camera sample nothing).
//
// Everything here is float32 on the vector units.  Operands that are the same for a whole wave (convolution, projection and
// MLP weights, the 160 attention sums) are read with wave-uniform addresses, i.e. through the scalar cache into SGPRs, as
// svs_conv2d reads its weights; per-lane data moves with vector loads and stores only.
#include "svs_common.h"
#include <cstdlib>
#include "svs_warp_taps.h"

namespace svs {
namespace transmvs {

// ---- a. DCNv2: out = relu?(scale * (deform_conv2d(in, offset, weight, mask) + bias) + shift) ---------------------------------
// One lane = one output pixel x all output channels.  Per kernel tap the lane forms its sampling point, the four corner
// weights and offsets and the mask ONCE, samples the 32 input channels and feeds each sample to the Cout accumulators of the
// tap (weights: packed [Cout/8][32][3][3][8] as for svs_conv2d, scalar loads); the nine per-tap sums are then added, which
// also keeps the float32 sum of 288 terms two-level.
constexpr int kDcnCin = 32;

struct DcnArgs {
  const float* in;      // (32,H,W)
  const float* om;      // (27,H,W): the raw conv_offset_mask output
  const float* w;       // packed [ceil(Cout/8)][32][3][3][8]
  const float* bias;    // [Cout] or nullptr
  const float* scale;   // [Cout] or nullptr (with shift: the folded BatchNorm behind the layer)
  const float* shift;
  float* out;           // (Cout,H,W)
  int Cout, H, W, relu;
};

template <int NG>
__global__ __launch_bounds__(256) void deform_conv2d_kernel(DcnArgs a) {
  constexpr int CT = NG * 8;
  const int HW = a.H * a.W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool live = p < HW;
  const int pp = live ? p : 0;                       // a lane beyond the image works on pixel 0 and stores nothing
  const int y = pp / a.W, x = pp - y * a.W;
  float acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = 0.0f;
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    const float dy = a.om[(size_t)(2 * k) * HW + pp], dx = a.om[(size_t)(2 * k + 1) * HW + pp];
    const float mask = 1.0f / (1.0f + __expf(-a.om[(size_t)(18 + k) * HW + pp]));
    const float h = (float)(y + k / 3 - 1) + dy, w = (float)(x + k % 3 - 1) + dx;
    float cw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int co[4] = {0, 0, 0, 0};
    // torchvision's bilinear_interpolate: 0 outside (-1, H) x (-1, W), a corner outside the image contributes 0.  Written so
    // that a NaN offset samples nothing (every comparison false): no index is formed from it.
    if (h > -1.0f && h < (float)a.H && w > -1.0f && w < (float)a.W) {
      const float hl = __builtin_floorf(h), wl = __builtin_floorf(w);
      const float lh = h - hl, lw = w - wl, hh = 1.0f - lh, hw = 1.0f - lw;
      const int h0 = (int)hl, w0 = (int)wl, h1 = h0 + 1, w1 = w0 + 1;
      if (h0 >= 0 && w0 >= 0) { cw[0] = hh * hw; co[0] = h0 * a.W + w0; }
      if (h0 >= 0 && w1 <= a.W - 1) { cw[1] = hh * lw; co[1] = h0 * a.W + w1; }
      if (h1 <= a.H - 1 && w0 >= 0) { cw[2] = lh * hw; co[2] = h1 * a.W + w0; }
      if (h1 <= a.H - 1 && w1 <= a.W - 1) { cw[3] = lh * lw; co[3] = h1 * a.W + w1; }
    }
    float tap[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) tap[c] = 0.0f;
#pragma unroll 4
    for (int ci = 0; ci < kDcnCin; ++ci) {
      const float* ip = a.in + (size_t)ci * HW;
      const float v = (((cw[0] * ip[co[0]] + cw[1] * ip[co[1]]) + cw[2] * ip[co[2]]) + cw[3] * ip[co[3]]) * mask;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const float4* wp = reinterpret_cast<const float4*>(a.w + ((size_t)(g * kDcnCin + ci) * 9 + k) * 8);   // wave-uniform
        const float4 w0 = wp[0], w1 = wp[1];
        const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int c = 0; c < 8; ++c) tap[g * 8 + c] = __builtin_fmaf(wv[c], v, tap[g * 8 + c]);
      }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] += tap[c];
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    if (c >= a.Cout) break;
    float r = acc[c];
    if (a.bias) r += a.bias[c];
    if (a.scale) r = r * a.scale[c] + a.shift[c];
    if (a.relu) r = __builtin_fmaxf(r, 0.0f);
    a.out[(size_t)c * HW + p] = r;
  }
}

// ---- b. Feature Matching Transformer ---------------------------------------------------------------------------------------
// Tokens are channel-last (L,32).  d_model 32, 8 heads of 4, feed-forward width 64 (models/FMT.py:78-94).
constexpr int kFmtC = 32, kFmtHeads = 8, kFmtFF = 64;
constexpr int kFmtSums = 160;                 // KV[h][m][d] (128) then Ksum[h][d] (32)
constexpr int kKvTokPerLane = 4;
constexpr int kKvTokPerBlock = 256 * kKvTokPerLane;

__device__ __forceinline__ void load_token(const float* t, float (&x)[kFmtC]) {
  const float4* p = reinterpret_cast<const float4*>(t);
#pragma unroll
  for (int i = 0; i < kFmtC / 4; ++i) {
    const float4 v = p[i];
    x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w;
  }
}

__device__ __forceinline__ void store_token(float* t, const float (&x)[kFmtC]) {
  float4* p = reinterpret_cast<float4*>(t);
#pragma unroll
  for (int i = 0; i < kFmtC / 4; ++i) p[i] = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
}

// row j of an nn.Linear weight (out,in) times x, plus the bias: the row is wave-uniform
template <int N>
__device__ __forceinline__ float linear_row(const float* __restrict__ w, const float* __restrict__ b, int j, const float (&x)[N]) {
  float s = b[j];
#pragma unroll
  for (int i = 0; i < N; ++i) s = __builtin_fmaf(w[j * N + i], x[i], s);
  return s;
}

// elu(x) + 1 (models/FMT.py:19)
__device__ __forceinline__ float elu1(float x) { return x > 0.0f ? x + 1.0f : __expf(x); }

struct PeArgs { float div[kFmtC / 4]; };

// PositionEncodingSine (temp_bug_fix=True; positions count from 1) added to a (32,H,W) map, written as tokens
__global__ __launch_bounds__(256) void fmt_tokens_in_kernel(const float* __restrict__ chw, int H, int W, PeArgs pe, float* __restrict__ tok) {
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const float fx = (float)(x + 1), fy = (float)(y + 1);
  float v[kFmtC];
#pragma unroll
  for (int g = 0; g < kFmtC / 4; ++g) {
    const float ax = fx * pe.div[g], ay = fy * pe.div[g];
    v[4 * g] = chw[(size_t)(4 * g) * HW + p] + sinf(ax);
    v[4 * g + 1] = chw[(size_t)(4 * g + 1) * HW + p] + cosf(ax);
    v[4 * g + 2] = chw[(size_t)(4 * g + 2) * HW + p] + sinf(ay);
    v[4 * g + 3] = chw[(size_t)(4 * g + 3) * HW + p] + cosf(ay);
  }
  store_token(tok + (size_t)p * kFmtC, v);
}

__global__ __launch_bounds__(256) void fmt_tokens_out_kernel(const float* __restrict__ tok, int HW, float* __restrict__ chw) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  float v[kFmtC];
  load_token(tok + (size_t)p * kFmtC, v);
#pragma unroll
  for (int c = 0; c < kFmtC; ++c) chw[(size_t)c * HW + p] = v[c];
}

struct KvArgs {
  const float* src;     // (S,32)
  const float *k_w, *k_b, *v_w, *v_b;
  float* partial;       // [blocks][160]
  int S;
};

// K = elu(W_k s + b_k) + 1, V = W_v s + b_v, and this block's share of sum_s K[s,h,d] V[s,h,m] and sum_s K[s,h,d].  A lane
// takes kKvTokPerLane tokens (a fixed assignment), the wave adds its lanes with a butterfly, the block adds its four waves
// in order: the same bits on every launch.
__global__ __launch_bounds__(256) void fmt_kv_kernel(KvArgs a) {
  __shared__ float red[4][kFmtSums];
  float sums[kFmtSums];
#pragma unroll
  for (int i = 0; i < kFmtSums; ++i) sums[i] = 0.0f;
#pragma unroll 1
  for (int t = 0; t < kKvTokPerLane; ++t) {
    const int s = blockIdx.x * kKvTokPerBlock + t * 256 + threadIdx.x;
    if (s < a.S) {
      float x[kFmtC];
      load_token(a.src + (size_t)s * kFmtC, x);
#pragma unroll
      for (int h = 0; h < kFmtHeads; ++h) {
        float K[4], V[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          K[d] = elu1(linear_row<kFmtC>(a.k_w, a.k_b, 4 * h + d, x));
          V[d] = linear_row<kFmtC>(a.v_w, a.v_b, 4 * h + d, x);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int d = 0; d < 4; ++d) sums[h * 16 + m * 4 + d] = __builtin_fmaf(K[d], V[m], sums[h * 16 + m * 4 + d]);
#pragma unroll
        for (int d = 0; d < 4; ++d) sums[128 + 4 * h + d] += K[d];
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kFmtSums; ++i) {
    float v = sums[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kFmtSums)
    a.partial[(size_t)blockIdx.x * kFmtSums + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// the last block: the per-block partials added in index order
__global__ __launch_bounds__(256) void fmt_kv_finish_kernel(const float* __restrict__ partial, int blocks, float* __restrict__ kvsum) {
  if (threadIdx.x >= kFmtSums) return;
  float s = 0.0f;
  for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * kFmtSums + threadIdx.x];
  kvsum[threadIdx.x] = s;
}

struct LayerArgs {
  const float* x;       // (L,32)
  const float* kvsum;   // 160
  const float *q_w, *q_b, *o_w, *o_b, *l1_w, *l1_b, *l2_w, *l2_b, *n1_w, *n1_b, *n2_w, *n2_b;
  float* out;           // (L,32)
  int L;
};

__device__ __forceinline__ void layer_norm(float (&x)[kFmtC], const float* __restrict__ g, const float* __restrict__ b) {
  float mean = 0.0f;
#pragma unroll
  for (int i = 0; i < kFmtC; ++i) mean += x[i];
  mean *= 1.0f / kFmtC;
  float var = 0.0f;
#pragma unroll
  for (int i = 0; i < kFmtC; ++i) { const float d = x[i] - mean; var = __builtin_fmaf(d, d, var); }
  const float r = 1.0f / __builtin_sqrtf(var * (1.0f / kFmtC) + 1e-5f);
#pragma unroll
  for (int i = 0; i < kFmtC; ++i) x[i] = (x[i] - mean) * r * g[i] + b[i];
}

// EncoderLayer.forward (models/FMT.py:96-111) for one query token per lane, given the source's 160 sums
__global__ __launch_bounds__(256) void fmt_layer_kernel(LayerArgs a) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= a.L) return;
  float x[kFmtC], att[kFmtC];
  load_token(a.x + (size_t)l * kFmtC, x);
  const float* __restrict__ kv = a.kvsum;
#pragma unroll
  for (int h = 0; h < kFmtHeads; ++h) {
    float Q[4], z = 1e-6f;
#pragma unroll
    for (int d = 0; d < 4; ++d) Q[d] = elu1(linear_row<kFmtC>(a.q_w, a.q_b, 4 * h + d, x));
    float qk = 0.0f;
#pragma unroll
    for (int d = 0; d < 4; ++d) qk = __builtin_fmaf(Q[d], kv[128 + 4 * h + d], qk);
    z = 1.0f / (qk + z);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      float s = 0.0f;
#pragma unroll
      for (int d = 0; d < 4; ++d) s = __builtin_fmaf(Q[d], kv[h * 16 + m * 4 + d], s);
      att[4 * h + m] = s * z;
    }
  }
  float x1[kFmtC];
#pragma unroll
  for (int j = 0; j < kFmtC; ++j) x1[j] = x[j] + linear_row<kFmtC>(a.o_w, a.o_b, j, att);
  layer_norm(x1, a.n1_w, a.n1_b);
  float hid[kFmtFF];
#pragma unroll
  for (int j = 0; j < kFmtFF; ++j) hid[j] = __builtin_fmaxf(linear_row<kFmtC>(a.l1_w, a.l1_b, j, x1), 0.0f);
#pragma unroll
  for (int j = 0; j < kFmtC; ++j) x[j] = x1[j] + linear_row<kFmtFF>(a.l2_w, a.l2_b, j, hid);
  layer_norm(x, a.n2_w, a.n2_b);
  store_token(a.out + (size_t)l * kFmtC, x);
}

// ---- c. the pathway step: out = bilinear_x2(conv1x1(x)) + y (align_corners=False, sizes exactly doubled) -------------------
// Output rows 2i+1 and 2i+2 both interpolate input rows i and i+1 (weights 3/4, 1/4 and 1/4, 3/4; the image's first and last
// row copy their input row), the same along x: a lane owns the 2x2 outputs between four input pixels, reduces those four
// pixels' channels once (the reduction comes first, as in the reference) and blends.
template <int CIN>
__global__ __launch_bounds__(256) void pathway_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                      const float* __restrict__ y, float* __restrict__ out, int h, int w) {
  constexpr int COUT = CIN / 2;
  const int nJ = w + 1;
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= (h + 1) * nJ) return;
  const int i = id / nJ - 1, j = id - (id / nJ) * nJ - 1;
  const int r0 = i < 0 ? 0 : i, r1 = i + 1 > h - 1 ? h - 1 : i + 1;
  const int c0 = j < 0 ? 0 : j, c1 = j + 1 > w - 1 ? w - 1 : j + 1;
  const int hw = h * w;
  float cv[4][COUT];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int c = 0; c < COUT; ++c) cv[q][c] = 0.0f;
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci) {
    const float* ip = x + (size_t)ci * hw;
    const float v[4] = {ip[r0 * w + c0], ip[r0 * w + c1], ip[r1 * w + c0], ip[r1 * w + c1]};
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
      const float wv = wgt[c * CIN + ci];              // wave-uniform
#pragma unroll
      for (int q = 0; q < 4; ++q) cv[q][c] = __builtin_fmaf(wv, v[q], cv[q][c]);
    }
  }
  const int H2 = 2 * h, W2 = 2 * w;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int oy = 2 * i + 1 + a;
    if (oy < 0 || oy >= H2) continue;
    const float ty = r0 == r1 ? 0.0f : (a ? 0.75f : 0.25f);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ox = 2 * j + 1 + b;
      if (ox < 0 || ox >= W2) continue;
      const float tx = c0 == c1 ? 0.0f : (b ? 0.75f : 0.25f);
#pragma unroll
      for (int c = 0; c < COUT; ++c) {
        const float top = (1.0f - tx) * cv[0][c] + tx * cv[1][c], bot = (1.0f - tx) * cv[2][c] + tx * cv[3][c];
        const size_t o = ((size_t)c * H2 + oy) * W2 + ox;
        out[o] = ((1.0f - ty) * top + ty * bot) + y[o];
      }
    }
  }
}

// ---- d. similarity cost volume with per-pixel view weights ----------------------------------------------------------------
using warp::kMaxSrc;
constexpr int kSimDz = 8;                       // depth planes per workgroup (a multiple of every C / 4)

struct SimArgs {
  const float* ref;               // (C,H,W)
  warp::SourceViews src;          // per source view: (H,W,C) features, rotation, translation (svs_warp_taps.h)
  const float* depth_values;      // (D,H,W)
  float* sims;                    // (n_src,D,H,W): per-view similarities
  int D, H, W;
};

// C/4 adjacent lanes own one pixel, 4 channels each, as in svs_warp_variance: a bilinear corner of the (H,W,C) source is one
// contiguous C-vector.  The group walks C/4 depth planes at a time: lane cg projects plane d0 + cg, the corners of each plane
// are then handed round the group with shuffles, so no lane repeats a projection.  The dot product with the reference
// feature is completed with a butterfly over the group.
template <int C, int NS>
__global__ __launch_bounds__(256) void warp_similarity_kernel(SimArgs a) {
  constexpr int LPV = C / 4, VPP = 256 / LPV;
  const int tid = threadIdx.x;
  const int cg = tid % LPV, vl = tid / LPV;
  const int lane = tid & 63, base = lane - cg;
  const int H = a.H, W = a.W, y = blockIdx.y;
  const int xr = blockIdx.x * VPP + vl;
  const bool live = xr < W;
  const int x = live ? xr : W - 1;                 // a group beyond the row repeats its last pixel and stores nothing
  const size_t HW = (size_t)H * W;
  f32x4 ref;
#pragma unroll
  for (int j = 0; j < 4; ++j) ref[j] = a.ref[(size_t)(4 * cg + j) * HW + (size_t)y * W + x];
  const int d_begin = blockIdx.z * kSimDz;
  const int d_end = d_begin + kSimDz < a.D ? d_begin + kSimDz : a.D;
  for (int d0 = d_begin; d0 < d_end; d0 += LPV) {
    f32x4 w4[NS];
    i32x4 o4[NS];
    const int dm = d0 + cg;
    const float depth = a.depth_values[((size_t)(dm < d_end ? dm : d_end - 1) * H + y) * W + x];
#pragma unroll
    // (models/module.py:296-321: align_corners=True, nothing sampled where the projected z is below 1e-6)
    for (int v = 0; v < NS; ++v) warp::bilinear_taps<C, warp::kAlignCorners, true>(a.src, v, x, y, H, W, depth, w4[v], o4[v]);
#pragma unroll
    for (int j = 0; j < LPV; ++j) {
      const int d = d0 + j;
      if (d >= d_end) break;                       // wave-uniform
#pragma unroll
      for (int v = 0; v < NS; ++v) {
        const char* __restrict__ src = reinterpret_cast<const char*>(a.src.src_hwc[v]);
        f32x4 warped = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float wk = __shfl(w4[v][k], base + j);
          const int ok = __shfl(o4[v][k], base + j);
          const f32x4 f = *reinterpret_cast<const f32x4*>(src + ((unsigned)ok + 16u * cg));
          warped = __builtin_elementwise_fma(f32x4{wk, wk, wk, wk}, f, warped);
        }
        float part = ((warped[0] * ref[0] + warped[1] * ref[1]) + warped[2] * ref[2]) + warped[3] * ref[3];
#pragma unroll
        for (int off = 1; off < LPV; off <<= 1) part += __shfl_xor(part, off);
        if (cg == 0 && live) a.sims[(((size_t)v * a.D + d) * H + y) * W + x] = part * (1.0f / C);
      }
    }
  }
}

// the net: 177 floats -- scale0[16] shift0[16] W1[8][16] shift1[8] w2[8] b2

// PixelwiseNet before its sigmoid: 1 -> 16 -> 8 -> 1 with BatchNorm folded by the caller (models/TransMVSNet.py:17-28)
__device__ __forceinline__ float pixel_wise_logit(const float* __restrict__ net, float s) {
  float a0[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) a0[j] = __builtin_fmaxf(__builtin_fmaf(net[j], s, net[16 + j]), 0.0f);
  float o = net[176];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float t = net[160 + i];
#pragma unroll
    for (int j = 0; j < 16; ++j) t = __builtin_fmaf(net[32 + 16 * i + j], a0[j], t);
    o = __builtin_fmaf(net[168 + i], __builtin_fmaxf(t, 0.0f), o);
  }
  return o;
}

struct SimFinishArgs {
  const float* sims;       // (n_src,D,H,W)
  const float* prev_w;     // (n_src,H/2,W/2) or nullptr
  const float* net;        // kNetFloats, used when prev_w is null
  float* out;              // (D,H,W)
  float* w_out;            // (n_src,H,W)
  int n_src, D, H, W;
};

// Stage 1: one lane per (view, pixel), w = max_d sigmoid(net(sim_v[d])).  The sigmoid is monotone, so the maximum is taken
// over the logits.
__global__ __launch_bounds__(256) void view_weights_kernel(SimFinishArgs a) {
  const int HW = a.H * a.W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const float* __restrict__ sim = a.sims + (size_t)blockIdx.y * a.D * HW + p;
  float mx = -__builtin_inff();
#pragma unroll 1
  for (int d = 0; d < a.D; ++d) mx = __builtin_fmaxf(mx, pixel_wise_logit(a.net, sim[(size_t)d * HW]));
  a.w_out[(size_t)blockIdx.y * HW + p] = 1.0f / (1.0f + __expf(-mx));
}

// One lane per pixel: similarity = sum_v sim_v w_v / (1e-5 + sum_v w_v), with the weights view_weights_kernel left in w_out
// or, at stages 2 and 3, the previous stage's at (y/2, x/2) (which are written to w_out at this stage's size).
__global__ __launch_bounds__(256) void sim_finish_kernel(SimFinishArgs a) {
  const int HW = a.H * a.W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / a.W, x = p - y * a.W;
  float wv[kMaxSrc], wsum = 1e-5f;
#pragma unroll
  for (int v = 0; v < kMaxSrc; ++v) {
    wv[v] = 0.0f;
    if (v < a.n_src) {
      if (a.prev_w) {
        wv[v] = a.prev_w[((size_t)v * (a.H / 2) + (y >> 1)) * (a.W / 2) + (x >> 1)];
        a.w_out[(size_t)v * HW + p] = wv[v];
      } else {
        wv[v] = a.w_out[(size_t)v * HW + p];
      }
      wsum += wv[v];
    }
  }
  for (int d = 0; d < a.D; ++d) {
    float s = 0.0f;
#pragma unroll
    for (int v = 0; v < kMaxSrc; ++v)
      if (v < a.n_src) s += a.sims[((size_t)v * a.D + d) * HW + p] * wv[v];
    a.out[(size_t)d * HW + p] = s / wsum;
  }
}

template <int C>
static void launch_sim(const SimArgs& a, int n_src, hipStream_t s) {
  constexpr int VPP = 256 / (C / 4);
  dim3 grid((a.W + VPP - 1) / VPP, a.H, (a.D + kSimDz - 1) / kSimDz);
  warp::dispatch_n_src(n_src, [&](auto ns) { warp_similarity_kernel<C, decltype(ns)::value><<<grid, 256, 0, s>>>(a); });
}

}  // namespace transmvs
}  // namespace svs

using namespace svs;
using namespace svs::transmvs;

extern "C" {

int svs_deform_conv2d(const float* in, const float* offset_mask, const float* weight_packed, const float* bias, const float* scale,
                      const float* shift, float* out, int Cout, int H, int W, int relu, void* hip_stream) {
  if (!in || !offset_mask || !weight_packed || !out || (scale == nullptr) != (shift == nullptr)) {
    set_error("svs_deform_conv2d: bad argument"); return SVS_EINVAL;
  }
  if (Cout < 1 || Cout > 32 || H < 1 || W < 1 || (long long)H * W * kDcnCin >= (1ll << 31) / 4) {
    set_error("svs_deform_conv2d: Cout must be 1..32 and 32 H W floats must stay below 2 GiB"); return SVS_ESHAPE;
  }
  DcnArgs a{in, offset_mask, weight_packed, bias, scale, shift, out, Cout, H, W, relu};
  hipStream_t s = (hipStream_t)hip_stream;
  const unsigned grid = (unsigned)((H * W + 255) / 256);
  switch ((Cout + 7) / 8) {
    case 1: deform_conv2d_kernel<1><<<grid, 256, 0, s>>>(a); break;
    case 2: deform_conv2d_kernel<2><<<grid, 256, 0, s>>>(a); break;
    case 3: deform_conv2d_kernel<3><<<grid, 256, 0, s>>>(a); break;
    default: deform_conv2d_kernel<4><<<grid, 256, 0, s>>>(a); break;
  }
  return check_launch("svs_deform_conv2d");
}

int svs_fmt_tokens_in(const float* chw, int H, int W, const float* div_term, float* tokens, void* hip_stream) {
  if (!chw || !div_term || !tokens || H < 1 || W < 1 || (long long)H * W * kFmtC >= (1ll << 31)) {
    set_error("svs_fmt_tokens_in: bad argument"); return SVS_EINVAL;
  }
  PeArgs pe;
  for (int i = 0; i < kFmtC / 4; ++i) pe.div[i] = div_term[i];          // HOST array
  fmt_tokens_in_kernel<<<(H * W + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(chw, H, W, pe, tokens);
  return check_launch("svs_fmt_tokens_in");
}

int svs_fmt_tokens_out(const float* tokens, int H, int W, float* chw, void* hip_stream) {
  if (!chw || !tokens || H < 1 || W < 1 || (long long)H * W * kFmtC >= (1ll << 31)) {
    set_error("svs_fmt_tokens_out: bad argument"); return SVS_EINVAL;
  }
  fmt_tokens_out_kernel<<<(H * W + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(tokens, H * W, chw);
  return check_launch("svs_fmt_tokens_out");
}

size_t svs_fmt_kv_workspace_bytes(int S) {
  return S < 1 ? 0 : (size_t)((S + kKvTokPerBlock - 1) / kKvTokPerBlock) * kFmtSums * sizeof(float);
}

int svs_fmt_kv(const float* source, int S, const float* k_w, const float* k_b, const float* v_w, const float* v_b, float* workspace,
               float* kvsum, void* hip_stream) {
  if (!source || !k_w || !k_b || !v_w || !v_b || !workspace || !kvsum || S < 1 || (long long)S * kFmtC >= (1ll << 31)) {
    set_error("svs_fmt_kv: bad argument"); return SVS_EINVAL;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  const int blocks = (S + kKvTokPerBlock - 1) / kKvTokPerBlock;
  KvArgs a{source, k_w, k_b, v_w, v_b, workspace, S};
  fmt_kv_kernel<<<blocks, 256, 0, s>>>(a);
  fmt_kv_finish_kernel<<<1, 256, 0, s>>>(workspace, blocks, kvsum);
  return check_launch("svs_fmt_kv");
}

int svs_fmt_layer(const float* x, int L, const float* kvsum, const float* const* weights, float* out, void* hip_stream) {
  if (!x || !kvsum || !weights || !out || L < 1 || (long long)L * kFmtC >= (1ll << 31)) {
    set_error("svs_fmt_layer: bad argument"); return SVS_EINVAL;
  }
  for (int i = 0; i < 12; ++i)
    if (!weights[i]) { set_error("svs_fmt_layer: null weight %d", i); return SVS_EINVAL; }
  LayerArgs a{x, kvsum, weights[0], weights[1], weights[2], weights[3], weights[4], weights[5], weights[6], weights[7],
              weights[8], weights[9], weights[10], weights[11], out, L};
  fmt_layer_kernel<<<(L + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch("svs_fmt_layer");
}

int svs_pathway_step(const float* x, const float* weight, const float* y, float* out, int Cin, int h, int w, void* hip_stream) {
  if (!x || !weight || !y || !out || h < 1 || w < 1) { set_error("svs_pathway_step: bad argument"); return SVS_EINVAL; }
  if ((Cin != 32 && Cin != 16) || (long long)h * w * 4 * Cin >= (1ll << 31)) {
    set_error("svs_pathway_step: Cin must be 32 or 16 (dim_reduction_1 / 2)"); return SVS_ESHAPE;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  const unsigned grid = (unsigned)(((h + 1) * (w + 1) + 255) / 256);
  if (Cin == 32) pathway_kernel<32><<<grid, 256, 0, s>>>(x, weight, y, out, h, w);
  else pathway_kernel<16><<<grid, 256, 0, s>>>(x, weight, y, out, h, w);
  return check_launch("svs_pathway_step");
}

size_t svs_warp_similarity_workspace_bytes(int n_src, int D, int H, int W) {
  return (n_src < 1 || D < 1 || H < 1 || W < 1) ? 0 : (size_t)n_src * D * H * W * sizeof(float);
}

int svs_warp_similarity(const float* ref_feature, const float* const* src_features_hwc, const float* rot_trans, int n_src, int C,
                        int D, int H, int W, const float* depth_values, const float* prev_weights, const float* net,
                        float* workspace, float* similarity, float* weights_out, void* hip_stream) {
  if (!ref_feature || !src_features_hwc || !rot_trans || !depth_values || !workspace || !similarity || !weights_out ||
      (!prev_weights && !net)) {
    set_error("svs_warp_similarity: null argument"); return SVS_EINVAL;
  }
  if (n_src < 1 || n_src > kMaxSrc || D < 1 || H < 2 || W < 2 || (prev_weights && ((H | W) & 1)) ||
      (long long)H * W * C * 4 >= (1ll << 31) || (long long)D * H * W >= (1ll << 31)) {
    set_error("svs_warp_similarity: bad sizes"); return SVS_ESHAPE;
  }
  if (C != 8 && C != 16 && C != 32) { set_error("svs_warp_similarity: C must be 8, 16 or 32"); return SVS_ESHAPE; }
  SimArgs a;
  a.ref = ref_feature; a.depth_values = depth_values; a.sims = workspace; a.D = D; a.H = H; a.W = W;
  if (const int rc = warp::fill_sources("svs_warp_similarity", a.src, src_features_hwc, rot_trans, n_src)) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  if (C == 8) launch_sim<8>(a, n_src, s);
  else if (C == 16) launch_sim<16>(a, n_src, s);
  else launch_sim<32>(a, n_src, s);
  SimFinishArgs f{workspace, prev_weights, net, similarity, weights_out, n_src, D, H, W};
  if (!prev_weights) view_weights_kernel<<<dim3((H * W + 255) / 256, n_src), 256, 0, s>>>(f);
  sim_finish_kernel<<<(H * W + 255) / 256, 256, 0, s>>>(f);
  return check_launch("svs_warp_similarity");
}

}  // extern "C"
