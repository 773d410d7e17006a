// Novel-view scores for gfx950 (eval_vsdf.py:186-212): the masked PSNR and the SSIM of V evaluation views of one size in
// two launches.
//
// Reference: for each view, rgb_pred = PNG codes / 255 and gt = the 8-bit ground truth / 255 (float32), mask 0/1 per
// channel.  PSNR: torch.mean((rgb_pred - gt)[mask == 1] ** 2) over the whole image, -10 log10 of it (finished on the host
// from the sum and count made here).  SSIM: skimage.metrics.structural_similarity(pred_fg, gt_fg, multichannel=True) in
// scikit-image 0.17.2 on the white-composited images x m + (1 - m): per channel uniform_filter(7) of x, y, x^2, y^2, xy,
// cov_norm = 49/48, data_range = 2 (dtype_range of float32 is (-1, 1), data_range is not passed), C1 = (0.01 * 2)^2,
// C2 = (0.03 * 2)^2, the S map cropped by 3 pixels on every side and averaged, then the three channel means averaged
// (restated in tests/nvs_oracle.py).
//
// Arithmetic: on the composited codes a = m ? p : 255, b = m ? g : 255 the 7x7 window sums of a, b, a^2, b^2, ab are
// exact int32 (at most 49 * 255^2), and 49 sum(a^2) - sum(a)^2 = 49 * 48 * 255^2 * vx exactly, so with every term scaled
// by 49^2 255^2 (means) or 49 * 48 * 255^2 (variances)
//   S = (2 A B + c1) (2 (49 Sab - A B) + c2) / ((A^2 + B^2 + c1) ((49 Saa - A^2) + (49 Sbb - B^2) + c2))
// with A = sum(a), B = sum(b), c1 = C1 49^2 255^2, c2 = C2 49 48 255^2: only S is floating point (float64).  The oracle
// runs skimage's float64 formula on the float32 values k / 255; the two agree to about 1e-9.
//
// Launch 1: one 256-thread workgroup per 64x16 output tile of one view.  The 70x22 halo tile of composited codes (all
// three channels) goes to LDS once, then per channel a horizontal pass writes the five 7-sums of 22 rows and a vertical
// pass forms S at the tile's pixels whose window lies wholly inside the image.  The masked squared code differences and
// the masked element count cover every pixel of the tile.  Each workgroup writes one partial record (int64 SSE and
// count, float64 S sum per channel) to the workspace.  Launch 2: one workgroup per view sums its tiles' records in a
// fixed order.  No atomics: the result is bit-identical run to run.
#include "svs_common.h"

namespace svs {
namespace nvs {

constexpr int kR = 3;                                   // window radius: win_size = 7
constexpr int kTileW = 64, kTileH = 16;
constexpr int kHaloW = kTileW + 2 * kR, kHaloH = kTileH + 2 * kR;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr double kC1s = (0.01 * 2) * (0.01 * 2) * (49.0 * 49.0) * (255.0 * 255.0);
constexpr double kC2s = (0.03 * 2) * (0.03 * 2) * (49.0 * 48.0) * (255.0 * 255.0);

struct Partial {
  long long sse, cnt;                                   // masked sum of squared code differences, masked elements
  double s[3];                                          // sum of S over the tile's cropped pixels, per channel
};

struct Grid {
  int tiles_x, tiles_y;
  long long tiles;                                      // per view
  Grid(int H, int W) : tiles_x((W + kTileW - 1) / kTileW), tiles_y((H + kTileH - 1) / kTileH) {
    tiles = (long long)tiles_x * tiles_y;
  }
};

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

struct TileArgs {
  const uint8_t* pred;                                  // (V,H,W,3) codes
  const uint8_t* gt;
  const uint8_t* mask;                                  // (V,H,W,3) nonzero: in the mask
  int H, W, tiles_x, tiles;
  Partial* part;                                        // (V, tiles)
};

__global__ __launch_bounds__(kThreads) void nvs_tile_kernel(TileArgs a) {
  __shared__ uint8_t ca[3][kHaloH][kHaloW];             // composited prediction codes
  __shared__ uint8_t cb[3][kHaloH][kHaloW];             // composited ground-truth codes
  __shared__ int hs[5][kHaloH][kTileW];                 // horizontal 7-sums of a, b, a^2, b^2, ab
  __shared__ long long red_i[2][kWaves];
  __shared__ double red_d[3][kWaves];
  const int tid = threadIdx.x;
  const int v = blockIdx.x / a.tiles, t = blockIdx.x - v * a.tiles;
  const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
  const int y0 = ty * kTileH, x0 = tx * kTileW;
  const size_t img = (size_t)v * a.H * a.W * 3;

  // halo tile, all channels: consecutive threads read consecutive bytes of a row
  int sse = 0, cnt = 0;
  for (int i = tid; i < kHaloH * kHaloW * 3; i += kThreads) {
    const int r = i / (kHaloW * 3), q = i - r * (kHaloW * 3);
    const int c = q / 3, ch = q - c * 3;
    const int y = y0 - kR + r, x = x0 - kR + c;
    uint8_t va = 255, vb = 255;                         // outside the image: read only by windows the crop drops
    if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
      const size_t o = img + ((size_t)y * a.W + x) * 3 + ch;
      const int p = a.pred[o], g = a.gt[o];
      if (a.mask[o]) {
        va = (uint8_t)p; vb = (uint8_t)g;
        if (r >= kR && r < kR + kTileH && c >= kR && c < kR + kTileW) {   // the tile itself: every pixel once
          sse += (p - g) * (p - g);
          cnt += 1;
        }
      }
    }
    ca[ch][r][c] = va;
    cb[ch][r][c] = vb;
  }
  __syncthreads();

  double ssum[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int ch = 0; ch < 3; ++ch) {
    for (int i = tid; i < kHaloH * kTileW; i += kThreads) {
      const int r = i / kTileW, c = i - r * kTileW;
      int sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
#pragma unroll
      for (int k = 0; k < 2 * kR + 1; ++k) {
        const int pa = ca[ch][r][c + k], pb = cb[ch][r][c + k];
        sa += pa; sb += pb; saa += pa * pa; sbb += pb * pb; sab += pa * pb;
      }
      hs[0][r][c] = sa; hs[1][r][c] = sb; hs[2][r][c] = saa; hs[3][r][c] = sbb; hs[4][r][c] = sab;
    }
    __syncthreads();
    for (int i = tid; i < kTileH * kTileW; i += kThreads) {
      const int r = i / kTileW, c = i - r * kTileW;
      const int y = y0 + r, x = x0 + c;
      if (y < kR || y >= a.H - kR || x < kR || x >= a.W - kR) continue;   // crop(S, 3)
      int s[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 2 * kR + 1; ++k)
#pragma unroll
        for (int m = 0; m < 5; ++m) s[m] += hs[m][r + k][c];
      const double A = s[0], B = s[1];
      const double vxx = (double)(49 * s[2] - s[0] * s[0]);          // exact in int32: |.| <= 49^2 255^2
      const double vyy = (double)(49 * s[3] - s[1] * s[1]);
      const double vxy = (double)(49 * s[4] - s[0] * s[1]);
      const double num = (2.0 * A * B + kC1s) * (2.0 * vxy + kC2s);
      const double den = (A * A + B * B + kC1s) * (vxx + vyy + kC2s);
      ssum[ch] += num / den;
    }
    __syncthreads();                                    // hs is rewritten by the next channel
  }

  // workgroup sums in a fixed order: waves by shuffles, then the four waves in order
  const long long wsse = wave_sum((long long)sse), wcnt = wave_sum((long long)cnt);
  double ws[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) ws[ch] = wave_sum(ssum[ch]);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    red_i[0][wave] = wsse; red_i[1][wave] = wcnt;
    red_d[0][wave] = ws[0]; red_d[1][wave] = ws[1]; red_d[2][wave] = ws[2];
  }
  __syncthreads();
  if (tid == 0) {
    Partial p{red_i[0][0], red_i[1][0], {red_d[0][0], red_d[1][0], red_d[2][0]}};
    for (int w = 1; w < kWaves; ++w) {
      p.sse += red_i[0][w]; p.cnt += red_i[1][w];
      p.s[0] += red_d[0][w]; p.s[1] += red_d[1][w]; p.s[2] += red_d[2][w];
    }
    a.part[(size_t)v * a.tiles + t] = p;
  }
}

// one workgroup per view: thread k sums tiles k, k + 256, ... in order, then the fixed-order workgroup sum.
// out[v] = (sse, count, mean over channels of the cropped S means)
__global__ __launch_bounds__(kThreads) void nvs_finish_kernel(const Partial* __restrict__ part, int tiles, double n_valid,
                                                              double* __restrict__ out) {
  __shared__ long long red_i[2][kWaves];
  __shared__ double red_d[3][kWaves];
  const int tid = threadIdx.x, v = blockIdx.x;
  const Partial* p = part + (size_t)v * tiles;
  long long sse = 0, cnt = 0;
  double s[3] = {0.0, 0.0, 0.0};
  for (int t = tid; t < tiles; t += kThreads) {
    sse += p[t].sse; cnt += p[t].cnt;
    s[0] += p[t].s[0]; s[1] += p[t].s[1]; s[2] += p[t].s[2];
  }
  sse = wave_sum(sse); cnt = wave_sum(cnt);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) s[ch] = wave_sum(s[ch]);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    red_i[0][wave] = sse; red_i[1][wave] = cnt;
    red_d[0][wave] = s[0]; red_d[1][wave] = s[1]; red_d[2][wave] = s[2];
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) {
      red_i[0][0] += red_i[0][w]; red_i[1][0] += red_i[1][w];
      red_d[0][0] += red_d[0][w]; red_d[1][0] += red_d[1][w]; red_d[2][0] += red_d[2][w];
    }
    // np.mean of the three channel results: ((m0 + m1) + m2) / 3
    const double m = ((red_d[0][0] / n_valid + red_d[1][0] / n_valid) + red_d[2][0] / n_valid) / 3.0;
    out[3 * (size_t)v] = (double)red_i[0][0];
    out[3 * (size_t)v + 1] = (double)red_i[1][0];
    out[3 * (size_t)v + 2] = m;
  }
}

inline int check_sizes(const char* what, int V, int H, int W) {
  if (V < 1) { set_error("%s: V must be >= 1", what); return SVS_EINVAL; }
  if (H < 2 * kR + 1 || W < 2 * kR + 1 || (long long)H * W > (1LL << 28)) {
    set_error("%s: H and W must be >= 7 (the SSIM window) with H*W <= 2^28", what); return SVS_ESHAPE;
  }
  if ((long long)V * Grid(H, W).tiles > 0x7fffffffLL) {
    set_error("%s: V * tiles exceeds the launch grid", what); return SVS_ESHAPE;
  }
  return SVS_OK;
}

}  // namespace nvs
}  // namespace svs

using namespace svs;
using namespace svs::nvs;

extern "C" {

size_t svs_nvs_workspace_bytes(int V, int H, int W) {
  if (V < 1 || H < 2 * kR + 1 || W < 2 * kR + 1) return 0;
  return (size_t)V * (size_t)Grid(H, W).tiles * sizeof(Partial);
}

int svs_nvs_score(const uint8_t* pred, const uint8_t* gt, const uint8_t* mask, int V, int H, int W, void* workspace,
                  double* out, void* hip_stream) {
  if (!pred || !gt || !mask || !workspace || !out) { set_error("svs_nvs_score: null argument"); return SVS_EINVAL; }
  int rc = check_sizes("svs_nvs_score", V, H, W);
  if (rc) return rc;
  const Grid g(H, W);
  hipStream_t s = (hipStream_t)hip_stream;
  Partial* part = (Partial*)workspace;
  TileArgs a{pred, gt, mask, H, W, g.tiles_x, (int)g.tiles, part};
  nvs_tile_kernel<<<(unsigned)(V * g.tiles), kThreads, 0, s>>>(a);
  if ((rc = check_launch("svs_nvs_score(tiles)"))) return rc;
  const double n_valid = (double)(H - 2 * kR) * (double)(W - 2 * kR);
  nvs_finish_kernel<<<V, kThreads, 0, s>>>(part, (int)g.tiles, n_valid, out);
  return check_launch("svs_nvs_score(finish)");
}

}  // extern "C"
