// Image-based rendering of one evaluation view for gfx950 (simple_ibr.py:116-235): the source images warped into the
// view through the rendered depths, weighted by geometric consistency and ray-direction agreement, and Laplacian-
// blended with the volume render.
//
// Reference: simple_ibr.py image_based_render (the per-view loop after check_geometric_consistency), Laplacian_Blending
// and get_lpIMG, with OpenCV's remap(INTER_CUBIC, BORDER_CONSTANT 0), erode(5x5, default border), pyrDown and pyrUp
// restated from their documented algorithms (tests/ibr_oracle.py).  The geometry (maps, geometric masks) comes from
// svs_fuse_view and the unit ray directions from svs_rays_from_uv; everything here is float32 storage and arithmetic.
// The reference keeps float32 up to the blend and runs the pyramids in float64: the float32 pyramids here sit within
// a few 1e-7 of it (tests/test_gpu_ibr.py).
//
// Two stages, each its own entry:
//   weights: one thread per reference pixel over the n_src <= 16 sources (cubic samples of image and direction,
//            cos_dir, masked weight, (n_src+1)-way softmax, fill images), then a 5x5 erosion of w > 0.2 through an LDS
//            tile with a 2-pixel halo, normalised masks;
//   blend:   pyrDown to levels 1..3 for every image and mask plane at once, then per level the blended Laplacian
//            sum_j m_jl (g_jl - up(g_j,l+1)) plus up(out_l+1), with every up() formed on the fly.
// Memory- and latency-bound gathers and stencils: no matrix cores.
#include "svs_image.h"

namespace svs {
namespace ibr {

using namespace svs::image;

constexpr int kMaxSrc = 16;
constexpr int kLevels = 4;            // Laplacian_Blending(num_levels=4): levels 0..3 are used
constexpr int kErodeTile = 16;        // erosion: 16x16 outputs per workgroup, 20x20 LDS tile
constexpr int kErodeHalo = 2;
constexpr size_t kAlign = 256;

inline size_t align_up(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

// Workspace layout, byte offsets: softmax weights (n_src+1,H,W) f32, w > 0.2 (n_src,H,W) u8, then for levels 1..3 the
// Gaussian image planes (n_src+1,h,w,3) and mask planes (n_src+1,h,w), then the reconstruction of levels 2 and 1 (h,w,3).
struct Layout {
  size_t weights, thr, gi[kLevels], gm[kLevels], out[kLevels - 1], total;
  Layout(int n_src, int H, int W) {
    const size_t nj = (size_t)n_src + 1, hw = (size_t)H * W;
    size_t o = 0;
    weights = o; o += align_up(nj * hw * 4);
    thr = o; o += align_up((size_t)n_src * hw);
    gi[0] = gm[0] = 0;                      // level 0: the caller's fill images and masks
    for (int l = 1; l < kLevels; ++l) {
      const size_t hwl = (size_t)(H >> l) * (W >> l);
      gi[l] = o; o += align_up(nj * hwl * 3 * 4);
      gm[l] = o; o += align_up(nj * hwl * 4);
    }
    out[0] = 0;                             // level 0: the caller's output
    for (int l = 1; l < kLevels - 1; ++l) {
      out[l] = o; o += align_up((size_t)(H >> l) * (W >> l) * 3 * 4);
    }
    total = o;
  }
};

// ---- cv2.remap(src, mapx, mapy, INTER_CUBIC), BORDER_CONSTANT 0, float32 (H,W,3) ----------------------------------
// The float maps become fixed point with 5 fractional bits (cvRound(x * 32), half to even); the 1-D weights are
// interpolateCubic(k / 32) with A = -0.75, the 2-D weight wy[i] * wx[j] in float32.  Inside (all 16 taps in the
// image) OpenCV sums each row left to right and adds the rows; otherwise it adds the in-image taps one by one from 0,
// and a window wholly outside gives 0.
__device__ __forceinline__ void cubic_coeffs(float x, float* c) {
  const float A = -0.75f;
  c[0] = ((A * (x + 1.0f) - 5.0f * A) * (x + 1.0f) + 8.0f * A) * (x + 1.0f) - 4.0f * A;
  c[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  c[2] = ((A + 2.0f) * (1.0f - x) - (A + 3.0f)) * (1.0f - x) * (1.0f - x) + 1.0f;
  c[3] = 1.0f - c[0] - c[1] - c[2];
}

struct CubicTap {
  int sx, sy;                         // top-left tap (ix - 1, iy - 1)
  int mode;                           // 0: wholly outside, 1: inside, 2: partly outside
  float w[16];
};

__device__ __forceinline__ void cubic_tap(float mx, float my, int H, int W, CubicTap& t) {
  const float fx32 = mx * 32.0f, fy32 = my * 32.0f;
  // cvRound of NaN / out-of-int-range gives INT_MIN on x86: far outside, as in svs_fusion.hip's remap_linear
  if (!(fx32 > -2.1e9f && fx32 < 2.1e9f) || !(fy32 > -2.1e9f && fy32 < 2.1e9f)) { t.mode = 0; return; }
  const int rx = (int)__builtin_rintf(fx32), ry = (int)__builtin_rintf(fy32);
  int ix = rx >> 5, iy = ry >> 5;
  ix = ix < -32768 ? -32768 : (ix > 32767 ? 32767 : ix);            // saturate_cast<short>
  iy = iy < -32768 ? -32768 : (iy > 32767 ? 32767 : iy);
  t.sx = ix - 1; t.sy = iy - 1;
  if (t.sx >= W || t.sx + 4 <= 0 || t.sy >= H || t.sy + 4 <= 0) { t.mode = 0; return; }
  t.mode = ((unsigned)t.sx < (unsigned)(W > 3 ? W - 3 : 0) && (unsigned)t.sy < (unsigned)(H > 3 ? H - 3 : 0)) ? 1 : 2;
  float wx[4], wy[4];
  cubic_coeffs((float)(rx & 31) * (1.0f / 32.0f), wx);
  cubic_coeffs((float)(ry & 31) * (1.0f / 32.0f), wy);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) t.w[i * 4 + j] = wy[i] * wx[j];
}

// the three channels of an (H,W,3) image at one tap window
__device__ __forceinline__ void cubic_sample3(const float* __restrict__ img, int H, int W, const CubicTap& t, float* o) {
  if (t.mode == 0) { o[0] = o[1] = o[2] = 0.0f; return; }
  if (t.mode == 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* S = img + ((size_t)(t.sy + i) * W + t.sx) * 3 + c;
        const float row = ((S[0] * t.w[i * 4] + S[3] * t.w[i * 4 + 1]) + S[6] * t.w[i * 4 + 2]) + S[9] * t.w[i * 4 + 3];
        sum = i ? sum + row : row;
      }
      o[c] = sum;
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float sum = 0.0f;                                      // cv * ONE with cv = 0; (S - cv) * w = S * w
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int y = t.sy + i;
      if (y < 0 || y >= H) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = t.sx + j;
        if (x >= 0 && x < W) sum = sum + img[((size_t)y * W + x) * 3 + c] * t.w[i * 4 + j];
      }
    }
    o[c] = sum;
  }
}

struct WeightArgs {
  const float* src_img[kMaxSrc];      // (H,W,3) each: read_img, uint8 / 255
  const float* src_dir[kMaxSrc];      // (H,W,3) each: unit ray directions of the source camera at integer pixels
  const float* ref_dir;               // (H,W,3)
  const float* pred;                  // (H,W,3) the volume render of the reference view
  const uint8_t* geo;                 // (n_src,H,W)
  const float* map_x;                 // (n_src,H,W)
  const float* map_y;
  int n_src, H, W;
  float* weights;                     // workspace (n_src+1,H,W)
  uint8_t* thr;                       // workspace (n_src,H,W)
  float* fill;                        // (n_src+1,H,W,3)
};

// simple_ibr.py:171-205.  Three passes over the views so that no per-view value lives in a register array: the
// sampled colours and 20 * w go to fill / weights first, then exp, then the normalised weight and the fill image.
__global__ __launch_bounds__(256) void ibr_weights_kernel(WeightArgs a) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  const int HW = a.H * a.W;
  if (pix >= HW) return;
  const float r0 = a.ref_dir[3 * pix], r1 = a.ref_dir[3 * pix + 1], r2 = a.ref_dir[3 * pix + 2];
  float mx = 0.0f;
  for (int v = 0; v < a.n_src; ++v) {
    const size_t o = (size_t)v * HW + pix;
    CubicTap t;
    cubic_tap(a.map_x[o], a.map_y[o], a.H, a.W, t);
    float col[3], d[3];
    cubic_sample3(a.src_img[v], a.H, a.W, t, col);
    cubic_sample3(a.src_dir[v], a.H, a.W, t, d);
    // sampled_src_dir /= np.linalg.norm(..., axis=2): squares summed left to right (0 / 0 gives NaN)
    const float n = __builtin_sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const float q0 = d[0] / n, q1 = d[1] / n, q2 = d[2] / n;
    float cs = (q0 * r0 + q1 * r1) + q2 * r2;
    // np.nan_to_num, then *= geo_mask
    if (__builtin_isnan(cs)) cs = 0.0f;
    else if (__builtin_isinf(cs)) cs = cs > 0.0f ? 3.4028234663852886e38f : -3.4028234663852886e38f;
    const float w = a.geo[o] ? cs : 0.0f;
    const float s = 20.0f * w;                             // softmax(20 * weight_masks, axis=0)
    mx = v == 0 ? s : __builtin_fmaxf(mx, s);
    a.weights[o] = s;
    float* f = a.fill + 3 * o;
    f[0] = col[0]; f[1] = col[1]; f[2] = col[2];
  }
  const float s_last = 20.0f * 0.2f;                       // the render's constant weight 0.2
  mx = __builtin_fmaxf(mx, s_last);
  float sum = 0.0f;
  for (int v = 0; v < a.n_src; ++v) {
    const size_t o = (size_t)v * HW + pix;
    const float e = expf(a.weights[o] - mx);
    a.weights[o] = e;
    sum = v == 0 ? e : sum + e;                            // np.sum over axis 0: in view order
  }
  const float e_last = expf(s_last - mx);
  sum = sum + e_last;
  const float p0 = a.pred[3 * pix], p1 = a.pred[3 * pix + 1], p2 = a.pred[3 * pix + 2];
  // fill: imgs * w + imgs[-1] * (1 - w); masks: w > 0.2 for the sources
  for (int v = 0; v < a.n_src; ++v) {
    const size_t o = (size_t)v * HW + pix;
    const float w = a.weights[o] / sum;
    a.weights[o] = w;
    a.thr[o] = w > 0.2f ? 1 : 0;
    float* f = a.fill + 3 * o;
    const float u = 1.0f - w;
    f[0] = f[0] * w + p0 * u; f[1] = f[1] * w + p1 * u; f[2] = f[2] * w + p2 * u;
  }
  const size_t o = (size_t)a.n_src * HW + pix;
  const float w = e_last / sum, u = 1.0f - w;
  a.weights[o] = w;
  float* f = a.fill + 3 * o;
  f[0] = p0 * w + p0 * u; f[1] = p1 * w + p1 * u; f[2] = p2 * w + p2 * u;
}

struct ErodeArgs {
  const float* weights;               // (n_src+1,H,W)
  const uint8_t* thr;                 // (n_src,H,W)
  int n_src, H, W;
  float* masks;                       // (n_src+1,H,W)
};

// simple_ibr.py:207-214: m_j = erode(w_j > 0.2, ones(5,5)) * w_j for the sources (pixels outside the image do not take
// part in the minimum), m_last = w_last + 1e-2, then m /= m.sum(0) summed in view order.
__global__ __launch_bounds__(kErodeTile * kErodeTile) void ibr_erode_kernel(ErodeArgs a) {
  constexpr int T = kErodeTile + 2 * kErodeHalo;
  __shared__ uint8_t tile[T][T];
  const int tx = threadIdx.x % kErodeTile, ty = threadIdx.x / kErodeTile;
  const int x0 = blockIdx.x * kErodeTile, y0 = blockIdx.y * kErodeTile;
  const int x = x0 + tx, y = y0 + ty;
  const bool live = x < a.W && y < a.H;
  const int HW = a.H * a.W;
  const size_t pix = live ? (size_t)y * a.W + x : 0;
  float sum = 0.0f;
  for (int v = 0; v < a.n_src; ++v) {
    const uint8_t* t = a.thr + (size_t)v * HW;
    for (int i = threadIdx.x; i < T * T; i += kErodeTile * kErodeTile) {
      const int gy = y0 - kErodeHalo + i / T, gx = x0 - kErodeHalo + i % T;
      tile[i / T][i % T] = (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) ? t[(size_t)gy * a.W + gx] : (uint8_t)1;
    }
    __syncthreads();
    uint8_t e = 1;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) e &= tile[ty + dy][tx + dx];
    __syncthreads();
    if (live) {
      const size_t o = (size_t)v * HW + pix;
      const float m = e ? a.weights[o] : 0.0f;
      a.masks[o] = m;
      sum = v == 0 ? m : sum + m;
    }
  }
  if (!live) return;
  const size_t ol = (size_t)a.n_src * HW + pix;
  const float ml = a.weights[ol] + 0.01f;
  sum = sum + ml;
  for (int v = 0; v < a.n_src; ++v) {
    const size_t o = (size_t)v * HW + pix;
    a.masks[o] = a.masks[o] / sum;
  }
  a.masks[ol] = ml / sum;
}

// ---- Gaussian pyramid: cv2.pyrDown, BORDER_REFLECT_101 (a level may be narrower than the 2-pixel halo) ------------------

struct DownArgs {
  const float* img;                   // (nj,h,w,3)
  const float* mask;                  // (nj,h,w)
  int nj, h, w;                       // source size; the destination is (h/2, w/2)
  float* img_out;
  float* mask_out;
};

// [1 4 6 4 1]^2 / 256 at the even rows and columns: each of the five source rows filtered horizontally, then the
// rows combined, in OpenCV's order (6 c + 4 (l + r) + ll + rr).  One thread per destination pixel and plane group
// (three image channels and the mask of one entry).
__global__ __launch_bounds__(256) void ibr_pyr_down_kernel(DownArgs a) {
  const int h2 = a.h >> 1, w2 = a.w >> 1;
  const int hw2 = h2 * w2;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.nj * hw2) return;
  const int j = gid / hw2, p = gid - j * hw2;
  const int y = p / w2, x = p - y * w2;
  int rows[5], cols[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    rows[k] = reflect101_any(2 * y - 2 + k, a.h);
    cols[k] = reflect101_any(2 * x - 2 + k, a.w);
  }
  const size_t base = (size_t)j * a.h * a.w;
  float acc[4], r[5];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float* src = c < 3 ? a.img + base * 3 + c : a.mask + base;
    const int st = c < 3 ? 3 : 1;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float* S = src + (size_t)rows[k] * a.w * st;
      r[k] = ((S[cols[2] * st] * 6.0f + (S[cols[1] * st] + S[cols[3] * st]) * 4.0f) + S[cols[0] * st]) + S[cols[4] * st];
    }
    acc[c] = (((r[2] * 6.0f + (r[1] + r[3]) * 4.0f) + r[0]) + r[4]) * (1.0f / 256.0f);
  }
  const size_t o = (size_t)j * hw2 + p;
  a.img_out[3 * o] = acc[0]; a.img_out[3 * o + 1] = acc[1]; a.img_out[3 * o + 2] = acc[2];
  a.mask_out[o] = acc[3];
}

// ---- cv2.pyrUp at one destination pixel ------------------------------------------------------------------------------
// Zeros injected to (2h, 2w), then 4 x the pyrDown kernel with BORDER_REFLECT_101 on the upsampled grid.  On the source
// grid: rows reflect at the top and replicate at the bottom; columns are 6 c + 2 r at the left edge, l + 7 c and 8 c at
// the right edge (one column: 8 c for both).  UpTap holds the source rows, the columns and the column formula.
enum UpCols { kUp8, kUpMid, kUpLeft, kUpRight, kUpOdd };

struct UpTap {
  int rows[3], cols[3];
  int kind;                           // UpCols
  bool odd_row;                       // 2 source rows (odd destination row) or 3
};

__device__ __forceinline__ void up_tap(int Y, int X, int h, int w, UpTap& t) {
  const int yy = Y >> 1, xx = X >> 1;
  t.odd_row = Y & 1;
  if (!t.odd_row) {
    t.rows[0] = reflect101_any(2 * (yy - 1), 2 * h) >> 1;
    t.rows[1] = yy;
    t.rows[2] = reflect101_any(2 * (yy + 1), 2 * h) >> 1;
  } else {
    t.rows[0] = yy;
    t.rows[1] = reflect101_any(2 * (yy + 1), 2 * h) >> 1;
    t.rows[2] = yy;
  }
  t.cols[0] = xx - 1; t.cols[1] = xx; t.cols[2] = xx + 1;
  if (w == 1) t.kind = kUp8;
  else if (X & 1) t.kind = xx == w - 1 ? kUp8 : kUpOdd;
  else t.kind = xx == 0 ? kUpLeft : (xx == w - 1 ? kUpRight : kUpMid);
}

// one source row filtered horizontally, in OpenCV's operation order
template <class F>
__device__ __forceinline__ float up_row(const UpTap& t, int r, F&& get) {
  switch (t.kind) {
    case kUp8: return get(r, t.cols[1]) * 8.0f;
    case kUpMid: return (get(r, t.cols[0]) + get(r, t.cols[1]) * 6.0f) + get(r, t.cols[2]);
    case kUpLeft: return get(r, t.cols[1]) * 6.0f + get(r, t.cols[2]) * 2.0f;
    case kUpRight: return get(r, t.cols[0]) + get(r, t.cols[1]) * 7.0f;
    default: return (get(r, t.cols[1]) + get(r, t.cols[2])) * 4.0f;
  }
}

// the vertical pass and the 1/64 scale
template <class F>
__device__ __forceinline__ float up_at(const UpTap& t, F&& get) {
  if (t.odd_row) return ((up_row(t, t.rows[0], get) + up_row(t, t.rows[1], get)) * 4.0f) * (1.0f / 64.0f);
  return ((up_row(t, t.rows[0], get) + up_row(t, t.rows[1], get) * 6.0f) + up_row(t, t.rows[2], get)) * (1.0f / 64.0f);
}

struct BlendArgs {
  const float* gi;                    // level l images (nj,h,w,3)
  const float* gm;                    // level l masks (nj,h,w)
  const float* gi_c;                  // level l+1 images (nj,h/2,w/2,3)
  const float* gm_c;                  // level l+1 masks: only when the coarse output is formed on the fly (l = 2)
  const float* out_c;                 // level l+1 reconstruction (h/2,w/2,3), or nullptr: sum_j m_j g_j of level l+1
  int nj, h, w;
  int clip;                           // last level: np.clip(0, 1)
  float* out;                         // (h,w,3)
};

// Laplacian_Blending (simple_ibr.py:103-136) at level l: LS_l = sum_j m_jl (g_jl - pyrUp(g_j,l+1)), accumulated from 0
// in entry order; out_l = pyrUp(out_l+1) + LS_l.  At the coarsest blended level out_3 = LS_3 = sum_j m_j3 g_j3 is formed
// where pyrUp reads it.
__global__ __launch_bounds__(256) void ibr_blend_level_kernel(BlendArgs a) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= a.h * a.w) return;
  const int Y = pix / a.w, X = pix - Y * a.w;
  const int hc = a.h >> 1, wc = a.w >> 1;
  const size_t hwc = (size_t)hc * wc, hw = (size_t)a.h * a.w;
  UpTap t;
  up_tap(Y, X, hc, wc, t);
  float ls[3] = {0.0f, 0.0f, 0.0f};
  for (int j = 0; j < a.nj; ++j) {
    const float m = a.gm[(size_t)j * hw + pix];
    const float* gc = a.gi_c + (size_t)j * hwc * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float up = up_at(t, [&](int r, int q) { return gc[((size_t)r * wc + q) * 3 + c]; });
      ls[c] = ls[c] + m * (a.gi[((size_t)j * hw + pix) * 3 + c] - up);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float prev;
    if (a.out_c) {
      prev = up_at(t, [&](int r, int q) { return a.out_c[((size_t)r * wc + q) * 3 + c]; });
    } else {
      prev = up_at(t, [&](int r, int q) {
        const size_t p = (size_t)r * wc + q;
        float s = 0.0f;
        for (int j = 0; j < a.nj; ++j) s = s + a.gm_c[(size_t)j * hwc + p] * a.gi_c[((size_t)j * hwc + p) * 3 + c];
        return s;
      });
    }
    float v = prev + ls[c];
    if (a.clip) v = __builtin_fminf(__builtin_fmaxf(v, 0.0f), 1.0f);
    a.out[(size_t)pix * 3 + c] = v;
  }
}

inline int check_sizes(const char* what, int n_src, int H, int W) {
  int rc = check_count(what, "n_src", n_src, kMaxSrc);
  if (rc || (rc = check_image(what, "H and W", H, W, 8))) return rc;
  if ((H & 7) || (W & 7)) { set_error("%s: H and W must be multiples of 8", what); return SVS_ESHAPE; }
  return SVS_OK;
}

}  // namespace ibr
}  // namespace svs

using namespace svs;
using namespace svs::ibr;

extern "C" {

size_t svs_ibr_workspace_bytes(int n_src, int H, int W) {
  // 0 for every size the two entries reject (check_sizes, without its error text)
  if (n_src < 1 || n_src > kMaxSrc || H < 8 || W < 8 || (H & 7) || (W & 7) || (long long)H * W > kMaxPixels) return 0;
  return Layout(n_src, H, W).total;
}

int svs_ibr_weights(const float* const* src_imgs, const float* const* src_dirs, const float* ref_dir, const float* pred_img,
                    const uint8_t* geo_mask, const float* map_x, const float* map_y, int n_src, int H, int W,
                    void* workspace, float* fill, float* masks, void* hip_stream) {
  if (!src_imgs || !src_dirs || !ref_dir || !pred_img || !geo_mask || !map_x || !map_y || !workspace || !fill || !masks) {
    set_error("svs_ibr_weights: null argument"); return SVS_EINVAL;
  }
  int rc = check_sizes("svs_ibr_weights", n_src, H, W);
  if (rc) return rc;
  const Layout L(n_src, H, W);
  WeightArgs a;
  for (int v = 0; v < kMaxSrc; ++v) { a.src_img[v] = nullptr; a.src_dir[v] = nullptr; }
  for (int v = 0; v < n_src; ++v) {
    if (!src_imgs[v] || !src_dirs[v]) { set_error("svs_ibr_weights: null source %d", v); return SVS_EINVAL; }
    a.src_img[v] = src_imgs[v]; a.src_dir[v] = src_dirs[v];
  }
  a.ref_dir = ref_dir; a.pred = pred_img; a.geo = geo_mask; a.map_x = map_x; a.map_y = map_y;
  a.n_src = n_src; a.H = H; a.W = W;
  a.weights = (float*)((char*)workspace + L.weights); a.thr = (uint8_t*)workspace + L.thr; a.fill = fill;
  hipStream_t s = (hipStream_t)hip_stream;
  ibr_weights_kernel<<<(H * W + 255) / 256, 256, 0, s>>>(a);
  rc = check_launch("svs_ibr_weights");
  if (rc) return rc;
  ErodeArgs e{a.weights, a.thr, n_src, H, W, masks};
  dim3 grid((W + kErodeTile - 1) / kErodeTile, (H + kErodeTile - 1) / kErodeTile);
  ibr_erode_kernel<<<grid, kErodeTile * kErodeTile, 0, s>>>(e);
  return check_launch("svs_ibr_weights(erode)");
}

int svs_ibr_laplacian_blend(const float* fill, const float* masks, int n_src, int H, int W, void* workspace, float* out,
                            void* hip_stream) {
  if (!fill || !masks || !workspace || !out) { set_error("svs_ibr_laplacian_blend: null argument"); return SVS_EINVAL; }
  int rc = check_sizes("svs_ibr_laplacian_blend", n_src, H, W);
  if (rc) return rc;
  const Layout L(n_src, H, W);
  const int nj = n_src + 1;
  char* ws = (char*)workspace;
  const float* gi[kLevels] = {fill, (float*)(ws + L.gi[1]), (float*)(ws + L.gi[2]), (float*)(ws + L.gi[3])};
  const float* gm[kLevels] = {masks, (float*)(ws + L.gm[1]), (float*)(ws + L.gm[2]), (float*)(ws + L.gm[3])};
  hipStream_t s = (hipStream_t)hip_stream;
  for (int l = 0; l + 1 < kLevels; ++l) {
    const int h = H >> l, w = W >> l;
    DownArgs d{gi[l], gm[l], nj, h, w, (float*)gi[l + 1], (float*)gm[l + 1]};
    const int n = nj * (h >> 1) * (w >> 1);
    ibr_pyr_down_kernel<<<(n + 255) / 256, 256, 0, s>>>(d);
    if ((rc = check_launch("svs_ibr_laplacian_blend(pyrDown)"))) return rc;
  }
  // levels 2, 1, 0; level 3's output is formed inside level 2's pyrUp
  float* outs[kLevels - 1] = {out, (float*)(ws + L.out[1]), (float*)(ws + L.out[2])};
  for (int l = kLevels - 2; l >= 0; --l) {
    const int h = H >> l, w = W >> l;
    BlendArgs b{gi[l], gm[l], gi[l + 1], gm[l + 1], l == kLevels - 2 ? nullptr : outs[l + 1], nj, h, w, l == 0, outs[l]};
    ibr_blend_level_kernel<<<(h * w + 255) / 256, 256, 0, s>>>(b);
    if ((rc = check_launch("svs_ibr_laplacian_blend(level)"))) return rc;
  }
  return SVS_OK;
}

}  // extern "C"
