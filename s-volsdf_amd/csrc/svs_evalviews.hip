// The per-view "finish" of evaluation rendering for gfx950 (eval_vsdf.py:230-262, volsdf/utils/plots.py:392-468): what
// the reference does in numpy on the host after merge_output, on the render's own device tensors.  What leaves the
// device per view is four small images instead of the (N,S) weights.  Restated in numpy in tests/evalviews_oracle.py.
//
// svs_view_finish: ONE pass over weights (N,S), the only large input (576x768, S = 98: 173 MB).
//   A wavefront owns 64 consecutive rays.  It walks them as 16 "row sets" of 4 rows: 4 S consecutive floats, which
//   start on a 16-byte boundary whatever S is, so a set is read as S float4 loads, lane after lane (coalesced; the
//   unaligned-base and the last-partial-vector cases fall back to guarded 4-byte loads of the SAME elements).  A
//   float4 can straddle two rows, so every lane keeps four partial sums, one per row of the set, and adds each element
//   to the sum of the row it belongs to, in element order; a 6-step xor butterfly then folds the 64 lanes.  The
//   order of additions depends on S and on the row's position in its set only: acc is bit-identical run after run.
//   Lane i of the wavefront keeps row i's sum, so the epilogue is one ray per lane:
//     rgb_codes    = (rgb * 255).astype(uint8)                  float32 multiply, see to_code()
//     normal_codes = (((n + 1) / 2) * 255).astype(uint8)        three float32 operations in that order
//     depth_est    = depth_values * scale_factor                one float32 multiply
//   to_code restates x86 numpy's float -> uint8 cast: truncate toward zero to int32, keep the low 8 bits (-1.5 -> 255,
//   300.7 -> 44, 1e6 -> 64).  Outside the int32 range and for NaN the x86 conversion yields 0x80000000, code 0.
//
// svs_view_depth_colors: visualize_depth's colour step, one pixel per lane.  numpy carries the colour table, the
//   checker and the matte in float64; so does this kernel (N double operations per view are free next to the render,
//   and a float32 matte would leave the final value up to ~3e-5 code units from numpy's, enough to flip a code).
//   What numpy computes in float32 -- (1 - acc) -- is float32 here too.
//
// No LDS, no scratch, plain vector stores.  No fma contraction (build.py).
#include "svs_common.h"

#include <climits>
#include <cmath>

namespace svs {
namespace evalviews {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kSetRows = 4;                              // rows per row set: 4 S floats are a whole number of float4
constexpr int kMaxSamples = 1 << 14;

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint8_t to_code(float x) {
  const int v = fabsf(x) < 2147483648.0f ? (int)x : INT_MIN;
  return (uint8_t)(v & 255);
}

__device__ __forceinline__ uint8_t to_code(double x) {
  const int v = fabs(x) < 2147483648.0 ? (int)x : INT_MIN;
  return (uint8_t)(v & 255);
}

struct FinishArgs {
  const float* rgb;                                     // (N,3)
  const float* normal;                                  // (N,3)
  const float* depth;                                   // (N)
  const float* weights;                                 // (N,S)
  uint8_t* rgb_codes;                                   // (N,3)
  uint8_t* normal_codes;                                // (N,3)
  float* depth_est;                                     // (N)
  float* acc;                                           // (N)
  int N, S;
  float scale;
  int vec;                                              // weights is 16-byte aligned
};

__global__ __launch_bounds__(kThreads) void view_finish_kernel(FinishArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long wave = (long long)blockIdx.x * (kThreads / kWave) + (threadIdx.x / kWave);
  const long long row0 = wave * kWave;                   // wave-uniform
  if (row0 >= a.N) return;
  const long long total = (long long)a.N * a.S;
  const int S = a.S;
  float mine = 0.0f;                                     // the sum of row row0 + lane
#pragma unroll 1
  for (int set = 0; set < kWave / kSetRows; ++set) {
    const long long r = row0 + (long long)set * kSetRows;
    if (r >= a.N) break;                                 // wave-uniform
    const long long base = r * S;                        // first float of the set: a multiple of 4
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (int j = lane; j < S; j += kWave) {              // S float4 per set
      const long long g = base + 4LL * j;
      float e[4];
      if (a.vec && g + 4 <= total) {
        const f4 v = __builtin_nontemporal_load((const f4*)(a.weights + g));
        e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = g + k < total ? a.weights[g + k] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = 4 * j + k;                         // element of the set; its row is q / S
        const int row = (q >= S) + (q >= 2 * S) + (q >= 3 * S);
        s0 += row == 0 ? e[k] : 0.0f;
        s1 += row == 1 ? e[k] : 0.0f;
        s2 += row == 2 ? e[k] : 0.0f;
        s3 += row == 3 ? e[k] : 0.0f;
      }
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
      s0 += __shfl_xor(s0, m, kWave);
      s1 += __shfl_xor(s1, m, kWave);
      s2 += __shfl_xor(s2, m, kWave);
      s3 += __shfl_xor(s3, m, kWave);
    }
    if ((lane >> 2) == set) {
      const int q = lane & 3;
      mine = q == 0 ? s0 : (q == 1 ? s1 : (q == 2 ? s2 : s3));
    }
  }
  const long long i = row0 + lane;
  if (i >= a.N) return;
  a.acc[i] = mine;
  a.depth_est[i] = a.depth[i] * a.scale;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.rgb_codes[3 * i + c] = to_code(a.rgb[3 * i + c] * 255.0f);
    const float n = (a.normal[3 * i + c] + 1.0f) / 2.0f;
    a.normal_codes[3 * i + c] = to_code(n * 255.0f);
  }
}

struct ColorArgs {
  const float* depth;                                   // (N) unscaled depth_values
  const float* acc;                                     // (N)
  const double* table;                                  // (table_len,3)
  uint8_t* codes;                                       // (N,3)
  int N, W, table_len;
  double lo, span;                                      // min(curve(lo), curve(hi)), |curve(hi) - curve(lo)|
};

__global__ __launch_bounds__(kThreads) void depth_colors_kernel(ColorArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  const double eps = (double)1.1920928955078125e-07f;    // np.finfo(np.float32).eps
  const double c = -log((double)a.depth[i] + eps);
  double v = (c - a.lo) / a.span;
  v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);               // np.clip keeps NaN
  if (v != v) v = 0.0;                                   // np.nan_to_num
  double xa = v * (double)a.table_len;                   // matplotlib's index rule: 1.0 belongs to the last entry
  if (xa == (double)a.table_len) xa = (double)(a.table_len - 1);
  int idx = (int)xa;
  idx = idx < 0 ? 0 : (idx > a.table_len - 1 ? a.table_len - 1 : idx);
  const int y = i / a.W, x = i - y * a.W;
  const bool light = (((y & 15) >> 3) ^ ((x & 15) >> 3)) != 0;      // the 8-pixel checker
  const double bg = light ? 1.0 : 0.8;
  const float w = a.acc[i];
  const double rest = bg * (double)(1.0f - w);           // numpy: 1 - acc stays float32
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double col = a.table[3 * idx + ch] * (double)w + rest;
    a.codes[3 * i + ch] = to_code(col * 255.0);
  }
}

}  // namespace evalviews
}  // namespace svs

using namespace svs;
using namespace svs::evalviews;

extern "C" {

int svs_view_finish(const float* rgb_values, const float* normal_map, const float* depth_values, const float* weights,
                    int n_pixels, int n_samples, float scale_factor, uint8_t* rgb_codes, uint8_t* normal_codes,
                    float* depth_est, float* acc, void* hip_stream) {
  const char* what = "svs_view_finish";
  if (!rgb_values || !normal_map || !depth_values || !weights || !rgb_codes || !normal_codes || !depth_est || !acc) {
    set_error("%s: null argument", what); return SVS_EINVAL;
  }
  if (n_pixels < 1 || n_pixels > (1 << 26)) { set_error("%s: n_pixels must be in 1..2^26", what); return SVS_ESHAPE; }
  if (n_samples < 1 || n_samples > kMaxSamples) {
    set_error("%s: n_samples must be in 1..%d", what, kMaxSamples); return SVS_ESHAPE;
  }
  FinishArgs a{rgb_values, normal_map, depth_values, weights, rgb_codes, normal_codes, depth_est, acc,
               n_pixels, n_samples, scale_factor, ((uintptr_t)weights & 15) == 0 ? 1 : 0};
  const unsigned blocks = (unsigned)(((long long)n_pixels + kThreads - 1) / kThreads);
  view_finish_kernel<<<blocks, kThreads, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch(what);
}

int svs_view_depth_colors(const float* depth, const float* acc, int n_pixels, int width, double lo, double hi,
                          const double* table, int table_len, uint8_t* codes, void* hip_stream) {
  const char* what = "svs_view_depth_colors";
  if (!depth || !acc || !table || !codes) { set_error("%s: null argument", what); return SVS_EINVAL; }
  if (n_pixels < 1 || n_pixels > (1 << 26) || width < 1 || n_pixels % width != 0) {
    set_error("%s: n_pixels must be in 1..2^26 and a multiple of width >= 1", what); return SVS_ESHAPE;
  }
  if (table_len < 1 || table_len > 65536) { set_error("%s: table_len must be in 1..65536", what); return SVS_ESHAPE; }
  const double eps = (double)1.1920928955078125e-07f;
  const double cl = -std::log(lo + eps), ch = -std::log(hi + eps);  // the curve of visualize_depth on the two bounds
  ColorArgs a{depth, acc, table, codes, n_pixels, width, table_len, cl < ch ? cl : ch, std::fabs(ch - cl)};
  if (cl != cl || ch != ch) a.lo = cl + ch;                          // np.minimum propagates NaN
  depth_colors_kernel<<<(n_pixels + kThreads - 1) / kThreads, kThreads, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch(what);
}

}  // extern "C"
