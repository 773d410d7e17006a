// Alpha compositing for gfx950, forward and backward, foreground-only and with the inverted-sphere background.
//
// Reference: volsdf/model/network.py:281-295 (volume_rendering) and :237-256,270-276 (the weighted reductions);
// volsdf/model/network_bg.py:76-125, 147-180 (fg / bg volume rendering and the composition).
// Compiled with -ffp-contract=off: same numeric contract as the sampler (svs_sampler.hip).  Every kernel is the sequence
// functions of svs_ray_scan.h applied to its sample sequences, plus its own last interval and reductions.
#include <initializer_list>

#include "svs_ray_scan.h"

namespace svs {
namespace composite {

constexpr int kMaxS = 256;    // samples of a foreground sequence held per ray
constexpr int kMaxBg = 64;    // inverse-sphere samples per ray

struct CompositeArgs {
  int R, S;
  const float* z;            // (R,S)
  const float* sdf;          // (R*S)
  const float* rgb;          // (R*S,3)
  const float* normals;      // (R*S,3) or nullptr
  const float* depth_scale;  // (R)
  const float* beta_param;   // device scalar: density.beta; beta = |beta| + beta_min (density.py:28-30)
  float beta_min;
  float* weights;            // (R,S)
  float* rgb_values;         // (R,3)
  float* depth_values;       // (R)
  float* depth_vals;         // (R,S) = z * depth_scale
  float* normal_map;         // (R,3) or nullptr
};

// sum_i w_i * v_i / |v_i| of a lane's samples: the normal map's summand (gradients.norm(2, -1))
__device__ __forceinline__ void add_normal(const float* normals, size_t p, float w, float& n0, float& n1, float& n2) {
  const float g0 = normals[3 * p], g1 = normals[3 * p + 1], g2 = normals[3 * p + 2];
  const float nn = norm3(g0, g1, g2);
  n0 += w * (g0 / nn); n1 += w * (g1 / nn); n2 += w * (g2 / nn);
}

__global__ __launch_bounds__(64) void composite_kernel(CompositeArgs a) {
  __shared__ float zs[kMaxS], fe[kMaxS], pre[kMaxS];
  const int r = blockIdx.x, lane = threadIdx.x, S = a.S;
  const float beta = __builtin_fabsf(*a.beta_param) + a.beta_min;
  for (int i = lane; i < S; i += 64) zs[i] = a.z[(size_t)r * S + i];
  __syncthreads();
  for (int i = lane; i < S; i += 64) {
    const float dist = i < S - 1 ? zs[i + 1] - zs[i] : 1e10f;
    fe[i] = dist * laplace_density(a.sdf[(size_t)r * S + i], beta);
  }
  __syncthreads();
  float sw = 0.0f, swz = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
  const float ds = a.depth_scale[r];
  seq_weights(fe, pre, S, S, lane, [&](int i, float w) {
    const size_t p = (size_t)r * S + i;
    a.weights[p] = w;
    a.depth_vals[p] = zs[i] * ds;
    sw += w; swz += w * zs[i];
    c0 += w * a.rgb[3 * p]; c1 += w * a.rgb[3 * p + 1]; c2 += w * a.rgb[3 * p + 2];
    if (a.normal_map) add_normal(a.normals, p, w, n0, n1, n2);
  });
  sw = wave_sum(sw); swz = wave_sum(swz); c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
  if (a.normal_map) { n0 = wave_sum(n0); n1 = wave_sum(n1); n2 = wave_sum(n2); }
  if (lane == 0) {
    a.rgb_values[3 * r] = c0; a.rgb_values[3 * r + 1] = c1; a.rgb_values[3 * r + 2] = c2;
    a.depth_values[r] = ds * (swz / (sw + 1e-8f));
    if (a.normal_map) { a.normal_map[3 * r] = n0; a.normal_map[3 * r + 1] = n1; a.normal_map[3 * r + 2] = n2; }
  }
}

// ---- backward: d(loss)/d(sdf, rgb, beta) from d(loss)/d(rgb_values, weights, depth_values) -----------------
// Forward (network.py:281-295): fe_i = dist_i * sigma(sdf_i, beta), w_i = (1 - exp(-fe_i)) * exp(-sum_{j<i} fe_j);
// rgb_values = sum w_i c_i, depth_values = ds * sum(w_i z_i) / (sum w_i + 1e-8).  Hand-derived reverse pass: dL/dfe_k by
// seq_weights_bwd, then
//   dsigma/dsdf = -exp(-|s|/beta) / (2 beta^2),  dsigma/dbeta = -sigma/beta + sgn(s) exp(-|s|/beta) |s| / (2 beta^3)
struct CompositeBwdArgs {
  int R, S;
  const float* z; const float* sdf; const float* rgb; const float* depth_scale;
  const float* beta_param; float beta_min;
  const float* d_rgb_values;   // (R,3)
  const float* d_weights;      // (R,S) or nullptr
  const float* d_depth_values; // (R) or nullptr
  float* d_sdf;                // (R*S)
  float* d_rgb;                // (R*S,3)
  float* d_beta_ray;           // (R): per-ray d loss / d beta (summed by beta_reduce_kernel)
};

// a sample of weight w and colour c = rgb[p]: writes d loss / d c = w * g, returns c . g, the colour term of d loss / d w
__device__ __forceinline__ double colour_grad(const float* rgb, size_t p, double w, double g0, double g1, double g2,
                                              float* d_rgb) {
  d_rgb[3 * p] = (float)(w * g0); d_rgb[3 * p + 1] = (float)(w * g1); d_rgb[3 * p + 2] = (float)(w * g2);
  return ((double)rgb[3 * p] * g0 + (double)rgb[3 * p + 1] * g1) + (double)rgb[3 * p + 2] * g2;
}

__global__ __launch_bounds__(64) void composite_bwd_kernel(CompositeBwdArgs a) {
  __shared__ double zs[kMaxS], fe[kMaxS], tr[kMaxS], dw[kMaxS], wt[kMaxS];
  const int r = blockIdx.x, lane = threadIdx.x, S = a.S;
  const double beta = (double)(__builtin_fabsf(*a.beta_param) + a.beta_min);
  for (int i = lane; i < S; i += 64) zs[i] = (double)a.z[(size_t)r * S + i];
  __syncthreads();
  auto dist = [&](int i) { return i < S - 1 ? (double)(float)(zs[i + 1] - zs[i]) : 1e10; };   // (the forward's float32 distance)
  for (int i = lane; i < S; i += 64) fe[i] = dist(i) * DensityD((double)a.sdf[(size_t)r * S + i], beta).sigma;
  __syncthreads();
  double sw = 0.0, swz = 0.0;
  seq_weights(fe, tr, wt, S, S, lane, [&](int i, double w) { sw += w; swz += w * zs[i]; });
  sw = wave_sum(sw); swz = wave_sum(swz);
  const double ds = (double)a.depth_scale[r];
  const double g0 = a.d_rgb_values[3 * r], g1 = a.d_rgb_values[3 * r + 1], g2 = a.d_rgb_values[3 * r + 2];
  const double gd = a.d_depth_values ? (double)a.d_depth_values[r] * ds : 0.0;
  const double den = sw + 1e-8;
  for (int i = lane; i < S; i += 64) {
    const size_t p = (size_t)r * S + i;
    double d = colour_grad(a.rgb, p, wt[i], g0, g1, g2, a.d_rgb);
    if (a.d_weights) d += (double)a.d_weights[p];
    d += gd * (zs[i] * den - swz) / (den * den);
    dw[i] = d;
  }
  __syncthreads();
  double dbeta = 0.0;
  seq_weights_bwd(fe, tr, wt, dw, S, lane, [&](int i, double dfe) {
    const size_t p = (size_t)r * S + i;
    const double dsig = dfe * dist(i);
    const DensityD dn((double)a.sdf[p], beta);
    a.d_sdf[p] = (float)(dsig * dn.dsig_dsdf);
    // exp(-fe) underflows long before dist = 1e10 matters; guard the 0 * inf of the last sample
    if (dfe != 0.0) dbeta += dsig * dn.dsig_dbeta;
  });
  dbeta = wave_sum(dbeta);
  if (lane == 0) a.d_beta_ray[r] = (float)dbeta;
}

// d loss / d density.beta = sign(beta_param) * sum over rays (float64, fixed order -> reproducible)
__global__ __launch_bounds__(256) void beta_reduce_kernel(const float* __restrict__ d_beta_ray, int R,
                                                          const float* __restrict__ beta_param, float* __restrict__ out,
                                                          int accumulate) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < R; i += 256) acc += (double)d_beta_ray[i];
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    const float bp = *beta_param;
    const float sg = bp > 0.0f ? 1.0f : (bp < 0.0f ? -1.0f : 0.0f);
    const float v = sg * (float)t;
    out[0] = accumulate ? out[0] + v : v;
  }
}

// ---- BG model: two sequences per ray.  The foreground's last interval ends at the sphere exit z_max, so its free energies
// are all finite and their total gives the transmittance in front of the background; the inverse-sphere sequence
// (descending inverse depths) carries the 1e10 interval.
struct CompositeBgArgs : CompositeArgs {     // (S = 97 fg samples, whose last interval ends at z_max)
  int Nb;                    // bg samples (32)
  const float* z_max;        // (R) sphere exit
  const float* z_bg;         // (R,Nb) descending inverse depths
  const float* bg_out0;      // (R*Nb) raw bg output[:,0]; density = |.|
  const float* bg_rgb;       // (R*Nb,3)
  const float* bg_depth;     // (R,Nb) conventional depths of the bg samples
  float* bg_trans;           // (R) transmittance behind the last fg sample
  float* bg_weights;         // (R,Nb)
  float* depth_values_all;   // (R)
};

// VolSDFNetworkBG.volume_rendering / bg_volume_rendering and the composition (network_bg.py:76-125, 147-180)
__global__ __launch_bounds__(64) void composite_bg_kernel(CompositeBgArgs a) {
  __shared__ float zs[kMaxS], fe[kMaxS], pre[kMaxS], bfe[kMaxBg], bpre[kMaxBg];
  const int r = blockIdx.x, lane = threadIdx.x, S = a.S, Nb = a.Nb;
  const float beta = __builtin_fabsf(*a.beta_param) + a.beta_min;
  for (int i = lane; i < S; i += 64) zs[i] = a.z[(size_t)r * S + i];
  for (int i = lane; i < Nb; i += 64) bpre[i] = a.z_bg[(size_t)r * Nb + i];
  __syncthreads();
  for (int i = lane; i < S; i += 64) {
    const float dist = i < S - 1 ? zs[i + 1] - zs[i] : a.z_max[r] - zs[i];
    fe[i] = dist * laplace_density(a.sdf[(size_t)r * S + i], beta);
  }
  for (int i = lane; i < Nb; i += 64) {
    const float dist = i < Nb - 1 ? bpre[i] - bpre[i + 1] : 1e10f;
    bfe[i] = dist * __builtin_fabsf(a.bg_out0[(size_t)r * Nb + i]);
  }
  __syncthreads();
  const float ds = a.depth_scale[r];
  float sw = 0.0f, swz = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, swa = 0.0f, swd = 0.0f;
  seq_weights(fe, pre, S, S + 1, lane, [&](int i, float w) {       // S + 1 prefixes: the last is the total
    const size_t p = (size_t)r * S + i;
    a.weights[p] = w;
    const float dv = zs[i] * ds;
    a.depth_vals[p] = dv;
    sw += w; swz += w * dv; swa += w; swd += w * (ds * zs[i]);
    c0 += w * a.rgb[3 * p]; c1 += w * a.rgb[3 * p + 1]; c2 += w * a.rgb[3 * p + 2];
    if (a.normal_map) add_normal(a.normals, p, w, n0, n1, n2);
  });
  const float tbg = sleef_expf(-pre[S]);
  float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
  seq_weights(bfe, bpre, Nb, Nb, lane, [&](int i, float bw) {
    const size_t p = (size_t)r * Nb + i;
    a.bg_weights[p] = bw;
    b0 += bw * a.bg_rgb[3 * p]; b1 += bw * a.bg_rgb[3 * p + 1]; b2 += bw * a.bg_rgb[3 * p + 2];
    const float wa = tbg * bw;
    swa += wa; swd += wa * (ds * a.bg_depth[p]);
  });
  sw = wave_sum(sw); swz = wave_sum(swz); c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
  b0 = wave_sum(b0); b1 = wave_sum(b1); b2 = wave_sum(b2); swa = wave_sum(swa); swd = wave_sum(swd);
  if (a.normal_map) { n0 = wave_sum(n0); n1 = wave_sum(n1); n2 = wave_sum(n2); }
  if (lane == 0) {
    a.bg_trans[r] = tbg;
    a.rgb_values[3 * r] = c0 + tbg * b0; a.rgb_values[3 * r + 1] = c1 + tbg * b1; a.rgb_values[3 * r + 2] = c2 + tbg * b2;
    a.depth_values[r] = swz / (sw + 1e-8f);
    a.depth_values_all[r] = swd / (swa + 1e-8f);
    if (a.normal_map) { a.normal_map[3 * r] = n0; a.normal_map[3 * r + 1] = n1; a.normal_map[3 * r + 2] = n2; }
  }
}

struct CompositeBgBwdArgs : CompositeBwdArgs {     // (d_depth_values: of the fg depth of network_bg.py:111-112)
  int Nb;
  const float* z_max; const float* z_bg; const float* bg_out0; const float* bg_rgb;
  const float* d_depth_all;    // (R) or nullptr: gradient of depth_values_all (network_bg.py:105-107) -- what the sparsity
                               // term of the loss reads (loss.py:72-73); needs bg_depth
  const float* bg_depth;       // (R,Nb) conventional depths of the inverse-sphere samples (with d_depth_all)
  float* d_bg_out0;            // (R*Nb)
  float* d_bg_rgb;             // (R*Nb,3)
};

// backward of composite_bg_kernel with respect to sdf, rgb, beta, the bg density logits and the bg colours
__global__ __launch_bounds__(64) void composite_bg_bwd_kernel(CompositeBgBwdArgs a) {
  __shared__ double zs[kMaxS], fe[kMaxS], tr[kMaxS], dw[kMaxS], wt[kMaxS], bz[kMaxBg], bfe[kMaxBg], btr[kMaxBg],
      bdw[kMaxBg], bwt[kMaxBg];
  const int r = blockIdx.x, lane = threadIdx.x, S = a.S, Nb = a.Nb;
  const double beta = (double)(__builtin_fabsf(*a.beta_param) + a.beta_min);
  for (int i = lane; i < S; i += 64) zs[i] = (double)a.z[(size_t)r * S + i];
  for (int i = lane; i < Nb; i += 64) bz[i] = (double)a.z_bg[(size_t)r * Nb + i];
  __syncthreads();
  const double zmax = (double)a.z_max[r];
  auto fg_dist = [&](int i) { return (double)(float)((i < S - 1 ? zs[i + 1] : zmax) - zs[i]); };   // the forward's float32 distances
  auto bg_dist = [&](int i) { return i < Nb - 1 ? (double)(float)(bz[i] - bz[i + 1]) : 1e10; };
  for (int i = lane; i < S; i += 64) fe[i] = fg_dist(i) * DensityD((double)a.sdf[(size_t)r * S + i], beta).sigma;
  for (int i = lane; i < Nb; i += 64) {
    const double o = (double)a.bg_out0[(size_t)r * Nb + i];
    bfe[i] = bg_dist(i) * (o < 0.0 ? -o : o);
  }
  __syncthreads();
  const double ds = (double)a.depth_scale[r];
  double sw = 0.0, swz = 0.0;
  seq_weights(fe, tr, wt, S, S + 1, lane, [&](int i, double w) { sw += w; swz += w * (zs[i] * ds); });
  sw = wave_sum(sw); swz = wave_sum(swz);
  const double tbg = tr[S];                         // the transmittance in front of the background
  const double g0 = a.d_rgb_values[3 * r], g1 = a.d_rgb_values[3 * r + 1], g2 = a.d_rgb_values[3 * r + 2];
  // background: colour sums, and the sums of depth_values_all = swd / (swa + 1e-8) over [w_fg, tbg * bw] with
  // depths ds * [z, bg_depth]
  const double ga = a.d_depth_all ? (double)a.d_depth_all[r] : 0.0;
  double bdot = 0.0;       // sum_c g_c * sum_k bw_k cb_kc
  double swa = 0.0, swd = 0.0;
  seq_weights(bfe, btr, bwt, Nb, Nb, lane, [&](int i, double bw) {
    const size_t p = (size_t)r * Nb + i;
    const double cg = colour_grad(a.bg_rgb, p, tbg * bw, g0, g1, g2, a.d_bg_rgb);
    bdot += bw * cg;
    bdw[i] = tbg * cg;                 // d loss / d bw_i (colour term; the depth term follows once the sums are known)
    if (a.d_depth_all) { swa += tbg * bw; swd += (tbg * bw) * (ds * (double)a.bg_depth[p]); }
  });
  bdot = wave_sum(bdot);
  double dall = 1.0, qnum = 0.0;       // depth_values_all's denominator and numerator
  if (a.d_depth_all) {
    swa = wave_sum(swa); swd = wave_sum(swd);
    dall = (swa + sw) + 1e-8; qnum = swd + swz;
  }
  // d depth_all / d (a weight with depth dv) = (dv * dall - qnum) / dall^2; through tbg it also reaches every fg free energy
  if (a.d_depth_all) {
    double bdep = 0.0;      // sum_k bw_k q_k: d depth_all / d tbg
    for (int i = lane; i < Nb; i += 64) {
      const double q = ((ds * (double)a.bg_depth[(size_t)r * Nb + i]) * dall - qnum) / (dall * dall);
      bdw[i] += ga * tbg * q;
      bdep += bwt[i] * q;
    }
    bdot += ga * wave_sum(bdep);
  }
  const double gd = a.d_depth_values ? (double)a.d_depth_values[r] : 0.0;
  const double den = sw + 1e-8;
  for (int i = lane; i < S; i += 64) {
    const size_t p = (size_t)r * S + i;
    double d = colour_grad(a.rgb, p, wt[i], g0, g1, g2, a.d_rgb);
    if (a.d_weights) d += (double)a.d_weights[p];
    d += gd * ((zs[i] * ds) * den - swz) / (den * den);
    if (a.d_depth_all) d += ga * ((zs[i] * ds) * dall - qnum) / (dall * dall);
    dw[i] = d;
  }
  __syncthreads();
  double dbeta = 0.0;
  seq_weights_bwd(fe, tr, wt, dw, S, lane, [&](int i, double dfe_seq) {
    const size_t p = (size_t)r * S + i;
    // every free energy also attenuates the background term: d (tbg * B) / d fe_i = -tbg * B
    const double dfe = dfe_seq - tbg * bdot;
    const double dsig = dfe * fg_dist(i);
    const DensityD dn((double)a.sdf[p], beta);
    a.d_sdf[p] = (float)(dsig * dn.dsig_dsdf);
    dbeta += dsig * dn.dsig_dbeta;
  });
  seq_weights_bwd(bfe, btr, bwt, bdw, Nb, lane, [&](int i, double dfe) {
    const size_t p = (size_t)r * Nb + i;
    const float o = a.bg_out0[p];
    const double sg = o > 0.0f ? 1.0 : (o < 0.0f ? -1.0 : 0.0);
    // exp(-fe) underflows long before dist = 1e10 matters; guard the 0 * inf of the last sample
    a.d_bg_out0[p] = dfe != 0.0 ? (float)((dfe * bg_dist(i)) * sg) : 0.0f;
  });
  dbeta = wave_sum(dbeta);
  if (lane == 0) a.d_beta_ray[r] = (float)dbeta;
}

}  // namespace composite
}  // namespace svs

using namespace svs;
using namespace svs::composite;

static bool all_set(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) if (!p) return false;
  return true;
}

// The argument checks of the four entry points: the required pointers set and n_rays > 0, the sample counts within what the
// kernels' LDS arrays hold (n_bg < 0: a foreground-only entry point), and normals where a normal map is asked for.
static int check_args(const char* name, bool ptrs_ok, int n_rays, int n_samples, int max_samples, int n_bg = -1,
                      bool normals_ok = true) {
  if (!ptrs_ok || n_rays <= 0) { set_error("%s: null/invalid argument", name); return SVS_EINVAL; }
  if (n_bg < 0) {
    if (n_samples < 2 || n_samples > max_samples) { set_error("%s: n_samples must be in [2,%d]", name, max_samples); return SVS_ESHAPE; }
  } else if (n_samples < 2 || n_samples > max_samples || n_bg < 2 || n_bg > kMaxBg) {
    set_error("%s: sample counts out of range", name); return SVS_ESHAPE;
  }
  if (!normals_ok) { set_error("%s: normal_map needs normals", name); return SVS_EINVAL; }
  return SVS_OK;
}

extern "C" {

int svs_composite(int n_rays, int n_samples, const float* z, const float* sdf, const float* rgb, const float* normals,
                  const float* depth_scale, const float* beta_param, float beta_min, float* weights, float* rgb_values,
                  float* depth_values, float* depth_vals, float* normal_map, void* hip_stream) {
  const bool ptrs_ok = all_set({z, sdf, rgb, depth_scale, beta_param, weights, rgb_values, depth_values, depth_vals});
  if (int rc = check_args("svs_composite", ptrs_ok, n_rays, n_samples, kMaxS, -1, !normal_map || normals)) return rc;
  CompositeArgs a{n_rays, n_samples, z, sdf, rgb, normals, depth_scale, beta_param, beta_min, weights, rgb_values,
                  depth_values, depth_vals, normal_map};
  composite_kernel<<<n_rays, 64, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch("svs_composite");
}

int svs_composite_bwd(int n_rays, int n_samples, const float* z, const float* sdf, const float* rgb,
                      const float* depth_scale, const float* beta_param, float beta_min, const float* d_rgb_values,
                      const float* d_weights, const float* d_depth_values, float* d_sdf, float* d_rgb,
                      float* d_beta_ray, float* d_beta_param, void* hip_stream) {
  const bool ptrs_ok = all_set({z, sdf, rgb, depth_scale, beta_param, d_rgb_values, d_sdf, d_rgb, d_beta_ray, d_beta_param});
  if (int rc = check_args("svs_composite_bwd", ptrs_ok, n_rays, n_samples, kMaxS)) return rc;
  CompositeBwdArgs a{n_rays, n_samples, z, sdf, rgb, depth_scale, beta_param, beta_min, d_rgb_values, d_weights,
                     d_depth_values, d_sdf, d_rgb, d_beta_ray};
  hipStream_t s = (hipStream_t)hip_stream;
  composite_bwd_kernel<<<n_rays, 64, 0, s>>>(a);
  beta_reduce_kernel<<<1, 256, 0, s>>>(d_beta_ray, n_rays, beta_param, d_beta_param, 0);
  return check_launch("svs_composite_bwd");
}

// BG model: fg weights with the sphere exit as the last interval end, bg weights, composition (network_bg.py:76-125).
// The foreground holds n_samples + 1 prefixes, hence one sample fewer than the foreground-only kernels.
int svs_composite_bg(int n_rays, int n_samples, int n_bg, const float* z, const float* z_max, const float* sdf,
                     const float* rgb, const float* normals, const float* depth_scale, const float* beta_param,
                     float beta_min, const float* z_bg, const float* bg_out0, const float* bg_rgb, const float* bg_depth,
                     float* weights, float* bg_trans, float* bg_weights, float* rgb_values, float* depth_values,
                     float* depth_values_all, float* depth_vals, float* normal_map, void* hip_stream) {
  const bool ptrs_ok = all_set({z, z_max, sdf, rgb, depth_scale, beta_param, z_bg, bg_out0, bg_rgb, bg_depth, weights, bg_trans,
                                bg_weights, rgb_values, depth_values, depth_values_all, depth_vals});
  if (int rc = check_args("svs_composite_bg", ptrs_ok, n_rays, n_samples, kMaxS - 1, n_bg, !normal_map || normals)) return rc;
  CompositeBgArgs a{{n_rays, n_samples, z, sdf, rgb, normals, depth_scale, beta_param, beta_min, weights, rgb_values,
                     depth_values, depth_vals, normal_map},
                    n_bg, z_max, z_bg, bg_out0, bg_rgb, bg_depth, bg_trans, bg_weights, depth_values_all};
  composite_bg_kernel<<<n_rays, 64, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch("svs_composite_bg");
}

// backward of svs_composite_bg with respect to sdf, rgb, density.beta, the bg density logits and the bg colours
// (d_weights, d_depth_values may be NULL); d_beta_ray (n_rays) is workspace, *d_beta_param receives the sum.
int svs_composite_bg_bwd(int n_rays, int n_samples, int n_bg, const float* z, const float* z_max, const float* sdf,
                         const float* rgb, const float* depth_scale, const float* beta_param, float beta_min,
                         const float* z_bg, const float* bg_out0, const float* bg_rgb, const float* d_rgb_values,
                         const float* d_weights, const float* d_depth_values, const float* d_depth_all,
                         const float* bg_depth, float* d_sdf, float* d_rgb,
                         float* d_bg_out0, float* d_bg_rgb, float* d_beta_ray, float* d_beta_param, void* hip_stream) {
  const bool ptrs_ok = all_set({z, z_max, sdf, rgb, depth_scale, beta_param, z_bg, bg_out0, bg_rgb, d_rgb_values, d_sdf, d_rgb,
                                d_bg_out0, d_bg_rgb, d_beta_ray, d_beta_param}) && (!d_depth_all || bg_depth);
  if (int rc = check_args("svs_composite_bg_bwd", ptrs_ok, n_rays, n_samples, kMaxS - 1, n_bg)) return rc;
  CompositeBgBwdArgs a{{n_rays, n_samples, z, sdf, rgb, depth_scale, beta_param, beta_min, d_rgb_values, d_weights,
                        d_depth_values, d_sdf, d_rgb, d_beta_ray},
                       n_bg, z_max, z_bg, bg_out0, bg_rgb, d_depth_all, bg_depth, d_bg_out0, d_bg_rgb};
  hipStream_t s = (hipStream_t)hip_stream;
  composite_bg_bwd_kernel<<<n_rays, 64, 0, s>>>(a);
  beta_reduce_kernel<<<1, 256, 0, s>>>(d_beta_ray, n_rays, beta_param, d_beta_param, 0);
  return check_launch("svs_composite_bg_bwd");
}

}  // extern "C"
