// What one sorted sample sequence of a ray needs, shared by the sampler (svs_sampler.hip) and compositing
// (svs_composite.hip): one wave per ray, the sequence in LDS, lane-strided loops.  linspace_at and wave_cumsum are part of
// the bit-exact float32 contract and exist only here; every unit that includes this header is
// compiled with -ffp-contract=off.
#pragma once
#include "svs_common.h"

namespace svs {

// torch.linspace(start,end,n)[i] in float32 (ATen: step=(end-start)/(n-1); fma(step,i,start) for i<n/2,
// fma(-step, n-1-i, end) otherwise)
__device__ __forceinline__ float linspace_at(float start, float end, int n, int i) {
  const float step = (end - start) / (float)(n - 1);
  return i < n / 2 ? __builtin_fmaf(step, (float)i, start) : __builtin_fmaf(-step, (float)(n - 1 - i), end);
}

// Canonical inclusive cumsum of m floats held in LDS (in -> out, may alias), float64 accumulation.
// Returns the total (prefix m-1) rounded to float32, in every lane.  Caller syncs before and after.
__device__ __forceinline__ float wave_cumsum(const float* in, float* out, int m, int lane) {
  const int c = (m + 63) >> 6;
  const int lo = lane * c;
  const int hi = (lo + c < m) ? lo + c : m;
  double tot = 0.0;
  for (int j = lo; j < hi; ++j) tot = tot + (double)in[j];
  double scan = tot;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(scan, d);
    if (lane >= d) scan = scan + o;
  }
  double off = __shfl_up(scan, 1);
  if (lane == 0) off = 0.0;
  double acc = 0.0;
  float last = 0.0f;
  for (int j = lo; j < hi; ++j) {
    acc = acc + (double)in[j];
    last = (float)(off + acc);
    out[j] = last;
  }
  const int owner = (m - 1) / c;
  return __shfl(last, owner);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Opacity weights of a sequence, float32, bit for bit the reference's volume_rendering (network.py:281-295):
// fe[0..m) free energies in -> pre[i] = sum_{j<i} fe_j for i < n (n = m, or m + 1: pre[m] is then the total), then
// each(i, w_i) with w_i = (1 - exp(-fe_i)) * exp(-pre_i) for the lane's samples i < m, so that a kernel's reductions run in
// the loop that forms the weights.  The exclusive prefix is the canonical cumsum of the shifted sequence [0, fe_0, ...], as
// the reference forms it.  Caller syncs before.
template <typename Each>
__device__ __forceinline__ void seq_weights(const float* fe, float* pre, int m, int n, int lane, Each each) {
  for (int i = lane; i < n; i += 64) pre[i] = i == 0 ? 0.0f : fe[i - 1];
  __syncthreads();
  wave_cumsum(pre, pre, n, lane);
  __syncthreads();
  for (int i = lane; i < m; i += 64) each(i, (1.0f - sleef_expf(-fe[i])) * sleef_expf(-pre[i]));
}

// ---- float64 forms, for the compositing BACKWARD kernels.  The forward kernels follow the bit-exact float32 contract of
// the sampler; their reverse passes have no such contract (the reference gets these gradients from float32 autograd) and
// d loss / d beta is a sum with 1 / beta^3 factors and heavy cancellation: in float32 it was 4e-4 off float64 autograd at
// beta = 0.005.  Everything between the float32 inputs and the float32 outputs of the reverse passes is therefore double.
__device__ __forceinline__ double dexp(double x) { return x < -745.0 ? 0.0 : exp(x); }
// out[j] = sum_{i <= j} in[i] (in place allowed); returns the total
__device__ __forceinline__ double wave_cumsum_incl(const double* in, double* out, int m, int lane) {
  const int c = (m + 63) >> 6;
  const int lo = lane * c;
  const int hi = (lo + c < m) ? lo + c : m;
  double tot = 0.0;
  for (int j = lo; j < hi; ++j) tot += in[j];
  double scan = tot;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(scan, d);
    if (lane >= d) scan += o;
  }
  double acc = scan - tot;
  for (int j = lo; j < hi; ++j) { acc += in[j]; out[j] = acc; }
  return __shfl(acc, (m - 1) / c);
}
// out[j] = sum_{i > j} in[i] (in place allowed), summed from the top down.  Not total - prefix: that difference carries
// eps times the whole ray's sum, which swamps a suffix behind an opaque surface at beta_min (test_composite_backward_edges
// [1e-12-2] and test_composite_bg_backward_edges[0.0-2]: d_sdf 5.6x and 2.1x its largest value off).  The last element's
// suffix is exactly 0 (its interval is 1e10).
__device__ __forceinline__ void wave_suffix_excl(const double* in, double* out, int m, int lane) {
  const int c = (m + 63) >> 6;
  const int lo = lane * c;
  const int hi = (lo + c < m) ? lo + c : m;
  double tot = 0.0;
  for (int j = hi - 1; j >= lo; --j) tot += in[j];
  double scan = tot;                    // -> sum of the chunks of lanes >= lane
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_down(scan, d);
    if (lane + d < 64) scan += o;
  }
  double acc = __shfl_down(scan, 1);    // the chunks of lanes > lane
  if (lane == 63) acc = 0.0;
  for (int j = hi - 1; j >= lo; --j) { const double v = in[j]; out[j] = acc; acc += v; }
}
// Laplace density and its derivatives in double (density.py:21-30)
struct DensityD {
  double sigma, dsig_dsdf, dsig_dbeta;
  __device__ __forceinline__ DensityD(double s, double beta) {
    const double as = s < 0.0 ? -s : s;
    const double e = dexp(-as / beta);
    const double sgn = s > 0.0 ? 1.0 : (s < 0.0 ? -1.0 : 0.0);
    // 0.5 + 0.5 * sgn * (e - 1) without its cancellation: formed as written, sigma for sdf / beta > 20 kept only
    // 1e-16 / e of its relative accuracy, which the last interval (1e10) carries into d_sdf and d beta
    // (test_composite_backward_edges[0.02-2/63/64/98/256]: d_sdf up to 130x its largest value off, d beta 4x its bound)
    sigma = (1.0 / beta) * (s > 0.0 ? 0.5 * e : 1.0 - 0.5 * e);
    // sign(0) = 0 in the reference's density: its gradient w.r.t. sdf vanishes there as well
    dsig_dsdf = s != 0.0 ? -0.5 * e / (beta * beta) : 0.0;
    dsig_dbeta = -sigma / beta + 0.5 * sgn * e * as / (beta * beta * beta);
  }
};

// fe[0..m) free energies in -> tr[i] = T_i = exp(-sum_{j<i} fe_j) for i < n (n = m, or m + 1: tr[m] is then the
// transmittance behind the sequence), w[i] = (1 - exp(-fe_i)) * T_i for i < m, and each(i, w_i) in the same loop.  The
// exclusive prefix is the inclusive scan of the shifted sequence: a last free energy over the 1e10 interval must not enter
// any partial sum, it would cost the prefixes of its lane's chunk 1e-5 of absolute accuracy.  Caller syncs before; synced
// on return.
template <typename Each>
__device__ __forceinline__ void seq_weights(const double* fe, double* tr, double* w, int m, int n, int lane, Each each) {
  for (int i = lane; i < n; i += 64) tr[i] = i == 0 ? 0.0 : fe[i - 1];
  __syncthreads();
  wave_cumsum_incl(tr, tr, n, lane);
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const double T = dexp(-tr[i]);
    tr[i] = T;
    if (i < m) { const double wi = (1.0 - dexp(-fe[i])) * T; w[i] = wi; each(i, wi); }
  }
  __syncthreads();
}

// The reverse pass of seq_weights: dw[i] = d loss / d w_i in -> each(k, d loss / d fe_k) for the lane's samples,
//   dL/dfe_k = dw_k * T_k * exp(-fe_k) - sum_{i>k} dw_i * w_i.
// w is used up: it holds the suffix sums on return.  Caller syncs before.
template <typename Each>
__device__ __forceinline__ void seq_weights_bwd(const double* fe, const double* tr, double* w, const double* dw, int m,
                                                int lane, Each each) {
  for (int i = lane; i < m; i += 64) w[i] = dw[i] * w[i];
  __syncthreads();
  wave_suffix_excl(w, w, m, lane);
  __syncthreads();
  for (int i = lane; i < m; i += 64) each(i, dw[i] * tr[i] * dexp(-fe[i]) - w[i]);
}

}  // namespace svs
