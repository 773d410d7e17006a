// The save tail of the runner (runner.py:283-290) for gfx950: exact order statistics of a float32 map, which give the
// bounds of the colour previews (np.quantile / np.percentile), and helpers/utils.py::visualize_depth per pixel.
// Restated in numpy in tests/golden/make_run_fixture.py (the reference's own function) and tests/test_gpu_run.py.
//
// svs_select_sorted_pairs = the k-th and the min(k+1, n-1)-th smallest of n floats for up to 4 ranks k: the two values
//   numpy's `linear` quantile interpolates between.  Radix selection, most significant digit first, over the
//   order-preserving 32-bit key of a float (sign bit set: all bits flipped; clear: sign bit set), so that the keys order
//   as a TOTAL order of the values: -inf < negatives < -0.0 < +0.0 < positives < +inf < NaN (every NaN has the largest
//   key).  np.sort orders by `<` and so leaves the order of -0.0 and +0.0 to its algorithm; everywhere else the two agree
//   bit for bit.  Four passes of one 8-bit digit:
//     count   every workgroup histograms the digit of the elements of its span (16 per thread) that still match a
//             rank's prefix, with LDS atomics into 256 bins per DISTINCT prefix (ranks that share a prefix share the
//             bins; in the first pass all do), then adds its non-zero bins to the pass's global histogram with integer
//             atomics.  Integer sums do not depend on arrival order: the result is the same from run to run.
//     decide  one workgroup: per rank the first digit whose cumulative count exceeds the rank's remainder; prefix,
//             remainder and the sharing of prefixes for the next pass stay on the device.  No host round trip.
//   8 bits per pass: 2 KiB of bins per prefix, 16 KiB for 8 prefixes -- nine such workgroups fit a CU's 160 KiB, so LDS
//   never limits residency below the eight 256-thread workgroups the wave slots allow; 11-bit digits would save one of the
//   four reads of a map that L2 / MALL hold anyway (7 MB at 1152x1536) and cost 64 KiB.  A map of one value puts all 64
//   lanes of a wave on one bin (64 LDS cycles per wave-instruction instead of 2): 1.8 M elements over 256 CUs is still a
//   few microseconds, so there is no per-wave aggregation.  The first pass also counts NaN, +inf and -inf.
// svs_depth_preview = visualize_depth (helpers/utils.py:197-224) for up to 3 maps that share bounds: invalid = NaN or
//   infinite; clamp to [lo, hi], invalid -> hi; (d - lo) / (hi - lo), * 255, each rounded to float32 on its own (IEEE
//   division), truncated; direct: the grey code, else row 255 - code of a 256x3 uint8 table; invalid pixels 0.
//   hi <= lo (or a NaN bound): the reference divides by zero and casts NaN, which is platform-defined; here all zeros.
#include "svs_image.h"

namespace svs {
namespace preview {

constexpr int kThreads = 256;
constexpr int kItems = 16;
constexpr int kSpan = kThreads * kItems;                // elements per workgroup and sweep
constexpr int kMaxBlocks = 2048;                        // beyond: grid-stride sweeps
constexpr int kMaxRanks = 4;
constexpr int kSlots = 2 * kMaxRanks;                   // slot 2j: rank k_j, slot 2j + 1: min(k_j + 1, n - 1)
constexpr int kBins = 256;
constexpr int kPasses = 4;
constexpr int kMaxMaps = 3;

struct SelState {
  unsigned prefix[kSlots];                              // the digits decided so far, right-aligned
  unsigned krem[kSlots];                                // the slot's rank among the elements that share its prefix
  int leader[kSlots];                                   // the first slot with the same prefix: the one whose bins are filled
  unsigned counts[4];                                   // NaN, +inf, -inf, unused
};
struct Ranks { unsigned k[kSlots]; };

constexpr size_t kHistWords = (size_t)kPasses * kSlots * kBins;
constexpr size_t kWorkspaceBytes = kHistWords * sizeof(unsigned) + sizeof(SelState);

__device__ __forceinline__ unsigned key_of(unsigned u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;            // NaN of either sign: last
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned bits_of(unsigned key) {           // 0xffffffff -> 0x7fffffff, a quiet NaN
  return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
}

// grid: min(ceil(n / kSpan), kMaxBlocks)
__global__ __launch_bounds__(kThreads) void count_kernel(const float* __restrict__ x, size_t n, int pass, int nslots,
                                                        unsigned* __restrict__ hist, SelState* __restrict__ st) {
  __shared__ unsigned h[kSlots * kBins];
  __shared__ unsigned cls[3];
  __shared__ unsigned s_prefix[kSlots];
  __shared__ int s_active[kSlots];
  const int tid = threadIdx.x;
  for (int t = tid; t < kSlots * kBins; t += kThreads) h[t] = 0;
  if (tid < 3) cls[tid] = 0;
  if (tid < kSlots) {
    s_prefix[tid] = pass ? st->prefix[tid] : 0u;
    s_active[tid] = tid < nslots && (pass ? st->leader[tid] == tid : tid == 0);
  }
  __syncthreads();
  const int shift = 24 - 8 * pass;
  for (size_t base = (size_t)blockIdx.x * kSpan; base < n; base += (size_t)gridDim.x * kSpan) {
#pragma unroll 4
    for (int it = 0; it < kItems; ++it) {
      const size_t i = base + (size_t)it * kThreads + tid;
      if (i >= n) break;
      const unsigned u = __float_as_uint(x[i]);
      const unsigned key = key_of(u);
      if (pass == 0) {
        atomicAdd(&h[key >> 24], 1u);
        if (key == 0xffffffffu) atomicAdd(&cls[0], 1u);
        else if (u == 0x7f800000u) atomicAdd(&cls[1], 1u);
        else if (u == 0xff800000u) atomicAdd(&cls[2], 1u);
      } else {
        const unsigned hi = key >> (shift + 8), d = (key >> shift) & 255u;
        for (int j = 0; j < nslots; ++j)
          if (s_active[j] && hi == s_prefix[j]) atomicAdd(&h[j * kBins + d], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* g = hist + (size_t)pass * kSlots * kBins;
  for (int t = tid; t < nslots * kBins; t += kThreads)
    if (h[t]) atomicAdd(&g[t], h[t]);
  if (pass == 0 && tid < 3 && cls[tid]) atomicAdd(&st->counts[tid], cls[tid]);
}

// one workgroup
__global__ __launch_bounds__(kThreads) void decide_kernel(const unsigned* __restrict__ hist, SelState* __restrict__ st, int pass,
                                                         int nslots, Ranks ranks, float* __restrict__ values,
                                                         unsigned* __restrict__ counts) {
  __shared__ unsigned h[kSlots * kBins];
  __shared__ unsigned s_prefix[kSlots];
  const int tid = threadIdx.x;
  const unsigned* g = hist + (size_t)pass * kSlots * kBins;
  for (int t = tid; t < nslots * kBins; t += kThreads) h[t] = g[t];
  __syncthreads();
  unsigned krem = 0;
  if (tid < nslots) {
    const int lead = pass ? st->leader[tid] : 0;
    krem = pass ? st->krem[tid] : ranks.k[tid];
    const unsigned* hh = h + lead * kBins;
    unsigned cum = 0;
    int d = 0;
    for (; d < kBins - 1; ++d) {                        // (the last bin takes what is left: d stays inside the table)
      const unsigned c = hh[d];
      if (krem < cum + c) break;
      cum += c;
    }
    krem -= cum;
    s_prefix[tid] = ((pass ? st->prefix[tid] : 0u) << 8) | (unsigned)d;
  }
  __syncthreads();
  if (tid < nslots) {
    int lead = tid;
    for (int i = tid - 1; i >= 0; --i)
      if (s_prefix[i] == s_prefix[tid]) lead = i;
    st->prefix[tid] = s_prefix[tid];
    st->krem[tid] = krem;
    st->leader[tid] = lead;
    if (pass == kPasses - 1) values[tid] = __uint_as_float(bits_of(s_prefix[tid]));
  }
  if (pass == kPasses - 1 && tid < 3) counts[tid] = st->counts[tid];
}

struct PreviewMap { const float* src; uint8_t* dst; int n; };
struct PreviewArgs { PreviewMap m[kMaxMaps]; float lo, hi; int direct; const uint8_t* table; };

// grid: (ceil(max n / kThreads), maps)
__global__ __launch_bounds__(kThreads) void preview_kernel(PreviewArgs a) {
  const PreviewMap m = a.m[blockIdx.y];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m.n) return;
  float d = m.src[i];
  const bool invalid = !(fabsf(d) <= 3.402823466e+38f);               // NaN or infinite
  uint8_t c = 0;
  const bool degenerate = !(a.hi > a.lo);
  if (!degenerate) {
    if (d < a.lo) d = a.lo;
    if (d > a.hi) d = a.hi;
    if (invalid) d = a.hi;
    const float s = __fdiv_rn(__fsub_rn(d, a.lo), __fsub_rn(a.hi, a.lo));
    c = (uint8_t)(int)__fmul_rn(s, 255.0f);
  }
  const bool black = invalid || degenerate;
  if (a.direct) {
    m.dst[i] = black ? (uint8_t)0 : c;
  } else {
    const uint8_t* row = a.table + 3 * (255 - (int)c);
    uint8_t* o = m.dst + 3 * (size_t)i;
    o[0] = black ? (uint8_t)0 : row[0];
    o[1] = black ? (uint8_t)0 : row[1];
    o[2] = black ? (uint8_t)0 : row[2];
  }
}

}  // namespace preview
}  // namespace svs

using namespace svs;
using namespace svs::preview;

extern "C" {

size_t svs_select_workspace_bytes(void) { return kWorkspaceBytes; }

int svs_select_sorted_pairs(const float* x, long long n, const long long* ranks, int n_ranks, void* workspace, float* values,
                            unsigned int* counts, void* hip_stream) {
  const char* what = "svs_select_sorted_pairs";
  if (!x || !ranks || !workspace || !values || !counts) { set_error("%s: null argument", what); return SVS_EINVAL; }
  if (((uintptr_t)workspace & 7) != 0) { set_error("%s: workspace must be 8-byte aligned", what); return SVS_EINVAL; }
  if (n < 1 || n > 0x7fffffffLL) { set_error("%s: n must be in 1..2^31-1", what); return SVS_ESHAPE; }
  if (n_ranks < 1 || n_ranks > kMaxRanks) { set_error("%s: n_ranks must be in 1..%d", what, kMaxRanks); return SVS_EINVAL; }
  Ranks r{};
  for (int j = 0; j < n_ranks; ++j) {
    if (ranks[j] < 0 || ranks[j] >= n) { set_error("%s: rank %d is outside 0..n-1", what, j); return SVS_EINVAL; }
    r.k[2 * j] = (unsigned)ranks[j];
    r.k[2 * j + 1] = (unsigned)(ranks[j] + 1 < n ? ranks[j] + 1 : n - 1);
  }
  hipStream_t s = (hipStream_t)hip_stream;
  unsigned* hist = (unsigned*)workspace;
  SelState* st = (SelState*)(hist + kHistWords);
  const hipError_t e = hipMemsetAsync(workspace, 0, kWorkspaceBytes, s);
  if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return (int)e; }
  const int nslots = 2 * n_ranks;
  const long long spans = (n + kSpan - 1) / kSpan;
  const unsigned blocks = (unsigned)(spans < kMaxBlocks ? spans : kMaxBlocks);
  int rc;
  for (int pass = 0; pass < kPasses; ++pass) {
    count_kernel<<<blocks, kThreads, 0, s>>>(x, (size_t)n, pass, nslots, hist, st);
    if ((rc = check_launch("svs_select_sorted_pairs(count)"))) return rc;
    decide_kernel<<<1, kThreads, 0, s>>>(hist, st, pass, nslots, r, values, counts);
    if ((rc = check_launch("svs_select_sorted_pairs(decide)"))) return rc;
  }
  return SVS_OK;
}

int svs_depth_preview(const float* map0, int n0, uint8_t* out0, const float* map1, int n1, uint8_t* out1, const float* map2,
                      int n2, uint8_t* out2, int n_maps, float lo, float hi, int direct, const uint8_t* table,
                      void* hip_stream) {
  const char* what = "svs_depth_preview";
  if (n_maps < 1 || n_maps > kMaxMaps) { set_error("%s: n_maps must be in 1..%d", what, kMaxMaps); return SVS_EINVAL; }
  PreviewArgs a{{{map0, out0, n0}, {map1, out1, n1}, {map2, out2, n2}}, lo, hi, direct ? 1 : 0, table};
  if (!direct && !table) { set_error("%s: null colour table", what); return SVS_EINVAL; }
  int most = 0;
  for (int k = 0; k < n_maps; ++k) {
    if (!a.m[k].src || !a.m[k].dst) { set_error("%s: null argument", what); return SVS_EINVAL; }
    if (a.m[k].n < 1 || (long long)a.m[k].n > image::kMaxPixels) {
      set_error("%s: every map must hold 1..2^26 pixels", what); return SVS_ESHAPE;
    }
    most = a.m[k].n > most ? a.m[k].n : most;
  }
  preview_kernel<<<dim3((most + kThreads - 1) / kThreads, n_maps), kThreads, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch(what);
}

}  // extern "C"
