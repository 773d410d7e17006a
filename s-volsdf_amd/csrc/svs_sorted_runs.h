// Sorted runs: the moves the geometry units share around a radix sort of integer keys (svs_meshsmooth.hip,
// svs_meshsimplify.hip, svs_poisson.hip, svs_cloud.hip).  Keys are sorted with hipcub's DeviceRadixSort, which is stable; a run
// is a stretch of equal keys in the sorted order.  Here: the scratch a sort needs, the sort calls, the heads of the runs (their
// scan is svs_scan.h), the first position of every key by binary search, and the positions of flagged elements.
// static / inline, like svs_scan.h: every unit that includes it gets its own copy.
#pragma once
#include <hipcub/hipcub.hpp>

#include "svs_workspace.h"

namespace svs {
namespace runs {

static inline int bit_length(unsigned v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// scratch for a sort of n keys (WithValues: with an unsigned value each) over any range of bits.  On a device hipcub's own
// answer decides, asked for all the bits of the key (fewer bits never need more).  The query needs a device; the floor -- a
// second buffer of the keys and values plus a margin -- does not, and lets the *_workspace_bytes entries answer without one.
template <typename Key, bool WithValues>
static size_t sort_scratch_bytes(size_t n) {
  size_t bytes = 0;
  const int m = (int)(n > 0 ? n : 1), bits = (int)(8 * sizeof(Key));
  hipError_t e;
  if constexpr (WithValues)                                 // (constexpr: a unit gets the kernels of the sorts it makes, no others)
    e = hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const Key*)nullptr, (Key*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr,
                                           m, 0, bits, (hipStream_t)0);
  else
    e = hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, (const Key*)nullptr, (Key*)nullptr, m, 0, bits, (hipStream_t)0);
  if (e != hipSuccess) { (void)hipGetLastError(); bytes = 0; }
  const size_t floor_bytes = (sizeof(Key) + sizeof(unsigned)) * (size_t)m + ((size_t)1 << 20);
  return bytes < floor_bytes ? floor_bytes : bytes;
}

// the bits [0, end_bit) of the keys decide; scratch_bytes is the caller's to keep (hipcub writes into its size argument)
template <typename Key>
static inline int sort_pairs(const char* name, void* scratch, size_t scratch_bytes, const Key* keys, Key* skeys, const unsigned* vals,
                             unsigned* svals, int n, int end_bit, hipStream_t s) {
  const hipError_t e = hipcub::DeviceRadixSort::SortPairs(scratch, scratch_bytes, keys, skeys, vals, svals, n, 0, end_bit, s);
  return e != hipSuccess ? ws::hip_fail(name, e) : SVS_OK;
}
template <typename Key>
static inline int sort_keys(const char* name, void* scratch, size_t scratch_bytes, const Key* keys, Key* skeys, int n, int end_bit,
                            hipStream_t s) {
  const hipError_t e = hipcub::DeviceRadixSort::SortKeys(scratch, scratch_bytes, keys, skeys, n, 0, end_bit, s);
  return e != hipSuccess ? ws::hip_fail(name, e) : SVS_OK;
}

// head[i] = 1 where a run starts; the run of the key `none` (what does not count, sorted behind the rest) has no head
template <typename Key>
static __global__ __launch_bounds__(256) void run_heads_kernel(const Key* __restrict__ skeys, int n, Key none, uint8_t* __restrict__ head) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Key k = skeys[i];
  head[i] = (k != none && (i == 0 || skeys[i - 1] != k)) ? 1 : 0;
}

// out[v] = the first sorted position whose key is >= v, v = 0 .. m: the run of key v is [out[v], out[v + 1])
template <typename Key>
static __global__ __launch_bounds__(256) void lower_bound_kernel(const Key* __restrict__ skeys, int n, int m, int* __restrict__ out) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v > m) return;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] < (Key)v) lo = mid + 1; else hi = mid;
  }
  out[v] = lo;
}

// seg_start[s] = the position of the flagged element with s flagged ones before it (offset: the scan of flag).  A template
// like its neighbours, so that only the units that launch it carry it; kBlock is the workgroup's size.
template <int kBlock>
static __global__ __launch_bounds__(kBlock) void seg_start_kernel(const uint8_t* __restrict__ flag, const int* __restrict__ offset, int n,
                                                                  int max_segs, int* __restrict__ seg_start) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const int s = offset[i];
  if (s < max_segs) seg_start[s] = i;
}

}  // namespace runs
}  // namespace svs
