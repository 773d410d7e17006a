// The uniform grid over a point cloud that the cloud kernels search (csrc/svs_cloud.hip builds it; svs_cloud.hip and
// svs_cloudknn.hip read it): points sorted by the key of their cell (hipcub's DeviceRadixSort, called through
// svs_sorted_runs.h) plus an open-addressing hash from cell key to the [begin, end) run of the cell in the sorted order.
#pragma once
#include "svs_common.h"

namespace svs {
namespace cloud {

typedef unsigned long long u64;
constexpr u64 kEmpty = ~0ull;
constexpr int kCellBits = 21;                     // per-axis cell index range [0, 2^21)

struct Grid {
  double ox, oy, oz, inv_h, h;                    // cell = floor((p - origin) * inv_h)
  const double* pts;                              // (n,3) points in SORTED order
  const unsigned* perm;                           // sorted position -> original index
  const u64* hkey;                                // hash table (capacity = mask + 1)
  const uint2* hrun;                              //   [begin, end) of the cell's run
  unsigned mask;
  int n;
};

__device__ __forceinline__ int cell_coord(double p, double o, double inv_h) {
  const double c = __builtin_floor((p - o) * inv_h);
  return c < 0.0 ? 0 : (c > (double)((1 << kCellBits) - 1) ? (1 << kCellBits) - 1 : (int)c);
}
__device__ __forceinline__ u64 cell_key(int ix, int iy, int iz) {
  return (u64)ix | ((u64)iy << kCellBits) | ((u64)iz << (2 * kCellBits));
}
__device__ __forceinline__ unsigned hash_slot(u64 k, unsigned mask) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return (unsigned)k & mask;
}
__device__ __forceinline__ uint2 find_run(const Grid& g, int ix, int iy, int iz) {
  if ((unsigned)ix >= (1u << kCellBits) || (unsigned)iy >= (1u << kCellBits) || (unsigned)iz >= (1u << kCellBits)) return make_uint2(0, 0);
  const u64 k = cell_key(ix, iy, iz);
  unsigned s = hash_slot(k, g.mask);
  while (true) {
    const u64 hk = g.hkey[s];
    if (hk == k) return g.hrun[s];
    if (hk == kEmpty) return make_uint2(0, 0);
    s = (s + 1) & g.mask;
  }
}

// Builds the grid of `pts` (n rows, cell size h, origin: HOST double[3]) in `ws` (svs_cloud_grid_bytes(n) bytes) on stream
// s; *g: the device-side view.  -> 0 or the code of a failed launch, with the error string set.  (svs_cloud.hip)
int build_grid(const double* pts, int n, const double* origin, double h, void* ws, hipStream_t s, Grid* g);

}  // namespace cloud
}  // namespace svs
