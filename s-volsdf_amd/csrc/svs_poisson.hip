// A surface from an oriented point cloud on gfx950 (svs_hip/poisson.py): Poisson reconstruction on one dense grid, after
// Kazhdan, Bolitho and Hoppe, "Poisson surface reconstruction" (2006), without octree; screening (Kazhdan and Hoppe 2013, the
// point term lumped into the diagonal weight * W) is opt-in through the svs_screened_* entries.  The rule is stated in
// include/svolsdf_hip.h and restated in float64 numpy by tests/poisson_oracle.py and tests/poisson_screen_oracle.py.
//
// Splat: the counted points are sorted by the index of their cell (a stable radix sort of the bits the cell count needs),
// the eight corner sums of a cell are formed in one fixed order -- segments of 64 consecutive points, one lane per segment,
// then one lane per cell over its segment sums -- and every node gathers from the at most eight cells around it: no float
// atomic, the same bytes in every run.
//
// Solve: conjugate gradients on float32 vectors with float64 arithmetic per element and float64 dot products.  An iteration
// is five launches and moves 44 bytes per node: the 7-point stencil fused with p.q (read p, write q), a one-workgroup pass
// over the partial sums that leaves alpha in device memory, the two axpys fused with r.r (read x p r q, write x r), the pass
// that leaves beta, and the direction update (read r p, write p).  The host never waits inside an iteration; every
// check_every iterations it downloads the 8 bytes of r.r.  The screened solve is the same five launches with the diagonal
// d = 6 / h^2 + weight * W as preconditioner: each of the three passes over the volume reads W once more (56 bytes per node),
// the axpy pass leaves r.r and r.(r / d) together, and r / d is never stored.
//
// The stencil kernel: a workgroup owns kTileJ x kTileK nodes of a plane and marches over kTileI planes.  A lane holds four
// consecutive nodes of the contiguous axis in registers for the planes i-1, i, i+1 and i+2 (the last one a prefetch); the
// current plane goes through LDS with one halo row and column on every side, so that a node is fetched once per tile plus
// the halo (1.16 in the plane, 1.125 along the march).  16-byte accesses when n2 % 4 == 0 and the bases are aligned,
// scalar ones otherwise; both walk the nodes in the same order, so both give the same sums.
// All float64 arithmetic is compiled with -ffp-contract=off.
#include "svs_common.h"
#include "svs_scan.h"
#include "svs_sorted_runs.h"

namespace svs {
namespace poisson {

constexpr int kSegment = 64;                                // points per segment of a cell's run
constexpr int kTileI = 16, kTileJ = 16, kTileK = 64;        // the stencil workgroup's extent along axes 0, 1, 2
constexpr int kThreads = 256;
constexpr int kGroup = 4;                                   // nodes per lane along the contiguous axis
constexpr int kFlatBlocks = 2048;                           // workgroups of the flat (axpy) kernels: they stride over the volume
constexpr int kLdsStride = kTileK + 8;                      // interior at column 4 (16-byte aligned), halos at 3 and 4 + kTileK
enum { kRR = 0, kBB = 1, kAlpha = 2, kBeta = 3, kRN = 4, kScalars = 8 };

struct Grid { double ox, oy, oz, h; long long n0, n1, n2; };

// the cell of a point and its position in it; false when the point does not count
__device__ __forceinline__ bool locate(const Grid& g, double px, double py, double pz, long long (&b)[3], double (&t)[3]) {
  if (!finite_f64(px) || !finite_f64(py) || !finite_f64(pz)) return false;
  const double q[3] = {(px - g.ox) / g.h, (py - g.oy) / g.h, (pz - g.oz) / g.h};
  const long long n[3] = {g.n0, g.n1, g.n2};
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double f = __builtin_floor(q[a]);
    ok = ok && finite_f64(f) && f >= 0.0 && f <= (double)(n[a] - 2);
    b[a] = ok ? (long long)f : 0;
    t[a] = q[a] - f;
  }
  return ok;
}

// weight of corner c = 4 di + 2 dj + dk: (wx * wy) * wz
__device__ __forceinline__ double corner_weight(const double (&t)[3], int c) {
  const double wx = (c & 4) ? t[0] : 1.0 - t[0], wy = (c & 2) ? t[1] : 1.0 - t[1], wz = (c & 1) ? t[2] : 1.0 - t[2];
  return wx * wy * wz;
}

// tree sum over the 256 threads of the workgroup, one fixed order; the result in every thread
__device__ __forceinline__ double block_sum(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int d = kThreads / 2; d > 0; d >>= 1) {
    if (t < d) s[t] += s[t + d];
    __syncthreads();
  }
  return s[0];
}

// ---- splat ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void point_keys_kernel(const double* __restrict__ pts, const float* __restrict__ normals, int n, Grid g,
                                                         unsigned n_cells, unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                         int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (i == 0) counts[0] = n;                                 // the head of the skipped run lowers it (run_heads_kernel)
  long long b[3];
  double t[3];
  bool ok = locate(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], b, t);
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && finite_f64((double)normals[3 * (size_t)i + a]);
  keys[i] = ok ? (unsigned)((b[0] * (g.n1 - 1) + b[1]) * (g.n2 - 1) + b[2]) : n_cells;
  vals[i] = (unsigned)i;
}

// a run = the points of one cell, or the skipped points (key n_cells, sorted behind every cell)
__global__ __launch_bounds__(256) void run_heads_kernel(const unsigned* __restrict__ skeys, int n, unsigned n_cells, uint8_t* __restrict__ head,
                                                        int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned k = skeys[i];
  const bool h = i == 0 || skeys[i - 1] != k;
  head[i] = h ? 1 : 0;
  if (h && k >= n_cells) counts[0] = i;
}

// run_first[r] = the first sorted position of run r, run_first[runs] = n
__global__ __launch_bounds__(256) void run_first_kernel(const uint8_t* __restrict__ head, const int* __restrict__ hoff, int n,
                                                        int* __restrict__ run_first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (head[i]) run_first[hoff[i]] = i;
  if (i == n - 1) run_first[hoff[i] + (int)head[i]] = n;
}

__global__ __launch_bounds__(256) void seg_flags_kernel(const unsigned* __restrict__ skeys, int n, unsigned n_cells, const uint8_t* __restrict__ head,
                                                        const int* __restrict__ hoff, const int* __restrict__ run_first,
                                                        uint8_t* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int r = hoff[i] + (int)head[i] - 1;
  flag[i] = (skeys[i] < n_cells && ((i - run_first[r]) & (kSegment - 1)) == 0) ? 1 : 0;
}

struct Partial { double s[8][4]; };                         // corner c: Vx, Vy, Vz, W; 256 bytes

// one lane per segment: its points left to right from zero
__global__ __launch_bounds__(256) void seg_sum_kernel(const double* __restrict__ pts, const float* __restrict__ normals, Grid g,
                                                      const unsigned* __restrict__ svals, const uint8_t* __restrict__ head,
                                                      const int* __restrict__ hoff, const int* __restrict__ run_first,
                                                      const int* __restrict__ seg_start, const int* __restrict__ n_segs, int max_segs,
                                                      Partial* __restrict__ part) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= max_segs || s >= *n_segs) return;
  const int i0 = seg_start[s];
  const int run_end = run_first[hoff[i0] + (int)head[i0]];
  const int i1 = i0 + kSegment < run_end ? i0 + kSegment : run_end;
  Partial q;
#pragma unroll
  for (int c = 0; c < 8; ++c) q.s[c][0] = q.s[c][1] = q.s[c][2] = q.s[c][3] = 0.0;
  for (int i = i0; i < i1; ++i) {
    const size_t p = svals[i];
    long long b[3];
    double t[3];
    if (!locate(g, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], b, t)) continue;   // (never: the point counted when it got its key)
    const double nx = (double)normals[3 * p], ny = (double)normals[3 * p + 1], nz = (double)normals[3 * p + 2];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double w = corner_weight(t, c);
      q.s[c][0] += w * nx; q.s[c][1] += w * ny; q.s[c][2] += w * nz; q.s[c][3] += w;
    }
  }
  part[s] = q;
}

// one lane per run: its segment sums left to right from zero, left in the run's first segment; cell_seg[cell] = that segment
__global__ __launch_bounds__(256) void cell_sum_kernel(const unsigned* __restrict__ skeys, unsigned n_cells, const int* __restrict__ run_first,
                                                       const int* __restrict__ soff, const int* __restrict__ n_runs, int max_runs,
                                                       int max_segs, Partial* __restrict__ part, int* __restrict__ cell_seg) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= max_runs || r >= *n_runs) return;
  const int b0 = run_first[r];
  const unsigned key = skeys[b0];
  if (key >= n_cells) return;                                // the skipped run
  const int count = run_first[r + 1] - b0;
  const int s0 = soff[b0], n_seg = (count + kSegment - 1) / kSegment;
  if (s0 >= max_segs) return;                                // (never: max_segs bounds the segments of any input)
  Partial q;
#pragma unroll
  for (int c = 0; c < 8; ++c) q.s[c][0] = q.s[c][1] = q.s[c][2] = q.s[c][3] = 0.0;
  for (int s = s0; s < s0 + n_seg && s < max_segs; ++s) {
    const Partial& w = part[s];
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) q.s[c][k] += w.s[c][k];
  }
  part[s0] = q;
  cell_seg[key] = s0;
}

// one lane per node: the corner sums of the at most eight cells around it, in ascending corner order from zero
__global__ __launch_bounds__(256) void node_gather_kernel(Grid g, const int* __restrict__ cell_seg, const Partial* __restrict__ part,
                                                          float* __restrict__ field) {
  const long long total = g.n0 * g.n1 * g.n2;
  const long long node = (long long)blockIdx.x * 256 + threadIdx.x;
  if (node >= total) return;
  const long long row = node / g.n2, k = node - row * g.n2, i = row / g.n1, j = row - i * g.n1;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const long long ci = i - (c >> 2), cj = j - ((c >> 1) & 1), ck = k - (c & 1);
    if (ci < 0 || cj < 0 || ck < 0 || ci > g.n0 - 2 || cj > g.n1 - 2 || ck > g.n2 - 2) continue;
    const int s = cell_seg[(ci * (g.n1 - 1) + cj) * (g.n2 - 1) + ck];
    if (s < 0) continue;
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] += part[s].s[c][p];
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) field[(size_t)p * (size_t)total + (size_t)node] = (float)acc[p];
}

// ---- divergence ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void divergence_kernel(const float* __restrict__ field, long long n0, long long n1, long long n2, double h,
                                                         float* __restrict__ rhs) {
  const long long total = n0 * n1 * n2;
  const long long node = (long long)blockIdx.x * 256 + threadIdx.x;
  if (node >= total) return;
  const long long row = node / n2, k = node - row * n2, i = row / n1, j = row - i * n1;
  const float* vx = field; const float* vy = field + total; const float* vz = field + 2 * total;
  const double xp = i + 1 < n0 ? (double)vx[node + n1 * n2] : 0.0, xm = i > 0 ? (double)vx[node - n1 * n2] : 0.0;
  const double yp = j + 1 < n1 ? (double)vy[node + n2] : 0.0, ym = j > 0 ? (double)vy[node - n2] : 0.0;
  const double zp = k + 1 < n2 ? (double)vz[node + 1] : 0.0, zm = k > 0 ? (double)vz[node - 1] : 0.0;
  rhs[node] = (float)(-(((xp - xm) + (yp - ym)) + (zp - zm)) / (2.0 * h));
}

// ---- the operator and conjugate gradients --------------------------------------------------------------------------------
struct Vol { long long n0, n1, n2; };

// four consecutive nodes of row (i,j) from k; 0 beyond the grid
template <bool kVec>
__device__ __forceinline__ f32x4 load_row4(const float* __restrict__ p, const Vol& v, long long i, long long j, long long k) {
  f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
  if (i < 0 || i >= v.n0 || j < 0 || j >= v.n1 || k >= v.n2) return o;
  const float* at = p + (i * v.n1 + j) * v.n2 + k;
  if (kVec) return *reinterpret_cast<const f32x4*>(at);     // n2 % 4 == 0: a group is inside or outside as a whole
  o.x = at[0];
  if (k + 1 < v.n2) o.y = at[1];
  if (k + 2 < v.n2) o.z = at[2];
  if (k + 3 < v.n2) o.w = at[3];
  return o;
}

__device__ __forceinline__ float load_node(const float* __restrict__ p, const Vol& v, long long i, long long j, long long k) {
  if (i < 0 || i >= v.n0 || j < 0 || j >= v.n1 || k < 0 || k >= v.n2) return 0.0f;
  return p[(i * v.n1 + j) * v.n2 + k];
}

// q = A p with A p = (6 p - ((((((i-1) + (i+1)) + (j-1)) + (j+1)) + (k-1)) + (k+1))) / h^2, 0 beyond the grid; partial[workgroup] =
// the workgroup's share of p.q (products of the stored float32 values, in float64).  kScreen: q = A p + (weight * W) * p, the
// lane's own four W values of a plane fetched one plane ahead like the halo (the other instantiations never touch W or weight)
template <bool kVec, bool kScreen>
__global__ __launch_bounds__(kThreads) void stencil_kernel(const float* __restrict__ p, float* __restrict__ q, Vol v, double h2,
                                                           double* __restrict__ partial, const float* __restrict__ W, double weight) {
  __shared__ __attribute__((aligned(16))) float plane[kTileJ + 2][kLdsStride];
  __shared__ double red[kThreads];
  const int tid = threadIdx.x, tj = tid / (kTileK / kGroup), tk = (tid % (kTileK / kGroup)) * kGroup;
  const long long k0 = (long long)blockIdx.x * kTileK, j0 = (long long)blockIdx.y * kTileJ, i0 = (long long)blockIdx.z * kTileI;
  const long long i1 = i0 + kTileI < v.n0 ? i0 + kTileI : v.n0;
  const long long j = j0 + tj, k = k0 + tk;
  // halo lanes: the first 32 threads load the rows j0 - 1 and j0 + kTileJ, the next 32 the columns k0 - 1 and k0 + kTileK
  const bool halo_row = tid < 2 * (kTileK / kGroup), halo_col = tid >= 64 && tid < 64 + 2 * kTileJ;
  const int hr = tid / (kTileK / kGroup);                    // 0: below, 1: above
  const long long hrow_j = hr == 0 ? j0 - 1 : j0 + kTileJ;
  const int hc_side = (tid - 64) / kTileJ, hc_row = (tid - 64) % kTileJ;
  const long long hcol_k = hc_side == 0 ? k0 - 1 : k0 + kTileK;

  f32x4 prev = load_row4<kVec>(p, v, i0 - 1, j, k), cur = load_row4<kVec>(p, v, i0, j, k), next = load_row4<kVec>(p, v, i0 + 1, j, k);
  f32x4 hrow = {0.0f, 0.0f, 0.0f, 0.0f};
  float hcol = 0.0f;
  if (halo_row) hrow = load_row4<kVec>(p, v, i0, hrow_j, k);
  if (halo_col) hcol = load_node(p, v, i0, j0 + hc_row, hcol_k);
  f32x4 wcur = {0.0f, 0.0f, 0.0f, 0.0f};
  if (kScreen) wcur = load_row4<kVec>(W, v, i0, j, k);
  double acc = 0.0;
  for (long long i = i0; i < i1; ++i) {
    const f32x4 next2 = load_row4<kVec>(p, v, i + 2 < i1 + 1 ? i + 2 : v.n0, j, k);       // prefetch; nothing past plane i1
    f32x4 hrow_next = {0.0f, 0.0f, 0.0f, 0.0f};
    float hcol_next = 0.0f;
    f32x4 wnext = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i + 1 < i1) {
      if (halo_row) hrow_next = load_row4<kVec>(p, v, i + 1, hrow_j, k);
      if (halo_col) hcol_next = load_node(p, v, i + 1, j0 + hc_row, hcol_k);
      if (kScreen) wnext = load_row4<kVec>(W, v, i + 1, j, k);
    }
    __syncthreads();                                         // the reads of the previous plane are done
    *reinterpret_cast<f32x4*>(&plane[tj + 1][4 + tk]) = cur;
    if (halo_row) *reinterpret_cast<f32x4*>(&plane[hr == 0 ? 0 : kTileJ + 1][4 + tk]) = hrow;
    if (halo_col) plane[hc_row + 1][hc_side == 0 ? 3 : 4 + kTileK] = hcol;
    __syncthreads();
    const f32x4 below = *reinterpret_cast<const f32x4*>(&plane[tj][4 + tk]);
    const f32x4 above = *reinterpret_cast<const f32x4*>(&plane[tj + 2][4 + tk]);
    const float left = plane[tj + 1][3 + tk], right = plane[tj + 1][8 + tk];
    if (j < v.n1 && k < v.n2) {
      const float c[6] = {left, cur.x, cur.y, cur.z, cur.w, right};
      const float pm[4] = {prev.x, prev.y, prev.z, prev.w}, pp[4] = {next.x, next.y, next.z, next.w};
      const float bm[4] = {below.x, below.y, below.z, below.w}, bp[4] = {above.x, above.y, above.z, above.w};
      const float wv[4] = {wcur.x, wcur.y, wcur.z, wcur.w};
      float out[4];
#pragma unroll
      for (int e = 0; e < kGroup; ++e) {
        // beyond the row's end the right neighbour is 0 (the loads gave 0 there)
        const double sum = (((((double)pm[e] + (double)pp[e]) + (double)bm[e]) + (double)bp[e]) + (double)c[e]) + (double)c[e + 2];
        if (kScreen) out[e] = (float)((6.0 * (double)c[e + 1] - sum) / h2 + (weight * (double)wv[e]) * (double)c[e + 1]);
        else out[e] = (float)((6.0 * (double)c[e + 1] - sum) / h2);
        if (k + e < v.n2) acc += (double)c[e + 1] * (double)out[e];
      }
      float* at = q + (i * v.n1 + j) * v.n2 + k;
      if (kVec) {
        f32x4 o; o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
        *reinterpret_cast<f32x4*>(at) = o;
      } else {
#pragma unroll
        for (int e = 0; e < kGroup; ++e)
          if (k + e < v.n2) at[e] = out[e];
      }
    }
    prev = cur; cur = next; next = next2; hrow = hrow_next; hcol = hcol_next; wcur = wnext;
  }
  const double total = block_sum(acc, red);
  if (partial && tid == 0) partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

// the flat kernels: group g = four consecutive elements, thread t of workgroup b takes g = b * 256 + t, then strides
__device__ __forceinline__ void load4(const float* __restrict__ p, long long at, long long total, bool vec, float (&o)[4]) {
  if (vec && at + kGroup <= total) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + at);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < kGroup; ++e) o[e] = at + e < total ? p[at + e] : 0.0f;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ p, long long at, long long total, bool vec, const float (&o)[4]) {
  if (vec && at + kGroup <= total) {
    f32x4 v; v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
    *reinterpret_cast<f32x4*>(p + at) = v;
  } else {
#pragma unroll
    for (int e = 0; e < kGroup; ++e)
      if (at + e < total) p[at + e] = o[e];
  }
}

// x = 0, r = p = rhs, partial = r.r
__global__ __launch_bounds__(kThreads) void cg_init_kernel(const float* __restrict__ rhs, long long total, int vec_rhs, int vec_x,
                                                           float* __restrict__ x, float* __restrict__ r, float* __restrict__ p,
                                                           double* __restrict__ partial) {
  __shared__ double red[kThreads];
  const long long groups = (total + kGroup - 1) / kGroup;
  const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  double acc = 0.0;
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kThreads) {
    float b[4];
    load4(rhs, g * kGroup, total, vec_rhs, b);
    store4(x, g * kGroup, total, vec_x, zero);
    store4(r, g * kGroup, total, true, b);
    store4(p, g * kGroup, total, true, b);
#pragma unroll
    for (int e = 0; e < kGroup; ++e) acc += (double)b[e] * (double)b[e];
  }
  const double sum = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// x += alpha p, r -= alpha q, partial = r.r of the stored r
__global__ __launch_bounds__(kThreads) void cg_axpy_kernel(long long total, int vec_x, const double* __restrict__ scal, float* __restrict__ x,
                                                           float* __restrict__ r, const float* __restrict__ p, const float* __restrict__ q,
                                                           double* __restrict__ partial) {
  __shared__ double red[kThreads];
  const long long groups = (total + kGroup - 1) / kGroup;
  const double alpha = scal[kAlpha];
  double acc = 0.0;
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kThreads) {
    float xv[4], rv[4], pv[4], qv[4];
    load4(x, g * kGroup, total, vec_x, xv);
    load4(r, g * kGroup, total, true, rv);
    load4(p, g * kGroup, total, true, pv);
    load4(q, g * kGroup, total, true, qv);
#pragma unroll
    for (int e = 0; e < kGroup; ++e) {
      xv[e] = (float)((double)xv[e] + alpha * (double)pv[e]);
      rv[e] = (float)((double)rv[e] - alpha * (double)qv[e]);
      acc += (double)rv[e] * (double)rv[e];                  // (elements past the end are 0)
    }
    store4(x, g * kGroup, total, vec_x, xv);
    store4(r, g * kGroup, total, true, rv);
  }
  const double sum = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// p = r + beta p
__global__ __launch_bounds__(kThreads) void cg_direction_kernel(long long total, const double* __restrict__ scal, const float* __restrict__ r,
                                                                float* __restrict__ p) {
  const long long groups = (total + kGroup - 1) / kGroup;
  const double beta = scal[kBeta];
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kThreads) {
    float rv[4], pv[4];
    load4(r, g * kGroup, total, true, rv);
    load4(p, g * kGroup, total, true, pv);
#pragma unroll
    for (int e = 0; e < kGroup; ++e) pv[e] = (float)((double)rv[e] + beta * (double)pv[e]);
    store4(p, g * kGroup, total, true, pv);
  }
}

// one workgroup: thread t sums the partials t, t + 256, ... from zero, then the tree; thread 0 updates the scalars
enum { kModeInit = 0, kModePQ = 1, kModeRR = 2 };
__global__ __launch_bounds__(kThreads) void cg_scalars_kernel(const double* __restrict__ partial, int n_partials, int mode, double* __restrict__ scal) {
  __shared__ double red[kThreads];
  double acc = 0.0;
  for (int b = threadIdx.x; b < n_partials; b += kThreads) acc += partial[b];
  const double sum = block_sum(acc, red);
  if (threadIdx.x != 0) return;
  if (mode == kModeInit) {
    scal[kRR] = sum; scal[kBB] = sum; scal[kRN] = sum; scal[kAlpha] = 0.0; scal[kBeta] = 0.0;
  } else if (mode == kModePQ) {
    scal[kAlpha] = sum > 0.0 ? scal[kRR] / sum : 0.0;        // p = 0 (r = 0 exactly): nothing moves any more
  } else {
    const double rr = scal[kRR];
    scal[kBeta] = rr > 0.0 ? sum / rr : 0.0;
    scal[kRR] = sum; scal[kRN] = sum;
  }
}

// ---- the screened system: A + diag(weight W), Jacobi-preconditioned conjugate gradients ------------------------------------
// d = 6 / h^2 + weight * W is the operator's diagonal; z = r / d is formed in float64 where it is needed and never stored.
enum { kRZ = 5 };                                           // r.z beside kRR .. kRN (svs_poisson_cg leaves the slot alone)

__device__ __forceinline__ double screened_diagonal(double six_h2, double weight, float w) { return six_h2 + weight * (double)w; }

// x = 0, r = rhs, p = r / d, partial = r.r, partial_z = r.(r / d)
__global__ __launch_bounds__(kThreads) void pcg_init_kernel(const float* __restrict__ rhs, const float* __restrict__ W, long long total,
                                                            int vec_rhs, int vec_w, int vec_x, double six_h2, double weight,
                                                            float* __restrict__ x, float* __restrict__ r, float* __restrict__ p,
                                                            double* __restrict__ partial, double* __restrict__ partial_z) {
  __shared__ double red[kThreads];
  const long long groups = (total + kGroup - 1) / kGroup;
  const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  double acc = 0.0, acc_z = 0.0;
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kThreads) {
    float b[4], wv[4], pv[4];
    load4(rhs, g * kGroup, total, vec_rhs, b);
    load4(W, g * kGroup, total, vec_w, wv);
#pragma unroll
    for (int e = 0; e < kGroup; ++e) {
      const double z = (double)b[e] / screened_diagonal(six_h2, weight, wv[e]);
      pv[e] = (float)z;
      acc += (double)b[e] * (double)b[e];                    // (elements past the end are 0, and their d is 6 / h^2 > 0)
      acc_z += (double)b[e] * z;
    }
    store4(x, g * kGroup, total, vec_x, zero);
    store4(r, g * kGroup, total, true, b);
    store4(p, g * kGroup, total, true, pv);
  }
  const double sum = block_sum(acc, red);
  const double sum_z = block_sum(acc_z, red);
  if (threadIdx.x == 0) { partial[blockIdx.x] = sum; partial_z[blockIdx.x] = sum_z; }
}

// x += alpha p, r -= alpha q, partial = r.r and partial_z = r.(r / d) of the stored r, both in the one pass
__global__ __launch_bounds__(kThreads) void pcg_axpy_kernel(long long total, int vec_x, int vec_w, double six_h2, double weight,
                                                            const double* __restrict__ scal, const float* __restrict__ W,
                                                            float* __restrict__ x, float* __restrict__ r, const float* __restrict__ p,
                                                            const float* __restrict__ q, double* __restrict__ partial,
                                                            double* __restrict__ partial_z) {
  __shared__ double red[kThreads];
  const long long groups = (total + kGroup - 1) / kGroup;
  const double alpha = scal[kAlpha];
  double acc = 0.0, acc_z = 0.0;
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kThreads) {
    float xv[4], rv[4], pv[4], qv[4], wv[4];
    load4(x, g * kGroup, total, vec_x, xv);
    load4(r, g * kGroup, total, true, rv);
    load4(p, g * kGroup, total, true, pv);
    load4(q, g * kGroup, total, true, qv);
    load4(W, g * kGroup, total, vec_w, wv);
#pragma unroll
    for (int e = 0; e < kGroup; ++e) {
      xv[e] = (float)((double)xv[e] + alpha * (double)pv[e]);
      rv[e] = (float)((double)rv[e] - alpha * (double)qv[e]);
      acc += (double)rv[e] * (double)rv[e];                  // (elements past the end are 0)
      acc_z += (double)rv[e] * ((double)rv[e] / screened_diagonal(six_h2, weight, wv[e]));
    }
    store4(x, g * kGroup, total, vec_x, xv);
    store4(r, g * kGroup, total, true, rv);
  }
  const double sum = block_sum(acc, red);
  const double sum_z = block_sum(acc_z, red);
  if (threadIdx.x == 0) { partial[blockIdx.x] = sum; partial_z[blockIdx.x] = sum_z; }
}

// p = r / d + beta p
__global__ __launch_bounds__(kThreads) void pcg_direction_kernel(long long total, int vec_w, double six_h2, double weight,
                                                                 const double* __restrict__ scal, const float* __restrict__ W,
                                                                 const float* __restrict__ r, float* __restrict__ p) {
  const long long groups = (total + kGroup - 1) / kGroup;
  const double beta = scal[kBeta];
  for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kThreads) {
    float rv[4], pv[4], wv[4];
    load4(r, g * kGroup, total, true, rv);
    load4(p, g * kGroup, total, true, pv);
    load4(W, g * kGroup, total, vec_w, wv);
#pragma unroll
    for (int e = 0; e < kGroup; ++e) pv[e] = (float)((double)rv[e] / screened_diagonal(six_h2, weight, wv[e]) + beta * (double)pv[e]);
    store4(p, g * kGroup, total, true, pv);
  }
}

// cg_scalars_kernel's order over two rows of partials (partial_z is not read in kModePQ); thread 0 updates the scalars
__global__ __launch_bounds__(kThreads) void pcg_scalars_kernel(const double* __restrict__ partial, const double* __restrict__ partial_z,
                                                               int n_partials, int mode, double* __restrict__ scal) {
  __shared__ double red[kThreads];
  double acc = 0.0, acc_z = 0.0;
  for (int b = threadIdx.x; b < n_partials; b += kThreads) {
    acc += partial[b];
    if (mode != kModePQ) acc_z += partial_z[b];
  }
  const double sum = block_sum(acc, red);
  const double sum_z = block_sum(acc_z, red);
  if (threadIdx.x != 0) return;
  if (mode == kModeInit) {
    scal[kRR] = sum; scal[kBB] = sum; scal[kRN] = sum; scal[kRZ] = sum_z; scal[kAlpha] = 0.0; scal[kBeta] = 0.0;
  } else if (mode == kModePQ) {
    scal[kAlpha] = sum > 0.0 ? scal[kRZ] / sum : 0.0;        // p = 0 (r = 0 exactly): nothing moves any more
  } else {
    const double rz = scal[kRZ];
    scal[kBeta] = rz > 0.0 ? sum_z / rz : 0.0;
    scal[kRR] = sum; scal[kRN] = sum; scal[kRZ] = sum_z;
  }
}

// ---- sample, level, trim -------------------------------------------------------------------------------------------------
// vals[i] = the trilinear value of x at point i (NaN for a point that does not count); partial[workgroup] = the sum over
// the workgroup's counted points, cpartial[workgroup] = their number
__global__ __launch_bounds__(kThreads) void sample_kernel(const float* __restrict__ x, Grid g, const double* __restrict__ pts, int n,
                                                          double* __restrict__ vals, double* __restrict__ partial, double* __restrict__ cpartial) {
  __shared__ double red[kThreads];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  double v = 0.0, one = 0.0;
  if (i < n) {
    long long b[3];
    double t[3];
    if (locate(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], b, t)) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const long long at = ((b[0] + (c >> 2)) * g.n1 + (b[1] + ((c >> 1) & 1))) * g.n2 + (b[2] + (c & 1));
        v += corner_weight(t, c) * (double)x[at];
      }
      one = 1.0;
      vals[i] = v;
    } else {
      vals[i] = __builtin_nan("");
    }
  }
  const double s = block_sum(v, red);
  const double c = block_sum(one, red);
  if (threadIdx.x == 0) { partial[blockIdx.x] = s; cpartial[blockIdx.x] = c; }
}

// out[0] = sum / count (0 when nothing counts), out[1] = count: the partials in the order of cg_scalars_kernel
__global__ __launch_bounds__(kThreads) void level_kernel(const double* __restrict__ partial, const double* __restrict__ cpartial, int n_partials,
                                                         double* __restrict__ out) {
  __shared__ double red[kThreads];
  double acc = 0.0, cnt = 0.0;
  for (int b = threadIdx.x; b < n_partials; b += kThreads) { acc += partial[b]; cnt += cpartial[b]; }
  const double s = block_sum(acc, red);
  const double c = block_sum(cnt, red);
  if (threadIdx.x == 0) { out[0] = c > 0.0 ? s / c : 0.0; out[1] = c; }
}

// keep[f] = the float64 sum, in corner order from zero, of W over the eight nodes of the face's cell is >= min_density
__global__ __launch_bounds__(256) void face_keep_kernel(const float* __restrict__ W, long long n0, long long n1, long long n2,
                                                        const int* __restrict__ cells, int n_faces, double min_density,
                                                        uint8_t* __restrict__ keep) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  const long long node = cells[f];
  bool ok = node >= 0 && node < n0 * n1 * n2;
  if (ok) {
    const long long row = node / n2, k = node - row * n2, i = row / n1, j = row - i * n1;
    ok = i + 1 < n0 && j + 1 < n1 && k + 1 < n2;            // a node on an upper face stands for no cell
    if (ok) {
      double sum = 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) sum += (double)W[((i + (c >> 2)) * n1 + (j + ((c >> 1) & 1))) * n2 + (k + (c & 1))];
      ok = sum >= min_density;                               // a NaN sum fails
    }
  }
  keep[f] = ok ? 1 : 0;
}

}  // namespace poisson
}  // namespace svs

using namespace svs;
using namespace svs::poisson;
using namespace svs::ws;

namespace {

// cells of a grid; 0 when a size is below 2
long long cell_count(int n0, int n1, int n2) {
  if (n0 < 2 || n1 < 2 || n2 < 2) return 0;
  return (long long)(n0 - 1) * (n1 - 1) * (n2 - 1);
}

struct SplatLayout {
  size_t keys, skeys, vals, svals, head, hoff, flag, soff, run_first, seg_start, part, cell_seg, counts, sort_tmp, sort_size, total;
  int max_segs;
};
SplatLayout splat_layout(int n, long long cells) {
  SplatLayout L;
  Bump b;
  const size_t np = (size_t)n;
  // a cell of m points has ceil(m / 64) <= m / 64 + 1 segments
  const size_t segs = np / kSegment + ((long long)np < cells ? np : (size_t)cells) + 1;
  L.max_segs = (int)(segs < 0x7fffffff ? segs : 0x7fffffff);
  L.keys = b.take(4 * np); L.skeys = b.take(4 * np); L.vals = b.take(4 * np); L.svals = b.take(4 * np);
  L.head = b.take(np); L.hoff = b.take(4 * np); L.flag = b.take(np); L.soff = b.take(4 * np);
  L.run_first = b.take(4 * (np + 2)); L.seg_start = b.take(4 * segs); L.part = b.take(sizeof(Partial) * segs);
  L.cell_seg = b.take(4 * (size_t)cells); L.counts = b.take(4 * sizeof(int));
  L.sort_size = runs::sort_scratch_bytes<unsigned, true>(np); L.sort_tmp = b.take(L.sort_size);
  L.total = b.o;
  return L;
}

struct CgLayout { size_t r, p, q, partial, scal, total; int n_partials; };
int stencil_blocks(int n0, int n1, int n2, dim3* grid) {
  const long long gx = (n2 + kTileK - 1) / kTileK, gy = (n1 + kTileJ - 1) / kTileJ, gz = (n0 + kTileI - 1) / kTileI;
  if (grid) *grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
  return (int)(gx * gy * gz);                                // <= 2^31 / 2^14 workgroups for a volume of int32 sizes below 2^31 nodes
}
// rows: the dot products a flat pass leaves partials of (the preconditioned solve's r.r and r.z: row 1 lies n_partials behind row 0)
CgLayout cg_layout(int n0, int n1, int n2, int rows = 1) {
  CgLayout L;
  Bump b;
  const size_t total = (size_t)n0 * n1 * n2;
  const int sb = stencil_blocks(n0, n1, n2, nullptr);
  L.n_partials = sb > kFlatBlocks ? sb : kFlatBlocks;
  L.r = b.take(4 * total); L.p = b.take(4 * total); L.q = b.take(4 * total);
  L.partial = b.take(sizeof(double) * (size_t)L.n_partials * (size_t)rows); L.scal = b.take(sizeof(double) * kScalars);
  L.total = b.o;
  return L;
}

int flat_blocks(long long total) {
  const long long groups = (total + kGroup - 1) / kGroup, blocks = (groups + kThreads - 1) / kThreads;
  return (int)(blocks < kFlatBlocks ? blocks : kFlatBlocks);
}

// the checks every entry shares: sizes (two nodes along every axis, fewer than 2^31 nodes), then the spacing
int check_grid(const char* name, int n0, int n1, int n2) {
  if (n0 < 2 || n1 < 2 || n2 < 2) { set_error("%s: a grid needs two nodes along every axis, got %d x %d x %d", name, n0, n1, n2); return SVS_ESHAPE; }
  if ((long long)n0 * n1 * n2 > 0x7fffffffLL) { set_error("%s: more than 2^31 - 1 nodes", name); return SVS_ESHAPE; }
  return SVS_OK;
}
int check_h(const char* name, double h) { return check_spacing(name, h, "node spacing"); }

void launch_stencil(const float* p, float* q, int n0, int n1, int n2, double h, double* partial, hipStream_t s) {
  dim3 grid;
  stencil_blocks(n0, n1, n2, &grid);
  const Vol v = {n0, n1, n2};
  const double h2 = h * h;
  const bool vec = (n2 % kGroup) == 0 && (((uintptr_t)p | (uintptr_t)q) & 15u) == 0;
  if (vec) stencil_kernel<true, false><<<grid, kThreads, 0, s>>>(p, q, v, h2, partial, nullptr, 0.0);
  else stencil_kernel<false, false><<<grid, kThreads, 0, s>>>(p, q, v, h2, partial, nullptr, 0.0);
}

// the screened instantiations: the 16-byte path needs W aligned as well
void launch_screened_stencil(const float* p, const float* W, float* q, int n0, int n1, int n2, double h, double weight, double* partial,
                             hipStream_t s) {
  dim3 grid;
  stencil_blocks(n0, n1, n2, &grid);
  const Vol v = {n0, n1, n2};
  const double h2 = h * h;
  const bool vec = (n2 % kGroup) == 0 && (((uintptr_t)p | (uintptr_t)q | (uintptr_t)W) & 15u) == 0;
  if (vec) stencil_kernel<true, true><<<grid, kThreads, 0, s>>>(p, q, v, h2, partial, W, weight);
  else stencil_kernel<false, true><<<grid, kThreads, 0, s>>>(p, q, v, h2, partial, W, weight);
}

int check_stopping(const char* name, double tol, int max_iter, int check_every) {
  if (!(tol > 0.0) || !(tol < 1.0)) { set_error("%s: tol must lie in (0,1)", name); return SVS_EINVAL; }
  if (max_iter < 1 || check_every < 1) { set_error("%s: max_iter and check_every must be at least 1", name); return SVS_EINVAL; }
  return SVS_OK;
}

// the host side of both solves: start() enqueues the first pass and the scalars, step() one iteration; every check_every
// iterations and at max_iter the 8 bytes of rn come down and the solve stops when rn <= tol^2 bb
template <typename Start, typename Step>
int cg_drive(const char* name, const double* scal, double tol, int max_iter, int check_every, hipStream_t s, int* iterations,
             double* residual, int* converged, Start start, Step step) {
  *iterations = 0; *residual = 0.0; *converged = 0;
  start();
  int rc = check_launch(name);
  if (rc) return rc;
  double bb = 0.0, rn = 0.0;
  rc = download(name, scal + kBB, 1, &bb, s);
  if (rc) return rc;
  if (!(bb > 0.0) || !finite_f64(bb)) {
    set_error("%s: no normal field (the right-hand side is zero or not finite: |rhs|^2 = %g)", name, bb); return SVS_EINVAL;
  }
  rn = bb;
  int it = 0;
  while (it < max_iter) {
    step();
    ++it;
    if (it % check_every == 0 || it == max_iter) {
      rc = check_launch(name);
      if (rc) return rc;
      rc = download(name, scal + kRN, 1, &rn, s);
      if (rc) return rc;
      if (rn <= tol * tol * bb) { *converged = 1; break; }
      if (!finite_f64(rn)) break;                            // not finite: more iterations change nothing
    }
  }
  *iterations = it;
  *residual = __builtin_sqrt(rn / bb);
  return SVS_OK;
}

int check_weight(const char* name, double weight) {
  if (!(weight >= 0.0) || !finite_f64(weight)) { set_error("%s: the screening weight must be finite and not negative, got %g", name, weight); return SVS_EINVAL; }
  return SVS_OK;
}

}  // namespace

extern "C" {

int svs_poisson_tile(int* tile) {
  if (!tile) return null_pointer("svs_poisson_tile");
  tile[0] = kTileI; tile[1] = kTileJ; tile[2] = kTileK;
  return SVS_OK;
}

size_t svs_poisson_splat_workspace_bytes(int n, int n0, int n1, int n2) {
  if (n < 0) n = 0;
  return splat_layout(n, cell_count(n0, n1, n2)).total + 256;
}

int svs_poisson_splat(const double* pts, const float* normals, int n, int n0, int n1, int n2, const double* origin, double h,
                      void* workspace, float* field, int* counts, void* hip_stream) {
  const char* name = "svs_poisson_splat";
  int rc = check_grid(name, n0, n1, n2);
  if (rc) return rc;
  if (n <= 0) { set_error("%s: no points (n = %d)", name, n); return SVS_ESHAPE; }
  if (!pts || !normals || !workspace || !field || !counts) return null_pointer(name);
  rc = check_origin(name, origin);
  if (rc) return rc;
  rc = check_h(name, h);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const long long cells = cell_count(n0, n1, n2), total = (long long)n0 * n1 * n2;
  const SplatLayout L = splat_layout(n, cells);
  char* base = aligned(workspace);
  unsigned* keys = (unsigned*)(base + L.keys); unsigned* skeys = (unsigned*)(base + L.skeys);
  unsigned* vals = (unsigned*)(base + L.vals); unsigned* svals = (unsigned*)(base + L.svals);
  uint8_t* head = (uint8_t*)(base + L.head); uint8_t* flag = (uint8_t*)(base + L.flag);
  int* hoff = (int*)(base + L.hoff); int* soff = (int*)(base + L.soff);
  int* run_first = (int*)(base + L.run_first); int* seg_start = (int*)(base + L.seg_start);
  Partial* part = (Partial*)(base + L.part); int* cell_seg = (int*)(base + L.cell_seg);
  int* dcounts = (int*)(base + L.counts);                    // counted, runs, segments
  const Grid g = {origin[0], origin[1], origin[2], h, n0, n1, n2};
  const int nb = (n + 255) / 256;
  hipError_t e = hipMemsetAsync(cell_seg, 0xff, sizeof(int) * (size_t)cells, s);
  if (e != hipSuccess) return hip_fail(name, e);
  point_keys_kernel<<<nb, 256, 0, s>>>(pts, normals, n, g, (unsigned)cells, keys, vals, dcounts);
  rc = runs::sort_pairs(name, base + L.sort_tmp, L.sort_size, keys, skeys, vals, svals, n, runs::bit_length((unsigned)cells), s);
  if (rc) return rc;
  run_heads_kernel<<<nb, 256, 0, s>>>(skeys, n, (unsigned)cells, head, dcounts);
  scan::mask_offsets(head, n, hoff, dcounts + 1, s);
  run_first_kernel<<<nb, 256, 0, s>>>(head, hoff, n, run_first);
  seg_flags_kernel<<<nb, 256, 0, s>>>(skeys, n, (unsigned)cells, head, hoff, run_first, flag);
  scan::mask_offsets(flag, n, soff, dcounts + 2, s);
  runs::seg_start_kernel<256><<<nb, 256, 0, s>>>(flag, soff, n, L.max_segs, seg_start);
  seg_sum_kernel<<<(L.max_segs + 255) / 256, 256, 0, s>>>(pts, normals, g, svals, head, hoff, run_first, seg_start, dcounts + 2, L.max_segs, part);
  cell_sum_kernel<<<nb, 256, 0, s>>>(skeys, (unsigned)cells, run_first, soff, dcounts + 1, n, L.max_segs, part, cell_seg);
  node_gather_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(g, cell_seg, part, field);
  rc = check_launch(name);
  if (rc) return rc;
  int counted = 0;
  rc = download(name, dcounts, 1, &counted, s);
  if (rc) return rc;
  counts[0] = counted; counts[1] = n - counted;
  return SVS_OK;
}

int svs_poisson_divergence(const float* field, int n0, int n1, int n2, double h, float* rhs, void* hip_stream) {
  const char* name = "svs_poisson_divergence";
  int rc = check_grid(name, n0, n1, n2);
  if (rc) return rc;
  if (!field || !rhs) return null_pointer(name);
  rc = check_h(name, h);
  if (rc) return rc;
  const long long total = (long long)n0 * n1 * n2;
  divergence_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(field, n0, n1, n2, h, rhs);
  return check_launch(name);
}

int svs_poisson_apply(const float* x, int n0, int n1, int n2, double h, float* y, void* hip_stream) {
  const char* name = "svs_poisson_apply";
  int rc = check_grid(name, n0, n1, n2);
  if (rc) return rc;
  if (!x || !y) return null_pointer(name);
  if (x == y) { set_error("%s: bad argument (x and y are the same array)", name); return SVS_EINVAL; }
  rc = check_h(name, h);
  if (rc) return rc;
  launch_stencil(x, y, n0, n1, n2, h, nullptr, (hipStream_t)hip_stream);
  return check_launch(name);
}

size_t svs_poisson_cg_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 2 || n1 < 2 || n2 < 2 || (long long)n0 * n1 * n2 > 0x7fffffffLL) return 0;
  return cg_layout(n0, n1, n2).total + 256;
}

int svs_poisson_cg(const float* rhs, int n0, int n1, int n2, double h, double tol, int max_iter, int check_every, void* workspace,
                   float* x, int* iterations, double* residual, int* converged, void* hip_stream) {
  const char* name = "svs_poisson_cg";
  int rc = check_grid(name, n0, n1, n2);
  if (rc) return rc;
  if (!rhs || !workspace || !x || !iterations || !residual || !converged) return null_pointer(name);
  rc = check_h(name, h);
  if (rc) return rc;
  rc = check_stopping(name, tol, max_iter, check_every);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const long long total = (long long)n0 * n1 * n2;
  const CgLayout L = cg_layout(n0, n1, n2);
  char* base = aligned(workspace);
  float* r = (float*)(base + L.r); float* p = (float*)(base + L.p); float* q = (float*)(base + L.q);
  double* partial = (double*)(base + L.partial); double* scal = (double*)(base + L.scal);
  const int fb = flat_blocks(total), sb = stencil_blocks(n0, n1, n2, nullptr);
  const int vec_rhs = ((uintptr_t)rhs & 15u) == 0, vec_x = ((uintptr_t)x & 15u) == 0;
  return cg_drive(name, scal, tol, max_iter, check_every, s, iterations, residual, converged,
                  [&] {
                    cg_init_kernel<<<fb, kThreads, 0, s>>>(rhs, total, vec_rhs, vec_x, x, r, p, partial);
                    cg_scalars_kernel<<<1, kThreads, 0, s>>>(partial, fb, kModeInit, scal);
                  },
                  [&] {
                    launch_stencil(p, q, n0, n1, n2, h, partial, s);
                    cg_scalars_kernel<<<1, kThreads, 0, s>>>(partial, sb, kModePQ, scal);
                    cg_axpy_kernel<<<fb, kThreads, 0, s>>>(total, vec_x, scal, x, r, p, q, partial);
                    cg_scalars_kernel<<<1, kThreads, 0, s>>>(partial, fb, kModeRR, scal);
                    cg_direction_kernel<<<fb, kThreads, 0, s>>>(total, scal, r, p);
                  });
}

int svs_screened_apply(const float* x, const float* W, int n0, int n1, int n2, double h, double weight, float* y, void* hip_stream) {
  const char* name = "svs_screened_apply";
  int rc = check_grid(name, n0, n1, n2);
  if (rc) return rc;
  if (!x || !W || !y) return null_pointer(name);
  if (x == y) { set_error("%s: bad argument (x and y are the same array)", name); return SVS_EINVAL; }
  rc = check_h(name, h);
  if (rc) return rc;
  rc = check_weight(name, weight);
  if (rc) return rc;
  launch_screened_stencil(x, W, y, n0, n1, n2, h, weight, nullptr, (hipStream_t)hip_stream);
  return check_launch(name);
}

size_t svs_screened_pcg_workspace_bytes(int n0, int n1, int n2) {
  if (n0 < 2 || n1 < 2 || n2 < 2 || (long long)n0 * n1 * n2 > 0x7fffffffLL) return 0;
  return cg_layout(n0, n1, n2, 2).total + 256;
}

int svs_screened_pcg(const float* rhs, const float* W, int n0, int n1, int n2, double h, double weight, double tol, int max_iter,
                     int check_every, void* workspace, float* x, int* iterations, double* residual, int* converged, void* hip_stream) {
  const char* name = "svs_screened_pcg";
  int rc = check_grid(name, n0, n1, n2);
  if (rc) return rc;
  if (!rhs || !W || !workspace || !x || !iterations || !residual || !converged) return null_pointer(name);
  rc = check_h(name, h);
  if (rc) return rc;
  rc = check_weight(name, weight);
  if (rc) return rc;
  rc = check_stopping(name, tol, max_iter, check_every);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const long long total = (long long)n0 * n1 * n2;
  const CgLayout L = cg_layout(n0, n1, n2, 2);
  char* base = aligned(workspace);
  float* r = (float*)(base + L.r); float* p = (float*)(base + L.p); float* q = (float*)(base + L.q);
  double* partial = (double*)(base + L.partial); double* partial_z = partial + L.n_partials; double* scal = (double*)(base + L.scal);
  const int fb = flat_blocks(total), sb = stencil_blocks(n0, n1, n2, nullptr);
  const int vec_rhs = ((uintptr_t)rhs & 15u) == 0, vec_x = ((uintptr_t)x & 15u) == 0, vec_w = ((uintptr_t)W & 15u) == 0;
  const double six_h2 = 6.0 / (h * h);
  return cg_drive(name, scal, tol, max_iter, check_every, s, iterations, residual, converged,
                  [&] {
                    pcg_init_kernel<<<fb, kThreads, 0, s>>>(rhs, W, total, vec_rhs, vec_w, vec_x, six_h2, weight, x, r, p, partial, partial_z);
                    pcg_scalars_kernel<<<1, kThreads, 0, s>>>(partial, partial_z, fb, kModeInit, scal);
                  },
                  [&] {
                    launch_screened_stencil(p, W, q, n0, n1, n2, h, weight, partial, s);
                    pcg_scalars_kernel<<<1, kThreads, 0, s>>>(partial, partial_z, sb, kModePQ, scal);
                    pcg_axpy_kernel<<<fb, kThreads, 0, s>>>(total, vec_x, vec_w, six_h2, weight, scal, W, x, r, p, q, partial, partial_z);
                    pcg_scalars_kernel<<<1, kThreads, 0, s>>>(partial, partial_z, fb, kModeRR, scal);
                    pcg_direction_kernel<<<fb, kThreads, 0, s>>>(total, vec_w, six_h2, weight, scal, W, r, p);
                  });
}

size_t svs_poisson_sample_workspace_bytes(int n) {
  if (n < 0) n = 0;
  return 2 * sizeof(double) * (size_t)((n + kThreads - 1) / kThreads + 1) + 2 * sizeof(double) + 512;
}

int svs_poisson_sample(const float* x, int n0, int n1, int n2, const double* origin, double h, const double* pts, int n,
                       void* workspace, double* vals, double* level, int* counted, void* hip_stream) {
  const char* name = "svs_poisson_sample";
  int rc = check_grid(name, n0, n1, n2);
  if (rc) return rc;
  if (n <= 0) { set_error("%s: no points (n = %d)", name, n); return SVS_ESHAPE; }
  if (!x || !pts || !workspace || !vals || !level || !counted) return null_pointer(name);
  rc = check_origin(name, origin);
  if (rc) return rc;
  rc = check_h(name, h);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const int nb = (n + kThreads - 1) / kThreads;
  double* partial = (double*)aligned(workspace);
  double* cpartial = partial + nb;
  double* out = cpartial + nb;
  const Grid g = {origin[0], origin[1], origin[2], h, n0, n1, n2};
  sample_kernel<<<nb, kThreads, 0, s>>>(x, g, pts, n, vals, partial, cpartial);
  level_kernel<<<1, kThreads, 0, s>>>(partial, cpartial, nb, out);
  rc = check_launch(name);
  if (rc) return rc;
  double host[2] = {0.0, 0.0};
  rc = download(name, out, 2, host, s);
  if (rc) return rc;
  *level = host[0]; *counted = (int)host[1];
  return SVS_OK;
}

int svs_poisson_face_keep(const float* W, int n0, int n1, int n2, const int* cells, int n_faces, double min_density, uint8_t* keep,
                          void* hip_stream) {
  const char* name = "svs_poisson_face_keep";
  int rc = check_grid(name, n0, n1, n2);
  if (rc) return rc;
  if (n_faces < 0) { set_error("%s: negative count", name); return SVS_ESHAPE; }
  if (n_faces == 0) return SVS_OK;
  if (!W || !cells || !keep) return null_pointer(name);
  face_keep_kernel<<<(n_faces + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(W, n0, n1, n2, cells, n_faces, min_density, keep);
  return check_launch(name);
}

}  // extern "C"
