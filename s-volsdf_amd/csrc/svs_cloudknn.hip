// Cleaning a fused point cloud on gfx950: k nearest neighbours, the statistics of statistical outlier removal, and
// PCA normals oriented towards the cameras (svs_hip/clouds.py, svs_hip/cloudclean.py).
//
// The neighbour search is svs_cloud.hip's: the uniform grid of svs_cloud_grid.h, rings of cells outwards, float64 distances
// in the kd-tree's arithmetic (ex*ex + ey*ey + ez*ez, no fused multiply-add: this unit is compiled with -ffp-contract=off).
// Going from one neighbour to k adds an ordered list per query.  It lives in LDS, laid out [slot][lane]: one lane owns one
// query, a wave's accesses to one slot are 64 consecutive 8-byte (distances) or 4-byte (indices) words -- conflict-free --
// and a runtime slot index costs nothing there, where a register array indexed at run time would go to scratch.  A
// workgroup is one wave: 64 * k * 12 bytes of LDS, 24 KB at k = 32, so six workgroups fit the 160 KB of a CU at the
// largest k and no barrier is needed (a lane touches its own column only).  Latency / gather bound work: no matrix cores.
#include "svs_cloud_grid.h"
#include "svs_common.h"
#include "svs_jacobi3.h"

namespace svs {
namespace cloud {

constexpr int kKnnLanes = 64;
constexpr int kKnnMaxK = 32;

__device__ __forceinline__ bool before(double d2, unsigned oj, double e2, unsigned ej) {
  return d2 < e2 || (d2 == e2 && oj < ej);                 // the order of the lists: (d2, original index)
}

// SORTED: the queries are the grid's own points (query == ref): lane t takes sorted position t, so that neighbouring lanes
// read neighbouring cells, and writes row perm[t].  exclude_base >= 0: reference exclude_base + row is skipped for query row.
template <bool SORTED>
__global__ __launch_bounds__(kKnnLanes) void knn_kernel(Grid g, const double* __restrict__ q, int nq, int k, int max_ring, double max_radius,
                                                        long long exclude_base, double* __restrict__ dist, int* __restrict__ idx,
                                                        double* __restrict__ mean_dist) {
  extern __shared__ double knn_lds[];                       // d2 [k][64] float64, then index [k][64] uint32
  double* sd = knn_lds + threadIdx.x;
  unsigned* si = (unsigned*)(knn_lds + (size_t)kKnnLanes * k) + threadIdx.x;
  const int t = blockIdx.x * kKnnLanes + threadIdx.x;
  if (t >= nq) return;
  const double* p = SORTED ? g.pts + 3 * (size_t)t : q + 3 * (size_t)t;
  const size_t row = SORTED ? (size_t)g.perm[t] : (size_t)t;
  const double x = p[0], y = p[1], z = p[2];
  const long long self = exclude_base >= 0 ? exclude_base + (long long)row : -1;
  const int cx = cell_coord(x, g.ox, g.inv_h), cy = cell_coord(y, g.oy, g.inv_h), cz = cell_coord(z, g.oz, g.inv_h);
  // margin to the walls of the (clamped) home cell, as nn_kernel's
  double margin = 1e300;
  {
    const double fx = (x - g.ox) * g.inv_h - (double)cx, fy = (y - g.oy) * g.inv_h - (double)cy, fz = (z - g.oz) * g.inv_h - (double)cz;
    const double m[6] = {fx, 1.0 - fx, fy, 1.0 - fy, fz, 1.0 - fz};
#pragma unroll
    for (int a = 0; a < 6; ++a) margin = m[a] < margin ? m[a] : margin;
    margin *= g.h;
  }
  // nothing at or beyond max_radius is ever listed: sqrt(d2) >= max_radius for certain once d2 exceeds this
  const double d2_cut = max_radius * max_radius * (1.0 + 1e-12);
  int cnt = 0;
  double worst = 1e300;                                     // the k-th entry once the list is full
  unsigned worst_idx = 0xffffffffu;
  for (int r = 0; r <= max_ring; ++r) {
    for (int dz = -r; dz <= r; ++dz)
      for (int dy = -r; dy <= r; ++dy) {
        const bool face = dz == -r || dz == r || dy == -r || dy == r;
        const int step = face ? 1 : (2 * r > 0 ? 2 * r : 1);           // interior rows of the shell: only the two x ends
        for (int dx = -r; dx <= r; dx += step) {
          const uint2 run = find_run(g, cx + dx, cy + dy, cz + dz);
          for (unsigned j = run.x; j < run.y; ++j) {
            const double ex = g.pts[3 * (size_t)j] - x, ey = g.pts[3 * (size_t)j + 1] - y, ez = g.pts[3 * (size_t)j + 2] - z;
            const double d2 = ex * ex + ey * ey + ez * ez;
            if (d2 > d2_cut) continue;
            const unsigned oj = g.perm[j];
            if ((long long)oj == self) continue;
            if (cnt == k && !before(d2, oj, worst, worst_idx)) continue;
            int s = cnt < k ? cnt : k - 1;                  // the slot that opens; entries after the new one move up by one
            while (s > 0) {
              const double pd = sd[(s - 1) * kKnnLanes];
              const unsigned pi = si[(s - 1) * kKnnLanes];
              if (!before(d2, oj, pd, pi)) break;
              sd[s * kKnnLanes] = pd; si[s * kKnnLanes] = pi;
              --s;
            }
            sd[s * kKnnLanes] = d2; si[s * kKnnLanes] = oj;
            if (cnt < k) ++cnt;
            if (cnt == k) { worst = sd[(k - 1) * kKnnLanes]; worst_idx = si[(k - 1) * kKnnLanes]; }
          }
        }
      }
    const double safe = (double)r * g.h + margin;
    if (cnt == k && safe > 0.0 && worst <= safe * safe) break;
  }
  double sum = 0.0;
  int finite = 0;
  for (int s = 0; s < k; ++s) {
    double d = __builtin_inf();
    int o = -1;
    if (s < cnt) {
      const double v = __builtin_sqrt(sd[s * kKnnLanes]);
      if (v < max_radius) { d = v; o = (int)si[s * kKnnLanes]; sum += v; ++finite; }
    }
    if (dist) dist[row * k + s] = d;
    if (idx) idx[row * k + s] = o;
  }
  if (mean_dist) mean_dist[row] = finite ? sum / (double)finite : __builtin_inf();
}

// ---- statistics of the finite mean distances: one fixed two-level order, no atomics (the pattern of mean_partial_kernel) ----
constexpr int kStatBlocks = 256;

// SECOND == false: per block (sum, count) of the finite entries; SECOND: (sum of squared deviations from *mean, count)
template <bool SECOND>
__global__ __launch_bounds__(256) void stats_partial_kernel(const double* __restrict__ d, int n, const double* __restrict__ mean,
                                                            double* __restrict__ part) {
  __shared__ double ss[256], sc[256];
  const double m = SECOND ? mean[0] : 0.0;
  double s = 0.0, c = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)kStatBlocks * 256) {
    const double v = d[i];
    if (finite_f64(v)) { s += SECOND ? (v - m) * (v - m) : v; c += 1.0; }
  }
  ss[threadIdx.x] = s; sc[threadIdx.x] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { ss[threadIdx.x] += ss[threadIdx.x + w]; sc[threadIdx.x] += sc[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = ss[0]; part[2 * blockIdx.x + 1] = sc[0]; }
}
template <bool SECOND>
__global__ void stats_final_kernel(const double* __restrict__ part, double* __restrict__ out) {
  double s = 0.0, c = 0.0;
  for (int b = 0; b < kStatBlocks; ++b) { s += part[2 * b]; c += part[2 * b + 1]; }
  if (SECOND) {
    out[2] = c < 2.0 ? 0.0 : __builtin_sqrt(s / (c - 1.0));
  } else {
    out[0] = c;
    out[1] = c > 0.0 ? s / c : 0.0;
  }
}

__global__ void outlier_mask_kernel(const double* __restrict__ d, int n, double threshold, uint8_t* __restrict__ keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = d[i];
  keep[i] = (finite_f64(v) && v <= threshold) ? 1 : 0;
}

// ---- normals: the eigenvector of the smallest eigenvalue of the neighbourhood's covariance, by cyclic Jacobi (svs_jacobi3.h) ----
__global__ __launch_bounds__(256) void normals_kernel(const double* __restrict__ pts, int n, const int* __restrict__ idx, int k,
                                                      int include_self, const int* __restrict__ view_index,
                                                      const double* __restrict__ centres, int n_views, float* __restrict__ normals,
                                                      float* __restrict__ curvature) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
  const int* nb = idx + (size_t)i * k;
  // two passes over the set: centroid, then the covariance about it (the point itself first, then the slots in order)
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int m = 0;
  if (include_self) { sx = px; sy = py; sz = pz; m = 1; }
  for (int s = 0; s < k; ++s) {
    const int j = nb[s];
    if (j < 0 || j >= n) continue;
    sx += pts[3 * (size_t)j]; sy += pts[3 * (size_t)j + 1]; sz += pts[3 * (size_t)j + 2];
    ++m;
  }
  float nx = 0.0f, ny = 0.0f, nz = 0.0f, curv = 0.0f;
  if (m >= 3) {
    const double inv_m = 1.0 / (double)m;
    const double mx = sx * inv_m, my = sy * inv_m, mz = sz * inv_m;
    double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
    if (include_self) {
      const double ex = px - mx, ey = py - my, ez = pz - mz;
      cxx = ex * ex; cxy = ex * ey; cxz = ex * ez; cyy = ey * ey; cyz = ey * ez; czz = ez * ez;
    }
    for (int s = 0; s < k; ++s) {
      const int j = nb[s];
      if (j < 0 || j >= n) continue;
      const double ex = pts[3 * (size_t)j] - mx, ey = pts[3 * (size_t)j + 1] - my, ez = pts[3 * (size_t)j + 2] - mz;
      cxx += ex * ex; cxy += ex * ey; cxz += ex * ez; cyy += ey * ey; cyz += ey * ez; czz += ez * ez;
    }
    double a[3][3] = {{cxx * inv_m, cxy * inv_m, cxz * inv_m}, {cxy * inv_m, cyy * inv_m, cyz * inv_m}, {cxz * inv_m, cyz * inv_m, czz * inv_m}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    jacobi_sweeps(a, v);
    const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
    // the smallest eigenvalue's column, the lowest index on a tie (selected, not indexed)
    const bool pick1 = l1 < l0 && l1 <= l2, pick2 = l2 < l0 && l2 < l1;
    double ex = pick2 ? v[0][2] : (pick1 ? v[0][1] : v[0][0]);
    double ey = pick2 ? v[1][2] : (pick1 ? v[1][1] : v[1][0]);
    double ez = pick2 ? v[2][2] : (pick1 ? v[2][1] : v[2][0]);
    const double lmin = pick2 ? l2 : (pick1 ? l1 : l0);
    const double trace = l0 + l1 + l2;
    curv = trace > 0.0 ? (float)((lmin > 0.0 ? lmin : 0.0) / trace) : 0.0f;
    const double len = __builtin_sqrt(ex * ex + ey * ey + ez * ez);
    if (len > 0.0) { ex /= len; ey /= len; ez /= len; }
    if (centres && n_views > 0) {
      int c = 0;
      if (view_index) {
        c = view_index[i];
        c = c < 0 ? 0 : (c >= n_views ? n_views - 1 : c);
      } else {
        double best = 1e300;
        for (int w = 0; w < n_views; ++w) {
          const double dx = centres[3 * w] - px, dy = centres[3 * w + 1] - py, dz = centres[3 * w + 2] - pz;
          const double d2 = dx * dx + dy * dy + dz * dz;
          if (d2 < best) { best = d2; c = w; }
        }
      }
      const double dot = ex * (centres[3 * c] - px) + ey * (centres[3 * c + 1] - py) + ez * (centres[3 * c + 2] - pz);
      if (dot < 0.0) { ex = -ex; ey = -ey; ez = -ez; }
    }
    nx = (float)ex; ny = (float)ey; nz = (float)ez;
  }
  normals[3 * (size_t)i] = nx; normals[3 * (size_t)i + 1] = ny; normals[3 * (size_t)i + 2] = nz;
  if (curvature) curvature[i] = curv;
}

}  // namespace cloud
}  // namespace svs

using namespace svs;
using namespace svs::cloud;

extern "C" {

int svs_cloud_knn(const double* ref, int n_ref, const double* query, int n_query, const double* origin, double cell, int k,
                  double max_radius, int exclude_same_index, void* grid_ws, double* dist, int* idx, double* mean_dist,
                  void* hip_stream) {
  if (!ref || !query || !origin || !grid_ws || n_ref < 0 || n_query < 0 || exclude_same_index < 0) {
    set_error("svs_cloud_knn: bad argument"); return SVS_EINVAL;
  }
  if (!dist && !idx && !mean_dist) { set_error("svs_cloud_knn: bad argument (no output)"); return SVS_EINVAL; }
  if (k < 1 || k > kKnnMaxK) { set_error("svs_cloud_knn: k must be in [1,%d]", kKnnMaxK); return SVS_EINVAL; }
  if (!(cell > 0.0) || !(max_radius > 0.0) || !(max_radius / cell <= 4096.0)) {
    set_error("svs_cloud_knn: need 0 < cell, 0 < max_radius <= 4096 cells"); return SVS_ESHAPE;
  }
  if (n_query == 0) return SVS_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  Grid g;
  int rc = build_grid(ref, n_ref, origin, cell, grid_ws, s, &g);
  if (rc) return rc;
  const int max_ring = n_ref == 0 ? 0 : (int)__builtin_ceil(max_radius / cell) + 1;
  const long long exclude_base = exclude_same_index ? (long long)exclude_same_index - 1 : -1;
  const size_t lds = (size_t)kKnnLanes * k * (sizeof(double) + sizeof(unsigned));
  const int blocks = (n_query + kKnnLanes - 1) / kKnnLanes;
  if (query == ref && n_query == n_ref)
    knn_kernel<true><<<blocks, kKnnLanes, lds, s>>>(g, query, n_query, k, max_ring, max_radius, exclude_base, dist, idx, mean_dist);
  else
    knn_kernel<false><<<blocks, kKnnLanes, lds, s>>>(g, query, n_query, k, max_ring, max_radius, exclude_base, dist, idx, mean_dist);
  return check_launch("svs_cloud_knn");
}

size_t svs_cloud_outlier_workspace_bytes(void) { return sizeof(double) * 2 * kStatBlocks; }

int svs_cloud_outlier_stats(const double* mean_dist, int n, double* workspace, double* out, void* hip_stream) {
  if (!mean_dist || !workspace || !out || n < 0) { set_error("svs_cloud_outlier_stats: bad argument"); return SVS_EINVAL; }
  hipStream_t s = (hipStream_t)hip_stream;
  stats_partial_kernel<false><<<kStatBlocks, 256, 0, s>>>(mean_dist, n, nullptr, workspace);
  stats_final_kernel<false><<<1, 1, 0, s>>>(workspace, out);
  stats_partial_kernel<true><<<kStatBlocks, 256, 0, s>>>(mean_dist, n, out + 1, workspace);
  stats_final_kernel<true><<<1, 1, 0, s>>>(workspace, out);
  return check_launch("svs_cloud_outlier_stats");
}

int svs_cloud_outlier_mask(const double* mean_dist, int n, double threshold, uint8_t* keep, void* hip_stream) {
  if (!mean_dist || !keep || n < 0) { set_error("svs_cloud_outlier_mask: bad argument"); return SVS_EINVAL; }
  if (n == 0) return SVS_OK;
  outlier_mask_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(mean_dist, n, threshold, keep);
  return check_launch("svs_cloud_outlier_mask");
}

int svs_cloud_normals(const double* pts, int n, const int* idx, int k, int include_self, const int* view_index,
                      const double* centres, int n_views, float* normals, float* curvature, void* hip_stream) {
  if (!pts || !idx || !normals || n < 0) { set_error("svs_cloud_normals: bad argument"); return SVS_EINVAL; }
  if (k < 1 || k > kKnnMaxK) { set_error("svs_cloud_normals: k must be in [1,%d]", kKnnMaxK); return SVS_EINVAL; }
  if (centres && n_views < 1) { set_error("svs_cloud_normals: centres need n_views >= 1"); return SVS_EINVAL; }
  if (view_index && !centres) { set_error("svs_cloud_normals: view_index needs centres"); return SVS_EINVAL; }
  if (n == 0) return SVS_OK;
  normals_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(pts, n, idx, k, include_self, view_index, centres, n_views,
                                                                      normals, curvature);
  return check_launch("svs_cloud_normals");
}

}  // extern "C"
