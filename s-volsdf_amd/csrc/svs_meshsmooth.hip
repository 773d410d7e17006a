// Smoothing a triangle mesh on gfx950 (svs_hip/meshsmooth.py): the mesh's connectivity, Taubin's lambda|mu smoothing and
// bilateral normal filtering with a vertex update.  The rule is stated in include/svolsdf_hip.h ("a mesh made smoother")
// and restated in float64 numpy by tests/meshsmooth_oracle.py.
//
// Connectivity: the six directed pairs of every valid face are sorted by a << 32 | b (hipcub radix sort over the bits the
// vertex count needs); a run of equal keys is one neighbour and its length the edge's use; a scan of the run heads
// (svs_scan.h) gives the compressed rows.  The (vertex, face) pairs are sorted by vertex alone: the sort is stable, so a
// vertex's faces stay in ascending order.  Row starts are binary searches in the sorted keys.  The sorts, the run heads and
// the plain lower bound are svs_sorted_runs.h's, shared with the other geometry units; which face is valid, svs_mesh_face.h.
// Smoothing: gathers, one lane per vertex (or face) walking its own list left to right, 256-lane workgroups.  No float
// atomics and no cooperative path for long lists: either would change the order of the sums.  All float64, compiled with
// -ffp-contract=off.  Bound by the bytes of the positions, the rows and the frames: no matrix cores.
#include "svs_common.h"
#include "svs_mesh_face.h"
#include "svs_scan.h"
#include "svs_sorted_runs.h"

namespace svs {
namespace smooth {

typedef unsigned long long u64;

constexpr int kMaxFaces = 0x7fffffff / 6;                   // 6 * n_faces directed pairs are indexed by int

// ---- connectivity --------------------------------------------------------------------------------------------------------
// pair 6 f + 2 side + direction; a pair of an invalid face gets the key n_verts << 32, behind every valid one.
// cnt[3] counts the valid faces (an integer atomic: the order does not matter).
__global__ __launch_bounds__(256) void pair_keys_kernel(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                        int n_faces, u64* __restrict__ pair_keys, unsigned* __restrict__ corner_keys,
                                                        unsigned* __restrict__ corner_vals, uint8_t* __restrict__ face_valid,
                                                        int* __restrict__ flags, int* __restrict__ cnt) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  meshface::Face t;
  const bool ok = meshface::load_face(verts, n_verts, faces, f, t);
  const int (&i)[3] = t.i;
  face_valid[f] = ok ? 1 : 0;
  const u64 none = (u64)(unsigned)n_verts << 32;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = i[k], b = i[k == 2 ? 0 : k + 1];
    pair_keys[6 * (size_t)f + 2 * k] = ok ? ((u64)(unsigned)a << 32 | (unsigned)b) : none;
    pair_keys[6 * (size_t)f + 2 * k + 1] = ok ? ((u64)(unsigned)b << 32 | (unsigned)a) : none;
    corner_keys[3 * (size_t)f + k] = ok ? (unsigned)a : (unsigned)n_verts;
    corner_vals[3 * (size_t)f + k] = (unsigned)f;
    if (ok) atomicOr(&flags[a], SVS_MESH_USED);
  }
  if (ok) atomicAdd(&cnt[3], 1);
}

// one lane per run head: the neighbour, whether its edge is a boundary edge, the flags of the edge's ends, and (where a < b,
// once per edge) the counts.  The run's length is only needed up to 3.
__global__ __launch_bounds__(256) void emit_nbr_kernel(const u64* __restrict__ skeys, const uint8_t* __restrict__ head,
                                                       const int* __restrict__ offset, int n, int* __restrict__ nbr,
                                                       uint8_t* __restrict__ nbr_boundary, int* __restrict__ flags, int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !head[i]) return;
  const u64 k = skeys[i];
  int use = 1;
  if (i + 1 < n && skeys[i + 1] == k) use = (i + 2 < n && skeys[i + 2] == k) ? 3 : 2;
  const int a = (int)(k >> 32), b = (int)(k & 0xffffffffu);
  const int at = offset[i];
  nbr[at] = b;
  nbr_boundary[at] = use == 1 ? 1 : 0;
  if (use == 1) atomicOr(&flags[a], SVS_MESH_BOUNDARY);
  if (use > 2) atomicOr(&flags[a], SVS_MESH_NONMANIFOLD);
  if (a < b) {
    atomicAdd(&cnt[0], 1);
    if (use == 1) atomicAdd(&cnt[1], 1);
    if (use > 2) atomicAdd(&cnt[2], 1);
  }
}

// nbr_start[v] = the run heads before the first sorted pair whose source is >= v; v = 0 .. n_verts
__global__ __launch_bounds__(256) void nbr_start_kernel(const u64* __restrict__ skeys, const int* __restrict__ offset,
                                                        const int* __restrict__ n_heads, int n, int n_verts, int* __restrict__ nbr_start) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v > n_verts) return;
  const u64 key = (u64)(unsigned)v << 32;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] < key) lo = mid + 1; else hi = mid;
  }
  nbr_start[v] = lo < n ? offset[lo] : *n_heads;
}

// ---- Taubin ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void taubin_pass_kernel(const double* __restrict__ x, double* __restrict__ y, int n_verts,
                                                          const int* __restrict__ nbr_start, const int* __restrict__ nbr,
                                                          const uint8_t* __restrict__ nbr_boundary, const int* __restrict__ flags,
                                                          double s, int boundary) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_verts) return;
  const double x0 = x[3 * (size_t)v], x1 = x[3 * (size_t)v + 1], x2 = x[3 * (size_t)v + 2];
  double y0 = x0, y1 = x1, y2 = x2;
  const int fl = flags[v];
  const bool edge = (fl & SVS_MESH_BOUNDARY) != 0;
  if ((fl & SVS_MESH_USED) && !(edge && boundary == SVS_SMOOTH_FIXED)) {
    const bool along = edge && boundary == SVS_SMOOTH_CURVE;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    int count = 0;
    const int e = nbr_start[v + 1];
    for (int t = nbr_start[v]; t < e; ++t) {
      if (along && !nbr_boundary[t]) continue;
      const size_t j = 3 * (size_t)nbr[t];
      m0 += x[j]; m1 += x[j + 1]; m2 += x[j + 2];
      ++count;
    }
    if (count > 0) {
      const double c = (double)count;
      y0 = x0 + s * (m0 / c - x0);
      y1 = x1 + s * (m1 / c - x1);
      y2 = x2 + s * (m2 / c - x2);
    }
  }
  y[3 * (size_t)v] = y0; y[3 * (size_t)v + 1] = y1; y[3 * (size_t)v + 2] = y2;
}

// ---- bilateral normal filtering ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void face_frames_kernel(const double* __restrict__ x, const int* __restrict__ faces,
                                                          const uint8_t* __restrict__ face_valid, int n_faces, double* __restrict__ normals,
                                                          double* __restrict__ areas, double* __restrict__ centroids) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  double n0 = 0.0, n1 = 0.0, n2 = 0.0, area = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
  if (face_valid[f]) {
    const size_t a = 3 * (size_t)faces[3 * (size_t)f], b = 3 * (size_t)faces[3 * (size_t)f + 1], c = 3 * (size_t)faces[3 * (size_t)f + 2];
    const double p0[3] = {x[a], x[a + 1], x[a + 2]}, p1[3] = {x[b], x[b + 1], x[b + 2]}, p2[3] = {x[c], x[c + 1], x[c + 2]};
    const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const double vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double L = __builtin_sqrt(nx * nx + ny * ny + nz * nz);
    n0 = nx / L; n1 = ny / L; n2 = nz / L;
    area = 0.5 * L;
    c0 = ((p0[0] + p1[0]) + p2[0]) / 3.0; c1 = ((p0[1] + p1[1]) + p2[1]) / 3.0; c2 = ((p0[2] + p1[2]) + p2[2]) / 3.0;
  }
  normals[3 * (size_t)f] = n0; normals[3 * (size_t)f + 1] = n1; normals[3 * (size_t)f + 2] = n2;
  areas[f] = area;
  centroids[3 * (size_t)f] = c0; centroids[3 * (size_t)f + 1] = c1; centroids[3 * (size_t)f + 2] = c2;
}

__global__ __launch_bounds__(256) void normal_pass_kernel(const int* __restrict__ faces, const uint8_t* __restrict__ face_valid, int n_faces,
                                                          const int* __restrict__ face_start, const int* __restrict__ vert_face,
                                                          const double* __restrict__ areas, const double* __restrict__ centroids,
                                                          const double* __restrict__ n_in, double* __restrict__ n_out, double rs2, double rn2) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  const double n0 = n_in[3 * (size_t)f], n1 = n_in[3 * (size_t)f + 1], n2 = n_in[3 * (size_t)f + 2];
  double o0 = n0, o1 = n1, o2 = n2;
  if (face_valid[f]) {
    const double c0 = centroids[3 * (size_t)f], c1 = centroids[3 * (size_t)f + 1], c2 = centroids[3 * (size_t)f + 2];
    const double area = areas[f];
    double s0 = area * n0, s1 = area * n1, s2 = area * n2;
    for (int k = 0; k < 3; ++k) {
      const int v = faces[3 * (size_t)f + k];
      const int e = face_start[v + 1];
      for (int t = face_start[v]; t < e; ++t) {
        const int g = vert_face[t];
        if (g == f) continue;
        const double dx = centroids[3 * (size_t)g] - c0, dy = centroids[3 * (size_t)g + 1] - c1, dz = centroids[3 * (size_t)g + 2] - c2;
        const double g0 = n_in[3 * (size_t)g], g1 = n_in[3 * (size_t)g + 1], g2 = n_in[3 * (size_t)g + 2];
        const double qx = n0 - g0, qy = n1 - g1, qz = n2 - g2;
        const double d2 = dx * dx + dy * dy + dz * dz;
        const double q2 = qx * qx + qy * qy + qz * qz;
        const double a = 1.0 - d2 / rs2, b = 1.0 - q2 / rn2;
        if (!(a > 0.0 && b > 0.0)) continue;
        const double w = (areas[g] * (a * a)) * (b * b);
        s0 += w * g0; s1 += w * g1; s2 += w * g2;
      }
    }
    const double Ls = __builtin_sqrt(s0 * s0 + s1 * s1 + s2 * s2);
    if (finite_f64(Ls) && Ls > 0.0) { o0 = s0 / Ls; o1 = s1 / Ls; o2 = s2 / Ls; }
  }
  n_out[3 * (size_t)f] = o0; n_out[3 * (size_t)f + 1] = o1; n_out[3 * (size_t)f + 2] = o2;
}

// the centroid of a face is recomputed from the pass's input positions where it is needed (measured against a separate
// centroid pass: NOTES/meshsmooth.md)
__global__ __launch_bounds__(256) void vertex_pass_kernel(const double* __restrict__ x, double* __restrict__ y, int n_verts,
                                                          const int* __restrict__ faces, const int* __restrict__ face_start,
                                                          const int* __restrict__ vert_face, const int* __restrict__ flags,
                                                          const double* __restrict__ normals, int boundary) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_verts) return;
  const double x0 = x[3 * (size_t)v], x1 = x[3 * (size_t)v + 1], x2 = x[3 * (size_t)v + 2];
  double y0 = x0, y1 = x1, y2 = x2;
  const int fl = flags[v];
  if ((fl & SVS_MESH_USED) && !((fl & SVS_MESH_BOUNDARY) && boundary == SVS_SMOOTH_FIXED)) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const int b = face_start[v], e = face_start[v + 1];
    for (int t = b; t < e; ++t) {
      const size_t f = (size_t)vert_face[t];
      const size_t i = 3 * (size_t)faces[3 * f], j = 3 * (size_t)faces[3 * f + 1], k = 3 * (size_t)faces[3 * f + 2];
      const double d0 = ((x[i] + x[j]) + x[k]) / 3.0 - x0;
      const double d1 = ((x[i + 1] + x[j + 1]) + x[k + 1]) / 3.0 - x1;
      const double d2 = ((x[i + 2] + x[j + 2]) + x[k + 2]) / 3.0 - x2;
      const double n0 = normals[3 * f], n1 = normals[3 * f + 1], n2 = normals[3 * f + 2];
      const double w = (n0 * d0 + n1 * d1) + n2 * d2;
      a0 += n0 * w; a1 += n1 * w; a2 += n2 * w;
    }
    if (e > b) {
      const double c = (double)(e - b);
      y0 = x0 + a0 / c; y1 = x1 + a1 / c; y2 = x2 + a2 / c;
    }
  }
  y[3 * (size_t)v] = y0; y[3 * (size_t)v + 1] = y1; y[3 * (size_t)v + 2] = y2;
}

}  // namespace smooth
}  // namespace svs

using namespace svs;
using namespace svs::smooth;
using namespace svs::ws;

namespace {

struct Layout { size_t pkeys, spkeys, head, offset, ckeys, sckeys, cvals, cnt, sort_tmp, sort_size, total; };
Layout layout(int n_faces) {
  Layout L;
  Bump b;
  const size_t np = 6 * (size_t)n_faces, nc = 3 * (size_t)n_faces;
  L.pkeys = b.take(8 * np); L.spkeys = b.take(8 * np); L.head = b.take(np); L.offset = b.take(4 * np);
  L.ckeys = b.take(4 * nc); L.sckeys = b.take(4 * nc); L.cvals = b.take(4 * nc); L.cnt = b.take(8 * sizeof(int));
  // one scratch serves both sorts: the directed pairs (keys alone) and the corners (with their faces)
  const size_t pairs = runs::sort_scratch_bytes<u64, false>(np), corners = runs::sort_scratch_bytes<unsigned, true>(nc);
  L.sort_size = pairs > corners ? pairs : corners;
  L.sort_tmp = b.take(L.sort_size);
  L.total = b.o;
  return L;
}

// the result of an odd number of passes lies in tmp: bring it home
int settle(const char* name, double* x, const double* cur, size_t doubles, hipStream_t s) {
  if (cur != x) {
    hipError_t e = hipMemcpyAsync(x, cur, sizeof(double) * doubles, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return hip_fail(name, e);
  }
  return check_launch(name);
}

}  // namespace

extern "C" {

size_t svs_mesh_smooth_workspace_bytes(int n_verts, int n_faces) {
  (void)n_verts;
  if (n_faces < 0) n_faces = 0;
  if (n_faces > kMaxFaces) n_faces = kMaxFaces;
  return layout(n_faces).total + 256;
}

int svs_mesh_adjacency(const float* verts, int n_verts, const int* faces, int n_faces, void* workspace, int* nbr_start, int* nbr,
                       uint8_t* nbr_boundary, int* face_start, int* vert_face, uint8_t* face_valid, int* flags, int* counts,
                       void* hip_stream) {
  const char* name = "svs_mesh_adjacency";
  int rc = check_counts(name, n_verts, n_faces, kMaxFaces);
  if (rc) return rc;
  if (!counts || !nbr_start || !face_start || (n_verts > 0 && (!verts || !flags)) ||
      (n_faces > 0 && (!faces || !workspace || !nbr || !nbr_boundary || !vert_face || !face_valid)))
    return null_pointer(name);
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  hipStream_t s = (hipStream_t)hip_stream;
  hipError_t e = hipMemsetAsync(nbr_start, 0, sizeof(int) * ((size_t)n_verts + 1), s);
  if (e == hipSuccess) e = hipMemsetAsync(face_start, 0, sizeof(int) * ((size_t)n_verts + 1), s);
  if (e == hipSuccess && n_verts > 0) e = hipMemsetAsync(flags, 0, sizeof(int) * (size_t)n_verts, s);
  if (e == hipSuccess && n_faces > 0) e = hipMemsetAsync(face_valid, 0, (size_t)n_faces, s);
  if (e != hipSuccess) return hip_fail(name, e);
  if (n_verts == 0 || n_faces == 0) {
    e = hipStreamSynchronize(s);
    return e != hipSuccess ? hip_fail(name, e) : SVS_OK;
  }
  const Layout L = layout(n_faces);
  char* base = aligned(workspace);
  u64* pkeys = (u64*)(base + L.pkeys); u64* spkeys = (u64*)(base + L.spkeys);
  uint8_t* head = (uint8_t*)(base + L.head); int* offset = (int*)(base + L.offset);
  unsigned* ckeys = (unsigned*)(base + L.ckeys); unsigned* sckeys = (unsigned*)(base + L.sckeys); unsigned* cvals = (unsigned*)(base + L.cvals);
  int* cnt = (int*)(base + L.cnt);                           // edges, boundary, non-manifold, valid faces, run heads
  const int n_pairs = 6 * n_faces, n_corners = 3 * n_faces;
  const int bits = runs::bit_length((unsigned)n_verts);
  const u64 none = (u64)(unsigned)n_verts << 32;
  e = hipMemsetAsync(cnt, 0, 8 * sizeof(int), s);
  if (e != hipSuccess) return hip_fail(name, e);
  pair_keys_kernel<<<(n_faces + 255) / 256, 256, 0, s>>>(verts, n_verts, faces, n_faces, pkeys, ckeys, cvals, face_valid, flags, cnt);
  rc = runs::sort_keys(name, base + L.sort_tmp, L.sort_size, pkeys, spkeys, n_pairs, 32 + bits, s);
  if (rc) return rc;
  rc = runs::sort_pairs(name, base + L.sort_tmp, L.sort_size, ckeys, sckeys, cvals, (unsigned*)vert_face, n_corners, bits, s);
  if (rc) return rc;
  runs::run_heads_kernel<u64><<<(n_pairs + 255) / 256, 256, 0, s>>>(spkeys, n_pairs, none, head);
  scan::mask_offsets(head, n_pairs, offset, cnt + 4, s);
  emit_nbr_kernel<<<(n_pairs + 255) / 256, 256, 0, s>>>(spkeys, head, offset, n_pairs, nbr, nbr_boundary, flags, cnt);
  nbr_start_kernel<<<(n_verts + 1 + 255) / 256, 256, 0, s>>>(spkeys, offset, cnt + 4, n_pairs, n_verts, nbr_start);
  runs::lower_bound_kernel<unsigned><<<(n_verts + 1 + 255) / 256, 256, 0, s>>>(sckeys, n_corners, n_verts, face_start);
  rc = check_launch(name);
  if (rc) return rc;
  int host[4] = {0, 0, 0, 0};
  rc = download(name, cnt, 4, host, s);
  if (rc) return rc;
  for (int k = 0; k < 4; ++k) counts[k] = host[k];
  return SVS_OK;
}

int svs_mesh_taubin(double* x, double* tmp, int n_verts, const int* nbr_start, const int* nbr, const uint8_t* nbr_boundary,
                    const int* flags, int iters, double lambda, double mu, int boundary, void* hip_stream) {
  const char* name = "svs_mesh_taubin";
  if (n_verts < 0) { set_error("%s: negative count", name); return SVS_ESHAPE; }
  // nbr and nbr_boundary may be null for a mesh without an edge: they are then never read
  if (n_verts > 0 && (!x || !tmp || !nbr_start || !flags)) return null_pointer(name);
  if (iters < 0) { set_error("%s: iters must not be negative", name); return SVS_EINVAL; }
  if (!(lambda > 0.0 && lambda <= 1.0)) { set_error("%s: lambda must lie in (0,1]", name); return SVS_EINVAL; }
  if (!(mu >= -2.0 && mu <= 0.0)) { set_error("%s: mu must lie in [-2,0]", name); return SVS_EINVAL; }
  if (boundary != SVS_SMOOTH_FIXED && boundary != SVS_SMOOTH_CURVE && boundary != SVS_SMOOTH_FREE) {
    set_error("%s: boundary must be SVS_SMOOTH_FIXED, SVS_SMOOTH_CURVE or SVS_SMOOTH_FREE", name); return SVS_EINVAL;
  }
  if (n_verts == 0 || iters == 0) return SVS_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  const int nb = (n_verts + 255) / 256;
  double* cur = x;
  double* nxt = tmp;
  for (int it = 0; it < iters; ++it)
    for (int half = 0; half < 2; ++half) {
      if (half == 1 && mu == 0.0) continue;
      taubin_pass_kernel<<<nb, 256, 0, s>>>(cur, nxt, n_verts, nbr_start, nbr, nbr_boundary, flags, half ? mu : lambda, boundary);
      double* w = cur; cur = nxt; nxt = w;
    }
  return settle(name, x, cur, 3 * (size_t)n_verts, s);
}

int svs_mesh_face_frames(const double* x, int n_verts, const int* faces, const uint8_t* face_valid, int n_faces, double* normals,
                         double* areas, double* centroids, void* hip_stream) {
  const char* name = "svs_mesh_face_frames";
  int rc = check_counts(name, n_verts, n_faces, kMaxFaces);
  if (rc) return rc;
  if (n_faces > 0 && (!faces || !face_valid || !normals || !areas || !centroids || (n_verts > 0 && !x))) return null_pointer(name);
  if (n_faces == 0) return SVS_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  if (n_verts == 0) {                                        // no face can be valid
    hipError_t e = hipMemsetAsync(normals, 0, sizeof(double) * 3 * (size_t)n_faces, s);
    if (e == hipSuccess) e = hipMemsetAsync(areas, 0, sizeof(double) * (size_t)n_faces, s);
    if (e == hipSuccess) e = hipMemsetAsync(centroids, 0, sizeof(double) * 3 * (size_t)n_faces, s);
    return e != hipSuccess ? hip_fail(name, e) : SVS_OK;
  }
  face_frames_kernel<<<(n_faces + 255) / 256, 256, 0, s>>>(x, faces, face_valid, n_faces, normals, areas, centroids);
  return check_launch(name);
}

int svs_mesh_normal_filter(const int* faces, const uint8_t* face_valid, int n_faces, int n_verts, const int* face_start,
                           const int* vert_face, const double* areas, const double* centroids, double* normals, double* tmp, int iters,
                           double rs, double rn, void* hip_stream) {
  const char* name = "svs_mesh_normal_filter";
  int rc = check_counts(name, n_verts, n_faces, kMaxFaces);
  if (rc) return rc;
  // vert_face may be null for a mesh without a valid face: it is then never read
  if (n_faces > 0 && (!faces || !face_valid || !face_start || !areas || !centroids || !normals || !tmp)) return null_pointer(name);
  if (iters < 0) { set_error("%s: iters must not be negative", name); return SVS_EINVAL; }
  if (!(rs > 0.0) || !finite_f64(rs)) { set_error("%s: rs must be positive and finite", name); return SVS_EINVAL; }
  if (!(rn > 0.0 && rn <= 2.0)) { set_error("%s: rn must lie in (0,2]", name); return SVS_EINVAL; }
  if (n_faces == 0 || iters == 0) return SVS_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  const int nb = (n_faces + 255) / 256;
  double* cur = normals;
  double* nxt = tmp;
  for (int it = 0; it < iters; ++it) {
    normal_pass_kernel<<<nb, 256, 0, s>>>(faces, face_valid, n_faces, face_start, vert_face, areas, centroids, cur, nxt, rs * rs, rn * rn);
    double* w = cur; cur = nxt; nxt = w;
  }
  return settle(name, normals, cur, 3 * (size_t)n_faces, s);
}

int svs_mesh_vertex_update(double* x, double* tmp, int n_verts, const int* faces, int n_faces, const int* face_start,
                           const int* vert_face, const int* flags, const double* normals, int iters, int boundary, void* hip_stream) {
  const char* name = "svs_mesh_vertex_update";
  int rc = check_counts(name, n_verts, n_faces, kMaxFaces);
  if (rc) return rc;
  // vert_face may be null for a mesh without a valid face: it is then never read
  if (n_verts > 0 && (!x || !tmp || !face_start || !flags || (n_faces > 0 && (!faces || !normals)))) return null_pointer(name);
  if (iters < 0) { set_error("%s: iters must not be negative", name); return SVS_EINVAL; }
  if (boundary != SVS_SMOOTH_FIXED && boundary != SVS_SMOOTH_FREE) {
    set_error("%s: boundary must be SVS_SMOOTH_FIXED or SVS_SMOOTH_FREE", name); return SVS_EINVAL;
  }
  if (n_verts == 0 || n_faces == 0 || iters == 0) return SVS_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  const int nb = (n_verts + 255) / 256;
  double* cur = x;
  double* nxt = tmp;
  for (int it = 0; it < iters; ++it) {
    vertex_pass_kernel<<<nb, 256, 0, s>>>(cur, nxt, n_verts, faces, face_start, vert_face, flags, normals, boundary);
    double* w = cur; cur = nxt; nxt = w;
  }
  return settle(name, x, cur, 3 * (size_t)n_verts, s);
}

}  // extern "C"
