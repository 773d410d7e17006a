// Simplifying a triangle mesh on gfx950 by vertex clustering with quadric error metrics (svs_hip/meshsimplify.py; after
// Lindstrom, "Out-of-core simplification of large polygonal models", 2000).  The rule is stated in
// include/svolsdf_hip.h and restated in float64 numpy by tests/meshsimplify_oracle.py.
//
// No priority queue and no serial collapses: the vertices used by valid faces are sorted by the key of their cell
// (svs_cloud_grid.h), the occupied cells ranked, every (face, corner) pair sorted by the rank of its corner's cell, and
// the quadric of a cell summed in one fixed order -- segments of 64 consecutive pairs, one lane per segment, then one lane
// per cell over its segment sums -- so that no float atomic is needed and every run gives the same bytes.  The 3x3
// eigenproblem per cell is the cyclic Jacobi of svs_jacobi3.h.  Faces are re-indexed, the collapsed ones dropped, and
// duplicates (the same set of three cells) removed by a sort of the packed triple: the first face in input order stays.
// All float64, compiled with -ffp-contract=off.  Plain wave64 kernels of 256 threads, sums in registers; the work is bound
// by the bytes the sorts and the gathers move, not by arithmetic: no matrix cores.
#include "svs_cloud_grid.h"
#include "svs_common.h"
#include "svs_jacobi3.h"
#include "svs_mesh_face.h"
#include "svs_scan.h"
#include "svs_sorted_runs.h"

namespace svs {
namespace simplify {

using cloud::cell_coord;
using cloud::cell_key;
using cloud::kCellBits;
using cloud::kEmpty;
using cloud::u64;
using meshface::Face;
using meshface::load_face;

constexpr int kSegment = 64;                                // pairs per segment of a cell's run
constexpr int kMaxCells = 1 << kCellBits;                   // occupied cells per call: three ranks pack into one key
constexpr int kMaxFaces = 0x7fffffff / 3;                   // 3 * n_faces pairs are indexed by int

struct Cells { double ox, oy, oz, inv_h, h; };

// ---- cells ---------------------------------------------------------------------------------------------------------------
// every lane that marks a vertex stores the same byte: the races are between equal values
__global__ __launch_bounds__(256) void mark_used_kernel(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                        int n_faces, uint8_t* __restrict__ used) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  Face t;
  if (!load_face(verts, n_verts, faces, f, t)) return;
  used[t.i[0]] = 1; used[t.i[1]] = 1; used[t.i[2]] = 1;
}

__global__ __launch_bounds__(256) void vert_keys_kernel(const float* __restrict__ verts, int n_verts, const uint8_t* __restrict__ used,
                                                        Cells g, u64* __restrict__ keys, unsigned* __restrict__ idx) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_verts) return;
  u64 k = kEmpty;
  if (used[v])
    k = cell_key(cell_coord((double)verts[3 * (size_t)v], g.ox, g.inv_h), cell_coord((double)verts[3 * (size_t)v + 1], g.oy, g.inv_h),
                 cell_coord((double)verts[3 * (size_t)v + 2], g.oz, g.inv_h));
  keys[v] = k;
  idx[v] = (unsigned)v;
}

// offset[i] = heads before sorted position i: the rank of i's cell is offset[i] + head[i] - 1
__global__ __launch_bounds__(256) void vert_rank_kernel(const u64* __restrict__ skeys, const unsigned* __restrict__ sidx,
                                                        const uint8_t* __restrict__ head, const int* __restrict__ offset, int n,
                                                        int* __restrict__ vert_cell) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  vert_cell[sidx[i]] = skeys[i] == kEmpty ? -1 : offset[i] + (int)head[i] - 1;
}

// ---- per-cell sums and the solve -----------------------------------------------------------------------------------------
// pair p = 3 f + k; key = the rank of corner k's cell, n_cells for a pair that does not count (sorted behind every cell)
__global__ __launch_bounds__(256) void pair_keys_kernel(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                        int n_faces, const int* __restrict__ vert_cell, int n_cells,
                                                        unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  Face t;
  const bool ok = load_face(verts, n_verts, faces, f, t);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    unsigned key = (unsigned)n_cells;
    if (ok) {
      const int r = vert_cell[t.i[k]];
      if ((unsigned)r < (unsigned)n_cells) key = (unsigned)r;
    }
    keys[3 * (size_t)f + k] = key;
    vals[3 * (size_t)f + k] = 3u * (unsigned)f + (unsigned)k;
  }
}

// begin[r], r = 0 .. n_cells, from runs::lower_bound_kernel: cell r's run is [begin[r], begin[r + 1])
__global__ __launch_bounds__(256) void seg_flags_kernel(const unsigned* __restrict__ skeys, int n_pairs, int n_cells,
                                                        const int* __restrict__ begin, uint8_t* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pairs) return;
  const unsigned k = skeys[i];
  flag[i] = (k < (unsigned)n_cells && ((i - begin[k]) & (kSegment - 1)) == 0) ? 1 : 0;
}

struct Partial {                                            // 128 bytes
  double s[13];                                             // A (xx xy xz yy yz zz), b, e, m
  long long c[3];                                           // colour codes
};

__device__ __forceinline__ void zero(Partial& q) {
#pragma unroll
  for (int j = 0; j < 13; ++j) q.s[j] = 0.0;
  q.c[0] = q.c[1] = q.c[2] = 0;
}

__device__ __forceinline__ void cell_centre(const Cells& g, const double (&p)[3], double (&c)[3]) {
  c[0] = g.ox + ((double)cell_coord(p[0], g.ox, g.inv_h) + 0.5) * g.h;
  c[1] = g.oy + ((double)cell_coord(p[1], g.oy, g.inv_h) + 0.5) * g.h;
  c[2] = g.oz + ((double)cell_coord(p[2], g.oz, g.inv_h) + 0.5) * g.h;
}

// one lane per segment: its pairs left to right from zero
__global__ __launch_bounds__(256) void seg_sum_kernel(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                      const uint8_t* __restrict__ colors, Cells g, const unsigned* __restrict__ skeys,
                                                      const unsigned* __restrict__ svals, const int* __restrict__ begin,
                                                      const int* __restrict__ seg_start, const int* __restrict__ n_segs, int max_segs,
                                                      Partial* __restrict__ part) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= max_segs || s >= *n_segs) return;
  const int i0 = seg_start[s];
  const int cell_end = begin[skeys[i0] + 1];
  const int i1 = i0 + kSegment < cell_end ? i0 + kSegment : cell_end;
  Partial q;
  zero(q);
  for (int i = i0; i < i1; ++i) {
    const unsigned p = svals[i];
    const int f = (int)(p / 3u), k = (int)(p - 3u * (unsigned)f);
    Face t;
    if (!load_face(verts, n_verts, faces, f, t)) continue;   // (never: the pair was valid when it got its key)
    const double (&pk)[3] = k == 0 ? t.p[0] : (k == 1 ? t.p[1] : t.p[2]);
    const int vk = k == 0 ? t.i[0] : (k == 1 ? t.i[1] : t.i[2]);
    double c[3];
    cell_centre(g, pk, c);
    const double d = -(t.n[0] * (t.p[0][0] - c[0]) + t.n[1] * (t.p[0][1] - c[1]) + t.n[2] * (t.p[0][2] - c[2]));
    q.s[0] += t.n[0] * t.n[0] / t.L; q.s[1] += t.n[0] * t.n[1] / t.L; q.s[2] += t.n[0] * t.n[2] / t.L;
    q.s[3] += t.n[1] * t.n[1] / t.L; q.s[4] += t.n[1] * t.n[2] / t.L; q.s[5] += t.n[2] * t.n[2] / t.L;
    q.s[6] += t.n[0] * d / t.L; q.s[7] += t.n[1] * d / t.L; q.s[8] += t.n[2] * d / t.L;
    q.s[9] += d * d / t.L;
    q.s[10] += pk[0] - c[0]; q.s[11] += pk[1] - c[1]; q.s[12] += pk[2] - c[2];
    if (colors) {
      q.c[0] += colors[3 * (size_t)vk]; q.c[1] += colors[3 * (size_t)vk + 1]; q.c[2] += colors[3 * (size_t)vk + 2];
    }
  }
  part[s] = q;
}

// one lane per cell: its segment sums left to right from zero, then the solve
__global__ __launch_bounds__(256) void cell_solve_kernel(const float* __restrict__ verts, const int* __restrict__ faces, Cells g, double tol,
                                                         const unsigned* __restrict__ svals, const int* __restrict__ begin,
                                                         const int* __restrict__ offset, int n_cells, int max_segs,
                                                         const Partial* __restrict__ part, float* __restrict__ out_verts,
                                                         uint8_t* __restrict__ out_colors, int* __restrict__ info, double* __restrict__ err) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_cells) return;
  const int b0 = begin[r], count = begin[r + 1] - b0;
  float ox = 0.0f, oy = 0.0f, oz = 0.0f;
  int code = 4;
  double e_out = 0.0;
  long long col[3] = {0, 0, 0};
  if (count > 0) {                                           // (always, for the vert_cell svs_mesh_cluster_cells wrote)
    Partial q;
    zero(q);
    const int s0 = offset[b0], n_seg = (count + kSegment - 1) / kSegment;
    for (int s = s0; s < s0 + n_seg && s < max_segs; ++s) {
      const Partial& w = part[s];
#pragma unroll
      for (int j = 0; j < 13; ++j) q.s[j] += w.s[j];
      q.c[0] += w.c[0]; q.c[1] += w.c[1]; q.c[2] += w.c[2];
    }
    // the cell's centre, from the corner of its first pair
    const unsigned p = svals[b0];
    const int v0 = faces[p];                                 // faces[3 f + k]
    const double pk[3] = {(double)verts[3 * (size_t)v0], (double)verts[3 * (size_t)v0 + 1], (double)verts[3 * (size_t)v0 + 2]};
    double c[3];
    cell_centre(g, pk, c);
    const double A[3][3] = {{q.s[0], q.s[1], q.s[2]}, {q.s[1], q.s[3], q.s[4]}, {q.s[2], q.s[4], q.s[5]}};
    const double b[3] = {q.s[6], q.s[7], q.s[8]};
    double a[3][3] = {{A[0][0], A[0][1], A[0][2]}, {A[1][0], A[1][1], A[1][2]}, {A[2][0], A[2][1], A[2][2]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    jacobi_sweeps(a, v);
    const double lam[3] = {a[0][0], a[1][1], a[2][2]};
    double lmax = lam[0];
    lmax = lam[1] > lmax ? lam[1] : lmax;
    lmax = lam[2] > lmax ? lam[2] : lmax;
    const double cnt = (double)count;
    const double mean[3] = {q.s[10] / cnt, q.s[11] / cnt, q.s[12] / cnt};
    double gk[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) gk[i] = -b[i] - (A[i][0] * mean[0] + A[i][1] * mean[1] + A[i][2] * mean[2]);
    double x[3] = {mean[0], mean[1], mean[2]};
    int rank = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (lam[i] > tol * lmax) {
        const double w = (v[0][i] * gk[0] + v[1][i] * gk[1] + v[2][i] * gk[2]) / lam[i];
        x[0] += v[0][i] * w; x[1] += v[1][i] * w; x[2] += v[2][i] * w;
        ++rank;
      }
    }
    bool fallback = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) fallback = fallback || !finite_f64(x[i]) || __builtin_fabs(x[i]) > g.h;
    if (fallback) { x[0] = mean[0]; x[1] = mean[1]; x[2] = mean[2]; }
    double xAx = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) xAx += x[i] * (A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2]);
    e_out = xAx + 2.0 * (b[0] * x[0] + b[1] * x[1] + b[2] * x[2]) + q.s[9];
    ox = (float)(c[0] + x[0]); oy = (float)(c[1] + x[1]); oz = (float)(c[2] + x[2]);
    code = rank | (fallback ? 4 : 0);
#pragma unroll
    for (int i = 0; i < 3; ++i) col[i] = (2 * q.c[i] + count) / (2 * (long long)count);
  }
  out_verts[3 * (size_t)r] = ox; out_verts[3 * (size_t)r + 1] = oy; out_verts[3 * (size_t)r + 2] = oz;
  if (out_colors) {
    out_colors[3 * (size_t)r] = (uint8_t)col[0]; out_colors[3 * (size_t)r + 1] = (uint8_t)col[1]; out_colors[3 * (size_t)r + 2] = (uint8_t)col[2];
  }
  info[r] = code;
  err[r] = e_out;
}

// ---- faces ---------------------------------------------------------------------------------------------------------------
// key = the three ranks ascending, 21 bits each (lowest rank in the lowest bits); drop = n_cells << 42 sorts behind every key
__global__ __launch_bounds__(256) void face_keys_kernel(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                        int n_faces, const int* __restrict__ vert_cell, int n_cells,
                                                        u64* __restrict__ keys, unsigned* __restrict__ idx) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  u64 key = (u64)n_cells << (2 * kCellBits);
  Face t;
  if (load_face(verts, n_verts, faces, f, t)) {
    int a = vert_cell[t.i[0]], b = vert_cell[t.i[1]], c = vert_cell[t.i[2]];
    if ((unsigned)a < (unsigned)n_cells && (unsigned)b < (unsigned)n_cells && (unsigned)c < (unsigned)n_cells && a != b && b != c && a != c) {
      int w;
      if (a > b) { w = a; a = b; b = w; }
      if (b > c) { w = b; b = c; c = w; }
      if (a > b) { w = a; a = b; b = w; }
      key = (u64)a | ((u64)b << kCellBits) | ((u64)c << (2 * kCellBits));
    }
  }
  keys[f] = key;
  idx[f] = (unsigned)f;
}

// the sort is stable: the head of a run of equal keys is the face with the lowest input index.  Every face is written once.
__global__ __launch_bounds__(256) void face_keep_kernel(const u64* __restrict__ skeys, const unsigned* __restrict__ sidx, int n, u64 drop,
                                                        uint8_t* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 k = skeys[i];
  keep[sidx[i]] = (k != drop && (i == 0 || skeys[i - 1] != k)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void face_emit_kernel(const int* __restrict__ faces, int n_faces, const int* __restrict__ vert_cell,
                                                        const uint8_t* __restrict__ keep, const int* __restrict__ offsets,
                                                        int* __restrict__ out_faces) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces || !keep[f]) return;
  const size_t o = 3 * (size_t)offsets[f];
#pragma unroll
  for (int k = 0; k < 3; ++k) out_faces[o + k] = vert_cell[faces[3 * (size_t)f + k]];
}

}  // namespace simplify
}  // namespace svs

using namespace svs;
using namespace svs::simplify;
using namespace svs::ws;

namespace {

int cell_bound(int n_verts) { return n_verts < kMaxCells ? n_verts : kMaxCells; }

struct CellsLayout { size_t used, keys, skeys, idx, sidx, head, offset, count, sort_tmp, sort_size, total; };
CellsLayout cells_layout(int n_verts) {
  CellsLayout L;
  Bump b;
  const size_t n = (size_t)n_verts;
  L.used = b.take(n); L.keys = b.take(8 * n); L.skeys = b.take(8 * n); L.idx = b.take(4 * n); L.sidx = b.take(4 * n);
  L.head = b.take(n); L.offset = b.take(4 * n); L.count = b.take(sizeof(int));
  L.sort_size = runs::sort_scratch_bytes<u64, true>(n); L.sort_tmp = b.take(L.sort_size);
  L.total = b.o;
  return L;
}

struct SolveLayout { size_t keys, skeys, vals, svals, begin, flag, offset, count, seg_start, part, sort_tmp, sort_size, total; int max_segs; };
SolveLayout solve_layout(int n_verts, int n_faces) {
  SolveLayout L;
  Bump b;
  const size_t np = 3 * (size_t)n_faces, nc = (size_t)cell_bound(n_verts);
  // a cell of m pairs has ceil(m / 64) <= m / 64 + 1 segments
  const size_t segs = np / kSegment + nc + 1;
  L.max_segs = (int)(segs < 0x7fffffff ? segs : 0x7fffffff);
  L.keys = b.take(4 * np); L.skeys = b.take(4 * np); L.vals = b.take(4 * np); L.svals = b.take(4 * np);
  L.begin = b.take(4 * (nc + 2)); L.flag = b.take(np); L.offset = b.take(4 * np); L.count = b.take(sizeof(int));
  L.seg_start = b.take(4 * segs); L.part = b.take(sizeof(Partial) * segs);
  L.sort_size = runs::sort_scratch_bytes<unsigned, true>(np); L.sort_tmp = b.take(L.sort_size);
  L.total = b.o;
  return L;
}

struct FacesLayout { size_t keys, skeys, idx, sidx, sort_tmp, sort_size, total; };
FacesLayout faces_layout(int n_faces) {
  FacesLayout L;
  Bump b;
  const size_t n = (size_t)n_faces;
  L.keys = b.take(8 * n); L.skeys = b.take(8 * n); L.idx = b.take(4 * n); L.sidx = b.take(4 * n);
  L.sort_size = runs::sort_scratch_bytes<u64, true>(n); L.sort_tmp = b.take(L.sort_size);
  L.total = b.o;
  return L;
}

// the cell of every entry: the origin's pointer, then the cell size, then the origin's values
int check_cell(const char* name, const double* origin, double h) {
  if (!origin) return null_pointer(name);
  const int rc = check_spacing(name, h, "cell size");
  return rc ? rc : check_origin(name, origin);
}

}  // namespace

extern "C" {

size_t svs_mesh_cluster_workspace_bytes(int n_verts, int n_faces) {
  if (n_verts < 0) n_verts = 0;
  if (n_faces < 0) n_faces = 0;
  if (n_faces > kMaxFaces) n_faces = kMaxFaces;
  size_t t = cells_layout(n_verts).total;
  const size_t s = solve_layout(n_verts, n_faces).total, f = faces_layout(n_faces).total;
  t = s > t ? s : t;
  t = f > t ? f : t;
  return t + 256;
}

int svs_mesh_cluster_cells(const float* verts, int n_verts, const int* faces, int n_faces, const double* origin, double h,
                           void* workspace, int* vert_cell, int* n_cells, void* hip_stream) {
  const char* name = "svs_mesh_cluster_cells";
  int rc = check_counts(name, n_verts, n_faces, kMaxFaces);
  if (rc) return rc;
  if (!n_cells || (n_verts > 0 && (!verts || !vert_cell || !workspace)) || (n_faces > 0 && !faces)) return null_pointer(name);
  rc = check_cell(name, origin, h);
  if (rc) return rc;
  *n_cells = 0;
  if (n_verts == 0) return SVS_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  hipError_t e;
  if (n_faces == 0) {
    e = hipMemsetAsync(vert_cell, 0xff, sizeof(int) * (size_t)n_verts, s);
    return e != hipSuccess ? hip_fail(name, e) : SVS_OK;
  }
  const CellsLayout L = cells_layout(n_verts);
  char* base = aligned(workspace);
  uint8_t* used = (uint8_t*)(base + L.used); uint8_t* head = (uint8_t*)(base + L.head);
  u64* keys = (u64*)(base + L.keys); u64* skeys = (u64*)(base + L.skeys);
  unsigned* idx = (unsigned*)(base + L.idx); unsigned* sidx = (unsigned*)(base + L.sidx);
  int* offset = (int*)(base + L.offset); int* count = (int*)(base + L.count);
  const Cells g = {origin[0], origin[1], origin[2], 1.0 / h, h};
  const int nb = (n_verts + 255) / 256;
  e = hipMemsetAsync(used, 0, (size_t)n_verts, s);
  if (e != hipSuccess) return hip_fail(name, e);
  mark_used_kernel<<<(n_faces + 255) / 256, 256, 0, s>>>(verts, n_verts, faces, n_faces, used);
  vert_keys_kernel<<<nb, 256, 0, s>>>(verts, n_verts, used, g, keys, idx);
  rc = runs::sort_pairs(name, base + L.sort_tmp, L.sort_size, keys, skeys, idx, sidx, n_verts, 64, s);
  if (rc) return rc;
  runs::run_heads_kernel<u64><<<nb, 256, 0, s>>>(skeys, n_verts, kEmpty, head);
  scan::mask_offsets(head, n_verts, offset, count, s);
  vert_rank_kernel<<<nb, 256, 0, s>>>(skeys, sidx, head, offset, n_verts, vert_cell);
  rc = check_launch(name);
  if (rc) return rc;
  int cells = 0;
  rc = download(name, count, 1, &cells, s);
  if (rc) return rc;
  *n_cells = cells;
  if (cells > kMaxCells) {
    set_error("%s: %d occupied cells, at most %d in one call (use a larger cell)", name, cells, kMaxCells); return SVS_ESHAPE;
  }
  return SVS_OK;
}

int svs_mesh_cluster_solve(const float* verts, int n_verts, const int* faces, int n_faces, const uint8_t* colors,
                           const double* origin, double h, double tol, const int* vert_cell, int n_cells, void* workspace,
                           float* out_verts, uint8_t* out_colors, int* info, double* err, void* hip_stream) {
  const char* name = "svs_mesh_cluster_solve";
  int rc = check_counts(name, n_verts, n_faces, kMaxFaces);
  if (rc) return rc;
  if (n_cells < 0) { set_error("%s: negative count", name); return SVS_ESHAPE; }
  if (n_cells > kMaxCells || n_cells > n_verts) {
    set_error("%s: %d cells, at most %d in one call and no more than the vertices", name, n_cells, kMaxCells); return SVS_ESHAPE;
  }
  if (n_cells > 0 && (!verts || !faces || !vert_cell || !workspace || !out_verts || !info || !err || (!colors != !out_colors))) {
    set_error("%s: bad argument (null pointer, or colours without their output)", name); return SVS_EINVAL;
  }
  rc = check_cell(name, origin, h);
  if (rc) return rc;
  if (!(tol > 0.0 && tol < 1.0)) { set_error("%s: tol must lie in (0,1)", name); return SVS_EINVAL; }
  if (n_cells == 0) return SVS_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  const SolveLayout L = solve_layout(n_verts, n_faces);
  char* base = aligned(workspace);
  unsigned* keys = (unsigned*)(base + L.keys); unsigned* skeys = (unsigned*)(base + L.skeys);
  unsigned* vals = (unsigned*)(base + L.vals); unsigned* svals = (unsigned*)(base + L.svals);
  int* begin = (int*)(base + L.begin); uint8_t* flag = (uint8_t*)(base + L.flag);
  int* offset = (int*)(base + L.offset); int* count = (int*)(base + L.count);
  int* seg_start = (int*)(base + L.seg_start); Partial* part = (Partial*)(base + L.part);
  const Cells g = {origin[0], origin[1], origin[2], 1.0 / h, h};
  const int n_pairs = 3 * n_faces;
  const int pb = (n_pairs + 255) / 256;
  // at most this many segments for THIS cell count (within what the workspace holds)
  const long long seg_cap = (long long)n_pairs / kSegment + n_cells;
  const int max_segs = (int)(seg_cap < L.max_segs ? seg_cap : L.max_segs);
  pair_keys_kernel<<<(n_faces + 255) / 256, 256, 0, s>>>(verts, n_verts, faces, n_faces, vert_cell, n_cells, keys, vals);
  rc = runs::sort_pairs(name, base + L.sort_tmp, L.sort_size, keys, skeys, vals, svals, n_pairs, runs::bit_length((unsigned)n_cells), s);
  if (rc) return rc;
  runs::lower_bound_kernel<unsigned><<<(n_cells + 1 + 255) / 256, 256, 0, s>>>(skeys, n_pairs, n_cells, begin);
  seg_flags_kernel<<<pb, 256, 0, s>>>(skeys, n_pairs, n_cells, begin, flag);
  scan::mask_offsets(flag, n_pairs, offset, count, s);
  runs::seg_start_kernel<256><<<pb, 256, 0, s>>>(flag, offset, n_pairs, max_segs, seg_start);
  seg_sum_kernel<<<(max_segs + 255) / 256, 256, 0, s>>>(verts, n_verts, faces, colors, g, skeys, svals, begin, seg_start, count, max_segs, part);
  cell_solve_kernel<<<(n_cells + 255) / 256, 256, 0, s>>>(verts, faces, g, tol, svals, begin, offset, n_cells, max_segs, part, out_verts,
                                                          out_colors, info, err);
  return check_launch(name);
}

int svs_mesh_cluster_faces_count(const float* verts, int n_verts, const int* faces, int n_faces, const int* vert_cell, int n_cells,
                                 void* workspace, uint8_t* keep, int* offsets, int* count, void* hip_stream) {
  const char* name = "svs_mesh_cluster_faces_count";
  int rc = check_counts(name, n_verts, n_faces, kMaxFaces);
  if (rc) return rc;
  if (n_cells < 0) { set_error("%s: negative count", name); return SVS_ESHAPE; }
  if (n_cells > kMaxCells) {
    set_error("%s: %d cells, at most %d in one call: three ranks of 21 bits make a face's key", name, n_cells, kMaxCells); return SVS_ESHAPE;
  }
  if (!count || (n_faces > 0 && (!faces || !workspace || !keep || !offsets || (n_verts > 0 && (!verts || !vert_cell)))))
    return null_pointer(name);
  hipStream_t s = (hipStream_t)hip_stream;
  if (n_faces == 0) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int), s);
    return e != hipSuccess ? hip_fail(name, e) : SVS_OK;
  }
  const FacesLayout L = faces_layout(n_faces);
  char* base = aligned(workspace);
  u64* keys = (u64*)(base + L.keys); u64* skeys = (u64*)(base + L.skeys);
  unsigned* idx = (unsigned*)(base + L.idx); unsigned* sidx = (unsigned*)(base + L.sidx);
  const int nb = (n_faces + 255) / 256;
  face_keys_kernel<<<nb, 256, 0, s>>>(verts, n_verts, faces, n_faces, vert_cell, n_cells, keys, idx);
  rc = runs::sort_pairs(name, base + L.sort_tmp, L.sort_size, keys, skeys, idx, sidx, n_faces,
                        2 * kCellBits + runs::bit_length((unsigned)n_cells), s);
  if (rc) return rc;
  face_keep_kernel<<<nb, 256, 0, s>>>(skeys, sidx, n_faces, (u64)n_cells << (2 * kCellBits), keep);
  scan::mask_offsets(keep, n_faces, offsets, count, s);
  return check_launch(name);
}

int svs_mesh_cluster_faces_emit(const int* faces, int n_faces, const int* vert_cell, const uint8_t* keep, const int* offsets,
                                int* out_faces, void* hip_stream) {
  const char* name = "svs_mesh_cluster_faces_emit";
  if (n_faces < 0) { set_error("%s: negative count", name); return SVS_ESHAPE; }
  if (n_faces > 0 && (!faces || !vert_cell || !keep || !offsets || !out_faces)) return null_pointer(name);
  if (n_faces == 0) return SVS_OK;
  face_emit_kernel<<<(n_faces + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(faces, n_faces, vert_cell, keep, offsets, out_faces);
  return check_launch(name);
}

}  // extern "C"
