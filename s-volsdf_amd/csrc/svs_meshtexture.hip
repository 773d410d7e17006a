// A texture atlas for a mesh, baked from a scan's photographs, for gfx950 (svs_hip.meshtexture): one chart per valid face, two
// charts per square cell of the atlas; the painter's gather (svs_paint_gather.h) run per texel; the conversion to codes with
// the vertex-colour fallback; a renderer that samples the atlas through the face map of svs_mesh_raster_resolve.  The
// reference has no such step; the arithmetic is this project's, fixed in include/svolsdf_hip.h and restated in
// tests/meshtexture_oracle.py.
//
// bake_kernel is a gather like paint_kernel: one lane per texel walks the launch's views in index order with its four
// accumulators in registers: no atomics, one fixed order, the same bytes in every run.  Lanes map to texels row-major across
// the atlas, or cell by cell under SVS_ATLAS_CELL_MAJOR (NOTES/meshtexture.md has both timings).  All arithmetic is float64
// without contraction.
#include "svs_common.h"
#include "svs_mesh_face.h"
#include "svs_paint_gather.h"
#include "svs_scan.h"
#include "svs_views.h"

namespace svs {
namespace meshtexture {

using namespace views;
using namespace paintgather;

constexpr int kMinCell = 6;
constexpr int kMaxSize = 32768;      // S * S stays below 2^31

// chart corner A_k of half h in a cell of c texels, local texel coordinates
__device__ __forceinline__ void chart_corner(int h, int c, int k, int& x, int& y) {
  if (h == 0) { x = k == 1 ? c - 4 : 1; y = k == 2 ? c - 4 : 1; }
  else        { x = k == 1 ? 2 : c - 2; y = k == 2 ? 2 : c - 2; }
}

// ---- slots -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slot_flags_kernel(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                         int n_faces, uint8_t* __restrict__ work) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  meshface::Face t;
  if (!meshface::load_face(verts, n_verts, faces, f, t)) { work[f] = 0; return; }
  double d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {                              // d_k: the squared length of the edge opposite corner k
    const int p = (k + 2) % 3, q = (k + 1) % 3;
    const double dx = t.p[p][0] - t.p[q][0], dy = t.p[p][1] - t.p[q][1], dz = t.p[p][2] - t.p[q][2];
    d[k] = dx * dx + dy * dy + dz * dz;
  }
  int r = 0;
  if (d[1] > d[r]) r = 1;
  if (d[2] > d[r]) r = 2;
  work[f] = (uint8_t)(1 + r);
}

__global__ __launch_bounds__(256) void slot_chart_kernel(const uint8_t* __restrict__ work, int n_faces, int* __restrict__ chart,
                                                         int* __restrict__ counts) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f == 0) counts[1] = n_faces - counts[0];
  if (f >= n_faces) return;
  const int w = work[f];
  chart[f] = w ? chart[f] * 4 + (w - 1) : -1;               // chart held the exclusive scan of the flags: the slot
}

// ---- uv ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uv_kernel(const int* __restrict__ chart, int n_faces, int n_slots, int S, int c,
                                                 float* __restrict__ uv, int* __restrict__ slot_face) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_faces) return;
  const int ch = chart[f];
  const int slot = ch >> 2, r = ch & 3;
  float* __restrict__ out = uv + (size_t)f * 6;
  if (ch < 0 || slot >= n_slots || r > 2) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = 0.0f;
    return;
  }
  slot_face[slot] = f;
  const int n = S / c, q = slot >> 1, h = slot & 1;
  const int ox = (q % n) * c, oy = (q / n) * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {                              // face corner (r + k) % 3 sits at A_k
    int ax, ay;
    chart_corner(h, c, k, ax, ay);
    const int j = (r + k) % 3;
    out[2 * j] = (float)(((double)(ox + ax) + 0.5) / (double)S);
    out[2 * j + 1] = (float)(1.0 - ((double)(oy + ay) + 0.5) / (double)S);
  }
}

// ---- a texel's face -----------------------------------------------------------------------------------------------------
struct AtlasArgs {
  const int* faces;
  const int* chart;
  const int* slot_face;
  int n_verts, n_faces, n_slots, S, c, rows;
};

struct Texel {
  int idx[3];                        // the vertices at chart corners A_0, A_1, A_2: face corners r, r + 1, r + 2
  double b[3];                       // the clamped barycentrics of the texel centre against A_0, A_1, A_2
};

// texel (i, j) -> its face and barycentrics; false when it has no face (nothing is read through an index out of range)
__device__ __forceinline__ bool texel_face(const AtlasArgs& a, int i, int j, Texel& t) {
  const int c = a.c, n = a.S / c;
  if (i >= n * c || j >= n * c) return false;
  const int qx = i / c, qy = j / c, li = i - qx * c, lj = j - qy * c;
  const int h = li + lj <= c - 2 ? 0 : 1;                    // the ownership rule
  const long long slot = 2LL * ((long long)qy * n + qx) + h;
  if (slot >= a.n_slots) return false;
  const int f = a.slot_face[slot];
  if (f < 0 || f >= a.n_faces) return false;
  const int ch = a.chart[f], r = ch & 3;
  if (ch < 0 || r > 2) return false;
  int idx[3];
  if (!face_indices(a.faces, f, a.n_verts, idx)) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) t.idx[k] = idx[(r + k) % 3];
  double b1, b2;
  if (h == 0) { b1 = (double)(li - 1) / (double)(c - 5); b2 = (double)(lj - 1) / (double)(c - 5); }
  else        { b1 = (double)((c - 2) - li) / (double)(c - 4); b2 = (double)((c - 2) - lj) / (double)(c - 4); }
  double b0 = 1.0 - b1 - b2;
  b0 = b0 > 0.0 ? b0 : 0.0; b1 = b1 > 0.0 ? b1 : 0.0; b2 = b2 > 0.0 ? b2 : 0.0;   // gutter texels: onto the triangle
  const double s = b0 + b1 + b2;
  t.b[0] = b0 / s; t.b[1] = b1 / s; t.b[2] = b2 / s;
  return true;
}

// ---- bake --------------------------------------------------------------------------------------------------------------
struct BakeArgs {
  GatherArgs g;
  AtlasArgs t;
  const float* verts;
  const float* normals;
  double* acc;
};

// kCellMajor: lanes walk the atlas cell by cell (a wave covers whole cells and its lanes share two faces) instead of row by
// row across it; the texel decides the arithmetic, so the bytes are the same either way
template <bool kCellMajor>
__global__ __launch_bounds__(256) void bake_kernel(BakeArgs a) {
  __shared__ double eye[kMaxViews][3];
  load_eyes(a.g.mats, a.g.n_views, eye);
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int i, j;
  if (kCellMajor) {
    const int c = a.t.c, n = a.t.S / c;
    const long long q = lane / (c * c);
    if (q >= ((long long)a.t.n_slots + 1) / 2) return;
    const int w = (int)(lane - q * (c * c)), lj = w / c;
    j = (int)(q / n) * c + lj; i = (int)(q % n) * c + (w - lj * c);
  } else {
    if (lane >= (long long)a.t.rows * a.t.S) return;
    j = (int)(lane / a.t.S); i = (int)(lane - (long long)j * a.t.S);
  }
  const long long at = (long long)j * a.t.S + i;             // j < rows in both orders
  Texel t;
  if (!texel_face(a.t, i, j, t)) return;
  double p[3], n[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 3; ++k)
    p[k] = t.b[0] * (double)a.verts[(size_t)t.idx[0] * 3 + k] + t.b[1] * (double)a.verts[(size_t)t.idx[1] * 3 + k] +
           t.b[2] * (double)a.verts[(size_t)t.idx[2] * 3 + k];
  if (a.normals) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      n[k] = t.b[0] * (double)a.normals[(size_t)t.idx[0] * 3 + k] + t.b[1] * (double)a.normals[(size_t)t.idx[1] * 3 + k] +
             t.b[2] * (double)a.normals[(size_t)t.idx[2] * 3 + k];
    const double len = __builtin_sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(finite3(n[0], n[1], n[2]) && len > 0.0 && len <= kBig)) return;          // no direction: skipped in every view
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
  }
  double* __restrict__ acc = a.acc + (size_t)at * 4;
  double r = acc[0], g = acc[1], b = acc[2], wsum = acc[3];
  gather(a.g, eye, p[0], p[1], p[2], n, a.normals != nullptr, r, g, b, wsum);
  acc[0] = r; acc[1] = g; acc[2] = b; acc[3] = wsum;
}

// ---- finish ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void finish_kernel(AtlasArgs a, const double* __restrict__ acc, const uint8_t* __restrict__ vert_rgb,
                                                     int flags, uint8_t* __restrict__ atlas, uint8_t* __restrict__ covered) {
  const long long at = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= (long long)a.rows * a.S) return;
  const int j = (int)(at / a.S), i = (int)(at - (long long)j * a.S);
  Texel t;
  if (!texel_face(a, i, j, t)) return;
  const double w = acc ? acc[(size_t)at * 4 + 3] : 0.0;
  if (w > 0.0) {
    acc_codes(acc[(size_t)at * 4], acc[(size_t)at * 4 + 1], acc[(size_t)at * 4 + 2], w, flags, atlas + (size_t)at * 3);
    covered[at] = 1;
  } else if (vert_rgb) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      atlas[(size_t)at * 3 + ch] = code_u8(t.b[0] * (double)vert_rgb[(size_t)t.idx[0] * 3 + ch] + t.b[1] * (double)vert_rgb[(size_t)t.idx[1] * 3 + ch] +
                                           t.b[2] * (double)vert_rgb[(size_t)t.idx[2] * 3 + ch]);
    covered[at] = 2;
  }
}

// ---- render ------------------------------------------------------------------------------------------------------------
struct RenderArgs {
  const int* face;
  const float* verts;
  const int* faces;
  const int* chart;
  const double* mats;
  const uint8_t* atlas;
  uint8_t* rgb;
  long long total;                   // n_views * H * W
  int n_verts, n_faces, H, W, face_base, S, c;
};

__global__ __launch_bounds__(256) void render_kernel(RenderArgs a) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.total) return;
  const int id = a.face[p];
  if (id < 0) return;
  const long long f = (long long)id - (long long)a.face_base;
  if (f < 0 || f >= a.n_faces) return;                       // another call's mesh: left untouched
  const int ch = a.chart[f], r = ch & 3, slot = ch >> 2;
  if (ch < 0 || r > 2) return;
  int idx[3];
  if (!face_indices(a.faces, f, a.n_verts, idx)) return;
  const int c = a.c, n = a.S / c, q = slot >> 1, h = slot & 1;
  if (q / n >= n) return;                                    // a chart that does not lie in this atlas
  const long long hw = (long long)a.H * a.W;
  const int view = (int)(p / hw);
  const long long at = p - (long long)view * hw;
  const int iy = (int)(at / a.W), ix = (int)(at - (long long)iy * a.W);
  const double* __restrict__ M = a.mats + (size_t)view * kMatsPerView;
  double x[3], y[3], z[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Corner cn;
    project(M, a.verts + (size_t)idx[k] * 3, 0.0, cn);
    x[k] = cn.x; y[k] = cn.y; z[k] = cn.cz;
  }
  const double A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]);
  double b[3], zc;
  barycentrics(x, y, z, A, ix, iy, b, zc);
  const int ox = (q % n) * c, oy = (q / n) * c;
  double X = 0.0, Y = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {                              // face corner k sits at A_((k - r) mod 3)
    int ax, ay;
    chart_corner(h, c, (k - r + 3) % 3, ax, ay);
    const double w = b[k] / z[k] * zc;
    X = k == 0 ? w * (double)(ox + ax) : X + w * (double)(ox + ax);
    Y = k == 0 ? w * (double)(oy + ay) : Y + w * (double)(oy + ay);
  }
  const double top = (double)(a.S - 1);
  X = X >= 0.0 ? X : 0.0; X = X > top ? top : X;             // NaN to 0
  Y = Y >= 0.0 ? Y : 0.0; Y = Y > top ? top : Y;
  double col[3];
  bilinear_rgb(a.atlas, a.S, a.S, X, Y, col);
#pragma unroll
  for (int k = 0; k < 3; ++k) a.rgb[p * 3 + k] = code_u8(col[k]);
}

// S, c and the slots they must hold; SVS_OK or SVS_ESHAPE with the error set
inline int check_layout(const char* name, int n_slots, int S, int c) {
  if (n_slots < 0) { set_error("%s: negative count", name); return SVS_ESHAPE; }
  if (c < kMinCell || S < c || S > kMaxSize) {
    set_error("%s: a cell of %d texels in an atlas of %d (cells of at least %d, an atlas of a cell to %d)", name, c, S, kMinCell, kMaxSize);
    return SVS_ESHAPE;
  }
  const long long n = S / c;
  if (2 * n * n < (long long)n_slots) {
    set_error("%s: %d charts do not fit an atlas of %d texels with cells of %d (%lld fit)", name, n_slots, S, c, 2 * n * n);
    return SVS_ESHAPE;
  }
  return SVS_OK;
}

inline int chart_rows(int n_slots, int S, int c) {
  const long long n = S / c, cells = ((long long)n_slots + 1) / 2;
  return (int)((cells + n - 1) / n * c);
}

}  // namespace meshtexture
}  // namespace svs

using namespace svs;
using namespace svs::meshtexture;

extern "C" {

int svs_mesh_atlas_slots(const float* verts, int n_verts, const int* faces, int n_faces, uint8_t* work, int* chart, int* counts,
                         void* hip_stream) {
  if (n_verts < 0 || n_faces < 0 || n_faces > 0x7fffffff / 4) {
    set_error("svs_mesh_atlas_slots: bad counts (%d vertices, %d faces: chart = slot * 4 + rotation is an int32)", n_verts, n_faces);
    return SVS_ESHAPE;
  }
  if (!counts || (n_faces > 0 && (!faces || !work || !chart || (n_verts > 0 && !verts)))) {
    set_error("svs_mesh_atlas_slots: null argument"); return SVS_EINVAL;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  if (n_faces == 0) {
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int), s) != hipSuccess) return check_launch("svs_mesh_atlas_slots");
    return SVS_OK;
  }
  const unsigned blocks = (unsigned)((n_faces + 255) / 256);
  slot_flags_kernel<<<blocks, 256, 0, s>>>(verts, n_verts, faces, n_faces, work);
  scan::mask_offsets(work, n_faces, chart, counts, s);
  slot_chart_kernel<<<blocks, 256, 0, s>>>(work, n_faces, chart, counts);
  return check_launch("svs_mesh_atlas_slots");
}

int svs_mesh_atlas_uv(const int* chart, int n_faces, int n_slots, int S, int c, float* uv, int* slot_face, void* hip_stream) {
  if (n_faces < 0) { set_error("svs_mesh_atlas_uv: negative count"); return SVS_ESHAPE; }
  if (int rc = check_layout("svs_mesh_atlas_uv", n_slots, S, c)) return rc;
  if (n_slots > n_faces) { set_error("svs_mesh_atlas_uv: %d charts for %d faces", n_slots, n_faces); return SVS_ESHAPE; }
  if (n_faces == 0) return SVS_OK;
  if (!chart || !uv || (n_slots > 0 && !slot_face)) { set_error("svs_mesh_atlas_uv: null argument"); return SVS_EINVAL; }
  uv_kernel<<<(unsigned)((n_faces + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(chart, n_faces, n_slots, S, c, uv, slot_face);
  return check_launch("svs_mesh_atlas_uv");
}

int svs_mesh_atlas_bake(const float* verts, int n_verts, const float* normals, const int* faces, int n_faces, const int* chart,
                        const int* slot_face, int n_slots, int S, int c, const double* mats, int n_views, int H, int W, double near,
                        const float* depth, const uint8_t* const* images, const uint8_t* const* masks, double rel, double abs_tol,
                        double cos_min, int power, int flags, double* acc, void* hip_stream) {
  const bool cell_major = flags & SVS_ATLAS_CELL_MAJOR;
  flags &= ~SVS_ATLAS_CELL_MAJOR;
  if (int rc = check_rules("svs_mesh_atlas_bake", n_views, H, W, near, rel, abs_tol, cos_min, power, flags)) return rc;
  if (n_verts < 0 || n_faces < 0) { set_error("svs_mesh_atlas_bake: negative count"); return SVS_ESHAPE; }
  if (int rc = check_layout("svs_mesh_atlas_bake", n_slots, S, c)) return rc;
  if (!images) { set_error("svs_mesh_atlas_bake: null argument (images)"); return SVS_EINVAL; }
  if (n_verts == 0 || n_faces == 0 || n_slots == 0 || n_views == 0) return SVS_OK;
  if (!verts || !faces || !chart || !slot_face || !mats || !depth || !acc) { set_error("svs_mesh_atlas_bake: null argument"); return SVS_EINVAL; }
  BakeArgs a;
  if (int rc = fill_gather_args("svs_mesh_atlas_bake", a.g, mats, n_views, H, W, near, depth, images, masks, rel, abs_tol, cos_min,
                                power, flags)) return rc;
  a.t.faces = faces; a.t.chart = chart; a.t.slot_face = slot_face;
  a.t.n_verts = n_verts; a.t.n_faces = n_faces; a.t.n_slots = n_slots; a.t.S = S; a.t.c = c; a.t.rows = chart_rows(n_slots, S, c);
  a.verts = verts; a.normals = normals; a.acc = acc;
  if (cell_major) {
    const long long total = (((long long)n_slots + 1) / 2) * c * c;
    bake_kernel<true><<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(a);
  } else {
    const long long total = (long long)a.t.rows * S;
    bake_kernel<false><<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(a);
  }
  return check_launch("svs_mesh_atlas_bake");
}

int svs_mesh_atlas_finish(const double* acc, const int* faces, int n_faces, int n_verts, const int* chart, const int* slot_face,
                          int n_slots, int S, int c, const uint8_t* vert_rgb, int flags, uint8_t* atlas, uint8_t* covered,
                          void* hip_stream) {
  if (n_verts < 0 || n_faces < 0) { set_error("svs_mesh_atlas_finish: negative count"); return SVS_ESHAPE; }
  if (int rc = check_layout("svs_mesh_atlas_finish", n_slots, S, c)) return rc;
  if (flags & ~(SVS_PAINT_BEST | SVS_PAINT_ONE_SIDED)) { set_error("svs_mesh_atlas_finish: unknown flags %d", flags); return SVS_EINVAL; }
  if (n_verts == 0 || n_faces == 0 || n_slots == 0 || (!acc && !vert_rgb)) return SVS_OK;
  if (!faces || !chart || !slot_face || !atlas || !covered) { set_error("svs_mesh_atlas_finish: null argument"); return SVS_EINVAL; }
  AtlasArgs t;
  t.faces = faces; t.chart = chart; t.slot_face = slot_face;
  t.n_verts = n_verts; t.n_faces = n_faces; t.n_slots = n_slots; t.S = S; t.c = c; t.rows = chart_rows(n_slots, S, c);
  const long long total = (long long)t.rows * S;
  finish_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(t, acc, vert_rgb, flags, atlas, covered);
  return check_launch("svs_mesh_atlas_finish");
}

int svs_mesh_atlas_render(const int* face, const float* verts, int n_verts, const int* faces, int n_faces, int face_base,
                          const int* chart, const double* mats, int n_views, int H, int W, const uint8_t* atlas, int S, int c,
                          uint8_t* rgb, void* hip_stream) {
  if (int rc = check_views("svs_mesh_atlas_render", n_views, H, W)) return rc;
  if (n_verts < 0 || n_faces < 0 || face_base < 0) { set_error("svs_mesh_atlas_render: negative count"); return SVS_ESHAPE; }
  if (int rc = check_layout("svs_mesh_atlas_render", 0, S, c)) return rc;
  if (n_views == 0 || n_faces == 0 || n_verts == 0) return SVS_OK;
  if (!face || !verts || !faces || !chart || !mats || !atlas || !rgb) { set_error("svs_mesh_atlas_render: null argument"); return SVS_EINVAL; }
  RenderArgs a;
  a.face = face; a.verts = verts; a.faces = faces; a.chart = chart; a.mats = mats; a.atlas = atlas; a.rgb = rgb;
  a.total = (long long)n_views * H * W;
  a.n_verts = n_verts; a.n_faces = n_faces; a.H = H; a.W = W; a.face_base = face_base; a.S = S; a.c = c;
  render_kernel<<<(unsigned)((a.total + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch("svs_mesh_atlas_render");
}

}  // extern "C"
