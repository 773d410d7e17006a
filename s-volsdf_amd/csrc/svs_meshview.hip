// A triangle mesh seen from a scan's cameras, for gfx950 (svs_hip.meshview): depth map, face ids, normals and a shaded
// picture per view, and the per-vertex visibility that cuts a mesh to what the cameras and the evaluation masks see.
// The reference has no such step; the arithmetic is this project's, fixed in include/svolsdf_hip.h and restated in
// tests/meshview_oracle.py.
//
// svs_mesh_raster is a scatter: every (view, face) pair tests the pixel centres of its clamped bounding box and folds
// key = float32 depth bits << 32 | face id into the pixel with a 64-bit unsigned minimum.  The minimum is associative
// and commutative and the key of a (pixel, face) pair depends on nothing else, so the buffer does not depend on the
// order of faces, lanes, waves or launches.  atomicMin(unsigned long long) is one global_atomic_umin_x2 on gfx950 (no
// compare-and-swap loop); a plain load in front of it keeps losers from issuing one (a stale load can only be larger
// than the stored key, which costs an atomic that loses, never a missed one).
//
// Two paths, because faces run from sub-pixel size to the whole image.  raster_small_kernel: one lane per (view, face)
// projects the three corners (float64, no intermediate buffer), and walks the box itself when it holds at most kSmallBox
// pixels; larger boxes are appended to a device list, one atomic add per wave (ballot, popcount, rank).
// raster_large_kernel: a fixed grid of waves strides that list (its length is read on the device: no host round trip),
// the 64 lanes of a wave stride one box.  Views are the grid's y dimension.
// All camera arithmetic is float64 without contraction; projection, pixel rule and face helpers are those of svs_views.h.
#include "svs_common.h"
#include "svs_views.h"

namespace svs {
namespace meshview {

using namespace views;

constexpr int kSmallBox = 64;        // pixels of a clamped box the setting-up lane walks itself
constexpr int kLargeBlocks = 2048;   // raster_large_kernel: 256 CUs x 8 workgroups of four waves
constexpr int kWorkHead = 4;         // ints of `work` in front of the list: list length, small faces, atomics (64 bit)
constexpr unsigned long long kEmpty = ~0ull;

enum { kFlagCount = 1, kFlagSmallOnly = 2, kFlagLargeOnly = 4 };

struct Face {
  double x[3], y[3], z[3], A;
  int lx, hx, ly, hy;                // the clamped box, inclusive; empty when lx > hx or ly > hy
};

// rules 1-5 of the header.  false: the face is skipped or its box holds no pixel.
__device__ __forceinline__ bool setup_face(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces, int f,
                                           const double* __restrict__ M, double near, int H, int W, Face& s) {
  int idx[3];
  if (!face_indices(faces, f, n_verts, idx)) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Corner c;
    ok = project(M, verts + (size_t)idx[k] * 3, near, c) && ok;
    s.x[k] = c.x; s.y[k] = c.y; s.z[k] = c.cz;
  }
  if (!ok) return false;
  s.A = (s.x[1] - s.x[0]) * (s.y[2] - s.y[0]) - (s.y[1] - s.y[0]) * (s.x[2] - s.x[0]);
  if (!finite(s.A) || s.A == 0.0) return false;
  // the box, clamped while still float64: every coordinate is finite here, the clamped ones are in [0, W-1] x [0, H-1]
  double lx = __builtin_ceil(__builtin_fmin(s.x[0], __builtin_fmin(s.x[1], s.x[2])));
  double hx = __builtin_floor(__builtin_fmax(s.x[0], __builtin_fmax(s.x[1], s.x[2])));
  double ly = __builtin_ceil(__builtin_fmin(s.y[0], __builtin_fmin(s.y[1], s.y[2])));
  double hy = __builtin_floor(__builtin_fmax(s.y[0], __builtin_fmax(s.y[1], s.y[2])));
  lx = lx < 0.0 ? 0.0 : lx;
  ly = ly < 0.0 ? 0.0 : ly;
  hx = hx > (double)(W - 1) ? (double)(W - 1) : hx;
  hy = hy > (double)(H - 1) ? (double)(H - 1) : hy;
  if (lx > hx || ly > hy) return false;
  s.lx = (int)lx; s.hx = (int)hx; s.ly = (int)ly; s.hy = (int)hy;
  return true;
}

// rules 6-9 -> 1 when an atomic was issued
__device__ __forceinline__ int pixel(const Face& s, int ix, int iy, unsigned id, unsigned long long* __restrict__ zview, int W) {
  double b[3], zc;
  if (!barycentrics(s.x, s.y, s.z, s.A, ix, iy, b, zc)) return 0;
  const float zf = (float)zc;
  if (!(zf > 0.0f) || zf == __builtin_inff()) return 0;    // NaN, <= 0 (an underflow), inf: no key
  const unsigned long long key = ((unsigned long long)__float_as_uint(zf) << 32) | id;
  unsigned long long* at = zview + (size_t)iy * (size_t)W + (size_t)ix;
  if (key >= *at) return 0;
  atomicMin(at, key);
  return 1;
}

struct RasterArgs {
  const float* verts;
  const int* faces;
  const double* mats;
  unsigned long long* zbuf;
  int* work;                         // [0] list length, [1] faces walked by the small path, [2..3] atomics; then the list
  long long capacity;                // entries the list holds
  double near;
  int n_verts, n_faces, n_views, H, W, face_base, flags;
};

__device__ __forceinline__ void count_atomics(int* work, int issued) {
  for (int o = 32; o > 0; o >>= 1) issued += __shfl_xor(issued, o);
  if ((threadIdx.x & 63) == 0 && issued) atomicAdd(reinterpret_cast<unsigned long long*>(work + 2), (unsigned long long)issued);
}

__global__ __launch_bounds__(256) void raster_small_kernel(RasterArgs a) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int view = blockIdx.y;
  const double* __restrict__ M = a.mats + (size_t)view * kMatsPerView;     // uniform over the workgroup
  Face s;
  const bool drawn = f < a.n_faces && setup_face(a.verts, a.n_verts, a.faces, (int)f, M, a.near, a.H, a.W, s);
  long long box = 0;
  if (drawn) box = (long long)(s.hx - s.lx + 1) * (long long)(s.hy - s.ly + 1);
  const bool large = drawn && box > kSmallBox;
  // the wave's large faces take consecutive list places behind one atomic add (every lane of the wave reaches this point)
  const unsigned long long votes = __ballot(large);
  if (votes) {
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)votes) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(a.work, __popcll(votes));
    base = __shfl(base, leader);
    if (large) {
      const long long at = (long long)base + __popcll(votes & ((1ull << lane) - 1ull));
      if (at < a.capacity) a.work[kWorkHead + at] = view * a.n_faces + (int)f;
    }
  }
  int issued = 0;
  if (drawn && !large && !(a.flags & kFlagLargeOnly)) {
    unsigned long long* zview = a.zbuf + (size_t)view * (size_t)a.H * (size_t)a.W;
    const unsigned id = (unsigned)(a.face_base + (int)f);
    for (int iy = s.ly; iy <= s.hy; ++iy)
      for (int ix = s.lx; ix <= s.hx; ++ix) issued += pixel(s, ix, iy, id, zview, a.W);
  }
  if (a.flags & kFlagCount) {
    count_atomics(a.work, issued);
    const unsigned long long walked = __ballot(drawn && !large);
    if ((threadIdx.x & 63) == 0 && walked) atomicAdd(a.work + 1, __popcll(walked));
  }
}

__global__ __launch_bounds__(256) void raster_large_kernel(RasterArgs a) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  long long n = a.work[0];                                   // final: the small kernel ran before this one on the stream
  n = n < a.capacity ? n : a.capacity;
  int issued = 0;
  for (long long e = wave; e < n; e += (long long)gridDim.x * 4) {
    const int entry = a.work[kWorkHead + e];                 // uniform over the wave
    if (entry < 0) continue;
    const int view = entry / a.n_faces, f = entry - view * a.n_faces;
    if (view >= a.n_views) continue;
    Face s;
    if (!setup_face(a.verts, a.n_verts, a.faces, f, a.mats + (size_t)view * kMatsPerView, a.near, a.H, a.W, s)) continue;
    unsigned long long* zview = a.zbuf + (size_t)view * (size_t)a.H * (size_t)a.W;
    const unsigned id = (unsigned)(a.face_base + f);
    const int bw = s.hx - s.lx + 1;
    const long long box = (long long)bw * (long long)(s.hy - s.ly + 1);
    for (long long p = lane; p < box; p += 64) {
      const int row = (int)(p / bw), col = (int)(p - (long long)row * bw);
      issued += pixel(s, s.lx + col, s.ly + row, id, zview, a.W);
    }
  }
  if (a.flags & kFlagCount) count_atomics(a.work, issued);
}

struct ResolveArgs {
  const unsigned long long* zbuf;
  const float* verts;
  const int* faces;
  const double* mats;
  const uint8_t* vert_rgb;
  float* depth;
  int* face;
  float* normal;
  uint8_t* shade;
  long long total;                   // n_views * H * W
  int n_verts, n_faces, H, W, face_base;
};

__global__ __launch_bounds__(256) void resolve_kernel(ResolveArgs a) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.total) return;
  const unsigned long long key = a.zbuf[p];
  if (key == kEmpty) {
    a.depth[p] = 0.0f;
    a.face[p] = -1;
    if (a.normal) { a.normal[p * 3] = 0.0f; a.normal[p * 3 + 1] = 0.0f; a.normal[p * 3 + 2] = 0.0f; }
    if (a.shade) { a.shade[p * 3] = 255; a.shade[p * 3 + 1] = 255; a.shade[p * 3 + 2] = 255; }
    return;
  }
  a.depth[p] = __uint_as_float((unsigned)(key >> 32));
  const int id = (int)(unsigned)(key & 0xffffffffull);
  a.face[p] = id;
  if (!a.normal && !a.shade) return;
  const long long f = (long long)id - (long long)a.face_base;
  if (f < 0 || f >= a.n_faces) return;                       // another call's mesh: left untouched
  int idx[3];
  if (!face_indices(a.faces, f, a.n_verts, idx)) return;
  const long long hw = (long long)a.H * a.W;
  const int view = (int)(p / hw);
  const long long q = p - (long long)view * hw;
  const int iy = (int)(q / a.W), ix = (int)(q - (long long)iy * a.W);
  const double* __restrict__ M = a.mats + (size_t)view * kMatsPerView;
  Corner c[3];
  Face s;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    project(M, a.verts + (size_t)idx[k] * 3, 0.0, c[k]);
    s.x[k] = c[k].x; s.y[k] = c[k].y; s.z[k] = c[k].cz;
  }
  // unit normal in camera space, towards the camera
  const double ux = c[1].cx - c[0].cx, uy = c[1].cy - c[0].cy, uz = c[1].cz - c[0].cz;
  const double vx = c[2].cx - c[0].cx, vy = c[2].cy - c[0].cy, vz = c[2].cz - c[0].cz;
  double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const double len = __builtin_sqrt(nx * nx + ny * ny + nz * nz);
  const bool unit = len > 0.0 && len <= kBig;
  nx = unit ? nx / len : 0.0; ny = unit ? ny / len : 0.0; nz = unit ? nz / len : 0.0;
  if (nz > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
  if (a.normal) { a.normal[p * 3] = (float)nx; a.normal[p * 3 + 1] = (float)ny; a.normal[p * 3 + 2] = (float)nz; }
  if (!a.shade) return;
  const double g = 0.2 + 0.8 * __builtin_fabs(nz);
  double col[3] = {1.0, 1.0, 1.0};
  if (a.vert_rgb) {
    s.A = (s.x[1] - s.x[0]) * (s.y[2] - s.y[0]) - (s.y[1] - s.y[0]) * (s.x[2] - s.x[0]);
    // b_k and zc again, whether or not float64 noise still calls the pixel covered (svs_mesh_raster did)
    double b[3], zc;
    barycentrics(s.x, s.y, s.z, s.A, ix, iy, b, zc);
    const double w0 = b[0] / s.z[0] * zc, w1 = b[1] / s.z[1] * zc, w2 = b[2] / s.z[2] * zc;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      col[ch] = w0 * ((double)a.vert_rgb[(size_t)idx[0] * 3 + ch] / 255.0) + w1 * ((double)a.vert_rgb[(size_t)idx[1] * 3 + ch] / 255.0) +
                w2 * ((double)a.vert_rgb[(size_t)idx[2] * 3 + ch] / 255.0);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) a.shade[p * 3 + ch] = code_u8(255.0 * (g * col[ch]));
}

struct VisibilityArgs {
  const float* verts;
  const double* mats;
  const float* depth;
  const uint8_t* mask[kMaxViews];
  int* seen;
  int* off_mask;
  double near, rel, abs_tol;
  int n_verts, n_views, H, W;
};

__global__ __launch_bounds__(256) void visibility_kernel(VisibilityArgs a) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= a.n_verts) return;
  int seen = 0, off = 0;
  for (int view = 0; view < a.n_views; ++view) {
    Corner c; size_t pix;
    if (!project(a.mats + (size_t)view * kMatsPerView, a.verts + (size_t)v * 3, a.near, c) || !nearest_pixel(c, a.H, a.W, pix)) continue;
    if (masked_out(a.mask[view], pix)) { ++off; continue; }
    const double d = (double)a.depth[(size_t)view * (size_t)a.H * (size_t)a.W + pix];
    if (not_hidden(d, c.cz, a.rel, a.abs_tol)) ++seen;
  }
  a.seen[v] += seen;
  a.off_mask[v] += off;
}

}  // namespace meshview
}  // namespace svs

using namespace svs;
using namespace svs::meshview;

extern "C" {

int svs_mesh_raster_small_box(void) { return kSmallBox; }

int svs_mesh_raster(const float* verts, int n_verts, const int* faces, int n_faces, const double* mats, int n_views, int H,
                    int W, double near, int face_base, unsigned long long* zbuf, int* work, long long work_ints, int flags,
                    void* hip_stream) {
  if (int rc = check_views("svs_mesh_raster", n_views, H, W)) return rc;
  if (!(near > 0.0)) { set_error("svs_mesh_raster: near must be positive"); return SVS_EINVAL; }
  if (n_verts < 0 || n_faces < 0 || face_base < 0 || (long long)face_base + n_faces > 0x7fffffffLL) {
    set_error("svs_mesh_raster: bad counts (%d vertices, %d faces, face_base %d: ids are int32)", n_verts, n_faces, face_base);
    return SVS_ESHAPE;
  }
  if (!work || work_ints < kWorkHead) { set_error("svs_mesh_raster: work holds at least %d ints", kWorkHead); return SVS_EINVAL; }
  if (n_faces == 0 || n_views == 0) return SVS_OK;         // nothing is touched, work included
  hipStream_t s = (hipStream_t)hip_stream;
  if (!verts || !faces || !mats || !zbuf) { set_error("svs_mesh_raster: null argument"); return SVS_EINVAL; }
  if ((long long)n_views * n_faces > 0x7fffffffLL || work_ints - kWorkHead < (long long)n_views * n_faces) {
    set_error("svs_mesh_raster: work needs %d + n_views * n_faces ints (int32 entries: chunk the faces)", kWorkHead);
    return SVS_ESHAPE;
  }
  RasterArgs a;
  a.verts = verts; a.faces = faces; a.mats = mats; a.zbuf = zbuf; a.work = work; a.capacity = work_ints - kWorkHead;
  a.near = near; a.n_verts = n_verts; a.n_faces = n_faces; a.n_views = n_views; a.H = H; a.W = W; a.face_base = face_base;
  a.flags = flags;
  if (hipMemsetAsync(work, 0, kWorkHead * sizeof(int), s) != hipSuccess) return check_launch("svs_mesh_raster");
  raster_small_kernel<<<dim3((unsigned)((n_faces + 255) / 256), (unsigned)n_views), 256, 0, s>>>(a);
  if (!(flags & kFlagSmallOnly)) raster_large_kernel<<<kLargeBlocks, 256, 0, s>>>(a);
  return check_launch("svs_mesh_raster");
}

int svs_mesh_raster_resolve(const unsigned long long* zbuf, const float* verts, int n_verts, const int* faces, int n_faces,
                            const double* mats, int n_views, int H, int W, int face_base, const uint8_t* vert_rgb, float* depth,
                            int* face, float* normal, uint8_t* shade, void* hip_stream) {
  if (int rc = check_views("svs_mesh_raster_resolve", n_views, H, W)) return rc;
  if (n_verts < 0 || n_faces < 0 || face_base < 0) { set_error("svs_mesh_raster_resolve: negative count"); return SVS_ESHAPE; }
  if (n_views == 0) return SVS_OK;
  if (!zbuf || !depth || !face || ((normal || shade) && n_faces > 0 && (!verts || !faces || !mats))) {
    set_error("svs_mesh_raster_resolve: null argument"); return SVS_EINVAL;
  }
  ResolveArgs a;
  a.zbuf = zbuf; a.verts = verts; a.faces = faces; a.mats = mats; a.vert_rgb = vert_rgb; a.depth = depth; a.face = face;
  a.normal = normal; a.shade = shade; a.total = (long long)n_views * H * W;
  a.n_verts = n_verts; a.n_faces = n_faces; a.H = H; a.W = W; a.face_base = face_base;
  resolve_kernel<<<(unsigned)((a.total + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch("svs_mesh_raster_resolve");
}

int svs_mesh_vertex_visibility(const float* verts, int n_verts, const double* mats, int n_views, int H, int W, double near,
                               const float* depth, const uint8_t* const* masks, double rel, double abs_tol, int* seen,
                               int* off_mask, void* hip_stream) {
  if (int rc = check_views("svs_mesh_vertex_visibility", n_views, H, W)) return rc;
  if (!(near > 0.0) || !(rel >= 0.0) || !(abs_tol >= 0.0)) {
    set_error("svs_mesh_vertex_visibility: near must be positive, rel and abs_tol not negative"); return SVS_EINVAL;
  }
  if (n_verts < 0) { set_error("svs_mesh_vertex_visibility: negative count"); return SVS_ESHAPE; }
  if (n_verts == 0 || n_views == 0) return SVS_OK;
  if (!verts || !mats || !depth || !seen || !off_mask) { set_error("svs_mesh_vertex_visibility: null argument"); return SVS_EINVAL; }
  VisibilityArgs a;
  a.verts = verts; a.mats = mats; a.depth = depth; a.seen = seen; a.off_mask = off_mask;
  view_pointers(masks, n_views, a.mask);
  a.near = near; a.rel = rel; a.abs_tol = abs_tol; a.n_verts = n_verts; a.n_views = n_views; a.H = H; a.W = W;
  visibility_kernel<<<(n_verts + 255) / 256, 256, 0, (hipStream_t)hip_stream>>>(a);
  return check_launch("svs_mesh_vertex_visibility");
}

}  // extern "C"
