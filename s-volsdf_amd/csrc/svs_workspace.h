// Host-side plumbing of the entries that work in a caller-supplied workspace (svs_meshsmooth.hip, svs_meshsimplify.hip,
// svs_poisson.hip, svs_cloud.hip): the carve-up into 256-byte slabs, the error returns with their one message text each,
// the download that ends an entry, and the argument checks more than one unit makes.  static / inline, like svs_scan.h:
// every unit that includes it gets its own copy.
#pragma once
#include "svs_common.h"

namespace svs {
namespace ws {

struct Bump {                                               // carve-up of the caller's workspace, 256-byte slabs
  size_t o = 0;
  size_t take(size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; }
};

// the first slab boundary in the caller's pointer: a workspace is sized with 256 bytes to spare for it
static inline char* aligned(void* ws) { return (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255); }

static inline int hip_fail(const char* name, hipError_t e) { set_error("%s: %s", name, hipGetErrorString(e)); return (int)e; }
static inline int null_pointer(const char* name) { set_error("%s: bad argument (null pointer)", name); return SVS_EINVAL; }

// host[0 .. n) = dev[0 .. n) once everything enqueued on s is done: the tail of an entry that returns counts
template <typename T>
static inline int download(const char* name, const T* dev, int n, T* host, hipStream_t s) {
  hipError_t e = hipMemcpyAsync(host, dev, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e != hipSuccess ? hip_fail(name, e) : SVS_OK;
}

// max_faces: what the unit's int indices allow (its pairs per face differ)
static inline int check_counts(const char* name, int n_verts, int n_faces, int max_faces) {
  if (n_verts < 0 || n_faces < 0) { set_error("%s: negative count", name); return SVS_ESHAPE; }
  if (n_faces > max_faces) { set_error("%s: more than %d faces", name, max_faces); return SVS_ESHAPE; }
  return SVS_OK;
}
static inline int check_origin(const char* name, const double* origin) {
  if (!origin) return null_pointer(name);
  if (!finite_f64(origin[0]) || !finite_f64(origin[1]) || !finite_f64(origin[2])) {
    set_error("%s: the origin must be finite", name); return SVS_EINVAL;
  }
  return SVS_OK;
}
// noun: "cell size", "node spacing"
static inline int check_spacing(const char* name, double h, const char* noun) {
  if (!(h > 0.0) || !finite_f64(h)) { set_error("%s: the %s must be positive and finite", name, noun); return SVS_EINVAL; }
  return SVS_OK;
}

}  // namespace ws
}  // namespace svs
