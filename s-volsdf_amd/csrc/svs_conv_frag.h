// What the matrix-core convolutions share (svs_conv_mfma / svs_conv_pair / svs_conv_gemm / svs_conv2d_mfma / svs_ucsnet /
// svs_lpips .hip): the vector types of v_mfma_f32_16x16x32_f16's operands, the two-piece fp16 split, the LDS pixel pitch,
// the one kernel that writes A fragments, and the dynamic-LDS opt-in of their launchers.
//
// A fragments: the weights of one k-step (K = 32) of one M tile (16 rows) are a PAIR of fragments [2 pieces][64 lanes][8] fp16
// (2 KiB): piece 0 the hi parts, piece 1 what hi leaves (mid).  Lane l holds row l & 15, k = 8 (l >> 4) + j, j = 0..7.  A
// layer's buffer is a sequence of such pairs; which weight sits at (pair, lane, j) is the layer's Map, stated once, directly
// above the kernel whose B-operand decode it mirrors.
#pragma once
#include "svs_common.h"

namespace svs {
namespace frag {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// v = h + m to float32 accuracy (22 bits while m is a normal fp16; not scaled: |v| >= 65504 gives h = inf)
__device__ __forceinline__ void split(float v, _Float16& h, _Float16& m) {
  h = (_Float16)v;
  m = (_Float16)(v - (float)h);
}
// eight consecutive values at once: one 16-byte operand unit and its mid piece
__device__ __forceinline__ void split(const float* v, f16x8& h, f16x8& m) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = v[j];
    const _Float16 hh = (_Float16)x;
    h[j] = hh;
    m[j] = (_Float16)(x - (float)hh);
  }
}

// Bytes per pixel and piece of a channel-last fp16 window in LDS: an odd multiple of 16, so that the 16-byte B-fragment
// reads of neighbouring pixels fall on different bank groups.
template <int CIN> constexpr int pitch() {
  static_assert(CIN == 8 || CIN == 16 || CIN == 32, "8, 16 or 32 channels");
  return CIN == 8 ? 16 : (CIN == 16 ? 48 : 80);
}

// The packer.  Map: a trivially copyable struct with the layer's sizes,
//   __host__ __device__ int n_fragments() const                                     -- fragment pairs in the buffer
//   __device__ float source(const float* w, int frag, int lane, int j) const        -- the weight at that place, or 0.0f
// One thread per element.  Nothing else writes an A fragment (svs_lpips.hip's packer, which scales rows, apart).
template <class Map>
__global__ void pack_fragments_kernel(const float* __restrict__ w, Map map, _Float16* __restrict__ frag) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= map.n_fragments() * 512) return;
  const int j = e & 7, lane = (e >> 3) & 63, f = e >> 9;
  _Float16 h, m;
  split(map.source(w, f, lane, j), h, m);
  const size_t base = ((size_t)f * 2 * 64 + lane) * 8 + j;
  frag[base] = h;
  frag[base + 64 * 8] = m;
}

// asynchronous on `s`, allocates nothing; `who` names the entry point in the error text
template <class Map>
int pack_fragments(const float* w, const Map& map, void* frag, hipStream_t s, const char* who) {
  const int n = map.n_fragments() * 512;
  pack_fragments_kernel<Map><<<(n + 255) / 256, 256, 0, s>>>(w, map, static_cast<_Float16*>(frag));
  return check_launch(who);
}

// Dynamic LDS above 64 KiB needs the attribute: set once per process and kernel (the static belongs to this
// instantiation), its result remembered; `bytes` is a constant of the kernel.
template <auto Kernel>
int opt_in_lds(int bytes, const char* who) {
  static const hipError_t e =
      hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e)); return (int)e; }
  return SVS_OK;
}

}  // namespace frag
}  // namespace svs
