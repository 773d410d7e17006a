// Per-point power-of-two scaling shared by the fp16x2 backward sweeps (svs_mlp_bwd_h2.hip, svs_bg_h2.hip); see the
// header of svs_mlp_bwd_h2.hip.
#pragma once
#include "svs_mlp_h2_dev.h"
#include "svs_blocks_h2.h"

namespace svs {
namespace mlp {

struct PointScale {
  float s_in, inv_in;   // the operand being consumed holds true * s_in
  float s_out;          // the operand being produced is split as true * s_out
  float m;              // running max |true| of the operand being produced (this lane's rows)
  float floor_m;        // lower bound of the maxima
  float gmax;           // max over everything tracked so far

  // s * mx in [2^4, 2^5)
  static __device__ __forceinline__ float pow2_for(float mx) {
    int e = (int)((__float_as_uint(mx) >> 23) & 0xff);
    e = e < 24 ? 24 : (e > 230 ? 230 : e);
    return __uint_as_float((unsigned)(258 - e) << 23);
  }
  static __device__ __forceinline__ float inv_pow2(float s) { return __uint_as_float((254u << 23) - __float_as_uint(s)); }
  // m0: max |true| of the first operand over the whole column (both lane halves)
  __device__ __forceinline__ void start(float m0, float fl) {
    floor_m = fl; gmax = m0;
    s_in = pow2_for(__builtin_fmaxf(m0, fl)); inv_in = inv_pow2(s_in);
    s_out = s_in; m = 0.0f;
  }
  // the first operand comes from a stored half block (svs_blocks_h2.h): its scale is the stored one; m0 its maximum
  __device__ __forceinline__ void start_stored(float s_stored, float m0, float fl) {
    floor_m = fl; gmax = m0;
    s_in = s_stored; inv_in = inv_pow2(s_in);
    s_out = pow2_for(__builtin_fmaxf(m0, fl)); m = 0.0f;
  }
  __device__ __forceinline__ void track(float v) { m = __builtin_fmaxf(m, __builtin_fabsf(v)); }
  // the operand just produced becomes the one consumed
  __device__ __forceinline__ void next() {
    m = __builtin_fmaxf(m, __shfl_xor(m, 32));
    gmax = __builtin_fmaxf(gmax, m);
    s_in = s_out; inv_in = inv_pow2(s_in);
    s_out = pow2_for(__builtin_fmaxf(m, floor_m));
    m = 0.0f;
  }
};

__device__ __forceinline__ void publish_max(float* slot, float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, d));
  if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned*>(slot), __float_as_uint(v));
}

// ---- the stores of one tile of a scaled block, and how many of them a barrier may leave in flight
// A tile is two fragments (k-steps 2 tp, 2 tp + 1) of the hi plane and, with GP, of the mid plane: kTileStores<GP> vector
// stores, numbered i = 0 .. kTileStores - 1 in issue order (fragment 0: hi, mid; fragment 1: hi, mid).  The radiance sweep
// (rgb_bwd_h2_kernel) issues a tile's stores through store_tile_piece() alone -- a loop of kTileStores trips -- and gives
// the SAME constant to Stream::advance_keep<N>: what the epilogue issues and what the barrier leaves in flight cannot
// drift apart (a too-large N would let the barrier pass before the chunk's LDS-DMA has landed -- silently).
// The SDF sweeps (PassAEpi / PassBEpi::store_slot) take their N from the constant too, but keep their store lines written
// out: routed through the loop, hipcc allocates the registers of their GP instances differently, and those launches are the
// step's HBM phase, whose machine code this header has no business changing.
template <bool GP>
constexpr int kTileStores = GP ? 4 : 2;
template <bool GP>
__device__ __forceinline__ void store_tile_piece(float* blk, int tp, int lane, int i, const f16x8* h, const f16x8* m) {
  const int f = GP ? i >> 1 : i;
  if (GP && (i & 1)) store_piece(blk, 2 * tp + f, lane, m[f], 1);
  else store_piece(blk, 2 * tp + f, lane, h[f], 0);
}
// all of them at once (an epilogue that is not spread over MFMA gaps)
template <bool GP>
__device__ __forceinline__ void store_tile_pieces(float* blk, int tp, int lane, const f16x8* h, const f16x8* m) {
#pragma unroll
  for (int i = 0; i < kTileStores<GP>; ++i) store_tile_piece<GP>(blk, tp, lane, i, h, m);
}
// Spread behind the LDS-DMA pieces of a 16-k-step tile (Stream::prefetch_step issues the 9 pieces in k-steps 0..8): store i
// goes out in k-step late_store_step(i) >= 9, so every store is younger than every piece, as advance_keep<N> requires.
// Fragment 0 is complete at k-step 7 (hi at 9, mid at 11: one store per MFMA gap), fragment 1 at k-step 15.
template <bool GP>
__device__ __forceinline__ constexpr int late_store_step(int i) {
  return (GP ? i >> 1 : i) ? 15 : ((GP && (i & 1)) ? 11 : 9);
}
template <bool GP>
__device__ __forceinline__ void store_tile_late(float* blk, int tp, int lane, int s, const f16x8* h, const f16x8* m) {
#pragma unroll
  for (int i = 0; i < kTileStores<GP>; ++i)
    if (s == late_store_step<GP>(i)) store_tile_piece<GP>(blk, tp, lane, i, h, m);
}

__device__ __forceinline__ void split_tile_scaled(const f32x16& y, int t, Pieces2& p, float s) {
  f32x16 v;
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = y[r] * s;
  split_tile(v, t, p);
}

}  // namespace mlp
}  // namespace svs
