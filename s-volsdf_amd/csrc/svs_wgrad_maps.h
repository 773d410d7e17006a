// Address maps of the fp16x2 weight-gradient GEMM (svs_wgrad.hip, namespace h2) on v_mfma_f32_16x16x32_f16, and the proof
// that every transposed LDS read of its loop is free of bank conflicts.
//
// One MFMA contracts a whole 32-point tile.  Lane l of an operand fragment holds feature l & 15 of a 16-feature tile
// (= k-step s of a plane, svs_blocks_h2.h) and the 8 contraction elements 8 g .. 8 g + 7 of lane group g = l >> 4.  Which
// POINT a contraction element is, is free as long as A, B and the factor table agree; a fragment is two
// ds_read_b64_tr_b16 (4 consecutive points x 16 features each), and group g takes the point quads
//     quad_of(g, 0), quad_of(g, 1) = {0, 2}, {1, 3}, {4, 6}, {5, 7}
// With the planes' slot map,
//     byte = 1024 s + 256 (a >> 1) + 128 ((a & 1) ^ (s & 1)) + 64 (p & 1) + 16 q + 8 (p >> 1)
// (a = point quad, q = point in the quad, p = the lane's feature quad), the two groups of a 32-lane half share s, so
// they must differ in the parity of a to land in the two 128-byte halves of one 256-byte line -- which is what the quad
// assignment does.  (The natural order, group g takes points 8 g .. 8 g + 7, is a 2-way conflict on every read.)
#pragma once

namespace svs {
namespace wgrad {
namespace h2 {
namespace maps {

// the point quad (four consecutive points) that lane group g takes with read r (0, 1) of a fragment
constexpr int quad_of(int g, int r) { return 4 * (g >> 1) + (g & 1) + 2 * r; }

// contraction element j (0..7) of lane group g is this point of the tile
constexpr int point_of(int g, int j) { return 4 * quad_of(g, j >> 2) + (j & 3); }

// byte address, inside a plane as the LDS-DMA left it, that `lane` gives to read r of the fragment of tile s
constexpr int plane_rd(int s, int lane, int r) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3, a = quad_of(g, r);
  return 1024 * s + 256 * (a >> 1) + 128 * ((a & 1) ^ (s & 1)) + 64 * (p & 1) + 16 * q + 8 * (p >> 1);
}
// The kernel forms that address as  base(parity of s) + immediate:  plane_rd(s, lane, r) = plane_base(s & 1, lane) +
// 1024 s + 256 r.
constexpr int plane_base(int parity, int lane) { return plane_rd(parity, lane, 0) - 1024 * parity; }

// narrow B image (the 32 extra input rows of a radiance first layer, split into fp16 pieces in LDS):
// [column tile c (0, 1)][32 points][16 features] fp16, 32-byte rows; the mid image follows the hi image
constexpr int narrow_at(int feature, int point) { return 1024 * (feature >> 4) + 32 * point + 2 * (feature & 15); }
constexpr int narrow_rd(int c, int lane, int r) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  return narrow_at(16 * c + 4 * p, 4 * quad_of(g, r) + q);
}
constexpr int narrow_base(int lane) { return narrow_rd(0, lane, 0); }

// factor table of an item: 32 fp16, laid out so that the 8 factors of a lane group's contraction elements are one
// 16-byte read at 16 g
constexpr int factor_pos(int point) {
  const int a = point >> 2;
  return 8 * (2 * (a >> 2) + (a & 1)) + 4 * ((a >> 1) & 1) + (point & 3);
}

// ---- proofs
// A transposed read is conflict-free when the 32 lanes of each half hit 32 distinct 8-byte slots of one 256-byte bank
// row (bank = (byte / 4) mod 64; every region these offsets are added to starts at a multiple of 256 bytes).
constexpr bool half_rows_ok(const int (&addr)[64]) {
  for (int h = 0; h < 2; ++h) {
    bool seen[32] = {};
    const int row = addr[32 * h] >> 8;
    for (int l = 0; l < 32; ++l) {
      const int b = addr[32 * h + l];
      if ((b & 7) || (b >> 8) != row) return false;
      const int slot = (b & 255) >> 3;
      if (seen[slot]) return false;
      seen[slot] = true;
    }
  }
  return true;
}

// every read of the wide loop: the A and the B planes are read by the same map -- all 16 tiles (row tiles of A, column
// tiles of B), both reads of a fragment, hi plane (offset 0) and mid plane (offset plane_bytes)
constexpr bool plane_reads_ok(int plane_bytes) {
  for (int plane = 0; plane < 2; ++plane)
    for (int s = 0; s < 16; ++s)
      for (int r = 0; r < 2; ++r) {
        int addr[64] = {};
        for (int l = 0; l < 64; ++l) {
          addr[l] = plane * plane_bytes + plane_rd(s, l, r);
          if (plane_rd(s, l, r) != plane_base(s & 1, l) + 1024 * s + 256 * r) return false;     // the kernel's form
        }
        if (!half_rows_ok(addr)) return false;
      }
  return true;
}
constexpr bool narrow_reads_ok(int piece_bytes) {
  for (int piece = 0; piece < 2; ++piece)
    for (int c = 0; c < 2; ++c)
      for (int r = 0; r < 2; ++r) {
        int addr[64] = {};
        for (int l = 0; l < 64; ++l) {
          addr[l] = piece * piece_bytes + narrow_rd(c, l, r);
          if (narrow_rd(c, l, r) != narrow_base(l) + 1024 * c + 256 * r) return false;
        }
        if (!half_rows_ok(addr)) return false;
      }
  return true;
}
// the factor table follows the fragments: element j of group g sits at 8 g + j, and the 32 points fill the 32 places
constexpr bool factor_table_ok() {
  bool seen[32] = {};
  for (int g = 0; g < 4; ++g)
    for (int j = 0; j < 8; ++j) {
      const int pt = point_of(g, j);
      if (pt < 0 || pt >= 32 || seen[pt] || factor_pos(pt) != 8 * g + j) return false;
      seen[pt] = true;
    }
  return true;
}
// the natural point order (group g reads quads 2 g, 2 g + 1) would not pass: kept as a check of the checker
constexpr bool natural_order_conflicts() {
  int addr[64] = {};
  for (int l = 0; l < 64; ++l) {
    const int g = l >> 4, q = (l & 15) >> 2, p = l & 3, a = 2 * g;
    addr[l] = 256 * (a >> 1) + 128 * (a & 1) + 64 * (p & 1) + 16 * q + 8 * (p >> 1);
  }
  return !half_rows_ok(addr);
}

// (plane_reads_ok and narrow_reads_ok are asserted in svs_wgrad.hip, with the kernel's own region sizes)
static_assert(factor_table_ok(), "factor table does not follow the fragments' point order");
static_assert(natural_order_conflicts(), "the conflict check accepts a map known to conflict");

}  // namespace maps
}  // namespace h2
}  // namespace wgrad
}  // namespace svs
