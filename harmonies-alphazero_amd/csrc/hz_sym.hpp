// hz_sym.hpp — the board's symmetry group as device code.
//
// The 23-cell board (rows of 5-4-5-4-5 hexes) has four automorphisms, and
// each is an automorphism of the whole game (the rule: include/hz_abi.h,
// "board symmetries").  Group element g in 0..3 maps an axial coordinate
//   0: (q, r)   1: (-q, -r)   2: (q + r, -r)   3: (-q - r, r)
// and g = a ^ b composes a and b (Klein four-group): 3 is 1 after 2, and
// every element is its own inverse.  On the 23-bit cell set (bit c = cell c
// of sorted(VALID_HEXES)):
//   g & 1  the half turn sends cell c to 22 - c: one bit reversal;
//   g & 2  the reflection fixes the five cells of row r = 0 and swaps nine
//          pairs of cells 3, 4 or 6 indices apart: three delta swaps on
//          disjoint bits, independent of one another.
// Masks and permutation are checked against the constexpr geometry below.
#pragma once
#include "hz_device.hpp"

namespace hz {

constexpr int kSyms = 4;

// sorted(VALID_HEXES) -> (q, r), as grid_bit / col_bit list them
__host__ __device__ constexpr int cell_q(int c) {
  constexpr int Q[23] = {-3, -2, -2, -2, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 3};
  return Q[c];
}
__host__ __device__ constexpr int cell_r(int c) {
  constexpr int R[23] = {2, 0, 1, 2, -2, -1, 0, 1, 2, -2, -1, 0, 1, 2, -2, -1, 0, 1, 2, -2, -1, 0, -2};
  return R[c];
}
__host__ __device__ constexpr int cell_at(int q, int r) {  // -1: not on the board
  for (int c = 0; c < 23; c++)
    if (cell_q(c) == q && cell_r(c) == r) return c;
  return -1;
}
// the image of cell c under g, from the coordinate map alone
__host__ __device__ constexpr int sym_cell_geom(int c, int g) {
  const int q = cell_q(c), r = cell_r(c);
  const int q2 = g == 0 ? q : g == 1 ? -q : g == 2 ? q + r : -q - r;
  const int r2 = (g == 1 || g == 2) ? -r : r;
  return cell_at(q2, r2);
}
static_assert(grid_bit(7) == (cell_r(7) + 2) * 7 + cell_q(7) + 3 && col_bit(20) == (cell_q(20) + 3) * 6 + cell_r(20) + 2,
              "the same cell order as grid_bit / col_bit");

// the lower cell of every pair the reflection swaps D indices apart
__host__ __device__ constexpr uint32_t swap_mask(int d) {
  uint32_t m = 0;
  for (int c = 0; c < 23; c++) m |= (uint32_t)(sym_cell_geom(c, 2) == c + d) << c;
  return m;
}
constexpr uint32_t kSwap3 = swap_mask(3), kSwap4 = swap_mask(4), kSwap6 = swap_mask(6);
static_assert(kSwap3 == 0x21084u && kSwap4 == 0x40001u && kSwap6 == 0x2108u, "reflection pairs");

// 23-bit cell set under g: bit c moves to bit perm[g][c].  Bits 23..31 of x
// are ignored by the swaps and dropped by the reversal.
__host__ __device__ constexpr uint32_t sym_cells(uint32_t x, int g) {
  const uint32_t t3 = ((x >> 3) ^ x) & kSwap3, t4 = ((x >> 4) ^ x) & kSwap4, t6 = ((x >> 6) ^ x) & kSwap6;
  const uint32_t y = x ^ t3 ^ (t3 << 3) ^ t4 ^ (t4 << 4) ^ t6 ^ (t6 << 6);
  const uint32_t v = (g & 2) ? y : x;
  return (g & 1) ? __builtin_bitreverse32(v) >> 9 : v;
}
__host__ __device__ constexpr bool sym_cells_ok() {
  for (int g = 0; g < kSyms; g++) {
    uint32_t seen = 0;
    for (int c = 0; c < 23; c++) {
      const int d = sym_cell_geom(c, g);
      if (d < 0 || sym_cells(1u << c, g) != 1u << d) return false;
      seen |= 1u << d;
    }
    if (seen != kAll23 || sym_cells(kAll23, g) != kAll23) return false;
    for (int h = 0; h < kSyms; h++)  // composition is xor
      for (int c = 0; c < 23; c++)
        if (sym_cell_geom(sym_cell_geom(c, h), g) != sym_cell_geom(c, g ^ h)) return false;
  }
  return true;
}
static_assert(sym_cells_ok(), "sym_cells is the cell permutation of the geometry");
static_assert(sym_cell_geom(0, 2) == 4 && sym_cell_geom(3, 2) == 9 && sym_cell_geom(22, 3) == 4, "perm tables");

// One plane word: both players' 23-bit sets (bits 0..22 and 32..54) are
// permuted, every other bit is kept.
__host__ __device__ constexpr uint64_t sym_plane(uint64_t w, int g) {
  const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
  const uint32_t lo2 = (lo & ~kAll23) | sym_cells(lo & kAll23, g);
  const uint32_t hi2 = (hi & ~kAll23) | sym_cells(hi & kAll23, g);
  return ((uint64_t)hi2 << 32) | lo2;
}

// The state under g: the stack code of cell c moves to cell perm[g][c] on
// both boards; piles and misc never see a coordinate.
__host__ __device__ constexpr void sym_state(State& s, int g) {
  for (int k = 0; k < 4; k++) s.pl[k] = sym_plane(s.pl[k], g);
}

// Action a under g: the pile choices (a < 5) are kept, a placement
// 5 + 23 t + c goes to 5 + 23 t + perm[g][c].
__host__ __device__ constexpr int sym_action(int a, int g) {
  if (a < 5) return a;
  const int t = (a - 5) / 23, c = a - 5 - 23 * t;
  return 5 + 23 * t + __builtin_ctz(sym_cells(1u << c, g));
}
static_assert(sym_action(4, 3) == 4 && sym_action(5, 1) == 27 && sym_action(142, 2) == 5 + 23 * 5 + 18, "action map");

// The symmetry a search evaluates a leaf under (include/hz_abi.h, "leaf
// symmetries"): a pure function of the board's key and the leaf's node id in
// the board's pool, so whoever encodes the leaf and whoever reads its policy
// row compute it on their own and agree.
__host__ __device__ __forceinline__ int leaf_sym_of(uint64_t key, int node) {
  return (int)(mix64(key ^ (0x9FB21C651E98DF25ULL * (uint64_t)(node + 1))) >> 62);
}

}  // namespace hz
