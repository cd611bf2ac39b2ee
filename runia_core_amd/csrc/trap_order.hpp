// Balanced order of the 32-row blocks of an upper-trapezoidal R [r, D] (runia_qr_trapezoid_f64) over the 32-column groups
// of its packed transpose: ONE rule for the setup code that permutes the rows (qr.hip) and for K2' (proj_sq.hip), which
// takes every group's first live chunk from it.
//
// Block b of R (rows 32 b .. 32 b + 31) is zero for k < 32 b, so the column group that holds it may skip b chunks of 32.
// With the column split, group positions 0-3 of a 256-column block belong to one workgroup (column half 0) and 4-7 to
// another (half 1): in the natural order they skip 0+1+2+3 = 6 and 4+5+6+7 = 22 of their 64 chunk-waves, and the half-0
// workgroups set the kernel's time.  A row permutation of [R | c] does not change || R h + c ||, so which block sits in
// which group is free: half 0 takes blocks {0, 3, 5, 6}, half 1 blocks {1, 2, 4, 7} of every FULL 256-column block, 14
// skipped chunk-waves each.  Block 0 stays at position 0 (column tile 0 skips nothing: a NaN in h still reaches every
// row's score).  A last, partial block (r no multiple of 256) and every r < 256 keep the natural order.
#pragma once
#include <cstdint>

// R block held by 32-column group `pos` (= column / 32) of pack(R'^T), R' = R in balanced order, for r rows.
__host__ __device__ inline int64_t trap_balanced_block(int64_t pos, int64_t r) {
  const int64_t cb = pos >> 3;
  if ((cb + 1) * 256 > r) return pos;
  // positions 0..7 -> 0 3 5 6 | 1 2 4 7, one hex digit each
  return cb * 8 + ((0x74216530u >> (4 * (unsigned)(pos & 7))) & 7u);
}

// First k at which that group's columns can be non-zero: everything below is exact zeros.
__host__ __device__ inline int64_t trap_balanced_first_k(int64_t pos, int64_t r) { return 32 * trap_balanced_block(pos, r); }
