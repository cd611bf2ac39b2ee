// Permutation memberships of the two-sample tests (shift.hip) as a pure function of (seed, p, i, n, N) - shared by the membership
// kernel and the host entry point runia_shift_perm_bits_host, so the CPU suite pins the stream the GPU walks (as boot_weights.hpp).
//   blk  = philox4x32_10(counter = (i, p >> 2, 0, 0x73686674 "shft"), key = (seed.lo, seed.hi))
//   word = component p & 3 of blk                      (one block serves four consecutive permutations of a row)
//   key  = word << 18 | i                              (50 bits, unique per row: i < 2^18)
// Row i belongs to the first set of permutation p >= 1 iff its key is among the n smallest of the N keys, i.e. the pair (word, i)
// is among the n smallest in lexicographic order; p = 0 is the identity (i < n).  Group sizes are exact.
// The n-th smallest key is found by a radix select over the key's digits (most significant first); every pass regenerates the
// words, so nothing of size N is stored.
#pragma once
#include "philox.hpp"

namespace runia_shift {

constexpr uint32_t kDomain = 0x73686674u;  // fourth counter word
constexpr int kIndexBits = 18;
constexpr int64_t kMaxRows = 1ll << kIndexBits;  // pooled rows of one test
constexpr int kPasses = 5, kBuckets = 2048;

__host__ __device__ __forceinline__ uint32_t word(uint64_t seed, uint32_t p, uint32_t i) {
  const runia_philox::u4 b = runia_philox::philox4x32_10(i, p >> 2, 0u, kDomain, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t c = p & 3u;
  return c == 0u ? b.x : (c == 1u ? b.y : (c == 2u ? b.z : b.w));
}

__host__ __device__ __forceinline__ uint64_t key(uint64_t seed, uint32_t p, uint32_t i) {
  return ((uint64_t)word(seed, p, i) << kIndexBits) | (uint64_t)i;
}

// digit `pass` of a key: bits shift .. shift + width - 1 (11 + 11 + 10 bits of the word, 11 + 7 bits of the index)
__host__ __device__ __forceinline__ int pass_shift(int pass) { return pass == 0 ? 39 : (pass == 1 ? 28 : (pass == 2 ? 18 : (pass == 3 ? 7 : 0))); }
__host__ __device__ __forceinline__ int pass_width(int pass) { return pass == 2 ? 10 : (pass == 4 ? 7 : 11); }

// the bucket that holds rank k (0-based) of a histogram, k reduced to the rank inside that bucket
__host__ __device__ __forceinline__ int find_bucket(const uint32_t* hist, int n_buckets, uint32_t& k) {
  int b = 0;
  while (b < n_buckets - 1 && k >= hist[b]) { k -= hist[b]; ++b; }
  return b;
}

}  // namespace runia_shift
