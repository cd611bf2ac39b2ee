// Poisson(1) bootstrap weights as a pure function of (seed, replicate, id) - shared by the replicate kernel (bootstrap.hip)
// and the host entry point runia_boot_weights_host, so the CPU suite pins the stream the GPU walks.
//   blk  = philox4x32_10(counter = (id, b >> 2, 0, 0x626f6f74 "boot"), key = (seed.lo, seed.hi))
//   word = component b & 3 of blk                      (one block serves four consecutive replicates of an id)
//   w    = number of thresholds T_k <= word,  T_k = floor(2^32 e^-1 sum_{j<=k} 1/j!),  k = 0 .. 12
// T_k is the Poisson(1) distribution function in 32-bit fixed point; T_12 = 2^32 - 1 is the last value that still rises, so
// the largest weight is 13 (probability 2^-32).  The 13 values were computed with 60-digit decimals; the host test
// recomputes them the same way.
#pragma once
#include "philox.hpp"

namespace runia_boot {

constexpr int kMaxWeight = 13;
constexpr uint32_t kDomain = 0x626f6f74u;  // fourth counter word

__host__ __device__ __forceinline__ uint32_t weight_of_word(uint32_t x) {
  uint32_t w = 0u;
  w += x >= 0x5e2d58d8u; w += x >= 0xbc5ab1b1u; w += x >= 0xeb715e1du; w += x >= 0xfb239797u;
  w += x >= 0xff1025f5u; w += x >= 0xffd90f3bu; w += x >= 0xfffa8b71u; w += x >= 0xffff540cu;
  w += x >= 0xffffed1fu; w += x >= 0xfffffe21u; w += x >= 0xffffffd4u; w += x >= 0xfffffffcu;
  w += x >= 0xffffffffu;
  return w;
}

// the block of replicates 4 q .. 4 q + 3 of `id`
__host__ __device__ __forceinline__ runia_philox::u4 quad_block(uint64_t seed, uint32_t q, uint32_t id) {
  return runia_philox::philox4x32_10(id, q, 0u, kDomain, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// the four weights of a block, 4 bits each: replicate 4 q + j in bits 4 j .. 4 j + 3
__host__ __device__ __forceinline__ uint32_t quad_weights(uint64_t seed, uint32_t q, uint32_t id) {
  const runia_philox::u4 b = quad_block(seed, q, id);
  return weight_of_word(b.x) | (weight_of_word(b.y) << 4) | (weight_of_word(b.z) << 8) | (weight_of_word(b.w) << 12);
}

__host__ __device__ __forceinline__ uint32_t weight(uint64_t seed, uint64_t b, uint32_t id) {
  return (quad_weights(seed, (uint32_t)(b >> 2), id) >> (4 * (unsigned)(b & 3))) & 15u;
}

}  // namespace runia_boot
