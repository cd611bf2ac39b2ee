// Static instruction count of the bootstrap weight function (no GPU needed):
//     python tools/isa_stats.py tools/microbench/boot_weight_isa.hip
// One Philox block and its four Poisson(1) weights per thread - what runia_boot_metrics spends per (row, four replicates)
// before its scans (csrc/boot_weights.hpp).  The kernel is never launched.
#include "../../runia_core_amd/csrc/boot_weights.hpp"

__global__ void boot_weight_isa_kernel(const uint32_t* __restrict__ ids, uint64_t seed, uint32_t quad, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  out[i] = runia_boot::quad_weights(seed, quad, ids[i]);
}
