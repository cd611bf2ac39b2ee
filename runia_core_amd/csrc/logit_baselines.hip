// Post-hoc baselines beyond the reference's registry (inference/extended_postprocessors.py): MaxLogit, KL-Matching, fDBD.
//   runia_row_logit_stats_f32: max, logsumexp, sum p log p and first argmax of every logits row in one pass (MaxLogit; the
//                              fit and the row terms of KL-Matching) - the launch shapes of runia_row_lse_msp_f32 (rowwise.hip)
//   runia_klm_score_f32      : max_c sum_k p_k log q_c[k] - sum_k p_k log p_k = -min_c KL(p || q_c) on the f32 matrix cores,
//                              p formed while the tile is staged (tile layer of nt_tile_f32.hpp)
//   runia_fdbd_score_f32     : mean distance to the decision boundaries of the final layer over the distance to the training mean
//   runia_row_dist_f32       : || x - mu ||_2 per row (fDBD's denominator; l2_normalize writes a normalised copy and proj_norm
//                              multiplies by a packed D x D projector, neither gives the plain norm without more traffic)
#include "nt_tile_f32.hpp"

namespace {

// ---- row statistics ------------------------------------------------------------------------------------------------------
// (best_take / wave_best / kNoIndex: the first-argmax helpers of common.hpp)
// e = exp(x - m) and its share of sum e (x - m); a class with e == 0 (x = -inf included) adds nothing: p log p -> 0 as p -> 0
__device__ __forceinline__ void stat_term(float x, float m, float& s, float& t) {
  const float d = x - m, e = expf(d);
  s += e;
  t += (e == 0.f) ? 0.f : e * d;
}

// m_raw: the row maximum; an infinite one is replaced by 0 in the exponent, as scipy.special.logsumexp does (rowwise.hip)
__device__ __forceinline__ float stat_shift(float m_raw) { return (m_raw == INFINITY || m_raw == -INFINITY) ? 0.f : m_raw; }

// s = sum e, t = sum e (x - m):  lse = log s + m;  sum p log p = sum (e / s) (x - m - log s) = t / s - log s
__device__ __forceinline__ void finish_stats(float m_raw, float m, float s, float t, int idx, float* max_logit, float* lse,
                                             float* neg_entropy, int32_t* argmax, int64_t row) {
  const float ls = logf(s);
  if (max_logit) max_logit[row] = m_raw;
  if (lse) lse[row] = ls + m;
  if (neg_entropy) neg_entropy[row] = t / s - ls;
  if (argmax) argmax[row] = (idx == kNoIndex) ? 0 : idx;
}

// C <= 16: one row per lane straight from global memory, the row in registers (lse_tiny_kernel)
template <int CT>
__global__ __launch_bounds__(256) void stats_tiny_kernel(const float* __restrict__ x, float* max_logit, float* lse,
                                                          float* neg_entropy, int32_t* argmax, int64_t N) {
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < N; row += (int64_t)gridDim.x * 256) {
    const float* p = x + row * CT;
    float v[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j) v[j] = p[j];
    float bv = -INFINITY;
    int bi = kNoIndex;
#pragma unroll
    for (int j = 0; j < CT; ++j) best_take(bv, bi, v[j], j);
    const float m = stat_shift(bv);
    float s = 0.f, t = 0.f;
#pragma unroll
    for (int j = 0; j < CT; ++j) stat_term(v[j], m, s, t);
    finish_stats(bv, m, s, t, bi, max_logit, lse, neg_entropy, argmax, row);
  }
}

// 16 < C <= 64: one row per lane, tile staged through LDS with coalesced loads (lse_small_kernel).  The sums run in class
// order from column 0 whatever the lane (a row's bits must not depend on where in the batch it sits - KL-Matching promises
// that of its scores), so the bank spread comes from an odd row pitch instead of lse_small_kernel's rotated start column.
constexpr int kSmallRows = 128;

__global__ __launch_bounds__(kSmallRows) void stats_small_kernel(const float* __restrict__ x, float* max_logit, float* lse,
                                                                  float* neg_entropy, int32_t* argmax, int64_t N, int C) {
  extern __shared__ float tile[];  // kSmallRows * (C | 1) floats
  const int tid = threadIdx.x, pitch = C | 1;
  for (int64_t r0 = (int64_t)blockIdx.x * kSmallRows; r0 < N; r0 += (int64_t)gridDim.x * kSmallRows) {
    const int rows = (int)((N - r0 < kSmallRows) ? (N - r0) : kSmallRows);
    const int total = rows * C;
    const float* src = x + r0 * C;
    __syncthreads();
    for (int i = tid; i < total; i += kSmallRows) {
      const int r = i / C;
      tile[r * pitch + (i - r * C)] = src[i];
    }
    __syncthreads();
    if (tid < rows) {
      const float* row = tile + tid * pitch;
      float bv = -INFINITY;
      int bi = kNoIndex;
      for (int k = 0; k < C; ++k) best_take(bv, bi, row[k], k);
      const float m = stat_shift(bv);
      float s = 0.f, t = 0.f;
      for (int k = 0; k < C; ++k) stat_term(row[k], m, s, t);
      finish_stats(bv, m, s, t, bi, max_logit, lse, neg_entropy, argmax, r0 + tid);
    }
  }
}

// C > 64: one wave per row; the row stays in registers when it fits (lse_wave_kernel)
template <int NCH>  // float4 chunks per lane; NCH == 0 -> re-read the row (any C)
__global__ __launch_bounds__(64 * kRowWaves) void stats_wave_kernel(const float* __restrict__ x, float* max_logit, float* lse,
                                                                    float* neg_entropy, int32_t* argmax, int64_t N,
                                                                    int64_t C) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * kRowWaves;
  for (int64_t row = (int64_t)blockIdx.x * kRowWaves + wave; row < N; row += wave_stride) {
    const float* p = x + row * C;
    float bv = -INFINITY, s = 0.f, t = 0.f, m;
    int bi = kNoIndex;
    if constexpr (NCH > 0) {
      const float4* p4 = reinterpret_cast<const float4*>(p);
      const int n4 = (int)(C >> 2);
      float4 v[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int i = lane + 64 * c;
        v[c] = (i < n4) ? p4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int i = lane + 64 * c;
        if (i < n4) {
          best_take(bv, bi, v[c].x, 4 * i);
          best_take(bv, bi, v[c].y, 4 * i + 1);
          best_take(bv, bi, v[c].z, 4 * i + 2);
          best_take(bv, bi, v[c].w, 4 * i + 3);
        }
      }
      wave_best(bv, bi);
      m = stat_shift(bv);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (lane + 64 * c < n4) {
          stat_term(v[c].x, m, s, t);
          stat_term(v[c].y, m, s, t);
          stat_term(v[c].z, m, s, t);
          stat_term(v[c].w, m, s, t);
        }
      }
    } else {
      for (int64_t i = lane; i < C; i += 64) best_take(bv, bi, p[i], (int)i);
      wave_best(bv, bi);
      m = stat_shift(bv);
      for (int64_t i = lane; i < C; i += 64) stat_term(p[i], m, s, t);
    }
    s = wave_sum_f32(s);
    t = wave_sum_f32(t);
    if (lane == 0) finish_stats(bv, m, s, t, bi, max_logit, lse, neg_entropy, argmax, row);
  }
}

// ---- KL-Matching ---------------------------------------------------------------------------------------------------------
// A workgroup owns 128 rows and walks the class tiles of log_q (128 classes each); for every tile the products
// sum_k p[row, k] log_q[c, k] are accumulated over k = 0 .. C-1 in 32-wide chunks on v_mfma_f32_32x32x2_f32 (2 x 2 waves x
// 2 x 2 tiles of 32 x 32, LDS image and k permutation of knn_dist_kernel) and folded into a running maximum per accumulator
// slot: the N x K products are never written.  The A tile is p = exp(logit - lse), formed when the chunk goes from registers
// to LDS (no N x C probability table).  Every product is a k-ordered fma chain of its own row and class: a row's score does
// not depend on the rows it is batched with.  A NaN product makes the row NaN (np.max), as a NaN logit does through p.
__device__ __forceinline__ void store_prob_chunk(const float (&v)[16], float (*dst)[KP], int tid, float row_lse, bool row_ok,
                                                 int64_t k0, int64_t C) {
  const int row = tid >> 1, half = tid & 1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t k = k0 + half * 16 + 2 * j;
    const float a = (row_ok && k < C) ? exp_nonpos(v[2 * j] - row_lse) : 0.f;
    const float b = (row_ok && k + 1 < C) ? exp_nonpos(v[2 * j + 1] - row_lse) : 0.f;
    *reinterpret_cast<float2*>(&dst[row][half * 16 + 2 * j]) = make_float2(a, b);
  }
}

__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }  // NaN sticks

__global__ __launch_bounds__(256) void klm_score_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                         const float* __restrict__ neg_entropy,
                                                         const float* __restrict__ log_q, const int32_t* __restrict__ valid,
                                                         float* __restrict__ score, int64_t N, int64_t C, int64_t K) {
  __shared__ __attribute__((aligned(16))) float As[TQ][KP];
  __shared__ __attribute__((aligned(16))) float Bs[TB][KP];
  __shared__ float red[2][TQ];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave >> 1, wb = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const bool vec = ((C & 3) == 0) && ((((uintptr_t)logits) & 15) == 0) && ((((uintptr_t)log_q) & 15) == 0);
  const int64_t q0 = (int64_t)blockIdx.x * TQ;  // (the grid covers every row block: runia_klm_score_f32)
  {
    const bool row_ok = q0 + (tid >> 1) < N;
    const float row_lse = row_ok ? lse[q0 + (tid >> 1)] : 0.f;
    float best[2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) best[a][r] = -INFINITY;
    for (int64_t m0 = 0; m0 < K; m0 += TB) {
      f32x16 acc[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
      float ra[16], rb[16];
      load_chunk(logits, q0, N, C, 0, ra, tid, vec);
      load_chunk(log_q, m0, K, C, 0, rb, tid, vec);
      for (int64_t k0 = 0; k0 < C; k0 += KCH) {
        __syncthreads();  // every wave has finished reading the previous chunk
        store_prob_chunk(ra, As, tid, row_lse, row_ok, k0, C);
        store_chunk<false>(rb, Bs, tid);
        __syncthreads();
        if (k0 + KCH < C) {
          load_chunk(logits, q0, N, C, k0 + KCH, ra, tid, vec);
          load_chunk(log_q, m0, K, C, k0 + KCH, rb, tid, vec);
        }
#pragma unroll
        for (int s = 0; s < KCH / 4; ++s) {
          float2 av[2], bv[2];
#pragma unroll
          for (int a = 0; a < 2; ++a) av[a] = *reinterpret_cast<const float2*>(&As[wq * 64 + a * 32 + li][4 * s + 2 * lh]);
#pragma unroll
          for (int b = 0; b < 2; ++b) bv[b] = *reinterpret_cast<const float2*>(&Bs[wb * 64 + b * 32 + li][4 * s + 2 * lh]);
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a].x, bv[b].x, acc[a][b], 0, 0, 0);
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a].y, bv[b].y, acc[a][b], 0, 0, 0);
            }
        }
      }
      // C[row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)][col = lane&31]: the lane's class of this tile joins its running maxima
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int64_t col = m0 + wb * 64 + b * 32 + li;
        const bool use = col < K && (!valid || valid[col] != 0);
        if (use) {
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) best[a][r] = max_nan(best[a][r], acc[a][b][r]);
        }
      }
    }
    // maxima over the 32 class lanes of a half wave, then over the two waves that share the rows
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = wave_reduce<32>(best[a][r], [](float x, float y) { return max_nan(x, y); });
        if (li == 0) red[wb][wq * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = v;
      }
    __syncthreads();
    if (tid < TQ && q0 + tid < N) score[q0 + tid] = max_nan(red[0][tid], red[1][tid]) - neg_entropy[q0 + tid];
  }
}

// ---- fDBD ----------------------------------------------------------------------------------------------------------------
// One wave per row, lane l holds classes l, l + 64, ...; the predicted class's row of the table is read contiguously by the
// same lanes.  Sums: per lane in class order, then the wave's fixed exchange tree.
template <int NV>  // registers per lane; NV == 0 -> re-read the row in chunks (any C)
__global__ __launch_bounds__(64 * kRowWaves) void fdbd_kernel(const float* __restrict__ logits,
                                                              const float* __restrict__ inv_dist,
                                                              const float* __restrict__ feat_dist, float* __restrict__ score,
                                                              int64_t N, int64_t C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * kRowWaves + wave; row < N; row += (int64_t)gridDim.x * kRowWaves) {
    const float* p = logits + row * C;
    float bv = -INFINITY, acc = 0.f;
    int bi = kNoIndex;
    if constexpr (NV > 0) {
      float v[NV];
#pragma unroll
      for (int t = 0; t < NV; ++t) {
        const int j = lane + 64 * t;
        v[t] = (j < C) ? p[j] : -INFINITY;  // (padding under index >= C: never the first maximum)
      }
#pragma unroll
      for (int t = 0; t < NV; ++t) {  // ascending index inside a lane: only a larger value takes over
        const bool take = v[t] > bv || (v[t] == bv && bi == kNoIndex);
        bv = take ? v[t] : bv;
        bi = take ? lane + 64 * t : bi;
      }
      wave_best(bv, bi);
      if (bi >= C) bi = 0;  // (a row of NaN: no class, or the padding, wins; its score is NaN through the other classes' terms)
      const float top = bv;
      const float* w = inv_dist + (int64_t)bi * C;
#pragma unroll
      for (int t = 0; t < NV; ++t) {
        const int j = lane + 64 * t;
        if (j < C && j != bi) acc += fabsf(top - v[t]) * w[j];
        // the table loads of 16 slots at a time: all 64 in flight next to the 64 logits left the register file
        if constexpr (NV > 16) if ((t & 15) == 15) __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      for (int64_t j = lane; j < C; j += 64) best_take(bv, bi, p[j], (int)j);
      wave_best(bv, bi);
      if (bi == kNoIndex) bi = 0;
      const float top = bv;
      const float* w = inv_dist + (int64_t)bi * C;
      for (int64_t j = lane; j < C; j += 64)
        if (j != bi) acc += fabsf(top - p[j]) * w[j];
    }
    acc = wave_sum_f32(acc);
    if (lane == 0) score[row] = acc / ((float)(C - 1) * feat_dist[row]);
  }
}

// ---- || x - mu ||_2 per row, f32: lane-strided squares in column order, the wave's exchange tree, one sqrt ----
__global__ __launch_bounds__(64 * kRowWaves) void row_dist_kernel(const float* __restrict__ x, const float* __restrict__ mu,
                                                                  float* __restrict__ out, int64_t N, int64_t D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool vec = ((D & 3) == 0) && ((((uintptr_t)x) & 15) == 0) && ((((uintptr_t)mu) & 15) == 0);
  for (int64_t row = (int64_t)blockIdx.x * kRowWaves + wave; row < N; row += (int64_t)gridDim.x * kRowWaves) {
    const float* p = x + row * D;
    float s = 0.f;
    if (vec) {
      const float4* p4 = reinterpret_cast<const float4*>(p);
      const float4* m4 = reinterpret_cast<const float4*>(mu);
      for (int64_t i = lane; i < (D >> 2); i += 64) {
        const float4 a = p4[i], b = m4[i];
        const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
        s += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
    } else {
      for (int64_t i = lane; i < D; i += 64) {
        const float d = p[i] - mu[i];
        s += d * d;
      }
    }
    s = wave_sum_f32(s);
    if (lane == 0) out[row] = sqrtf(s);
  }
}

}  // namespace

extern "C" int runia_row_logit_stats_f32(const float* logits, float* max_logit, float* lse, float* neg_entropy,
                                         int32_t* argmax, int64_t N, int64_t C, runia_stream_t stream) {
  if (N < 0 || C <= 0 || C > 0x7fffffffll) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!logits || (!max_logit && !lse && !neg_entropy && !argmax)) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  if (C <= 16) {
    const unsigned grid = runia_stream_grid(N, 256);
#define RUNIA_STATS_TINY(CT) \
  case CT: stats_tiny_kernel<CT><<<grid, 256, 0, s>>>(logits, max_logit, lse, neg_entropy, argmax, N); break;
    switch ((int)C) {
      RUNIA_STATS_TINY(1) RUNIA_STATS_TINY(2) RUNIA_STATS_TINY(3) RUNIA_STATS_TINY(4) RUNIA_STATS_TINY(5) RUNIA_STATS_TINY(6)
      RUNIA_STATS_TINY(7) RUNIA_STATS_TINY(8) RUNIA_STATS_TINY(9) RUNIA_STATS_TINY(10) RUNIA_STATS_TINY(11)
      RUNIA_STATS_TINY(12) RUNIA_STATS_TINY(13) RUNIA_STATS_TINY(14) RUNIA_STATS_TINY(15) RUNIA_STATS_TINY(16)
    }
#undef RUNIA_STATS_TINY
    return runia_check_launch();
  }
  if (C <= 64) {
    const size_t shmem = (size_t)kSmallRows * (C | 1) * sizeof(float);
    stats_small_kernel<<<runia_stream_grid(N, kSmallRows), kSmallRows, shmem, s>>>(logits, max_logit, lse, neg_entropy, argmax, N,
                                                                           (int)C);
    return runia_check_launch();
  }
  const unsigned grid = runia_rows_grid(N);
  constexpr int kT = 64 * kRowWaves;
  const bool vec = ((C & 3) == 0) && ((((uintptr_t)logits) & 15) == 0);
  const int64_t n4 = C >> 2;
  if (vec && n4 <= 64)
    stats_wave_kernel<1><<<grid, kT, 0, s>>>(logits, max_logit, lse, neg_entropy, argmax, N, C);
  else if (vec && n4 <= 128)
    stats_wave_kernel<2><<<grid, kT, 0, s>>>(logits, max_logit, lse, neg_entropy, argmax, N, C);
  else if (vec && n4 <= 256)
    stats_wave_kernel<4><<<grid, kT, 0, s>>>(logits, max_logit, lse, neg_entropy, argmax, N, C);
  else if (vec && n4 <= 512)
    stats_wave_kernel<8><<<grid, kT, 0, s>>>(logits, max_logit, lse, neg_entropy, argmax, N, C);
  else
    stats_wave_kernel<0><<<grid, kT, 0, s>>>(logits, max_logit, lse, neg_entropy, argmax, N, C);
  return runia_check_launch();
}

extern "C" int runia_klm_score_f32(const float* logits, const float* lse, const float* neg_entropy, const float* log_q,
                                   const int32_t* valid, float* score, int64_t N, int64_t C, int64_t K,
                                   runia_stream_t stream) {
  if (N < 0 || C <= 0 || K <= 0) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!logits || !lse || !neg_entropy || !log_q || !score) return RUNIA_E_INVALID;
  const int64_t blocks = (N + TQ - 1) / TQ;
  if (blocks > 0x7fffffffll) return RUNIA_E_INVALID;
  klm_score_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(logits, lse, neg_entropy, log_q, valid, score, N, C, K);
  return runia_check_launch();
}

extern "C" int runia_fdbd_score_f32(const float* logits, const float* inv_dist, const float* feat_dist, float* score,
                                    int64_t N, int64_t C, runia_stream_t stream) {
  if (N < 0 || C < 2 || C > 0x7fffffffll) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!logits || !inv_dist || !feat_dist || !score) return RUNIA_E_INVALID;
  const unsigned grid = runia_rows_grid(N);
  constexpr int kT = 64 * kRowWaves;
  hipStream_t s = as_stream(stream);
  // the row in registers up to 4 096 classes (where GEN leaves its register form), re-read in chunks beyond
  if (C <= 64) fdbd_kernel<1><<<grid, kT, 0, s>>>(logits, inv_dist, feat_dist, score, N, C);
  else if (C <= 256) fdbd_kernel<4><<<grid, kT, 0, s>>>(logits, inv_dist, feat_dist, score, N, C);
  else if (C <= 1024) fdbd_kernel<16><<<grid, kT, 0, s>>>(logits, inv_dist, feat_dist, score, N, C);
  else if (C <= 4096) fdbd_kernel<64><<<grid, kT, 0, s>>>(logits, inv_dist, feat_dist, score, N, C);
  else fdbd_kernel<0><<<grid, kT, 0, s>>>(logits, inv_dist, feat_dist, score, N, C);
  return runia_check_launch();
}

extern "C" int runia_row_dist_f32(const float* x, const float* mu, float* out, int64_t N, int64_t D, runia_stream_t stream) {
  if (N < 0 || D <= 0) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!x || !mu || !out) return RUNIA_E_INVALID;
  row_dist_kernel<<<runia_rows_grid(N), 64 * kRowWaves, 0, as_stream(stream)>>>(x, mu, out, N, D);
  return runia_check_launch();
}
