// PaCMAP on the device (Wang, Huang, Rudin, Shaposhnik, "Understanding How Dimension Reduction Tools Work", JMLR 22(201),
// 2021): the exact kNN graph, the three kinds of pairs and one Adam iteration per launch.  The reference exports
// fit_pacmap / apply_pacmap_transform / plot_samples_pacmap on top of pacmap==0.7.0 (dimensionality_reduction.py:88-177);
// pacmap, numba and annoy are not on this platform, so this is the only implementation.
//
//   runia_pacmap_knn_f32    exact kNN of Q query rows among N bank rows: f32 sum of squared differences in column order,
//                           one sorted top-K list per query kept in registers (no Q x N matrix in HBM).  Order: ascending
//                           (squared distance, index); with exclude_self, bank row q is left out of query q's list by index.
//   runia_pacmap_pairs      NB selection from the candidate table (scaled distances, or the first n_nb for a transform),
//                           MN and FP sampling with the Philox stream below.
//   runia_pacmap_step_f32   one Adam iteration: each row's gradient from its grouped pair list, Y_t -> Y_{t+1} in a second
//                           buffer (no launch reads what it writes; no atomics: bitwise reproducible).
//
// Philox counter layout (philox4x32_10, key = (seed.lo, seed.hi), the draw is output word 0):
//   counter = (row, (kind << 16) | slot, candidate, attempt)
//     kind 0 = MN   slot 0..n_MN-1, candidate 0..5, attempt 0
//     kind 1 = FP   slot 0..n_FP-1, candidate 0,    attempt 0, 1, ... (a rejected draw takes the next attempt)
//     kind 2 = the "random" init (host side, embedding.py): slot = component, words 0 and 1 feed one Box-Muller pair
//   uniform -> index in [0, M): floor(u32 * M / 2^32)
//   MN: M = N - 1, index j' -> row j' + (j' >= row) (the other N - 1 rows); FP: M = bank rows, rejected when it is the
//   row itself (fit), one of the row's NB partners, or an FP partner drawn before.
#include "common.hpp"
#include "philox.hpp"

namespace {

// ---- kNN ---------------------------------------------------------------------------------------------------------------
constexpr int kKnnWaves = 8;                      // waves per workgroup
constexpr int kKnnQW = 8;                         // queries per wave
constexpr int kKnnQT = kKnnWaves * kKnnQW;        // 64 queries per workgroup
constexpr int kKnnBT = RUNIA_WAVE;                // bank rows per chunk: one per lane
constexpr int kKnnDC = 64;                        // feature columns staged at a time
constexpr int kKnnSlots = RUNIA_PACMAP_MAX_K / RUNIA_WAVE;  // list entries per lane: position p = slot * 64 + lane

__device__ __forceinline__ bool key_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

__device__ __forceinline__ float readlane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// A workgroup owns 64 queries; wave w keeps the sorted lists of queries 8w .. 8w+7 (kKnnSlots entries per lane each).  Per
// chunk of 64 bank rows, lane l accumulates the squared distances of bank row b0 + l to its wave's 8 queries (query columns
// as broadcast LDS reads, bank row from a padded LDS tile), then each query's wave inserts the candidates that beat its K-th
// entry one at a time (lowest lane first; the key order is total, so the result does not depend on the insertion order).
__global__ void __launch_bounds__(kKnnWaves * RUNIA_WAVE) pacmap_knn_kernel(
    const float* __restrict__ q, int64_t Q, const float* __restrict__ bank, int64_t N, int64_t D, int K, int exclude_self,
    int* __restrict__ out_idx, float* __restrict__ out_dist) {
  __shared__ float qs[kKnnDC][kKnnQT];        // query tile, column-major: a wave's 8 queries of one column are adjacent
  __shared__ float bs[kKnnBT][kKnnDC + 1];    // bank tile, padded rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * kKnnQT;
  const int64_t qw = q0 + wave * kKnnQW;      // first query of this wave

  float ld[kKnnQW][kKnnSlots];
  int li[kKnnQW][kKnnSlots];
#pragma unroll
  for (int j = 0; j < kKnnQW; ++j)
#pragma unroll
    for (int s = 0; s < kKnnSlots; ++s) { ld[j][s] = INFINITY; li[j][s] = 0x7fffffff; }
  const int ks = (K - 1) >> 6, kl = (K - 1) & 63;  // slot and lane of the K-th entry
  const bool q_resident = D <= kKnnDC;

  for (int64_t b0 = 0; b0 < N; b0 += kKnnBT) {
    float acc[kKnnQW];
#pragma unroll
    for (int j = 0; j < kKnnQW; ++j) acc[j] = 0.f;
    for (int64_t k0 = 0; k0 < D; k0 += kKnnDC) {
      const int kc = (int)min<int64_t>(kKnnDC, D - k0);
      __syncthreads();
      if (!q_resident || b0 == 0) {
        for (int e = tid; e < kKnnQT * kKnnDC; e += kKnnWaves * RUNIA_WAVE) {
          const int r = e / kKnnDC, c = e % kKnnDC;
          const int64_t gq = q0 + r;
          qs[c][r] = (gq < Q && c < kc) ? q[gq * D + k0 + c] : 0.f;
        }
      }
      for (int e = tid; e < kKnnBT * kKnnDC; e += kKnnWaves * RUNIA_WAVE) {
        const int r = e / kKnnDC, c = e % kKnnDC;
        const int64_t gb = b0 + r;
        bs[r][c] = (gb < N && c < kc) ? bank[gb * D + k0 + c] : 0.f;
      }
      __syncthreads();
      for (int c = 0; c < kc; ++c) {
        const float b = bs[lane][c];
        const float4 qa = *reinterpret_cast<const float4*>(&qs[c][wave * kKnnQW]);
        const float4 qb = *reinterpret_cast<const float4*>(&qs[c][wave * kKnnQW + 4]);
        const float qv[kKnnQW] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
        for (int j = 0; j < kKnnQW; ++j) {
          const float d = qv[j] - b;
          acc[j] = fmaf(d, d, acc[j]);
        }
      }
    }
    const int64_t m = b0 + lane;
    const int mi = (int)m;
#pragma unroll
    for (int j = 0; j < kKnnQW; ++j) {
      const int64_t qi = qw + j;
      if (qi >= Q) continue;  // wave-uniform
      const float dj = acc[j] == acc[j] ? acc[j] : INFINITY;  // a NaN row ranks last but still fills the list
      const bool valid = m < N && !(exclude_self && m == qi);
      float thr_d = readlane_f(ks == 0 ? ld[j][0] : (ks == 1 ? ld[j][1] : ld[j][2]), kl);
      int thr_i = __builtin_amdgcn_readlane(ks == 0 ? li[j][0] : (ks == 1 ? li[j][1] : li[j][2]), kl);
      bool pass = valid && key_less(dj, mi, thr_d, thr_i);
      uint64_t mask = __ballot(pass);
      while (mask) {
        const int c = __builtin_ctzll(mask);
        const float cd = readlane_f(dj, c);
        const int ci = __builtin_amdgcn_readlane(mi, c);
        int pos = 0;
#pragma unroll
        for (int s = 0; s < kKnnSlots; ++s) pos += __popcll(__ballot(key_less(ld[j][s], li[j][s], cd, ci)));
        float pd[kKnnSlots];
        int pi[kKnnSlots];
#pragma unroll
        for (int s = 0; s < kKnnSlots; ++s) {
          // the entry at position p - 1: the lane below, or lane 63 of the slot below for lane 0
          const float up_d = __shfl_up(ld[j][s], 1, 64);
          const int up_i = __shfl_up(li[j][s], 1, 64);
          const float wrap_d = s > 0 ? readlane_f(ld[j][s > 0 ? s - 1 : 0], 63) : INFINITY;
          const int wrap_i = s > 0 ? __builtin_amdgcn_readlane(li[j][s > 0 ? s - 1 : 0], 63) : 0x7fffffff;
          pd[s] = lane == 0 ? wrap_d : up_d;
          pi[s] = lane == 0 ? wrap_i : up_i;
        }
#pragma unroll
        for (int s = 0; s < kKnnSlots; ++s) {
          const int p = s * 64 + lane;
          if (p == pos) { ld[j][s] = cd; li[j][s] = ci; }
          else if (p > pos) { ld[j][s] = pd[s]; li[j][s] = pi[s]; }
        }
        thr_d = readlane_f(ks == 0 ? ld[j][0] : (ks == 1 ? ld[j][1] : ld[j][2]), kl);
        thr_i = __builtin_amdgcn_readlane(ks == 0 ? li[j][0] : (ks == 1 ? li[j][1] : li[j][2]), kl);
        mask &= mask - 1;
        mask &= __ballot(pass && key_less(dj, mi, thr_d, thr_i));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kKnnQW; ++j) {
    const int64_t qi = qw + j;
    if (qi >= Q) continue;
#pragma unroll
    for (int s = 0; s < kKnnSlots; ++s) {
      const int p = s * 64 + lane;
      if (p < K) {
        out_idx[qi * K + p] = li[j][s];
        out_dist[qi * K + p] = sqrtf(ld[j][s]);
      }
    }
  }
}

// ---- pairs -------------------------------------------------------------------------------------------------------------
constexpr int kPairWaves = 4;  // one wave per row

__device__ __forceinline__ uint32_t draw_word(uint64_t seed, uint32_t row, uint32_t kind, uint32_t slot, uint32_t cand,
                                              uint32_t attempt) {
  return runia_philox::philox4x32_10(row, (kind << 16) | slot, cand, attempt, (uint32_t)seed, (uint32_t)(seed >> 32)).x;
}

__device__ __forceinline__ int64_t draw_index(uint32_t u, int64_t m) { return (int64_t)(((uint64_t)u * (uint64_t)m) >> 32); }

// sig_i = max(mean(d_i[3 : min(6, K)]), 1e-10); 1e-10 when K <= 3
__global__ void pacmap_sig_kernel(const float* __restrict__ dist, int64_t N, int K, float* __restrict__ sig) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int hi = K < 6 ? K : 6;
  float s = 0.f;
  for (int p = 3; p < hi; ++p) s += dist[i * K + p];
  const float m = hi > 3 ? s / (float)(hi - 3) : 0.f;
  sig[i] = m > 1e-10f ? m : 1e-10f;
}

__device__ __forceinline__ float sq_dist_rows(const float* __restrict__ a, const float* __restrict__ b, int64_t D) {
  float s = 0.f;
  for (int64_t k = 0; k < D; ++k) {
    const float d = a[k] - b[k];
    s = fmaf(d, d, s);
  }
  return s;
}

__global__ void __launch_bounds__(kPairWaves * RUNIA_WAVE) pacmap_pairs_kernel(
    const float* __restrict__ x, int64_t R, const float* __restrict__ bank, int64_t Nb, int64_t D,
    const int* __restrict__ knn_idx, const float* __restrict__ knn_dist, int K, const float* __restrict__ sig, int n_nb,
    int n_mn, int n_fp, uint64_t seed, int transform, int* __restrict__ pair_nb, int* __restrict__ pair_mn,
    int* __restrict__ pair_fp) {
  __shared__ float sc[kPairWaves][RUNIA_PACMAP_MAX_K];
  __shared__ int nb[kPairWaves][RUNIA_PACMAP_MAX_K];
  __shared__ float mdist[kPairWaves][RUNIA_PACMAP_MAX_MN * 6];
  __shared__ int midx[kPairWaves][RUNIA_PACMAP_MAX_MN * 6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kPairWaves + wave;
  const bool live = i < R;  // wave-uniform; every wave still reaches the barriers

  // NB: scaled distance d^2 / sig_i / sig_j (fit) or the plain candidate order (transform); rank = number of candidates
  // before it in (scaled, candidate position) order
  if (live) {
    const float si = transform ? 1.f : sig[i];
    for (int c = lane; c < K; c += 64) {
      const float d = knn_dist[i * K + c];
      const int j = min(max(knn_idx[i * K + c], 0), (int)(Nb - 1));  // (always in range for a table of the kNN kernel)
      sc[wave][c] = transform ? (float)c : (d * d / si) / sig[j];
    }
  }
  __syncthreads();
  if (live) {
    for (int c = lane; c < K; c += 64) {
      const float v = sc[wave][c];
      int rank = 0;
      for (int c2 = 0; c2 < K; ++c2) {
        const float w = sc[wave][c2];
        rank += (w < v || (w == v && c2 < c)) ? 1 : 0;
      }
      if (rank < n_nb) {
        const int j = min(max(knn_idx[i * K + c], 0), (int)(Nb - 1));
        nb[wave][rank] = j;
        pair_nb[(i * n_nb + rank) * 2 + 0] = (int)i;
        pair_nb[(i * n_nb + rank) * 2 + 1] = j;
      }
    }
  }
  // MN: 6 draws among the other rows, the second closest (ties: earlier draw)
  if (live && !transform) {
    const int ne = n_mn * 6;
    for (int e = lane; e < ne; e += 64) {
      const int slot = e / 6, cand = e % 6;
      const int64_t jp = draw_index(draw_word(seed, (uint32_t)i, 0u, (uint32_t)slot, (uint32_t)cand, 0u), Nb - 1);
      const int64_t j = jp + (jp >= i ? 1 : 0);
      midx[wave][e] = (int)j;
      mdist[wave][e] = sq_dist_rows(x + i * D, bank + j * D, D);
    }
  }
  __syncthreads();
  if (!live) return;  // no barrier below
  if (!transform) {
    for (int slot = lane; slot < n_mn; slot += 64) {
      int pick = 0;
      for (int c = 0; c < 6; ++c) {
        const float v = mdist[wave][slot * 6 + c];
        int rank = 0;
        for (int c2 = 0; c2 < 6; ++c2) {
          const float w = mdist[wave][slot * 6 + c2];
          rank += (w < v || (w == v && c2 < c)) ? 1 : 0;
        }
        if (rank == 1) pick = c;
      }
      pair_mn[(i * n_mn + slot) * 2 + 0] = (int)i;
      pair_mn[(i * n_mn + slot) * 2 + 1] = midx[wave][slot * 6 + pick];
    }
  }
  // FP: the whole wave draws the same candidate; lanes test it against their share of the NB partners (LDS) and of the FP
  // partners accepted so far (registers: FP slot f lives in lane f % 64, register f / 64)
  int nbr[RUNIA_PACMAP_MAX_K / 64];
#pragma unroll
  for (int r = 0; r < RUNIA_PACMAP_MAX_K / 64; ++r) {
    const int p = r * 64 + lane;
    nbr[r] = p < n_nb ? nb[wave][p] : -1;
  }
  int fpr[RUNIA_PACMAP_MAX_FP / 64];
#pragma unroll
  for (int r = 0; r < RUNIA_PACMAP_MAX_FP / 64; ++r) fpr[r] = -1;
  for (int f = 0; f < n_fp; ++f) {
    int64_t j = 0;
    for (uint32_t a = 0;; ++a) {
      j = draw_index(draw_word(seed, (uint32_t)i, 1u, (uint32_t)f, 0u, a), Nb);
      bool hit = false;
#pragma unroll
      for (int r = 0; r < RUNIA_PACMAP_MAX_K / 64; ++r) hit |= nbr[r] == (int)j;
#pragma unroll
      for (int r = 0; r < RUNIA_PACMAP_MAX_FP / 64; ++r) hit |= fpr[r] == (int)j;
      const bool reject = (!transform && j == i) || __ballot(hit) != 0ull;
      // a bounded search: the caller guarantees n_FP free rows, so 2^20 rejections in a row do not happen in practice;
      // the bound only keeps a bad argument from spinning (the last draw, a valid row index, is then kept)
      if (!reject || a >= (1u << 20)) break;
    }
    if ((f & 63) == lane) {
#pragma unroll
      for (int r = 0; r < RUNIA_PACMAP_MAX_FP / 64; ++r)
        if (r == (f >> 6)) fpr[r] = (int)j;
    }
    if (lane == 0) {
      pair_fp[(i * n_fp + f) * 2 + 0] = (int)i;
      pair_fp[(i * n_fp + f) * 2 + 1] = (int)j;
    }
  }
}

// ---- one Adam iteration ------------------------------------------------------------------------------------------------
constexpr int kStepLanes = 16;  // lanes per row: entries strided over them, then a fixed butterfly sum
constexpr int kStepThreads = 256;

struct StepConsts {
  float w_nb, w_mn, w_fp, lr_t, b1c, b2c, eps;  // b1c = 1 - beta1, b2c = 1 - beta2
};

// C > 0: compile-time components; C == 0: run-time nc <= 16
template <int C>
__global__ void __launch_bounds__(kStepThreads) pacmap_step_kernel(
    const float* __restrict__ y_in, const float* __restrict__ y_part, float* __restrict__ y_out, float* __restrict__ m_buf,
    float* __restrict__ v_buf, const int64_t* __restrict__ offsets, const int* __restrict__ entries, int64_t R, int nc_rt,
    StepConsts k) {
  constexpr int CM = C > 0 ? C : RUNIA_PACMAP_MAX_COMPONENTS;
  const int nc = C > 0 ? C : nc_rt;
  const int sub = threadIdx.x % kStepLanes;
  const int64_t r = ((int64_t)blockIdx.x * kStepThreads + threadIdx.x) / kStepLanes;
  const bool live = r < R;
  float yi[CM], g[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    yi[c] = (live && c < nc) ? y_in[r * nc + c] : 0.f;
    g[c] = 0.f;
  }
  if (live) {
    const int64_t e1 = offsets[r + 1];
    for (int64_t e = offsets[r] + sub; e < e1; e += kStepLanes) {
      const int ent = entries[e];
      const int kind = (int)((unsigned)ent >> 30);
      const int64_t p = ent & 0x3fffffff;
      float dy[CM];
      float d = 1.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        dy[c] = c < nc ? yi[c] - y_part[p * nc + c] : 0.f;
        d = fmaf(dy[c], dy[c], d);
      }
      float w;
      if (kind == RUNIA_PACMAP_KIND_NB) {
        const float t = 10.f + d;
        w = k.w_nb * (20.f / (t * t));
      } else if (kind == RUNIA_PACMAP_KIND_MN) {
        const float t = 10000.f + d;
        w = k.w_mn * (20000.f / (t * t));
      } else {
        const float t = 1.f + d;
        w = -k.w_fp * (2.f / (t * t));  // repels
      }
#pragma unroll
      for (int c = 0; c < CM; ++c) g[c] = fmaf(w, dy[c], g[c]);
    }
  }
#pragma unroll  // (hand-written: the butterfly runs from 1 up, wave_reduce adds from the widest step down)
  for (int o = 1; o < kStepLanes; o <<= 1)
#pragma unroll
    for (int c = 0; c < CM; ++c) g[c] += lane_xor(g[c], o);
  if (!live || sub >= nc) return;
  // lane `sub` updates component `sub` (registers are indexed statically)
  float gc = 0.f, yc = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c == sub) { gc = g[c]; yc = yi[c]; }
  const int64_t o = r * nc + sub;
  float m = m_buf[o], v = v_buf[o];
  m = m + k.b1c * (gc - m);
  v = v + k.b2c * (gc * gc - v);
  m_buf[o] = m;
  v_buf[o] = v;
  y_out[o] = yc - k.lr_t * m / (sqrtf(v) + k.eps);
}

}  // namespace

extern "C" int runia_pacmap_knn_f32(const float* q, int64_t Q, const float* bank, int64_t N, int64_t D, int K,
                                    int exclude_self, int32_t* idx, float* dist, runia_stream_t stream) {
  if (Q < 0 || N < 1 || D < 1 || K < 1 || K > RUNIA_PACMAP_MAX_K || N > 0x7fffffffll || K > N - (exclude_self ? 1 : 0) ||
      (exclude_self && Q > N) || (Q > 0 && (!q || !bank || !idx || !dist)))
    return RUNIA_E_INVALID;
  if (Q == 0) return RUNIA_OK;
  const int64_t blocks = (Q + kKnnQT - 1) / kKnnQT;
  RUNIA_LAUNCH_TIMED(pacmap_knn_kernel, dim3((unsigned)blocks), dim3(kKnnWaves * RUNIA_WAVE), 0, as_stream(stream), q, Q,
                     bank, N, D, K, exclude_self, idx, dist);
  return runia_check_launch();
}

extern "C" size_t runia_pacmap_pairs_workspace_bytes(int64_t R) { return R > 0 ? (size_t)R * sizeof(float) : 0; }

extern "C" int runia_pacmap_pairs(const float* x, int64_t R, const float* bank, int64_t Nb, int64_t D, const int32_t* knn_idx,
                                  const float* knn_dist, int K, int n_nb, int n_mn, int n_fp, uint64_t seed, int transform,
                                  int32_t* pair_nb, int32_t* pair_mn, int32_t* pair_fp, void* workspace,
                                  size_t workspace_bytes, runia_stream_t stream) {
  if (R < 0 || Nb < 2 || D < 1 || K < 1 || K > RUNIA_PACMAP_MAX_K || n_nb < 1 || n_nb > K || n_mn < 0 ||
      n_mn > RUNIA_PACMAP_MAX_MN || n_fp < 0 || n_fp > RUNIA_PACMAP_MAX_FP || Nb > RUNIA_PACMAP_MAX_ROWS ||
      R > RUNIA_PACMAP_MAX_ROWS || (transform && n_mn != 0) || (!transform && R != Nb) ||
      n_fp > Nb - n_nb - (transform ? 0 : 1) || (R > 0 && (!x || !bank || !knn_idx || !knn_dist || !pair_nb)) ||
      (R > 0 && n_mn > 0 && !pair_mn) || (R > 0 && n_fp > 0 && !pair_fp))
    return RUNIA_E_INVALID;
  if (R == 0) return RUNIA_OK;
  if (!transform && ws_refused(workspace, workspace_bytes, runia_pacmap_pairs_workspace_bytes(R), 1)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  float* sig = reinterpret_cast<float*>(workspace);
  if (!transform)
    RUNIA_LAUNCH_TIMED(pacmap_sig_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, knn_dist, R, K, sig);
  RUNIA_LAUNCH_TIMED(pacmap_pairs_kernel, dim3((unsigned)((R + kPairWaves - 1) / kPairWaves)), dim3(kPairWaves * RUNIA_WAVE),
                     0, s, x, R, bank, Nb, D, knn_idx, knn_dist, K, transform ? nullptr : sig, n_nb, n_mn, n_fp, seed,
                     transform, pair_nb, pair_mn, pair_fp);
  return runia_check_launch();
}

extern "C" int runia_pacmap_phase_weights(int t, float* w) {
  if (!w || t < 0) return RUNIA_E_INVALID;
  if (t < 100) {
    const float f = (float)t / 100.f;
    w[0] = 2.f; w[1] = (1.f - f) * 1000.f + f * 3.f; w[2] = 1.f;
  } else if (t < 200) {
    w[0] = 3.f; w[1] = 3.f; w[2] = 1.f;
  } else {
    w[0] = 1.f; w[1] = 0.f; w[2] = 1.f;
  }
  return RUNIA_OK;
}

extern "C" int runia_pacmap_step_f32(const float* y_in, const float* y_part, float* y_out, float* m, float* v,
                                     const int64_t* offsets, const int32_t* entries, int64_t R, int n_components, int t,
                                     float lr, runia_stream_t stream) {
  if (R < 0 || n_components < 1 || n_components > RUNIA_PACMAP_MAX_COMPONENTS || t < 0 ||
      (R > 0 && (!y_in || !y_part || !y_out || !m || !v || !offsets || !entries)) || y_out == y_in || y_out == y_part)
    return RUNIA_E_INVALID;
  if (R == 0) return RUNIA_OK;
  float w[3];
  runia_pacmap_phase_weights(t, w);
  StepConsts k;
  k.w_nb = w[0]; k.w_mn = w[1]; k.w_fp = w[2];
  k.lr_t = (float)((double)lr * sqrt(1.0 - pow(0.999, t + 1)) / (1.0 - pow(0.9, t + 1)));
  k.b1c = 0.1f; k.b2c = 0.001f; k.eps = 1e-7f;
  const int64_t blocks = (R * kStepLanes + kStepThreads - 1) / kStepThreads;
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)blocks), block(kStepThreads);
  if (n_components == 2)
    RUNIA_LAUNCH_TIMED(pacmap_step_kernel<2>, grid, block, 0, s, y_in, y_part, y_out, m, v, offsets, entries, R, 2, k);
  else if (n_components == 3)
    RUNIA_LAUNCH_TIMED(pacmap_step_kernel<3>, grid, block, 0, s, y_in, y_part, y_out, m, v, offsets, entries, R, 3, k);
  else
    RUNIA_LAUNCH_TIMED(pacmap_step_kernel<0>, grid, block, 0, s, y_in, y_part, y_out, m, v, offsets, entries, R,
                       n_components, k);
  return runia_check_launch();
}
