// Conformal prediction sets (evaluation/conformal.py): LAC, APS and RAPS scores from one read of the logits.
//   runia_conformal_label_scores: the score s_y and the rank r_y of every row's label (the calibration half: no sort)
//   runia_conformal_sets        : the set {c : s_c <= qhat} of every row: its size, its members as packed bits, whether it holds
//                                 the label.  The row is ordered inside the workgroup in LDS (order.hpp).
//   runia_conformal_reduce      : size / covered / labels -> an integer record (counts, size histogram, per-class counts)
// With m the row maximum, e_k = exp(beta (x_k - m)), S0 = sum e_k, p_k = e_k / S0; classes ordered by logit, descending, equal
// logits by lower index first; r_c the 1-based rank of c and B_c the sum of p_k over the classes ordered before c:
//   lac  s_c = 1 - p_c      aps  s_c = B_c + u p_c      raps  s_c = B_c + u p_c + lam max(0, r_c - k_reg)
// A class at -inf has p = 0 and is ordered last (among its like by index).  A row with a NaN or +inf logit, or with no finite
// logit, has no softmax: NaN scores, rank 0, size 0, no members, not covered.
#include "common.hpp"
#include "elem.hpp"
#include "conformal_core.hpp"

namespace {

constexpr int kMaxSetClasses = 8192;  // runia_conformal_sets: the row's keys and indices in 48 KB of LDS

// ---- label scores ----------------------------------------------------------------------------------------------------------
struct Acc {
  float s0, a;  // sum e_k, sum of e_k over the classes ordered before the label
  int before;
};

__device__ __forceinline__ void acc_take(Acc& c, float x, int k, float m, float beta, float xy, int y) {
  const float e = softmax_term(x, m, beta);
  const bool first = x > xy || (x == xy && k < y);
  c.s0 += e;
  c.a += first ? e : 0.f;
  c.before += first ? 1 : 0;
}

__device__ __forceinline__ void finish_label(const Method& M, const float* u, float* score, int32_t* rank, int64_t row, float m,
                                             const Acc& c, float xy, bool used) {
  const bool ok = used && c.s0 > 0.f && c.s0 < INFINITY;  // (a NaN fails both)
  float s = __builtin_nanf("");
  if (ok) {
    const float r = 1.f / c.s0;
    s = score_of(M, softmax_term(xy, m, M.beta) * r, c.a * r, u ? u[row] : 1.f, c.before + 1);
  }
  if (score) score[row] = s;
  if (rank) rank[row] = ok ? c.before + 1 : 0;
}

// C <= 64: one row per lane, the tile widened into LDS with coalesced loads, odd row pitch (calib_small_kernel)
constexpr int kSmallRows = 128;

template <class T>
__global__ __launch_bounds__(kSmallRows) void conformal_label_small_kernel(const typename T::elem* __restrict__ x, int64_t stride,
                                                                           Labels L, const float* __restrict__ u, Method M,
                                                                           float* __restrict__ score, int32_t* __restrict__ rank,
                                                                           int64_t N, int C) {
  extern __shared__ float tile[];  // kSmallRows * (C | 1) floats
  const int tid = threadIdx.x, pitch = C | 1;
  for (int64_t r0 = (int64_t)blockIdx.x * kSmallRows; r0 < N; r0 += (int64_t)gridDim.x * kSmallRows) {
    const int rows = (int)((N - r0 < kSmallRows) ? (N - r0) : kSmallRows);
    const int total = rows * C;
    __syncthreads();
    for (int i = tid; i < total; i += kSmallRows) {
      const int r = i / C, k = i - r * C;
      tile[r * pitch + k] = ld1<T>(x + (r0 + r) * stride + k);
    }
    __syncthreads();
    if (tid < rows) {
      const float* row = tile + tid * pitch;
      bool used;
      const int y = row_class(L, r0 + tid, C, used);
      const float xy = row[y];
      float m = -INFINITY;
      for (int k = 0; k < C; ++k) m = fmaxf(m, row[k]);
      Acc c = {0.f, 0.f, 0};
      for (int k = 0; k < C; ++k) acc_take(c, row[k], k, m, M.beta, xy, y);
      finish_label(M, u, score, rank, r0 + tid, m, c, xy, used);
    }
  }
}

// elements 4 i .. 4 i + 3 of a row of C: one aligned load (VEC) or four guarded ones; -inf beyond the row (it adds nothing and
// is ordered before no class).  The lane-to-element map is the same in both forms, so the sums are as well.
template <class T, bool VEC>
__device__ __forceinline__ void ld_quad(const typename T::elem* p, int64_t i, int64_t C, float* v) {
  if constexpr (VEC) {
    if constexpr (T::kBytes == 4) ld16<T>(p + 4 * i, v);
    else ld8<T>(p + 4 * i, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (4 * i + j < C) ? ld1<T>(p + 4 * i + j) : -INFINITY;
  }
}

// C > 64: one wave per row, four consecutive elements per lane and load.
//   NCH > 0 : NCH loads per lane, the row in registers: maximum first, then the sums (C <= 256 NCH)
//   NCH == 0: any C in one pass, four loads at a time; a lane moves its running maximum and rescales its sums when it does,
//             and the lanes' sums are rescaled once more to the wave's maximum before they are added (calib_wave_kernel)
template <class T, int NCH, bool VEC>
__global__ __launch_bounds__(64 * kRowWaves) void conformal_label_wave_kernel(const typename T::elem* __restrict__ x,
                                                                             int64_t stride, Labels L,
                                                                             const float* __restrict__ u, Method M,
                                                                             float* __restrict__ score,
                                                                             int32_t* __restrict__ rank, int64_t N, int64_t C) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * kRowWaves;
  const int64_t n4 = (C + 3) >> 2;  // loads per row
  for (int64_t row = (int64_t)blockIdx.x * kRowWaves + wave; row < N; row += wave_stride) {
    const typename T::elem* p = x + row * stride;
    bool used;
    const int y = row_class(L, row, C, used);
    const float xy = ld1<T>(p + y);
    float m = -INFINITY;
    Acc c = {0.f, 0.f, 0};
    if constexpr (NCH > 0) {
      float v[NCH][4];
#pragma unroll
      for (int q = 0; q < NCH; ++q) {
        const int i = lane + 64 * q;
        if (i < n4) ld_quad<T, VEC>(p, i, C, v[q]);
        else v[q][0] = v[q][1] = v[q][2] = v[q][3] = -INFINITY;
      }
#pragma unroll
      for (int q = 0; q < NCH; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, v[q][j]);
      }
      m = wave_max_f32(m);
#pragma unroll
      for (int q = 0; q < NCH; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc_take(c, v[q][j], 4 * (lane + 64 * q) + j, m, M.beta, xy, y);
      }
    } else {
      constexpr int U = 4;
      for (int64_t i0 = 0; i0 < n4; i0 += 64 * U) {
        float v[U][4];
#pragma unroll
        for (int q = 0; q < U; ++q) {
          const int64_t i = i0 + lane + 64 * q;
          if (i < n4) ld_quad<T, VEC>(p, i, C, v[q]);
          else v[q][0] = v[q][1] = v[q][2] = v[q][3] = -INFINITY;
        }
        const float m_old = m;
#pragma unroll
        for (int q = 0; q < U; ++q) {
#pragma unroll
          for (int j = 0; j < 4; ++j) m = fmaxf(m, v[q][j]);
        }
        if (m > m_old && m_old != -INFINITY) {  // (sums of a lane without a finite logit yet: 0 or NaN)
          const float f = exp_nonpos(-M.beta * (m - m_old));
          c.s0 *= f;
          c.a *= f;
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
#pragma unroll
          for (int j = 0; j < 4; ++j) acc_take(c, v[q][j], (int)(4 * (i0 + lane + 64 * q) + j), m, M.beta, xy, y);
        }
      }
      const float m_lane = m;
      m = wave_max_f32(m);
      if (m > m_lane && m_lane != -INFINITY) {
        const float f = exp_nonpos(-M.beta * (m - m_lane));
        c.s0 *= f;
        c.a *= f;
      }
    }
    c.s0 = wave_sum_f32(c.s0);
    c.a = wave_sum_f32(c.a);
    c.before = wave_sum(c.before);
    if (lane == 0) finish_label(M, u, score, rank, row, m, c, xy, used);
  }
}

template <class T>
int launch_label(const void* logits, int64_t stride, const Labels& L, const float* u, const Method& M, float* score,
                 int32_t* rank, int64_t N, int64_t C, hipStream_t s) {
  const typename T::elem* x = static_cast<const typename T::elem*>(logits);
  if (C <= 64) {
    const size_t shmem = (size_t)kSmallRows * (C | 1) * sizeof(float);
    conformal_label_small_kernel<T><<<runia_stream_grid(N, kSmallRows), kSmallRows, shmem, s>>>(x, stride, L, u, M, score, rank,
                                                                                                 N, (int)C);
    return runia_check_launch();
  }
  const unsigned grid = runia_rows_grid(N);
  constexpr int kT = 64 * kRowWaves;
  // one load of four elements: every row as aligned as the first, and whole
  const bool vec = ((C & 3) == 0) && ((stride & 3) == 0) && ((((uintptr_t)logits) & (uintptr_t)(4 * T::kBytes - 1)) == 0);
  const int64_t n4 = (C + 3) >> 2;
#define RUNIA_CONF_LABEL(NCH)                                                                                      \
  do {                                                                                                             \
    if (vec) conformal_label_wave_kernel<T, NCH, true><<<grid, kT, 0, s>>>(x, stride, L, u, M, score, rank, N, C); \
    else conformal_label_wave_kernel<T, NCH, false><<<grid, kT, 0, s>>>(x, stride, L, u, M, score, rank, N, C);    \
  } while (0)
  if (n4 <= 64) RUNIA_CONF_LABEL(1);
  else if (n4 <= 128) RUNIA_CONF_LABEL(2);
  else if (n4 <= 256) RUNIA_CONF_LABEL(4);
  else if (n4 <= 512) RUNIA_CONF_LABEL(8);
  else RUNIA_CONF_LABEL(0);
#undef RUNIA_CONF_LABEL
  return runia_check_launch();
}

// ---- sets ------------------------------------------------------------------------------------------------------------------
// A group of TPR threads owns a row; a workgroup of 256 threads holds 256 / TPR rows.  P = max(TPR, C rounded up to a power of
// two) slots per row in LDS: key[P] (uint32: ascending key order is descending logit order), idx[P] (uint16), then the set's
// bits.  Every thread of the workgroup meets every barrier: P and the trip counts depend on C alone.
//   1. load: slot i <- class i (coalesced), the padding slots sort last; the group's maximum and NaN flag
//   2. order (aps, raps): lds_bitonic_sort on (key, idx), P / 2 compare-exchanges per step
//   3. sums: a thread owns P / TPR consecutive slots: e of each (written over the key), the thread's sum, the group's exclusive
//      scan of those sums -> S0 and the thread's offset
//   4. sets: s of each slot from the running sum, the compare with qhat, the bit of its class (integer atomic-or in LDS)
//   5. out: the words, size = their popcount, covered = the label's bit
template <int TPR>
struct Group {
  static constexpr int kWidth = TPR < 64 ? TPR : 64;  // lanes of one wave that belong to the group
  static constexpr int kWaves = TPR / kWidth;
};

template <int TPR>
__device__ __forceinline__ float group_max(float v, float* red) {
  using G = Group<TPR>;
  v = wave_reduce<G::kWidth>(v, [](float a, float b) { return fmaxf(a, b); });
  if constexpr (G::kWaves > 1) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < G::kWaves; ++w) v = fmaxf(v, red[w]);
  }
  return v;
}

template <int TPR>
__device__ __forceinline__ int group_sum(int v, int* red) {
  using G = Group<TPR>;
  v = wave_sum<G::kWidth>(v);
  if constexpr (G::kWaves > 1) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < G::kWaves; ++w) v += red[w];
  }
  return v;
}

// the sum of v over the group's threads before this one, and over all of them: a fixed order
template <int TPR>
__device__ __forceinline__ float group_exclusive_scan(float v, float& total, float* red) {
  using G = Group<TPR>;
  const int l = threadIdx.x & (G::kWidth - 1);
  float inc = v;
#pragma unroll
  for (int o = 1; o < G::kWidth; o <<= 1) {
    const float t = __shfl_up(inc, o, G::kWidth);
    inc = (l >= o) ? inc + t : inc;
  }
  const float prev = __shfl_up(inc, 1, G::kWidth);
  float excl = (l >= 1) ? prev : 0.f;
  total = __shfl(inc, G::kWidth - 1, G::kWidth);
  if constexpr (G::kWaves > 1) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) red[w] = inc;
    __syncthreads();
    float off = 0.f, all = 0.f;
#pragma unroll
    for (int i = 0; i < G::kWaves; ++i) {
      off = (i == w) ? all : off;
      all += red[i];
    }
    excl = off + excl;
    total = all;
  }
  return excl;
}

template <class T, int TPR>
__global__ __launch_bounds__(256) void conformal_sets_kernel(const typename T::elem* __restrict__ x, int64_t stride, Labels L,
                                                             const float* __restrict__ u, Method M, float qhat,
                                                             int32_t* __restrict__ size, int32_t* __restrict__ members,
                                                             uint8_t* __restrict__ covered, int64_t N, int C, int P) {
  constexpr int R = 256 / TPR;  // rows per workgroup
  extern __shared__ uint32_t lds[];
  __shared__ float red_m[4], red_f[4];
  __shared__ int red_b[4], red_n[4];
  const int g = threadIdx.x / TPR, t = threadIdx.x % TPR;
  const int PW = (P + 31) >> 5, W = (C + 31) >> 5;
  uint32_t* key = lds + (size_t)g * P;
  uint16_t* idx = reinterpret_cast<uint16_t*>(lds + (size_t)R * P) + (size_t)g * P;
  uint32_t* bits = lds + (size_t)R * P + (size_t)R * P / 2 + (size_t)g * PW;
  const int E = P / TPR;  // slots per thread in steps 3 and 4
  for (int64_t base = (int64_t)blockIdx.x * R; base < N; base += (int64_t)gridDim.x * R) {
    const int64_t row = base + g;
    const bool live = row < N;
    // 1. load
    float m = -INFINITY;
    int bad = 0;
    const typename T::elem* p = x + (live ? row : 0) * stride;
    for (int i = t; i < P; i += TPR) {
      uint32_t k = 0xffffffffu;
      if (live && i < C) {
        const float v = ld1<T>(p + i);
        m = fmaxf(m, v);
        bad |= (v != v) ? 1 : 0;
        k = descending_key(v);
      }
      key[i] = k;
      idx[i] = (uint16_t)i;
    }
    for (int w = t; w < PW; w += TPR) bits[w] = 0u;
    m = group_max<TPR>(m, red_m);
    bad = group_sum<TPR>(bad, red_b);
    const bool ok = live && bad == 0 && m > -INFINITY && m < INFINITY;
    __syncthreads();
    // 2. order
    if (M.kind != kLac) {
      lds_bitonic_sort(P, t, TPR, [&](int lo, int hi, bool up) {
        const uint32_t ka = key[lo], kb = key[hi], ia = idx[lo], ib = idx[hi];
        if ((ka > kb || (ka == kb && ia > ib)) == up) {  // a after b: by key, ties by index
          key[lo] = kb, key[hi] = ka;
          idx[lo] = (uint16_t)ib, idx[hi] = (uint16_t)ia;
        }
      });
    }
    // 3. sums
    float mine = 0.f;
    for (int i = t * E; i < (t + 1) * E; ++i) {
      const uint32_t k = key[i];
      const float e = (k == 0xffffffffu && idx[i] >= C) ? 0.f : softmax_term(key_logit(k), m, M.beta);
      key[i] = __float_as_uint(e);
      mine += e;
    }
    float s0;
    float run = group_exclusive_scan<TPR>(mine, s0, red_f);
    // 4. sets
    if (ok) {
      const float r = 1.f / s0;
      const float ur = u ? u[row] : 1.f;
      for (int i = t * E; i < (t + 1) * E; ++i) {
        const float e = __uint_as_float(key[i]);
        const int c = idx[i];
        const float s = score_of(M, e * r, run * r, ur, i + 1);
        run += e;
        if (c < C && s <= qhat) atomicOr(&bits[c >> 5], 1u << (c & 31));
      }
    }
    __syncthreads();
    // 5. out
    int n = 0;
    for (int w = t; w < W; w += TPR) {
      const uint32_t b = bits[w];
      n += __popc(b);
      if (live && members) members[row * W + w] = (int32_t)b;
    }
    n = group_sum<TPR>(n, red_n);
    if (live && t == 0) {
      size[row] = n;
      if (covered) {
        bool used;
        const int y = row_class(L, row, C, used);
        covered[row] = (used && ((bits[y >> 5] >> (y & 31)) & 1u)) ? 1 : 0;
      }
    }
    __syncthreads();
  }
}

static inline int sets_slots(int64_t C, int tpr) {
  int p = tpr;
  while (p < C) p <<= 1;
  return p;
}

template <class T>
int launch_sets(const void* logits, int64_t stride, const Labels& L, const float* u, const Method& M, float qhat, int32_t* size,
                int32_t* members, uint8_t* covered, int64_t N, int C, hipStream_t s) {
  const typename T::elem* x = static_cast<const typename T::elem*>(logits);
#define RUNIA_CONF_SETS(TPR)                                                                                              \
  do {                                                                                                                    \
    const int P = sets_slots(C, TPR), R = 256 / TPR;                                                                      \
    const size_t shmem = (size_t)R * (6 * (size_t)P + 4 * (size_t)((P + 31) >> 5));                                       \
    conformal_sets_kernel<T, TPR><<<runia_rows_grid(N, R), 256, shmem, s>>>(x, stride, L, u, M, qhat, size, members,      \
                                                                            covered, N, C, P);                            \
  } while (0)
  if (C <= 64) RUNIA_CONF_SETS(16);
  else if (C <= 2048) RUNIA_CONF_SETS(64);
  else RUNIA_CONF_SETS(256);
#undef RUNIA_CONF_SETS
  return runia_check_launch();
}

// ---- reduce ----------------------------------------------------------------------------------------------------------------
// The record, int64: [0] rows used  [1] rows covered  [2] sum of sizes  [3 ..) hist[H]  class_count[C]  class_covered[C], with
// H = min(C + 1, 512) and the last slot of hist meaning "that size or more".  Integers only: the order of the atomics is free.
// hist, and the per-class counts up to 512 classes, are counted in LDS per workgroup and added to the record once.
constexpr int kRedThreads = 256, kMaxHist = 512, kRecHead = 3, kMaxLdsClasses = 512;
constexpr int kRedRowsPerBlock = 8 * kRedThreads;  // a workgroup walks at least that many rows, so its LDS counts pay off

__device__ __forceinline__ void add_i64(int64_t* p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

__global__ __launch_bounds__(kRedThreads) void conformal_reduce_kernel(const int32_t* __restrict__ size,
                                                                       const uint8_t* __restrict__ covered, Labels L, int64_t N,
                                                                       int64_t C, int H, int64_t* __restrict__ out) {
  __shared__ int hist[kMaxHist], cls[2][kMaxLdsClasses];
  const bool local = C <= kMaxLdsClasses;  // the per-class counts of this workgroup's rows in LDS, flushed once
  for (int i = threadIdx.x; i < H; i += kRedThreads) hist[i] = 0;
  if (local) {
    for (int i = threadIdx.x; i < (int)C; i += kRedThreads) cls[0][i] = cls[1][i] = 0;
  }
  __syncthreads();
  int64_t* class_count = out + kRecHead + H;
  int64_t* class_covered = class_count + C;
  int64_t used = 0, cov = 0, sum = 0;
  for (int64_t row = (int64_t)blockIdx.x * kRedThreads + threadIdx.x; row < N; row += (int64_t)gridDim.x * kRedThreads) {
    const int64_t y = label_at(L, row);
    if (y < 0 || y >= C || (L.has_ignore && y == L.ignore)) continue;
    const int n = size[row];
    const int hit = covered[row] ? 1 : 0;
    used += 1;
    cov += hit;
    sum += n;
    atomicAdd(&hist[n < 0 ? 0 : (n < H - 1 ? n : H - 1)], 1);
    if (local) {
      atomicAdd(&cls[0][y], 1);
      if (hit) atomicAdd(&cls[1][y], 1);
    } else {
      add_i64(class_count + y, 1);
      if (hit) add_i64(class_covered + y, 1);
    }
  }
  used = wave_sum(used);
  cov = wave_sum(cov);
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0 && used) {
    add_i64(out + 0, used);
    add_i64(out + 1, cov);
    add_i64(out + 2, sum);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += kRedThreads) {
    if (hist[i]) add_i64(out + kRecHead + i, hist[i]);
  }
  if (local) {
    for (int i = threadIdx.x; i < (int)C; i += kRedThreads) {
      if (cls[0][i]) add_i64(class_count + i, cls[0][i]);
      if (cls[1][i]) add_i64(class_covered + i, cls[1][i]);
    }
  }
}

}  // namespace

extern "C" int runia_conformal_label_scores(const void* logits, int dtype, int64_t row_stride, const void* labels,
                                            int labels_i64, int has_ignore, int64_t ignore_index, const float* u, int method,
                                            float beta, float lam, int k_reg, float* score, int32_t* rank, int64_t N, int64_t C,
                                            runia_stream_t stream) {
  if (!elem_dtype_ok(dtype) || N < 0 || C <= 0 || C > 0x7fffffffll - 2048 || row_stride < C ||
      !method_ok(method, beta, lam, k_reg))
    return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!logits || !labels || (!score && !rank)) return RUNIA_E_INVALID;
  const Labels L = {labels, labels_i64 != 0, has_ignore != 0, ignore_index};
  const Method M = {method, beta, lam, k_reg};
  hipStream_t s = as_stream(stream);
  return dispatch_elem(dtype, [&](auto tag) {
    return launch_label<decltype(tag)>(logits, row_stride, L, u, M, score, rank, N, C, s);
  });
}

extern "C" int runia_conformal_max_classes(void) { return kMaxSetClasses; }

extern "C" int runia_conformal_sets(const void* logits, int dtype, int64_t row_stride, const void* labels, int labels_i64,
                                    int has_ignore, int64_t ignore_index, const float* u, int method, float beta, float lam,
                                    int k_reg, float qhat, int32_t* size, int32_t* members, uint8_t* covered, int64_t N,
                                    int64_t C, runia_stream_t stream) {
  if (!elem_dtype_ok(dtype) || N < 0 || C <= 0 || C > kMaxSetClasses || row_stride < C || !method_ok(method, beta, lam, k_reg) ||
      qhat != qhat)
    return RUNIA_E_INVALID;
  if (covered && !labels) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!logits || !size) return RUNIA_E_INVALID;
  const Labels L = {labels, labels_i64 != 0, has_ignore != 0, ignore_index};
  const Method M = {method, beta, lam, k_reg};
  hipStream_t s = as_stream(stream);
  return dispatch_elem(dtype, [&](auto tag) {
    return launch_sets<decltype(tag)>(logits, row_stride, L, u, M, qhat, size, members, covered, N, (int)C, s);
  });
}

extern "C" int64_t runia_conformal_record_slots(int64_t C) {
  if (C <= 0 || C > 0x7fffffffll) return 0;
  return kRecHead + (C + 1 < kMaxHist ? C + 1 : kMaxHist) + 2 * C;
}

extern "C" int runia_conformal_reduce(const int32_t* size, const uint8_t* covered, const void* labels, int labels_i64,
                                      int has_ignore, int64_t ignore_index, int64_t N, int64_t C, void* out,
                                      runia_stream_t stream) {
  if (N < 0 || C <= 0 || C > 0x7fffffffll || !out) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(out, 0, (size_t)runia_conformal_record_slots(C) * sizeof(int64_t), s) != hipSuccess) return RUNIA_E_LAUNCH;
  if (N == 0) return RUNIA_OK;
  if (!size || !covered || !labels) return RUNIA_E_INVALID;
  const Labels L = {labels, labels_i64 != 0, has_ignore != 0, ignore_index};
  const int H = (int)(C + 1 < kMaxHist ? C + 1 : kMaxHist);
  conformal_reduce_kernel<<<runia_stream_grid(N, kRedRowsPerBlock), kRedThreads, 0, s>>>(size, covered, L, N, C, H,
                                                                                   static_cast<int64_t*>(out));
  return runia_check_launch();
}
