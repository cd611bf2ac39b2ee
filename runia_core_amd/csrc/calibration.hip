// Confidence calibration (evaluation/calibration.py; TempScale of inference/extended_postprocessors.py).
//   runia_calib_rows      : everything calibration needs from ONE read of the logits at a temperature 1 / beta: per row the first
//                           argmax, the top softmax probability, the negative log-likelihood and Brier score of the label, and the
//                           first and second derivative of the nll in beta (the Newton step of the temperature fit)
//   runia_calib_reduce_f32: the per-row table -> n_used, n_correct, the four f64 sums and the reliability table, in a fixed order
//                           (per-workgroup partials, then one ordered pass; integer counts, no floating-point atomics)
// The arithmetic of a row lives in calib_core.hpp (shared with pixel_calibration.hip).
// With m the row maximum, d_k = x_k - m and e_k = exp(beta d_k), a row is the four sums
//   S0 = sum e_k   S1 = sum e_k d_k   S2 = sum e_k d_k^2   Q = sum e_k^2          (p_k = e_k / S0)
// and the label's d_y:  conf = 1 / S0,  nll = log S0 - beta d_y,  brier = Q / S0^2 - 2 p_y + 1,  g = S1 / S0 - d_y,
// h = max(0, S2 / S0 - (S1 / S0)^2).  A class at -inf adds nothing; a NaN logit makes the row's outputs NaN.
#include "common.hpp"
#include "elem.hpp"
#include "calib_core.hpp"

namespace {

struct Labels {
  const void* p;   // int32 or int64 [N]; NULL: no labels (pred and conf only)
  int is_i64, has_ignore;
  int64_t ignore;
};

struct RowOut {
  int32_t* pred;
  float *conf, *nll, *brier, *g, *h;
};

__device__ __forceinline__ int64_t label_at(const Labels& L, int64_t row) {
  return L.is_i64 ? static_cast<const int64_t*>(L.p)[row] : (int64_t) static_cast<const int32_t*>(L.p)[row];
}

// the class whose logit the row needs (0 for a row without one) and whether the row is scored against a label
__device__ __forceinline__ int row_class(const Labels& L, int64_t row, int64_t C, bool& used) {
  used = false;
  if (!L.p) return 0;
  const int64_t y = label_at(L, row);
  used = y >= 0 && y < C && !(L.has_ignore && y == L.ignore);
  return used ? (int)y : 0;
}

__device__ __forceinline__ void finish_row(const RowOut& o, int64_t row, float beta, float m, Sums a, int bi, float xy,
                                           bool labelled, bool used) {
  if (o.pred) o.pred[row] = (bi == kNoIndex) ? 0 : bi;
  const RowVals v = finish_vals(beta, m, a, xy, used);
  if (o.conf) o.conf[row] = (!labelled || used) ? v.conf : __builtin_nanf("");
  if (o.nll) o.nll[row] = v.nll;
  if (o.brier) o.brier[row] = v.brier;
  if (o.g) o.g[row] = v.g;
  if (o.h) o.h[row] = v.h;
}

// four elements per lane and load: 16 bytes of f32, 8 bytes of f16 / bf16
template <class T>
__device__ __forceinline__ void ld4(const typename T::elem* p, float* v) {
  if constexpr (T::kBytes == 4) ld16<T>(p, v);
  else ld8<T>(p, v);
}

// C <= 16: one row per lane, the row in registers (stats_tiny_kernel)
template <class T, int CT>
__global__ __launch_bounds__(256) void calib_tiny_kernel(const typename T::elem* __restrict__ x, Labels L, float beta, RowOut o,
                                                          int64_t N) {
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < N; row += (int64_t)gridDim.x * 256) {
    const typename T::elem* p = x + row * CT;
    float v[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j) v[j] = ld1<T>(p + j);
    bool used;
    const int y = row_class(L, row, CT, used);
    float m = -INFINITY, xy = v[0];
    int bi = kNoIndex;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      best_take(m, bi, v[j], j);
      xy = (j == y) ? v[j] : xy;
    }
    Sums a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < CT; ++j) term(v[j], m, beta, a);
    finish_row(o, row, beta, m, a, bi, xy, L.p != nullptr, used);
  }
}

// 16 < C <= 64: one row per lane, the tile widened into LDS with coalesced loads, odd row pitch (stats_small_kernel)
constexpr int kSmallRows = 128;

template <class T>
__global__ __launch_bounds__(kSmallRows) void calib_small_kernel(const typename T::elem* __restrict__ x, Labels L, float beta,
                                                                  RowOut o, int64_t N, int C) {
  extern __shared__ float tile[];  // kSmallRows * (C | 1) floats
  const int tid = threadIdx.x, pitch = C | 1;
  for (int64_t r0 = (int64_t)blockIdx.x * kSmallRows; r0 < N; r0 += (int64_t)gridDim.x * kSmallRows) {
    const int rows = (int)((N - r0 < kSmallRows) ? (N - r0) : kSmallRows);
    const int total = rows * C;
    const typename T::elem* src = x + r0 * C;
    __syncthreads();
    for (int i = tid; i < total; i += kSmallRows) {
      const int r = i / C;
      tile[r * pitch + (i - r * C)] = ld1<T>(src + i);
    }
    __syncthreads();
    if (tid < rows) {
      const float* row = tile + tid * pitch;
      bool used;
      const int y = row_class(L, r0 + tid, C, used);
      float m = -INFINITY;
      int bi = kNoIndex;
      for (int k = 0; k < C; ++k) best_take(m, bi, row[k], k);
      Sums a = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < C; ++k) term(row[k], m, beta, a);
      finish_row(o, r0 + tid, beta, m, a, bi, row[y], L.p != nullptr, used);
    }
  }
}

// C > 64: one wave per row.
//   NCH > 0 : NCH four-element loads per lane, the row in registers: maximum first, then the sums (stats_wave_kernel)
//   NCH == 0: any C in one pass.  A lane takes U loads at a time (VEC: four elements each), moves its running maximum and
//             rescales its sums when it does; the lanes' sums are rescaled once more to the wave's maximum before they are added.
// The label's logit is one more load from a line the row's own loads bring in.
template <class T, int NCH, bool VEC>
__global__ __launch_bounds__(64 * kRowWaves) void calib_wave_kernel(const typename T::elem* __restrict__ x, Labels L, float beta,
                                                                    RowOut o, int64_t N, int64_t C) {
  static_assert(NCH == 0 || VEC, "the register form loads four elements at a time");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * kRowWaves;
  for (int64_t row = (int64_t)blockIdx.x * kRowWaves + wave; row < N; row += wave_stride) {
    const typename T::elem* p = x + row * C;
    bool used;
    const int y = row_class(L, row, C, used);
    const float xy = ld1<T>(p + y);
    float m = -INFINITY;
    int bi = kNoIndex;
    Sums a = {0.f, 0.f, 0.f, 0.f};
    if constexpr (NCH > 0) {
      const int n4 = (int)(C >> 2);
      float v[NCH][4];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int i = lane + 64 * c;
        if (i < n4) ld4<T>(p + 4 * i, v[c]);
        else v[c][0] = v[c][1] = v[c][2] = v[c][3] = -INFINITY;
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int i = lane + 64 * c;
        if (i < n4) {
#pragma unroll
          for (int j = 0; j < 4; ++j) best_take(m, bi, v[c][j], 4 * i + j);
        }
      }
      wave_best(m, bi);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (lane + 64 * c < n4) {
#pragma unroll
          for (int j = 0; j < 4; ++j) term(v[c][j], m, beta, a);
        }
      }
    } else {
      constexpr int U = VEC ? 4 : 8, E = VEC ? 4 : 1;
      const int64_t n = VEC ? (C >> 2) : C;  // loads per row
      for (int64_t i0 = 0; i0 < n; i0 += 64 * U) {
        float v[U][E];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t i = i0 + lane + 64 * u;
          if (i < n) {
            if constexpr (VEC) ld4<T>(p + 4 * i, v[u]);
            else v[u][0] = ld1<T>(p + i);
          } else {
#pragma unroll
            for (int j = 0; j < E; ++j) v[u][j] = -INFINITY;
          }
        }
        const float m_old = m;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t i = i0 + lane + 64 * u;
          if (i < n) {
#pragma unroll
            for (int j = 0; j < E; ++j) best_take(m, bi, v[u][j], (int)(E * i + j));
          }
        }
        if (m > m_old && m_old != -INFINITY) rescale(a, m - m_old, beta);  // (sums of a lane without a finite logit yet: 0 or NaN)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (i0 + lane + 64 * u < n) {
#pragma unroll
            for (int j = 0; j < E; ++j) term(v[u][j], m, beta, a);
          }
        }
      }
      const float m_lane = m;
      wave_best(m, bi);
      if (m > m_lane && m_lane != -INFINITY) rescale(a, m - m_lane, beta);
    }
    a.s0 = wave_sum_f32(a.s0);
    a.s1 = wave_sum_f32(a.s1);
    a.s2 = wave_sum_f32(a.s2);
    a.q = wave_sum_f32(a.q);
    if (lane == 0) finish_row(o, row, beta, m, a, bi, xy, L.p != nullptr, used);
  }
}

template <class T>
int launch_rows(const void* logits, const Labels& L, float beta, const RowOut& o, int64_t N, int64_t C, hipStream_t s) {
  const typename T::elem* x = static_cast<const typename T::elem*>(logits);
  if (C <= 16) {
    const unsigned grid = runia_stream_grid(N, 256);
#define RUNIA_CALIB_TINY(CT) \
  case CT: calib_tiny_kernel<T, CT><<<grid, 256, 0, s>>>(x, L, beta, o, N); break;
    switch ((int)C) {
      RUNIA_CALIB_TINY(1) RUNIA_CALIB_TINY(2) RUNIA_CALIB_TINY(3) RUNIA_CALIB_TINY(4) RUNIA_CALIB_TINY(5) RUNIA_CALIB_TINY(6)
      RUNIA_CALIB_TINY(7) RUNIA_CALIB_TINY(8) RUNIA_CALIB_TINY(9) RUNIA_CALIB_TINY(10) RUNIA_CALIB_TINY(11)
      RUNIA_CALIB_TINY(12) RUNIA_CALIB_TINY(13) RUNIA_CALIB_TINY(14) RUNIA_CALIB_TINY(15) RUNIA_CALIB_TINY(16)
    }
#undef RUNIA_CALIB_TINY
    return runia_check_launch();
  }
  if (C <= 64) {
    const size_t shmem = (size_t)kSmallRows * (C | 1) * sizeof(float);
    calib_small_kernel<T><<<runia_stream_grid(N, kSmallRows), kSmallRows, shmem, s>>>(x, L, beta, o, N, (int)C);
    return runia_check_launch();
  }
  const unsigned grid = runia_rows_grid(N);
  constexpr int kT = 64 * kRowWaves;
  // four elements per load: C % 4 == 0 keeps every row as aligned as the first
  const bool vec = ((C & 3) == 0) && ((((uintptr_t)logits) & (uintptr_t)(4 * T::kBytes - 1)) == 0);
  const int64_t n4 = C >> 2;
  if (vec && n4 <= 64) calib_wave_kernel<T, 1, true><<<grid, kT, 0, s>>>(x, L, beta, o, N, C);
  else if (vec && n4 <= 128) calib_wave_kernel<T, 2, true><<<grid, kT, 0, s>>>(x, L, beta, o, N, C);
  else if (vec && n4 <= 256) calib_wave_kernel<T, 4, true><<<grid, kT, 0, s>>>(x, L, beta, o, N, C);
  else if (vec && n4 <= 512) calib_wave_kernel<T, 8, true><<<grid, kT, 0, s>>>(x, L, beta, o, N, C);
  else if (vec) calib_wave_kernel<T, 0, true><<<grid, kT, 0, s>>>(x, L, beta, o, N, C);
  else calib_wave_kernel<T, 0, false><<<grid, kT, 0, s>>>(x, L, beta, o, N, C);
  return runia_check_launch();
}

// ---- row reduce ----------------------------------------------------------------------------------------------------------
// The record, in 8-byte slots: n_used, n_correct (int64) | sum nll, brier, g, h (f64) | count[n_bins], n_correct[n_bins] (int64) |
// conf_sum[n_bins] (f64).  A workgroup owns a contiguous range of rows; a wave walks it 64 rows at a time, lane = row.  Scalars:
// per-lane f64 sums, the exchange tree, the waves in order.  Bins: for every bin present among the 64 rows, the tree sum of its
// rows' conf goes to the wave's own table in LDS (lane 0, in program order).  The final pass adds the partials in block order.
constexpr int kRedThreads = 256, kRedWaves = kRedThreads / 64;
constexpr int kHead = 6, kMaxBins = 512;

static inline int64_t reduce_rows_per_block(int64_t N) {
  int64_t r = (N + 1023) / 1024;
  r = (r + kRedThreads - 1) / kRedThreads * kRedThreads;
  return r < 2048 ? 2048 : r;
}
static inline int64_t reduce_blocks(int64_t N) {
  const int64_t r = reduce_rows_per_block(N);
  return N > 0 ? (N + r - 1) / r : 1;
}

__global__ __launch_bounds__(kRedThreads) void calib_partial_kernel(const int32_t* __restrict__ pred,
                                                                     const float* __restrict__ conf,
                                                                     const float* __restrict__ nll,
                                                                     const float* __restrict__ brier,
                                                                     const float* __restrict__ g, const float* __restrict__ h,
                                                                     Labels L, int64_t N, int n_bins, int64_t rows_per_block,
                                                                     double* __restrict__ part) {
  extern __shared__ double bins[];  // [kRedWaves][3][n_bins]: conf_sum (f64), count, n_correct (int64 bits)
  __shared__ double sred[kRedWaves][4];
  __shared__ int64_t ired[kRedWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < kRedWaves * 3 * n_bins; i += kRedThreads) bins[i] = 0.0;  // (+0.0 is the int64 0 as well)
  __syncthreads();
  double* w_conf = bins + (size_t)wave * 3 * n_bins;
  int64_t* w_cnt = reinterpret_cast<int64_t*>(w_conf + n_bins);
  int64_t* w_cor = w_cnt + n_bins;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
  int64_t n_used = 0, n_correct = 0;
  double s_nll = 0.0, s_brier = 0.0, s_g = 0.0, s_h = 0.0;
  for (int64_t base = r0 + 64 * wave; base < r1; base += kRedThreads) {
    const int64_t row = base + lane;
    bool use = row < r1, hit = false;
    if (use) {
      const int64_t y = label_at(L, row);
      use = !(L.has_ignore && y == L.ignore);
      hit = use && pred && (int64_t)pred[row] == y;
    }
    if (use) {
      n_used += 1;
      n_correct += hit ? 1 : 0;
      if (nll) s_nll += (double)nll[row];
      if (brier) s_brier += (double)brier[row];
      if (g) s_g += (double)g[row];
      if (h) s_h += (double)h[row];
    }
    if (n_bins > 0) {
      const float c = use ? conf[row] : 0.f;
      const int b = use ? conf_bin(c, n_bins) : -1;
      uint64_t todo = __ballot(b >= 0);
      while (todo) {  // (wave-uniform: every bin present among these rows, lowest lane first)
        const int bb = __shfl(b, __ffsll((unsigned long long)todo) - 1, 64);
        const bool mine = b == bb;
        const uint64_t members = __ballot(mine);
        const uint64_t hits = __ballot(mine && hit);
        const double cs = wave_sum(mine ? (double)c : 0.0);
        if (lane == 0) {
          w_conf[bb] += cs;
          w_cnt[bb] += __popcll(members);
          w_cor[bb] += __popcll(hits);
        }
        todo &= ~members;
      }
    }
  }
  n_used = wave_sum(n_used);
  n_correct = wave_sum(n_correct);
  s_nll = wave_sum(s_nll);
  s_brier = wave_sum(s_brier);
  s_g = wave_sum(s_g);
  s_h = wave_sum(s_h);
  if (lane == 0) {
    ired[wave][0] = n_used;
    ired[wave][1] = n_correct;
    sred[wave][0] = s_nll;
    sred[wave][1] = s_brier;
    sred[wave][2] = s_g;
    sred[wave][3] = s_h;
  }
  __syncthreads();
  double* rec = part + (size_t)blockIdx.x * (kHead + 3 * n_bins);
  int64_t* irec = reinterpret_cast<int64_t*>(rec);
  if (tid < 2) {
    int64_t v = 0;
    for (int w = 0; w < kRedWaves; ++w) v += ired[w][tid];
    irec[tid] = v;
  } else if (tid < kHead) {
    double v = 0.0;
    for (int w = 0; w < kRedWaves; ++w) v += sred[w][tid - 2];
    rec[tid] = v;
  }
  for (int b = tid; b < n_bins; b += kRedThreads) {
    double cs = 0.0;
    int64_t cnt = 0, cor = 0;
    for (int w = 0; w < kRedWaves; ++w) {
      const double* t = bins + (size_t)w * 3 * n_bins;
      cs += t[b];
      cnt += reinterpret_cast<const int64_t*>(t + n_bins)[b];
      cor += reinterpret_cast<const int64_t*>(t + 2 * n_bins)[b];
    }
    irec[kHead + b] = cnt;
    irec[kHead + n_bins + b] = cor;
    rec[kHead + 2 * n_bins + b] = cs;
  }
}

// one thread per slot of the record, the workgroups' partials in order
__global__ __launch_bounds__(kRedThreads) void calib_final_kernel(const double* __restrict__ part, int64_t blocks, int n_bins,
                                                                   double* __restrict__ out) {
  const int slots = kHead + 3 * n_bins;
  for (int s = threadIdx.x; s < slots; s += kRedThreads) {
    const bool integer = s < 2 || (s >= kHead && s < kHead + 2 * n_bins);
    if (integer) {
      int64_t v = 0;
      for (int64_t b = 0; b < blocks; ++b) v += reinterpret_cast<const int64_t*>(part)[b * slots + s];
      reinterpret_cast<int64_t*>(out)[s] = v;
    } else {
      double v = 0.0;
      for (int64_t b = 0; b < blocks; ++b) v += part[b * slots + s];
      out[s] = v;
    }
  }
}

}  // namespace

extern "C" int runia_calib_rows(const void* logits, int dtype, const void* labels, int labels_i64, int has_ignore,
                                int64_t ignore_index, float beta, int32_t* pred, float* conf, float* nll, float* brier, float* g,
                                float* h, int64_t N, int64_t C, runia_stream_t stream) {
  if (!elem_dtype_ok(dtype) || N < 0 || C <= 0 || C > 0x7fffffffll || !(beta > 0.f) || beta == INFINITY) return RUNIA_E_INVALID;
  if (!labels && (nll || brier || g || h)) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!logits || (!pred && !conf && !nll && !brier && !g && !h)) return RUNIA_E_INVALID;
  const Labels L = {labels, labels_i64 != 0, has_ignore != 0, ignore_index};
  const RowOut o = {pred, conf, nll, brier, g, h};
  hipStream_t s = as_stream(stream);
  return dispatch_elem(dtype, [&](auto tag) { return launch_rows<decltype(tag)>(logits, L, beta, o, N, C, s); });
}

extern "C" size_t runia_calib_reduce_workspace_bytes(int64_t N, int n_bins) {
  if (N < 0 || n_bins < 0 || n_bins > kMaxBins) return 0;
  return (size_t)reduce_blocks(N) * (kHead + 3 * n_bins) * sizeof(double);
}

extern "C" int runia_calib_reduce_f32(const int32_t* pred, const float* conf, const float* nll, const float* brier,
                                      const float* g, const float* h, const void* labels, int labels_i64, int has_ignore,
                                      int64_t ignore_index, int64_t N, int n_bins, void* out, void* workspace,
                                      size_t workspace_bytes, runia_stream_t stream) {
  if (N < 0 || n_bins < 0 || n_bins > kMaxBins || !out) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  const size_t rec_bytes = (size_t)(kHead + 3 * n_bins) * sizeof(double);
  if (N == 0) return hipMemsetAsync(out, 0, rec_bytes, s) == hipSuccess ? RUNIA_OK : RUNIA_E_LAUNCH;
  if (!labels || (n_bins > 0 && !conf)) return RUNIA_E_INVALID;
  if (ws_refused(workspace, workspace_bytes, runia_calib_reduce_workspace_bytes(N, n_bins), 1)) return RUNIA_E_WORKSPACE;
  const Labels L = {labels, labels_i64 != 0, has_ignore != 0, ignore_index};
  const int64_t blocks = reduce_blocks(N);
  const size_t shmem = (size_t)kRedWaves * 3 * n_bins * sizeof(double);
  calib_partial_kernel<<<(unsigned)blocks, kRedThreads, shmem, s>>>(pred, conf, nll, brier, g, h, L, N, n_bins,
                                                                    reduce_rows_per_block(N), static_cast<double*>(workspace));
  if (runia_check_launch() != RUNIA_OK) return RUNIA_E_LAUNCH;
  calib_final_kernel<<<1, kRedThreads, 0, s>>>(static_cast<const double*>(workspace), blocks, n_bins,
                                               static_cast<double*>(out));
  return runia_check_launch();
}
