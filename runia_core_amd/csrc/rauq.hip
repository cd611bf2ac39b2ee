// RAUQ - recurrent attention-based uncertainty of one LLM generation (Vazhentsev et al. 2025), from the attention maps of
// HuggingFace `generate(output_attentions=True)` (reference llm_uncertainty/scores.py:155-344, attention_aggregation.py).
//
// The maps are read where they lie: a device table of n_gen x L descriptors (pointer, head / row / column strides in
// elements, k = last dimension, q = query rows) describes batch 0 of every step's tensor, so the caller's tensors are
// neither copied nor made contiguous.  Four kernels:
//   gather  (L, H, N) f32 token-aggregation values, one wave per (token, layer, head) row: attn[0, h, 0, -2] of steps
//           1 .. n_gen-1 ("original") or the row mean of step g's row 0 rounded to the map dtype ("mean_all_tokens")
//   score   one workgroup: head choice (argmax of the mean over tokens 1.. / mean over heads), exp of the log-probs, the
//           sequential confidence recurrence in f32 in the reference's operation order, -mean log, max over layers
//   rows    rollout row pass, one workgroup per (layer, row of the reconstructed T x T map): row sum of mean_h A + I, the
//           diagonal and sub-diagonal of A^ = rownorm(mean_h A + I), and a flag "a prompt-block entry above the diagonal
//           is non-zero"
//   chain   rollout for general maps: a k-row block R (1^T, or the last n rows of I) left-multiplied through the layers,
//           R <- (R diag(1/r_l)) M_l + R diag(1/r_l), column partials per row block written to a ping-pong buffer and
//           reduced in a fixed order by the next layer's workgroups (no atomics: repeated calls are bitwise equal)
// When no layer sets the flag every A^_l is lower-triangular and the sub-diagonal of the product needs only the
// diagonals and sub-diagonals of the factors (one_pass_kernel): "original" rollout then reads the maps once.
//
// Batched calls (runia_rauqb_*) score every row of a left-padded batch: a table of descriptors with the batch stride and a
// [B] table of {pad_b, n_b}.  Each kernel forms row b's own view of a map (row_view) and runs the one-row device code on
// it, so a row's bits are those of the one-row calls on its slices.  The chains run the one-row chain_kernel, row after row.
#include <algorithm>

#include "common.hpp"
#include "elem.hpp"

namespace {

struct MapDesc {  // one (step, layer) map, batch 0; strides and sizes in elements
  int64_t ptr, head_stride, row_stride, col_stride, k, q;
};

// one (step, layer) map of a batched call: batch 0 plus the batch stride; strides and sizes in elements
struct BMapDesc {
  int64_t ptr, batch_stride, head_stride, row_stride, col_stride, k, q;
};

struct RowInfo {  // one batch row: its prompt's left-pad count and the generated tokens scored
  int64_t pad, n;
};

// ET below: the element tag of the maps (elem.hpp); T is taken in this file, it is the side of the T x T rollout map.
// Row b's own map, as the one-row path sees the slice [b, :, pad:, pad:] of step 0 or [b, :, :, pad:] of a later step.
// A step 0 of one query row is not sliced by rows (the caller allows it only without padding).
template <class ET>
__device__ __forceinline__ MapDesc row_view(const BMapDesc& d, int64_t b, int64_t pad, bool step0) {
  const bool by_rows = step0 && d.q > 1;
  const int64_t off = b * d.batch_stride + pad * d.col_stride + (by_rows ? pad * d.row_stride : 0);
  return MapDesc{d.ptr + off * ET::kBytes, d.head_stride, d.row_stride, d.col_stride, d.k - pad, by_rows ? d.q - pad : d.q};
}

// map (step s, layer l) at index s * L + l: the one-row table as it is, or row b's views of a batched table
struct OneTab {
  const MapDesc* t;
  __device__ __forceinline__ MapDesc operator()(int64_t idx, bool) const { return t[idx]; }
};
template <class ET>
struct RowTab {
  const BMapDesc* t;
  int64_t b, pad;
  __device__ __forceinline__ MapDesc operator()(int64_t idx, bool step0) const { return row_view<ET>(t[idx], b, pad, step0); }
};

template <class ET>
__device__ __forceinline__ float ld(const MapDesc& m, int64_t off) {
  return ld1<ET>(reinterpret_cast<const typename ET::elem*>(m.ptr) + off);
}

// an f32 value rounded to the map dtype (round to nearest even, as torch's casts) and widened back
template <class ET>
__device__ __forceinline__ float round_to(float x) {
  return widen(ET{}, narrow(ET{}, x));
}
// bf16 hands a NaN back as it came, payload and all (narrow would write torch's quiet NaN)
template <>
__device__ __forceinline__ float round_to<BF16>(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return x;
  return __uint_as_float(bf16_round_bits(u) & 0xffff0000u);
}

// ---- gather ------------------------------------------------------------------------------------------------------------
// the token-aggregation value of query row 0 of map m (every lane returns it)
template <class ET>
__device__ __forceinline__ float gather_value(const MapDesc& m, int h, int lane, int mean_all) {
  const int64_t base = (int64_t)h * m.head_stride;  // query row 0
  if (!mean_all) return ld<ET>(m, base + (m.k - 2) * m.col_stride);
  if (m.k < 512) {
    // torch's own summation order (ATen cascade_sum): the head choice of the per-head mode compares row means that all
    // sit near 1/k for softmax rows, and is decided in their last bits
    return round_to<ET>(torch_row_sum([&](int j) { return ld<ET>(m, base + (int64_t)j * m.col_stride); }, (int)m.k) / (float)m.k);
  }
  float s = 0.f;
  for (int64_t j = lane; j < m.k; j += 64) s += ld<ET>(m, base + j * m.col_stride);
  s = wave_sum_f32(s);
  return round_to<ET>(s / (float)m.k);
}

template <class ET>
__global__ __launch_bounds__(256) void gather_kernel(const MapDesc* __restrict__ tab, int L, int H, int N, int mean_all,
                                                     float* __restrict__ w) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (int64_t)N * L * H) return;
  const int i = (int)(row / ((int64_t)L * H)), l = (int)((row / H) % L), h = (int)(row % H);
  const int g = mean_all ? i : i + 1;  // "original" reads steps 1 .. n_gen-1
  const float v = gather_value<ET>(tab[(int64_t)g * L + l], h, lane, mean_all);
  if (lane == 0) w[((int64_t)l * H + h) * N + i] = v;
}

// batched: one wave per (row b, token i < N_b, layer, head) into w[b][l][h][N] (N = the largest N_b)
template <class ET>
__global__ __launch_bounds__(256) void gather_batch_kernel(const BMapDesc* __restrict__ tab, const RowInfo* __restrict__ rows,
                                                           int B, int L, int H, int N, int mean_all, float* __restrict__ w) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int64_t per_b = (int64_t)N * L * H;
  if (row >= (int64_t)B * per_b) return;
  const int b = (int)(row / per_b);
  const int64_t r = row % per_b;
  const int i = (int)(r / ((int64_t)L * H)), l = (int)((r / H) % L), h = (int)(r % H);
  const RowInfo ri = rows[b];
  if (i >= (mean_all ? ri.n : ri.n - 1)) return;
  const int g = mean_all ? i : i + 1;
  const float v = gather_value<ET>(row_view<ET>(tab[(int64_t)g * L + l], b, ri.pad, g == 0), h, lane, mean_all);
  if (lane == 0) w[(((int64_t)b * L + l) * H + h) * N + i] = v;
}

// ---- score -------------------------------------------------------------------------------------------------------------
// head_mode 0: argmax head of each layer, 1: mean over heads, 2: one series att[N] (rollout; 1-D mean of the logs)
// att holds N values per (layer, head) at a row stride of ld; one workgroup
__device__ __forceinline__ void score_body(const float* __restrict__ att, int64_t ld, int L, int H, int N, int head_mode,
                                           const float* __restrict__ log_probs, const double* __restrict__ alphas,
                                           int n_alpha, float* __restrict__ scores, int* __restrict__ heads,
                                           float* __restrict__ series, float* __restrict__ unc) {
  const int t = threadIdx.x;
  if (head_mode == 0) {
    for (int l = t; l < L; l += blockDim.x) {
      int best = 0;
      float bv = 0.f;
      for (int h = 0; h < H; ++h) {
        const float* r = att + ((int64_t)l * H + h) * ld + 1;
        const float mu = torch_row_sum([&](int i) { return r[i]; }, N - 1) / (float)(N - 1);  // NaN for N == 1
        // torch.argmax: NaN is the maximum, the first index wins ties
        if (h == 0 || (!(bv != bv) && ((mu != mu) || mu > bv))) { best = h; bv = mu; }
      }
      if (heads) heads[l] = best;
      for (int i = 0; i < N; ++i) series[(int64_t)l * N + i] = att[((int64_t)l * H + best) * ld + i];
    }
  } else if (head_mode == 1) {
    for (int64_t e = t; e < (int64_t)L * N; e += blockDim.x) {
      const int l = (int)(e / N), i = (int)(e % N);
      float s = 0.f;
      for (int h = 0; h < H; ++h) s += att[((int64_t)l * H + h) * ld + i];
      series[e] = s / (float)H;
    }
  } else {
    for (int i = t; i < N; i += blockDim.x) series[i] = att[i];
  }
  __syncthreads();
  for (int e = t; e < L * n_alpha; e += blockDim.x) {
    const int l = e / n_alpha, a = e % n_alpha;
    const float* s = series + (int64_t)l * N;
    const float ca = (float)alphas[a], cb = (float)(1.0 - alphas[a]);
    float conf = expf(log_probs[0]);
    float acc = logf(conf);  // (N, L) mean over dim 0: one running f32 sum per layer
    double acc_d = (double)acc;
    for (int i = 1; i < N; ++i) {
      const float t1 = ca * expf(log_probs[i]);
      const float t2 = cb * s[i];
      const float t3 = t2 * conf;
      conf = t1 + t3;
      const float lg = logf(conf);
      acc += lg;
      acc_d += (double)lg;
    }
    unc[e] = head_mode == 2 ? -(float)(acc_d / (double)N) : -(acc / (float)N);
  }
  __syncthreads();
  for (int a = t; a < n_alpha; a += blockDim.x) {
    float m = unc[a];
    for (int l = 1; l < L; ++l) {
      const float u = unc[l * n_alpha + a];
      if (m != m || u != u) m = __builtin_nanf("");  // torch.max propagates NaN
      else m = fmaxf(m, u);
    }
    scores[a] = m;
  }
}

__global__ __launch_bounds__(256) void score_kernel(const float* __restrict__ att, int L, int H, int N, int head_mode,
                                                    const float* __restrict__ log_probs, const double* __restrict__ alphas,
                                                    int n_alpha, float* __restrict__ scores, int* __restrict__ heads,
                                                    float* __restrict__ series, float* __restrict__ unc) {
  score_body(att, N, L, H, N, head_mode, log_probs, alphas, n_alpha, scores, heads, series, unc);
}

// batched: one workgroup per row b, att at att + b * L * H * ld.  N_b = n_b - 1 ("original" gathers) or n_b; a row whose
// one-row call raises (N_b < 1, or n_b < 2 for the rollout) gets NaN
__global__ __launch_bounds__(256) void score_batch_kernel(const float* __restrict__ att, const RowInfo* __restrict__ rows,
                                                          int64_t ld, int L, int H, int head_mode, int mean_all,
                                                          const float* __restrict__ log_probs, int64_t lp_stride,
                                                          const double* __restrict__ alphas, int n_alpha,
                                                          float* __restrict__ scores, float* __restrict__ series,
                                                          float* __restrict__ unc) {
  const int b = blockIdx.x;
  const int64_t n = rows[b].n;
  const int N = (int)(head_mode == 2 || mean_all ? n : n - 1);
  float* out = scores + (int64_t)b * n_alpha;
  if (N < 1 || (head_mode == 2 && n < 2)) {
    for (int a = threadIdx.x; a < n_alpha; a += blockDim.x) out[a] = __builtin_nanf("");
    return;
  }
  score_body(att + (int64_t)b * L * H * ld, ld, L, H, N, head_mode, log_probs + (int64_t)b * lp_stride, alphas, n_alpha,
             out, nullptr, series + (int64_t)b * L * ld, unc + (int64_t)b * L * n_alpha);
}

// ---- rollout -----------------------------------------------------------------------------------------------------------
// Row i of the reconstructed (T x T) map of a layer (reference _reconstruct_attention_matrix): i < in - row i of step 0's
// block (row 0 when step 0 has one query row: torch broadcasts it), in columns; i == in - never written (zero); i > in -
// step i - in, in + (i - in) = i columns.
struct RowRef {
  MapDesc m;
  int64_t off;  // element offset of (head 0, the row, column 0)
  int64_t k;    // stored columns (0: zero row)
};

template <class Tab>
__device__ __forceinline__ RowRef row_ref(const Tab& tab, int L, int l, int in, int i) {
  RowRef r;
  if (i < in) {
    r.m = tab(l, true);
    r.off = (r.m.q == 1 ? 0 : (int64_t)i) * r.m.row_stride;
    r.k = in;
  } else if (i == in) {
    r.m = tab(l, true);
    r.off = 0;
    r.k = 0;
  } else {
    r.m = tab((int64_t)(i - in) * L + l, false);
    r.off = 0;
    r.k = i;
  }
  return r;
}

// sum over heads of column j (head order 0 .. H-1, as torch's mean over dim 0 of (H, T, T)); nz: a non-zero entry
template <class ET>
__device__ __forceinline__ float head_sum(const RowRef& r, int H, int64_t j, bool& nz) {
  const int64_t off = r.off + j * r.m.col_stride;
  float acc = 0.f;
  int h0 = 0;
  for (; h0 + 8 <= H; h0 += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld<ET>(r.m, off + (int64_t)(h0 + u) * r.m.head_stride);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc += v[u];
      nz |= v[u] != 0.f;
    }
  }
  for (; h0 < H; ++h0) {
    const float v = ld<ET>(r.m, off + (int64_t)h0 * r.m.head_stride);
    acc += v;
    nz |= v != 0.f;
  }
  return acc;
}

// row i of layer l: rsum / diag / sub at element e
template <class ET, class Tab>
__device__ __forceinline__ void rows_body(const Tab& tab, int L, int H, int in, int i, int l, int64_t e,
                                          float* __restrict__ rsum, float* __restrict__ diag, float* __restrict__ sub,
                                          int* __restrict__ upper_flag) {
  const int t = threadIdx.x;
  __shared__ float part[4];
  __shared__ float m_diag, m_sub;
  if (t == 0) { m_diag = 0.f; m_sub = 0.f; }
  __syncthreads();
  const RowRef r = row_ref(tab, L, l, in, i);
  float s = 0.f;
  bool upper = false;
  const float inv_h_div = (float)H;
  for (int64_t j = t; j < r.k; j += 256) {
    bool nz = false;
    const float m = head_sum<ET>(r, H, j, nz) / inv_h_div;
    s += m;
    if (j > i) upper |= nz;
    if (j == i) m_diag = m;
    if (j == i - 1) m_sub = m;
  }
  s = wave_sum_f32(s);
  if ((t & 63) == 0) part[t >> 6] = s;
  if (upper) atomicOr(upper_flag, 1);
  __syncthreads();
  if (t == 0) {
    const float rs = ((part[0] + part[1]) + (part[2] + part[3])) + 1.0f;  // + the identity's 1
    rsum[e] = rs;
    diag[e] = (m_diag + 1.0f) / rs;
    sub[e] = m_sub / rs;  // A^[i, i-1] (0 for i == 0)
  }
}

template <class ET>
__global__ __launch_bounds__(256) void rows_kernel(const MapDesc* __restrict__ tab, int L, int H, int in, int T,
                                                   float* __restrict__ rsum, float* __restrict__ diag,
                                                   float* __restrict__ sub, int* __restrict__ upper_flag) {
  const int i = blockIdx.x, l = blockIdx.y;
  rows_body<ET>(OneTab{tab}, L, H, in, i, l, (int64_t)l * T + i, rsum, diag, sub, upper_flag);
}

// batched: grid (T, L, B) with T = in + n_gen; row b's map has T_b = in - pad_b + n_b rows (in[b][l][T] layout), rows
// with n_b < 2 are skipped (their one-row call raises)
template <class ET>
__global__ __launch_bounds__(256) void rows_batch_kernel(const BMapDesc* __restrict__ tab, const RowInfo* __restrict__ rows,
                                                         int L, int H, int in, int T, float* __restrict__ rsum,
                                                         float* __restrict__ diag, float* __restrict__ sub,
                                                         int* __restrict__ upper_flags) {
  const int i = blockIdx.x, l = blockIdx.y, b = blockIdx.z;
  const RowInfo ri = rows[b];
  const int in_b = in - (int)ri.pad;
  if (ri.n < 2 || i >= in_b + ri.n) return;
  rows_body<ET>(RowTab<ET>{tab, b, ri.pad}, L, H, in_b, i, l, ((int64_t)b * L + l) * T + i, rsum, diag, sub,
                upper_flags + b);
}

// causal maps: joint[i+1, i] of A^_{L-1} ... A^_0 from the diagonals and sub-diagonals, for i = T-n-1 .. T-2
// (diag / sub of layer l at l * ld)
__device__ __forceinline__ float one_pass_value(const float* __restrict__ diag, const float* __restrict__ sub, int L,
                                                int64_t ld, int i) {
  double d = 1.0, s = 0.0;
  for (int l = 0; l < L; ++l) {
    const int64_t e = (int64_t)l * ld + i;
    s = (double)diag[e + 1] * s + (double)sub[e + 1] * d;
    d = (double)diag[e] * d;
  }
  return (float)s;
}

__global__ __launch_bounds__(256) void one_pass_kernel(const float* __restrict__ diag, const float* __restrict__ sub, int L,
                                                       int T, int n, float* __restrict__ att) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  att[c] = one_pass_value(diag, sub, L, T, T - n - 1 + c);
}

// batched: row b = blockIdx.y when n_b >= 2 and its upper flag is clear; att[b][c], c < n_b, at a row stride of ld_att
__global__ __launch_bounds__(256) void one_pass_batch_kernel(const float* __restrict__ diag, const float* __restrict__ sub,
                                                             const RowInfo* __restrict__ rows,
                                                             const int* __restrict__ upper_flags, int L, int in, int T,
                                                             int64_t ld_att, float* __restrict__ att) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  const RowInfo ri = rows[b];
  if (ri.n < 2 || upper_flags[b] != 0 || c >= ri.n) return;
  const int T_b = in - (int)ri.pad + (int)ri.n;
  const int64_t base = (int64_t)b * L * T;
  att[(int64_t)b * ld_att + c] = one_pass_value(diag + base, sub + base, L, T, T_b - (int)ri.n - 1 + c);
}

constexpr int kChainRows = 8;     // rows of the map per chain workgroup
constexpr int kChainCols = 256;   // columns per chain workgroup (one per thread)

// One layer of the chain, R row `r` = blockIdx.z, rows [b*8, b*8+8) = blockIdx.y, columns [c*256, c*256+256) = blockIdx.x.
// State in:  v_prev[k][T] (R diag(1/r) of the previous layer) and p_prev[k][nb][T] (its column partials); first layer: the
// initial R.  Out: v_cur (rows of this block, written by the column-0 workgroups), p_cur[r][b][columns].
template <class ET>
__global__ __launch_bounds__(256) void chain_kernel(const MapDesc* __restrict__ tab, int L, int H, int in, int T, int l,
                                                    int first, int init_ones, int n, int causal, int nb,
                                                    const float* __restrict__ rsum, const double* __restrict__ v_prev,
                                                    const double* __restrict__ p_prev, double* __restrict__ v_cur,
                                                    double* __restrict__ p_cur) {
  const int c0 = blockIdx.x * kChainCols, b = blockIdx.y, r = blockIdx.z, t = threadIdx.x;
  const int i0 = b * kChainRows;
  __shared__ double vp[kChainRows];
  if (t < kChainRows) {
    const int i = i0 + t;
    double v = 0.0;
    if (i < T) {
      if (first) {
        v = init_ones ? 1.0 : (i == T - n + r ? 1.0 : 0.0);
      } else {
        const double* pp = p_prev + (int64_t)r * nb * T + i;
        for (int bb = 0; bb < nb; ++bb) v += pp[(int64_t)bb * T];
        v += v_prev[(int64_t)r * T + i];
      }
      v /= (double)rsum[(int64_t)l * T + i];
      if (blockIdx.x == 0) v_cur[(int64_t)r * T + i] = v;
    }
    vp[t] = v;
  }
  __syncthreads();
  const int64_t j = c0 + t;
  if (j >= T) return;
  double acc = 0.0;
  for (int u = 0; u < kChainRows; ++u) {
    const int i = i0 + u;
    if (i >= T) break;
    const RowRef rr = row_ref(OneTab{tab}, L, l, in, i);
    const int64_t kk = (causal && i < in) ? (int64_t)i + 1 : rr.k;  // causal maps: nothing above the diagonal
    if (j >= kk || vp[u] == 0.0) continue;
    bool nz = false;
    const float m = head_sum<ET>(rr, H, j, nz) / (float)H;
    acc += vp[u] * (double)m;
  }
  p_cur[((int64_t)r * nb + b) * T + j] = acc;
}

// batched: before row b's chain, its own one-row map table (n_b * L views) and its rsum repacked as [L][T_b], so the
// chain itself is chain_kernel on the row's own maps
template <class ET>
__global__ __launch_bounds__(256) void chain_row_kernel(const BMapDesc* __restrict__ tab, int b, int pad, int L, int n,
                                                        int T, int T_b, const float* __restrict__ rsum_b,
                                                        MapDesc* __restrict__ row_tab, float* __restrict__ row_rsum) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (int64_t)n * L) row_tab[e] = row_view<ET>(tab[e], b, pad, e < L);
  if (e < (int64_t)L * T_b) row_rsum[e] = rsum_b[(e / T_b) * T + e % T_b];
}

// att[c]: "mean_all_tokens" - column T-n+c of 1^T joint over T; "original" - entry (r = c, column T-n-1+c) of the n-row R
__global__ __launch_bounds__(256) void chain_final_kernel(int T, int n, int mean_all, int nb, const double* __restrict__ v,
                                                          const double* __restrict__ p, float* __restrict__ att) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int r = mean_all ? 0 : c;
  const int64_t j = mean_all ? T - n + c : T - n - 1 + c;
  double s = 0.0;
  for (int bb = 0; bb < nb; ++bb) s += p[((int64_t)r * nb + bb) * T + j];
  s += v[(int64_t)r * T + j];
  att[c] = mean_all ? (float)(s / (double)T) : (float)s;
}

// ---- workspace layout --------------------------------------------------------------------------------------------------
struct Plan {
  float *rsum, *diag, *sub, *series, *unc, *row_rsum;
  double *v[2], *p[2];
  MapDesc* row_tab;
  int64_t nb;
};

// 256-byte slots on a 16-byte aligned base.  One generation: B = 1 and a series of max(n_gen, n) floats per layer.
// Batched calls: the row-pass regions hold [B][L][T] (T = input_length + n_gen), series [B][L][n_gen], unc [B][L][n_alpha];
// the chain regions (and the chained row's own map table and rsum) are sized for the largest row and reused row after row
static Plan plan(WsWalk& w, int64_t B, int64_t L, int64_t n_gen, int64_t series_n, int64_t in, int64_t chain_rows, int n_alpha,
                 bool batched) {
  Plan o{};
  const int64_t T = in > 0 ? in + n_gen : 0;
  o.nb = T > 0 ? (T + kChainRows - 1) / kChainRows : 0;
  // the rollout regions first: their offsets depend on (B, L, T) only
  o.rsum = w.take<float>(B * L * T, 256);
  o.diag = w.take<float>(B * L * T, 256);
  o.sub = w.take<float>(B * L * T, 256);
  o.series = w.take<float>(B * L * series_n, 256);
  o.unc = w.take<float>(B * L * n_alpha, 256);
  const int64_t k = T > 0 ? chain_rows : 0;
  o.v[0] = w.take<double>(k * T, 256);
  o.v[1] = w.take<double>(k * T, 256);
  o.p[0] = w.take<double>(k * o.nb * T, 256);
  o.p[1] = w.take<double>(k * o.nb * T, 256);
  o.row_tab = w.take<MapDesc>(batched && k > 0 ? n_gen * L : 0, 256);
  o.row_rsum = w.take<float>(batched && k > 0 ? L * T : 0, 256);
  return o;
}
static Plan plan_one(WsWalk& w, int64_t L, int64_t n_gen, int64_t in, int64_t n, int64_t chain_rows, int n_alpha) {
  return plan(w, 1, L, n_gen, n_gen > n ? n_gen : n, in, chain_rows, n_alpha, false);
}
static Plan plan_batch(WsWalk& w, int64_t B, int64_t L, int64_t n_gen, int64_t in, int64_t chain_rows, int n_alpha) {
  return plan(w, B, L, n_gen, n_gen, in, chain_rows, n_alpha, true);
}

constexpr int64_t kMaxDim = 1 << 20;
static bool dims_ok(int64_t n_gen, int64_t L, int64_t H) {
  return n_gen >= 1 && n_gen <= kMaxDim && L >= 1 && L <= 4096 && H >= 1 && H <= 4096;
}

}  // namespace

extern "C" size_t runia_rauq_workspace_bytes(int64_t L, int64_t n_gen, int64_t input_length, int64_t n, int64_t chain_rows,
                                             int n_alpha) {
  if (L < 1 || n_gen < 1 || input_length < 0 || n < 0 || chain_rows < 0 || n_alpha < 0) return 0;
  return ws_bytes([&](WsWalk& w) { plan_one(w, L, n_gen, input_length, n, chain_rows, n_alpha); });
}

extern "C" int runia_rauq_gather(const void* table, int dtype, int64_t n_gen, int64_t L, int64_t H, int token_agg, float* w,
                                 runia_stream_t stream) {
  if (!table || !w || !elem_dtype_ok(dtype) || (token_agg != 0 && token_agg != 1) || !dims_ok(n_gen, L, H))
    return RUNIA_E_INVALID;
  const int64_t N = token_agg ? n_gen : n_gen - 1;
  if (N < 1) return RUNIA_E_INVALID;
  const int64_t rows = N * L * H;
  const unsigned grid = (unsigned)((rows + 3) / 4);
  const MapDesc* tab = reinterpret_cast<const MapDesc*>(table);
  return dispatch_elem(dtype, [&](auto et) {
    gather_kernel<decltype(et)><<<grid, 256, 0, as_stream(stream)>>>(tab, (int)L, (int)H, (int)N, token_agg, w);
    return runia_check_launch();
  });
}

extern "C" int runia_rauq_score(const float* att, int64_t L, int64_t H, int64_t N, int head_mode, const float* log_probs,
                                const double* alphas, int n_alpha, float* scores, int* heads, void* workspace,
                                size_t workspace_bytes, runia_stream_t stream) {
  if (!att || !log_probs || !alphas || !scores || n_alpha < 1 || N < 1 || N > kMaxDim || head_mode < 0 || head_mode > 2 ||
      L < 1 || L > 4096 || H < 1 || H > 4096 || (head_mode == 2 && (L != 1 || H != 1)))
    return RUNIA_E_INVALID;
  // the layout's series region holds L * max(n_gen, n) floats: N of them per layer
  WsWalk w(workspace);
  const Plan o = plan_one(w, L, N, 0, 0, 0, n_alpha);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  score_kernel<<<1, 256, 0, as_stream(stream)>>>(att, (int)L, (int)H, (int)N, head_mode, log_probs, alphas, n_alpha, scores,
                                                 head_mode == 0 ? heads : nullptr, o.series,
                                                 o.unc);
  return runia_check_launch();
}

extern "C" int runia_rauq_rollout_rows(const void* table, int dtype, int64_t n_gen, int64_t L, int64_t H,
                                       int64_t input_length, int* upper_flag, void* workspace, size_t workspace_bytes,
                                       runia_stream_t stream) {
  if (!table || !upper_flag || !elem_dtype_ok(dtype) || !dims_ok(n_gen, L, H) || n_gen < 2 || input_length < 1 ||
      input_length + n_gen > kMaxDim)
    return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const Plan o = plan_one(w, L, n_gen, input_length, 0, 0, 1);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  const int T = (int)(input_length + n_gen);
  if (hipMemsetAsync(upper_flag, 0, sizeof(int), as_stream(stream)) != hipSuccess) return RUNIA_E_LAUNCH;
  const MapDesc* tab = reinterpret_cast<const MapDesc*>(table);
  return dispatch_elem(dtype, [&](auto et) {
    rows_kernel<decltype(et)><<<dim3((unsigned)T, (unsigned)L), 256, 0, as_stream(stream)>>>(
        tab, (int)L, (int)H, (int)input_length, T, o.rsum,
        o.diag, o.sub, upper_flag);
    return runia_check_launch();
  });
}

extern "C" int runia_rauq_rollout_att(const void* table, int dtype, int64_t n_gen, int64_t L, int64_t H,
                                      int64_t input_length, int token_agg, int route, int64_t n, float* att, void* workspace,
                                      size_t workspace_bytes, runia_stream_t stream) {
  if (!table || !att || !elem_dtype_ok(dtype) || !dims_ok(n_gen, L, H) || n_gen < 2 || input_length < 1 ||
      input_length + n_gen > kMaxDim || (token_agg != 0 && token_agg != 1) || route < 0 || route > 2 ||
      (route == 0 && token_agg != 0) || n < 1)
    return RUNIA_E_INVALID;
  const int64_t T = input_length + n_gen;
  if ((token_agg == 0 && n > T - 1) || (token_agg == 1 && n > T)) return RUNIA_E_INVALID;
  const int64_t k = route == 0 ? 0 : (token_agg ? 1 : n);
  WsWalk w(workspace);
  const Plan o = plan_one(w, L, n_gen, input_length, n, k, 1);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  if (k > 65535) return RUNIA_E_INVALID;
  const float* rsum = o.rsum;
  const unsigned out_grid = (unsigned)((n + 255) / 256);
  hipStream_t s = as_stream(stream);
  if (route == 0) {
    one_pass_kernel<<<out_grid, 256, 0, s>>>(o.diag,
                                             o.sub, (int)L, (int)T, (int)n, att);
    return runia_check_launch();
  }
  const MapDesc* tab = reinterpret_cast<const MapDesc*>(table);
  double* const *v = o.v, *const *p = o.p;
  const dim3 grid((unsigned)((T + kChainCols - 1) / kChainCols), (unsigned)o.nb, (unsigned)k);
  int cur = 0;
  int rc = RUNIA_OK;
  for (int64_t l = L - 1; l >= 0 && rc == RUNIA_OK; --l) {
    const int first = l == L - 1;
    rc = dispatch_elem(dtype, [&](auto et) {
      chain_kernel<decltype(et)><<<grid, 256, 0, s>>>(tab, (int)L, (int)H, (int)input_length, (int)T, (int)l, first,
                                                    token_agg, (int)n, route == 1, (int)o.nb, rsum, v[cur ^ 1],
                                                    p[cur ^ 1], v[cur], p[cur]);
      return runia_check_launch();
    });
    cur ^= 1;
  }
  if (rc != RUNIA_OK) return rc;
  chain_final_kernel<<<out_grid, 256, 0, s>>>((int)T, (int)n, token_agg, (int)o.nb, v[cur ^ 1], p[cur ^ 1], att);
  return runia_check_launch();
}

// ---- batched entry points ------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t kMaxBatch = 65535;  // grid y / z
}

extern "C" size_t runia_rauqb_workspace_bytes(int64_t B, int64_t L, int64_t n_gen, int64_t input_length, int64_t chain_rows,
                                              int n_alpha) {
  if (B < 1 || B > kMaxBatch || L < 1 || n_gen < 1 || input_length < 0 || chain_rows < 0 || n_alpha < 0) return 0;
  return ws_bytes([&](WsWalk& w) { plan_batch(w, B, L, n_gen, input_length, chain_rows, n_alpha); });
}

extern "C" int runia_rauqb_gather(const void* table, const void* rows, int dtype, int64_t B, int64_t n_gen, int64_t L,
                                  int64_t H, int token_agg, float* w, runia_stream_t stream) {
  if (!table || !rows || !w || !elem_dtype_ok(dtype) || (token_agg != 0 && token_agg != 1) || B < 1 ||
      B > kMaxBatch || !dims_ok(n_gen, L, H))
    return RUNIA_E_INVALID;
  const int64_t N = token_agg ? n_gen : n_gen - 1;
  if (N < 1) return RUNIA_E_INVALID;
  const int64_t waves = B * N * L * H;
  if ((waves + 3) / 4 > 0x7fffffff) return RUNIA_E_INVALID;
  const unsigned grid = (unsigned)((waves + 3) / 4);
  const BMapDesc* tab = reinterpret_cast<const BMapDesc*>(table);
  const RowInfo* ri = reinterpret_cast<const RowInfo*>(rows);
  return dispatch_elem(dtype, [&](auto et) {
    gather_batch_kernel<decltype(et)><<<grid, 256, 0, as_stream(stream)>>>(tab, ri, (int)B, (int)L, (int)H, (int)N,
                                                                           token_agg, w);
    return runia_check_launch();
  });
}

extern "C" int runia_rauqb_score(const float* att, const void* rows, int64_t B, int64_t L, int64_t H, int64_t N,
                                 int head_mode, int token_agg, const float* log_probs, int64_t lp_stride,
                                 const double* alphas, int n_alpha, float* scores, void* workspace, size_t workspace_bytes,
                                 runia_stream_t stream) {
  if (!att || !rows || !log_probs || !alphas || !scores || n_alpha < 1 || B < 1 || B > kMaxBatch || N < 1 || N > kMaxDim ||
      head_mode < 0 || head_mode > 2 || (token_agg != 0 && token_agg != 1) || L < 1 || L > 4096 || H < 1 || H > 4096 ||
      (head_mode == 2 && (L != 1 || H != 1)) || lp_stride < 1)
    return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const Plan o = plan_batch(w, B, L, N, 0, 0, n_alpha);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  score_batch_kernel<<<(unsigned)B, 256, 0, as_stream(stream)>>>(
      att, reinterpret_cast<const RowInfo*>(rows), N, (int)L, (int)H, head_mode, token_agg, log_probs, lp_stride, alphas,
      n_alpha, scores, o.series, o.unc);
  return runia_check_launch();
}

extern "C" int runia_rauqb_rollout_rows(const void* table, const void* rows, int dtype, int64_t B, int64_t n_gen, int64_t L,
                                        int64_t H, int64_t input_length, int* upper_flags, void* workspace,
                                        size_t workspace_bytes, runia_stream_t stream) {
  if (!table || !rows || !upper_flags || !elem_dtype_ok(dtype) || B < 1 || B > kMaxBatch || !dims_ok(n_gen, L, H) ||
      n_gen < 2 || input_length < 1 || input_length + n_gen > kMaxDim)
    return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const Plan o = plan_batch(w, B, L, n_gen, input_length, 0, 1);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  const int T = (int)(input_length + n_gen);
  if (hipMemsetAsync(upper_flags, 0, sizeof(int) * (size_t)B, as_stream(stream)) != hipSuccess) return RUNIA_E_LAUNCH;
  const BMapDesc* tab = reinterpret_cast<const BMapDesc*>(table);
  return dispatch_elem(dtype, [&](auto et) {
    rows_batch_kernel<decltype(et)><<<dim3((unsigned)T, (unsigned)L, (unsigned)B), 256, 0, as_stream(stream)>>>(
        tab, reinterpret_cast<const RowInfo*>(rows), (int)L, (int)H, (int)input_length, T,
        o.rsum, o.diag, o.sub,
        upper_flags);
    return runia_check_launch();
  });
}

extern "C" int runia_rauqb_rollout_att(const void* table, const void* rows, const int64_t* host_rows, const int* upper_flags,
                                       const int* host_upper, int dtype, int64_t B, int64_t n_gen, int64_t L, int64_t H,
                                       int64_t input_length, int token_agg, float* att, void* workspace,
                                       size_t workspace_bytes, runia_stream_t stream) {
  if (!table || !rows || !host_rows || !upper_flags || !host_upper || !att || !elem_dtype_ok(dtype) || B < 1 ||
      B > kMaxBatch || !dims_ok(n_gen, L, H) || n_gen < 2 || input_length < 1 || input_length + n_gen > kMaxDim ||
      (token_agg != 0 && token_agg != 1))
    return RUNIA_E_INVALID;
  // every row's route, and the chain rows the largest chain carries
  int64_t k = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t pad = host_rows[2 * b], n = host_rows[2 * b + 1];
    if (pad < 0 || pad >= input_length || n < 1 || n > n_gen) return RUNIA_E_INVALID;
    if (n >= 2 && (token_agg || host_upper[b])) k = std::max(k, token_agg ? (int64_t)1 : n);
  }
  if (k > 65535) return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const Plan o = plan_batch(w, B, L, n_gen, input_length, k, 1);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  const int64_t T = input_length + n_gen;
  const float* rsum = o.rsum;
  if (!token_agg) {  // route 0 for every row with a clear flag, in one launch
    one_pass_batch_kernel<<<dim3((unsigned)((n_gen + 255) / 256), (unsigned)B), 256, 0, s>>>(
        o.diag, o.sub,
        reinterpret_cast<const RowInfo*>(rows), upper_flags, (int)L, (int)input_length, (int)T, n_gen, att);
    const int rc = runia_check_launch();
    if (rc != RUNIA_OK) return rc;
  }
  const BMapDesc* tab = reinterpret_cast<const BMapDesc*>(table);
  double* const *v = o.v, *const *p = o.p;
  for (int64_t b = 0; b < B; ++b) {  // the chains, row after row, in the one workspace
    const int64_t pad = host_rows[2 * b], n = host_rows[2 * b + 1];
    if (n < 2 || !(token_agg || host_upper[b])) continue;
    const int route = host_upper[b] ? 2 : 1;
    const int64_t in_b = input_length - pad, T_b = in_b + n, nb = (T_b + kChainRows - 1) / kChainRows;
    const dim3 grid((unsigned)((T_b + kChainCols - 1) / kChainCols), (unsigned)nb, (unsigned)(token_agg ? 1 : n));
    MapDesc* row_tab = o.row_tab;
    float* row_rsum = o.row_rsum;
    const int64_t prep = std::max(n * L, L * T_b);
    int rc = dispatch_elem(dtype, [&](auto et) {
      chain_row_kernel<decltype(et)><<<(unsigned)((prep + 255) / 256), 256, 0, s>>>(
          tab, (int)b, (int)pad, (int)L, (int)n, (int)T, (int)T_b, rsum + b * L * T, row_tab, row_rsum);
      return runia_check_launch();
    });
    int cur = 0;
    for (int64_t l = L - 1; l >= 0 && rc == RUNIA_OK; --l) {
      const int first = l == L - 1;
      rc = dispatch_elem(dtype, [&](auto et) {
        chain_kernel<decltype(et)><<<grid, 256, 0, s>>>(row_tab, (int)L, (int)H, (int)in_b, (int)T_b, (int)l, first,
                                                      token_agg, (int)n, route == 1, (int)nb, row_rsum, v[cur ^ 1],
                                                      p[cur ^ 1], v[cur], p[cur]);
        return runia_check_launch();
      });
      cur ^= 1;
    }
    if (rc != RUNIA_OK) return rc;
    chain_final_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((int)T_b, (int)n, token_agg, (int)nb, v[cur ^ 1],
                                                                     p[cur ^ 1], att + b * n_gen);
    rc = runia_check_launch();
    if (rc != RUNIA_OK) return rc;
  }
  return RUNIA_OK;
}
