// LLM-Check (Sriramanan et al., NeurIPS 2024): the two white-box scores of ONE generation from one pass, DESIGN 4.59.
//   hidden score     (1/T) log det(C C^T + alpha I_T), C = the T x d hidden states of a layer centred over d per token
//   attention score  sum_h (1/T) sum_t log A_h[t, t]
// Sigma = C C^T + alpha I is symmetric positive definite by construction, so its singular values are its eigenvalues and
// the mean log-eigenvalue is (2/T) sum log L_ii of its Cholesky factor: no eigen-solver runs here.
//   1. llmc_mean_kernel    one wave per (matrix, token): the f64 mean over d, one fixed order
//   2. llmc_gram_kernel    one workgroup per (matrix, 64 x 64 tile pair of the lower triangle): d streams in 32-deep chunks,
//                          widened and centred while both row panels are staged in LDS, v_mfma_f64_16x16x4_f64
//   3. llmc_logdet_kernel  one workgroup per matrix: left-looking blocked Cholesky by 64-column panels - the panel's tiles
//                          take the product of the solved panels on the matrix cores (the Gram kernel's tile product, fed
//                          from the factor itself), the diagonal block is factored in LDS, the rows below are solved against it
//   4. llmc_attn_kernel    one wave per (row, layer, head): the diagonal read in place, f64 log, one fixed-order sum
// No atomics and no split across workgroups: every entry has one summation order, so a matrix's bits depend on its own
// row of the batch alone.
#include "common.hpp"
#include "elem.hpp"
#include "mfma_f64_tile.hpp"

namespace {

using runia_mfma::APITCH;
using runia_mfma::KC;

constexpr int TB = 64;                      // tile edge: 4 waves x 16-row strips, 4 column tiles of 16
constexpr int PANEL = TB * APITCH;          // doubles of one staged 64 x 32 row panel
constexpr int kStageDoubles = 4 * PANEL;    // two buffers x (A panel, B panel): 69 632 bytes
constexpr int kGramLds = kStageDoubles * (int)sizeof(double);
constexpr int kLogdetLds = (kStageDoubles + TB * TB) * (int)sizeof(double);  // + the 32 KB diagonal block: 102 400 bytes
constexpr int64_t kMaxT = 1024;

struct HidDesc { int64_t ptr, batch_stride, row_stride; };  // one (step, layer) tensor of hidden states (elements)
struct AttDesc { int64_t ptr, sb, sh, sr, sc, k, q; };      // rauq._batch_table's descriptor
struct RowWin { int64_t s, T; };                            // the token window of a batch row

// the states of position `pos` of batch row b at layer l: step 0 holds positions < P, step g >= 1 position P + g - 1
template <class T>
__device__ __forceinline__ const typename T::elem* token_row(const HidDesc* __restrict__ table, int64_t L, int64_t l,
                                                             int64_t P, int64_t b, int64_t pos) {
  const HidDesc hd = table[(pos < P ? 0 : pos - P + 1) * L + l];
  return reinterpret_cast<const typename T::elem*>(hd.ptr) + b * hd.batch_stride + (pos < P ? pos : 0) * hd.row_stride;
}

// eight consecutive elements from column j (a multiple of 8) of a row of d, zero past d: 16-byte loads where the row allows
template <class T>
__device__ __forceinline__ void load8(const typename T::elem* row, int64_t j, int64_t d, bool aligned, float* v) {
  if (aligned && j + 8 <= d) {
    ld16<T>(row + j, v);
    if constexpr (T::V == 4) ld16<T>(row + j + 4, v + 4);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = j + e < d ? ld1<T>(row + j + e) : 0.f;
  }
}

__device__ __forceinline__ void put8(double* dst, const double* c) {
#pragma unroll
  for (int e = 0; e < 8; e += 2) *reinterpret_cast<double2*>(dst + e) = make_double2(c[e], c[e + 1]);
}

// ---- 1. row means -----------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void llmc_mean_kernel(const HidDesc* __restrict__ table, const RowWin* __restrict__ rows,
                                                        int64_t L, int64_t P, int64_t d, int64_t M, int Tpad,
                                                        double* __restrict__ mean) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= M * Tpad) return;
  const int64_t m = w / Tpad, b = m / L, l = m % L;
  const int t = (int)(w % Tpad);
  const RowWin rw = rows[b];
  if (t >= rw.T) return;
  const typename T::elem* row = token_row<T>(table, L, l, P, b, rw.s + t);
  double s = 0.0;
  for (int64_t j = lane; j < d; j += 64) s += (double)ld1<T>(row + j);
  s = wave_sum(s);
  if (lane == 0) mean[m * Tpad + t] = s / (double)d;
}

// ---- the 64 x 64 tile product both matrix kernels share -----------------------------------------------------------------------
// acc[c] += Pa[16 wave + ., :] Pb[16 c + ., :]^T over `chunks` >= 1 chunks of 32 columns.  `src` fetches a chunk of both
// row panels into registers (fetch) and writes it, as f64, into a staged pair of panels (store): thread t owns 8 columns
// (t & 3) of row t >> 2.  The next chunk's loads are issued in front of a chunk's matrix instructions and first touched
// behind them; two buffers, one barrier per chunk.  A diagonal pair stages one panel and reads both operands from it.
// Rows are [row][k] with the pitch of mfma_f64_tile.hpp, so the A fragment (lane -> row li, k lg) and the B fragment
// (lane -> k lg, column li: B[k][j] = Pb[j][k]) are the same conflict-free read.
template <class Src>
__device__ __forceinline__ void tile_product(d4 (&acc)[4], Src& src, int chunks, bool diag, double* stage) {
  const int lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  src.fetch(0);
  src.store(stage, stage + PANEL);
  __syncthreads();
  int buf = 0;
  for (int ch = 0; ch < chunks; ++ch) {
    const bool more = ch + 1 < chunks;  // (uniform)
    if (more) src.fetch(ch + 1);
    const double* pa = stage + buf * 2 * PANEL;
    const double* pb = diag ? pa : pa + PANEL;
    double a[KC / 4];
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) a[s] = pa[(16 * wave + li) * APITCH + 4 * s + lg];
#pragma unroll
    for (int s = 0; s < KC / 4; ++s)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], pb[(16 * c + li) * APITCH + 4 * s + lg], acc[c], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);  // (the fetched values are first touched here)
    if (more) src.store(stage + (buf ^ 1) * 2 * PANEL, stage + (buf ^ 1) * 2 * PANEL + PANEL);
    __syncthreads();
    buf ^= 1;
  }
}

// ---- 2. centred Gram ----------------------------------------------------------------------------------------------------------
// The two row panels of a tile pair, read from the states where they lie: widened exactly, the token's mean subtracted in
// f64; rows past T_b and columns past d are staged as zero.
template <class T>
struct StateSrc {
  const typename T::elem *ra, *rb;
  double ma, mb;
  int64_t d, k0;
  int at;  // this thread's offset in a panel
  bool oka, okb, ala, alb, diag;
  float va[8], vb[8];

  __device__ __forceinline__ void fetch(int ch) {
    k0 = (int64_t)ch * KC + (threadIdx.x & 3) * 8;
    if (oka) load8<T>(ra, k0, d, ala, va);
    if (!diag && okb) load8<T>(rb, k0, d, alb, vb);
  }
  __device__ __forceinline__ void centre(double* dst, const float* v, bool ok, double m) const {
    double c[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = (ok && k0 + e < d) ? (double)v[e] - m : 0.0;
    put8(dst, c);
  }
  __device__ __forceinline__ void store(double* pa, double* pb) const {
    centre(pa + at, va, oka, ma);
    if (!diag) centre(pb + at, vb, okb, mb);
  }
};

// The same for the d x d form (below): a panel row is a FEATURE, the contraction runs over the window's tokens.  Thread t owns
// feature t >> 2 of each panel and 8 consecutive tokens; features past d and tokens past T_b are staged as zero.
template <class T>
struct FeatureSrc {
  const HidDesc* table;
  const double* mean;  // the matrix's token means
  int64_t L, l, P, b, s, Tw, d, ja, jb, k0;
  int at;
  bool diag;
  float va[8], vb[8];
  double mk[8];

  __device__ __forceinline__ void fetch(int ch) {
    k0 = (int64_t)ch * KC + (threadIdx.x & 3) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      va[e] = vb[e] = 0.f;
      mk[e] = 0.0;
      if (k0 + e < Tw) {
        const typename T::elem* row = token_row<T>(table, L, l, P, b, s + k0 + e);
        mk[e] = mean[k0 + e];
        if (ja < d) va[e] = ld1<T>(row + ja);
        if (!diag && jb < d) vb[e] = ld1<T>(row + jb);
      }
    }
  }
  __device__ __forceinline__ void centre(double* dst, const float* v, bool ok) const {
    double c[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = (ok && k0 + e < Tw) ? (double)v[e] - mk[e] : 0.0;
    put8(dst, c);
  }
  __device__ __forceinline__ void store(double* pa, double* pb) const {
    centre(pa + at, va, ja < d);
    if (!diag) centre(pb + at, vb, jb < d);
  }
};

// A window longer than the states are wide (d < T_b) has rank(C C^T) < d, so T_b - d + 1 eigenvalues of Sigma sit at alpha
// and each carries the rounding of Gram entries of size |c|^2 relative to alpha.  There the kernels work on the d x d form:
//   det(C C^T + alpha I_T) = alpha^(T - d) det(C^T C + alpha I_d),
// one eigenvalue at alpha instead of T - d + 1 (measured 5 - 50 x closer to a long-double reference), and the smaller matrix.
// n_b = min(T_b, d) is the order of row b's matrix; the choice depends on the row's own window alone.
template <class T>
__global__ __launch_bounds__(256) void llmc_gram_kernel(const HidDesc* __restrict__ table, const RowWin* __restrict__ rows,
                                                        int64_t L, int64_t P, int64_t d, int Tpad, int npairs, double alpha,
                                                        const double* __restrict__ mean, double* __restrict__ sigma) {
  extern __shared__ double llmc_lds[];
  const int64_t m = blockIdx.x / npairs, b = m / L, l = m % L;
  int ti = 0, tj = (int)(blockIdx.x % npairs);  // row ti of the lower triangle holds ti + 1 pairs
  while (tj > ti) { tj -= ti + 1; ++ti; }
  const RowWin rw = rows[b];
  const bool dual = d < rw.T;  // (uniform)
  const int64_t n = dual ? d : rw.T;
  if ((int64_t)ti * TB >= n) return;  // (uniform: a smaller matrix of the batch has fewer tiles)
  const int tid = threadIdx.x, srow = tid >> 2;
  const int64_t ta = (int64_t)ti * TB + srow, tb = (int64_t)tj * TB + srow;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (d4){0.0, 0.0, 0.0, 0.0};
  if (dual) {
    FeatureSrc<T> src;
    src.table = table;
    src.mean = mean + m * Tpad;
    src.L = L, src.l = l, src.P = P, src.b = b, src.s = rw.s, src.Tw = rw.T, src.d = d;
    src.ja = ta, src.jb = tb;
    src.at = srow * APITCH + (tid & 3) * 8;
    src.diag = ti == tj;
    tile_product(acc, src, (int)((rw.T + KC - 1) / KC), src.diag, llmc_lds);
  } else {
    StateSrc<T> src;
    src.d = d;
    src.diag = ti == tj;
    src.at = srow * APITCH + (tid & 3) * 8;
    src.oka = ta < rw.T;
    src.okb = tb < rw.T;
    src.ra = src.oka ? token_row<T>(table, L, l, P, b, rw.s + ta) : nullptr;
    src.rb = src.okb ? token_row<T>(table, L, l, P, b, rw.s + tb) : nullptr;
    src.ala = (reinterpret_cast<uintptr_t>(src.ra) & 15) == 0;
    src.alb = (reinterpret_cast<uintptr_t>(src.rb) & 15) == 0;
    src.ma = src.oka ? mean[m * Tpad + ta] : 0.0;
    src.mb = src.okb ? mean[m * Tpad + tb] : 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) src.va[e] = src.vb[e] = 0.f;
    tile_product(acc, src, (int)((d + KC - 1) / KC), src.diag, llmc_lds);
  }
  // alpha on the diagonal; a padded row gets a unit diagonal: its factor is the identity and adds log 1 = 0 to the sum
  const int lane = tid & 63, li = lane & 15, lg = lane >> 4, wave = tid >> 6;
  double* out = sigma + m * Tpad * Tpad;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = (int64_t)ti * TB + 16 * wave + lg + 4 * r, j = (int64_t)tj * TB + 16 * c + li;
      double v = acc[c][r];
      if (i == j) v = i < n ? v + alpha : 1.0;
      out[i * Tpad + j] = v;
    }
}

// ---- 3. blocked log-determinant -------------------------------------------------------------------------------------------------
// The row panels of a factor tile: rows of the matrix itself, columns 0 .. 64 k - 1 (the panels solved so far).
struct FactorSrc {
  const double *ra, *rb;
  int at;
  bool diag;
  double va[8], vb[8];

  __device__ __forceinline__ void fetch(int ch) {
    const int k0 = ch * KC + (threadIdx.x & 3) * 8;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const double2 t = *reinterpret_cast<const double2*>(ra + k0 + e);
      va[e] = t.x;
      va[e + 1] = t.y;
      if (!diag) {
        const double2 u = *reinterpret_cast<const double2*>(rb + k0 + e);
        vb[e] = u.x;
        vb[e + 1] = u.y;
      }
    }
  }
  __device__ __forceinline__ void store(double* pa, double* pb) const {
    put8(pa + at, va);
    if (!diag) put8(pb + at, vb);
  }
};

// Left-looking by 64-column panels, everything in one fixed order.  Panel k:
//   a. tile (i, k), i >= k, loses sum_{q < k} L[i, q] L[k, q]^T: the tile product over the 64 k columns solved so far;
//   b. the diagonal block goes to LDS and is factored there, column by column (two barriers a column, 64 columns);
//   c. every row below is solved against it by one thread, the row in registers, the block read from LDS as broadcasts.
// sum log L_ii is carried by every thread (the same values), out = (2 sum + (T - n) log alpha) / T.  A pivot that is not positive (NaN included)
// ends the matrix with NaN.  Rows past n of the last panel have a unit diagonal and zeros: they factor to the identity.
__global__ __launch_bounds__(256) void llmc_logdet_kernel(const RowWin* __restrict__ rows, int64_t L, int Tpad, int64_t d,
                                                          double alpha, double* sigma, double* out) {
  extern __shared__ double llmc_lds[];
  double* blk = llmc_lds + kStageDoubles;
  const int64_t m = blockIdx.x;
  const int64_t T = rows[m / L].T, n = d < T ? d : T;  // the order of this row's matrix (llmc_gram_kernel)
  const int nb = (int)((n + TB - 1) / TB);
  double* S = sigma + m * Tpad * Tpad;
  const int tid = threadIdx.x, srow = tid >> 2;
  const int lane = tid & 63, li = lane & 15, lg = lane >> 4, wave = tid >> 6;
  double logsum = 0.0;
  for (int k = 0; k < nb; ++k) {
    if (k > 0) {
      for (int i = k; i < nb; ++i) {
        FactorSrc src;
        src.ra = S + (int64_t)(TB * i + srow) * Tpad;
        src.rb = S + (int64_t)(TB * k + srow) * Tpad;
        src.at = srow * APITCH + (tid & 3) * 8;
        src.diag = i == k;
        d4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = (d4){0.0, 0.0, 0.0, 0.0};
        tile_product(acc, src, 2 * k, src.diag, llmc_lds);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* p = S + (int64_t)(TB * i + 16 * wave + lg + 4 * r) * Tpad + TB * k + 16 * c + li;
            *p -= acc[c][r];
          }
      }
      __syncthreads();  // the updated tiles are read by other threads below
    }
    for (int e = tid; e < TB * TB; e += 256) blk[e] = S[(int64_t)(TB * k + (e >> 6)) * Tpad + TB * k + (e & 63)];
    for (int j = 0; j < TB; ++j) {
      __syncthreads();
      const double p = blk[j * TB + j];
      if (!(p > 0.0)) {  // (uniform: every thread reads the same pivot)
        if (tid == 0) out[m] = __builtin_nan("");
        return;
      }
      const double ljj = sqrt(p);
      logsum += log(ljj);
      if (tid > j && tid < TB) blk[tid * TB + j] = blk[tid * TB + j] / ljj;
      __syncthreads();
      if (tid == 0) blk[j * TB + j] = ljj;
      for (int e = tid; e < (TB - 1 - j) * TB; e += 256) {
        const int i = j + 1 + (e >> 6), q = e & 63;
        if (q > j && q <= i) blk[i * TB + q] = fma(-blk[i * TB + j], blk[q * TB + j], blk[i * TB + q]);
      }
    }
    __syncthreads();
    const int r0 = TB * (k + 1), below = TB * nb - r0;
    // the block is read through an offset the compiler cannot see is zero: known uniform, every entry went through a scalar
    // register on its way to the multiply (hipcc of ROCm 7.2: 2 109 scalar spills in this kernel, none with the offset;
    // `-Rpass-analysis=kernel-resource-usage` prints the count - the result does not depend on it, only the time)
    int zero = 0;
    asm volatile("" : "+v"(zero));
    const double* lb = blk + zero;
    for (int r = tid; r < below; r += 256) {
      double* row = S + (int64_t)(r0 + r) * Tpad + TB * k;
      double x[TB];
#pragma unroll
      for (int e = 0; e < TB; e += 2) {
        const double2 t = *reinterpret_cast<const double2*>(row + e);
        x[e] = t.x;
        x[e + 1] = t.y;
      }
#pragma unroll
      for (int j = 0; j < TB; ++j) {
        x[j] = x[j] / lb[j * TB + j];
#pragma unroll
        for (int q = j + 1; q < TB; ++q) {
          x[q] = fma(-x[j], lb[q * TB + j], x[q]);
          if ((q & 15) == 15) __builtin_amdgcn_sched_barrier(0);  // (at most 16 block entries in flight: the row fills the file)
        }
      }
#pragma unroll
      for (int e = 0; e < TB; e += 2) *reinterpret_cast<double2*>(row + e) = make_double2(x[e], x[e + 1]);
    }
    __syncthreads();  // the solved panel is read by the next panel's products; blk is rewritten
  }
  if (tid == 0) out[m] = (2.0 * logsum + (n < T ? (double)(T - n) * log(alpha) : 0.0)) / (double)T;
}

// ---- 4. attention diagonals -----------------------------------------------------------------------------------------------------
// position pos < P: A[pos, pos] of the prompt block (step 0); pos >= P: the last column of the one query row of step
// pos - P + 1.  log 0 = -inf and NaN travel through the sum.
template <class T>
__global__ __launch_bounds__(256) void llmc_attn_kernel(const AttDesc* __restrict__ table, const RowWin* __restrict__ rows,
                                                        int64_t B, int64_t L, int64_t H, int64_t P,
                                                        double* __restrict__ per_head) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= B * L * H) return;
  const int64_t h = w % H, l = (w / H) % L, b = w / (H * L);
  const RowWin rw = rows[b];
  double s = 0.0;
  for (int64_t t = lane; t < rw.T; t += 64) {
    const int64_t pos = rw.s + t;
    const AttDesc ad = table[(pos < P ? 0 : pos - P + 1) * L + l];
    const int64_t r = pos < P ? pos : 0, c = pos < P ? pos : ad.k - 1;
    const typename T::elem* p = reinterpret_cast<const typename T::elem*>(ad.ptr) + b * ad.sb + h * ad.sh + r * ad.sr + c * ad.sc;
    s += log((double)ld1<T>(p));
  }
  s = wave_sum(s);
  if (lane == 0) per_head[w] = s / (double)rw.T;
}

// the heads of a (row, layer) summed in ascending order
__global__ __launch_bounds__(256) void llmc_head_sum_kernel(const double* __restrict__ per_head, int64_t n, int64_t H,
                                                            double* __restrict__ scores) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int64_t h = 0; h < H; ++h) s += per_head[i * H + h];
  scores[i] = s;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int64_t padded(int64_t T) { return (T + TB - 1) / TB * TB; }

struct Plan {
  double *mean, *sigma;  // [M, Tpad] token means | [M, Tpad, Tpad] the matrices, factored in place
};
Plan make_plan(WsWalk& w, int64_t M, int64_t T_max) {
  const int64_t tp = padded(T_max);
  Plan p;
  p.mean = w.take<double>((size_t)(M * tp), 16);
  p.sigma = w.take<double>((size_t)(M * tp * tp), 16);
  return p;
}

// the largest window of the host copy of `rows`, or -1 when a window is empty, negative or leaves [0, n_pos); *n_max (optional)
// receives the largest matrix order min(T_b, d)
int64_t max_window(const int64_t* host_rows, int64_t B, int64_t n_pos, int64_t d = 0, int64_t* n_max = nullptr) {
  int64_t t_max = 0, nm = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t s = host_rows[2 * b], T = host_rows[2 * b + 1];
    if (s < 0 || T < 1 || T > n_pos || s > n_pos - T) return -1;
    if (T > t_max) t_max = T;
    if ((d < T ? d : T) > nm) nm = d < T ? d : T;
  }
  if (n_max) *n_max = nm;
  return t_max;
}

}  // namespace

extern "C" int64_t runia_llmcheck_workspace_bytes(int64_t M, int64_t T_max) {
  if (M < 1 || T_max < 1 || T_max > kMaxT) return 0;
  return (int64_t)ws_bytes([&](WsWalk& w) { make_plan(w, M, T_max); });
}

// means and Gram matrices into the workspace (or, `sigma_out` set, the matrices there), then, `scores` set, the log-dets
static int llmcheck_run(const void* table, const void* rows, const int64_t* host_rows, int dtype, int64_t B, int64_t n_steps,
                        int64_t L, int64_t P, int64_t d, double alpha, double* sigma_out, double* scores, void* workspace,
                        size_t workspace_bytes, runia_stream_t stream) {
  if (!table || !rows || !host_rows || !(scores || sigma_out) || !elem_dtype_ok(dtype) || B < 1 || n_steps < 1 || L < 1 ||
      P < 1 || d < 1 || B * L > (1 << 20))
    return RUNIA_E_INVALID;
  int64_t n_max = 0;
  const int64_t t_max = max_window(host_rows, B, P + n_steps - 1, d, &n_max);
  if (t_max < 1 || t_max > kMaxT) return RUNIA_E_INVALID;
  const int64_t M = B * L;
  WsWalk w(workspace);
  Plan plan = make_plan(w, M, t_max);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  if (sigma_out) plan.sigma = sigma_out;
  const int tp = (int)padded(t_max), nt = (int)padded(n_max) / TB, npairs = nt * (nt + 1) / 2;
  hipStream_t s = as_stream(stream);
  const HidDesc* tab = static_cast<const HidDesc*>(table);
  const RowWin* rw = static_cast<const RowWin*>(rows);
  static std::atomic<uint64_t> gram_ok[3], logdet_ok{0};
  const int rc = dispatch_elem(dtype, [&](auto tag) {
    using T = decltype(tag);
    const void* gram = reinterpret_cast<const void*>(llmc_gram_kernel<T>);
    if (int e = runia_allow_dynamic_lds(gram, kGramLds, gram_ok[dtype])) return e;
    llmc_mean_kernel<T><<<(unsigned)((M * tp + 3) / 4), 256, 0, s>>>(tab, rw, L, P, d, M, tp, plan.mean);
    RUNIA_LAUNCH_TIMED(llmc_gram_kernel<T>, (unsigned)(M * npairs), 256, kGramLds, s, tab, rw, L, P, d, tp, npairs, alpha,
                       plan.mean, plan.sigma);
    return (int)RUNIA_OK;
  });
  if (rc) return rc;
  if (scores) {
    if (int e = runia_allow_dynamic_lds(reinterpret_cast<const void*>(llmc_logdet_kernel), kLogdetLds, logdet_ok)) return e;
    RUNIA_LAUNCH_TIMED(llmc_logdet_kernel, (unsigned)M, 256, kLogdetLds, s, rw, L, tp, d, alpha, plan.sigma, scores);
  }
  return runia_check_launch();
}

extern "C" int runia_llmcheck_hidden(const void* table, const void* rows, const int64_t* host_rows, int dtype, int64_t B,
                                     int64_t n_steps, int64_t L, int64_t P, int64_t d, double alpha, double* scores,
                                     void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (!scores) return RUNIA_E_INVALID;
  return llmcheck_run(table, rows, host_rows, dtype, B, n_steps, L, P, d, alpha, nullptr, scores, workspace, workspace_bytes,
                      stream);
}

extern "C" int runia_llmcheck_gram(const void* table, const void* rows, const int64_t* host_rows, int dtype, int64_t B,
                                   int64_t n_steps, int64_t L, int64_t P, int64_t d, double alpha, double* sigma,
                                   void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (!sigma) return RUNIA_E_INVALID;
  return llmcheck_run(table, rows, host_rows, dtype, B, n_steps, L, P, d, alpha, sigma, nullptr, workspace, workspace_bytes,
                      stream);
}

extern "C" int runia_llmcheck_attention(const void* table, const void* rows, const int64_t* host_rows, int dtype, int64_t B,
                                        int64_t n_steps, int64_t L, int64_t H, int64_t P, double* per_head, double* scores,
                                        runia_stream_t stream) {
  if (!table || !rows || !host_rows || !per_head || !scores || !elem_dtype_ok(dtype) || B < 1 || n_steps < 1 || L < 1 ||
      H < 1 || P < 1)
    return RUNIA_E_INVALID;
  if (max_window(host_rows, B, P + n_steps - 1) < 1) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  const int64_t n = B * L;
  dispatch_elem(dtype, [&](auto tag) {
    using T = decltype(tag);
    llmc_attn_kernel<T><<<(unsigned)((n * H + 3) / 4), 256, 0, s>>>(static_cast<const AttDesc*>(table),
                                                                    static_cast<const RowWin*>(rows), B, L, H, P, per_head);
    return 0;
  });
  llmc_head_sum_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(per_head, n, H, scores);
  return runia_check_launch();
}
