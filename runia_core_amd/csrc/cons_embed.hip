// Embedding-level sample consistency: the greedy token matching of BERTScore between the samples of a prompt, on a layer's
// hidden states read where generate() left them, DESIGN 4.61.  For samples i, j of group g with (centred) unit tokens x^, y^
//   cov[g, i, j] = (1 / n_i) sum_{a in i} max_{b in j} <x^_a, y^_b>
// Nothing of size T x T or N x d is written: the cosines live in accumulator registers and leave them as maxima.
//   0. cemb_init_kernel    zeroes the means, the NaN flags and the column-maximum keys (no memset: graphs replay kernels)
//   1. cemb_mean_kernel    one workgroup per (group, 512 features): the f64 sum over the group's content tokens, wave w takes the
//                          tokens = w mod 4 of the group's flat order, the four partial sums meet in LDS in wave order -> f32 means
//   2. cemb_norm_kernel    one wave per token: c = x - m in f32 (the subtraction the main kernel repeats), sum c^2 in f64, one
//                          butterfly -> 1 / |c| in f32 (0 for a zero token); a sum that is not finite raises the group's flag
//   3. cemb_main_kernel    one workgroup per (group, sample pair i <= j, block of 128 tokens of i); it sweeps the tokens of j in
//                          tiles of 128.  d streams in stages of 64 bytes per row: a chunk is fetched through the descriptors one
//                          stage ahead, widened, centred by the mean chunk, scaled by the inverse norm and written to one of two
//                          LDS buffers in the matrix-core input type.  A 16-bit type takes the f32 value v as TWO elements, hi =
//                          round(v) and lo = round(v - hi) (v - hi is exact in f32), and a product as hi hi' + hi lo' + lo hi':
//                          one rounding alone moves a cosine by up to 2 x 2^-11 (f16) / 2 x 2^-8 (bf16), measured 1.35 of the
//                          stated bound at d = 5; with the pair what is dropped is of the order 2^-22 / 2^-16.  Row
//                          pitch 144 bytes (hi, lo, 16 of padding; 80 bytes for f32, as logit_lens.hip).  4 waves of 64 x 64 (2 x 2
//                          tiles of mfma 32x32x16 bf16 / f16, 32x32x2 f32).  Lane l of a wave owns column (token of j) l & 31 of a
//                          tile, its 16 registers are rows (r & 3) + 8 (r >> 2) + 4 (l >> 5).
//      epilogue            rows past n_i and columns past n_j are masked to -inf and nothing else.  Column maxima: a serial maximum
//                          per lane, then integer atomicMax on ordered keys in LDS (lane halves, row waves) and from there in the
//                          workspace (the row blocks of i).  Row maxima: a 32-lane butterfly per register, folded into an LDS
//                          array of keys over the column sweep; complete inside the workgroup, stored as f32.
//   4. cemb_finish_kernel  one wave per entry (g, i, j): the f64 mean of the row maxima of pair (i, j), i <= j, or of the column
//                          maxima of pair (j, i) - an unordered pair is multiplied once.  Lane l adds tokens l, l + 64, ..., one
//                          butterfly.  Both samples empty: 1; one empty: 0; a flagged group: NaN.
// A maximum does not depend on the order of its operands, every sum has one order and every quantity is a function of its own
// group: the same call gives the same bits, and a group's bits do not depend on the rest of the batch.
#include "common.hpp"
#include "elem.hpp"

#include <type_traits>

namespace {

constexpr int kMaxK = RUNIA_CONS_MAX_K;
constexpr int64_t kMaxT = RUNIA_CONS_EMBED_MAX_T;
constexpr int64_t kMaxD = (int64_t)1 << 20;
constexpr int kTile = 128;               // tokens of i per workgroup, tokens of j per column tile
// uint4 per staged row: 64 bytes of k (16-bit types: hi, then 64 bytes of lo) + 16 of padding - an odd count, so 16 consecutive
// rows fall into the 16 different 16-byte bank groups
template <class T> constexpr int kPitch = T::kBytes == 4 ? 5 : 9;
template <class T> constexpr int kStageVec = 2 * kTile * kPitch<T>;
template <class T> constexpr int kMainLds = 2 * kStageVec<T> * 16;  // two buffers: 40 960 bytes f32, 73 728 bytes f16 / bf16
constexpr int kMeanCols = 512;           // features per workgroup of the mean kernel: 64 lanes x 8

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct HidDesc { int64_t ptr, batch_stride, row_stride; };  // one step's hidden states of the layer (llm_check.hip)
struct RowWin { int64_t s, T; };                            // the content window of a batch row

// the states of position `pos` of batch row b: step 0 holds positions < P, step g >= 1 position P + g - 1
template <class T>
__device__ __forceinline__ const typename T::elem* token_row(const HidDesc* __restrict__ table, int64_t P, int64_t b, int64_t pos) {
  const HidDesc hd = table[pos < P ? 0 : pos - P + 1];
  return reinterpret_cast<const typename T::elem*>(hd.ptr) + b * hd.batch_stride + (pos < P ? pos : 0) * hd.row_stride;
}

// T::V consecutive elements (16 bytes) from element k (a multiple of T::V), zero past d and for a null row
template <class T>
__device__ __forceinline__ uint4 load_slot(const typename T::elem* row, int64_t k, int64_t d) {
  if (!row || k >= d) return make_uint4(0u, 0u, 0u, 0u);
  if ((reinterpret_cast<uintptr_t>(row) & 15) == 0 && k + T::V <= d) return *reinterpret_cast<const uint4*>(row + k);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if constexpr (T::kBytes == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < d) w[e] = __float_as_uint(row[k + e]);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < d) w[e >> 1] |= (uint32_t)row[k + e] << (16 * (e & 1));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <class T>
__device__ __forceinline__ void widen_slot(uint4 raw, float* v) {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
  if constexpr (T::kBytes == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __uint_as_float(w[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = widen(T{}, (uint16_t)(w[e] & 0xffffu));
      v[2 * e + 1] = widen(T{}, (uint16_t)(w[e] >> 16));
    }
  }
}

// f32 -> the matrix-core input type, to nearest even, by the conversion instructions of the target (a NaN stays a NaN: its
// group is flagged by the norm kernel whatever its payload becomes here)
__device__ __forceinline__ uint32_t round_pair(F16, float lo, float hi) {
  return (uint32_t)narrow(F16{}, lo) | ((uint32_t)narrow(F16{}, hi) << 16);
}
__device__ __forceinline__ uint32_t round_pair(BF16, float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 f = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2));
}

template <class T>
__device__ __forceinline__ uint4 round_slot(const float* v) {
  return make_uint4(round_pair(T{}, v[0], v[1]), round_pair(T{}, v[2], v[3]), round_pair(T{}, v[4], v[5]),
                    round_pair(T{}, v[6], v[7]));
}

// v = (x - m) * inv of one 16-byte slot in f32 -> hi = v (f32) or round(v) and, for a 16-bit type, lo = round(v - hi);
// m: the T::V means of the slot's features
template <class T>
__device__ __forceinline__ void centre_scale(uint4 raw, const float* m, float inv, uint4& hi, uint4& lo) {
  float v[T::V];
  widen_slot<T>(raw, v);
#pragma unroll
  for (int e = 0; e < T::V; ++e) v[e] = (v[e] - m[e]) * inv;
  if constexpr (T::kBytes == 4) {
    hi = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
  } else {
    hi = round_slot<T>(v);
    float h[T::V];
    widen_slot<T>(hi, h);
#pragma unroll
    for (int e = 0; e < T::V; ++e) v[e] -= h[e];  // (exact: both lie within one binade step of each other)
    lo = round_slot<T>(v);
  }
}

template <class T>
__device__ __forceinline__ void mma(f32x16& acc, uint4 a, uint4 b) {
  if constexpr (std::is_same<T, BF16>::value) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  } else if constexpr (std::is_same<T, F16>::value) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
}

__host__ __device__ inline int64_t pairs_of(int64_t k) { return k * (k + 1) / 2; }
// pair q of the upper triangle, row by row: (0,0) (0,1) .. (0,K-1) (1,1) ..
__host__ __device__ inline int64_t pair_index(int64_t i, int64_t j, int64_t k) { return i * k - i * (i - 1) / 2 + (j - i); }

// ---- 0. clear ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cemb_init_kernel(uint32_t* __restrict__ words, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) words[i] = 0u;
}

// ---- 1. group means ---------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void cemb_mean_kernel(const HidDesc* __restrict__ table, const RowWin* __restrict__ rows,
                                                        int64_t K, int64_t P, int64_t d, int64_t dp, int64_t blocks_d,
                                                        float* __restrict__ mean) {
  __shared__ double part[4][kMeanCols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = blockIdx.x / blocks_d, j0 = (blockIdx.x % blocks_d) * kMeanCols + lane * 8;
  double s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.0;
  int64_t before = 0;  // content tokens of the samples in front
  for (int64_t i = 0; i < K; ++i) {
    const RowWin rw = rows[g * K + i];
    // this wave's tokens of the sample: flat index before + t = wave (mod 4)
    for (int64_t t = (wave - before % 4 + 4) % 4; t < rw.T; t += 4) {
      const typename T::elem* row = token_row<T>(table, P, g * K + i, rw.s + t);
      float v[8];
      widen_slot<T>(load_slot<T>(row, j0, d), v);
      if constexpr (T::V == 4) widen_slot<T>(load_slot<T>(row, j0 + 4, d), v + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += (double)v[e];
    }
    before += rw.T;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[wave][lane * 8 + e] = s[e];
  __syncthreads();
  for (int c = threadIdx.x; c < kMeanCols; c += 256) {
    const int64_t j = (blockIdx.x % blocks_d) * kMeanCols + c;
    if (j < d) {
      const double total = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
      mean[g * dp + j] = before > 0 ? (float)(total / (double)before) : 0.f;
    }
  }
}

// ---- 2. inverse norms -------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void cemb_norm_kernel(const HidDesc* __restrict__ table, const RowWin* __restrict__ rows,
                                                        int64_t B, int64_t K, int64_t P, int64_t d, int64_t dp, int64_t Tp,
                                                        int64_t T_max, const float* __restrict__ mean,
                                                        float* __restrict__ inv, uint32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= B * T_max) return;
  const int64_t r = w / T_max, t = w % T_max;
  const RowWin rw = rows[r];
  if (t >= rw.T) return;
  const typename T::elem* row = token_row<T>(table, P, r, rw.s + t);
  const float* m = mean + (r / K) * dp;
  double s = 0.0;
  for (int64_t j = (int64_t)lane * T::V; j < d; j += 64 * T::V) {
    float v[T::V];
    widen_slot<T>(load_slot<T>(row, j, d), v);
#pragma unroll
    for (int e = 0; e < T::V; ++e) {
      const float c = v[e] - m[j + e];  // (past d: 0 - 0, the mean rows are padded with zeros)
      s += (double)c * (double)c;
    }
  }
  s = wave_sum(s);
  if (lane == 0) {
    const bool finite = s < kInfD();  // (false for NaN)
    if (!finite) flags[r / K] = 1u;
    inv[r * Tp + t] = (finite && s > 0.0) ? (float)(1.0 / sqrt(s)) : 0.f;
  }
}

// ---- 3. cosines and their maxima ----------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void cemb_main_kernel(const HidDesc* __restrict__ table, const RowWin* __restrict__ rows,
                                                        int64_t K, int64_t P, int64_t d, int64_t dp, int64_t Tp, int64_t nrb,
                                                        const float* __restrict__ mean, const float* __restrict__ inv,
                                                        float* __restrict__ rowmax, uint32_t* __restrict__ colkeys) {
  extern __shared__ __attribute__((aligned(16))) uint4 cemb_stage[];  // 2 x (128 rows of i + 128 rows of j) x the row pitch
  uint4* stage = cemb_stage;
  constexpr int pitch = kPitch<T>, stage_vec = kStageVec<T>;
  constexpr bool split = T::kBytes == 2;  // hi and lo elements
  __shared__ uint32_t rowkey[kTile], colkey[kTile];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave & 1, wc = wave >> 1;  // this wave's half of the rows (tokens of i) and of the columns (tokens of j)
  const int64_t npairs = pairs_of(K);
  const int64_t rb = blockIdx.x % nrb, q = (blockIdx.x / nrb) % npairs, g = blockIdx.x / (nrb * npairs);
  int64_t i = 0, j = q;  // row i of the upper triangle holds K - i pairs
  while (j >= K - i) { j -= K - i; ++i; }
  j += i;
  const int64_t ri = g * K + i, rj = g * K + j;
  const RowWin wi = rows[ri], wj = rows[rj];
  const int64_t a0 = rb * kTile;
  if (a0 >= wi.T || wj.T == 0) return;  // (uniform, in front of every barrier)

  const int srow = tid >> 2, sq = tid & 3;  // staging: 16-byte slot sq of tile rows srow and srow + 64
  const typename T::elem* arow[2];
  const typename T::elem* brow[2];
  float ainv[2], binv[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t a = a0 + srow + 64 * h;
    const bool ok = a < wi.T;
    arow[h] = ok ? token_row<T>(table, P, ri, wi.s + a) : nullptr;
    ainv[h] = ok ? inv[ri * Tp + a] : 0.f;
  }
  if (tid < kTile) rowkey[tid] = colkey[tid] = 0u;  // below the key of every value (the sweeps below are behind barriers)
  const float* gmean = mean + g * dp;

  constexpr int kPerStage = 4 * T::V;
  const int64_t nstage = (d + kPerStage - 1) / kPerStage;
  const int64_t ntiles = (wj.T + kTile - 1) / kTile;
  for (int64_t ct = 0; ct < ntiles; ++ct) {
    const int64_t b0 = ct * kTile;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t b = b0 + srow + 64 * h;
      const bool ok = b < wj.T;
      brow[h] = ok ? token_row<T>(table, P, rj, wj.s + b) : nullptr;
      binv[h] = ok ? inv[rj * Tp + b] : 0.f;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    uint4 fa[2], fb[2];
    float fm[T::V];
    auto fetch = [&](int64_t sg) {
      const int64_t k = sg * kPerStage + sq * T::V;  // (< dp: the mean rows are padded to whole stages)
#pragma unroll
      for (int e = 0; e < T::V; e += 4) {
        const float4 m4 = *reinterpret_cast<const float4*>(gmean + k + e);
        fm[e] = m4.x, fm[e + 1] = m4.y, fm[e + 2] = m4.z, fm[e + 3] = m4.w;
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        fa[h] = load_slot<T>(arow[h], k, d);
        fb[h] = load_slot<T>(brow[h], k, d);
      }
    };
    auto store = [&](int buf) {
      uint4* base = stage + buf * stage_vec;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        uint4 hi, lo;
        centre_scale<T>(fa[h], fm, ainv[h], hi, lo);
        base[(srow + 64 * h) * pitch + sq] = hi;
        if constexpr (split) base[(srow + 64 * h) * pitch + 4 + sq] = lo;
        centre_scale<T>(fb[h], fm, binv[h], hi, lo);
        base[(kTile + srow + 64 * h) * pitch + sq] = hi;
        if constexpr (split) base[(kTile + srow + 64 * h) * pitch + 4 + sq] = lo;
      }
    };
    fetch(0);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int64_t sg = 0; sg < nstage; ++sg) {
      const bool more = sg + 1 < nstage;  // (uniform)
      if (more) fetch(sg + 1);
      const uint4* pa = stage + buf * stage_vec + (wr * 64 + li) * pitch + lh;
      const uint4* pb = stage + buf * stage_vec + (kTile + wc * 64 + li) * pitch + lh;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint4 xa[2], xb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) xa[a] = pa[a * 32 * pitch + 2 * s];
#pragma unroll
        for (int b = 0; b < 2; ++b) xb[b] = pb[b * 32 * pitch + 2 * s];
        if constexpr (split) {  // the two small products first, then hi hi'
          uint4 la[2], lb[2];
#pragma unroll
          for (int a = 0; a < 2; ++a) la[a] = pa[a * 32 * pitch + 4 + 2 * s];
#pragma unroll
          for (int b = 0; b < 2; ++b) lb[b] = pb[b * 32 * pitch + 4 + 2 * s];
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
              mma<T>(acc[a][b], la[a], xb[b]);
              mma<T>(acc[a][b], xa[a], lb[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int a = 0; a < 2; ++a) mma<T>(acc[a][b], xa[a], xb[b]);
      }
      __builtin_amdgcn_sched_barrier(0);  // (the fetched values are first touched here)
      if (more) store(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }

    // ---- the tile's maxima: acc[a][b][r] is row wr 64 + 32 a + (r & 3) + 8 (r >> 2) + 4 lh, column wc 64 + 32 b + li ----
    const float ninf = -__builtin_inff();
    float cmax[2] = {ninf, ninf};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * 64 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const bool row_ok = a0 + row < wi.T;
        float rmax = ninf;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float v = acc[a][b][r];
          if (row_ok) cmax[b] = v > cmax[b] ? v : cmax[b];
          const float u = b0 + wc * 64 + 32 * b + li < wj.T ? v : ninf;
          rmax = u > rmax ? u : rmax;
        }
        rmax = wave_reduce<32>(rmax, [](float x, float y) { return x > y ? x : y; });
        if (li == 0 && row_ok) atomicMax(&rowkey[row], asc_key(rmax));
      }
    if (i != j) {  // (uniform; a sample against itself needs one direction)
#pragma unroll
      for (int b = 0; b < 2; ++b) atomicMax(&colkey[wc * 64 + 32 * b + li], asc_key(cmax[b]));
    }
    __syncthreads();
    if (i != j && tid < kTile) {
      const int64_t b = b0 + tid;
      if (b < wj.T) atomicMax(&colkeys[(g * npairs + q) * Tp + b], colkey[tid]);
      colkey[tid] = 0u;  // (its next atomics are behind the barriers of the next tile's stages)
    }
  }
  // (the last __syncthreads above closes the row keys)
  if (tid < kTile && a0 + tid < wi.T) rowmax[(g * npairs + q) * Tp + a0 + tid] = asc_value(rowkey[tid]);
}

// ---- 4. coverage --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cemb_finish_kernel(const RowWin* __restrict__ rows, int64_t G, int64_t K, int64_t Tp,
                                                          const float* __restrict__ rowmax,
                                                          const uint32_t* __restrict__ colkeys,
                                                          const uint32_t* __restrict__ flags, double* __restrict__ cov) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= G * K * K) return;
  const int64_t j = w % K, i = (w / K) % K, g = w / (K * K);
  const int64_t ni = rows[g * K + i].T, nj = rows[g * K + j].T;
  double out;
  if (flags[g]) {
    out = __builtin_nan("");
  } else if (ni == 0 || nj == 0) {
    out = (ni == 0 && nj == 0) ? 1.0 : 0.0;
  } else {
    const int64_t npairs = pairs_of(K);
    double s = 0.0;
    if (i <= j) {
      const float* src = rowmax + (g * npairs + pair_index(i, j, K)) * Tp;
      for (int64_t t = lane; t < ni; t += 64) s += (double)src[t];
    } else {
      const uint32_t* src = colkeys + (g * npairs + pair_index(j, i, K)) * Tp;
      for (int64_t t = lane; t < ni; t += 64) s += (double)asc_value(src[t]);
    }
    out = wave_sum(s) / (double)ni;
  }
  if (lane == 0) cov[w] = out;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int64_t padded_t(int64_t T_max) { return T_max < 1 ? kTile : (T_max + kTile - 1) / kTile * kTile; }
int64_t padded_d(int64_t d) { return (d + 31) / 32 * 32; }  // whole stages of every element type

struct Plan {
  uint32_t* cleared;  // mean | flags | colkeys, one run of 32-bit words that launch 0 clears
  float* mean;        // [G, dp]
  uint32_t* flags;    // [G]
  uint32_t* colkeys;  // [G, pairs, Tp]
  int64_t cleared_words;
  float* inv;         // [G K, Tp]
  float* rowmax;      // [G, pairs, Tp]
};
Plan make_plan(WsWalk& w, int64_t G, int64_t K, int64_t T_max, int64_t d) {
  const int64_t tp = padded_t(T_max), dp = padded_d(d), np = pairs_of(K);
  Plan p;
  p.mean = w.take<float>((size_t)(G * dp), 16);
  p.flags = w.take<uint32_t>((size_t)G, 16);
  p.colkeys = w.take<uint32_t>((size_t)(G * np * tp), 16);
  p.cleared = reinterpret_cast<uint32_t*>(p.mean);
  p.cleared_words = (int64_t)(w.used() / 4);
  p.inv = w.take<float>((size_t)(G * K * tp), 16);
  p.rowmax = w.take<float>((size_t)(G * np * tp), 16);
  return p;
}

bool dims_ok(int64_t G, int64_t K, int64_t T_max, int64_t d) {
  return G >= 1 && K >= 2 && K <= kMaxK && T_max >= 0 && T_max <= kMaxT && d >= 1 && d <= kMaxD && G <= (1 << 20) / K;
}

}  // namespace

extern "C" int64_t runia_cons_embed_workspace_bytes(int64_t groups, int64_t k, int64_t T_max, int64_t d) {
  if (!dims_ok(groups, k, T_max, d)) return 0;
  return (int64_t)ws_bytes([&](WsWalk& w) { make_plan(w, groups, k, T_max, d); });
}

extern "C" int runia_cons_embed(const void* table, const void* rows, const int64_t* host_rows, int dtype, int64_t groups,
                                int64_t k, int64_t n_steps, int64_t P, int64_t d, int center, double* cov, void* workspace,
                                size_t workspace_bytes, runia_stream_t stream) {
  if (!table || !rows || !host_rows || !cov || !elem_dtype_ok(dtype) || n_steps < 1 || P < 1 || !dims_ok(groups, k, 0, d))
    return RUNIA_E_INVALID;
  const int64_t B = groups * k, n_pos = P + n_steps - 1;
  int64_t t_max = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t s = host_rows[2 * b], T = host_rows[2 * b + 1];
    if (s < 0 || T < 0 || T > kMaxT || T > n_pos || s > n_pos - T) return RUNIA_E_INVALID;
    if (T > t_max) t_max = T;
  }
  WsWalk w(workspace);
  const Plan plan = make_plan(w, groups, k, t_max, d);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  const int64_t tp = padded_t(t_max), dp = padded_d(d), nrb = tp / kTile, blocks_d = (d + kMeanCols - 1) / kMeanCols;
  hipStream_t s = as_stream(stream);
  const HidDesc* tab = static_cast<const HidDesc*>(table);
  const RowWin* rw = static_cast<const RowWin*>(rows);
  static std::atomic<uint64_t> main_ok[3];
  const int lds_rc = dispatch_elem(dtype, [&](auto tag) {  // (before the first launch: a refusal leaves nothing half done)
    using T = decltype(tag);
    return runia_allow_dynamic_lds(reinterpret_cast<const void*>(cemb_main_kernel<T>), kMainLds<T>, main_ok[dtype]);
  });
  if (lds_rc) return lds_rc;
  cemb_init_kernel<<<runia_stream_grid(plan.cleared_words, 256), 256, 0, s>>>(plan.cleared, plan.cleared_words);
  dispatch_elem(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (t_max > 0) {
      if (center)
        cemb_mean_kernel<T><<<(unsigned)(groups * blocks_d), 256, 0, s>>>(tab, rw, k, P, d, dp, blocks_d, plan.mean);
      cemb_norm_kernel<T><<<(unsigned)((B * t_max + 3) / 4), 256, 0, s>>>(tab, rw, B, k, P, d, dp, tp, t_max, plan.mean,
                                                                           plan.inv, plan.flags);
      RUNIA_LAUNCH_TIMED(cemb_main_kernel<T>, (unsigned)(groups * pairs_of(k) * nrb), 256, kMainLds<T>, s, tab, rw, k, P, d, dp, tp,
                         nrb, plan.mean, plan.inv, plan.rowmax, plan.colkeys);
    }
    return (int)RUNIA_OK;
  });
  cemb_finish_kernel<<<(unsigned)((groups * k * k + 3) / 4), 256, 0, s>>>(rw, groups, k, tp, plan.rowmax, plan.colkeys,
                                                                          plan.flags, cov);
  return runia_check_launch();
}
