// Kernel two-sample tests on the device (evaluation/shift.py): the MMD permutation test of Gretton et al. and the
// energy distance on two row tables X [n, D], Y [m, D], pooled Z = [X; Y], N = n + m <= 2^18.
//   * shift_perm_bits_kernel: one workgroup per permutation finds the n-th smallest (word, i) key (shift_perm.hpp) with histogram
//     passes that regenerate the Philox words, and writes the membership as packed bits (row p, bit i, u32 words).
//   * shift_colsum / shift_mean / shift_norms: the pooled column mean in f32 (f64 sums in a fixed order) and the squared norms of the
//     centred rows.  The linear kernel is not translation invariant: its mean is zero.
//   * shift_fused_kernel: grid = 32-column I tiles x J segments (<= 2048 pooled rows).  Per 128-row J step every wave forms one
//     32 x 32 tile X = Z_J Z_I^T on v_mfma_f32_32x32x2_f32 (rows j in the registers, column i on the lane), applies the kernel
//     function in registers, splits the values into three exact bf16 pieces and leaves them in LDS as ready B fragments; then every
//     wave accumulates Q^T[p, i] += sum_j a_p[j] X[j, i] for ITS quarter of the permutation columns on v_mfma_f32_32x32x16_bf16,
//     the 0/1 memberships expanded from the bits as the A operand.  The product sums over the row index of X, so the accumulator
//     layout of the first product is the operand layout of the second; K is symmetric, hence the (J, I) orientation.  An
//     all-ones column behind the permutation columns gives the row sums.  At the end of the segment the workgroup writes
//     sum_i a_p[i] Q^T[p, i] (for t) and sum_i a_p[i] Q^T[ones, i] (for u) per (I tile, segment, column).  The N x N kernel matrix
//     never exists.
//   * shift_reduce_kernel / shift_stats_kernel: f64 sums of the partials in an order fixed by the shape, the statistics of all
//     permutations, the count and the p-value.  No float atomics anywhere: the same bits from call to call.
#include "common.hpp"
#include "elem.hpp"
#include "shift_perm.hpp"

#include <algorithm>
#include <vector>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

enum { kRbf = 0, kEnergy = 1, kLinear = 2 };
enum { kBiased = 0, kUnbiased = 1 };

constexpr int kTI = 32, kTJ = 128, kKC = 32, kKP = 34;  // I tile, J step, staged k chunk and its LDS pitch
constexpr int kMaxSeg = 2048;                            // pooled rows of a J segment: the longest f32 chain
constexpr int kMaxChunkCols = 1024;                      // columns of one launch, identity and ones columns included
constexpr int kMaxBandwidths = 8;
constexpr int kMeanSegs = 64;
constexpr int kSampleRows = 2048;
constexpr size_t kPartBudget = (size_t)64 << 20;         // bytes of partials kept at once
// Ablation (profiles/README.md, shift_ablate): 1 = the memberships of a launch's columns are expanded once into a bf16 table of ready
// A fragments in the workspace (64 bytes per column and 32 rows); 0 = expanded from the bits inside the loop.
#ifndef SHIFT_MEMBER_TABLE
#define SHIFT_MEMBER_TABLE 0
#endif

// ---- memberships ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void shift_perm_bits_kernel(uint64_t seed, uint32_t n, uint32_t N, uint32_t first,
                                                              uint32_t* __restrict__ bits, int64_t row_words) {
  __shared__ uint32_t hist[runia_shift::kBuckets];
  __shared__ uint32_t part[256];
  __shared__ uint64_t s_prefix;
  __shared__ uint32_t s_rank;
  const int tid = threadIdx.x;
  const uint32_t p = first + blockIdx.x;
  uint32_t* row = bits + (int64_t)blockIdx.x * row_words;
  uint64_t thr = 0;
  if (p != 0u) {  // (uniform over the workgroup)
    uint64_t prefix = 0, mask = 0;
    uint32_t k = n - 1u;
    for (int pass = 0; pass < runia_shift::kPasses; ++pass) {
      const int shift = runia_shift::pass_shift(pass), width = runia_shift::pass_width(pass);
      for (int b = tid; b < runia_shift::kBuckets; b += 256) hist[b] = 0u;
      __syncthreads();
      for (uint32_t i = tid; i < N; i += 256u) {
        const uint64_t key = runia_shift::key(seed, p, i);
        if ((key & mask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & ((1u << width) - 1u)], 1u);  // (LDS, integer)
      }
      __syncthreads();
      uint32_t s = 0u;
#pragma unroll
      for (int e = 0; e < 8; ++e) s += hist[8 * tid + e];
      part[tid] = s;
      __syncthreads();
      if (tid == 0) {
        uint32_t kk = k;
        const int g = runia_shift::find_bucket(part, 256, kk);
        const int b = 8 * g + runia_shift::find_bucket(hist + 8 * g, 8, kk);
        s_prefix = prefix | ((uint64_t)b << shift);
        s_rank = kk;
      }
      __syncthreads();
      prefix = s_prefix;
      k = s_rank;
      mask |= ((1ull << width) - 1ull) << shift;
    }
    thr = prefix;  // the n-th smallest key
  }
  for (int64_t w = tid; w < row_words; w += 256) {
    uint32_t v = 0u;
    for (int b = 0; b < 32; ++b) {
      const int64_t i = w * 32 + b;
      if (i < (int64_t)N) {
        const bool in = (p == 0u) ? (i < (int64_t)n) : (runia_shift::key(seed, p, (uint32_t)i) <= thr);
        v |= (in ? 1u : 0u) << b;
      }
    }
    row[w] = v;
  }
}

// ---- rows of the pooled table -------------------------------------------------------------------------------------------------
struct Rows {
  const void* x;
  const void* y;
  int64_t n, N, D, sx, sy;  // row strides in elements
};

template <class T>
__device__ __forceinline__ const typename T::elem* row_ptr(const Rows& r, int64_t g) {
  typedef const typename T::elem* P;
  return g < r.n ? reinterpret_cast<P>(r.x) + g * r.sx : reinterpret_cast<P>(r.y) + (g - r.n) * r.sy;
}

// four consecutive elements from element k of a row (k % 4 == 0): one aligned load when `vec`, element loads otherwise; 0 past D
template <class T>
__device__ __forceinline__ void ld4(const typename T::elem* p, int64_t k, int64_t D, bool vec, float* v) {
  if (vec && k + 4 <= D) {
    if constexpr (T::kBytes == 4) ld16<T>(p + k, v);
    else ld8<T>(p + k, v);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (k + e < D) ? ld1<T>(p + k + e) : 0.f;
  }
}

template <class T>
__device__ __forceinline__ bool rows_vec(const Rows& r) {
  const uintptr_t a = T::kBytes == 4 ? 15 : 7;
  return ((r.sx | r.sy) & 3) == 0 && (((uintptr_t)r.x | (uintptr_t)r.y) & a) == 0;
}

template <class T>
__global__ __launch_bounds__(256) void shift_colsum_kernel(Rows r, double* __restrict__ colpart, int64_t rows_per) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= r.D) return;
  const int64_t g0 = (int64_t)blockIdx.y * rows_per, g1 = g0 + rows_per < r.N ? g0 + rows_per : r.N;
  double s = 0.0;
  for (int64_t g = g0; g < g1; ++g) s += (double)ld1<T>(row_ptr<T>(r, g) + col);
  colpart[(int64_t)blockIdx.y * r.D + col] = s;
}

__global__ __launch_bounds__(256) void shift_mean_kernel(const double* __restrict__ colpart, int nseg, int64_t N, int64_t D,
                                                         int centre, float* __restrict__ mean) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= D) return;
  double s = 0.0;
  for (int k = 0; k < nseg; ++k) s += colpart[(int64_t)k * D + col];  // (the segments in order)
  mean[col] = centre ? (float)(s / (double)N) : 0.f;
}

// squared norms of the centred rows, 0 for the padding rows N .. Npad - 1
template <class T>
__global__ __launch_bounds__(64 * kRowWaves) void shift_norms_kernel(Rows r, const float* __restrict__ mean, int64_t Npad,
                                                                      float* __restrict__ norms) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * kRowWaves + wave;
  if (g >= Npad) return;
  float s = 0.f;
  if (g < r.N) {
    const typename T::elem* p = row_ptr<T>(r, g);
    for (int64_t k = lane; k < r.D; k += 64) {
      const float v = ld1<T>(p + k) - mean[k];
      s = fmaf(v, v, s);
    }
    s = wave_sum_f32(s);
  }
  if (lane == 0) norms[g] = s;
}

// ---- the fused statistic kernel -----------------------------------------------------------------------------------------------
struct FusedArgs {
  Rows r;
  const float* mean;
  const float* norms;
  const uint32_t* bits;
  int64_t row_words, p0;
  int ncols;          // permutation columns of this launch; the ones column is column `ncols`
  int dtype, kind, nbw;
  float g[kMaxBandwidths];  // 1 / (2 sigma^2)
  int64_t seg_len, it0;
  int nseg, cstride;
  float* part_t;
  float* part_u;
  const uint4* table;  // SHIFT_MEMBER_TABLE: [word of 32 rows][column][2 s + h] fragments
};

__device__ __forceinline__ uint32_t member_word(const FusedArgs& a, int c, int64_t w) {
  if (c < a.ncols) return a.bits[(a.p0 + c) * a.row_words + w];
  if (c == a.ncols) {  // the ones column: the rows that exist
    const int64_t rem = a.r.N - w * 32;
    return rem >= 32 ? 0xffffffffu : (rem <= 0 ? 0u : ((1u << (int)rem) - 1u));
  }
  return 0u;
}

// A ROWS x 32 chunk of the pooled rows row0 ... at k0 ... (zero outside the table), in two halves so that the global loads of the
// next chunk are in flight while the matrix cores work on this one (as nt_tile_f32.hpp):
//   load_rows : global -> ROWS / 8 registers per thread
//   store_rows: registers -> LDS
// The values are staged as they are read; the chunk's 32 means sit beside them in LDS and are subtracted as the operands are
// read (the same f32 subtraction as in shift_norms_kernel).  A row past the table thus enters the product as -mean: its
// memberships are 0 in every column, the ones column included.
template <class T, int ROWS>
__device__ __forceinline__ void load_rows(const Rows& r, int64_t row0, int64_t k0, float (&v)[ROWS * kKC / 256], int tid,
                                          bool vec) {
  constexpr int kPer = ROWS * kKC / 256, kTpr = kKC / kPer;  // elements per thread, threads per row
  static_assert(kPer % 4 == 0, "whole groups of four");
  const int row = tid / kTpr, kk = (tid % kTpr) * kPer;
  const int64_t g = row0 + row;
  const typename T::elem* p = row_ptr<T>(r, g < r.N ? g : 0);
#pragma unroll
  for (int e = 0; e < kPer; e += 4) {
    const int64_t k = k0 + kk + e;
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    if (g < r.N && k < r.D) ld4<T>(p, k, r.D, vec, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[e + j] = w[j];
  }
}

template <int ROWS>
__device__ __forceinline__ void store_rows(const float (&v)[ROWS * kKC / 256], float (*dst)[kKP], int tid) {
  constexpr int kPer = ROWS * kKC / 256, kTpr = kKC / kPer;
  const int row = tid / kTpr, kk = (tid % kTpr) * kPer;
#pragma unroll
  for (int e = 0; e < kPer; e += 2) *reinterpret_cast<float2*>(&dst[row][kk + e]) = make_float2(v[e], v[e + 1]);
}

template <class T>
__device__ __forceinline__ void load_both(const FusedArgs& a, int64_t J0, int64_t I0, int64_t k0, float (&vj)[kTJ * kKC / 256],
                                          float (&vi)[kTI * kKC / 256], int tid) {
  const bool vec = rows_vec<T>(a.r);
  load_rows<T, kTJ>(a.r, J0, k0, vj, tid, vec);
  load_rows<T, kTI>(a.r, I0, k0, vi, tid, vec);
}

__device__ __forceinline__ uint32_t bf16_bits(float f) { return (uint32_t)narrow(BF16{}, f); }
__device__ __forceinline__ float bf16_value(uint32_t b) { return __uint_as_float(b << 16); }

// two membership bits (bit 0 -> low half) as a pair of bf16 0 / 1
__device__ __forceinline__ uint32_t member_pair(uint32_t two_bits) {
  return ((two_bits & 1u) | ((two_bits & 2u) << 15)) * 0x3f80u;
}

// the A fragment of k step s, lane half h, from a column's membership word of 32 rows: element e is row 16 s + 8 (e >> 2) + 4 h + (e & 3)
__device__ __forceinline__ uint4 member_fragment(uint32_t word, int s, int h) {
  const uint32_t v = word >> (16 * s + 4 * h);
  return make_uint4(member_pair(v), member_pair(v >> 2), member_pair(v >> 8), member_pair(v >> 10));
}

#if SHIFT_MEMBER_TABLE
__global__ __launch_bounds__(256) void shift_member_table_kernel(FusedArgs a, uint4* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (word, column)
  if (i >= a.row_words * a.cstride) return;
  const uint32_t mw = member_word(a, (int)(i % a.cstride), i / a.cstride);
#pragma unroll
  for (int f = 0; f < 4; ++f) table[i * 4 + f] = member_fragment(mw, f >> 1, f & 1);
}
#endif

template <int NT>
__global__ __launch_bounds__(256) void shift_fused_kernel(FusedArgs a) {
  __shared__ __attribute__((aligned(16))) float zj[kTJ][kKP];
  __shared__ __attribute__((aligned(16))) float zi[kTI][kKP];
  __shared__ __attribute__((aligned(16))) uint4 frag[4][2][3][64];  // [wave of X][k step][piece][lane]
  __shared__ float nrm[kTJ];
  __shared__ float rsum[kTI];
  __shared__ __attribute__((aligned(8))) float mk[kKC];  // the chunk's means, 0 past D
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int64_t N = a.r.N, D = a.r.D;
  const int64_t it = a.it0 + blockIdx.x, I0 = it * kTI;
  const int64_t Jbeg = (int64_t)blockIdx.y * a.seg_len, Jend = Jbeg + a.seg_len < N ? Jbeg + a.seg_len : N;
  const int64_t icol = I0 + li;
  const float ni = icol < N ? a.norms[icol] : 0.f;

  f32x16 q[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) q[t][r] = 0.f;

  float vj[kTJ * kKC / 256], vi[kTI * kKC / 256], vm = 0.f;
  auto load_chunk = [&](int64_t J0, int64_t k0) {
    if (tid < kKC) vm = (k0 + tid < D) ? a.mean[k0 + tid] : 0.f;
    switch (a.dtype) {
      case kF32: load_both<F32>(a, J0, I0, k0, vj, vi, tid); break;
      case kF16: load_both<F16>(a, J0, I0, k0, vj, vi, tid); break;
      default: load_both<BF16>(a, J0, I0, k0, vj, vi, tid); break;
    }
  };
  load_chunk(Jbeg, 0);
  for (int64_t J0 = Jbeg; J0 < Jend; J0 += kTJ) {
    // ---- X = Z_J Z_I^T: rows j in the registers, column i on the lane ----
    f32x16 x;
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = 0.f;
    for (int64_t k0 = 0; k0 < D; k0 += kKC) {
      __syncthreads();  // the previous chunk (and the previous step's norms and fragments) has been read
      if (k0 == 0 && tid < kTJ) nrm[tid] = a.norms[J0 + tid];  // (norms are padded to whole J steps)
      store_rows<kTJ>(vj, zj, tid);
      store_rows<kTI>(vi, zi, tid);
      if (tid < kKC) mk[tid] = vm;
      __syncthreads();
      // the next chunk's loads fly while the matrix cores consume this one (across the J steps as well)
      if (k0 + kKC < D) load_chunk(J0, k0 + kKC);
      else if (J0 + kTJ < Jend) load_chunk(J0 + kTJ, 0);
#pragma unroll
      for (int s = 0; s < kKC / 4; ++s) {
        const float2 av = *reinterpret_cast<const float2*>(&zj[wave * 32 + li][4 * s + 2 * lh]);
        const float2 bv = *reinterpret_cast<const float2*>(&zi[li][4 * s + 2 * lh]);
        const float2 mv = *reinterpret_cast<const float2*>(&mk[4 * s + 2 * lh]);
        x = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x - mv.x, bv.x - mv.x, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y - mv.y, bv.y - mv.y, x, 0, 0, 0);
      }
    }
    // ---- the kernel function, in registers; register r is row (r & 3) + 8 (r >> 2) + 4 lh of the wave's tile ----
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jl = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      float v = x[r];
      if (a.kind != kLinear) {
        float d2 = (nrm[jl] + ni) - 2.0f * v;
        d2 = d2 < 0.f ? 0.f : d2;             // (a NaN stays a NaN)
        if (J0 + jl == icol) d2 = 0.f;        // the diagonal, exactly
        if (a.kind == kRbf) {
          v = 0.f;
          for (int b = 0; b < a.nbw; ++b) v += exp_nonpos(-d2 * a.g[b]);
        } else {
          v = -sqrtf(d2);
        }
      }
      x[r] = v;
    }
    // ---- three exact bf16 pieces, stored as the B fragments of the second product: the fragment of k step s is registers
    //      8 s .. 8 s + 7, element e of lane half h being row 16 s + 8 (e >> 2) + 4 h + (e & 3) of X ----
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      uint32_t w[3][4];
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        uint32_t pc[2][3];
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          const float v = x[8 * s + e + o];
          const uint32_t hi = bf16_bits(v);
          const float r1 = v - bf16_value(hi);
          const uint32_t mid = bf16_bits(r1);
          const float r2 = r1 - bf16_value(mid);
          pc[o][0] = hi; pc[o][1] = mid; pc[o][2] = bf16_bits(r2);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c][e >> 1] = pc[0][c] | (pc[1][c] << 16);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) frag[wave][s][c][lane] = make_uint4(w[c][0], w[c][1], w[c][2], w[c][3]);
    }
    __syncthreads();
    // ---- Q^T[p, i] += sum_j a_p[j] X[j, i] for this wave's columns: memberships are the A operand (lane = column p) ----
#pragma unroll 1
    for (int wx = 0; wx < 4; ++wx) {
      bf16x8 b[2][3];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[s][c] = __builtin_bit_cast(bf16x8, frag[wx][s][c][lane]);
      const int64_t wj = J0 / 32 + wx;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#if SHIFT_MEMBER_TABLE
        const uint4* tf = a.table + (wj * a.cstride + (wave * NT + t) * 32 + li) * 4 + lh;
#else
        const uint32_t mw = member_word(a, (wave * NT + t) * 32 + li, wj);
#endif
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#if SHIFT_MEMBER_TABLE
          const bf16x8 am = __builtin_bit_cast(bf16x8, tf[2 * s]);
#else
          const bf16x8 am = __builtin_bit_cast(bf16x8, member_fragment(mw, s, lh));
#endif
#pragma unroll
          for (int c = 0; c < 3; ++c) q[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, b[s][c], q[t], 0, 0, 0);
        }
      }
    }
  }

  // ---- the segment's partials: sum_i a_p[i] Q^T[p, i] and sum_i a_p[i] Q^T[ones, i] ----
  {
    const int ot = a.ncols >> 5, orow = a.ncols & 31;  // the ones column: tile, row in the tile
    const int oreg = (orow & 3) + 4 * (orow >> 3), oh = (orow >> 2) & 1;
    __syncthreads();
    if (wave == ot / NT && lh == oh) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t == ot % NT && r == oreg) rsum[li] = q[t][r];
    }
    __syncthreads();
  }
  const float ri = rsum[li];
  const int64_t ent = ((int64_t)blockIdx.x * a.nseg + blockIdx.y) * a.cstride;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = (wave * NT + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const bool in = (member_word(a, c, it) >> li) & 1u;
      float tv = in ? q[t][r] : 0.f, uv = in ? ri : 0.f;
      tv = wave_sum<32>(tv);  // (the 32 lanes of a half)
      uv = wave_sum<32>(uv);
      if (li == 0) {
        a.part_t[ent + c] = tv;
        a.part_u[ent + c] = uv;
      }
    }
}

// ---- sums of the partials, statistics -------------------------------------------------------------------------------------------
// block = 32 columns x 8 entry lanes; every column's entries are summed in f64 in an order fixed by (nent, 8)
__global__ __launch_bounds__(256) void shift_reduce_kernel(const float* __restrict__ part_t, const float* __restrict__ part_u,
                                                           int64_t nent, int cstride, int ncols, int64_t p0, int accumulate,
                                                           double* __restrict__ t, double* __restrict__ u, double* __restrict__ su) {
  __shared__ double st[8][32], sv[8][32];
  const int cl = threadIdx.x & 31, el = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  double x = 0.0, y = 0.0;
  if (c <= ncols)
    for (int64_t e = el; e < nent; e += 8) {
      x += (double)part_t[e * cstride + c];
      y += (double)part_u[e * cstride + c];
    }
  st[el][cl] = x;
  sv[el][cl] = y;
  __syncthreads();
  if (el == 0 && c <= ncols) {
    for (int k = 1; k < 8; ++k) { x += st[k][cl]; y += sv[k][cl]; }
    double* dt = c < ncols ? t + p0 + c : su;  // the ones column's u is S
    double* du = c < ncols ? u + p0 + c : su + 1;
    if (c == ncols) x = y;
    *dt = accumulate ? *dt + x : x;
    *du = accumulate ? *du + y : y;
  }
}

// linear kernel, unbiased estimator: sum of k_ii = |z_i|^2 over the first set of permutation p (block p), over all rows (block P)
__global__ __launch_bounds__(256) void shift_diag_kernel(const float* __restrict__ norms, const uint32_t* __restrict__ bits,
                                                         int64_t row_words, int64_t N, int64_t P, double* __restrict__ diag) {
  __shared__ double sh[256];
  const int64_t p = blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) {
    const bool in = p == P || ((bits[p * row_words + (i >> 5)] >> (i & 31)) & 1u);
    s += in ? (double)norms[i] : 0.0;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) diag[p] = sh[0];
}

__device__ __forceinline__ double shift_stat(double t, double u, double S, double dA, double dB, double n, double m, int unbiased) {
  const double AA = t, AB = u - t, BB = S - 2.0 * u + t;
  if (unbiased) return (AA - dA) / (n * (n - 1.0)) + (BB - dB) / (m * (m - 1.0)) - 2.0 * AB / (n * m);
  return AA / (n * n) + BB / (m * m) - 2.0 * AB / (n * m);
}

__global__ __launch_bounds__(256) void shift_stats_kernel(const double* __restrict__ t, const double* __restrict__ u,
                                                          const double* __restrict__ su, const double* __restrict__ diag, int64_t P,
                                                          int64_t n, int64_t m, int kind, int nbw, int unbiased,
                                                          double* __restrict__ S, double* __restrict__ stats,
                                                          long long* __restrict__ count, double* __restrict__ p_value) {
  __shared__ unsigned long long cnt;
  if (threadIdx.x == 0) cnt = 0ull;
  __syncthreads();
  const double dn = (double)n, dm = (double)m, s = su[0];
  auto stat_of = [&](int64_t p) {
    double dA = 0.0, dB = 0.0;
    if (kind == kRbf) { dA = dn * nbw; dB = dm * nbw; }
    else if (kind == kLinear && unbiased) { dA = diag[p]; dB = diag[P] - diag[p]; }
    return shift_stat(t[p], u[p], s, dA, dB, dn, dm, unbiased);
  };
  const double s0 = stat_of(0);
  unsigned long long mine = 0ull;
  for (int64_t p = threadIdx.x; p < P; p += 256) {
    const double v = stat_of(p);
    stats[p] = v;
    if (p >= 1 && v >= s0) ++mine;
  }
  atomicAdd(&cnt, mine);  // (LDS, integer)
  __syncthreads();
  if (threadIdx.x == 0) {
    *S = s;
    *count = (long long)cnt;
    *p_value = (s0 == s0) ? (1.0 + (double)cnt) / (double)P : __builtin_nan("");  // P = 1 + n_perm
  }
}

// ---- the median's sample ----------------------------------------------------------------------------------------------------
// out[k M - k (k + 1) / 2 + (l - k - 1)] = |z_a - z_b| for sample rows k < l, row k of the sample being pooled row floor(k N / M)
template <class T>
__global__ __launch_bounds__(256) void shift_pairwise_kernel(Rows r, int64_t M, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k = blockIdx.x;
  const typename T::elem* pa = row_ptr<T>(r, k * r.N / M);
  for (int64_t l = k + 1 + wave; l < M; l += 4) {
    const typename T::elem* pb = row_ptr<T>(r, l * r.N / M);
    float s = 0.f;
    for (int64_t c = lane; c < r.D; c += 64) {
      const float d = ld1<T>(pa + c) - ld1<T>(pb + c);
      s = fmaf(d, d, s);
    }
    s = wave_sum_f32(s);
    if (lane == 0) out[k * M - k * (k + 1) / 2 + (l - k - 1)] = sqrtf(s);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct Plan {
  int64_t N, Npad, row_words, P, nit, seg_len, nit_batch;
  int nseg, nsegm, NT, cstride, chunk_cols;
  // the regions of the workspace (256-byte slots)
  float *mean, *norms, *part_t, *part_u;
  double *colpart, *su, *diag;
  uint32_t* bits;
  uint4* table;
};

bool make_plan(WsWalk& w, int64_t n, int64_t m, int64_t d, int64_t n_perm, Plan& pl) {
  if (n < 1 || m < 1 || d < 1 || d >= (1ll << 31) || n_perm < 1 || n_perm >= (1ll << 31)) return false;
  if (n + m > runia_shift::kMaxRows) return false;
  pl.N = n + m;
  pl.Npad = round_up(pl.N, kTJ);
  pl.row_words = pl.Npad / 32;
  pl.P = 1 + n_perm;
  pl.nit = (pl.N + kTI - 1) / kTI;
  // enough segments to fill the device at small N, never more than kMaxSeg rows in one
  const int64_t want = std::max<int64_t>(1, (1024 + pl.nit - 1) / pl.nit);
  pl.seg_len = std::min<int64_t>(kMaxSeg, std::max<int64_t>(kTJ, round_up((pl.N + want - 1) / want, kTJ)));
  pl.nseg = (int)((pl.N + pl.seg_len - 1) / pl.seg_len);
  pl.nsegm = (int)std::min<int64_t>(kMeanSegs, (pl.N + 31) / 32);
  pl.chunk_cols = (int)std::min<int64_t>(pl.P, kMaxChunkCols - 1);
  pl.NT = 1;
  while (pl.NT * 128 < pl.chunk_cols + 1) pl.NT *= 2;
  pl.cstride = pl.NT * 128;
  pl.nit_batch = std::max<int64_t>(1, std::min<int64_t>(pl.nit, (int64_t)(kPartBudget / 8) / ((int64_t)pl.nseg * pl.cstride)));
  pl.mean = w.take<float>(d, 256);
  pl.norms = w.take<float>(pl.Npad, 256);
  pl.colpart = w.take<double>((size_t)pl.nsegm * (size_t)d, 256);
  pl.su = w.take<double>(2, 256);
  pl.diag = w.take<double>(pl.P + 1, 256);
  pl.bits = w.take<uint32_t>((size_t)pl.P * (size_t)pl.row_words, 256);
  const size_t part = (size_t)pl.nit_batch * (size_t)pl.nseg * (size_t)pl.cstride;
  pl.part_t = w.take<float>(part, 256);
  pl.part_u = w.take<float>(part, 256);
#if SHIFT_MEMBER_TABLE
  pl.table = w.take<uint4>((size_t)pl.row_words * (size_t)pl.cstride * 4, 256);
#endif
  return true;
}

int perm_bits_args_ok(int64_t n, int64_t N, int64_t first_perm, int64_t n_rows, const void* bits, int64_t row_words) {
  if (N < 2 || N > runia_shift::kMaxRows || n < 1 || n >= N) return 0;
  if (first_perm < 0 || n_rows < 1 || first_perm + n_rows > (1ll << 31)) return 0;
  return bits && row_words >= (N + 31) / 32;
}

template <int NT>
void launch_fused(const FusedArgs& fa, dim3 grid, hipStream_t s) {
  RUNIA_LAUNCH_TIMED(shift_fused_kernel<NT>, grid, dim3(256), 0, s, fa);
}

}  // namespace

extern "C" size_t runia_shift_workspace_bytes(int64_t n, int64_t m, int64_t d, int64_t n_perm) {
  WsWalk w;
  Plan pl;
  return make_plan(w, n, m, d, n_perm, pl) ? w.used() : 0;
}

extern "C" int runia_shift_perm_bits(uint64_t seed, int64_t n, int64_t N, int64_t first_perm, int64_t n_rows, uint32_t* bits,
                                     int64_t row_words, runia_stream_t stream) {
  if (!perm_bits_args_ok(n, N, first_perm, n_rows, bits, row_words)) return RUNIA_E_INVALID;
  shift_perm_bits_kernel<<<(unsigned)n_rows, 256, 0, as_stream(stream)>>>(seed, (uint32_t)n, (uint32_t)N, (uint32_t)first_perm, bits,
                                                                         row_words);
  return runia_check_launch();
}

extern "C" int runia_shift_perm_bits_host(uint64_t seed, int64_t n, int64_t N, int64_t first_perm, int64_t n_rows, uint32_t* bits,
                                          int64_t row_words) {
  if (!perm_bits_args_ok(n, N, first_perm, n_rows, bits, row_words)) return RUNIA_E_INVALID;
  std::vector<uint32_t> hist(runia_shift::kBuckets);
  for (int64_t r = 0; r < n_rows; ++r) {
    const uint32_t p = (uint32_t)(first_perm + r);
    uint32_t* row = bits + r * row_words;
    uint64_t thr = 0;
    if (p != 0u) {
      uint64_t prefix = 0, mask = 0;
      uint32_t k = (uint32_t)n - 1u;
      for (int pass = 0; pass < runia_shift::kPasses; ++pass) {
        const int shift = runia_shift::pass_shift(pass), width = runia_shift::pass_width(pass);
        std::fill(hist.begin(), hist.end(), 0u);
        for (uint32_t i = 0; i < (uint32_t)N; ++i) {
          const uint64_t key = runia_shift::key(seed, p, i);
          if ((key & mask) == prefix) ++hist[(uint32_t)(key >> shift) & ((1u << width) - 1u)];
        }
        const int b = runia_shift::find_bucket(hist.data(), runia_shift::kBuckets, k);
        prefix |= (uint64_t)b << shift;
        mask |= ((1ull << width) - 1ull) << shift;
      }
      thr = prefix;
    }
    for (int64_t w = 0; w < row_words; ++w) {
      uint32_t v = 0u;
      for (int b = 0; b < 32; ++b) {
        const int64_t i = w * 32 + b;
        if (i < N) {
          const bool in = (p == 0u) ? (i < n) : (runia_shift::key(seed, p, (uint32_t)i) <= thr);
          v |= (in ? 1u : 0u) << b;
        }
      }
      row[w] = v;
    }
  }
  return RUNIA_OK;
}

extern "C" int64_t runia_shift_sample_rows(int64_t N) { return N < kSampleRows ? N : kSampleRows; }

extern "C" int runia_shift_pairwise_sample(const void* x, int64_t n, int64_t x_stride, const void* y, int64_t m, int64_t y_stride,
                                           int64_t d, int dtype, float* out, runia_stream_t stream) {
  if (n < 1 || m < 1 || d < 1 || n + m > runia_shift::kMaxRows || x_stride < d || y_stride < d) return RUNIA_E_INVALID;
  if (!elem_dtype_ok(dtype) || !x || !y || !out) return RUNIA_E_INVALID;
  const Rows r{x, y, n, n + m, d, x_stride, y_stride};
  const int64_t M = runia_shift_sample_rows(n + m);
  hipStream_t s = as_stream(stream);
  dispatch_elem(dtype, [&](auto tag) {
    typedef decltype(tag) T;
    shift_pairwise_kernel<T><<<(unsigned)(M - 1), 256, 0, s>>>(r, M, out);
    return 0;
  });
  return runia_check_launch();
}

extern "C" int runia_shift_mmd(const void* x, int64_t n, int64_t x_stride, const void* y, int64_t m, int64_t y_stride, int64_t d,
                               int dtype, int kind, const double* bandwidths, int n_bandwidths, int estimator, uint64_t seed,
                               int64_t n_perm, double* t, double* u, double* S, double* stats, int64_t* count, double* p_value,
                               void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  WsWalk w(workspace);
  Plan pl;
  if (!make_plan(w, n, m, d, n_perm, pl)) return RUNIA_E_INVALID;
  if (!elem_dtype_ok(dtype) || kind < kRbf || kind > kLinear || (estimator != kBiased && estimator != kUnbiased)) return RUNIA_E_INVALID;
  if (estimator == kUnbiased && (n < 2 || m < 2)) return RUNIA_E_INVALID;
  if (x_stride < d || y_stride < d) return RUNIA_E_INVALID;
  if (kind == kRbf) {
    if (!bandwidths || n_bandwidths < 1 || n_bandwidths > kMaxBandwidths) return RUNIA_E_INVALID;
    for (int b = 0; b < n_bandwidths; ++b)
      if (bandwidths[b] <= 0.0) return RUNIA_E_INVALID;  // (a NaN bandwidth passes: non-finite rows give NaN results)
  }
  if (!x || !y || !t || !u || !S || !stats || !count || !p_value) return RUNIA_E_INVALID;
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  float *mean = pl.mean, *norms = pl.norms, *part_t = pl.part_t, *part_u = pl.part_u;
  double *colpart = pl.colpart, *su = pl.su, *diag = pl.diag;
  uint32_t* bits = pl.bits;
  const Rows r{x, y, n, pl.N, d, x_stride, y_stride};

  shift_perm_bits_kernel<<<(unsigned)pl.P, 256, 0, s>>>(seed, (uint32_t)n, (uint32_t)pl.N, 0u, bits, pl.row_words);
  const int64_t rows_per = (pl.N + pl.nsegm - 1) / pl.nsegm;
  const unsigned dblocks = (unsigned)((d + 255) / 256);
  dispatch_elem(dtype, [&](auto tag) {
    typedef decltype(tag) T;
    shift_colsum_kernel<T><<<dim3(dblocks, (unsigned)pl.nsegm), 256, 0, s>>>(r, colpart, rows_per);
    shift_mean_kernel<<<dblocks, 256, 0, s>>>(colpart, pl.nsegm, pl.N, d, kind != kLinear, mean);
    shift_norms_kernel<T><<<runia_rows_grid(pl.Npad), 64 * kRowWaves, 0, s>>>(r, mean, pl.Npad, norms);
    return 0;
  });
  const bool want_diag = kind == kLinear && estimator == kUnbiased;
  if (want_diag) shift_diag_kernel<<<(unsigned)(pl.P + 1), 256, 0, s>>>(norms, bits, pl.row_words, pl.N, pl.P, diag);

  FusedArgs fa;
  fa.r = r; fa.mean = mean; fa.norms = norms; fa.bits = bits; fa.row_words = pl.row_words;
  fa.dtype = dtype; fa.kind = kind; fa.nbw = kind == kRbf ? n_bandwidths : 0;
  for (int b = 0; b < kMaxBandwidths; ++b) fa.g[b] = b < fa.nbw ? (float)(1.0 / (2.0 * bandwidths[b] * bandwidths[b])) : 0.f;
  fa.seg_len = pl.seg_len; fa.nseg = pl.nseg; fa.cstride = pl.cstride; fa.part_t = part_t; fa.part_u = part_u;
  fa.table = nullptr; fa.it0 = 0;
  for (int64_t p0 = 0; p0 < pl.P; p0 += pl.chunk_cols) {
    fa.p0 = p0;
    fa.ncols = (int)std::min<int64_t>(pl.chunk_cols, pl.P - p0);
#if SHIFT_MEMBER_TABLE
    fa.table = pl.table;
    shift_member_table_kernel<<<runia_stream_grid(pl.row_words * pl.cstride, 256), 256, 0, s>>>(
        fa, pl.table);
#endif
    for (int64_t it0 = 0; it0 < pl.nit; it0 += pl.nit_batch) {
      const int64_t nb = std::min<int64_t>(pl.nit_batch, pl.nit - it0);
      fa.it0 = it0;
      const dim3 grid((unsigned)nb, (unsigned)pl.nseg);
      switch (pl.NT) {
        case 1: launch_fused<1>(fa, grid, s); break;
        case 2: launch_fused<2>(fa, grid, s); break;
        case 4: launch_fused<4>(fa, grid, s); break;
        default: launch_fused<8>(fa, grid, s); break;
      }
      // (every chunk forms the same ones column: S is rewritten with the same bits)
      shift_reduce_kernel<<<(unsigned)((fa.ncols + 1 + 31) / 32), 256, 0, s>>>(part_t, part_u, nb * pl.nseg, pl.cstride, fa.ncols, p0,
                                                                             it0 > 0, t, u, su);
    }
  }
  shift_stats_kernel<<<1, 256, 0, s>>>(t, u, su, want_diag ? diag : nullptr, pl.P, n, m, kind, fa.nbw, estimator == kUnbiased, S, stats,
                                       reinterpret_cast<long long*>(count), p_value);
  return runia_check_launch();
}
