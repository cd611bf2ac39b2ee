// Per-feature two-sample Kolmogorov-Smirnov statistics under the observed split and n_perm permutations (evaluation/
// shift_univariate.py): the (1 + n_perm) x D integer table that the max-T adjustment is built from.
// Two row tables X [n, D], Y [m, D], pooled Z = [X; Y], N = n + m <= kMaxRows.  For column d and permutation p the pooled values are
// walked in ascending order, v += m for a member of the first set of p and v -= n otherwise, and T[p, d] = max |v| over the last
// positions of the runs of equal values: an exact integer <= n m (the KS statistic is T / (n m)).
//   * ks_sort_kernel: one workgroup per column of the pass.  The column is read where it lies, turned into monotone u32 keys (-0
//     folded into +0, NaN flagged), and (key, row) pairs are sorted in LDS (order.hpp).  It writes, per sorted position,
//     the row index with the run-end flag in bit 31, and the column's valid flag.
//   * ks_transpose_kernel: the membership bits of shift.hip (row p, bit i) once per call as [N, words of 32 permutations], rows
//     padded to whole groups of 8 words, so that the permutations of one sorted position are consecutive words.
//   * ks_walk_kernel: grid = 256-permutation groups x columns; a lane owns one permutation.  Per 256 sorted positions a thread
//     gathers the 8 membership words of ITS position (32 bytes of one row of the transposed table) and leaves them in LDS; the
//     gather of the next tile and the order of the one after are in flight while the waves walk this one.  Per position and wave:
//     one broadcast LDS read of (word, run-end mask), bit extract, v = bit * N + v, |v - (k + 1) n| in one v_sad_u32, the mask
//     (all ones at a run end, 0 elsewhere) and the maximum: no branch and no select in the loop.
// Everything is integer: the same bits from call to call, whatever the order of the launches.
#include "common.hpp"
#include "elem.hpp"

#include <algorithm>

namespace {

constexpr int64_t kMaxRows = 16384;            // pooled rows: 16384 (key, row) pairs of 8 bytes are 128 KiB of LDS; n m <= 2^26
constexpr int64_t kMaxCols = 4096;             // columns of one pass, at most
constexpr int64_t kMaxPerm = (1ll << 20) - 1;  // permutations of one call: 2^15 membership words per row (a grid's y extent is 65535)
constexpr size_t kOrderBudget = (size_t)64 << 20;  // bytes of row orders kept at once
constexpr int kTile = 256;                     // sorted positions staged per step of the walk (= threads of its workgroup)
constexpr int kBlockWords = 8;                 // membership words (32 permutations each) of a walk workgroup
constexpr uint32_t kEndBit = 0x80000000u;

struct Cols {
  const void* x;
  const void* y;
  int64_t n, N, sx, sy;  // row strides in elements
};

template <class T>
__device__ __forceinline__ float col_value(const Cols& c, int64_t i, int64_t d) {
  typedef const typename T::elem* P;
  return ld1<T>(i < c.n ? reinterpret_cast<P>(c.x) + i * c.sx + d : reinterpret_cast<P>(c.y) + (i - c.n) * c.sy + d);
}

// ---- order ----------------------------------------------------------------------------------------------------------------------
// s: np2 (a power of two >= N) pairs key << 32 | row; the padding pairs are all ones and sort behind every row
template <class T>
__global__ __launch_bounds__(1024) void ks_sort_kernel(Cols c, int64_t d0, int np2, uint32_t* __restrict__ order, int64_t ord_stride,
                                                       int32_t* __restrict__ valid) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s[];
  __shared__ int s_nan;
  const int tid = threadIdx.x, nt = blockDim.x, N = (int)c.N;
  const int64_t d = d0 + blockIdx.x;
  if (tid == 0) s_nan = 0;
  __syncthreads();
  bool nan = false;
  for (int i = tid; i < np2; i += nt) {
    unsigned long long e = ~0ull;
    if (i < N) {
      const float v = col_value<T>(c, i, d);
      nan |= v != v;
      // ascending as numbers, -0 == +0; +-inf are ordinary extremes
      e = ((unsigned long long)asc_key(fold_zero(v)) << 32) | (unsigned long long)i;
    }
    s[i] = e;
  }
  if (nan) s_nan = 1;  // (every writer stores the same value)
  __syncthreads();
  lds_bitonic_sort(s, np2, tid, nt);
  uint32_t* out = order + (int64_t)blockIdx.x * ord_stride;
  for (int k = tid; k < N; k += nt) {
    const unsigned long long e = s[k];
    const bool end = k == N - 1 || (uint32_t)(s[k + 1] >> 32) != (uint32_t)(e >> 32);
    out[k] = (uint32_t)e | (end ? kEndBit : 0u);
  }
  if (tid == 0) valid[d] = s_nan ? 0 : 1;
}

// ---- memberships, one row per pooled row ------------------------------------------------------------------------------------------
// memT[i * pw + w] bit b = membership of row i in permutation 32 w + b (0 past P); bits: row p, bit i (runia_shift_perm_bits)
__global__ __launch_bounds__(256) void ks_transpose_kernel(const uint32_t* __restrict__ bits, int64_t row_words, int64_t N, int64_t P,
                                                           int64_t pw, uint32_t* __restrict__ memT) {
  // grid = (ceil(N / 256), pw): exactly one thread per (row i, word w), i fastest, so a wave reads two words of `bits` per b.
  // pw <= 2^15 (kMaxPerm) fits the grid's y extent; no cap on the workgroups, hence no grid-stride loop.
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (i >= N) return;
  uint32_t v = 0u;
  for (int b = 0; b < 32; ++b) {
    const int64_t p = w * 32 + b;
    if (p < P) v |= ((bits[p * row_words + (i >> 5)] >> (i & 31)) & 1u) << b;
  }
  memT[i * pw + w] = v;
}

// ---- walk -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTile) void ks_walk_kernel(const uint32_t* __restrict__ order, int64_t ord_stride,
                                                        const uint32_t* __restrict__ memT, int64_t pw,
                                                        const int32_t* __restrict__ valid, int N, int n, int64_t P, int64_t D,
                                                        int64_t d0, long long* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) uint2 s_mem[kTile][kBlockWords];  // (membership word, run-end mask) per position
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t d = d0 + blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kTile + tid;
  if (!valid[d]) {  // (uniform over the workgroup)
    if (p < P) table[p * D + d] = -1;
    return;
  }
  const uint32_t* ord = order + (int64_t)blockIdx.y * ord_stride;
  const uint32_t* mrow = memT + (int64_t)blockIdx.x * kBlockWords;
  auto load_order = [&](int k) { return k < N ? ord[k] : 0u; };
  auto gather = [&](int k, uint32_t o, uint4& a, uint4& b) {
    a = b = make_uint4(0u, 0u, 0u, 0u);  // a position past N moves nothing and ends no run
    if (k < N) {
      const uint4* q = reinterpret_cast<const uint4*>(mrow + (int64_t)(o & ~kEndBit) * pw);
      a = q[0];
      b = q[1];
    }
  };
  uint32_t o_cur = load_order(tid), o_next = load_order(kTile + tid);
  uint4 a, b;
  gather(tid, o_cur, a, b);
  const int sh = lane & 31, wsel = 2 * wave + (lane >> 5);
  const bool live = (int64_t)blockIdx.x * kTile + wave * 64 < P;  // (uniform over the wave)
  uint32_t v = 0u, best = 0u;  // v = N * (members among the positions so far): <= n N < 2^31
  for (int k0 = 0; k0 < N; k0 += kTile) {
    __syncthreads();  // the previous tile has been walked
    {
      const uint32_t e = (o_cur >> 31) ? 0xffffffffu : 0u;
      uint4* dst = reinterpret_cast<uint4*>(&s_mem[tid][0]);
      dst[0] = make_uint4(a.x, e, a.y, e);
      dst[1] = make_uint4(a.z, e, a.w, e);
      dst[2] = make_uint4(b.x, e, b.y, e);
      dst[3] = make_uint4(b.z, e, b.w, e);
    }
    __syncthreads();
    // the next tile's words and the order of the tile after it fly while this one is walked
    o_cur = o_next;
    gather(k0 + kTile + tid, o_cur, a, b);
    o_next = load_order(k0 + 2 * kTile + tid);
    if (live) {
      uint32_t kn = (uint32_t)(k0 * n);  // (k + 1) n below: <= N n
#pragma unroll 8
      for (int j = 0; j < kTile; ++j) {
        kn += (uint32_t)n;
        const uint2 we = s_mem[j][wsel];
        v += __umul24(__builtin_amdgcn_ubfe(we.x, sh, 1), (uint32_t)N);
        uint32_t dv;  // |m * members - n * others| in one instruction (the compiler forms min, max and a subtraction)
        asm("v_sad_u32 %0, %1, %2, 0" : "=v"(dv) : "v"(v), "s"(kn));
        best = max(best, dv & we.y);                          // counts at a run end only
      }
    }
  }
  if (p < P) table[p * D + d] = (long long)best;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct Plan {
  int64_t N, P, row_words, pw, ord_stride, cols;
  int np2, threads;
  uint32_t *bits, *memT, *order;  // the regions of the workspace (256-byte slots)
};

bool shape_ok(int64_t n, int64_t m, int64_t n_perm) {
  return n >= 1 && m >= 1 && n + m <= kMaxRows && n_perm >= 0 && n_perm <= kMaxPerm;
}

int64_t columns_per_pass(int64_t n, int64_t m) {
  const int64_t per_col = round_up(n + m, 64) * 4;
  return std::max<int64_t>(1, std::min<int64_t>(kMaxCols, (int64_t)kOrderBudget / per_col));
}

bool make_plan(WsWalk& w, int64_t n, int64_t m, int64_t d, int64_t n_perm, Plan& pl) {
  if (!shape_ok(n, m, n_perm) || d < 1 || d >= (1ll << 31)) return false;
  pl.N = n + m;
  pl.P = 1 + n_perm;
  pl.row_words = (pl.N + 31) / 32;
  pl.pw = round_up((pl.P + 31) / 32, kBlockWords);
  pl.ord_stride = round_up(pl.N, 64);
  pl.cols = std::min<int64_t>(d, columns_per_pass(n, m));
  pl.np2 = 2;
  while (pl.np2 < pl.N) pl.np2 *= 2;
  pl.threads = pl.np2 >= 2048 ? 1024 : 256;
  pl.bits = w.take<uint32_t>((size_t)pl.P * (size_t)pl.row_words, 256);
  pl.memT = w.take<uint32_t>((size_t)pl.N * (size_t)pl.pw, 256);
  pl.order = w.take<uint32_t>((size_t)pl.cols * (size_t)pl.ord_stride, 256);
  return true;
}

template <class T>
int launch_sort(const Cols& c, int64_t d0, int64_t cols, const Plan& pl, uint32_t* order, int32_t* valid, hipStream_t s) {
  static std::atomic<uint64_t> lds_ok{0};
  if (int rc = runia_allow_dynamic_lds(reinterpret_cast<const void*>(ks_sort_kernel<T>), (int)(kMaxRows * 8), lds_ok)) return rc;
  ks_sort_kernel<T><<<(unsigned)cols, pl.threads, (size_t)pl.np2 * 8, s>>>(c, d0, pl.np2, order, pl.ord_stride, valid);
  return RUNIA_OK;
}

}  // namespace

extern "C" int64_t runia_ks_max_rows(void) { return kMaxRows; }

extern "C" int64_t runia_ks_columns_per_pass(int64_t n, int64_t m, int64_t n_perm) {
  return shape_ok(n, m, n_perm) ? columns_per_pass(n, m) : 0;
}

extern "C" size_t runia_ks_workspace_bytes(int64_t n, int64_t m, int64_t d, int64_t n_perm) {
  WsWalk w;
  Plan pl;
  return make_plan(w, n, m, d, n_perm, pl) ? w.used() : 0;
}

extern "C" int runia_ks_perm_table(const void* x, int64_t n, int64_t x_stride, const void* y, int64_t m, int64_t y_stride, int64_t d,
                                   int dtype, uint64_t seed, int64_t n_perm, int64_t* table, int32_t* valid, void* workspace,
                                   size_t workspace_bytes, runia_stream_t stream) {
  WsWalk w(workspace);
  Plan pl;
  if (!make_plan(w, n, m, d, n_perm, pl)) return RUNIA_E_INVALID;
  if (!elem_dtype_ok(dtype) || x_stride < d || y_stride < d) return RUNIA_E_INVALID;
  if (!x || !y || !table || !valid) return RUNIA_E_INVALID;
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  uint32_t *bits = pl.bits, *memT = pl.memT, *order = pl.order;
  const Cols c{x, y, n, pl.N, x_stride, y_stride};

  if (int rc = runia_shift_perm_bits(seed, n, pl.N, 0, pl.P, bits, pl.row_words, stream)) return rc;
  ks_transpose_kernel<<<dim3((unsigned)((pl.N + 255) / 256), (unsigned)pl.pw), 256, 0, s>>>(bits, pl.row_words, pl.N, pl.P, pl.pw, memT);
  const unsigned pgroups = (unsigned)((pl.P + kTile - 1) / kTile);
  for (int64_t d0 = 0; d0 < d; d0 += pl.cols) {
    const int64_t cols = std::min<int64_t>(pl.cols, d - d0);
    if (int rc = dispatch_elem(dtype, [&](auto tag) { return launch_sort<decltype(tag)>(c, d0, cols, pl, order, valid, s); })) return rc;
    RUNIA_LAUNCH_TIMED(ks_walk_kernel, dim3(pgroups, (unsigned)cols), dim3(kTile), 0, s, order, pl.ord_stride, memT, pl.pw, valid,
                       (int)pl.N, (int)n, pl.P, d, d0, reinterpret_cast<long long*>(table));
  }
  return runia_check_launch();
}
