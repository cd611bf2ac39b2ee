// eigen_score of many sample groups in one launch (reference llm_uncertainty/scores.py:49-66, utils.py:102-117; Chen et
// al. 2024).  e holds groups * k rows of `hidden` values (f32 / f16 / bf16, unit column stride, any row stride): the
// last-token hidden states hidden_states[-1][layer] of generate(num_return_sequences=k) on a batch of prompts, prompt-major
// as HF's repeat_interleave leaves them, read in place.  Group g = rows g*k .. g*k+k-1:
//
//   out[g] = [ sum_{top min(k, hidden)} log(max(lambda_i, 0) + alpha) + (hidden - min(k, hidden)) log(alpha) ] / hidden,
//
// lambda = eigenvalues of the centred Gram matrix Ec Ec^T / (k - 1) - the non-zero spectrum of the reference's
// torch.cov(E.T) (the Gram form of llm_uncertainty/scores.py, which runs centred_gram_kernel and the Jacobi sweeps of
// eigh.hip with one host read-back per sweep).
//
// One workgroup of 256 threads per group, no atomics, no state shared between workgroups: a group's bits do not depend
// on the other groups of the launch.  LDS: 64 KB, two 4 096-double halves.
//   Gram     column chunks of C = 4096 / kpad columns (kpad = k rounded up to 4) are staged in half 0 as f64, centred by
//            their f64 column mean over the k rows (centred_gram_kernel's arithmetic: widen, mean in row order, product
//            in f64).  The k(k+1)/2 entries are covered by Q = kb(kb+1)/2 tiles of 4 x 4 entries (kb = kpad / 4, tile
//            rows <= tile columns): one tile per thread, 16 accumulators, 8 LDS reads per 16 products; R = 256 / Q
//            threads share a tile and take every R-th column.  The R partials are summed in slot order into G (half 1).
//   Jacobi   cyclic two-sided Jacobi on G in LDS without eigenvectors: jacobi_lds_sweeps of jacobi.hpp (ordering, the
//            eigenvalue form of the rotation threshold, block updates and stopping rule are described there); a group
//            still rotating after 30 sweeps gets NaN.
//   Score    diag(G) clamped at 0, ranked in descending order, the top min(k, hidden) summed in that order in f64.
#include <math.h>

#include "common.hpp"
#include "elem.hpp"
#include "jacobi.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = 64;
constexpr int kHalf = 4096;  // doubles per LDS half: kMaxK x kMaxK, and the staged chunk
constexpr int kMaxSweeps = 30;

template <class T>
__global__ __launch_bounds__(kThreads) void eigen_score_kernel(const void* __restrict__ e, int k, int64_t hidden,
                                                              int64_t row_stride, double alpha, double* __restrict__ out) {
  __shared__ double lds[2 * kHalf];
  double* stage = lds;         // Gram: staged chunk, then the slot partials; Jacobi: rotations, norm, flag, eigenvalues
  double* G = lds + kHalf;     // [k, k] row-major
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;
  const char* group = reinterpret_cast<const char*>(e) + g * k * row_stride * T::kBytes;
  const typename T::elem* rows = reinterpret_cast<const typename T::elem*>(group);

  // ---- Gram matrix ----------------------------------------------------------------------------------------------------
  const int kb = (k + 3) / 4, kpad = 4 * kb;
  const int Q = kb * (kb + 1) / 2;  // <= 136
  const int R = kThreads / Q;       // >= 1
  const int C = kHalf / kpad;       // columns per chunk
  const bool active = tid < Q * R;
  const int tile = tid % Q, slot = tid / Q;
  int ti = 0, rem = tile;
  while (rem >= kb - ti) { rem -= kb - ti; ++ti; }
  const int tj = ti + rem;  // tile rows 4 ti .. 4 ti + 3, columns 4 tj .. 4 tj + 3
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;

  for (int64_t h0 = 0; h0 < hidden; h0 += C) {
    const int w = (int)min((int64_t)C, hidden - h0);
    for (int idx = tid; idx < k * w; idx += kThreads) {
      const int r = idx / w, c = idx - r * w;
      stage[r * C + c] = (double)ld1<T>(rows + (int64_t)r * row_stride + h0 + c);
    }
    __syncthreads();
    // centre every column by its mean over the k rows; padding rows (k .. kpad-1) only feed entries that are dropped
    for (int c = tid; c < w; c += kThreads) {
      double mean = 0.0;
      for (int r = 0; r < k; ++r) mean += stage[r * C + c];
      mean /= (double)k;
      for (int r = 0; r < k; ++r) stage[r * C + c] -= mean;
      for (int r = k; r < kpad; ++r) stage[r * C + c] = 0.0;
    }
    __syncthreads();
    if (active) {
      const double* xa = stage + (4 * ti) * C;
      const double* xb = stage + (4 * tj) * C;
      for (int c = slot; c < w; c += R) {
        double va[4], vb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { va[a] = xa[a * C + c]; vb[a] = xb[a * C + c]; }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] += va[a] * vb[b];
      }
    }
    __syncthreads();
  }
  if (active) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) stage[(slot * Q + tile) * 16 + a * 4 + b] = acc[a][b];
  }
  __syncthreads();
  const double denom = (double)(k - 1);
  for (int idx = tid; idx < Q * 16; idx += kThreads) {
    const int t = idx >> 4, a = (idx >> 2) & 3, b = idx & 3;
    int I = 0, x = t;
    while (x >= kb - I) { x -= kb - I; ++I; }
    const int i = 4 * I + a, j = 4 * (I + x) + b;
    if (i > j || j >= k) continue;
    double s = 0.0;
    for (int sl = 0; sl < R; ++sl) s += stage[(sl * Q + t) * 16 + a * 4 + b];
    G[i * k + j] = s / denom;
    G[j * k + i] = s / denom;
  }
  __syncthreads();

  // ---- cyclic Jacobi on G ---------------------------------------------------------------------------------------------
  double* rot = stage;             // [64]: cosines, sines of the step's rotations
  double* part = stage + 64;       // [256]: Frobenius norm partials
  double* lam = stage + 320;       // [64]: eigenvalues in descending order
  int* flag = reinterpret_cast<int*>(stage + 384);
  int* nan_seen = flag + 1;
  const bool converged = jacobi_lds_sweeps<kThreads, false>(G, nullptr, k, kMaxSweeps, rot, part, flag);

  // ---- score ----------------------------------------------------------------------------------------------------------
  if (tid == 0) nan_seen[0] = 0;
  __syncthreads();
  if (tid < k) {
    double v = G[tid * k + tid];
    v = v < 0.0 ? 0.0 : v;  // NaN stays NaN
    if (isnan(v)) {
      nan_seen[0] = 1;
    } else {
      int rank = 0;
      for (int j = 0; j < k; ++j) {
        double u = G[j * k + j];
        u = u < 0.0 ? 0.0 : u;
        rank += (u > v || (u == v && j < tid)) ? 1 : 0;
      }
      lam[rank] = v;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double res = __builtin_nan("");
    if (converged && !nan_seen[0]) {
      const int64_t top = min((int64_t)k, hidden);
      double total = 0.0;
      for (int i = 0; i < (int)top; ++i) total += log(lam[i] + alpha);
      total += (double)(hidden - top) * log(alpha);
      res = total / (double)hidden;
    }
    out[g] = res;
  }
}

}  // namespace

extern "C" int runia_eigen_score_batch(const void* e, int dtype_code, int64_t groups, int64_t k, int64_t hidden,
                                       int64_t row_stride, double alpha, double* out, runia_stream_t stream) {
  if (!e || !out || groups <= 0 || groups > 0x7fffffffll || k < 2 || k > kMaxK || hidden <= 0 || row_stride < 0 ||
      !elem_dtype_ok(dtype_code))
    return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  dispatch_elem(dtype_code, [&](auto t) {
    eigen_score_kernel<decltype(t)><<<(unsigned)groups, kThreads, 0, s>>>(e, (int)k, hidden, row_stride, alpha, out);
  });
  return runia_check_launch();
}
