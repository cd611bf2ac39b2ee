// Setup-time helper of the folded LaREM score (proj_sq.hip, K2'): the score -|| M h + c ||^2 does not change under an orthogonal
// Q applied from the left, so M [r, D] (r <= D) is replaced once per fitted state by the upper-trapezoidal R = Q M
// (R[j][k] = 0 for k < j) and c by Q c; K2' then skips the k range in which a column tile of R^T holds only zeros.
// Householder reflections on the augmented [M | c] - not the Cholesky factor of M^T M, which squares the condition number
// of the leading block.  ONE workgroup walks the columns (the matrix is 1 MB and stays in L2; a few milliseconds, once):
// every sum below is added up in an order this code fixes - no atomics, nothing that follows the grid - because every rank
// of a sharded job has to fold the same fitted arrays into the same bits.
#include "common.hpp"
#include "trap_order.hpp"

namespace {

constexpr int kQrThreads = 1024, kQrLanes = 512, kQrSlices = kQrThreads / kQrLanes;
constexpr int64_t kQrMaxRows = 4096;  // the reflection vector lives in LDS

// a [r][D] row-major and q [r] hold [M | c] on entry, [R | Q c] on return.  Column k of the augmented matrix is a + k
// (stride D) for k < D and q (stride 1) for k == D.
__global__ __launch_bounds__(kQrThreads) void qr_trapezoid_kernel(const double* __restrict__ m, const double* __restrict__ c,
                                                                   double* __restrict__ a, double* __restrict__ q, int64_t r,
                                                                   int64_t D) {
  __shared__ double v[kQrMaxRows];
  __shared__ double ps[kQrSlices][kQrLanes];
  __shared__ double scal[2];  // alpha (the new diagonal element), denom (v^T v / 2; 0 = no reflection)
  const int tid = threadIdx.x, lane = tid & 63;
  const int cl = tid % kQrLanes, sl = tid / kQrLanes;
  if (a != m)
    for (int64_t e = tid; e < r * D; e += kQrThreads) a[e] = m[e];
  if (q != c)
    for (int64_t e = tid; e < r; e += kQrThreads) q[e] = c[e];
  __syncthreads();
  for (int64_t j = 0; j + 1 < r; ++j) {
    const int64_t rows = r - j;
    for (int64_t i = tid; i < rows; i += kQrThreads) v[i] = a[(j + i) * D + j];
    __syncthreads();
    if (tid < 64) {
      // sum of squares below the diagonal: lane l adds rows l + 1, l + 65, ... in that order, then a fixed butterfly
      double s = 0.0;
      for (int64_t i = 1 + lane; i < rows; i += 64) s = fma(v[i], v[i], s);
      s += shfl_xor_f64(s, 1);
      s += shfl_xor_f64(s, 2);
      s += shfl_xor_f64(s, 4);
      s += shfl_xor_f64(s, 8);
      s += shfl_xor_f64(s, 16);
      s += shfl_xor_f64(s, 32);
      if (lane == 0) {
        const double x0 = v[0];
        if (s == 0.0) {  // nothing to annihilate (also a column that is zero from here down): no reflection, no division
          scal[0] = x0;
          scal[1] = 0.0;
        } else {
          const double norm = sqrt(fma(x0, x0, s));
          const double alpha = (x0 > 0.0) ? -norm : norm;  // v0 = x0 - alpha adds magnitudes: no cancellation
          v[0] = x0 - alpha;
          scal[0] = alpha;
          scal[1] = norm * (norm + fabs(x0));  // = v^T v / 2, so H = I - v v^T / denom
        }
      }
    }
    __syncthreads();
    const double alpha = scal[0], denom = scal[1];
    if (denom != 0.0) {
      // columns j + 1 .. D in blocks of kQrLanes; a column's dot product with v is two row-slice chains (rows ascending)
      // added as slice 0 + slice 1
      const int64_t half = (rows + 1) / 2;
      const int64_t i0 = sl * half, i1 = (i0 + half < rows) ? i0 + half : rows;
      for (int64_t kb = j + 1; kb <= D; kb += kQrLanes) {
        const int64_t k = kb + cl;
        const bool live = k <= D;
        double* col = (k < D) ? a + j * D + k : q + j;
        const int64_t stride = (k < D) ? D : 1;
        double s = 0.0;
        if (live) {
#pragma unroll 8
          for (int64_t i = i0; i < i1; ++i) s = fma(v[i], col[i * stride], s);
        }
        ps[sl][cl] = s;
        __syncthreads();
        if (live) {
          const double w = (ps[0][cl] + ps[1][cl]) / denom;
#pragma unroll 8
          for (int64_t i = i0; i < i1; ++i) col[i * stride] = fma(-v[i], w, col[i * stride]);
        }
        __syncthreads();
      }
    }
    // column j itself: the diagonal element and exact zeros below it (written, not left as rounding residue; without a
    // reflection they were zeros or squares that underflowed)
    for (int64_t i = tid; i < rows; i += kQrThreads) a[(j + i) * D + j] = (i == 0) ? alpha : 0.0;
    __syncthreads();
  }
}

// Row gather into the balanced block order (trap_order.hpp): output row i, in 32-column group i / 32 of pack(out^T),
// is the row of `a` with the same offset in the R block that group holds; c goes with its rows.  One workgroup per row.
__global__ __launch_bounds__(256) void trap_balance_rows_kernel(const double* __restrict__ a, const double* __restrict__ q,
                                                                 double* __restrict__ a_out, double* __restrict__ q_out,
                                                                 int64_t r, int64_t D) {
  const int64_t i = blockIdx.x;
  const int64_t src = trap_balanced_block(i / 32, r) * 32 + i % 32;
  for (int64_t k = threadIdx.x; k < D; k += 256) a_out[i * D + k] = a[src * D + k];
  if (threadIdx.x == 0) q_out[i] = q[src];
}

}  // namespace

extern "C" int runia_qr_trapezoid_f64(const double* m, const double* c, double* r_out, double* c_out, int64_t r, int64_t D,
                                      runia_stream_t stream) {
  if (r <= 0 || D <= 0 || r > D || r > kQrMaxRows) return RUNIA_E_INVALID;
  if (!m || !c || !r_out || !c_out) return RUNIA_E_INVALID;
  qr_trapezoid_kernel<<<1, kQrThreads, 0, as_stream(stream)>>>(m, c, r_out, c_out, r, D);
  return runia_check_launch();
}

extern "C" int runia_trap_balance_order(int64_t* src_rows, int64_t r) {
  if (r <= 0 || !src_rows) return RUNIA_E_INVALID;
  for (int64_t i = 0; i < r; ++i) src_rows[i] = trap_balanced_block(i / 32, r) * 32 + i % 32;
  return RUNIA_OK;
}

extern "C" int runia_trap_balance_rows_f64(const double* r_in, const double* c_in, double* r_out, double* c_out, int64_t r,
                                           int64_t D, runia_stream_t stream) {
  if (r <= 0 || D <= 0 || r > D || r > 0x7fffffff) return RUNIA_E_INVALID;
  if (!r_in || !c_in || !r_out || !c_out || r_in == r_out || c_in == c_out) return RUNIA_E_INVALID;
  trap_balance_rows_kernel<<<(unsigned)r, 256, 0, as_stream(stream)>>>(r_in, c_in, r_out, c_out, r, D);
  return runia_check_launch();
}
