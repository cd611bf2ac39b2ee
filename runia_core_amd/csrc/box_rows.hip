// runia_ragged_rows: the per-image tensors of a detector's output dictionary ({image id: {"latent_space_means": (k_i, D),
// "features": ..., "logits": ...}}, reference feature_extraction/utils.py:160-191) stacked into ONE (total, D) table - the
// torch.cat of get_aggregated_data_dict, with its per-image torch.log(logits + 1e-10) folded in - by one launch whatever
// the number of images.
//
// Work item = 16 bytes of one output row (V = 4 f32 / 8 f16 / 8 bf16 values); a workgroup takes 256 consecutive items.
// Its first and last row are looked up in the prefix sum of the row counts by binary search (two lanes, through LDS);
// every lane then finds its own row's segment inside that short range - empty segments (images without detections) cost
// one more step of the search, never a workgroup.  A segment whose rows are contiguous in the columns, 16-byte aligned
// and a whole number of vectors apart moves as 16-byte loads and stores (every detector output in practice); any other
// segment (transposed or sliced views, an odd leading dimension), and the last partial vector of a row, moves element
// by element through the tensor's own strides.  Plain vector stores only.
#include "common.hpp"
#include "elem.hpp"

namespace {

// torch.log(x + 1e-10) on a tensor of T: the sum is formed in f32 and rounded to T, the logarithm is taken in f32 and
// rounded to T (an f16 zero stays zero: 1e-10 is below half of the smallest f16 denormal -> -inf, as torch gives)
template <class T>
__device__ __forceinline__ typename T::elem log_eps(typename T::elem x) {
  const float s = widen(T{}, narrow(T{}, widen(T{}, x) + 1e-10f));
  return narrow(T{}, logf(s));
}

struct Seg { int64_t ptr, rows, rs, cs; };  // one descriptor of the table

// last segment s in [lo, hi] with start[s] <= row (start is non-decreasing; equal neighbours = empty segments, skipped
// because the LAST such s is the one whose start[s + 1] > row)
__device__ __forceinline__ int64_t find_seg(const int64_t* __restrict__ start, int64_t lo, int64_t hi, int64_t row) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (start[mid] <= row) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <class T, int MODE>
__global__ __launch_bounds__(256) void ragged_rows_kernel(const int64_t* __restrict__ table,
                                                          const int64_t* __restrict__ start, int64_t n_seg, int64_t total,
                                                          int64_t D, uint32_t vpr, typename T::elem* __restrict__ out,
                                                          int64_t ld, int out_vec, int32_t* __restrict__ seg_of_row) {
  typedef typename T::elem E;
  constexpr int V = T::V;
  __shared__ int64_t range[2];
  const int64_t item0 = (int64_t)blockIdx.x * 256;
  const int64_t row0 = item0 / vpr;  // uniform
  const uint32_t in0 = (uint32_t)(item0 - row0 * vpr);
  int64_t row_last = row0 + (in0 + 255u) / vpr;
  if (row_last >= total) row_last = total - 1;
  if (threadIdx.x < 2) range[threadIdx.x] = find_seg(start, 0, n_seg - 1, threadIdx.x == 0 ? row0 : row_last);
  __syncthreads();
  const uint32_t local = in0 + threadIdx.x;
  const int64_t row = row0 + local / vpr;
  const uint32_t cv = local % vpr;
  if (row >= total) return;
  const int64_t s = find_seg(start, range[0], range[1], row);
  const int64_t* d = table + 4 * s;
  const int64_t base = d[0], rs = d[2], cs = d[3];
  const int64_t r = row - start[s], c0 = (int64_t)cv * V;
  if (seg_of_row && cv == 0) seg_of_row[row] = (int32_t)s;
  const E* src = reinterpret_cast<const E*>(base) + r * rs + c0 * cs;
  E* dst = out + row * ld + c0;
  const bool vec = out_vec && cs == 1 && (base & 15) == 0 && (rs % V) == 0 && c0 + V <= D;
  if (vec) {
    uint4 w = *reinterpret_cast<const uint4*>(src);
    if constexpr (MODE == 1) {
      E e[V];
      __builtin_memcpy(e, &w, 16);
#pragma unroll
      for (int j = 0; j < V; ++j) e[j] = log_eps<T>(e[j]);
      __builtin_memcpy(&w, e, 16);
    }
    *reinterpret_cast<uint4*>(dst) = w;
  } else {
    const int n = D - c0 < V ? (int)(D - c0) : V;
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (j < n) {
        const E x = src[j * cs];
        dst[j] = MODE == 1 ? log_eps<T>(x) : x;
      }
  }
}

template <class T>
int launch(const int64_t* table, const int64_t* start, int64_t n_seg, int64_t total, int64_t D, int mode, void* out,
           int64_t ld, int32_t* seg_of_row, hipStream_t s) {
  typedef typename T::elem E;
  constexpr int V = T::V;
  const int64_t vpr = (D + V - 1) / V;
  if (vpr > 0x7fffffffll - 256) return RUNIA_E_INVALID;
  const int64_t blocks = (total * vpr + 255) / 256;
  if (blocks > 0x7fffffffll) return RUNIA_E_INVALID;
  const int out_vec = reinterpret_cast<uintptr_t>(out) % 16 == 0 && ld % V == 0;
  if (mode == 0)
    ragged_rows_kernel<T, 0><<<(unsigned)blocks, 256, 0, s>>>(table, start, n_seg, total, D, (uint32_t)vpr,
                                                              static_cast<E*>(out), ld, out_vec, seg_of_row);
  else
    ragged_rows_kernel<T, 1><<<(unsigned)blocks, 256, 0, s>>>(table, start, n_seg, total, D, (uint32_t)vpr,
                                                              static_cast<E*>(out), ld, out_vec, seg_of_row);
  return runia_check_launch();
}

}  // namespace

extern "C" int runia_ragged_rows(const int64_t* table, const int64_t* row_start, int64_t n_seg, int64_t total, int64_t D,
                                 int dtype, int mode, void* out, int64_t ld, int32_t* seg_of_row, runia_stream_t stream) {
  if (n_seg < 0 || total < 0 || D <= 0 || !elem_dtype_ok(dtype) ||
      (mode != RUNIA_RAGGED_COPY && mode != RUNIA_RAGGED_LOG_EPS) || ld < D || n_seg > 0x7fffffffll)
    return RUNIA_E_INVALID;
  if (total == 0 || n_seg == 0) return RUNIA_OK;
  if (!table || !row_start || !out) return RUNIA_E_INVALID;
  return dispatch_elem(dtype, [&](auto t) {
    return launch<decltype(t)>(table, row_start, n_seg, total, D, mode, out, ld, seg_of_row, as_stream(stream));
  });
}
