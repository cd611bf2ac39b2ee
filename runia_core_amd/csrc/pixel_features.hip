// Per-pixel Mahalanobis maps from the feature maps of a segmentation decoder, read where the model left them, and the
// pieces that fit the Gaussians from labelled maps without a (pixels x C) table.
//   runia_pixfeat_score        ONE launch over G maps of (C, h, w) features in f32 / f16 / bf16 (NCHW, channels_last or any
//                              strided view): distance = min_c |W (x - m0) - mz_c|^2, its argmin and all K distances.
//   runia_pixfeat_label_hist   pixels per class of (G, h, w) label maps.
//   runia_pixfeat_gather_rows  deterministic subsample of the labelled pixels into an (n, C) f32 row table, in pixel order.
//
// Score.  z = W (x - m0) is a product of the lower-triangular [C, C] whitening matrix with a [C, pixels] operand that NCHW
// already stores channel-major with the pixels contiguous: the transposed form of what nt_tile_f32.hpp stages.  A 256-thread
// workgroup owns 128 consecutive pixels of the flattened G * h * w axis (a tile may straddle two images: every pixel carries
// its own address).  32 channels at a time are widened, centred (x - m0) and put into LDS as Xs[channel][pixel] (pitch 132:
// rows stay 16-byte aligned; a ds_read_b32 of 32 consecutive pixels per lane half has no bank conflict whatever the pitch);
// W is staged K-contiguous as Ws[j][34] exactly as nt_tile_f32.hpp stages its operands (one ds_read_b64 feeds two k-steps,
// same k permutation on both operands: step 2s takes k = 4s + 2 (lane >> 5), step 2s + 1 the one after).  On
// v_mfma_f32_32x32x2_f32 W is the A operand (rows j) and X the B operand (columns = pixels), so that in the accumulators
// a lane holds ONE pixel (lane & 31) and 16 of the 32 rows j of a tile: wave v owns pixels 32 v .. 32 v + 31 and all 128
// columns j of the block (4 accumulator tiles, 64 registers).  The epilogue d_c += sum_j (z_j - mz_cj)^2 therefore runs
// inside a lane over its 64 values, with mz of the block in LDS read as broadcast 16-byte rows; the two halves of the wave
// (rows j + 4 (lane >> 5)) are added once, at the very end.  z never leaves the registers.  The difference form is the
// point: with feature means away from zero |z|^2 - 2 z.mz + |mz|^2 cancels to nothing in f32.
// The chunk is read in one of three ways, picked per launch from the strides: four neighbouring pixels of a channel plane
// per load (NCHW), 16 neighbouring channels of a pixel per thread (channels_last; transposed on its way into Xs), or
// element by element through the strides (crops, odd bases).  All three fill the same Xs: the results are the same bits.
// (The view and the staging are in pixel_map.hpp, shared with pixel_knn.hip.)
// W is lower triangular: column block jb needs the channel chunks up to its own last row only (trapezoid form, as K2').
// The running sums of up to 32 classes live in registers; K > 32 repeats the product per group of 32 classes (the kernel
// is laid out for K <= 32: Cityscapes 19, VOC 21).  Every sum runs in one lane in a fixed order, no atomics: results are
// run-to-run bit identical and do not depend on where in the batch a pixel sits.
//
// A distance that is not finite (NaN or inf features) is written as NaN, for that pixel alone (a pixel is a column of the
// B operand: nothing of it reaches another column).  A class whose mz row starts with +inf is excluded: it scores +inf.
#include <cfloat>

#include "common.hpp"
#include "elem.hpp"
#include "philox.hpp"
#include "pixel_map.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTJ = 128;    // columns of z per block
constexpr int kKG = 32;     // classes whose running sums a lane keeps in registers
constexpr int kMaxK = 256;
constexpr int kChunkPix = 1024;  // pixels per chunk of the gather

struct ScoreArgs {
  MapView v;
  int K, vecw;
  const float *m0, *W, *mz;
  float* dist;
  int* nearest;
  float* cd;
};

// ---- the score kernel -----------------------------------------------------------------------------------------------------------
template <class T, int LOAD>
__global__ __launch_bounds__(256) void pixfeat_score_kernel(ScoreArgs a) {
  constexpr bool VEC = LOAD == kLoadVec;
  __shared__ __attribute__((aligned(16))) float Xs[kKCh][kXP];
  __shared__ __attribute__((aligned(16))) float Ws[kTJ][kWP];
  __shared__ __attribute__((aligned(16))) float Ms[kKG][kXP];
  __shared__ float m0s[kMaxC];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int C = a.v.C, K = a.K;
  const int64_t p0 = (int64_t)blockIdx.x * kTP;

  for (int c = tid; c < kMaxC; c += 256) m0s[c] = c < C ? a.m0[c] : 0.f;

  // the four pixels (channels_last: the one pixel) this thread stages
  int64_t off[4];
  const int nv = staged_pixels<LOAD>(a.v, p0, tid, off);
  // the pixel whose sums this lane holds
  const int64_t pm = p0 + wave * 32 + li;
  const bool mine = pm < a.v.P;
  const int64_t gm = mine ? pm / a.v.HW : 0, qm = mine ? pm - gm * a.v.HW : 0;

  float best = INFINITY;
  int bi = 0;
  bool bad = false;

  for (int kg0 = 0; kg0 < K; kg0 += kKG) {
    const int kg = K - kg0 < kKG ? K - kg0 : kKG;
    float dreg[kKG];
#pragma unroll
    for (int c = 0; c < kKG; ++c) dreg[c] = 0.f;

    for (int j0 = 0; j0 < C; j0 += kTJ) {
      __syncthreads();  // the epilogue of the block before is through with Ms
      for (int idx = tid; idx < kg * kTJ; idx += 256) {
        const int c = idx >> 7, j = idx & (kTJ - 1);
        Ms[c][j] = j0 + j < C ? a.mz[(int64_t)(kg0 + c) * C + j0 + j] : 0.f;
      }
      f32x16 acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      const int kend = j0 + kTJ < C ? j0 + kTJ : C;  // W[j, c] = 0 for c > j: the chunks past the block's last row are skipped
      float xr[16], wr[16];
      if constexpr (LOAD == kLoadCLast) load_x_cl<T>(a.v, off[0], nv > 0, 0, tid, xr);
      else load_x<T, VEC>(a.v, off, nv, 0, tid, xr);
      load_w(a.W, C, C, j0, 0, tid, a.vecw != 0, wr);
      for (int k0 = 0; k0 < kend; k0 += kKCh) {
        __syncthreads();  // every wave has finished reading the previous chunk
        if constexpr (LOAD == kLoadCLast) store_x_cl(xr, Xs, m0s, k0, tid);
        else store_x(xr, Xs, m0s, k0, tid);
        store_w(wr, Ws, tid);
        __syncthreads();
        if (k0 + kKCh < kend) {  // next chunk's loads fly while the matrix cores consume this one
          if constexpr (LOAD == kLoadCLast) load_x_cl<T>(a.v, off[0], nv > 0, k0 + kKCh, tid, xr);
          else load_x<T, VEC>(a.v, off, nv, k0 + kKCh, tid, xr);
          load_w(a.W, C, C, j0, k0 + kKCh, tid, a.vecw != 0, wr);
        }
#pragma unroll
        for (int s = 0; s < kKCh / 4; ++s) {
          const float bx = Xs[4 * s + 2 * lh][wave * 32 + li], by = Xs[4 * s + 2 * lh + 1][wave * 32 + li];
          float2 av[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) av[t] = *reinterpret_cast<const float2*>(&Ws[t * 32 + li][4 * s + 2 * lh]);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].x, bx, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].y, by, acc[t], 0, 0, 0);
          }
        }
      }
      // acc[t][r] = z[j0 + 32 t + (r & 3) + 8 (r >> 2) + 4 lh] of pixel li
#pragma unroll
      for (int c = 0; c < kKG; ++c) {
        if (c < kg) {
          float s = dreg[c];
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
              const float4 m = *reinterpret_cast<const float4*>(&Ms[c][t * 32 + 8 * rq + 4 * lh]);
              const float d0 = acc[t][4 * rq] - m.x, d1 = acc[t][4 * rq + 1] - m.y;
              const float d2 = acc[t][4 * rq + 2] - m.z, d3 = acc[t][4 * rq + 3] - m.w;
              s = fmaf(d0, d0, s);
              s = fmaf(d1, d1, s);
              s = fmaf(d2, d2, s);
              s = fmaf(d3, d3, s);
            }
          dreg[c] = s;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kKG; ++c) {
      if (c < kg) {
        const int cls = kg0 + c;
        float d = dreg[c] + __shfl_xor(dreg[c], 32, 64);
        const bool excluded = a.mz[(int64_t)cls * C] == INFINITY;
        d = excluded ? INFINITY : (d < INFINITY ? d : __builtin_nanf(""));
        bad = bad || d != d;
        if (d < best) {
          best = d;
          bi = cls;
        }
        if (a.cd && mine && lh == 0) a.cd[(gm * K + cls) * a.v.HW + qm] = d;
      }
    }
  }
  if (mine && lh == 0) {
    if (a.dist) a.dist[pm] = bad ? __builtin_nanf("") : best;
    if (a.nearest) a.nearest[pm] = bad ? 0 : bi;
  }
}

// ---- labels ---------------------------------------------------------------------------------------------------------------------
enum { kLabI64 = 0, kLabI32 = 1, kLabU8 = 2 };

__device__ __forceinline__ int64_t load_label(const void* lab, int code, int64_t p) {
  if (code == kLabI64) return static_cast<const int64_t*>(lab)[p];
  if (code == kLabI32) return static_cast<const int32_t*>(lab)[p];
  return static_cast<const uint8_t*>(lab)[p];
}

// counts of whole numbers: the order of the additions does not show in the result
__global__ __launch_bounds__(256) void pixfeat_hist_kernel(const void* __restrict__ lab, int code, int64_t N, int K,
                                                           int64_t ignore, unsigned long long* __restrict__ counts,
                                                           unsigned long long* __restrict__ dropped) {
  __shared__ unsigned h[kMaxK + 1];
  for (int c = threadIdx.x; c <= kMaxK; c += 256) h[c] = 0u;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (int64_t)gridDim.x * 256) {
    const int64_t l = load_label(lab, code, p);
    atomicAdd(&h[(l != ignore && l >= 0 && l < K) ? (int)l : kMaxK], 1u);
  }
  __syncthreads();
  for (int c = threadIdx.x; c <= kMaxK; c += 256)
    if (h[c]) atomicAdd(c < kMaxK ? counts + c : dropped, (unsigned long long)h[c]);
}

struct GatherArgs {
  MapView v;
  int lab_code, K;
  const void* lab;
  const float* keep_prob;
  int64_t ignore, ctr0;  // ctr0 = image_offset * h * w: the draw of pixel p of the call has counter ctr0 + p
  uint64_t seed;
  float* rows;
  int* row_labels;
  int64_t max_rows;
  int64_t* offsets;  // [chunks]: kept pixels per chunk, then (after the scan) kept pixels before the chunk
  int64_t* n_out;
};

// label of pixel p if it is kept, -1 otherwise: a pure function of (seed, ctr0 + p, label)
__device__ __forceinline__ int kept_label(const GatherArgs& a, int64_t p) {
  if (p >= a.v.P) return -1;
  const int64_t l = load_label(a.lab, a.lab_code, p);
  if (l == a.ignore || l < 0 || l >= a.K) return -1;
  const uint64_t ctr = (uint64_t)(a.ctr0 + p);
  const runia_philox::u4 b = runia_philox::philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)a.seed,
                                                         (uint32_t)(a.seed >> 32));
  return runia_philox::to_uniform(b.x) < a.keep_prob[l] ? (int)l : -1;
}

__global__ __launch_bounds__(256) void pixfeat_gather_count_kernel(GatherArgs a) {
  __shared__ int wsum[4];
  const int64_t p = (int64_t)blockIdx.x * kChunkPix + 4 * threadIdx.x;
  int n = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) n += kept_label(a, p + j) >= 0;
  int total;
  block_scan_excl<256>(n, wsum, total);
  if (threadIdx.x == 0) a.offsets[blockIdx.x] = total;
}

// one workgroup: counts -> the kept pixels before every chunk, and their sum
__global__ __launch_bounds__(1024) void pixfeat_gather_scan_kernel(int64_t* __restrict__ offsets, int64_t chunks,
                                                                   int64_t* __restrict__ n_out) {
  __shared__ long long s[1024];
  long long carry = 0;
  for (int64_t base = 0; base < chunks; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const long long v = i < chunks ? offsets[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const long long t = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
      __syncthreads();
      s[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < chunks) offsets[i] = carry + s[threadIdx.x] - v;
    carry += s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_out = carry;
}

template <class T>
__global__ __launch_bounds__(256) void pixfeat_gather_write_kernel(GatherArgs a) {
  typedef typename T::elem E;
  __shared__ int wsum[4];
  __shared__ int64_t koff[kChunkPix];
  __shared__ int klab[kChunkPix];
  const int64_t p = (int64_t)blockIdx.x * kChunkPix + 4 * threadIdx.x;
  int lab[4], n = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lab[j] = kept_label(a, p + j);
    n += lab[j] >= 0;
  }
  int total;
  int at = block_scan_excl<256>(n, wsum, total);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (lab[j] >= 0) {
      koff[at] = pixel_offset(a.v, p + j);
      klab[at] = lab[j];
      ++at;
    }
  }
  __syncthreads();
  const int64_t row0 = a.offsets[blockIdx.x];
  const E* x = static_cast<const E*>(a.v.x);
  const int C = a.v.C;
  for (int r = threadIdx.x; r < total; r += 256)
    if (row0 + r < a.max_rows) a.row_labels[row0 + r] = klab[r];
  for (int64_t idx = threadIdx.x; idx < (int64_t)total * C; idx += 256) {
    const int r = (int)(idx / C), c = (int)(idx - (int64_t)r * C);
    if (row0 + r < a.max_rows) a.rows[(row0 + r) * C + c] = widen(T{}, x[koff[r] + (int64_t)c * a.v.sc]);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
}  // namespace

extern "C" size_t runia_pixfeat_workspace_bytes(int64_t C, int64_t K) {
  (void)C;
  (void)K;
  return 0;  // the running sums live in registers and LDS: nothing scales with the pixels, and nothing is needed
}

extern "C" int runia_pixfeat_score(const void* features, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn,
                                   int64_t sc, int64_t sh, int64_t sw, const float* m0, const float* Wmat, const float* mz,
                                   int64_t K, float* distance, int32_t* nearest, float* class_distances, void* workspace,
                                   size_t workspace_bytes, runia_stream_t stream) {
  (void)workspace;
  (void)workspace_bytes;
  if (C < 1 || C > kMaxC || K < 1 || K > kMaxK || !elem_dtype_ok(dtype) || !view_ok(G, C, H, W, sn, sc, sh, sw))
    return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;
  if (!features || !m0 || !Wmat || !mz || (!distance && !nearest && !class_distances)) return RUNIA_E_INVALID;
  ScoreArgs a;
  a.v = make_view(features, G, C, H, W, sn, sc, sh, sw);
  a.K = (int)K;
  a.vecw = (C % 4 == 0 && reinterpret_cast<uintptr_t>(Wmat) % 16 == 0) ? 1 : 0;
  a.m0 = m0; a.W = Wmat; a.mz = mz;
  a.dist = distance; a.nearest = nearest; a.cd = class_distances;
  const unsigned grid = (unsigned)((a.v.P + kTP - 1) / kTP);
  hipStream_t s = as_stream(stream);
  return dispatch_elem(dtype, [&](auto t) {
    typedef decltype(t) T;
    if (view_allows_vec(a.v, G, H, T::kBytes)) pixfeat_score_kernel<T, kLoadVec><<<grid, 256, 0, s>>>(a);
    else if (view_allows_clast(a.v, G, H, T::V)) pixfeat_score_kernel<T, kLoadCLast><<<grid, 256, 0, s>>>(a);
    else pixfeat_score_kernel<T, kLoadElem><<<grid, 256, 0, s>>>(a);
    return runia_check_launch();
  });
}

extern "C" int runia_pixfeat_label_hist(const void* labels, int label_dtype, int64_t N, int64_t K, int64_t ignore_index,
                                        int64_t* counts, int64_t* dropped, runia_stream_t stream) {
  if (N < 0 || N > (kLim << 6) || K < 1 || K > kMaxK || label_dtype < kLabI64 || label_dtype > kLabU8 || !counts || !dropped)
    return RUNIA_E_INVALID;
  if (N > 0 && !labels) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)K, s) != hipSuccess ||
      hipMemsetAsync(dropped, 0, sizeof(int64_t), s) != hipSuccess)
    return RUNIA_E_LAUNCH;
  if (N == 0) return RUNIA_OK;
  pixfeat_hist_kernel<<<runia_stream_grid(N, 256 * 16), 256, 0, s>>>(
      labels, label_dtype, N, (int)K, ignore_index, reinterpret_cast<unsigned long long*>(counts),
      reinterpret_cast<unsigned long long*>(dropped));
  return runia_check_launch();
}

extern "C" size_t runia_pixfeat_gather_workspace_bytes(int64_t pixels) {
  if (pixels <= 0) return 0;
  return (size_t)((pixels + kChunkPix - 1) / kChunkPix) * sizeof(int64_t);
}

extern "C" int runia_pixfeat_gather_rows(const void* features, int dtype, int64_t G, int64_t C, int64_t H, int64_t W,
                                         int64_t sn, int64_t sc, int64_t sh, int64_t sw, const void* labels, int label_dtype,
                                         int64_t K, int64_t ignore_index, const float* keep_prob, uint64_t seed,
                                         int64_t image_offset, float* rows, int32_t* row_labels, int64_t max_rows,
                                         int64_t* n_out, void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (C > kMaxC || K < 1 || K > kMaxK || !elem_dtype_ok(dtype) || !view_ok(G, C, H, W, sn, sc, sh, sw) ||
      label_dtype < kLabI64 || label_dtype > kLabU8 || image_offset < 0 || image_offset > kLim || max_rows < 0 || !n_out ||
      !keep_prob)
    return RUNIA_E_INVALID;
  if ((rows == nullptr) != (row_labels == nullptr)) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  const int64_t P = G * H * W;
  if (P == 0) return hipMemsetAsync(n_out, 0, sizeof(int64_t), s) == hipSuccess ? RUNIA_OK : RUNIA_E_LAUNCH;
  if (!features || !labels) return RUNIA_E_INVALID;
  const size_t need = runia_pixfeat_gather_workspace_bytes(P);
  if (ws_refused(workspace, workspace_bytes, need, 8)) return RUNIA_E_WORKSPACE;
  GatherArgs a;
  a.v = make_view(features, G, C, H, W, sn, sc, sh, sw);
  a.lab_code = label_dtype;
  a.K = (int)K;
  a.lab = labels;
  a.keep_prob = keep_prob;
  a.ignore = ignore_index;
  a.ctr0 = image_offset * a.v.HW;
  a.seed = seed;
  a.rows = rows;
  a.row_labels = row_labels;
  a.max_rows = max_rows;
  a.offsets = static_cast<int64_t*>(workspace);
  a.n_out = n_out;
  const int64_t chunks = (P + kChunkPix - 1) / kChunkPix;
  pixfeat_gather_count_kernel<<<(unsigned)chunks, 256, 0, s>>>(a);
  pixfeat_gather_scan_kernel<<<1, 1024, 0, s>>>(a.offsets, chunks, n_out);
  if (rows && max_rows > 0)
    dispatch_elem(dtype, [&](auto t) {
      typedef decltype(t) T;
      pixfeat_gather_write_kernel<T><<<(unsigned)chunks, 256, 0, s>>>(a);
      return 0;
    });
  return runia_check_launch();
}
