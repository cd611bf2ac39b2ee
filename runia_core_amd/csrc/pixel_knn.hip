// Per-pixel k-nearest-neighbour maps from the feature maps of a segmentation decoder against a bank of in-distribution pixel
// features, read where the model left them, and the greedy k-center selection that builds such a bank.
//   runia_pixknn_score        ONE launch over G maps of (C, h, w) features in f32 / f16 / bf16 (NCHW, channels_last or any
//                             strided view): the k smallest squared distances of every pixel to the M bank rows, ascending,
//                             with the indices of those rows, the k-th and the mean of the k.
//   runia_kcenter_greedy_f32  farthest-point selection of n_pick rows of an (N, D) table, one launch per pick.
//
// Score.  d[p, j] = |x~_p|^2 - 2 x~_p . b~_j + |b~_j|^2 with x~ = x - center and the bank already centred: the centring keeps
// the digits of the Gram form when the features sit away from zero.  The loop is the one of pixel_features.hip with the bank
// in the place of the whitening matrix (pixel_map.hpp holds what the two share): a 256-thread workgroup owns 128 consecutive
// pixels of the flattened G * h * w axis (a tile may straddle images), 32 channels at a time of x - center go to LDS as
// Xs[channel][pixel] through one of three load forms that fill the same Xs, 128 bank rows x 32 channels go to Bs[row][34].
// On v_mfma_f32_32x32x2_f32 the bank rows are the A operand and the pixels the B operand, so that a lane holds ONE pixel
// (lane & 31) and, per 128-row bank block, 64 of its dot products: rows j0 + 32 t + (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of
// accumulator register r of tile t - in ascending order of j along (t, r).  The X chunk is staged again for every bank block
// (it comes from L2 after the first).  |x~|^2 is summed from the very values the matrix cores read while the first bank block
// passes (each lane half its half of the channels, in channel order; the halves are added once), so it is there before the
// first epilogue and every candidate is compared as the finished distance max(0, |x~|^2 + (|b~|^2 - 2 dot)).
// A tile's 16 distances pass through the lane's own column of an LDS strip, so that the selection is a loop (the insertion
// stands in the code four times per kernel, not 64: the build stays short).
// The k best (distance, index) are the last k entries of an ascending list of 16 in registers per lane (one kernel for every
// k: the entries in front hold -inf, which nothing goes before, so the k-th best is always the last entry and no register is
// indexed); a candidate is first compared with that last entry - the common case ends there - and inserted behind its equals
// otherwise.  A lane sees its rows in ascending order, so equal distances keep the lower index first; the two lane halves hold
// different rows of the same pixel, and their lists are merged once after the last block, in (distance, index) order.
// Every sum runs in one lane in a fixed order, no atomics: results are run-to-run bit identical and do not depend on where in
// the batch a pixel sits or on the load form.  A pixel whose |x~|^2 is not finite (NaN or inf features) gets NaN distances and
// index -1; it is a column of the B operand and nothing of it reaches another column.
//
// k-center.  Launch t finds the newest centre (t = 0: `first`; later: the argmax the launch before left as one (value, index)
// per workgroup, reduced again by every workgroup - a maximum with the lowest index on ties does not depend on the order),
// measures every row against it in difference form (a wave per row, lanes stride the columns, fmaf chain then the wave's
// butterfly sum: a fixed order), lowers min_dist and leaves its own per-workgroup maxima for the next launch.  The launches
// are queued back to back; nothing is read back in between.  Once the largest remaining distance is not positive every
// remaining row duplicates a picked one and the later launches only write -1.
#include <cmath>

#include "common.hpp"
#include "elem.hpp"
#include "pixel_map.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTB = 128;              // bank rows per block
constexpr int kMaxKnn = 16;           // neighbours per pixel
constexpr int64_t kMaxBank = 1 << 22;
constexpr int kKcBlocks = 1024;       // workgroups of a k-center launch at most (each leaves one maximum)
constexpr int kKcMaxD = 1024;

struct KnnArgs {
  MapView v;
  int M, k, vecb;
  const float *center, *bank, *bank_sq;
  float* dist;
  int* idx;
  float* kth;
  float* mean;
};

// (d, j) goes before (e, ei): smaller distance; LEX: on equal distances the lower index
template <bool LEX>
__device__ __forceinline__ bool goes_before(float d, int j, float e, int ei) {
  return d < e || (LEX && d == e && j < ei);
}

// insert (d, j) into the ascending list, behind its equals (LEX: in index order); the last entry falls out
template <int KK, bool LEX>
__device__ __forceinline__ void list_insert(float (&dv)[KK], int (&di)[KK], float d, int j) {
#pragma unroll
  for (int i = KK - 1; i > 0; --i) {
    if (goes_before<LEX>(d, j, dv[i - 1], di[i - 1])) {
      dv[i] = dv[i - 1];
      di[i] = di[i - 1];
    } else if (goes_before<LEX>(d, j, dv[i], di[i])) {
      dv[i] = d;
      di[i] = j;
    }
  }
  if (goes_before<LEX>(d, j, dv[0], di[0])) {
    dv[0] = d;
    di[0] = j;
  }
}

template <class T, int LOAD>
__global__ __launch_bounds__(256) void pixknn_score_kernel(KnnArgs a) {
  constexpr bool VEC = LOAD == kLoadVec;
  constexpr int KK = kMaxKnn;
  __shared__ __attribute__((aligned(16))) float Xs[kKCh][kXP];
  __shared__ __attribute__((aligned(16))) float Bs[kTB][kWP];
  __shared__ __attribute__((aligned(16))) float Bq[kTB];
  __shared__ float Ds[4][16][64];  // per wave: the 16 distances of one accumulator tile, a column per lane
  __shared__ float cs[kMaxC];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int C = a.v.C, M = a.M, k = a.k;
  const int64_t p0 = (int64_t)blockIdx.x * kTP;

  for (int c = tid; c < kMaxC; c += 256) cs[c] = c < C ? a.center[c] : 0.f;

  // the four pixels (channels_last: the one pixel) this thread stages
  int64_t off[4];
  const int nv = staged_pixels<LOAD>(a.v, p0, tid, off);
  // the pixel whose list this lane holds
  const int64_t pm = p0 + wave * 32 + li;
  const bool mine = pm < a.v.P;
  const int64_t gm = mine ? pm / a.v.HW : 0, qm = mine ? pm - gm * a.v.HW : 0;

  float dv[KK];
  int di[KK];
#pragma unroll
  for (int i = 0; i < KK; ++i) {  // the k best are the LAST k entries: the k-th best, what a candidate has to beat, is dv[KK - 1]
    dv[i] = i >= KK - k ? INFINITY : -INFINITY;  // (nothing goes before -inf: the entries in front are never touched)
    di[i] = -1;
  }
  float xsq = 0.f;

  for (int j0 = 0; j0 < M; j0 += kTB) {
    __syncthreads();  // the epilogue of the block before is through with Bq
    if (tid < kTB) Bq[tid] = j0 + tid < M ? a.bank_sq[j0 + tid] : 0.f;
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float xr[16], wr[16];
    if constexpr (LOAD == kLoadCLast) load_x_cl<T>(a.v, off[0], nv > 0, 0, tid, xr);
    else load_x<T, VEC>(a.v, off, nv, 0, tid, xr);
    load_w(a.bank, M, C, j0, 0, tid, a.vecb != 0, wr);
    for (int k0 = 0; k0 < C; k0 += kKCh) {
      __syncthreads();  // every wave has finished reading the previous chunk
      if constexpr (LOAD == kLoadCLast) store_x_cl(xr, Xs, cs, k0, tid);
      else store_x(xr, Xs, cs, k0, tid);
      store_w(wr, Bs, tid);
      __syncthreads();
      if (k0 + kKCh < C) {  // next chunk's loads fly while the matrix cores consume this one
        if constexpr (LOAD == kLoadCLast) load_x_cl<T>(a.v, off[0], nv > 0, k0 + kKCh, tid, xr);
        else load_x<T, VEC>(a.v, off, nv, k0 + kKCh, tid, xr);
        load_w(a.bank, M, C, j0, k0 + kKCh, tid, a.vecb != 0, wr);
      }
#pragma unroll
      for (int s = 0; s < kKCh / 4; ++s) {
        const float bx = Xs[4 * s + 2 * lh][wave * 32 + li], by = Xs[4 * s + 2 * lh + 1][wave * 32 + li];
        if (j0 == 0) {
          xsq = fmaf(bx, bx, xsq);
          xsq = fmaf(by, by, xsq);
        }
        float2 av[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) av[t] = *reinterpret_cast<const float2*>(&Bs[t * 32 + li][4 * s + 2 * lh]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].x, bx, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].y, by, acc[t], 0, 0, 0);
        }
      }
    }
    if (j0 == 0) xsq += __shfl_xor(xsq, 32, 64);
    // acc[t][r] = x~ . b~_j, j = j0 + 32 t + (r & 3) + 8 (r >> 2) + 4 lh, of pixel li: ascending j along (t, r).  A tile's 16
    // distances go through the lane's own column of Ds (no other lane reads it: no barrier) so that the loop over them is a
    // loop and the insertion stands in the code four times, not 64
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const float4 q4 = *reinterpret_cast<const float4*>(&Bq[t * 32 + 8 * rq + 4 * lh]);
        const float q[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = xsq + fmaf(-2.f, acc[t][4 * rq + e], q[e]);
          Ds[wave][4 * rq + e][lane] = d < 0.f ? 0.f : d;  // (a NaN stays a NaN and is never inserted)
        }
      }
      const int jt = j0 + t * 32 + 4 * lh;
      for (int r = 0; r < 16; ++r) {
        const int j = jt + (r & 3) + 8 * (r >> 2);
        const float d = Ds[wave][r][lane];
        if (j < M && d < dv[KK - 1]) list_insert<KK, false>(dv, di, d, j);
      }
    }
  }

  // the other lane half holds the other rows of the same pixel: merge its list in, in (distance, index) order
  float ov[KK];
  int oi[KK];
#pragma unroll
  for (int i = 0; i < KK; ++i) {
    ov[i] = __shfl_xor(dv[i], 32, 64);
    oi[i] = __shfl_xor(di[i], 32, 64);
  }
#pragma unroll
  for (int i = 0; i < KK; ++i)
    if (oi[i] >= 0) list_insert<KK, true>(dv, di, ov[i], oi[i]);

  if (mine && lh == 0) {
    const bool bad = !(xsq < INFINITY);  // NaN or inf among the pixel's features
    const int64_t base = gm * k * a.v.HW + qm;
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < KK; ++e) {
      const int i = e - (KK - k);  // the rank of entry e
      if (i >= 0) {
        const float d = bad ? __builtin_nanf("") : dv[e];
        if (a.dist) a.dist[base + i * a.v.HW] = d;
        if (a.idx) a.idx[base + i * a.v.HW] = bad ? -1 : di[e];
        sum = i == 0 ? d : sum + d;
      }
    }
    if (a.kth) a.kth[pm] = bad ? __builtin_nanf("") : dv[KK - 1];
    if (a.mean) a.mean[pm] = sum / (float)k;
  }
}

// ---- k-center -------------------------------------------------------------------------------------------------------------------
struct KcBest {
  float v;
  int i;
};

struct KcArgs {
  const float* rows;
  int64_t N;
  int D, t, first, nb_prev, vec;
  float* min_dist;
  const KcBest* prev;
  KcBest* next;
  int* picked;
  float* radius;
  int64_t* n_picked;
};

__global__ __launch_bounds__(256) void kcenter_step_kernel(KcArgs a) {
  __shared__ __attribute__((aligned(16))) float ctr[kKcMaxD];
  __shared__ float wv[4];
  __shared__ int wi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the newest centre: the largest min_dist the launch before found, lowest index on ties
  float bv = INFINITY;
  int bi = a.first;
  if (a.t > 0) {
    bv = -1.f;
    bi = kNoIndex;
    for (int e = tid; e < a.nb_prev; e += 256) best_take(bv, bi, a.prev[e].v, a.prev[e].i);
    wave_best(bv, bi);
    if (lane == 0) {
      wv[wave] = bv;
      wi[wave] = bi;
    }
    __syncthreads();
    bv = wv[0];
    bi = wi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best_take(bv, bi, wv[w], wi[w]);
    __syncthreads();  // wv and wi are used again below
  }
  const bool stop = !(bv > 0.f);  // every remaining row duplicates a picked one (the same in every workgroup)
  if (blockIdx.x == 0 && tid == 0) {
    a.picked[a.t] = stop ? -1 : bi;
    a.radius[a.t] = stop ? 0.f : bv;
    if (!stop) *a.n_picked = a.t + 1;
  }
  if (stop) {
    if (tid == 0) a.next[blockIdx.x] = KcBest{0.f, kNoIndex};  // the launches after this one stop as well
    return;
  }
  const int D = a.D;
  for (int c = tid; c < D; c += 256) ctr[c] = a.rows[(int64_t)bi * D + c];
  __syncthreads();

  float mv = -1.f;
  int mi = kNoIndex;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < a.N; row += (int64_t)gridDim.x * 4) {
    const float* p = a.rows + row * D;
    float s = 0.f;
    if (a.vec) {
      for (int c = lane; c < (D >> 2); c += 64) {
        const float4 x = reinterpret_cast<const float4*>(p)[c], m = reinterpret_cast<const float4*>(ctr)[c];
        const float d0 = x.x - m.x, d1 = x.y - m.y, d2 = x.z - m.z, d3 = x.w - m.w;
        s = fmaf(d0, d0, s);
        s = fmaf(d1, d1, s);
        s = fmaf(d2, d2, s);
        s = fmaf(d3, d3, s);
      }
    } else {
      for (int c = lane; c < D; c += 64) {
        const float d = p[c] - ctr[c];
        s = fmaf(d, d, s);
      }
    }
    s = wave_sum_f32(s);
    float m = s;
    if (a.t > 0) {
      const float old = a.min_dist[row];
      m = s < old ? s : old;
    }
    if (lane == 0) a.min_dist[row] = m;
    best_take(mv, mi, m, (int)row);
  }
  if (lane == 0) {
    wv[wave] = mv;
    wi[wave] = mi;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) best_take(mv, mi, wv[w], wi[w]);
    a.next[blockIdx.x] = KcBest{mv, mi};
  }
}

__global__ __launch_bounds__(256) void kcenter_tail_kernel(int* __restrict__ picked, float* __restrict__ radius, int64_t from,
                                                           int64_t to) {
  for (int64_t i = from + (int64_t)blockIdx.x * 256 + threadIdx.x; i < to; i += (int64_t)gridDim.x * 256) {
    picked[i] = -1;
    radius[i] = 0.f;
  }
}

struct KcPlan { float* min_dist; KcBest* best[2]; };  // [N] (16-byte slot) | two sets of per-workgroup records
KcPlan kc_plan(WsWalk& w, int64_t N) {
  KcPlan p;
  p.min_dist = w.take<float>(N, 16);
  p.best[0] = w.take<KcBest>(kKcBlocks);
  p.best[1] = w.take<KcBest>(kKcBlocks);
  return p;
}

}  // namespace

extern "C" size_t runia_pixknn_workspace_bytes(int64_t C, int64_t M, int64_t k) {
  (void)C;
  (void)M;
  (void)k;
  return 0;  // the lists live in registers: nothing scales with the pixels or the bank, and nothing is needed
}

extern "C" int runia_pixknn_score(const void* features, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn,
                                  int64_t sc, int64_t sh, int64_t sw, const float* center, const float* bank,
                                  const float* bank_sq, int64_t M, int64_t k, float* distances, int32_t* indices,
                                  float* kth_distance, float* mean_distance, void* workspace, size_t workspace_bytes,
                                  runia_stream_t stream) {
  (void)workspace;
  (void)workspace_bytes;
  if (C < 1 || C > kMaxC || k < 1 || k > kMaxKnn || M < k || M > kMaxBank || !elem_dtype_ok(dtype) ||
      !view_ok(G, C, H, W, sn, sc, sh, sw))
    return RUNIA_E_INVALID;
  if (G > 0 && H * W > 0 && G * H * W > kLim) return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;
  if (!features || !center || !bank || !bank_sq || (!distances && !indices && !kth_distance && !mean_distance))
    return RUNIA_E_INVALID;
  KnnArgs a;
  a.v = make_view(features, G, C, H, W, sn, sc, sh, sw);
  a.M = (int)M;
  a.k = (int)k;
  a.vecb = (C % 4 == 0 && reinterpret_cast<uintptr_t>(bank) % 16 == 0) ? 1 : 0;
  a.center = center; a.bank = bank; a.bank_sq = bank_sq;
  a.dist = distances; a.idx = indices; a.kth = kth_distance; a.mean = mean_distance;
  const unsigned grid = (unsigned)((a.v.P + kTP - 1) / kTP);
  hipStream_t s = as_stream(stream);
  return dispatch_elem(dtype, [&](auto t) {
    typedef decltype(t) T;
    if (view_allows_vec(a.v, G, H, T::kBytes)) pixknn_score_kernel<T, kLoadVec><<<grid, 256, 0, s>>>(a);
    else if (view_allows_clast(a.v, G, H, T::V)) pixknn_score_kernel<T, kLoadCLast><<<grid, 256, 0, s>>>(a);
    else pixknn_score_kernel<T, kLoadElem><<<grid, 256, 0, s>>>(a);
    return runia_check_launch();
  });
}

extern "C" size_t runia_kcenter_workspace_bytes(int64_t N, int64_t D) {
  if (N < 1 || N > kLim || D < 1 || D > kKcMaxD) return 0;
  return ws_bytes([&](WsWalk& w) { kc_plan(w, N); });
}

extern "C" int runia_kcenter_greedy_f32(const float* rows, int64_t N, int64_t D, int64_t first, int64_t n_pick,
                                        int32_t* picked, float* radius, int64_t* n_picked, void* workspace,
                                        size_t workspace_bytes, runia_stream_t stream) {
  if (N < 1 || N > kLim || D < 1 || D > kKcMaxD || first < 0 || first >= N || n_pick < 1 || n_pick > kLim || !rows || !picked ||
      !radius || !n_picked)
    return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const KcPlan plan = kc_plan(w, N);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  KcArgs a;
  a.rows = rows;
  a.N = N;
  a.D = (int)D;
  a.first = (int)first;
  a.vec = (D % 4 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0) ? 1 : 0;
  a.min_dist = plan.min_dist;
  KcBest* const* best = plan.best;
  a.picked = picked;
  a.radius = radius;
  a.n_picked = n_picked;
  const int64_t blocks = (N + 3) / 4;
  const int nb = (int)(blocks < kKcBlocks ? blocks : kKcBlocks);
  a.nb_prev = nb;
  hipStream_t s = as_stream(stream);
  const int64_t steps = n_pick < N ? n_pick : N;  // N picks at the most: then nothing is left
  for (int64_t t = 0; t < steps; ++t) {
    a.t = (int)t;
    a.prev = best[(t + 1) & 1];
    a.next = best[t & 1];
    kcenter_step_kernel<<<nb, 256, 0, s>>>(a);
  }
  if (n_pick > steps) kcenter_tail_kernel<<<runia_stream_grid(n_pick - steps, 256), 256, 0, s>>>(picked, radius, steps, n_pick);
  return runia_check_launch();
}
