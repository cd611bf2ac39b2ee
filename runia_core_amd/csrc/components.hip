// Connected-component labelling of N binary images (H, W) and the overlap statistics of the component-level anomaly
// segmentation metrics (sIoU, PPV, F1*: Chan et al. 2021, SegmentMeIfYouCan); evaluation/components.py, DESIGN 4.45.
//   runia_cc_label     labels int32 (N, H, W): 0 background, 1 .. counts[n] in raster order of each component's first pixel
//                      (the per-image contract of scipy.ndimage.label), 4- or 8-connectivity.  An image is a uint8 mask or an
//                      f32 score map compared with one of T thresholds inside the tile kernel (no predicted mask in memory).
//   runia_cc_overlap   integer sizes / intersections per component and the distinct (GT component, predicted component)
//                      pairs, one candidate key per row run of a pair.
//   runia_cc_relabel   labels through a per-component table (the min_component_size filter).
//
// Labelling is union-find on parent pointers that are image-global pixel indices (int32, -1 = background), always linked
// towards the SMALLER index: the root of a component is its first pixel in raster order, so the canonical numbering is the
// exclusive count of roots before it and does not depend on the order in which atomics arrive.  Six launches:
//   1 cc_tile_kernel     one workgroup per RUNIA_CC_TILE_H x RUNIA_CC_TILE_W tile: source -> LDS, unions with the left / upper
//                        neighbours by atomicMin in LDS, every pixel flattened to its tile root, parents stored.
//   2 cc_merge_kernel    one thread per pixel of a tile's first row / first column: unions with its neighbours in the tile
//                        above / to the left (the diagonal ones at the corners included under 8-connectivity).
//   3 cc_flatten_kernel  every pixel -> its root; roots counted per 1024-pixel chunk.
//   4 cc_scan_kernel     per image, exclusive scan of the chunk counts; counts[n].
//   5 cc_rank_kernel     roots take -(rank + 1) (scan of the root flags inside the chunk, in pixel order).
//   6 cc_final_kernel    every pixel reads the rank of its root.
// A phase that needs another phase's plain stores is another launch (the eight L2s are not coherent for plain accesses
// inside one).  Inside 2, 3 and 6 a parent that another workgroup may rewrite in the same launch is read with an agent-scope
// relaxed atomic load and linked with an agent-scope atomicMin: whatever value arrives is an ancestor (2, 3) or one of the two
// encodings of the same rank (6), so staleness costs steps, never correctness.
// No loop waits for another workgroup.  find() walks strictly decreasing indices, union() retries only with the strictly
// smaller parent atomicMin returned; both also carry a step cap (pixels of a tile / of an image) that sets the error word.
#include "common.hpp"

namespace {

constexpr int TH = RUNIA_CC_TILE_H, TW = RUNIA_CC_TILE_W, kTilePix = TH * TW;
constexpr int kThreads = 256;
constexpr int kPerThread = kTilePix / kThreads;
constexpr int kChunkTrips = 4, kChunk = kThreads * kChunkTrips;  // pixels per workgroup of the flat passes
static_assert(kTilePix % kThreads == 0 && kTilePix <= 8192 && TW >= 2 && TH >= 2, "tile shape");

constexpr unsigned kErrFind = 1u, kErrUnion = 2u;

struct CcSource {
  const uint8_t* mask;   // (N, H, W), or
  const float* score;    // (G, H, W) with thr[T]: image n = t * G + g is score[g] compared with thr[t]
  const float* thr;
  const uint8_t* valid;  // (N, H, W) with a mask, (G, H, W) with scores; may be null
  int64_t G;
  int less;
};

__device__ __forceinline__ bool source_pixel(const CcSource& s, int64_t n, int64_t HW, int64_t pix) {
  if (s.score) {
    const int64_t g = n % s.G, at = g * HW + pix;
    const float x = s.score[at], d = s.thr[n / s.G];
    const bool on = s.less ? x < d : x > d;  // NaN: neither
    return on && (!s.valid || s.valid[at] != 0);
  }
  const int64_t at = n * HW + pix;
  return s.mask[at] != 0 && (!s.valid || s.valid[at] != 0);
}

// ---- union-find on LDS (workgroup scope) and on the parent image (agent scope) ------------------------------------------------
template <bool GLOBAL>
__device__ __forceinline__ int uf_load(int* p) {
  if constexpr (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GLOBAL>
__device__ __forceinline__ int uf_min(int* p, int v) {
  if constexpr (GLOBAL) return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// root of x: parents never exceed their pixel, so the chain strictly decreases and ends within `cap` steps
template <bool GLOBAL>
__device__ __forceinline__ int uf_find(int* P, int x, int cap, unsigned& err) {
  for (int s = 0; s <= cap; ++s) {
    const int p = uf_load<GLOBAL>(P + x);
    if (p == x) return x;
    x = p;
  }
  err |= kErrFind;
  return x;
}

// link the larger root under the smaller one; when another thread linked it first (atomicMin returns its smaller parent),
// go on with that parent
template <bool GLOBAL>
__device__ __forceinline__ void uf_union(int* P, int a, int b, int cap, unsigned& err) {
  for (int s = 0; s <= cap; ++s) {
    a = uf_find<GLOBAL>(P, a, cap, err);
    b = uf_find<GLOBAL>(P, b, cap, err);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = uf_min<GLOBAL>(P + a, b);
    if (old == a) return;
    a = old;  // < a
  }
  err |= kErrUnion;
}

__device__ __forceinline__ void report(unsigned err, unsigned* word) {
  if (err) atomicOr(word, err);
}

// ---- 1: tiles ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cc_tile_kernel(CcSource src, int H, int W, int ntx, int nty, int conn8,
                                                           int* __restrict__ P, unsigned* err_word) {
  __shared__ int L[kTilePix];
  const int b = blockIdx.x;
  const int tx = b % ntx, ty = (b / ntx) % nty;
  const int64_t n = b / (ntx * nty), HW = (int64_t)H * W;
  const int y0 = ty * TH, x0 = tx * TW;
  unsigned err = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int li = k * kThreads + threadIdx.x, y = y0 + li / TW, x = x0 + li % TW;
    const bool on = y < H && x < W && source_pixel(src, n, HW, (int64_t)y * W + x);
    L[li] = on ? li : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int li = k * kThreads + threadIdx.x, ly = li / TW, lx = li % TW;
    if (uf_load<false>(L + li) < 0) continue;
    const bool left = lx > 0 && uf_load<false>(L + li - 1) >= 0;
    const bool up = ly > 0 && uf_load<false>(L + li - TW) >= 0;
    if (left) uf_union<false>(L, li, li - 1, kTilePix, err);
    if (up) uf_union<false>(L, li, li - TW, kTilePix, err);
    if (conn8 && ly > 0 && !up) {  // (with the upper pixel set, both diagonals are its row neighbours)
      if (!left && lx > 0 && uf_load<false>(L + li - TW - 1) >= 0) uf_union<false>(L, li, li - TW - 1, kTilePix, err);
      if (lx < TW - 1 && uf_load<false>(L + li - TW + 1) >= 0) uf_union<false>(L, li, li - TW + 1, kTilePix, err);
    }
  }
  __syncthreads();
  const int64_t base = n * HW;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int li = k * kThreads + threadIdx.x, y = y0 + li / TW, x = x0 + li % TW;
    if (y >= H || x >= W) continue;
    int parent = -1;
    if (uf_load<false>(L + li) >= 0) {
      const int r = uf_find<false>(L, li, kTilePix, err);
      parent = (int)(base + (int64_t)(y0 + r / TW) * W + x0 + r % TW);
    }
    P[base + (int64_t)y * W + x] = parent;
  }
  report(err, err_word);
}

// ---- 2: tile borders ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void merge_with(int* P, int me, int other, int cap, unsigned& err) {
  if (uf_load<true>(P + other) >= 0) uf_union<true>(P, me, other, cap, err);
}

__global__ __launch_bounds__(kThreads) void cc_merge_kernel(int* P, int H, int W, int ntx, int nty, int conn8, int64_t n_rows,
                                                            int64_t items, unsigned* err_word) {
  const int64_t HW = (int64_t)H * W;
  const int cap = (int)(HW < 0x7ffffff0ll ? HW : 0x7ffffff0ll);
  unsigned err = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += (int64_t)gridDim.x * kThreads) {
    if (i < n_rows) {  // a pixel of a tile's first row against the row above
      const int64_t per = (int64_t)(nty - 1) * W, n = i / per, r = i % per;
      const int y = (int)(r / W + 1) * TH, x = (int)(r % W);
      const int me = (int)(n * HW + (int64_t)y * W + x);
      if (uf_load<true>(P + me) < 0) continue;
      const int up = me - W;
      if (uf_load<true>(P + up) >= 0) {
        uf_union<true>(P, me, up, cap, err);
      } else if (conn8) {
        if (x > 0) merge_with(P, me, up - 1, cap, err);
        if (x < W - 1) merge_with(P, me, up + 1, cap, err);
      }
    } else {  // a pixel of a tile's first column against the column to its left
      const int64_t j = i - n_rows, per = (int64_t)(ntx - 1) * H, n = j / per, r = j % per;
      const int x = (int)(r / H + 1) * TW, y = (int)(r % H);
      const int me = (int)(n * HW + (int64_t)y * W + x);
      if (uf_load<true>(P + me) < 0) continue;
      const int left = me - 1;
      if (uf_load<true>(P + left) >= 0) {
        uf_union<true>(P, me, left, cap, err);
      } else if (conn8) {
        if (y > 0) merge_with(P, me, left - W, cap, err);
        if (y < H - 1) merge_with(P, me, left + W, cap, err);
      }
    }
  }
  report(err, err_word);
}

// ---- 3: flatten, count the roots of every chunk -------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cc_flatten_kernel(int* P, int64_t HW, int cpi, int* __restrict__ chunk_count,
                                                              unsigned* err_word) {
  __shared__ int s_wave[kThreads / 64];
  const int64_t n = blockIdx.x / cpi, start = (int64_t)(blockIdx.x % cpi) * kChunk, base = n * HW;
  const int cap = (int)(HW < 0x7ffffff0ll ? HW : 0x7ffffff0ll);
  unsigned err = 0;
  int roots = 0;
#pragma unroll
  for (int k = 0; k < kChunkTrips; ++k) {
    const int64_t i = start + k * kThreads + threadIdx.x;
    if (i >= HW) continue;
    const int me = (int)(base + i);
    const int p = uf_load<true>(P + me);
    if (p < 0) continue;
    const int r = uf_find<true>(P, p, cap, err);
    if (r != p) __hip_atomic_store(P + me, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    roots += r == me;
  }
  int total;
  __syncthreads();
  block_scan_excl<kThreads>(roots, s_wave, total);
  if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
  report(err, err_word);
}

// ---- 4: per image, where every chunk's ranks begin ----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cc_scan_kernel(const int* __restrict__ chunk_count, int* __restrict__ chunk_base,
                                                           int cpi, int* __restrict__ counts) {
  __shared__ int s_wave[kThreads / 64];
  const int64_t row = (int64_t)blockIdx.x * cpi;
  int carry = 0;
  for (int c0 = 0; c0 < cpi; c0 += kThreads) {
    const int c = c0 + threadIdx.x;
    const int v = c < cpi ? chunk_count[row + c] : 0;
    int total;
    __syncthreads();  // (s_wave of the previous trip has been read)
    const int ex = block_scan_excl<kThreads>(v, s_wave, total);
    if (c < cpi) chunk_base[row + c] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// ---- 5: roots take -(rank + 1) -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cc_rank_kernel(int* __restrict__ P, int64_t HW, int cpi,
                                                           const int* __restrict__ chunk_base) {
  __shared__ int s_wave[kThreads / 64];
  const int64_t n = blockIdx.x / cpi, start = (int64_t)(blockIdx.x % cpi) * kChunk, base = n * HW;
  int running = chunk_base[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kChunkTrips; ++k) {
    const int64_t i = start + k * kThreads + threadIdx.x;
    const bool root = i < HW && P[base + i] == (int)(base + i);
    int total;
    __syncthreads();  // (s_wave of the previous trip has been read)
    const int ex = block_scan_excl<kThreads>(root ? 1 : 0, s_wave, total);
    if (root) P[base + i] = -(running + ex + 1) - 1;
    running += total;
  }
}

// ---- 6: every pixel reads its root's rank --------------------------------------------------------------------------------------
// A root holds -(rank + 1) until its own thread turns it into rank: a reader takes either form.
__global__ __launch_bounds__(kThreads) void cc_final_kernel(int* P, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int p = P[i];  // (written by this thread alone in this launch)
    int lab = 0;
    if (p < -1) {
      lab = -p - 1;
    } else if (p >= 0) {
      const int v = uf_load<true>(P + p);
      lab = v < 0 ? -v - 1 : v;
    }
    __hip_atomic_store(P + i, lab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- overlap statistics --------------------------------------------------------------------------------------------------------
constexpr int kSeg = 8;  // consecutive pixels of one thread

struct OverlapArgs {
  const int *gt, *gt_off, *pred, *pred_off;
  int64_t G, NI, HW, W, Kg, segs, items, cap;
  int *gt_size, *gt_inter, *pred_size, *pred_inter;
  long long* keys;
  unsigned long long* n_keys;
  int stats;
};

__device__ __forceinline__ void flush_gt(const OverlapArgs& a, int64_t t, int goff, int run, int size, int inter) {
  if (run <= 0) return;
  if (a.gt_size && t == 0) atomicAdd(a.gt_size + goff + run - 1, size);
  if (inter) atomicAdd(a.gt_inter + t * a.Kg + goff + run - 1, inter);
}
__device__ __forceinline__ void flush_pred(const OverlapArgs& a, int poff, int run, int size, int inter) {
  if (run <= 0) return;
  atomicAdd(a.pred_size + poff + run - 1, size);
  if (inter) atomicAdd(a.pred_inter + poff + run - 1, inter);
}

// A thread walks kSeg consecutive pixels of image n = t * G + g: the sizes and intersections of the label runs it sees go to
// the integer tables once per run, and a pixel set in both label images whose left neighbour (same row) holds another pair
// starts a run of its pair: one candidate key ((t * Kg + k) << 32 | k_hat) per such run, placed by one counter add per thread.
__global__ __launch_bounds__(kThreads) void cc_overlap_kernel(OverlapArgs a) {
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < a.items; it += (int64_t)gridDim.x * kThreads) {
    const int64_t n = it / a.segs, i0 = (it % a.segs) * kSeg, g = n % a.G, t = n / a.G;
    const int* gl = a.gt ? a.gt + g * a.HW : nullptr;
    const int* pl = a.pred ? a.pred + n * a.HW : nullptr;
    const int goff = gl ? a.gt_off[g] : 0, poff = pl ? a.pred_off[n] : 0;
    int64_t col = i0 % a.W;
    int pa = 0, pb = 0;  // the labels of the pixel before
    if (col != 0) {
      pa = gl ? gl[i0 - 1] : 0;
      pb = pl ? pl[i0 - 1] : 0;
    }
    int run_a = 0, size_a = 0, inter_a = 0, run_b = 0, size_b = 0, inter_b = 0, n_new = 0;
    unsigned new_mask = 0;
    long long fresh[kSeg];
#pragma unroll
    for (int j = 0; j < kSeg; ++j) {
      const int64_t i = i0 + j;
      const bool in = i < a.HW;
      const int la = in && gl ? gl[i] : 0, lb = in && pl ? pl[i] : 0;
      if (a.stats) {
        if (la != run_a) {
          flush_gt(a, t, goff, run_a, size_a, inter_a);
          run_a = la; size_a = 0; inter_a = 0;
        }
        if (lb != run_b) {
          flush_pred(a, poff, run_b, size_b, inter_b);
          run_b = lb; size_b = 0; inter_b = 0;
        }
        size_a += 1; inter_a += lb > 0;
        size_b += 1; inter_b += la > 0;
      }
      const bool is_new = la > 0 && lb > 0 && (col == 0 || la != pa || lb != pb);
      fresh[j] = ((long long)(t * a.Kg + goff + la - 1) << 32) | (long long)(unsigned)(poff + lb - 1);
      new_mask |= (is_new ? 1u : 0u) << j;
      n_new += is_new;
      pa = la;
      pb = lb;
      col = col + 1 == a.W ? 0 : col + 1;
    }
    if (a.stats) {
      flush_gt(a, t, goff, run_a, size_a, inter_a);
      flush_pred(a, poff, run_b, size_b, inter_b);
    }
    if (n_new && a.n_keys) {
      unsigned long long at = atomicAdd(a.n_keys, (unsigned long long)n_new);
      if (a.keys) {
#pragma unroll
        for (int j = 0; j < kSeg; ++j) {
          if ((new_mask >> j) & 1u) {
            if ((int64_t)at < a.cap) a.keys[at] = fresh[j];
            ++at;
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void cc_relabel_kernel(int* __restrict__ labels, const int* __restrict__ off,
                                                              const int* __restrict__ map, int64_t HW, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int l = labels[i];
    if (l > 0) labels[i] = map[off[(unsigned)i / (unsigned)HW] + l - 1];  // (i < 2^31)
  }
}

int64_t chunks_per_image(int64_t HW) { return (HW + kChunk - 1) / kChunk; }

}  // namespace

extern "C" int runia_cc_tile_h(void) { return TH; }
extern "C" int runia_cc_tile_w(void) { return TW; }

struct CcPlan { unsigned* err_word; int *chunk_count, *chunk_base; };  // error word (16-byte slot) | [N][chunks] x 2
static CcPlan cc_plan(WsWalk& w, int64_t N, int64_t HW) {
  const size_t chunks = (size_t)N * (size_t)chunks_per_image(HW);
  CcPlan p;
  p.err_word = w.take<unsigned>(1, 16);
  p.chunk_count = w.take<int>(chunks);
  p.chunk_base = w.take<int>(chunks);
  return p;
}
extern "C" size_t runia_cc_label_workspace_bytes(int64_t N, int64_t H, int64_t W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return ws_bytes([&](WsWalk& w) { cc_plan(w, N, H * W); });
}

extern "C" int runia_cc_label(const uint8_t* mask, const float* score, const float* thresholds, int64_t T, int less,
                              const uint8_t* valid, int64_t G, int64_t H, int64_t W, int connectivity, int32_t* labels,
                              int32_t* counts, void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  const int64_t lim = 0x7fffffffll;
  if (G < 0 || H < 0 || W < 0 || G > lim || H > lim || W > lim || (connectivity != 4 && connectivity != 8)) return RUNIA_E_INVALID;
  if ((mask != nullptr) == (score != nullptr) && G > 0 && H * W > 0) return RUNIA_E_INVALID;
  if (score ? (T < 0 || T > lim) : T != 1) return RUNIA_E_INVALID;
  const int64_t N = G * T, HW = H * W;
  if (N == 0 || HW == 0) return RUNIA_OK;
  if (HW > lim || N > lim / HW) return RUNIA_E_INVALID;  // parents are int32
  if (!labels || !counts || (score && !thresholds)) return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const CcPlan plan = cc_plan(w, N, HW);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  unsigned* err_word = plan.err_word;
  const int cpi = (int)chunks_per_image(HW);
  int *chunk_count = plan.chunk_count, *chunk_base = plan.chunk_base;
  if (hipMemsetAsync(err_word, 0, 16, s) != hipSuccess) return RUNIA_E_LAUNCH;
  const int ntx = (int)((W + TW - 1) / TW), nty = (int)((H + TH - 1) / TH), conn8 = connectivity == 8;
  CcSource src{mask, score, thresholds, valid, score ? G : N, less != 0};
  cc_tile_kernel<<<(unsigned)(N * ntx * nty), kThreads, 0, s>>>(src, (int)H, (int)W, ntx, nty, conn8, labels, err_word);
  const int64_t n_rows = N * (nty - 1) * W, n_cols = N * (ntx - 1) * H;
  if (n_rows + n_cols > 0)
    cc_merge_kernel<<<runia_stream_grid(n_rows + n_cols, kThreads), kThreads, 0, s>>>(labels, (int)H, (int)W, ntx, nty, conn8,
                                                                                      n_rows, n_rows + n_cols, err_word);
  cc_flatten_kernel<<<(unsigned)(N * cpi), kThreads, 0, s>>>(labels, HW, cpi, chunk_count, err_word);
  cc_scan_kernel<<<(unsigned)N, kThreads, 0, s>>>(chunk_count, chunk_base, cpi, counts);
  cc_rank_kernel<<<(unsigned)(N * cpi), kThreads, 0, s>>>(labels, HW, cpi, chunk_base);
  cc_final_kernel<<<runia_stream_grid(N * HW, kThreads), kThreads, 0, s>>>(labels, N * HW);
  if (runia_check_launch() != RUNIA_OK) return RUNIA_E_LAUNCH;
  unsigned err = 0;
  if (hipMemcpyAsync(&err, err_word, sizeof(err), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return RUNIA_E_LAUNCH;
  return err ? RUNIA_E_STEPCAP : RUNIA_OK;
}

extern "C" int runia_cc_overlap(const int32_t* gt_labels, const int32_t* gt_offsets, const int32_t* pred_labels,
                                const int32_t* pred_offsets, int64_t G, int64_t T, int64_t H, int64_t W, int64_t Kg,
                                int32_t* gt_size, int32_t* gt_inter, int32_t* pred_size, int32_t* pred_inter, int64_t* keys,
                                int64_t key_capacity, uint64_t* n_keys, int stats, runia_stream_t stream) {
  const int64_t lim = 0x7fffffffll;
  if (G < 0 || T < 0 || H < 0 || W < 0 || Kg < 0 || key_capacity < 0 || G > lim || T > lim || H > lim || W > lim || Kg > lim)
    return RUNIA_E_INVALID;
  const int64_t NI = pred_labels ? G * T : G, HW = H * W;
  if (NI == 0 || HW == 0) return RUNIA_OK;
  if (HW > lim || NI > lim / HW || (T > 0 && Kg > lim / T)) return RUNIA_E_INVALID;
  if (!gt_labels && !pred_labels) return RUNIA_E_INVALID;
  if ((gt_labels && !gt_offsets) || (pred_labels && !pred_offsets)) return RUNIA_E_INVALID;
  if (stats && ((pred_labels && !pred_size) || (gt_labels && pred_labels && (!gt_inter || !pred_inter)))) return RUNIA_E_INVALID;
  if (stats && gt_labels && !pred_labels && !gt_size) return RUNIA_E_INVALID;
  if (keys && (!n_keys || !gt_labels || !pred_labels)) return RUNIA_E_INVALID;
  OverlapArgs a;
  a.gt = gt_labels; a.gt_off = gt_offsets; a.pred = pred_labels; a.pred_off = pred_offsets;
  a.G = G; a.NI = NI; a.HW = HW; a.W = W; a.Kg = Kg;
  a.segs = (HW + kSeg - 1) / kSeg;
  a.items = NI * a.segs;
  a.cap = key_capacity;
  a.gt_size = gt_size; a.gt_inter = gt_inter; a.pred_size = pred_size; a.pred_inter = pred_inter;
  a.keys = reinterpret_cast<long long*>(keys);
  a.n_keys = (gt_labels && pred_labels) ? reinterpret_cast<unsigned long long*>(n_keys) : nullptr;
  a.stats = stats != 0;
  cc_overlap_kernel<<<runia_stream_grid(a.items, kThreads), kThreads, 0, as_stream(stream)>>>(a);
  return runia_check_launch();
}

extern "C" int runia_cc_relabel(int32_t* labels, const int32_t* offsets, const int32_t* map, int64_t N, int64_t H, int64_t W,
                                runia_stream_t stream) {
  const int64_t lim = 0x7fffffffll;
  if (N < 0 || H < 0 || W < 0 || N > lim || H > lim || W > lim) return RUNIA_E_INVALID;
  const int64_t HW = H * W;
  if (N == 0 || HW == 0) return RUNIA_OK;
  if (HW > lim || N > lim / HW || !labels || !offsets || !map) return RUNIA_E_INVALID;
  cc_relabel_kernel<<<runia_stream_grid(N * HW, kThreads), kThreads, 0, as_stream(stream)>>>(labels, offsets, map, HW, N * HW);
  return runia_check_launch();
}
