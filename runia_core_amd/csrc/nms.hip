// Greedy non-maximum suppression on the device (torchvision.ops.nms, which the reference calls from
// ObjectDetectionExtractor.yolo_get_logits, feature_extraction/abstract_classes.py:606-715), and the YOLOv8 candidate
// filter in front of it.  No torchvision on this platform: this is the only implementation.
//
//   runia_yolo_candidates_f32  per anchor of one image's head (4 + nc + nm, A): best class score and first best index,
//                              candidate test, then an in-order compaction (per-block counts, exclusive scan by every
//                              block over the counts before it, wave ballots inside the block: no atomics, the order is
//                              the anchor order whatever the timing);
//   runia_nms_keys_f32         sort keys (descending score, ascending index) as int64;
//   runia_nms_sort_keys        bitonic sort of up to RUNIA_NMS_SORT_MAX keys in one workgroup's LDS (the caller sorts
//                              longer lists with a device sort of the same keys: the keys are distinct, so every correct
//                              sort gives the same order);
//   runia_nms_sorted_f32       IoU bitmask over upper-triangular 64 x 64 tiles, then the greedy walk in ONE workgroup
//                              with the "removed" bitmap in LDS.  Only the kept count ever needs to reach the host.
#include "common.hpp"

namespace {

constexpr int kCandThreads = 256;  // anchors per workgroup of the candidate kernels (4 waves)
constexpr int kSortThreads = 1024;
constexpr int kWalkThreads = 256;

__device__ __forceinline__ int64_t key_index(int64_t key) { return key & 0x7fffffff; }

// ---- YOLOv8 candidates -------------------------------------------------------------------------------------------------
// pass 1: best class per anchor -> cls_ws[a] (class index, or -1 when the anchor is no candidate), score_ws[a], and the
// candidate count of every workgroup -> counts[blockIdx.x]
__global__ void __launch_bounds__(kCandThreads) yolo_best_class_kernel(
    const float* __restrict__ pred, int64_t A, int nc, float conf_thres, const float* __restrict__ classes, int n_classes,
    int* __restrict__ cls_ws, float* __restrict__ score_ws, int* __restrict__ counts) {
  __shared__ int wave_counts[kCandThreads / RUNIA_WAVE];
  const int64_t a = (int64_t)blockIdx.x * kCandThreads + threadIdx.x;
  bool cand = false;
  if (a < A) {
    const float* col = pred + 4 * A + a;  // class row 0 of this anchor; rows are A apart (channel-major)
    float best = col[0];
    int j = 0;
    bool has_nan = best != best;
    for (int c = 1; c < nc; ++c) {
      const float v = col[(int64_t)c * A];
      if (v != v) has_nan = true;
      else if (v > best) { best = v; j = c; }
    }
    // torch.amax propagates a NaN and `NaN > thr` is false: such an anchor is dropped
    cand = !has_nan && best > conf_thres;
    if (cand && classes != nullptr) {
      bool in = false;
      for (int q = 0; q < n_classes; ++q) in |= ((float)j == classes[q]);
      cand = in;
    }
    cls_ws[a] = cand ? j : -1;
    score_ws[a] = best;
  }
  const uint64_t m = __ballot(cand);
  const int wave = threadIdx.x / RUNIA_WAVE, lane = threadIdx.x % RUNIA_WAVE;
  if (lane == 0) wave_counts[wave] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kCandThreads / RUNIA_WAVE; ++w) s += wave_counts[w];
    counts[blockIdx.x] = s;
  }
}

// pass 2: every workgroup adds the counts of the workgroups before it, then writes its candidates in anchor order:
// boxes (rows 0-3 as they are, plus the class offset cls * max_wh in f32), score, anchor, class.  The last workgroup
// writes the total.
__global__ void __launch_bounds__(kCandThreads) yolo_compact_kernel(
    const float* __restrict__ pred, int64_t A, float max_wh, const int* __restrict__ cls_ws,
    const float* __restrict__ score_ws, const int* __restrict__ counts, float* __restrict__ cand_boxes,
    float* __restrict__ cand_scores, int* __restrict__ cand_anchor, int* __restrict__ cand_cls, int64_t* __restrict__ count) {
  __shared__ int64_t partial[kCandThreads];
  __shared__ int wave_counts[kCandThreads / RUNIA_WAVE];
  const int tid = threadIdx.x;
  int64_t s = 0;
  for (int64_t b = tid; b < (int64_t)blockIdx.x; b += kCandThreads) s += counts[b];
  partial[tid] = s;
  __syncthreads();
  for (int h = kCandThreads / 2; h > 0; h >>= 1) {
    if (tid < h) partial[tid] += partial[tid + h];
    __syncthreads();
  }
  const int64_t base = partial[0];
  const int64_t a = (int64_t)blockIdx.x * kCandThreads + tid;
  const int j = a < A ? cls_ws[a] : -1;
  const bool cand = j >= 0;
  const uint64_t m = __ballot(cand);
  const int wave = tid / RUNIA_WAVE, lane = tid % RUNIA_WAVE;
  if (lane == 0) wave_counts[wave] = __popcll(m);
  __syncthreads();
  int off = 0;
  for (int w = 0; w < wave; ++w) off += wave_counts[w];
  off += __popcll(m & ((1ull << lane) - 1ull));
  if (cand) {
    const int64_t k = base + off;
    const float c = (float)j * max_wh;
    cand_boxes[4 * k + 0] = pred[0 * A + a] + c;
    cand_boxes[4 * k + 1] = pred[1 * A + a] + c;
    cand_boxes[4 * k + 2] = pred[2 * A + a] + c;
    cand_boxes[4 * k + 3] = pred[3 * A + a] + c;
    cand_scores[k] = score_ws[a];
    cand_anchor[k] = (int)a;
    cand_cls[k] = j;
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    int total = 0;
    for (int w = 0; w < kCandThreads / RUNIA_WAVE; ++w) total += wave_counts[w];
    *count = base + total;
  }
}

// ---- sort keys ---------------------------------------------------------------------------------------------------------
__global__ void nms_keys_kernel(const float* __restrict__ scores, int64_t n, int64_t* __restrict__ keys) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    // larger score, smaller key; -0 on +0 (equal for torch.sort as well).  Every NaN - either sign, any payload - takes the one
    // key 0, in front of +inf's (no other value has it: it is desc_key of the all-ones NaN alone), so the index orders the NaNs
    // among themselves: torch.sort(descending=True, stable=True).  By its bits a sign-set NaN would come last, behind -inf.
    const float v = scores[i];
    keys[i] = ((int64_t)(v != v ? 0u : desc_key(fold_zero(v))) << 31) | i;
  }
}

// bitonic sort of n <= RUNIA_NMS_SORT_MAX keys in LDS, padded to a power of two with INT64_MAX (above every key)
__global__ void __launch_bounds__(kSortThreads) nms_sort_small_kernel(int64_t* __restrict__ keys, int n, int p) {
  __shared__ int64_t s[RUNIA_NMS_SORT_MAX];
  for (int i = threadIdx.x; i < p; i += kSortThreads) s[i] = i < n ? keys[i] : INT64_MAX;
  __syncthreads();
  lds_bitonic_sort(s, p, (int)threadIdx.x, kSortThreads);
  for (int i = threadIdx.x; i < n; i += kSortThreads) keys[i] = s[i];
}

// ---- IoU bitmask ---------------------------------------------------------------------------------------------------------
// One wave per (row block, column block >= row block).  Lane l holds row box rb * 64 + l; the tile's 64 column boxes sit in
// LDS.  Bit c of mask[row * nb + cb] is set when IoU(row, cb * 64 + c) > thr, for columns after the row only (the walk never
// reads the others).  torchvision's expression, f32, in its order; 0/0 is NaN and compares false.
__global__ void __launch_bounds__(RUNIA_WAVE) nms_mask_kernel(const float* __restrict__ boxes,
                                                             const int64_t* __restrict__ keys, int64_t m, int nb, float thr,
                                                             uint64_t* __restrict__ mask) {
  const int cb = blockIdx.x, rb = blockIdx.y;
  if (cb < rb) return;
  __shared__ float cbox[RUNIA_WAVE][4];
  const int lane = threadIdx.x;
  const int64_t col = (int64_t)cb * RUNIA_WAVE + lane;
  if (col < m) {
    const int64_t bi = key_index(keys[col]);
    cbox[lane][0] = boxes[4 * bi + 0];
    cbox[lane][1] = boxes[4 * bi + 1];
    cbox[lane][2] = boxes[4 * bi + 2];
    cbox[lane][3] = boxes[4 * bi + 3];
  }
  __syncthreads();
  const int64_t row = (int64_t)rb * RUNIA_WAVE + lane;
  if (row >= m) return;
  const int64_t ri = key_index(keys[row]);
  const float a0 = boxes[4 * ri + 0], a1 = boxes[4 * ri + 1], a2 = boxes[4 * ri + 2], a3 = boxes[4 * ri + 3];
  const float sa = (a2 - a0) * (a3 - a1);
  const int ncols = (int)min<int64_t>(RUNIA_WAVE, m - (int64_t)cb * RUNIA_WAVE);
  const int c0 = cb == rb ? lane + 1 : 0;
  uint64_t bits = 0;
  for (int c = c0; c < ncols; ++c) {
    const float b0 = cbox[c][0], b1 = cbox[c][1], b2 = cbox[c][2], b3 = cbox[c][3];
    const float left = a0 > b0 ? a0 : b0, right = a2 < b2 ? a2 : b2;
    const float top = a1 > b1 ? a1 : b1, bottom = a3 < b3 ? a3 : b3;
    float w = right - left, h = bottom - top;
    w = w < 0.f ? 0.f : w;  // std::max(w, 0): a NaN stays NaN
    h = h < 0.f ? 0.f : h;
    const float inter = w * h;
    const float sb = (b2 - b0) * (b3 - b1);
    if (inter / (sa + sb - inter) > thr) bits |= 1ull << c;
  }
  mask[row * nb + cb] = bits;
}

// ---- greedy walk ---------------------------------------------------------------------------------------------------------
// One workgroup.  Per column block b: wave 0 resolves the block's 64 boxes from the removed word and the diagonal tile
// (register reads, no memory latency inside the block), then all threads OR the rows of the boxes kept in b into the removed
// words of the later blocks (independent loads, one pass per block).  Stops after max_det kept boxes.
__global__ void __launch_bounds__(kWalkThreads) nms_walk_kernel(const uint64_t* __restrict__ mask,
                                                               const int64_t* __restrict__ keys, int64_t m, int nb,
                                                               int64_t max_det, int64_t* __restrict__ keep,
                                                               int64_t* __restrict__ count) {
  __shared__ uint64_t removed[RUNIA_NMS_MAX_BOXES / RUNIA_WAVE];
  __shared__ int kept_rows[RUNIA_WAVE];
  __shared__ int n_kept;
  const int tid = threadIdx.x;
  for (int b = tid; b < nb; b += kWalkThreads) removed[b] = 0;
  __syncthreads();
  int64_t cnt = 0;
  for (int b = 0; b < nb && cnt < max_det; ++b) {
    const int rows = (int)min<int64_t>(RUNIA_WAVE, m - (int64_t)b * RUNIA_WAVE);
    if (tid < RUNIA_WAVE) {
      const uint64_t d = tid < rows ? mask[((int64_t)b * RUNIA_WAVE + tid) * nb + b] : 0ull;
      const uint32_t dlo = (uint32_t)d, dhi = (uint32_t)(d >> 32);
      uint64_t r = removed[b];
      int k = 0;
      for (int t = 0; t < rows && cnt + k < max_det; ++t) {
        if (!((r >> t) & 1ull)) {
          if (tid == 0) kept_rows[k] = t;
          ++k;
          const uint32_t lo = __builtin_amdgcn_readlane(dlo, t), hi = __builtin_amdgcn_readlane(dhi, t);
          r |= ((uint64_t)hi << 32) | lo;
        }
      }
      if (tid == 0) n_kept = k;
    }
    __syncthreads();
    const int k = n_kept;
    if (tid < k) keep[cnt + tid] = key_index(keys[(int64_t)b * RUNIA_WAVE + kept_rows[tid]]);
    cnt += k;
    if (cnt < max_det) {
      for (int cb = b + 1 + tid; cb < nb; cb += kWalkThreads) {
        uint64_t acc = 0;
        for (int q = 0; q < k; ++q) acc |= mask[((int64_t)b * RUNIA_WAVE + kept_rows[q]) * nb + cb];
        removed[cb] |= acc;
      }
    }
    __syncthreads();
  }
  if (tid == 0) *count = cnt;
}

}  // namespace

struct CandPlan { int* cls; float* score; int* counts; int64_t blocks; };  // best class and score per anchor | count per workgroup
static CandPlan cand_plan(WsWalk& w, int64_t A) {
  CandPlan p;
  p.blocks = (A + kCandThreads - 1) / kCandThreads;
  p.cls = w.take<int>(A);
  p.score = w.take<float>(A);
  p.counts = w.take<int>(p.blocks);
  return p;
}
extern "C" size_t runia_yolo_candidates_workspace_bytes(int64_t A) {
  if (A <= 0) return 0;
  return ws_bytes([&](WsWalk& w) { cand_plan(w, A); });
}

extern "C" int runia_yolo_candidates_f32(const float* pred, int64_t A, int nc, int nm, float conf_thres,
                                         const float* classes, int n_classes, float max_wh, float* cand_boxes,
                                         float* cand_scores, int* cand_anchor, int* cand_cls, int64_t* count,
                                         void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (!pred || !cand_boxes || !cand_scores || !cand_anchor || !cand_cls || !count || A <= 0 || A > RUNIA_YOLO_MAX_ANCHORS || nc < 1 ||
      nm < 0 || n_classes < 0 || (n_classes > 0 && !classes))
    return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const CandPlan plan = cand_plan(w, A);
  if (ws_refused(workspace, workspace_bytes, w.used(), 1)) return RUNIA_E_WORKSPACE;
  const int64_t blocks = plan.blocks;
  int *cls_ws = plan.cls, *counts = plan.counts;
  float* score_ws = plan.score;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(yolo_best_class_kernel, dim3((unsigned)blocks), dim3(kCandThreads), 0, s, pred, A, nc, conf_thres,
                     n_classes > 0 ? classes : nullptr, n_classes, cls_ws, score_ws, counts);
  hipLaunchKernelGGL(yolo_compact_kernel, dim3((unsigned)blocks), dim3(kCandThreads), 0, s, pred, A, max_wh, cls_ws, score_ws,
                     counts, cand_boxes, cand_scores, cand_anchor, cand_cls, count);
  return runia_check_launch();
}

extern "C" int runia_nms_keys_f32(const float* scores, int64_t n, int64_t* keys, runia_stream_t stream) {
  if (n < 0 || n > 0x7fffffffll || (n > 0 && (!scores || !keys))) return RUNIA_E_INVALID;
  if (n == 0) return RUNIA_OK;
  hipLaunchKernelGGL(nms_keys_kernel, dim3(runia_stream_grid(n, 256)), dim3(256), 0, as_stream(stream), scores, n, keys);
  return runia_check_launch();
}

extern "C" int runia_nms_sort_keys(int64_t* keys, int64_t n, runia_stream_t stream) {
  if (n < 0 || n > RUNIA_NMS_SORT_MAX || (n > 0 && !keys)) return RUNIA_E_INVALID;
  if (n <= 1) return RUNIA_OK;
  int p = 1;
  while (p < n) p <<= 1;
  hipLaunchKernelGGL(nms_sort_small_kernel, dim3(1), dim3(kSortThreads), 0, as_stream(stream), keys, (int)n, p);
  return runia_check_launch();
}

extern "C" size_t runia_nms_workspace_bytes(int64_t m) {
  if (m <= 0) return 0;
  const int64_t nb = (m + RUNIA_WAVE - 1) / RUNIA_WAVE;
  return (size_t)(m * nb * 8);
}

extern "C" int runia_nms_sorted_f32(const float* boxes, const int64_t* sorted_keys, int64_t m, float iou_threshold,
                                    int64_t max_det, int64_t* keep, int64_t* count, void* workspace, size_t workspace_bytes,
                                    runia_stream_t stream) {
  if (m < 0 || m > RUNIA_NMS_MAX_BOXES || max_det < 0 || !count || (m > 0 && (!boxes || !sorted_keys || !keep)))
    return RUNIA_E_INVALID;
  if (m > 0 && ws_refused(workspace, workspace_bytes, runia_nms_workspace_bytes(m), 1)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  const int nb = (int)((m + RUNIA_WAVE - 1) / RUNIA_WAVE);
  uint64_t* mask = reinterpret_cast<uint64_t*>(workspace);
  if (m > 0 && max_det > 0)
    hipLaunchKernelGGL(nms_mask_kernel, dim3(nb, nb), dim3(RUNIA_WAVE), 0, s, boxes, sorted_keys, m, nb, iou_threshold, mask);
  hipLaunchKernelGGL(nms_walk_kernel, dim3(1), dim3(kWalkThreads), 0, s, mask, sorted_keys, m, nb, max_det, keep, count);
  return runia_check_launch();
}
