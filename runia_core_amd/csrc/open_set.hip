// Open-set object detection evaluation (reference evaluation/open_set.py: OpenSetEvaluator.process / evaluate, voc_eval,
// _compute_precision_recall, _get_unk_det_as_known, voc_ap, get_gtu_uu_per_class) for every method of a dataset at once.
//
//   quantize   float(f"{x:.pf}") of f32 / f64 / int inputs (the reference's format-and-parse round trip), optionally
//              after the +1 that process() adds to xmin and ymin in the box's own dtype; for the confidences also the
//              integer key k = x * 10^3 rounded half-to-even (the value is fl(k / 10^p) exactly)
//   bucket sort stable counting sort of int keys in [0, nb): per-chunk histograms, one scan, and a scatter in which one
//              wave walks its chunk in order and ranks equal keys with ballots (ties keep their input order)
//   overlaps   per detection (ovmax, first argmax) of the reference IoU against the ground truth of its label's group
//              and against the unknown ground truth: method-independent, computed once per dataset
//   match      per (method, sorted detection): relabelling, the confidence filter and the TP / FP / skip flags.  The greedy
//              match is order free: jmax does not depend on which boxes are taken, so a candidate (ovmax > t) is a TP
//              exactly when it is the earliest candidate of its (method, class, ground-truth slot).  That earliest
//              position is an integer minimum per slot; no float atomics, every result is reproducible bit for bit.
//   curves     one workgroup per (method, class) segment of the class partition: cumulative tp / fp / open-set fp,
//              rec, prec, the sentinel-envelope AP (or the 11-point VOC07 AP), the WI pair at recall 0.8 and the counts.
// The IoU keeps the reference's operation order in f64; the library builds with -ffp-contract=off, so nothing is fused.
#include "common.hpp"

#include <type_traits>

namespace {

enum { kF32 = 0, kF64 = 1, kI32 = 2, kI64 = 3 };

constexpr int kSortChunk = 4096;  // keys per histogram / scatter chunk
constexpr int kMaxBuckets = 8192; // LDS: one int per bucket
constexpr int kSummary = 8;       // doubles per (method, class) summary

// float(f"{x:.{p}f}") for a double x: k = x * 10^p rounded half-to-even from the exact product, then fl(k / 10^p).
// |x| 10^p >= 2^53 prints every digit of x, which parses back to x.  NaN / inf pass through, -0.0 keeps its sign.
__device__ __forceinline__ double quantize_one(double x, double s, long long* key) {
  const double y = x * s;
  if (!(__builtin_fabs(y) < 9007199254740992.0)) {  // NaN, inf and |x| 10^p >= 2^53
    *key = -1;
    return x;
  }
  double t = __builtin_rint(y);
  const double e = __builtin_fma(x, s, -y);  // exact x * s = y + e
  const double h = y - t;                    // exact (Sterbenz)
  if (h == 0.5 && e > 0.0) t += 1.0;
  else if (h == -0.5 && e < 0.0) t -= 1.0;
  *key = (long long)t;
  const double r = t / s;
  return r == 0.0 ? __builtin_copysign(0.0, x) : r;
}

template <typename T>
__global__ void quantize_kernel(const T* __restrict__ x, int64_t n, int period, unsigned add_one_mask, double scale,
                                double* __restrict__ out, int32_t* __restrict__ key_out, int key_max, int* __restrict__ bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    T v = x[i];
    if ((add_one_mask >> (int)(i % period)) & 1u) v = (T)(v + (T)1);  // the +1 of process(), in the input's dtype
    long long k;
    double q;
    if constexpr (std::is_integral<T>::value) {
      q = (double)v;  // an integer prints with zero decimals and parses back to the nearest double
      k = __builtin_fabs(q) * scale < 9007199254740992.0 ? (long long)v * (long long)scale : -1;
    } else {
      q = quantize_one((double)v, scale, &k);
    }
    out[i] = q;
    if (key_out) {
      // descending confidence -> ascending sort key; a confidence outside [0, 1] (or NaN) flags the call
      if (k < 0 || k > key_max) {
        atomicOr(bad, 1);
        key_out[i] = 0;
      } else {
        key_out[i] = key_max - (int)k;
      }
    }
  }
}

// ---- stable bucket sort -----------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) sort_hist_kernel(const int32_t* __restrict__ keys, int64_t n, int nb, int nchunks,
                                                        int32_t* __restrict__ counts) {
  __shared__ int h[kMaxBuckets];
  for (int b = threadIdx.x; b < nb; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * kSortChunk;
  const int64_t hi = lo + kSortChunk < n ? lo + kSortChunk : n;
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) atomicAdd(&h[keys[i]], 1);  // LDS integer counts
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += blockDim.x) counts[(int64_t)b * nchunks + blockIdx.x] = h[b];
}

// exclusive scan of the bucket-major counts in place (one workgroup); bucket_start[b] = first output slot of bucket b
__global__ void __launch_bounds__(1024) sort_scan_kernel(int32_t* __restrict__ counts, int64_t total, int nb, int nchunks,
                                                         int64_t* __restrict__ bucket_start) {
  __shared__ int64_t part[1024];
  const int64_t per = (total + blockDim.x - 1) / blockDim.x;
  const int64_t lo = threadIdx.x * per;
  const int64_t hi = lo + per < total ? lo + per : total;
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += counts[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < (int)blockDim.x; off <<= 1) {
    const int64_t v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (int64_t i = lo; i < hi; ++i) {
    const int32_t c = counts[i];
    counts[i] = (int32_t)run;
    if (i % nchunks == 0) bucket_start[i / nchunks] = run;
    run += c;
  }
  if (threadIdx.x == blockDim.x - 1) bucket_start[nb] = part[blockDim.x - 1];
}

// one wave per chunk, in input order: equal keys of a 64-key step are ranked by ballot, so ties keep their order
__global__ void __launch_bounds__(64) sort_scatter_kernel(const int32_t* __restrict__ keys, int64_t n, int nb, int nchunks,
                                                          const int32_t* __restrict__ offsets, int32_t* __restrict__ perm) {
  __shared__ int cursor[kMaxBuckets];
  const int lane = threadIdx.x;
  for (int b = lane; b < nb; b += 64) cursor[b] = offsets[(int64_t)b * nchunks + blockIdx.x];
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int64_t lo = (int64_t)blockIdx.x * kSortChunk;
  const int64_t hi = lo + kSortChunk < n ? lo + kSortChunk : n;
  for (int64_t base = lo; base < hi; base += 64) {
    const int64_t i = base + lane;
    const int key = i < hi ? keys[i] : -1;
    bool pending = i < hi;
    for (;;) {
      const unsigned long long act = __ballot(pending);
      if (act == 0ull) break;
      const int leader = __ffsll((long long)act) - 1;
      const int lk = __shfl(key, leader, 64);
      const bool mine = pending && key == lk;
      const unsigned long long same = __ballot(mine);
      const int start = cursor[lk];
      if (mine) {
        perm[start + __popcll(same & lt)] = (int32_t)i;
        pending = false;
      }
      __syncthreads();
      if (lane == leader) cursor[lk] = start + __popcll(same);
      __syncthreads();
    }
  }
}

// ---- overlaps -----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double np_max(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }
__device__ __forceinline__ double np_min(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }

// (ovmax, jmax) of _compute_overlaps + np.max / np.argmax over the ground truth [g0, g1); jmax is a global position
__device__ void overlap_max(const double* bb, const double* __restrict__ gt, int32_t g0, int32_t g1, double* ovmax,
                            int32_t* jmax) {
  double best = -__builtin_inf();
  int32_t arg = -1;
  bool seen_nan = false;
  for (int32_t j = g0; j < g1; ++j) {
    const double* g = gt + 4 * (int64_t)j;
    const double ixmin = np_max(g[0], bb[0]);
    const double iymin = np_max(g[1], bb[1]);
    const double ixmax = np_min(g[2], bb[2]);
    const double iymax = np_min(g[3], bb[3]);
    const double iw = np_max(ixmax - ixmin + 1.0, 0.0);
    const double ih = np_max(iymax - iymin + 1.0, 0.0);
    const double inters = iw * ih;
    const double uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (g[2] - g[0] + 1.0) * (g[3] - g[1] + 1.0) - inters;
    const double ov = inters / uni;
    if (seen_nan) continue;
    if (ov != ov) {  // np.max is NaN, np.argmax the first NaN
      seen_nan = true;
      best = ov;
      arg = j;
    } else if (arg < 0 || ov > best) {
      best = ov;
      arg = j;
    }
  }
  *ovmax = best;
  *jmax = arg;
}

__global__ void overlaps_kernel(const double* __restrict__ boxes, const int32_t* __restrict__ det_img,
                                const int32_t* __restrict__ det_group, int64_t n, const double* __restrict__ gt,
                                const int32_t* __restrict__ gt_off, int n_img, int n_groups, int unk_group,
                                double* __restrict__ ov, int32_t* __restrict__ jpos) {
  for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x) {
    const int img = det_img[d];
    double o0 = -__builtin_inf(), o1 = -__builtin_inf();
    int32_t j0 = -1, j1 = -1;
    if (img >= 0 && img < n_img) {
      double bb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) bb[k] = boxes[4 * d + k];
      const int g = det_group[d];
      if (g >= 0 && g < n_groups) {
        const int64_t c = (int64_t)g * n_img + img;
        overlap_max(bb, gt, gt_off[c], gt_off[c + 1], &o0, &j0);
      }
      if (unk_group >= 0 && unk_group < n_groups) {
        const int64_t c = (int64_t)unk_group * n_img + img;
        overlap_max(bb, gt, gt_off[c], gt_off[c + 1], &o1, &j1);
      }
    }
    ov[2 * d] = o0;
    ov[2 * d + 1] = o1;
    jpos[2 * d] = j0;
    jpos[2 * d + 1] = j1;
  }
}

// ---- match --------------------------------------------------------------------------------------------------------------

struct MatchArgs {
  const int32_t* perm;       // sorted position -> detection
  int64_t n;
  int n_methods, n_classes;  // classes = known + the unknown class (index n_classes - 1)
  const int32_t* label;
  const int32_t* det_img;
  const double* ov;
  const int32_t* jpos;
  const double* mscore;      // [M, n] raw method scores, exact in the comparison dtype
  const double* thr;         // [M] thresholds rounded to that dtype
  int open_set, unk_label;
  const double* conf;        // raw confidences in the filter's dtype, NULL: no filter
  double min_conf;
  const int32_t* group_of_class;
  const int32_t* gstart;     // first ground-truth position of each group
  const int64_t* cbase;      // first slot of each class
  int64_t n_slots;
  double ovthresh;
};

struct Row {
  int c;        // class after relabelling; n_classes: not evaluated for this method
  int annotated;
  int cand;     // ovmax > t in an annotated image
  int unk;      // overlap with the unknown ground truth > t
  int64_t slot;
};

__device__ __forceinline__ Row match_row(const MatchArgs& a, int m, int64_t p) {
  Row r;
  const int d = a.perm[p];
  const int K = a.n_classes - 1;
  const int lab = a.label[d];
  const bool relabel = a.open_set ? lab == a.unk_label : a.mscore[(int64_t)m * a.n + d] < a.thr[m];
  int c = relabel ? K : lab;
  if (c < 0 || c > K) c = a.n_classes;
  if (a.conf && !(a.conf[d] >= a.min_conf)) c = a.n_classes;
  r.c = c;
  r.annotated = a.det_img[d] >= 0;
  const int which = c == K ? 1 : 0;
  const double o = a.ov[2 * (int64_t)d + which];
  const int32_t j = a.jpos[2 * (int64_t)d + which];
  r.cand = c < a.n_classes && r.annotated && o > a.ovthresh && j >= 0;
  r.unk = r.annotated && a.ov[2 * (int64_t)d + 1] > a.ovthresh;
  r.slot = r.cand ? a.cbase[c] + (j - a.gstart[a.group_of_class[c]]) : -1;
  if (r.slot >= a.n_slots) r.slot = -1, r.cand = 0;
  return r;
}

__global__ void match_min_kernel(MatchArgs a, int32_t* __restrict__ key, int32_t* __restrict__ minpos) {
  const int64_t total = (int64_t)a.n_methods * a.n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / a.n);
    const int64_t p = i - (int64_t)m * a.n;
    const Row r = match_row(a, m, p);
    key[i] = m * (a.n_classes + 1) + r.c;
    if (r.cand) atomicMin(&minpos[(int64_t)m * a.n_slots + r.slot], (int)p);
  }
}

// flags: 1 TP, 2 FP (0: skipped, in an image without annotations), 4 open-set FP (overlaps unknown ground truth)
__global__ void match_flag_kernel(MatchArgs a, const int32_t* __restrict__ minpos, uint8_t* __restrict__ flags) {
  const int64_t total = (int64_t)a.n_methods * a.n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / a.n);
    const int64_t p = i - (int64_t)m * a.n;
    const Row r = match_row(a, m, p);
    uint8_t f = 0;
    if (r.annotated) f = (r.cand && minpos[(int64_t)m * a.n_slots + r.slot] == (int)p) ? 1 : 2;
    if (r.unk) f |= 4;
    flags[i] = f;
  }
}

// GTU / UU partition key of get_gtu_uu_per_class: class-major GTU, then class-major UU, then rows not evaluated
__global__ void gtu_key_kernel(const int32_t* __restrict__ key, const uint8_t* __restrict__ flags, int64_t n, int n_classes,
                               int32_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = key[i];
    out[i] = c >= n_classes ? 2 * n_classes : ((flags[i] & 4) ? c : n_classes + c);
  }
}

__global__ void gather_kernel(const double* __restrict__ src, const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx0,
                              int64_t n_src, int64_t n, double* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t j = idx0[i];
    if (idx1) j = idx1[j];
    out[i] = (j >= 0 && j < n_src) ? src[j] : __builtin_nan("");
  }
}

// ---- curves -------------------------------------------------------------------------------------------------------------

constexpr int kCurveThreads = 256;

struct I3 {
  int a, b, c;
};

__device__ __forceinline__ I3 operator+(I3 x, I3 y) { return I3{x.a + y.a, x.b + y.b, x.c + y.c}; }

// inclusive suffix max within the block (thread order reversed)
__device__ double block_suffix_max(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < kCurveThreads; o <<= 1) {
    const double x = threadIdx.x + o < kCurveThreads ? sh[threadIdx.x + o] : 0.0;
    __syncthreads();
    sh[threadIdx.x] = sh[threadIdx.x] > x ? sh[threadIdx.x] : x;
    __syncthreads();
  }
  const double r = sh[threadIdx.x];
  __syncthreads();
  return r;
}

__device__ double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = kCurveThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// summary per (method, class): ap, rec[-1], prec[-1], tp+fp and fp_os at the first argmin |rec - 0.8|, open-set FP count,
// max(tp+fp), number of rows
__global__ void __launch_bounds__(kCurveThreads) curves_kernel(
    const int32_t* __restrict__ part, const int64_t* __restrict__ bucket_start, const uint8_t* __restrict__ flags, int64_t n,
    int n_classes, const int64_t* __restrict__ npos, int use_07, double* __restrict__ summary, double* __restrict__ rec_out,
    double* __restrict__ prec_out, double* __restrict__ tpfp_out, double* __restrict__ fpos_out, double* __restrict__ ws_rec,
    double* __restrict__ ws_prec) {
  __shared__ I3 sh3[kCurveThreads / 64];
  __shared__ double shd[kCurveThreads];
  __shared__ double sh_wi[kCurveThreads];
  __shared__ long long sh_wi_i[kCurveThreads];
  __shared__ int sh_cnt[11];
  __shared__ double sh_p07[11];
  const int seg = blockIdx.x;  // m * (n_classes + 1) + c
  const int m = seg / (n_classes + 1), c = seg % (n_classes + 1);
  if (c == n_classes) return;  // rows not evaluated
  const int64_t lo = bucket_start[seg], hi = bucket_start[seg + 1];
  const int64_t nd = hi - lo;
  const double np_ = (double)npos[c];
  const double eps = 2.220446049250313e-16;
  if (threadIdx.x < 11) sh_cnt[threadIdx.x] = 0;
  __syncthreads();
  // forward: cumulative counts, rec, prec, WI argmin, counts of rec < t for the 11 VOC07 thresholds
  I3 carry = {0, 0, 0};
  double wi_best = __builtin_inf();
  long long wi_idx = -1;
  int lt07[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) lt07[k] = 0;
  for (int64_t t0 = 0; t0 < nd; t0 += kCurveThreads) {
    const int64_t r = t0 + threadIdx.x;
    I3 v = {0, 0, 0};
    if (r < nd) {
      const uint8_t f = flags[part[lo + r]];
      v.a = f & 1;
      v.b = (f >> 1) & 1;
      v.c = (f >> 2) & 1;
    }
    I3 tot;
    const I3 s = carry + block_scan_excl<kCurveThreads>(v, [](I3 x, I3 y) { return x + y; }, I3{0, 0, 0}, sh3, tot) + v;
    __syncthreads();  // (sh3 is free for the next trip)
    carry = carry + tot;
    if (r < nd) {
      const double tp = (double)s.a, fp = (double)s.b;
      const double rec = npos[c] > 0 ? tp / np_ : tp;
      const double tpfp = tp + fp;
      const double prec = tp / (tpfp > eps ? tpfp : eps);
      ws_rec[lo + r] = rec;
      ws_prec[lo + r] = prec;
      if (rec_out) {
        rec_out[lo + r] = rec;
        prec_out[lo + r] = prec;
        tpfp_out[lo + r] = tpfp;
        fpos_out[lo + r] = (double)s.c;
      }
      const double dist = __builtin_fabs(rec - 0.8);
      if (dist < wi_best) wi_best = dist, wi_idx = r;  // rows ascend per thread: the first wins
#pragma unroll
      for (int k = 0; k < 11; ++k) lt07[k] += rec < (double)k * 0.1;
    }
  }
  // first argmin over the block
  sh_wi[threadIdx.x] = wi_best;
  sh_wi_i[threadIdx.x] = wi_idx;
  __syncthreads();
  for (int o = kCurveThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double b = sh_wi[threadIdx.x + o];
      const long long bi = sh_wi_i[threadIdx.x + o];
      const long long ai = sh_wi_i[threadIdx.x];
      if (bi >= 0 && (ai < 0 || b < sh_wi[threadIdx.x] || (b == sh_wi[threadIdx.x] && bi < ai))) {
        sh_wi[threadIdx.x] = b;
        sh_wi_i[threadIdx.x] = bi;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 11; ++k) atomicAdd(&sh_cnt[k], lt07[k]);  // LDS integer counts
  __syncthreads();
  // backward: precision envelope (suffix max, sentinel 0), AP terms (delta rec) * envelope
  double run_max = 0.0, acc = 0.0;
  if (threadIdx.x < 11) sh_p07[threadIdx.x] = 0.0;
  __syncthreads();
  const int64_t ntiles = (nd + kCurveThreads - 1) / kCurveThreads;
  for (int64_t tile = ntiles - 1; tile >= 0; --tile) {
    const int64_t r = tile * kCurveThreads + threadIdx.x;
    const double pr = r < nd ? ws_prec[lo + r] : 0.0;
    double env = block_suffix_max(pr, shd);
    env = env > run_max ? env : run_max;
    if (threadIdx.x == 0) shd[0] = env;  // thread 0 holds the maximum of this tile and everything after it
    __syncthreads();
    const double tmax = shd[0];
    __syncthreads();
    if (r < nd) {
      const double rc = ws_rec[lo + r];
      const double prev = r > 0 ? ws_rec[lo + r - 1] : 0.0;
      if (rc != prev) acc += (rc - prev) * env;
#pragma unroll
      for (int k = 0; k < 11; ++k)
        if (sh_cnt[k] == r) sh_p07[k] = env;
    }
    run_max = tmax;
  }
  const double ap_sum = block_sum(acc, shd);
  __syncthreads();
  if (threadIdx.x == 0) {
    double ap;
    if (use_07) {
      ap = 0.0;
      for (int k = 0; k < 11; ++k) ap = ap + (sh_cnt[k] < nd ? sh_p07[k] : 0.0) / 11.0;
    } else {
      ap = ap_sum;  // the last sentinel term (1 - rec[-1]) * 0 adds nothing
    }
    double* o = summary + (int64_t)(m * n_classes + c) * kSummary;
    o[0] = ap;
    o[7] = (double)nd;
    o[5] = (double)carry.c;
    o[6] = (double)(carry.a + carry.b);
    if (nd > 0) {
      const double tp = (double)carry.a, fp = (double)carry.b;
      o[1] = npos[c] > 0 ? tp / np_ : tp;
      const double tpfp = tp + fp;
      o[2] = tp / (tpfp > eps ? tpfp : eps);
      const long long wi = sh_wi_i[0];
      // tp+fp and fp_os at row wi: read back from the stored curves
      o[3] = (double)wi;
      o[4] = 0.0;
    } else {
      o[1] = o[2] = o[3] = o[4] = 0.0;
    }
  }
}

// tp+fp and the open-set FP count at each segment's WI row (one thread per segment; the WI row index is in summary[3])
__global__ void wi_fill_kernel(const int32_t* __restrict__ part, const int64_t* __restrict__ bucket_start,
                               const uint8_t* __restrict__ flags, int n_segments, int n_classes, double* __restrict__ summary) {
  // counts up to the WI row: one workgroup per segment, strided sum in a fixed order
  __shared__ int sa[kCurveThreads], sb[kCurveThreads];
  const int seg = blockIdx.x;
  const int m = seg / (n_classes + 1), c = seg % (n_classes + 1);
  if (seg >= n_segments || c == n_classes) return;
  double* o = summary + (int64_t)(m * n_classes + c) * kSummary;
  const int64_t lo = bucket_start[seg], nd = bucket_start[seg + 1] - lo;
  if (nd <= 0) return;
  const int64_t wi = (int64_t)o[3];
  int a = 0, b = 0;
  for (int64_t r = threadIdx.x; r <= wi; r += blockDim.x) {
    const uint8_t f = flags[part[lo + r]];
    a += (f & 3) != 0;
    b += (f >> 2) & 1;
  }
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sa[threadIdx.x] += sa[threadIdx.x + s], sb[threadIdx.x] += sb[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    o[3] = (double)sa[0];
    o[4] = (double)sb[0];
  }
}

int64_t sort_chunks(int64_t n) { return (n + kSortChunk - 1) / kSortChunk; }

}  // namespace

extern "C" int runia_osod_quantize(const void* x, int dtype, int64_t n, int period, unsigned add_one_mask, int decimals,
                                   double* out, int32_t* key_out, int key_max, int32_t* bad, runia_stream_t stream) {
  if (n < 0 || n > 0x7fffffffll || period < 1 || period > 32 || decimals < 0 || decimals > 15 || dtype < kF32 || dtype > kI64)
    return RUNIA_E_INVALID;
  if (n == 0) return RUNIA_OK;
  if (!x || !out || (key_out && (!bad || key_max < 0))) return RUNIA_E_INVALID;
  double s = 1.0;
  for (int i = 0; i < decimals; ++i) s *= 10.0;
  const hipStream_t st = as_stream(stream);
  const unsigned grid = runia_stream_grid(n, 256);
  switch (dtype) {
    case kF32: quantize_kernel<float><<<grid, 256, 0, st>>>((const float*)x, n, period, add_one_mask, s, out, key_out, key_max, bad); break;
    case kF64: quantize_kernel<double><<<grid, 256, 0, st>>>((const double*)x, n, period, add_one_mask, s, out, key_out, key_max, bad); break;
    case kI32: quantize_kernel<int32_t><<<grid, 256, 0, st>>>((const int32_t*)x, n, period, add_one_mask, s, out, key_out, key_max, bad); break;
    default: quantize_kernel<int64_t><<<grid, 256, 0, st>>>((const int64_t*)x, n, period, add_one_mask, s, out, key_out, key_max, bad); break;
  }
  return runia_check_launch();
}

extern "C" size_t runia_osod_sort_workspace_bytes(int64_t n, int nb) {
  if (n < 0 || n > 0x7fffffffll || nb < 1 || nb > kMaxBuckets) return 0;
  const int64_t e = (int64_t)nb * sort_chunks(n > 0 ? n : 1);
  return round_up((size_t)e * 4, 16);
}

extern "C" int runia_osod_bucket_sort(const int32_t* keys, int64_t n, int nb, int32_t* perm, int64_t* bucket_start,
                                      void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (n < 0 || n > 0x7fffffffll || nb < 1 || nb > kMaxBuckets || !bucket_start || (n > 0 && (!keys || !perm)))
    return RUNIA_E_INVALID;
  const size_t need = runia_osod_sort_workspace_bytes(n, nb);
  if (ws_refused(workspace, workspace_bytes, need, 1)) return RUNIA_E_WORKSPACE;
  const hipStream_t st = as_stream(stream);
  const int nch = (int)sort_chunks(n > 0 ? n : 1);
  int32_t* counts = reinterpret_cast<int32_t*>(workspace);
  // keys must lie in [0, nb): the histogram indexes LDS with them, so the caller's keys are trusted (the wrappers make them)
  sort_hist_kernel<<<nch, 256, 0, st>>>(keys, n, nb, nch, counts);
  sort_scan_kernel<<<1, 1024, 0, st>>>(counts, (int64_t)nb * nch, nb, nch, bucket_start);
  if (n > 0) sort_scatter_kernel<<<nch, 64, 0, st>>>(keys, n, nb, nch, counts, perm);
  return runia_check_launch();
}

extern "C" int runia_osod_overlaps(const double* boxes, const int32_t* det_img, const int32_t* det_group, int64_t n,
                                   const double* gt_boxes, const int32_t* gt_off, int n_img, int n_groups, int unk_group,
                                   double* ov, int32_t* jpos, runia_stream_t stream) {
  if (n < 0 || n > 0x7fffffffll || n_img < 0 || n_groups < 0 || !gt_off) return RUNIA_E_INVALID;
  if (n == 0) return RUNIA_OK;
  if (!boxes || !det_img || !det_group || !ov || !jpos) return RUNIA_E_INVALID;
  overlaps_kernel<<<runia_stream_grid(n, 256), 256, 0, as_stream(stream)>>>(boxes, det_img, det_group, n, gt_boxes, gt_off,
                                                                           n_img, n_groups, unk_group, ov, jpos);
  return runia_check_launch();
}

extern "C" size_t runia_osod_match_workspace_bytes(int n_methods, int64_t n_slots) {
  if (n_methods < 1 || n_slots < 0) return 0;
  return round_up((size_t)((int64_t)n_methods * (n_slots > 0 ? n_slots : 1)) * 4, 16);
}

extern "C" int runia_osod_match(const int32_t* perm, int64_t n, int n_methods, int n_classes, const int32_t* label,
                                const int32_t* det_img, const double* ov, const int32_t* jpos, const double* mscore,
                                const double* thr, int open_set, int unk_label, const double* conf, double min_conf,
                                const int32_t* group_of_class, const int32_t* gstart, const int64_t* cbase, int64_t n_slots,
                                double ovthresh, int32_t* key, uint8_t* flags, void* workspace, size_t workspace_bytes,
                                runia_stream_t stream) {
  if (n < 0 || n_methods < 1 || n_classes < 1 || n_slots < 0 || (int64_t)n_methods * n > 0x7fffffffll ||
      (int64_t)n_methods * (n_classes + 1) > kMaxBuckets)
    return RUNIA_E_INVALID;
  if (n == 0) return RUNIA_OK;
  if (!perm || !label || !det_img || !ov || !jpos || !group_of_class || !gstart || !cbase || !key || !flags) return RUNIA_E_INVALID;
  if (!open_set && (!mscore || !thr)) return RUNIA_E_INVALID;
  const size_t need = runia_osod_match_workspace_bytes(n_methods, n_slots);
  if (ws_refused(workspace, workspace_bytes, need, 1)) return RUNIA_E_WORKSPACE;
  const hipStream_t st = as_stream(stream);
  int32_t* minpos = reinterpret_cast<int32_t*>(workspace);
  if (hipMemsetAsync(minpos, 0x7f, need, st) != hipSuccess) return RUNIA_E_LAUNCH;
  MatchArgs a{perm, n, n_methods, n_classes, label, det_img, ov, jpos, mscore, thr, open_set, unk_label, conf, min_conf,
              group_of_class, gstart, cbase, n_slots, ovthresh};
  const int64_t total = (int64_t)n_methods * n;
  match_min_kernel<<<runia_stream_grid(total, 256), 256, 0, st>>>(a, key, minpos);
  match_flag_kernel<<<runia_stream_grid(total, 256), 256, 0, st>>>(a, minpos, flags);
  return runia_check_launch();
}

extern "C" int runia_osod_gtu_keys(const int32_t* key, const uint8_t* flags, int64_t n, int n_classes, int32_t* out,
                                   runia_stream_t stream) {
  if (n < 0 || n > 0x7fffffffll || n_classes < 1 || 2 * n_classes + 1 > kMaxBuckets) return RUNIA_E_INVALID;
  if (n == 0) return RUNIA_OK;
  if (!key || !flags || !out) return RUNIA_E_INVALID;
  gtu_key_kernel<<<runia_stream_grid(n, 256), 256, 0, as_stream(stream)>>>(key, flags, n, n_classes, out);
  return runia_check_launch();
}

extern "C" int runia_osod_gather_f64(const double* src, int64_t n_src, const int32_t* idx0, const int32_t* idx1, int64_t n,
                                     double* out, runia_stream_t stream) {
  if (n < 0 || n > 0x7fffffffll || n_src < 0) return RUNIA_E_INVALID;
  if (n == 0) return RUNIA_OK;
  if (!src || !idx0 || !out) return RUNIA_E_INVALID;
  gather_kernel<<<runia_stream_grid(n, 256), 256, 0, as_stream(stream)>>>(src, idx1, idx0, n_src, n, out);
  return runia_check_launch();
}

extern "C" size_t runia_osod_curves_workspace_bytes(int64_t rows) {
  if (rows < 0 || rows > 0x7fffffffll) return 0;
  return (size_t)(2 * (rows > 0 ? rows : 1) * 8);
}

extern "C" int runia_osod_curves(const int32_t* part, const int64_t* bucket_start, const uint8_t* flags, int64_t n,
                                 int n_methods, int n_classes, const int64_t* npos, int use_07, double* summary, double* rec,
                                 double* prec, double* tpfp, double* fpos, void* workspace, size_t workspace_bytes,
                                 runia_stream_t stream) {
  const int64_t rows = (int64_t)n_methods * n;
  if (n < 0 || n_methods < 1 || n_classes < 1 || rows > 0x7fffffffll || (int64_t)n_methods * (n_classes + 1) > kMaxBuckets)
    return RUNIA_E_INVALID;
  if (!bucket_start || !npos || !summary || (n > 0 && (!part || !flags))) return RUNIA_E_INVALID;
  if (rec && (!prec || !tpfp || !fpos)) return RUNIA_E_INVALID;
  const size_t need = runia_osod_curves_workspace_bytes(rows);
  if (ws_refused(workspace, workspace_bytes, need, 1)) return RUNIA_E_WORKSPACE;
  double* ws = reinterpret_cast<double*>(workspace);
  const int segs = n_methods * (n_classes + 1);
  const hipStream_t st = as_stream(stream);
  curves_kernel<<<segs, kCurveThreads, 0, st>>>(part, bucket_start, flags, n, n_classes, npos, use_07, summary, rec, prec,
                                                tpfp, fpos, ws, ws + (rows > 0 ? rows : 1));
  wi_fill_kernel<<<segs, kCurveThreads, 0, st>>>(part, bucket_start, flags, segs, n_classes, summary);
  return runia_check_launch();
}
