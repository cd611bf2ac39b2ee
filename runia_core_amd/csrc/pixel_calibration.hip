// Calibration of a segmentation head from its (G, C, H, W) logits read where the model left them, and (G, H, W) labels:
//   runia_pixel_calib_accumulate  ONE pass over the logits at a temperature 1 / beta that ADDS into a small device record:
//                                 n_used / n_correct / n_bad, the f64 sums of nll, brier, g, h (the Newton step of the
//                                 temperature fit), the top-label reliability table, the per-class support / predicted / hit
//                                 counters (pixel accuracy, IoU) and, when asked for, the class-wise reliability table
//                                 (class-wise ECE); optionally the per-pixel conf and pred maps.  No per-pixel row table.
// The arithmetic of a pixel is the row arithmetic of calibration.hip (calib_core.hpp): the maximum and first argmax in
// ascending class order, then the four sums in ascending class order under that maximum, all inside one lane.
//
// In NCHW the classes of a pixel are H * W elements apart.  Load forms (pixel_map.hpp's view and rules), one per launch:
//   kLoadVec    w has unit stride, every other stride and the base a multiple of four elements, the (joined) row a multiple
//               of four pixels: a lane owns four neighbouring pixels of a class plane (16- / 8-byte loads) and walks the planes
//   kLoadCLast  the classes have unit stride (channels_last): a lane owns one pixel and walks its contiguous classes
//   kLoadElem   anything else (crops, odd bases, row tails): a lane owns one pixel, element loads through the strides
// Two kernels, picked on the host from C:
//   register form, C <= 24 (Cityscapes 19, VOC 21): the C logits of a lane's pixels stay in registers; every logit is read once
//   general form, any C <= 1024: the planes are walked twice (maximum, then the sums under it) and a third time for the
//               class-wise table; the re-reads come from the caches (a workgroup returns to a line after C loads)
//
// Determinism.  Counts are integers: LDS integer atomics per workgroup, flushed with global integer atomics into a zeroed
// table in the workspace.  The conf sums of the two reliability tables are kept as integer multiples of 2^-30 (a confidence
// rounds to the nearest multiple: at most 2^-31 off, 60 times below the f32 resolution of a confidence near 1; a uint64
// holds 2^34 pixels) and take the same route.  The four float sums are f64: per lane in item order, a fixed tree over the
// lanes, the waves in order, one partial per workgroup; the final kernel adds the partials in a fixed order and then adds
// everything into the record, one thread per slot.  No floating-point atomics: the same calls give the same bits.
#include "common.hpp"
#include "elem.hpp"
#include "calib_core.hpp"
#include "pixel_map.hpp"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kRegC = 24;                  // widest head of the register form
constexpr int kItemsPerThread = 2;         // lane items of a workgroup's range, per thread, while the grid is below its cap
constexpr int kMaxBlocks = 2048;
constexpr int kMaxBins = RUNIA_PIXCAL_MAX_BINS, kMaxClasswise = RUNIA_PIXCAL_MAX_CLASSWISE;
constexpr int kHead = RUNIA_PIXCAL_HEAD_SLOTS;
constexpr int kTabHead = 4;                // n_used, n_correct, n_bad, n_nan of the workspace table
constexpr int64_t kMaxPixels = (int64_t)1 << 34;
constexpr float kFix = 1073741824.f;       // 2^30
enum { kLabI64 = 0, kLabI32 = 1, kLabU8 = 2 };
enum { kModeHead = RUNIA_PIXCAL_MODE_HEAD, kModeTop = RUNIA_PIXCAL_MODE_TOP, kModeClasswise = RUNIA_PIXCAL_MODE_CLASSWISE };

struct CalArgs {
  MapView v;
  const void* lab;
  int lab_code, has_ignore;
  int64_t ignore;
  float beta;
  int n_bins, mode;          // n_bins: 0 in the head-only mode
  int64_t items, items_per_block;
  float* conf_map;
  int32_t* pred_map;
  int vec_store;             // both maps (where given) are 16-byte aligned
  double* part;              // [blocks][4] sums of nll, brier, g, h
  unsigned long long* tab;   // the integer table (zeroed): head | top-label | per-class | class-wise
};

__device__ __forceinline__ int64_t load_label(const void* lab, int code, int64_t p) {
  if (code == kLabI64) return static_cast<const int64_t*>(lab)[p];
  if (code == kLabI32) return static_cast<const int32_t*>(lab)[p];
  return static_cast<const uint8_t*>(lab)[p];
}

// a probability as a multiple of 2^-30 (0 for a NaN: those pixels are counted apart)
__device__ __forceinline__ unsigned long long fix30(float p) {
  return (p == p) ? (unsigned long long)rintf(p * kFix) : 0ull;
}

// The tables of one workgroup in LDS: 64-bit sums first, then 32-bit counts (a workgroup scores fewer than 2^32 pixels).
struct Tables {
  unsigned long long *top_conf, *cw_conf;
  unsigned *head, *top_cnt, *top_cor, *sup, *prd, *hit, *cw_cnt, *cw_pos;
  int nb, C, E;  // bins of the top-label table, classes of the counters, entries of the class-wise table (0: not kept)
};

__host__ __device__ inline void table_sizes(int mode, int C, int n_bins, int& nb, int& Cc, int& E) {
  nb = mode >= kModeTop ? n_bins : 0;
  Cc = mode >= kModeTop ? C : 0;
  E = mode == kModeClasswise ? C * n_bins : 0;
}
__host__ __device__ inline size_t lds_bytes(int nb, int Cc, int E) {
  return (size_t)(nb + E) * 8 + (size_t)(kTabHead + 2 * nb + 3 * Cc + 2 * E) * 4;
}

// Neighbouring pixels mostly share their class and their confidence bin, and every lane of a wave would then add to the
// same LDS word: a lane merges what it has for one table entry and adds when the entry changes (and at the end).
struct TopRun {  // the top-label table
  int b;
  unsigned cnt, cor;
  unsigned long long conf;
};
struct ClsRun {  // the per-class counters
  int y, pred;
  unsigned n;
};

__device__ __forceinline__ void flush_run(const Tables& t, TopRun& r) {
  if (r.cnt) {
    atomicAdd(&t.top_cnt[r.b], r.cnt);
    if (r.cor) atomicAdd(&t.top_cor[r.b], r.cor);
    atomicAdd(&t.top_conf[r.b], r.conf);
  }
  r.cnt = r.cor = 0u;
  r.conf = 0ull;
}
__device__ __forceinline__ void flush_run(const Tables& t, ClsRun& r) {
  if (r.n) {
    atomicAdd(&t.sup[r.y], r.n);
    atomicAdd(&t.prd[r.pred], r.n);
    if (r.y == r.pred) atomicAdd(&t.hit[r.y], r.n);
  }
  r.n = 0u;
}

struct LaneAcc {  // what a lane carries through its items
  double sum[4];     // nll, brier, g, h
  unsigned cnt[4];   // n_used, n_correct, n_bad, n_nan
  TopRun top;
  ClsRun cls;
};

// one scored-or-not pixel into the lane's sums and runs; -> its pred
__device__ __forceinline__ int account(const Tables& t, LaneAcc& acc, int bi, const RowVals& r, int y, bool used, bool bad) {
  const int pred = (bi == kNoIndex) ? 0 : bi;
  acc.cnt[2] += bad ? 1u : 0u;
  if (!used) return pred;
  const bool hit = pred == y;
  acc.sum[0] += (double)r.nll;
  acc.sum[1] += (double)r.brier;
  acc.sum[2] += (double)r.g;
  acc.sum[3] += (double)r.h;
  acc.cnt[0] += 1u;
  acc.cnt[1] += hit ? 1u : 0u;
  acc.cnt[3] += (r.conf != r.conf) ? 1u : 0u;
  if (t.nb > 0) {
    const int b = conf_bin(r.conf, t.nb);
    if (b != acc.top.b) {
      flush_run(t, acc.top);
      acc.top.b = b;
    }
    acc.top.cnt += 1u;
    acc.top.cor += hit ? 1u : 0u;
    acc.top.conf += fix30(r.conf);
  }
  if (t.C > 0) {
    if (y != acc.cls.y || pred != acc.cls.pred) {
      flush_run(t, acc.cls);
      acc.cls.y = y;
      acc.cls.pred = pred;
    }
    acc.cls.n += 1u;
  }
  return pred;
}

// class k of a lane's used pixels into the class-wise table: p_k = e_k / S0
template <int PPL>
__device__ __forceinline__ void account_class(const Tables& t, int k, const float (&x)[PPL], const float (&m)[PPL], float beta,
                                              const float (&rs0)[PPL], const int (&y)[PPL], const bool (&used)[PPL]) {
  int e0 = -1;
  unsigned n = 0u, pos = 0u;
  unsigned long long fx = 0ull;
  auto flush = [&]() {
    if (n) {
      atomicAdd(&t.cw_cnt[e0], n);
      if (pos) atomicAdd(&t.cw_pos[e0], pos);
      atomicAdd(&t.cw_conf[e0], fx);
    }
    n = pos = 0u;
    fx = 0ull;
  };
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    if (!used[j]) continue;
    const float p = class_exp(x[j], m[j], beta) * rs0[j];
    const int e = k * t.nb + conf_bin(p, t.nb);
    if (e != e0) {
      flush();
      e0 = e;
    }
    n += 1u;
    pos += (k == y[j]) ? 1u : 0u;
    fx += fix30(p);
  }
  flush();
}

// CMAX > 0: the register form (EXACT: C == CMAX); CMAX == 0: the general form
template <class T, int LOAD, int CMAX, bool EXACT>
__global__ __launch_bounds__(kThreads) void pixcal_kernel(CalArgs a) {
  constexpr int PPL = LOAD == kLoadVec ? 4 : 1;
  typedef typename T::elem E;
  extern __shared__ unsigned long long lds64[];
  __shared__ double sred[kWaves][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = EXACT ? CMAX : a.v.C;
  const int64_t sc = LOAD == kLoadCLast ? 1 : a.v.sc;

  Tables t;
  table_sizes(a.mode, C, a.n_bins, t.nb, t.C, t.E);
  t.top_conf = lds64;
  t.cw_conf = t.top_conf + t.nb;
  t.head = reinterpret_cast<unsigned*>(t.cw_conf + t.E);
  t.top_cnt = t.head + kTabHead;
  t.top_cor = t.top_cnt + t.nb;
  t.sup = t.top_cor + t.nb;
  t.prd = t.sup + t.C;
  t.hit = t.prd + t.C;
  t.cw_cnt = t.hit + t.C;
  t.cw_pos = t.cw_cnt + t.E;
  const int n_words = (int)(lds_bytes(t.nb, t.C, t.E) / 4);
  for (int i = tid; i < n_words; i += kThreads) reinterpret_cast<unsigned*>(lds64)[i] = 0u;
  __syncthreads();

  LaneAcc acc;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc.sum[k] = 0.0;
    acc.cnt[k] = 0u;
  }
  acc.top = {0, 0u, 0u, 0ull};
  acc.cls = {0, 0, 0u};
  const int64_t t0 = (int64_t)blockIdx.x * a.items_per_block;
  const int64_t t1 = (t0 + a.items_per_block < a.items) ? t0 + a.items_per_block : a.items;
  for (int64_t it = t0 + tid; it < t1; it += kThreads) {
    const int64_t pix0 = it * PPL;  // (vector form: the joined row is a multiple of four pixels, no group is cut)
    const E* p = static_cast<const E*>(a.v.x) + pixel_offset(a.v, pix0);
    int y[PPL];        // the class (0 for a pixel that is not scored)
    bool used[PPL], bad[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int64_t yl = a.lab ? load_label(a.lab, a.lab_code, pix0 + j) : -1;
      const bool ignored = !a.lab || (a.has_ignore && yl == a.ignore);
      const bool in = yl >= 0 && yl < C;
      used[j] = in && !ignored;
      bad[j] = !in && !ignored;
      y[j] = used[j] ? (int)yl : 0;
    }
    float conf[PPL], m[PPL];
    int pred[PPL];
    bool any = false;
#pragma unroll
    for (int j = 0; j < PPL; ++j) any = any || used[j];
    if constexpr (CMAX > 0) {
      float v[PPL][CMAX];
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {  // every load is issued; a class past C re-reads the last plane and is masked
        const int cc = (EXACT || c < C) ? c : C - 1;
        float x[PPL];
        load_px<T, LOAD>(p + cc * sc, x);
#pragma unroll
        for (int j = 0; j < PPL; ++j) v[j][c] = (EXACT || c < C) ? x[j] : -INFINITY;
      }
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        float xy = v[j][0];
        int bi = kNoIndex;
        m[j] = -INFINITY;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          best_take(m[j], bi, v[j][c], c);
          xy = (c == y[j]) ? v[j][c] : xy;
        }
        Sums s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CMAX; ++c) term(v[j][c], m[j], a.beta, s);  // (a class past C is -inf: it adds 0)
        const RowVals r = finish_vals(a.beta, m[j], s, xy, used[j]);
        conf[j] = r.conf;
        pred[j] = account(t, acc, bi, r, y[j], used[j], bad[j]);
      }
      if (t.E > 0 && any) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          if (EXACT || c < C) {
            float x[PPL];
#pragma unroll
            for (int j = 0; j < PPL; ++j) x[j] = v[j][c];
            account_class<PPL>(t, c, x, m, a.beta, conf, y, used);
          }
        }
      }
    } else {
      float xy[PPL];
      int bi[PPL];
      Sums s[PPL];
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        m[j] = -INFINITY;
        bi[j] = kNoIndex;
        xy[j] = 0.f;
        s[j] = {0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll 4
      for (int c = 0; c < C; ++c) {  // walk 1: the maximum and the first argmax
        float x[PPL];
        load_px<T, LOAD>(p + c * sc, x);
#pragma unroll
        for (int j = 0; j < PPL; ++j) best_take(m[j], bi[j], x[j], c);
      }
#pragma unroll 4
      for (int c = 0; c < C; ++c) {  // walk 2: the sums under it, and the label's logit
        float x[PPL];
        load_px<T, LOAD>(p + c * sc, x);
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          term(x[j], m[j], a.beta, s[j]);
          xy[j] = (c == y[j]) ? x[j] : xy[j];
        }
      }
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        const RowVals r = finish_vals(a.beta, m[j], s[j], xy[j], used[j]);
        conf[j] = r.conf;
        pred[j] = account(t, acc, bi[j], r, y[j], used[j], bad[j]);
      }
      if (t.E > 0 && any) {
        for (int c = 0; c < C; ++c) {  // walk 3: the class-wise table
          float x[PPL];
          load_px<T, LOAD>(p + c * sc, x);
          account_class<PPL>(t, c, x, m, a.beta, conf, y, used);
        }
      }
    }
    if constexpr (PPL == 4) {
      if (a.vec_store) {
        if (a.conf_map) *reinterpret_cast<float4*>(a.conf_map + pix0) = make_float4(conf[0], conf[1], conf[2], conf[3]);
        if (a.pred_map) *reinterpret_cast<int4*>(a.pred_map + pix0) = make_int4(pred[0], pred[1], pred[2], pred[3]);
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      if (a.conf_map) a.conf_map[pix0 + j] = conf[j];
      if (a.pred_map) a.pred_map[pix0 + j] = pred[j];
    }
  }
  if (t.nb > 0) flush_run(t, acc.top);
  if (t.C > 0) flush_run(t, acc.cls);

  // the four sums and the four counts: the lanes by a fixed tree, the waves in order
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc.sum[k] = wave_sum(acc.sum[k]);
    acc.cnt[k] = wave_sum(acc.cnt[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sred[wave][k] = acc.sum[k];
      if (acc.cnt[k]) atomicAdd(&t.head[k], acc.cnt[k]);
    }
  }
  __syncthreads();  // (also: every LDS atomic of the workgroup is done)
  if (tid < 4) {
    double s = 0.0;
    for (int w = 0; w < kWaves; ++w) s += sred[w][tid];
    a.part[(size_t)blockIdx.x * 4 + tid] = s;
  }
  // the tables: whatever the workgroup counted, into the workspace table (integer adds: any order gives the same sums)
  unsigned long long* g = a.tab;
  auto flush32 = [&](const unsigned* src, int n, unsigned long long* dst) {
    for (int i = tid; i < n; i += kThreads) {
      const unsigned v = src[i];
      if (v) atomicAdd(dst + i, (unsigned long long)v);
    }
  };
  auto flush64 = [&](const unsigned long long* src, int n, unsigned long long* dst) {
    for (int i = tid; i < n; i += kThreads) {
      const unsigned long long v = src[i];
      if (v) atomicAdd(dst + i, v);
    }
  };
  flush32(t.head, kTabHead, g);
  g += kTabHead;
  flush32(t.top_cnt, 2 * t.nb, g);  // count, correct
  flush64(t.top_conf, t.nb, g + 2 * t.nb);
  g += 3 * t.nb;
  flush32(t.sup, 3 * t.C, g);  // support, predicted, hit
  g += 3 * t.C;
  flush32(t.cw_cnt, 2 * t.E, g);  // count, pos
  flush64(t.cw_conf, t.E, g + 2 * t.E);
}

// The workspace table and the workgroups' partial sums into the record: rec[i] += ..., one thread per slot.  Record slot of
// table entry i >= kTabHead: i - kTabHead + kHead (the two are laid out alike after their heads).
__global__ __launch_bounds__(kThreads) void pixcal_final_kernel(const double* __restrict__ part, int64_t blocks,
                                                                 const unsigned long long* __restrict__ tab, int nb, int Cc,
                                                                 int E, int n_bins, int C, int64_t* __restrict__ rec) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {  // wave k: sum k of the partials; lane l adds blocks l, l + 64, ... in order, then the fixed tree
    double s = 0.0;
    for (int64_t b = lane; b < blocks; b += 64) s += part[b * 4 + wave];
    s = wave_sum(s);
    if (lane == 0) reinterpret_cast<double*>(rec)[3 + wave] += s;
  }
  if (tid < 3) rec[tid] += (int64_t)tab[tid];
  const bool nan = tab[3] != 0;  // a scored pixel without a softmax: bin 0 of every table it entered, and a NaN sum there
  const double step = 1.0 / (double)kFix, qnan = __builtin_nan("");
  // the record keeps the offsets of its full layout whatever the mode holds
  const int64_t rec_top = kHead, rec_cls = rec_top + 3 * (int64_t)n_bins, rec_cw = rec_cls + 3 * (int64_t)C;
  const unsigned long long* g = tab + kTabHead;
  for (int i = tid; i < 3 * nb; i += kThreads) {
    if (i < 2 * nb) rec[rec_top + i] += (int64_t)g[i];
    else reinterpret_cast<double*>(rec)[rec_top + i] += (double)g[i] * step + ((nan && i == 2 * nb) ? qnan : 0.0);
  }
  g += 3 * nb;
  for (int i = tid; i < 3 * Cc; i += kThreads) rec[rec_cls + i] += (int64_t)g[i];
  g += 3 * Cc;
  for (int i = tid; i < 3 * E; i += kThreads) {
    if (i < 2 * E) rec[rec_cw + i] += (int64_t)g[i];
    else reinterpret_cast<double*>(rec)[rec_cw + i] += (double)g[i] * step + ((nan && (i - 2 * E) % nb == 0) ? qnan : 0.0);
  }
}

// workgroups and lane items per workgroup of a launch over `items` lane items
void grid_of(int64_t items, int64_t& blocks, int64_t& per_block) {
  per_block = kThreads * kItemsPerThread;
  blocks = (items + per_block - 1) / per_block;
  if (blocks > kMaxBlocks) {
    per_block = (int64_t)round_up((size_t)((items + kMaxBlocks - 1) / kMaxBlocks), kThreads);
    blocks = (items + per_block - 1) / per_block;
  }
  if (blocks < 1) blocks = 1;
}

struct Plan {
  double* part;
  unsigned long long* tab;
  size_t tab_entries;
};

// sized before the strides are known: by the one-pixel-per-lane launch, which has the most workgroups
Plan make_plan(WsWalk& w, int64_t P, int nb, int Cc, int E) {
  int64_t blocks, per_block;
  grid_of(P, blocks, per_block);
  Plan p;
  p.part = w.take<double>((size_t)blocks * 4);
  p.tab_entries = (size_t)kTabHead + 3 * (size_t)nb + 3 * (size_t)Cc + 3 * (size_t)E;
  p.tab = w.take<unsigned long long>(p.tab_entries);
  return p;
}

bool sizes_ok(int64_t G, int64_t C, int64_t H, int64_t W, int n_bins, int mode) {
  if (G < 0 || H < 0 || W < 0 || C < 1 || C > kMaxC || G > kLim || H > kLim || W > kLim) return false;
  if (mode < kModeHead || mode > kModeClasswise) return false;
  if (mode == kModeHead ? n_bins != 0 : (n_bins < 1 || n_bins > kMaxBins)) return false;
  if (mode == kModeClasswise && C * n_bins > kMaxClasswise) return false;
  return G == 0 || H * W == 0 || G * H * W <= kMaxPixels;
}

template <class T, int LOAD, int CMAX, bool EXACT>
int launch_one(const CalArgs& a, unsigned grid, size_t lds, hipStream_t s) {
  static std::atomic<uint64_t> lds_ok{0};
  if (lds > 48 * 1024) {
    if (int rc = runia_allow_dynamic_lds(reinterpret_cast<const void*>(pixcal_kernel<T, LOAD, CMAX, EXACT>), 96 * 1024, lds_ok))
      return rc;
  }
  pixcal_kernel<T, LOAD, CMAX, EXACT><<<grid, kThreads, lds, s>>>(a);
  return runia_check_launch();
}

template <class T, int LOAD>
int launch_form(const CalArgs& a, unsigned grid, size_t lds, hipStream_t s) {
  if (a.v.C == 19) return launch_one<T, LOAD, 19, true>(a, grid, lds, s);
  if (a.v.C == 21) return launch_one<T, LOAD, 21, true>(a, grid, lds, s);
  if (a.v.C <= kRegC) return launch_one<T, LOAD, kRegC, false>(a, grid, lds, s);
  return launch_one<T, LOAD, 0, false>(a, grid, lds, s);
}

}  // namespace

extern "C" int64_t runia_pixel_calib_workspace_bytes(int64_t G, int64_t C, int64_t H, int64_t W, int n_bins, int mode) {
  if (!sizes_ok(G, C, H, W, n_bins, mode) || G == 0 || H * W == 0) return 0;
  int nb, Cc, E;
  table_sizes(mode, (int)C, n_bins, nb, Cc, E);
  return (int64_t)ws_bytes([&](WsWalk& w) { make_plan(w, G * H * W, nb, Cc, E); });
}

extern "C" int runia_pixel_calib_accumulate(const void* logits, int dtype, int64_t G, int64_t C, int64_t H, int64_t W,
                                            int64_t sn, int64_t sc, int64_t sh, int64_t sw, const void* labels,
                                            int label_dtype, int has_ignore, int64_t ignore_index, float beta, int n_bins,
                                            int mode, void* record, float* conf_map, int32_t* pred_map, void* workspace,
                                            size_t workspace_bytes, runia_stream_t stream) {
  if (!elem_dtype_ok(dtype) || !sizes_ok(G, C, H, W, n_bins, mode) || !view_ok(G, C, H, W, sn, sc, sh, sw) ||
      label_dtype < kLabI64 || label_dtype > kLabU8 || !(beta > 0.f) || beta == INFINITY)
    return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;  // nothing to add
  if (!logits || (!record && !conf_map && !pred_map) || (record && !labels) ||
      reinterpret_cast<uintptr_t>(record) % 8 != 0)
    return RUNIA_E_INVALID;
  const int64_t P = G * H * W;
  int nb, Cc, E;
  table_sizes(mode, (int)C, n_bins, nb, Cc, E);
  if (ws_refused(workspace, workspace_bytes, (size_t)runia_pixel_calib_workspace_bytes(G, C, H, W, n_bins, mode), 8))
    return RUNIA_E_WORKSPACE;
  WsWalk walk(workspace);
  const Plan plan = make_plan(walk, P, nb, Cc, E);
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(plan.tab, 0, plan.tab_entries * sizeof(unsigned long long), s) != hipSuccess) return RUNIA_E_LAUNCH;
  CalArgs a;
  a.v = make_view(logits, G, C, H, W, sn, sc, sh, sw);
  a.lab = record ? labels : nullptr;  // (maps alone: no pixel is scored)
  a.lab_code = label_dtype;
  a.has_ignore = has_ignore != 0;
  a.ignore = ignore_index;
  a.beta = beta;
  a.n_bins = n_bins;
  a.mode = mode;
  a.conf_map = conf_map;
  a.pred_map = pred_map;
  a.vec_store = (reinterpret_cast<uintptr_t>(conf_map) % 16 == 0 && reinterpret_cast<uintptr_t>(pred_map) % 16 == 0) ? 1 : 0;
  a.part = plan.part;
  a.tab = plan.tab;
  const size_t lds = lds_bytes(nb, Cc, E);
  int64_t blocks = 0;
  const int rc = dispatch_elem(dtype, [&](auto tag) {
    typedef decltype(tag) T;
    const bool vec = view_allows_vec(a.v, G, H, T::kBytes);
    a.items = vec ? P / 4 : P;
    grid_of(a.items, blocks, a.items_per_block);
    if (vec) return launch_form<T, kLoadVec>(a, (unsigned)blocks, lds, s);
    if (a.v.sc == 1 && C > 1) return launch_form<T, kLoadCLast>(a, (unsigned)blocks, lds, s);
    return launch_form<T, kLoadElem>(a, (unsigned)blocks, lds, s);
  });
  if (rc != RUNIA_OK || !record) return rc;
  pixcal_final_kernel<<<1, kThreads, 0, s>>>(plan.part, blocks, plan.tab, nb, Cc, E, n_bins, (int)C,
                                             static_cast<int64_t*>(record));
  return runia_check_launch();
}
