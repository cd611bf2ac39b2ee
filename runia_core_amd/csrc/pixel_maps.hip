// Per-pixel uncertainty maps of a segmentation head (DeepLabv3+, U-Net): predictive entropy, mutual information, MSP, energy,
// max logit, label and the mean distribution of every pixel from the n_mc stochastic forward passes, read where the model
// left them.
//   runia_pixel_uncertainty_maps   ONE launch over G images x n_mc passes of (C, H, W) logits in f32 / f16 / bf16, NCHW,
//                                  channels_last or any strided view.  The definition is the reference's
//                                  get_predictive_uncertainty_score (inference/funcs.py:430-465) applied to one row per
//                                  (image, pixel, sample) - on the 4-D tensor itself that function sums the wrong axis.
//   runia_pixel_map_reduce_f32     mean / max / count of a (G, H, W) map per image under an optional uint8 mask.
//
// In NCHW the classes of a pixel are H * W elements apart, so the row kernels (funcs_rows.hip: a lane or a wave owns a
// class-contiguous row) do not apply.  Here a lane owns kPix = 4 neighbouring pixels and walks the class planes: consecutive
// lanes read consecutive pixels of every plane (one 16-byte load per lane and plane for f32, 8 bytes for f16 / bf16 - the
// per-pixel state below caps a lane at four pixels), and all sums over classes run inside one lane in ascending class order
// (no cross-lane reduction, no atomics: run-to-run bit identical).  Arithmetic per element is mcd_uncertainty_kernel's:
// exp_nonpos(x - max), the quotient by div_by_rcp, p * log_nonneg(p) with 0 * log 0 = NaN, denormals kept.
//
// Two kernels, picked on the host from C:
//   pixel_maps_reg_kernel    C <= 24 (Cityscapes 19, VOC 21): the C logits of a sample and the C running means of a pixel
//                            stay in registers; every logit is read once.
//   pixel_maps_2pass_kernel  any C: pass A reads the n_mc samples once for their max / sum-of-exp (online, one exponential
//                            per logit) and keeps three floats per (pixel, sample) - in LDS while 3 * n_mc * kPix * 64 floats
//                            fit 64 KB, else in the caller's workspace; pass B walks the classes, re-reads the n_mc logits
//                            of a class (from the caches: a workgroup's footprint is revisited after C * n_mc loads) and forms
//                            pbar_c, its entropy term and the samples' entropy terms on the fly.  Also taken when max_logit
//                            is wanted (the register kernel has no room for a second C-sized array per pixel).
// Loads are 4 pixels wide when w has unit stride and every other stride and base is a multiple of four elements; a group cut
// by the end of a row, an odd base or any other stride pattern (channels_last: sc == 1; crops) is read element by element
// through the strides, in place.  Rows that follow one another in memory (sh == W * sw) are treated as one long row.
#include <cfloat>

#include "common.hpp"
#include "elem.hpp"

namespace {

constexpr int kPix = 4;        // pixels per lane of the vector variants
constexpr int kRegC = 24;      // widest head of the register kernel
constexpr int kLdsBytes = 64 * 1024;

struct PixArgs {
  const void* const* ptrs;  // n_mc bases of (G, C, H, W) blocks, or one base of (G * n_mc, C, H, W) when `single`
  int64_t sn, sc, sh, sw;   // element strides (sh, sw of the collapsed rows)
  int64_t HW, items, P;     // pixels per image; G * Hr * GW lane items; G * H * W
  int G, C, Hr, Wr, GW, n_mc, single, vec;
  float *pred_h, *mi, *msp, *energy, *max_logit, *mean_probs;
  int* label;
  float* ws;                // [n_mc][3][P] row statistics of the two-pass kernel when they do not fit LDS
};

template <class T>
__device__ __forceinline__ const typename T::elem* sample_base(const PixArgs& a, int64_t g, int s) {
  typedef typename T::elem E;
  if (a.single) return static_cast<const E*>(a.ptrs[0]) + (g * a.n_mc + s) * a.sn;
  return static_cast<const E*>(a.ptrs[s]) + g * a.sn;
}

// every base a multiple of PPL elements?  (uniform; the strides were checked on the host)
template <class T, int PPL>
__device__ __forceinline__ bool bases_aligned(const PixArgs& a) {
  if (PPL == 1 || !a.vec) return false;
  const uintptr_t mask = PPL * sizeof(typename T::elem) - 1;
  uintptr_t bits = 0;
  const int n = a.single ? 1 : a.n_mc;
  for (int s = 0; s < n; ++s) bits |= reinterpret_cast<uintptr_t>(a.ptrs[s]);
  return (bits & mask) == 0;
}

// PPL neighbouring pixels of one class plane.  VEC: one aligned load.  Otherwise element by element through sw; the lanes
// past the end of the row (j >= nv) re-read the last valid pixel, so that no load sits behind a branch.
template <class T, int PPL, bool VEC>
__device__ __forceinline__ void load_px(const typename T::elem* p, int64_t sw, int nv, float (&v)[PPL]) {
  if constexpr (VEC) {
    static_assert(PPL == 4, "vector loads are four pixels wide");
    if constexpr (T::kBytes == 4) ld16<T>(p, v);
    else ld8<T>(p, v);
  } else {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int jj = j < nv ? j : nv - 1;
      v[j] = widen(T{}, p[jj * sw]);
    }
  }
}

struct PixOut {  // one pixel's results
  float ph, mi, msp, en, ml;
  int lab;
};

__device__ __forceinline__ void store_px(const PixArgs& a, int64_t pix, const PixOut& o) {
  if (a.pred_h) a.pred_h[pix] = o.ph;
  if (a.mi) a.mi[pix] = o.mi;
  if (a.msp) a.msp[pix] = o.msp;
  if (a.energy) a.energy[pix] = o.en;
  if (a.max_logit) a.max_logit[pix] = o.ml;
  if (a.label) a.label[pix] = o.lab;
}

// ---- C <= CMAX: logits and means in registers ------------------------------------------------------------------------------
template <class T, int PPL, int CMAX, bool EXACT, bool VEC>
__device__ __forceinline__ void reg_item(const PixArgs& a, int64_t g, int64_t off, int64_t pix0, int nv) {
  const int C = EXACT ? CMAX : a.C;
  const float fn = (float)a.n_mc;
  float mean[PPL][CMAX];
  float eh[PPL], en[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    eh[j] = 0.f;
    en[j] = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) mean[j][c] = 0.f;
  }
  for (int s = 0; s < a.n_mc; ++s) {
    const typename T::elem* p = sample_base<T>(a, g, s) + off;
    float v[PPL][CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {  // every load is issued; a class past C re-reads the last plane and is masked
      const int cc = (EXACT || c < C) ? c : C - 1;
      float x[PPL];
      load_px<T, PPL, VEC>(p + cc * a.sc, a.sw, nv, x);
#pragma unroll
      for (int j = 0; j < PPL; ++j) v[j][c] = (EXACT || c < C) ? x[j] : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      float m = -INFINITY;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) m = fmaxf(m, v[j][c]);
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        v[j][c] = (EXACT || c < C) ? exp_nonpos(v[j][c] - m) : 0.f;
        sum += v[j][c];
      }
      const float rsum = 1.0f / sum;
      float h = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if (EXACT || c < C) {
          const float pr = div_by_rcp(v[j][c], sum, rsum);
          mean[j][c] += pr;
          h += pr * log_nonneg(pr);
        }
      }
      eh[j] -= h;
      en[j] += m + log_nonneg(sum);
    }
  }
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    if (j < nv) {
      PixOut o;
      float ph = 0.f, best = -INFINITY;
      int lab = 0;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if (EXACT || c < C) {
          const float e = mean[j][c] / fn;
          ph += e * log_nonneg(e);
          if (e > best) {
            best = e;
            lab = c;
          }
          if (a.mean_probs) a.mean_probs[((int64_t)(pix0 / a.HW) * C + c) * a.HW + pix0 % a.HW + j] = e;
        }
      }
      o.ph = -ph;
      o.mi = -ph - eh[j] / fn;
      o.msp = best;
      o.en = en[j] / fn;
      o.ml = 0.f;  // (not produced by this kernel: max_logit goes to the two-pass kernel)
      o.lab = lab;
      store_px(a, pix0 + j, o);
    }
  }
}

template <class T, int PPL, int CMAX, bool EXACT>
__global__ __launch_bounds__(256) void pixel_maps_reg_kernel(PixArgs a) {
  const bool aligned = bases_aligned<T, PPL>(a);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < a.items; t += (int64_t)gridDim.x * 256) {
    const int64_t gw = t % a.GW, r = t / a.GW, h = r % a.Hr, g = r / a.Hr;
    const int64_t w0 = gw * PPL;
    const int nv = a.Wr - w0 < PPL ? (int)(a.Wr - w0) : PPL;
    const int64_t off = h * a.sh + w0 * a.sw, pix0 = g * a.HW + h * a.Wr + w0;
    if constexpr (PPL > 1) {
      if (aligned && nv == PPL) {
        reg_item<T, PPL, CMAX, EXACT, true>(a, g, off, pix0, nv);
        continue;
      }
    }
    reg_item<T, PPL, CMAX, EXACT, false>(a, g, off, pix0, nv);
  }
}

// ---- any C: row statistics first, then the classes ---------------------------------------------------------------------------
// st(s, k, j): statistic k (0 max, 1 sum of exp, 2 its reciprocal) of sample s of the lane's pixel j
template <int PPL, bool LDS>
struct Stats {
  float* base;
  int64_t s1;
  __device__ __forceinline__ float& at(int s, int k, int j) const {
    if constexpr (LDS) return base[((s * 3 + k) * PPL + j) * 64];
    else return base[(int64_t)(s * 3 + k) * s1 + j];
  }
};

template <class T, int PPL, bool LDS, bool VEC>
__device__ __forceinline__ void two_pass_item(const PixArgs& a, const Stats<PPL, LDS>& st, int64_t g, int64_t off,
                                              int64_t pix0, int nv) {
  const int C = a.C;
  const float fn = (float)a.n_mc;
  float en[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) en[j] = 0.f;
  for (int s = 0; s < a.n_mc; ++s) {  // pass A
    const typename T::elem* p = sample_base<T>(a, g, s) + off;
    float m[PPL], sum[PPL];
    load_px<T, PPL, VEC>(p, a.sw, nv, m);
    // A row that opens with -inf (masked classes) starts from (-FLT_MAX, 0) instead of (-inf, 1): a second -inf would give
    // d = -inf - (-inf) = NaN below and leave the NaN in the sum.  From there every -inf adds 0, the first finite logit
    // rescales the sum by exp(-huge) = 0, and only a row of nothing but -inf ends with sum == 0: it gets its -inf back.
    // Rows that open with a finite logit run as before, bit for bit.
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const bool masked = m[j] == -INFINITY;
      sum[j] = masked ? 0.f : 1.f;
      m[j] = masked ? -FLT_MAX : m[j];
    }
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
      float x[PPL];
      load_px<T, PPL, VEC>(p + c * a.sc, a.sw, nv, x);
#pragma unroll
      for (int j = 0; j < PPL; ++j) {  // sum of exp(x - running max): one exponential per logit
        const float d = x[j] - m[j];
        const float e = exp_nonpos(-fabsf(d));
        sum[j] = d > 0.f ? fmaf(sum[j], e, 1.f) : sum[j] + e;
        m[j] = fmaxf(m[j], x[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) m[j] = sum[j] == 0.f ? -INFINITY : m[j];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      if (LDS || j < nv) {
        st.at(s, 0, j) = m[j];
        st.at(s, 1, j) = sum[j];
        st.at(s, 2, j) = 1.0f / sum[j];
      }
      en[j] += m[j] + log_nonneg(sum[j]);
    }
  }
  float ph[PPL], eh[PPL], best[PPL], ml[PPL];
  int lab[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    ph[j] = 0.f;
    eh[j] = 0.f;
    best[j] = -INFINITY;
    ml[j] = -INFINITY;
    lab[j] = 0;
  }
  const int64_t gimg = pix0 / a.HW, pin = pix0 % a.HW;
  for (int c = 0; c < C; ++c) {  // pass B
    float mean[PPL], xs[PPL], hc[PPL];  // of this class: sum over the samples of p, of x and of p log p
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      mean[j] = 0.f;
      xs[j] = 0.f;
      hc[j] = 0.f;
    }
#pragma unroll 4
    for (int s = 0; s < a.n_mc; ++s) {
      float x[PPL];
      load_px<T, PPL, VEC>(sample_base<T>(a, g, s) + off + c * a.sc, a.sw, nv, x);
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        const int jj = (LDS || j < nv) ? j : nv - 1;
        const float pr = div_by_rcp(exp_nonpos(x[j] - st.at(s, 0, jj)), st.at(s, 1, jj), st.at(s, 2, jj));
        mean[j] += pr;
        hc[j] -= pr * log_nonneg(pr);
        xs[j] += x[j];
      }
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const float e = mean[j] / fn;
      ph[j] += e * log_nonneg(e);
      eh[j] += hc[j];
      if (e > best[j]) {
        best[j] = e;
        lab[j] = c;
      }
      ml[j] = fmaxf(ml[j], xs[j] / fn);
      if (a.mean_probs && j < nv) a.mean_probs[(gimg * C + c) * a.HW + pin + j] = e;
    }
  }
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    if (j < nv) {
      PixOut o;
      o.ph = -ph[j];
      o.mi = -ph[j] - eh[j] / fn;
      o.msp = best[j];
      o.en = en[j] / fn;
      o.ml = ml[j];
      o.lab = lab[j];
      store_px(a, pix0 + j, o);
    }
  }
}

template <class T, int PPL, bool LDS>
__global__ __launch_bounds__(64) void pixel_maps_2pass_kernel(PixArgs a) {
  extern __shared__ float stat_lds[];  // [n_mc][3][PPL][64]
  const bool aligned = bases_aligned<T, PPL>(a);
  for (int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x; t < a.items; t += (int64_t)gridDim.x * 64) {
    const int64_t gw = t % a.GW, r = t / a.GW, h = r % a.Hr, g = r / a.Hr;
    const int64_t w0 = gw * PPL;
    const int nv = a.Wr - w0 < PPL ? (int)(a.Wr - w0) : PPL;
    const int64_t off = h * a.sh + w0 * a.sw, pix0 = g * a.HW + h * a.Wr + w0;
    Stats<PPL, LDS> st;
    st.base = LDS ? stat_lds + threadIdx.x : a.ws + pix0;
    st.s1 = a.P;
    if constexpr (PPL > 1) {
      if (aligned && nv == PPL) {
        two_pass_item<T, PPL, LDS, true>(a, st, g, off, pix0, nv);
        continue;
      }
    }
    two_pass_item<T, PPL, LDS, false>(a, st, g, off, pix0, nv);
  }
}

template <class T, int PPL>
int launch_ppl(const PixArgs& a, bool two_pass, hipStream_t s) {
  if (!two_pass) {
    const unsigned grid = runia_stream_grid(a.items, 256);
    if (a.C == 19) pixel_maps_reg_kernel<T, PPL, 19, true><<<grid, 256, 0, s>>>(a);
    else if (a.C == 21) pixel_maps_reg_kernel<T, PPL, 21, true><<<grid, 256, 0, s>>>(a);
    else if (a.C <= 8) pixel_maps_reg_kernel<T, PPL, 8, false><<<grid, 256, 0, s>>>(a);
    else pixel_maps_reg_kernel<T, PPL, kRegC, false><<<grid, 256, 0, s>>>(a);
    return runia_check_launch();
  }
  const unsigned grid = runia_stream_grid(a.items, 64);
  const int64_t lds = (int64_t)a.n_mc * 3 * PPL * 64 * sizeof(float);
  if (lds <= kLdsBytes) pixel_maps_2pass_kernel<T, PPL, true><<<grid, 64, (size_t)lds, s>>>(a);
  else pixel_maps_2pass_kernel<T, PPL, false><<<grid, 64, 0, s>>>(a);
  return runia_check_launch();
}

// ---- per-image mean / max / count of a map ------------------------------------------------------------------------------------
// One workgroup per image; every thread adds its pixels (tid, tid + 1024, ...) in f64, then a fixed tree over the lanes and
// the 16 waves: the same bits on every run.  NaN pixels make the mean NaN; the max skips them (fmaxf).
__global__ __launch_bounds__(1024) void pixel_map_reduce_kernel(const float* __restrict__ map, const uint8_t* __restrict__ valid,
                                                                 int64_t HW, float* __restrict__ mean, float* __restrict__ mx,
                                                                 int64_t* __restrict__ count) {
  __shared__ double s_sum[16];
  __shared__ float s_max[16];
  __shared__ long long s_cnt[16];
  const int64_t g = blockIdx.x;
  const float* p = map + g * HW;
  const uint8_t* v = valid ? valid + g * HW : nullptr;
  double sum = 0.0;
  float m = -INFINITY;
  long long cnt = 0;
  for (int64_t i = threadIdx.x; i < HW; i += 1024) {
    if (!v || v[i]) {
      const float x = p[i];
      sum += (double)x;
      m = fmaxf(m, x);
      ++cnt;
    }
  }
  sum = wave_sum(sum);
  m = wave_max_f32(m);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = sum;
    s_max[threadIdx.x >> 6] = m;
    s_cnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    float tm = -INFINITY;
    long long tc = 0;
    for (int w = 0; w < 16; ++w) {
      t += s_sum[w];
      tm = fmaxf(tm, s_max[w]);
      tc += s_cnt[w];
    }
    if (mean) mean[g] = tc ? (float)(t / (double)tc) : __builtin_nanf("");
    if (mx) mx[g] = tm;
    if (count) count[g] = tc;
  }
}

bool two_pass_needed(int64_t C, int want_max_logit) { return C > kRegC || want_max_logit; }

bool strides_allow_vec(const PixArgs& a, int64_t sample_rows) {
  auto ok = [](int64_t stride, int64_t extent) { return extent <= 1 || stride % kPix == 0; };
  return a.sw == 1 && a.Wr >= kPix && ok(a.sh, a.Hr) && ok(a.sc, a.C) && ok(a.sn, sample_rows);
}

}  // namespace

extern "C" size_t runia_pixel_maps_workspace_bytes(int64_t G, int64_t C, int64_t H, int64_t W, int n_mc, int want_max_logit) {
  if (G <= 0 || C <= 0 || H <= 0 || W <= 0 || n_mc < 1) return 0;
  if (!two_pass_needed(C, want_max_logit)) return 0;
  // the narrowest launch keeps 3 * n_mc * 64 floats per workgroup: in LDS up to 64 KB, whatever the strides turn out to be
  if ((int64_t)n_mc * 3 * kPix * 64 * (int64_t)sizeof(float) <= kLdsBytes) return 0;
  return (size_t)n_mc * 3 * (size_t)(G * H * W) * sizeof(float);
}

extern "C" int runia_pixel_uncertainty_maps(const void* const* table, int single, int dtype, int64_t G, int n_mc, int64_t C,
                                            int64_t H, int64_t W, int64_t sn, int64_t sc, int64_t sh, int64_t sw, float* pred_h,
                                            float* mi, float* msp, float* energy, float* max_logit, int32_t* label,
                                            float* mean_probs, void* workspace, size_t workspace_bytes,
                                            runia_stream_t stream) {
  const int64_t lim = 0x7fffffffll;
  if (G < 0 || C < 1 || H < 0 || W < 0 || n_mc < 1 || G > lim || C > lim || H > lim || W > lim || !elem_dtype_ok(dtype) ||
      sn < 0 || sc < 0 || sh < 0 || sw < 0 || (single != 0 && single != 1))
    return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;
  if (G * H * W > (lim << 8) || n_mc > (1 << 20)) return RUNIA_E_INVALID;
  if (!table || (!pred_h && !mi && !msp && !energy && !max_logit && !label && !mean_probs)) return RUNIA_E_INVALID;
  const size_t need = runia_pixel_maps_workspace_bytes(G, C, H, W, n_mc, max_logit != nullptr);
  if (need && ws_refused(workspace, workspace_bytes, need, 4)) return RUNIA_E_WORKSPACE;
  PixArgs a;
  a.ptrs = table;
  a.sn = sn; a.sc = sc; a.sh = sh; a.sw = sw;
  a.HW = H * W;
  a.P = G * a.HW;
  a.G = (int)G; a.C = (int)C; a.n_mc = n_mc; a.single = single;
  const bool flat = H == 1 || sh == W * sw;  // the rows follow one another: one long row
  a.Hr = flat ? 1 : (int)H;
  if (flat && a.HW > lim) return RUNIA_E_INVALID;
  a.Wr = flat ? (int)a.HW : (int)W;
  a.pred_h = pred_h; a.mi = mi; a.msp = msp; a.energy = energy; a.max_logit = max_logit; a.mean_probs = mean_probs;
  a.label = label;
  a.ws = static_cast<float*>(workspace);
  a.vec = strides_allow_vec(a, single ? G * n_mc : G) ? 1 : 0;
  const int ppl = a.vec ? kPix : 1;
  a.GW = (a.Wr + ppl - 1) / ppl;
  a.items = G * a.Hr * a.GW;
  const bool two_pass = two_pass_needed(C, max_logit != nullptr);
  hipStream_t s = as_stream(stream);
  return dispatch_elem(dtype, [&](auto t) {
    typedef decltype(t) T;
    return a.vec ? launch_ppl<T, kPix>(a, two_pass, s) : launch_ppl<T, 1>(a, two_pass, s);
  });
}

extern "C" int runia_pixel_map_reduce_f32(const float* map, const uint8_t* valid, int64_t G, int64_t HW, float* mean,
                                          float* max, int64_t* count, runia_stream_t stream) {
  if (G < 0 || HW < 0 || G > 0x7fffffffll) return RUNIA_E_INVALID;
  if (G == 0) return RUNIA_OK;
  if ((!map && HW > 0) || (!mean && !max && !count)) return RUNIA_E_INVALID;
  pixel_map_reduce_kernel<<<(unsigned)G, 1024, 0, as_stream(stream)>>>(map, valid, HW, mean, max, count);
  return runia_check_launch();
}
