// f3: the step in front of the sampler for object-level inference (BASELINE config 4): torchvision.ops.roi_align as
// _dropblock_rois_get_entropy / _reduce_features_to_rois call it (reference feature_extraction/object_level.py:283-292,
// 340-349: output_size per hooked layer, spatial_scale = W_feat / W_img, sampling_ratio, aligned=True), written from the
// published algorithm (torchvision is absent from the image: roi_align kernel of torchvision/csrc/ops):
//   roi box scaled by spatial_scale, shifted by -0.5 when aligned; bin = roi / pooled; every bin averages a
//   grid_h x grid_w lattice of bilinear samples (grid = sampling_ratio, or ceil(roi / pooled) when <= 0);
//   samples further than one pixel outside the map contribute 0, coordinates are clamped to the map.
// Output [K, C, PH, PW] f32 = the (N, C, H, W) input of the sampler kernels (runia_mc_entropy_f32 for 2x2/4x4/7x7/8x8).
#include "common.hpp"
#include "roi_source.hpp"

namespace {

__device__ __forceinline__ float bilinear(const float* __restrict__ in, int H, int W, float y, float x) {
  if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return 0.f;
  if (y <= 0.f) y = 0.f;
  if (x <= 0.f) x = 0.f;
  int y_low = (int)y, x_low = (int)x, y_high, x_high;
  if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else { y_high = y_low + 1; }
  if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else { x_high = x_low + 1; }
  const float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.f - ly, hx = 1.f - lx;
  const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
  const float v1 = in[y_low * W + x_low], v2 = in[y_low * W + x_high];
  const float v3 = in[y_high * W + x_low], v4 = in[y_high * W + x_high];
  return w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
}

__global__ __launch_bounds__(256) void roi_align_kernel(const float* __restrict__ input, const float* __restrict__ boxes,
                                                        const int* __restrict__ batch_idx, float* __restrict__ out,
                                                        int64_t total, int64_t B, int C, int H, int W, int PH, int PW,
                                                        float spatial_scale, int sampling_ratio, int aligned) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int pw = (int)(idx % PW), ph = (int)((idx / PW) % PH);
    const int c = (int)((idx / ((int64_t)PW * PH)) % C);
    const int64_t k = idx / ((int64_t)PW * PH * C);
    const float* box = boxes + k * 4;
    const int b = batch_idx ? batch_idx[k] : 0;
    if (b < 0 || b >= B) {  // an image index outside the batch: a defined result (zeros), never a read outside the feature maps
      out[idx] = 0.f;
      continue;
    }
    const float offset = aligned ? 0.5f : 0.f;
    const float x1 = box[0] * spatial_scale - offset, y1 = box[1] * spatial_scale - offset;
    const float x2 = box[2] * spatial_scale - offset, y2 = box[3] * spatial_scale - offset;
    float roi_w = x2 - x1, roi_h = y2 - y1;
    if (!aligned) { roi_w = fmaxf(roi_w, 1.f); roi_h = fmaxf(roi_h, 1.f); }
    const float bin_h = roi_h / (float)PH, bin_w = roi_w / (float)PW;
    const int grid_h = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(roi_h / (float)PH);
    const int grid_w = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(roi_w / (float)PW);
    const float count = fmaxf((float)(grid_h * grid_w), 1.f);
    const float* in = input + ((int64_t)b * C + c) * (int64_t)H * W;
    float acc = 0.f;
    for (int iy = 0; iy < grid_h; ++iy) {
      const float y = y1 + (float)ph * bin_h + ((float)iy + 0.5f) * bin_h / (float)grid_h;
      for (int ix = 0; ix < grid_w; ++ix) {
        const float x = x1 + (float)pw * bin_w + ((float)ix + 0.5f) * bin_w / (float)grid_w;
        acc += bilinear(in, H, W, y, x);
      }
    }
    out[idx] = acc / count;
  }
}

// ---- roi_align folded into the sampler's load (mc_sampler.hip, roi_load_map) ---------------------------------------------------
// The feature map in NHWC, so that the 64 channels of a wave read one bilinear tap as one contiguous run.
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int C,
                                                            int64_t HW) {
  __shared__ float tile[64][65];
  const int64_t b = blockIdx.z;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int c = c0 + ty + 4 * r;
    const int64_t p = p0 + tx;
    tile[ty + 4 * r][tx] = (c < C && p < HW) ? in[(b * C + c) * HW + p] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t p = p0 + ty + 4 * r;
    const int c = c0 + tx;
    if (c < C && p < HW) out[(b * HW + p) * C + c] = tile[tx][ty + 4 * r];
  }
}

// One thread per sample row or sample column of a ROI (PH * G rows, then PW * G columns).  The coordinates, the validity
// test, the clamping and the weights are those of `bilinear` / roi_align_kernel above, expression for expression (they are
// separable: y and x never meet before the four products).
__global__ __launch_bounds__(256) void roi_sample_table_kernel(RoiSource src, const float* __restrict__ boxes,
                                                                const int* __restrict__ batch_idx, unsigned* __restrict__ tab,
                                                                int64_t K, int64_t B, int C, int H, int W, int PH, int PW,
                                                                float spatial_scale, int G, int aligned) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<RoiSource*>(tab) = src;
  unsigned* roi_tab = tab + 16;  // 64 bytes of RoiSource in front
  const int nrows = PH * G, ncols = PW * G, per_roi = nrows + ncols, roi_dwords = 8 + 4 * per_roi;
  const int64_t total = K * per_roi;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t k = idx / per_roi;
    const int j = (int)(idx % per_roi);
    const bool is_row = j < nrows;
    const int sidx = is_row ? j : j - nrows;
    const int bin = sidx / G, sub = sidx % G;
    const float* box = boxes + k * 4;
    const float offset = aligned ? 0.5f : 0.f;
    const float lo = box[is_row ? 1 : 0] * spatial_scale - offset, hi = box[is_row ? 3 : 2] * spatial_scale - offset;
    float extent = hi - lo;
    if (!aligned) extent = fmaxf(extent, 1.f);
    const int P = is_row ? PH : PW, L = is_row ? H : W;
    const float bin_sz = extent / (float)P;
    float t = lo + (float)bin * bin_sz + ((float)sub + 0.5f) * bin_sz / (float)G;
    unsigned* hd = roi_tab + k * (int64_t)roi_dwords;
    unsigned* e = hd + 8 + 4 * j;
    // An image index outside [0, B) would move the loader's buffer descriptor off the feature maps (its own range check then
    // protects nothing): such a ROI is made of "outside" samples only - every tap beyond the buffer, weights 0 - on image 0,
    // i.e. the zeros runia_roi_align_f32 writes for it.
    const int image = batch_idx ? batch_idx[k] : 0;
    const bool bad_image = image < 0 || image >= B;
    if (j == 0) {
      hd[0] = bad_image ? 0u : (unsigned)image;
#pragma unroll
      for (int q = 1; q < 8; ++q) hd[q] = 0u;
    }
    const bool outside = bad_image || (t < -1.0f || t > (float)L);
    // a sample row / column more than a pixel outside the map contributes nothing (roi_align's `continue`): its byte offset is
    // the size of the image - every tap of it lies beyond the buffer the loader reads through, and such a load returns 0 -
    // and its weights are 0, so the sample is +0.0 without a test in the loader (the scalar offset is part of the range check
    // on gfx950: tools/microbench/buffer_soffset_range.hip)
    if (outside) {
      e[0] = e[1] = (unsigned)src.image_bytes;
      e[2] = e[3] = 0u;
      continue;
    }
    if (t <= 0.f) t = 0.f;
    int low = (int)t, high;
    if (low >= L - 1) { high = low = L - 1; t = (float)low; } else { high = low + 1; }
    const float l = t - (float)low, h = 1.f - l;
    const unsigned step = is_row ? (unsigned)W * (unsigned)C * 4u : (unsigned)C * 4u;
    e[0] = (unsigned)low * step;
    e[1] = (unsigned)high * step;
    e[2] = __float_as_uint(h);
    e[3] = __float_as_uint(l);
  }
}

}  // namespace

size_t runia_roi_sample_table_bytes(int64_t K, int PH, int PW, int G) {
  return 64 + (size_t)K * (size_t)(8 + 4 * (PH * G + PW * G)) * 4;
}

int runia_roi_sample_table(const float* feat_nhwc, const float* boxes, const int* batch_idx, void* table, size_t table_bytes,
                           int64_t K, int64_t B, int C, int H, int W, int PH, int PW, double spatial_scale, int G, int aligned,
                           hipStream_t s) {
  if (table_bytes < runia_roi_sample_table_bytes(K, PH, PW, G) || PH * G > 32 || PW * G > 32) return RUNIA_E_WORKSPACE;
  if ((int64_t)H * W * C * 4 >= (int64_t)1 << 30) return RUNIA_E_INVALID;  // (offsets of outside samples: row + column + channel stay below 2^32)
  RoiSource src;
  src.nhwc = feat_nhwc;
  src.table = reinterpret_cast<const unsigned*>(table) + 16;
  src.image_bytes = (int64_t)H * W * C * 4;
  src.C = C;
  src.roi_dwords = 8 + 4 * (PH * G + PW * G);
  const int64_t total = K * (PH * G + PW * G);
  roi_sample_table_kernel<<<runia_stream_grid(total, 256), 256, 0, s>>>(src, boxes, batch_idx, reinterpret_cast<unsigned*>(table),
                                                                        K, B, C, H, W, PH, PW, (float)spatial_scale, G, aligned);
  return runia_check_launch();
}

extern "C" int runia_nchw_to_nhwc_f32(const float* in, float* out, int64_t B, int C, int64_t HW, runia_stream_t stream) {
  if (B < 0 || C <= 0 || HW <= 0 || B > 65535) return RUNIA_E_INVALID;
  if (B == 0) return RUNIA_OK;
  if (!in || !out) return RUNIA_E_INVALID;
  const dim3 grid((unsigned)((HW + 63) / 64), (unsigned)((C + 63) / 64), (unsigned)B);
  nchw_to_nhwc_kernel<<<grid, 256, 0, as_stream(stream)>>>(in, out, C, HW);
  return runia_check_launch();
}

extern "C" int runia_roi_align_f32(const float* input, const float* boxes, const int* batch_idx, float* out, int64_t K,
                                   int64_t B, int C, int H, int W, int PH, int PW, double spatial_scale,
                                   int sampling_ratio, int aligned, runia_stream_t stream) {
  if (K < 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || PH <= 0 || PW <= 0) return RUNIA_E_INVALID;
  if (K == 0) return RUNIA_OK;
  if (!input || !boxes || !out) return RUNIA_E_INVALID;
  if (B > 1 && !batch_idx) return RUNIA_E_INVALID;
  const int64_t total = K * C * PH * PW;
  roi_align_kernel<<<runia_stream_grid(total, 256), 256, 0, as_stream(stream)>>>(
      input, boxes, batch_idx, out, total, B, C, H, W, PH, PW, (float)spatial_scale, sampling_ratio, aligned);
  return runia_check_launch();
}

// ---- roi_align(...).mean((2, 3)) without the (K, C, PH, PW) tensor ------------------------------------------------------
// The out-of-map test, the clamping and the weights of `bilinear` work on each axis separately and the sample lattice is the
// product of PH * grid_h sample rows and PW * grid_w sample columns, so the mean over all samples of a box is
//   mean[k, c] = 1 / (PH * PW * grid_h * grid_w) * sum_r sum_q Wy[r] * Wx[q] * x[b, r, q, c]
// with Wy [H] / Wx [W] the per-axis bilinear weights of the samples added up per pixel row / column.  One workgroup per
// (box, 256-channel chunk): the weights in LDS (f64, every row / column summed by one thread in sample order), the rows and
// columns of non-zero weight compacted in order (wave ballots), then every wave takes a contiguous quarter of the
// (row, column) pairs with one lane per four channels (16-byte loads of the channels-last map, contiguous per wave) and an
// f64 accumulator; the four quarters are added in wave order.  No atomics: two calls give equal bits.
// The pairs of non-zero weight are at most (2 * PH * grid_h) x (2 * PW * grid_w): never more loads than the direct form's
// 4 * PH * PW * grid_h * grid_w taps, far fewer when the samples are denser than the pixels (small boxes, adaptive grids).
// ROI_MEANS_FORM=1 (tools/ablate/build_lib_variant.sh): the direct form over the sample pairs, four taps each, for the
// ablation only (samples past 256 per axis give NaN there).
#ifndef ROI_MEANS_FORM
#define ROI_MEANS_FORM 0
#endif

namespace {

constexpr int kRmThreads = 256;
constexpr int kRmChunk = 256;  // channels per workgroup: 64 lanes x 4

struct RmAxis {
  float lo;     // first sample coordinate base (box edge * scale - offset)
  float bin;    // bin size
  int grid;     // samples per bin
  int n;        // samples on the axis (P * grid, 0 when grid <= 0)
};

__device__ __forceinline__ RmAxis rm_axis(float e0, float e1, float spatial_scale, int aligned, int P, int sampling_ratio) {
  const float offset = aligned ? 0.5f : 0.f;
  RmAxis a;
  a.lo = e0 * spatial_scale - offset;
  const float hi = e1 * spatial_scale - offset;
  float extent = hi - a.lo;
  if (!aligned) extent = fmaxf(extent, 1.f);
  a.bin = extent / (float)P;
  a.grid = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(extent / (float)P);
  a.n = a.grid > 0 ? P * a.grid : 0;
  return a;
}

// sample s of an axis -> its two pixel taps and weights (as `bilinear`: the coordinate expression of roi_align_kernel; a
// sample more than one pixel outside the map gets weights 0 on tap 0)
__device__ __forceinline__ void rm_sample(const RmAxis& a, int s, int L, int& low, int& high, float& wl, float& wh) {
  const int bin = s / a.grid, sub = s - bin * a.grid;
  float t = a.lo + (float)bin * a.bin + ((float)sub + 0.5f) * a.bin / (float)a.grid;
  if (!(t >= -1.0f && t <= (float)L)) {  // (also a NaN coordinate: never an index from it)
    low = high = 0;
    wl = wh = 0.f;
    return;
  }
  if (t <= 0.f) t = 0.f;
  low = (int)t;
  if (low >= L - 1) { high = low = L - 1; t = (float)low; } else { high = low + 1; }
  const float l = t - (float)low;
  wl = 1.f - l;
  wh = l;
}

// Dense per-pixel weights of one axis: thread t owns pixels t, t + 256, ...; samples staged 256 at a time.
__device__ void rm_axis_weights(const RmAxis& a, int L, double* __restrict__ w, int* __restrict__ s_lo, int* __restrict__ s_hi,
                                float* __restrict__ s_wl, float* __restrict__ s_wh) {
  const int tid = threadIdx.x;
  for (int p = tid; p < L; p += kRmThreads) w[p] = 0.0;
  for (int s0 = 0; s0 < a.n; s0 += kRmThreads) {
    const int cnt = min(kRmThreads, a.n - s0);
    __syncthreads();  // (the previous chunk's readers are done)
    if (tid < cnt) rm_sample(a, s0 + tid, L, s_lo[tid], s_hi[tid], s_wl[tid], s_wh[tid]);
    __syncthreads();
    for (int p = tid; p < L; p += kRmThreads) {
      double acc = w[p];
      for (int j = 0; j < cnt; ++j) {
        if (s_lo[j] == p) acc += (double)s_wl[j];
        if (s_hi[j] == p) acc += (double)s_wh[j];
      }
      w[p] = acc;
    }
  }
}

// rows / columns of non-zero weight, in order, by one wave
__device__ int rm_compact(const double* __restrict__ w, int L, int* __restrict__ idx, double* __restrict__ cw) {
  const int lane = threadIdx.x & 63;
  int n = 0;
  for (int base = 0; base < L; base += 64) {
    const int p = base + lane;
    const double v = p < L ? w[p] : 0.0;
    const bool nz = v != 0.0;
    const unsigned long long m = __ballot(nz);
    if (nz) {
      const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
      idx[pos] = p;
      cw[pos] = v;
    }
    n += __popcll(m);
  }
  return n;
}

template <bool VEC>
__device__ __forceinline__ void rm_load4(const float* __restrict__ px, int c0, int C, float v[4]) {
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(px + c0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = c0 + i < C ? px[c0 + i] : 0.f;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kRmThreads) void roi_means_kernel(const float* __restrict__ feat, const float* __restrict__ boxes,
                                                               const int* __restrict__ batch_idx, float* __restrict__ out,
                                                               int64_t ldo, int64_t K, int64_t B, int C, int H, int W,
                                                               int PH, int PW, float spatial_scale, int sampling_ratio,
                                                               int aligned, int n_chunks) {
  extern __shared__ double rm_lds[];
  double* wy = rm_lds;                                  // [H]
  double* wx = wy + H;                                  // [W]
  double* rw = wx + W;                                  // [H] compacted row weights
  double* cw = rw + H;                                  // [W]
  double* part = cw + W;                                // [3][64][4] partial sums of waves 1..3
  int* ridx = reinterpret_cast<int*>(part + 3 * 64 * 4);  // [H]
  int* cidx = ridx + H;                                 // [W]
  int* s_lo = cidx + W;                                 // [256] staged samples
  int* s_hi = s_lo + kRmThreads;
  float* s_wl = reinterpret_cast<float*>(s_hi + kRmThreads);
  float* s_wh = s_wl + kRmThreads;
  int* counts = reinterpret_cast<int*>(s_wh + kRmThreads);  // [2]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t total = K * (int64_t)n_chunks;
  for (int64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
    const int64_t k = blk / n_chunks;
    const int chunk = (int)(blk - k * n_chunks);
    const int c0 = chunk * kRmChunk + 4 * lane;
    float* orow = out + k * ldo;
    const int b = batch_idx ? batch_idx[k] : 0;
    const float* box = boxes + k * 4;
    const RmAxis ay = rm_axis(box[1], box[3], spatial_scale, aligned, PH, sampling_ratio);
    const RmAxis ax = rm_axis(box[0], box[2], spatial_scale, aligned, PW, sampling_ratio);
    if (b < 0 || b >= B || ay.n == 0 || ax.n == 0) {  // an image outside the batch, or no samples: a row of zeros
      if (wave == 0)
        for (int i = 0; i < 4; ++i)
          if (c0 + i < C) orow[c0 + i] = 0.f;
      continue;
    }
    const float* img = feat + (int64_t)b * H * W * C;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int np = 0;
#if ROI_MEANS_FORM == 0
    __syncthreads();  // (LDS of the previous box is free)
    rm_axis_weights(ay, H, wy, s_lo, s_hi, s_wl, s_wh);
    rm_axis_weights(ax, W, wx, s_lo, s_hi, s_wl, s_wh);
    __syncthreads();
    if (wave == 0) {
      const int n = rm_compact(wy, H, ridx, rw);
      if (lane == 0) counts[0] = n;
    } else if (wave == 1) {
      const int n = rm_compact(wx, W, cidx, cw);
      if (lane == 0) counts[1] = n;
    }
    __syncthreads();
    const int nr = counts[0], nc = counts[1];
    np = nr * nc;
    // this wave's contiguous quarter of the (row, column) pairs
    const int p0 = (int)((int64_t)np * wave / 4), p1 = (int)((int64_t)np * (wave + 1) / 4);
    if (c0 < C && p0 < p1) {
      int i = p0 / nc, j = p0 - (p0 / nc) * nc;
      for (int p = p0; p < p1; ++p) {
        const double wgt = rw[i] * cw[j];
        float v[4];
        rm_load4<VEC>(img + ((int64_t)ridx[i] * W + cidx[j]) * C, c0, C, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += wgt * (double)v[q];
        if (++j == nc) { j = 0; ++i; }
      }
    }
#else
    // direct form: every (sample row, sample column) pair, four taps
    __syncthreads();
    int* ylo = counts + 4;  // staged samples of both axes (at most 256 each), behind everything else
    int* yhi = ylo + kRmThreads;
    int* xlo = yhi + kRmThreads;
    int* xhi = xlo + kRmThreads;
    float* ywl = reinterpret_cast<float*>(xhi + kRmThreads);
    float* ywh = ywl + kRmThreads;
    float* xwl = ywh + kRmThreads;
    float* xwh = xwl + kRmThreads;
    const bool fits = ay.n <= kRmThreads && ax.n <= kRmThreads;
    if (fits && tid < ay.n) rm_sample(ay, tid, H, ylo[tid], yhi[tid], ywl[tid], ywh[tid]);
    if (fits && tid < ax.n) rm_sample(ax, tid, W, xlo[tid], xhi[tid], xwl[tid], xwh[tid]);
    __syncthreads();
    np = fits ? ay.n * ax.n : 0;
    const int p0 = (int)((int64_t)np * wave / 4), p1 = (int)((int64_t)np * (wave + 1) / 4);
    if (c0 < C && p0 < p1) {
      for (int p = p0; p < p1; ++p) {
        const int i = p / ax.n, j = p - (p / ax.n) * ax.n;
        const int ty[2] = {ylo[i], yhi[i]}, tx[2] = {xlo[j], xhi[j]};
        const float wyv[2] = {ywl[i], ywh[i]}, wxv[2] = {xwl[j], xwh[j]};
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            float v[4];
            rm_load4<VEC>(img + ((int64_t)ty[u] * W + tx[e]) * C, c0, C, v);
            const double wgt = (double)wyv[u] * (double)wxv[e];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += wgt * (double)v[q];
          }
      }
    }
    if (!fits) acc[0] = acc[1] = acc[2] = acc[3] = __builtin_nan("");
#endif
    if (wave > 0)
#pragma unroll
      for (int q = 0; q < 4; ++q) part[((wave - 1) * 64 + lane) * 4 + q] = acc[q];
    __syncthreads();
    if (wave == 0 && c0 < C) {
      const double scale = 1.0 / ((double)PH * (double)PW * (double)ay.grid * (double)ax.grid);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double s = acc[q];
        for (int w = 0; w < 3; ++w) s += part[(w * 64 + lane) * 4 + q];
        if (c0 + q < C) orow[c0 + q] = (float)(s * scale);
      }
    }
  }
}

}  // namespace

static size_t runia_roi_means_lds_bytes(int H, int W) {
  return (size_t)(2 * (H + W) + 3 * 64 * 4) * 8 + (size_t)(H + W) * 4 + (size_t)4 * kRmThreads * 4 + 16;
}

extern "C" int runia_roi_means_f32(const float* feat_nhwc, const float* boxes, const int* batch_idx, float* out, int64_t ldo,
                                   int64_t col_offset, int64_t K, int64_t B, int C, int H, int W, int PH, int PW,
                                   double spatial_scale, int sampling_ratio, int aligned, runia_stream_t stream) {
  if (K < 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || PH <= 0 || PW <= 0 || col_offset < 0) return RUNIA_E_INVALID;
  if (K > 0 && ldo < col_offset + C) return RUNIA_E_INVALID;
  if (H + W > RUNIA_ROI_MEANS_MAX_HW) return RUNIA_E_INVALID;
  if ((int64_t)H * W * C * 4 >= (int64_t)1 << 30) return RUNIA_E_INVALID;  // (the per-image limit of runia_roi_mc_entropy_f32)
  if (K == 0) return RUNIA_OK;
  if (!feat_nhwc || !boxes || !out) return RUNIA_E_INVALID;
  if (B > 1 && !batch_idx) return RUNIA_E_INVALID;
  const int n_chunks = (C + kRmChunk - 1) / kRmChunk;
  size_t lds = runia_roi_means_lds_bytes(H, W);
#if ROI_MEANS_FORM != 0
  lds += (size_t)8 * kRmThreads * 4 + 16;
#endif
  const unsigned grid = runia_stream_grid(K * n_chunks, 1);
  float* o = out + col_offset;
  const bool vec = (C % 4) == 0 && (reinterpret_cast<uintptr_t>(feat_nhwc) % 16) == 0;
  if (vec)
    roi_means_kernel<true><<<grid, kRmThreads, lds, as_stream(stream)>>>(feat_nhwc, boxes, batch_idx, o, ldo, K, B, C, H, W, PH,
                                                                         PW, (float)spatial_scale, sampling_ratio, aligned,
                                                                         n_chunks);
  else
    roi_means_kernel<false><<<grid, kRmThreads, lds, as_stream(stream)>>>(feat_nhwc, boxes, batch_idx, o, ldo, K, B, C, H, W, PH,
                                                                          PW, (float)spatial_scale, sampling_ratio, aligned,
                                                                          n_chunks);
  return runia_check_launch();
}
