// runia_mcd_reduce_rows: the reduction MCDSamplesExtractor applies to the hooked activation after every stochastic forward
// pass (reference feature_extraction/image_level.py:366-410: mean(dim=3).mean(dim=2) / mean(dim=3) / avg_pool2d / squeeze,
// then reshape(1, -1) and two levels of torch.cat), written straight into the pass's rows of the (B * mcd, D) sample table.
//
// Every mode is an average pooling with a rectangular window (divisor kh*kw, padding counted, floor): fullmean = window
// (H, W); mean = window (1, W); avgpool = (k, k) stride s padding p; copy = (1, 1).  The map is read in the dtype and with
// the strides the model produced.  Five kernels, picked on the host from the strides:
//   unit stride along W, window spans whole rows (fullmean, mean):
//     mcd_seg_wave_kernel     2^k lanes (<= 64) per output, 16-byte loads over the 16-byte aligned body of each row
//                             segment, scalar head and tail, shuffle reduction - many small maps (512 x 7 x 7)
//     mcd_plane_block_kernel  one workgroup (512 or 1024 threads) per output - few large maps (256 x 128 x 256)
//   unit stride along C (channels_last), 16-byte aligned pixels:
//     mcd_cl_reduce_kernel    fullmean: lanes along C (16 bytes each), pixel slots across the rest of the workgroup, LDS sum
//                             over the slots; with few images, or more than 512 pixels per slot, the pixels of an image
//                             are split over S workgroups whose partial means are added with float atomics into rows
//                             zeroed by mcd_zero_rows_kernel
//     mcd_cl_pool_kernel      mean / avgpool / copy: one thread per (output position, 16 bytes of channels)
//   anything else:  mcd_elem_kernel, one thread per output value, scalar loads, any strides.
// f32 accumulation; f16 / bf16 are widened exactly.  Plain stores (and float atomics in the split case) only.
#include "common.hpp"
#include "elem.hpp"

namespace {

struct McdArgs {
  const void* x;
  float* out;
  int64_t sb, sc, sh, sw;  // element strides of the (B, C, H, W) view
  int64_t ld, row0, row_step;
  int B, C, H, W;
  int kh, kw, sth, stw, ph, pw, OH, OW;
  float div;  // kh * kw
};

template <class T>
__device__ __forceinline__ float sum16(const typename T::elem* p) {
  float v[T::V];
  ld16<T>(p, v);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < T::V; j += 2) s += v[j] + v[j + 1];
  return s;
}

// Sum of n contiguous elements at p by lanes g = 0 .. G-1 (each lane's share): scalar loads up to the first 16-byte
// boundary and after the last one, 16-byte loads in between, four independent loads in flight per lane.
template <class T>
__device__ __forceinline__ float seg_sum(const typename T::elem* p, int64_t n, int g, int G) {
  constexpr int V = T::V;
  const int64_t a = (int64_t)(reinterpret_cast<uintptr_t>(p) / sizeof(typename T::elem));
  int64_t head = (V - (a % V)) % V;
  if (head > n) head = n;
  const int64_t nv = (n - head) / V, tail0 = head + nv * V;
  float acc = 0.f;
  for (int64_t i = g; i < head; i += G) acc += ld1<T>(p + i);
  for (int64_t i = tail0 + g; i < n; i += G) acc += ld1<T>(p + i);
  const typename T::elem* pv = p + head;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int64_t v = g;
  for (; v + 3 * (int64_t)G < nv; v += 4 * (int64_t)G) {
    const float t0 = sum16<T>(pv + v * V), t1 = sum16<T>(pv + (v + G) * V);
    const float t2 = sum16<T>(pv + (v + 2 * (int64_t)G) * V), t3 = sum16<T>(pv + (v + 3 * (int64_t)G) * V);
    s0 += t0; s1 += t1; s2 += t2; s3 += t3;
  }
  for (; v < nv; v += G) s0 += sum16<T>(pv + v * V);
  return acc + ((s0 + s1) + (s2 + s3));
}

__device__ __forceinline__ float* out_row(const McdArgs& a, int64_t b) { return a.out + (a.row0 + b * a.row_step) * a.ld; }

// ---- unit stride along W, whole-row windows ------------------------------------------------------------------------------
// item = (b, c, oh): rows oh*sth .. oh*sth + kh - 1 of plane (b, c), seen as `nrows` segments of `rowlen` elements
// (nrows = 1 when the rows of the window are contiguous).  team = 2^team_log2 lanes per item.
template <class T>
__global__ __launch_bounds__(256) void mcd_seg_wave_kernel(McdArgs a, int team_log2, int nrows, int64_t rowlen,
                                                            int64_t items) {
  const typename T::elem* x = static_cast<const typename T::elem*>(a.x);
  const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int team = 1 << team_log2, g = (int)(gt & (team - 1));
  const int64_t item = gt >> team_log2;
  const bool live = item < items;
  float acc = 0.f;
  int64_t b = 0, c = 0, oh = 0;
  if (live) {
    oh = item % a.OH;
    const int64_t bc = item / a.OH;
    c = bc % a.C;
    b = bc / a.C;
    const typename T::elem* p = x + b * a.sb + c * a.sc + (oh * a.sth) * a.sh;
    for (int r = 0; r < nrows; ++r) acc += seg_sum<T>(p + r * a.sh, rowlen, g, team);
  }
  for (int o = team >> 1; o; o >>= 1) acc += __shfl_xor(acc, o);  // (a run-time team width: stays a loop)
  if (live && g == 0) out_row(a, b)[c * a.OH + oh] = acc / a.div;
}

template <class T>
__global__ __launch_bounds__(1024) void mcd_plane_block_kernel(McdArgs a, int nrows, int64_t rowlen) {
  __shared__ float part[16];
  const typename T::elem* x = static_cast<const typename T::elem*>(a.x);
  const int64_t item = blockIdx.x;
  const int64_t oh = item % a.OH, bc = item / a.OH, c = bc % a.C, b = bc / a.C;
  const typename T::elem* p = x + b * a.sb + c * a.sc + (oh * a.sth) * a.sh;
  const int tid = threadIdx.x, nthr = blockDim.x;
  float acc = 0.f;
  if (nrows == 1) {
    acc = seg_sum<T>(p, rowlen, tid, nthr);
  } else {  // one wave per row
    for (int r = tid >> 6; r < nrows; r += nthr >> 6) acc += seg_sum<T>(p + r * a.sh, rowlen, tid & 63, 64);
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int w = 0; w < (nthr >> 6); ++w) s += part[w];
    out_row(a, b)[c * a.OH + oh] = s / a.div;
  }
}

// ---- unit stride along C ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mcd_zero_rows_kernel(McdArgs a, int64_t D) {
  const int64_t n = (int64_t)a.B * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out_row(a, i / D)[i % D] = 0.f;
}

// fullmean.  Workgroup = (image b, channel chunk, pixel split s of S); thread = (ct: 16 bytes of channels, ps: pixel slot).
template <class T>
__global__ __launch_bounds__(256) void mcd_cl_reduce_kernel(McdArgs a, int ct_log2, int nchunk, int S, int flat) {
  constexpr int V = T::V;
  __shared__ float sm[256 * V];
  const typename T::elem* x = static_cast<const typename T::elem*>(a.x);
  const int64_t blk = blockIdx.x;
  const int s = (int)(blk % S), chunk = (int)((blk / S) % nchunk);
  const int64_t b = blk / ((int64_t)S * nchunk);
  const int t = threadIdx.x, CT = 1 << ct_log2, PS = 256 >> ct_log2;
  const int ct = t & (CT - 1), ps = t >> ct_log2;
  const int64_t c0 = ((int64_t)chunk * CT + ct) * V;
  const int nval = c0 >= a.C ? 0 : (a.C - c0 < V ? (int)(a.C - c0) : V);
  const int64_t npix = (int64_t)a.H * a.W, lo = npix * s / S, hi = npix * (s + 1) / S;
  const typename T::elem* base = x + b * a.sb + c0;  // sc == 1
  auto pix = [&](int64_t i) -> int64_t {
    if (flat) return i * a.sw;
    const int64_t h = i / a.W;
    return h * a.sh + (i - h * a.W) * a.sw;
  };
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (nval == V) {
    int64_t i = lo + ps;
    for (; i + 3 * (int64_t)PS < hi; i += 4 * (int64_t)PS) {
      float v0[V], v1[V], v2[V], v3[V];
      ld16<T>(base + pix(i), v0);
      ld16<T>(base + pix(i + PS), v1);
      ld16<T>(base + pix(i + 2 * PS), v2);
      ld16<T>(base + pix(i + 3 * PS), v3);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += (v0[j] + v1[j]) + (v2[j] + v3[j]);
    }
    for (; i < hi; i += PS) {
      float v0[V];
      ld16<T>(base + pix(i), v0);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += v0[j];
    }
  } else if (nval > 0) {  // the last, partial group of channels
    for (int64_t i = lo + ps; i < hi; i += PS) {
      const typename T::elem* p = base + pix(i);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (j < nval) acc[j] += ld1<T>(p + j);
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) sm[t * V + j] = acc[j];  // [ps][ct * V + j]
  __syncthreads();
  const int width = CT * V;
  float* row = out_row(a, b);
  for (int idx = t; idx < width; idx += 256) {
    float sum = 0.f;
    for (int q = 0; q < PS; ++q) sum += sm[q * width + idx];
    const int64_t c = (int64_t)chunk * width + idx;
    if (c < a.C) {
      if (S > 1) atomicAdd(row + c, sum / a.div);
      else row[c] = sum / a.div;
    }
  }
}

// mean / avgpool / copy.  A wave = 8 neighbouring output columns x 8 neighbouring 16-byte channel groups: 128-byte runs on
// the read side, 32-byte runs on the write side.
template <class T>
__global__ __launch_bounds__(256) void mcd_cl_pool_kernel(McdArgs a, int64_t total) {
  constexpr int V = T::V;
  const typename T::elem* x = static_cast<const typename T::elem*>(a.x);
  const int64_t cv = (a.C + V - 1) / V, cvh_n = (cv + 7) / 8, owb_n = (a.OW + 7) / 8;
  for (int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x; gt < total; gt += (int64_t)gridDim.x * 256) {
    const int cl = (int)(gt & 7), owi = (int)((gt >> 3) & 7);
    int64_t rest = gt >> 6;
    const int64_t cvi = (rest % cvh_n) * 8 + cl;
    rest /= cvh_n;
    const int64_t ow = (rest % owb_n) * 8 + owi;
    rest /= owb_n;
    const int64_t oh = rest % a.OH, b = rest / a.OH;
    if (cvi >= cv || ow >= a.OW) continue;
    const int64_t c0 = cvi * V;
    const int nval = a.C - c0 < V ? (int)(a.C - c0) : V;
    const typename T::elem* base = x + b * a.sb + c0;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    const int64_t h0 = oh * a.sth - a.ph, w0 = ow * a.stw - a.pw;
    for (int y = 0; y < a.kh; ++y) {
      const int64_t ih = h0 + y;
      if (ih < 0 || ih >= a.H) continue;
      for (int z = 0; z < a.kw; ++z) {
        const int64_t iw = w0 + z;
        if (iw < 0 || iw >= a.W) continue;
        const typename T::elem* p = base + ih * a.sh + iw * a.sw;
        if (nval == V) {
          float v[V];
          ld16<T>(p, v);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] += v[j];
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (j < nval) acc[j] += ld1<T>(p + j);
        }
      }
    }
    float* row = out_row(a, b);
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (j < nval) row[((c0 + j) * a.OH + oh) * a.OW + ow] = acc[j] / a.div;
  }
}

// ---- any strides ----------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void mcd_elem_kernel(McdArgs a, int64_t D, int64_t total) {
  const typename T::elem* x = static_cast<const typename T::elem*>(a.x);
  for (int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x; gt < total; gt += (int64_t)gridDim.x * 256) {
    const int64_t d = gt % D, b = gt / D;
    const int64_t ow = d % a.OW, oh = (d / a.OW) % a.OH, c = d / ((int64_t)a.OW * a.OH);
    const typename T::elem* base = x + b * a.sb + c * a.sc;
    const int64_t h0 = oh * a.sth - a.ph, w0 = ow * a.stw - a.pw;
    float acc = 0.f;
    for (int y = 0; y < a.kh; ++y) {
      const int64_t ih = h0 + y;
      if (ih < 0 || ih >= a.H) continue;
      for (int z = 0; z < a.kw; ++z) {
        const int64_t iw = w0 + z;
        if (iw >= 0 && iw < a.W) acc += ld1<T>(base + ih * a.sh + iw * a.sw);
      }
    }
    out_row(a, b)[d] = acc / a.div;
  }
}

int ceil_log2(int64_t v) {
  int l = 0;
  while (((int64_t)1 << l) < v) ++l;
  return l;
}

constexpr int64_t kPlaneBlockBytes = 32 * 1024;  // a window of at least this many bytes gets a workgroup of its own
constexpr int64_t kClTargetBlocks = 512;         // workgroups wanted before the pixels of an image stop being split
constexpr int64_t kClMaxSlotPixels = 512;        // pixels one slot sums in sequence at most (128 chained f32 additions)

template <class T>
int launch(const McdArgs& a, hipStream_t s) {
  constexpr int V = T::V;
  const int64_t esz = sizeof(typename T::elem);
  const int64_t D = (int64_t)a.C * a.OH * a.OW, total = (int64_t)a.B * D;
  const bool whole_rows = a.pw == 0 && a.ph == 0 && a.kw == a.W && a.OW == 1;
  const bool whole_map = whole_rows && a.kh == a.H;  // then OH == 1
  if (whole_rows && (a.sw == 1 || a.W == 1)) {
    const bool joined = a.kh == 1 || a.sh == a.W;  // the rows of a window follow one another in memory
    const int nrows = joined ? 1 : a.kh;
    const int64_t rowlen = joined ? (int64_t)a.kh * a.W : a.W;
    const int64_t items = (int64_t)a.B * a.C * a.OH, bytes = (int64_t)a.kh * a.W * esz;
    if (bytes >= kPlaneBlockBytes && items <= 0x7fffffffll) {
      const int threads = bytes >= 4 * kPlaneBlockBytes ? 1024 : 512;
      mcd_plane_block_kernel<T><<<(unsigned)items, threads, 0, s>>>(a, nrows, rowlen);
      return runia_check_launch();
    }
    int64_t vecs = (rowlen + V - 1) / V;
    if (vecs > 64) vecs = 64;
    const int team_log2 = ceil_log2(vecs);
    const int64_t blocks = ((items << team_log2) + 255) / 256;
    if (blocks > 0x7fffffffll) return RUNIA_E_INVALID;
    mcd_seg_wave_kernel<T><<<(unsigned)blocks, 256, 0, s>>>(a, team_log2, nrows, rowlen, items);
    return runia_check_launch();
  }
  auto vec_ok = [&](int64_t stride, int extent) { return extent == 1 || stride % V == 0; };
  const bool cl = a.sc == 1 && a.C >= V && reinterpret_cast<uintptr_t>(a.x) % 16 == 0 && vec_ok(a.sb, a.B) &&
                  vec_ok(a.sh, a.H) && vec_ok(a.sw, a.W);
  if (cl && whole_map) {
    const int64_t cv = ((int64_t)a.C + V - 1) / V;
    const int ct_log2 = ceil_log2(cv > 256 ? 256 : cv);
    const int CT = 1 << ct_log2, PS = 256 / CT;
    const int64_t nchunk = (cv + CT - 1) / CT, npix = (int64_t)a.H * a.W;
    int64_t S = (kClTargetBlocks + a.B * nchunk - 1) / (a.B * nchunk);
    const int64_t most = npix / (4 * (int64_t)PS);  // at least four pixels per slot
    if (S > most) S = most;
    // a slot adds its pixels one after another (in groups of four): keep that chain short whatever the batch size
    const int64_t chain = (npix + kClMaxSlotPixels * PS - 1) / (kClMaxSlotPixels * PS);
    if (S < chain) S = chain;
    if (S < 1) S = 1;
    const int64_t blocks = (int64_t)a.B * nchunk * S;
    if (blocks > 0x7fffffffll) return RUNIA_E_INVALID;
    if (S > 1) {
      mcd_zero_rows_kernel<<<runia_stream_grid(total, 256), 256, 0, s>>>(a, D);
      if (runia_check_launch() != RUNIA_OK) return RUNIA_E_LAUNCH;
    }
    const int flat = a.H == 1 || a.sh == a.W * a.sw;
    mcd_cl_reduce_kernel<T><<<(unsigned)blocks, 256, 0, s>>>(a, ct_log2, (int)nchunk, (int)S, flat);
    return runia_check_launch();
  }
  if (cl) {
    const int64_t cv = ((int64_t)a.C + V - 1) / V;
    const int64_t threads = (int64_t)a.B * a.OH * ((a.OW + 7) / 8) * ((cv + 7) / 8) * 64;
    mcd_cl_pool_kernel<T><<<runia_stream_grid(threads, 256), 256, 0, s>>>(a, threads);
    return runia_check_launch();
  }
  mcd_elem_kernel<T><<<runia_stream_grid(total, 256), 256, 0, s>>>(a, D, total);
  return runia_check_launch();
}

}  // namespace

extern "C" int runia_mcd_reduce_rows(const void* x, int dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t sb,
                                     int64_t sc, int64_t sh, int64_t sw, int mode, int kernel, int stride, int padding,
                                     float* table, int64_t table_rows, int64_t ld, int64_t row0, int64_t row_step,
                                     runia_stream_t stream) {
  const int64_t lim = 0x7fffffffll;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0 || B > lim || C > lim || H > lim || W > lim || !elem_dtype_ok(dtype) ||
      sb < 0 || sc < 0 || sh < 0 || sw < 0 || table_rows < 0 || ld < 0 || row0 < 0 || row_step < 0)
    return RUNIA_E_INVALID;
  McdArgs a;
  a.x = x; a.out = table;
  a.sb = sb; a.sc = sc; a.sh = sh; a.sw = sw;
  a.ld = ld; a.row0 = row0; a.row_step = row_step;
  a.B = (int)B; a.C = (int)C; a.H = (int)H; a.W = (int)W;
  a.ph = a.pw = 0;
  switch (mode) {
    case RUNIA_MCD_FULLMEAN: a.kh = a.sth = a.H; a.kw = a.stw = a.W; break;
    case RUNIA_MCD_MEAN: a.kh = a.sth = 1; a.kw = a.stw = a.W; break;
    case RUNIA_MCD_COPY: a.kh = a.sth = 1; a.kw = a.stw = 1; break;
    case RUNIA_MCD_AVGPOOL:
      // torch.nn.functional.avg_pool2d: "pad should be at most half of effective kernel size"
      if (kernel <= 0 || stride <= 0 || padding < 0 || 2 * (int64_t)padding > kernel) return RUNIA_E_INVALID;
      a.kh = a.kw = kernel; a.sth = a.stw = stride; a.ph = a.pw = padding;
      if (H + 2 * (int64_t)padding < kernel || W + 2 * (int64_t)padding < kernel) return RUNIA_E_INVALID;
      break;
    default: return RUNIA_E_INVALID;
  }
  a.OH = (int)((H + 2 * (int64_t)a.ph - a.kh) / a.sth + 1);
  a.OW = (int)((W + 2 * (int64_t)a.pw - a.kw) / a.stw + 1);
  a.div = (float)a.kh * (float)a.kw;
  const int64_t D = (int64_t)a.C * a.OH * a.OW;
  if (D > lim * 64) return RUNIA_E_INVALID;
  if (B == 0) return RUNIA_OK;
  if (!x || !table || ld < D || (B > 1 && row_step < 1) || row0 + (B - 1) * row_step >= table_rows) return RUNIA_E_INVALID;
  return dispatch_elem(dtype, [&](auto t) { return launch<decltype(t)>(a, as_stream(stream)); });
}
