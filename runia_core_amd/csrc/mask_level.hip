// Anomaly maps of a mask classifier (MaskFormer / Mask2Former): RbA, the max class score and its label, EAM, and the class
// scores themselves, from (G, Q, K [+ 1]) class logits and (G, Q, h, w) mask logits read where the model left them, upsampled
// to (H, W) inside the kernel.  The definition is in include/runia_hip.h.
//   runia_maskq_maps   two launches: the prologue (softmax rows -> the weight matrix of every image, the interpolation tables),
//                      then ONE launch that interpolates, applies the sigmoid, multiplies and reduces.
//
// The product.  S[k][pixel] = sum_q P[q][k] s[q][pixel] is, per image, a (K + 1) x Q by Q x pixels product (row K carries a[q] =
// max_k P[q][k] and gives EAM).  A 256-thread workgroup owns 128 consecutive pixels of ONE image (the weights differ per image:
// a tile never straddles two, the last tile of an image is short).  32 queries at a time, every thread interpolates and
// squashes its 16 values into Xs[q][pixel] (pixel_map.hpp's Xs; pitch 132) and the weights go to Ws[row][34]; on
// v_mfma_f32_32x32x2_f32 the weights are the A operand and s the B operand, so wave v holds pixels 32 v .. 32 v + 31 in its
// lanes and NT tiles of 32 rows in its accumulators (NT = 1, 2, 4, 8 for K + 1 <= 32, 64, 128, 256: one accumulator set, 128
// registers at most, no second pass over the interpolation).  The queries of a k-step are taken in ascending order: the first
// MFMA of a group of four takes q, q + 1 on the two lane halves, the second q + 2, q + 3 (Ws stores the middle two swapped so
// that one 8-byte read feeds both).
// The source.  At the identity size the chunk is read in pixel_map.hpp's three load forms (four pixels of a query plane per
// load; 16 queries of a pixel per thread for channels_last; element loads), all filling the same Xs.  Otherwise the four taps
// of a pixel are not neighbours of the next pixel's in memory: every tap is an element load through the strides, whatever
// the layout (the source is 1 / 16 of the output at 4 x and stays in L2), with the tap offsets and weights of a thread's four
// pixels in registers for the whole tile.
// The epilogue.  A lane holds, of its pixel, the rows with ((row >> 2) & 1) == lane >> 5.  It sums tanh and takes max / argmax
// over its rows in ascending order; the two halves are combined with one exchange in a fixed order (lower half first).  No
// atomics: the same call gives the same bits, and an output does not depend on which others are asked for.
#include "common.hpp"
#include "elem.hpp"
#include "pixel_map.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxK = RUNIA_MASKQ_MAX_CLASSES;
constexpr int kMaxQ = RUNIA_MASKQ_MAX_QUERIES;
constexpr int64_t kMaxSide = RUNIA_MASKQ_MAX_SIDE;
constexpr int64_t kMaxPixels = (int64_t)1 << RUNIA_MASKQ_MAX_PIXELS_LOG2;
constexpr int kLoadInterp = 3;  // beside pixel_map.hpp's three forms: bilinear taps, element loads

// ---- the prologue ---------------------------------------------------------------------------------------------------------------
struct PreArgs {
  const void* cls;
  int64_t cg, cq, ck;
  int Q, K, Kc, R32, Q32;
  int64_t soft_items;  // G * Q32
  unsigned soft_blocks;
  float* Wt;
  int32_t *ty0, *tx0;
  float *tly, *tlx;
  int H, W, h, w;
};

// n = max((2 i + 1) src - dst, 0) over 2 dst: the quotient and the remainder as one f32 division (both operands < 2^25: exact)
__device__ __forceinline__ void coord(int i, int dst, int src, int32_t& i0, float& l) {
  int64_t n = (2 * (int64_t)i + 1) * src - dst;
  n = n < 0 ? 0 : n;
  const int64_t d = 2 * (int64_t)dst;
  const int64_t q = n / d;
  i0 = (int32_t)q;
  l = (float)(n - q * d) / (float)d;
}

template <class T>
__global__ __launch_bounds__(256) void maskq_prologue_kernel(PreArgs a) {
  typedef typename T::elem E;
  if (blockIdx.x >= a.soft_blocks) {  // the tables
    const int64_t i = (int64_t)(blockIdx.x - a.soft_blocks) * 256 + threadIdx.x;
    if (i < a.H) coord((int)i, a.H, a.h, a.ty0[i], a.tly[i]);
    else if (i < (int64_t)a.H + a.W) coord((int)(i - a.H), a.W, a.w, a.tx0[i - a.H], a.tlx[i - a.H]);
    return;
  }
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= a.soft_items) return;
  const int64_t g = it / a.Q32;
  const int q = (int)(it - g * a.Q32);
  float* wt = a.Wt + g * a.R32 * a.Q32 + q;  // column q of the image's [R32][Q32] matrix
  if (q >= a.Q) {
    for (int r = 0; r < a.R32; ++r) wt[(int64_t)r * a.Q32] = 0.f;
    return;
  }
  const E* x = static_cast<const E*>(a.cls) + g * a.cg + (int64_t)q * a.cq;
  float m = ld1<T>(x);
  for (int j = 1; j < a.Kc; ++j) m = fmaxf(m, ld1<T>(x + j * a.ck));
  float sum = 0.f;
  for (int j = 0; j < a.Kc; ++j) sum += expf(ld1<T>(x + j * a.ck) - m);
  float best = 0.f;
  for (int k = 0; k < a.K; ++k) {
    const float p = expf(ld1<T>(x + k * a.ck) - m) / sum;
    wt[(int64_t)k * a.Q32] = p;
    if (k == 0 || (best == best && (p > best || p != p))) best = p;
  }
  wt[(int64_t)a.K * a.Q32] = best;
  for (int r = a.K + 1; r < a.R32; ++r) wt[(int64_t)r * a.Q32] = 0.f;
}

// ---- the main launch ------------------------------------------------------------------------------------------------------------
struct MainArgs {
  MapView v;                   // the mask logits (G, Q, h, w): v.C = Q (the identity forms read through it)
  int64_t sn, sc, sh, sw;      // its strides as given (the interpolating form)
  const float* Wt;
  int R32, Q32, K;
  const int32_t *ty0, *tx0;
  const float *tly, *tlx;
  int H, W, h, w;
  int64_t HW, tiles;           // output pixels and workgroups per image
  float *rba, *mx, *eam, *semseg;
  int32_t* label;
};

__device__ __forceinline__ float sigmoid(float u) { return __builtin_amdgcn_rcpf(1.0f + __expf(-u)); }

template <class T, int LOAD, int NT>
__global__ __launch_bounds__(256) void maskq_maps_kernel(MainArgs a) {
  typedef typename T::elem E;
  __shared__ __attribute__((aligned(16))) float Xs[kKCh][kXP];
  __shared__ __attribute__((aligned(16))) float Ws[NT * 32][kWP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int Q = a.v.C, K = a.K;
  const int64_t g = (int64_t)blockIdx.x / a.tiles;
  const int64_t t0 = ((int64_t)blockIdx.x - g * a.tiles) * kTP;  // the tile's first pixel inside image g
  const float* Wg = a.Wt + g * a.R32 * a.Q32;

  // what this thread stages: four neighbouring pixels (channels_last: one pixel) of the tile
  MapView v = a.v;
  v.P = (g + 1) * a.HW;  // the tile ends with its image
  int64_t off[4];
  int nv = 0;
  int32_t tap[4][4];
  float lx[4], ly[4];
  if constexpr (LOAD == kLoadInterp) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t pix = t0 + 4 * (tid & 31) + j;
      int32_t y0 = 0, x0 = 0;
      ly[j] = lx[j] = 0.f;
      if (pix < a.HW) {  // (a pixel past the image reads element (0, 0): its column of the product is never written)
        const int64_t Y = pix / a.W, X = pix - Y * a.W;
        y0 = a.ty0[Y];
        ly[j] = a.tly[Y];
        x0 = a.tx0[X];
        lx[j] = a.tlx[X];
      }
      const int32_t y1 = y0 + 1 < a.h ? y0 + 1 : a.h - 1, x1 = x0 + 1 < a.w ? x0 + 1 : a.w - 1;
      tap[j][0] = (int32_t)(y0 * a.sh + x0 * a.sw);
      tap[j][1] = (int32_t)(y0 * a.sh + x1 * a.sw);
      tap[j][2] = (int32_t)(y1 * a.sh + x0 * a.sw);
      tap[j][3] = (int32_t)(y1 * a.sh + x1 * a.sw);
    }
  } else {
    nv = staged_pixels<LOAD>(v, g * a.HW + t0, tid, off);
  }

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (int q0 = 0; q0 < a.Q32; q0 += kKCh) {
    __syncthreads();  // every wave has finished reading the previous chunk
    if constexpr (LOAD == kLoadInterp) {
      const E* xg = static_cast<const E*>(a.v.x) + g * a.sn;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = i * 8 + (tid >> 5), q = q0 + row;
        const E* xq = xg + (int64_t)(q < Q ? q : Q - 1) * a.sc;  // (a query past Q re-reads the last plane and is masked)
        float m[4][4], s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int c = 0; c < 4; ++c) m[j][c] = ld1<T>(xq + tap[j][c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float wx0 = 1.0f - lx[j], wy0 = 1.0f - ly[j];
          const float top = wx0 * m[j][0] + lx[j] * m[j][1];
          const float bot = wx0 * m[j][2] + lx[j] * m[j][3];
          s[j] = q < Q ? sigmoid(wy0 * top + ly[j] * bot) : 0.f;
        }
        *reinterpret_cast<float4*>(&Xs[row][4 * (tid & 31)]) = make_float4(s[0], s[1], s[2], s[3]);
      }
    } else if constexpr (LOAD == kLoadCLast) {
      float xr[16];
      load_x_cl<T>(v, off[0], nv > 0, q0, tid, xr);
      const int pix = tid >> 1, r0 = (tid & 1) * 16;
#pragma unroll
      for (int i = 0; i < 16; ++i) Xs[r0 + i][pix] = q0 + r0 + i < Q ? sigmoid(xr[i]) : 0.f;
    } else {
      float xr[16];
      load_x<T, LOAD == kLoadVec>(v, off, nv, q0, tid, xr);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = i * 8 + (tid >> 5);
        const bool in = q0 + row < Q;
        *reinterpret_cast<float4*>(&Xs[row][4 * (tid & 31)]) =
            make_float4(in ? sigmoid(xr[4 * i]) : 0.f, in ? sigmoid(xr[4 * i + 1]) : 0.f, in ? sigmoid(xr[4 * i + 2]) : 0.f,
                        in ? sigmoid(xr[4 * i + 3]) : 0.f);
      }
    }
    // the weights: NT * 32 rows x 32 queries, four queries per load; the middle two swapped (the k order of the steps below)
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int idx = tid + 256 * i, row = idx >> 3, c4 = idx & 7;
      const float4 wv = row < a.R32 ? *reinterpret_cast<const float4*>(Wg + (int64_t)row * a.Q32 + q0 + 4 * c4)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);  // (R32 = 96: the fourth tile of NT = 4 is empty)
      *reinterpret_cast<float2*>(&Ws[row][4 * c4]) = make_float2(wv.x, wv.z);
      *reinterpret_cast<float2*>(&Ws[row][4 * c4 + 2]) = make_float2(wv.y, wv.w);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kKCh / 4; ++s) {
      const float bx = Xs[4 * s + lh][wave * 32 + li], by = Xs[4 * s + 2 + lh][wave * 32 + li];
      float2 av[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) av[t] = *reinterpret_cast<const float2*>(&Ws[t * 32 + li][4 * s + 2 * lh]);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t * 32 >= a.R32) continue;  // (uniform: an empty tile stays zero)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].x, bx, acc[t], 0, 0, 0);  // q = 4 s + lh
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].y, by, acc[t], 0, 0, 0);  // q = 4 s + 2 + lh
      }
    }
  }

  // acc[t][r] = S[32 t + (r & 3) + 8 (r >> 2) + 4 lh] of pixel wave * 32 + li
  const int64_t pm = t0 + wave * 32 + li;
  const bool mine = pm < a.HW;
  float th = 0.f, best = 0.f, ev = 0.f;
  int bi = -1;
  bool bad = false;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float sv = acc[t][r];
      if (row < K) {
        if (a.rba) th += tanhf(sv);
        bad = bad || sv != sv;
        if (bi < 0 || sv > best) {
          best = sv;
          bi = row;
        }
        if (a.semseg && mine) a.semseg[(g * K + row) * a.HW + pm] = sv;
      }
      if (row == K) ev = sv;
    }
  // the other half of the wave holds the other rows of the same pixel
  const float th_o = __shfl_xor(th, 32, 64), best_o = __shfl_xor(best, 32, 64);
  const int bi_o = __shfl_xor(bi, 32, 64);
  const bool bad_o = __shfl_xor(bad ? 1 : 0, 32, 64) != 0;
  ev = __shfl(ev, li + 32 * ((K >> 2) & 1), 64);
  const float th_sum = lh == 0 ? th + th_o : th_o + th;  // lower half first, on both halves
  if (bi_o >= 0 && (bi < 0 || best_o > best || (best_o == best && bi_o < bi))) {
    best = best_o;
    bi = bi_o;
  }
  bad = bad || bad_o;
  if (!mine) return;
  const int64_t po = g * a.HW + pm;
  if (lh == 0) {
    if (a.rba) a.rba[po] = -th_sum;
    if (a.mx) a.mx[po] = bad ? __builtin_nanf("") : best;
  } else {
    if (a.label) a.label[po] = bad ? -1 : bi;
    if (a.eam) a.eam[po] = -ev;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct Plan {
  float* Wt;
  int32_t *ty0, *tx0;
  float *tly, *tlx;
};

int rows32(int64_t K) { return (int)round_up((size_t)K + 1, 32); }

Plan plan_ws(WsWalk& w, int64_t G, int64_t Q, int64_t K, int64_t H, int64_t W, bool ident) {
  Plan p = {};
  p.Wt = w.take<float>((size_t)G * rows32(K) * round_up((size_t)Q, 32), 16);
  if (!ident) {
    p.ty0 = w.take<int32_t>((size_t)H, 16);
    p.tly = w.take<float>((size_t)H, 16);
    p.tx0 = w.take<int32_t>((size_t)W, 16);
    p.tlx = w.take<float>((size_t)W, 16);
  }
  return p;
}

bool sizes_ok(int64_t G, int64_t Q, int64_t K, int64_t H, int64_t W, int64_t h, int64_t w) {
  if (K < 1 || K > kMaxK || Q < 1 || Q > kMaxQ || G < 0 || G > kLim) return false;
  if (H < 0 || W < 0 || h < 0 || w < 0 || H > kMaxSide || W > kMaxSide || h > kMaxSide || w > kMaxSide) return false;
  if (G > 0 && H * W > 0) {
    if (h * w == 0 || G * H * W > kMaxPixels || G * ((H * W + kTP - 1) / kTP) > kLim) return false;
  }
  return true;
}

template <class T, int LOAD>
int launch_main(const MainArgs& a, unsigned grid, hipStream_t s) {
  if (a.R32 <= 32) maskq_maps_kernel<T, LOAD, 1><<<grid, 256, 0, s>>>(a);
  else if (a.R32 <= 64) maskq_maps_kernel<T, LOAD, 2><<<grid, 256, 0, s>>>(a);
  else if (a.R32 <= 128) maskq_maps_kernel<T, LOAD, 4><<<grid, 256, 0, s>>>(a);
  else maskq_maps_kernel<T, LOAD, 8><<<grid, 256, 0, s>>>(a);
  return runia_check_launch();
}

}  // namespace

extern "C" int64_t runia_maskq_workspace_bytes(int64_t G, int64_t Q, int64_t K, int64_t H, int64_t W, int64_t h, int64_t w) {
  if (!sizes_ok(G, Q, K, H, W, h, w) || G == 0 || H * W == 0) return 0;
  return (int64_t)ws_bytes([&](WsWalk& wk) { plan_ws(wk, G, Q, K, H, W, H == h && W == w); });
}

extern "C" int runia_maskq_maps(const void* class_logits, int class_dtype, int64_t cg, int64_t cq, int64_t ck, int has_void,
                                const void* mask_logits, int mask_dtype, int64_t G, int64_t Q, int64_t K, int64_t h, int64_t w,
                                int64_t sn, int64_t sc, int64_t sh, int64_t sw, int64_t H, int64_t W, float* rba,
                                float* max_score, int32_t* label, float* eam, float* semseg, void* workspace,
                                size_t workspace_bytes, runia_stream_t stream) {
  if (!elem_dtype_ok(class_dtype) || !elem_dtype_ok(mask_dtype) || !sizes_ok(G, Q, K, H, W, h, w) || cg < 0 || cq < 0 || ck < 0 ||
      sn < 0 || sc < 0 || sh < 0 || sw < 0)
    return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;
  if (!view_ok(G, Q, h, w, sn, sc, sh, sw) || (h - 1) * sh + (w - 1) * sw > kLim) return RUNIA_E_INVALID;
  if (!class_logits || !mask_logits || (!rba && !max_score && !label && !eam && !semseg)) return RUNIA_E_INVALID;
  const bool ident = H == h && W == w;
  const size_t need = (size_t)runia_maskq_workspace_bytes(G, Q, K, H, W, h, w);
  if (ws_refused(workspace, workspace_bytes, need, 16)) return RUNIA_E_WORKSPACE;
  WsWalk walk(workspace);
  const Plan p = plan_ws(walk, G, Q, K, H, W, ident);
  hipStream_t s = as_stream(stream);

  PreArgs pa;
  pa.cls = class_logits;
  pa.cg = cg; pa.cq = cq; pa.ck = ck;
  pa.Q = (int)Q;
  pa.K = (int)K;
  pa.Kc = (int)K + (has_void ? 1 : 0);
  pa.R32 = rows32(K);
  pa.Q32 = (int)round_up((size_t)Q, 32);
  pa.soft_items = G * pa.Q32;
  pa.soft_blocks = (unsigned)((pa.soft_items + 255) / 256);
  pa.Wt = p.Wt;
  pa.ty0 = p.ty0; pa.tx0 = p.tx0; pa.tly = p.tly; pa.tlx = p.tlx;
  pa.H = (int)H; pa.W = (int)W; pa.h = (int)h; pa.w = (int)w;
  const unsigned table_blocks = ident ? 0u : (unsigned)((H + W + 255) / 256);
  dispatch_elem(class_dtype, [&](auto t) {
    maskq_prologue_kernel<decltype(t)><<<pa.soft_blocks + table_blocks, 256, 0, s>>>(pa);
    return 0;
  });
  if (int rc = runia_check_launch()) return rc;

  MainArgs a;
  a.v = make_view(mask_logits, G, Q, h, w, sn, sc, sh, sw);
  a.sn = sn; a.sc = sc; a.sh = sh; a.sw = sw;
  a.Wt = p.Wt;
  a.R32 = pa.R32; a.Q32 = pa.Q32; a.K = (int)K;
  a.ty0 = p.ty0; a.tx0 = p.tx0; a.tly = p.tly; a.tlx = p.tlx;
  a.H = (int)H; a.W = (int)W; a.h = (int)h; a.w = (int)w;
  a.HW = H * W;
  a.tiles = (a.HW + kTP - 1) / kTP;
  a.rba = rba; a.mx = max_score; a.eam = eam; a.semseg = semseg; a.label = label;
  const unsigned grid = (unsigned)(G * a.tiles);
  return dispatch_elem(mask_dtype, [&](auto t) {
    typedef decltype(t) T;
    if (!ident) return launch_main<T, kLoadInterp>(a, grid, s);
    if (view_allows_vec(a.v, G, h, T::kBytes)) return launch_main<T, kLoadVec>(a, grid, s);
    if (view_allows_clast(a.v, G, h, T::V)) return launch_main<T, kLoadCLast>(a, grid, s);
    return launch_main<T, kLoadElem>(a, grid, s);
  });
}
