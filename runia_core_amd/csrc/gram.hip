// runia_gram_layer: the Gram-matrix OoD statistics of Sastry & Oore (ICML 2020) of one hooked activation, without the
// (B, C, C) Gram matrices.  The recipe sums the rows of G_p = F^p (F^p)^T; that row sum is
//   t[b,p,c] = sum_x F[b,c,x]^p S_p[b,x],   S_p[b,x] = sum_j F[b,j,x]^p,   v = sign(t) |t|^(1/p),   p = 1 .. P <= 16:
// one read of the map and ~4P flops an element.  The map (B, C, H, W) is read where it lies (f32 / f16 / bf16, any strides).
//
// Main launch, gram_tile_kernel: 512 threads per workgroup = (image, kTilePositions consecutive pixels), taken as tiles
// of X pixels (X = 8, 16 or 32, from C and the element size alone: nothing depends on the batch, so an image's bits do
// not depend on its neighbours).  A tile's C x X block is staged once in LDS in the map's own element type with an odd
// word pitch.  Up to 1 024 channels (two per thread in pass B; eight per thread spilled registers) are staged at once;
// wider layers go through the block in chunks of 1 024 channels at X = 32, twice (the second read of a chunk comes from
// the cache), one tile per workgroup.
//   staging  lines of contiguous elements - a channel's pixels when the plane is flat with unit stride, a pixel's channels
//            when sc == 1 - are cut at 16-byte addresses: head and tail by element loads, the body by 16-byte loads;
//            any other view by element loads.  Pixels past the map are zeros (0^p adds nothing).
//   pass A   thread = (pixel x, channel slice): S_p[x] over its channels by repeated multiplication, P sums in registers;
//            the slices of a wave by a butterfly, the 8 waves through LDS in wave order.
//   pass B   GB lanes own two channels and add F^p S_p over their
//            pixel quads into P registers, across all tiles of the workgroup; the lanes of a channel by a butterfly.
//   The (P, C) partial of the workgroup goes to the workspace with plain stores.  No matrix instruction: the left
//   operand of the product changes with p, the work is 4P flops per element read.
// Finish launch: adds an image's partials in workgroup order, takes the signed root (p = 1, 2, 4, 8, 16 by sqrt chains,
//   else exp2(log2|t| / p)), and STATS writes v (B, P, C); FIT folds v into the ordered-key tables of class label[b] with
//   integer atomicMin / atomicMax (order-free: the same bits every run); SCORE adds the deviation over (p, c) in a fixed
//   order, one f32 per image, and never writes v.
#include "common.hpp"
#include "elem.hpp"

namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;  // of the main launch: 256 registers a thread
constexpr int kScoreThreads = 1024, kScoreWaves = kScoreThreads / 64;
constexpr int kMaxP = RUNIA_GRAM_MAX_POWERS;
constexpr int kMinX = 8, kMaxX = 32;
constexpr int kKch = 2;                         // channels of one thread in pass B
constexpr int kChunk = kKch * kThreads;         // channels staged at once at most
constexpr int64_t kStageTarget = 48 * 1024;     // stage bytes up to which X grows (two workgroups per compute unit)
constexpr int64_t kStageTargetWide = 136 * 1024;  // ... of a chunked layer: its partials leave per tile, so the widest tile
constexpr int kTilePositions = 128;             // pixels of one workgroup (its tiles share the pass-B registers)

struct GramPlan {
  int X, lx, pitch;   // tile width, its log2, elements between the LDS rows of two channels
  int chunk, nchunk;  // channels staged at once, number of such chunks
  int tpw;            // tiles per workgroup
  int64_t ntw;        // workgroups per image
  int gb;             // pass B: lanes per channel
  int mode;           // staging: 0 element loads, 1 lines along the pixels, 2 lines along the channels
  int64_t ps;         // element stride between two pixels of a flat plane (mode 1: 1)
  size_t lds;         // dynamic LDS bytes
};

int pad_of(int esz) { return 4 / esz; }  // one 32-bit word

GramPlan make_plan(int dtype, int64_t C, int64_t H, int64_t W, int64_t sc, int64_t sh, int64_t sw, int P) {
  const int esz = dtype == kF32 ? 4 : 2;
  GramPlan g;
  g.chunk = (int)(C < kChunk ? C : kChunk);
  g.nchunk = (int)((C + g.chunk - 1) / g.chunk);
  g.X = kMaxX;
  while (g.X > kMinX && g.chunk * (g.X + pad_of(esz)) * esz > (g.nchunk > 1 ? kStageTargetWide : kStageTarget)) g.X >>= 1;
  g.lx = g.X == 8 ? 3 : (g.X == 16 ? 4 : 5);
  g.pitch = g.X + pad_of(esz);
  g.tpw = g.nchunk > 1 ? 1 : kTilePositions / g.X;
  const int64_t HW = H * W, ntiles = (HW + g.X - 1) / g.X;
  g.ntw = (ntiles + g.tpw - 1) / g.tpw;
  g.gb = 1;
  while (g.gb * 2 <= g.X / 4 && (kThreads / (g.gb * 2)) * kKch >= g.chunk) g.gb *= 2;
  const bool flat = H == 1 || W == 1 || sh == W * sw;
  g.ps = W == 1 ? sh : sw;
  const int V = 16 / esz;
  if (sc == 1 && C >= V) g.mode = 2;
  else if (flat && (g.ps == 1 || HW == 1)) g.mode = 1;
  else g.mode = 0;
  g.lds = (size_t)g.chunk * g.pitch * esz;
  g.lds = round_up(g.lds, 16) + (size_t)(kWaves + 1) * P * g.X * sizeof(float);
  return g;
}

struct GramArgs {
  const void* x;
  float* part;  // [B * ntw][P][C]
  int64_t sb, sc, sh, sw, ps;
  int C, H, W, P;
  int X, lx, pitch, chunk, nchunk, tpw, gb, mode;
  int stage_bytes;  // of the staged block, a multiple of 16
  int64_t ntw, HW;
};

template <class T>
__device__ __forceinline__ void ld16_raw(const typename T::elem* p, typename T::elem* v) {
  const uint4 r = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  if constexpr (T::V == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(w[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = (uint16_t)(w[j] & 0xffffu);
      v[2 * j + 1] = (uint16_t)(w[j] >> 16);
    }
  }
}

// `nlines` lines of n contiguous elements: element e of line l, at src(l) + e, goes to dst[l * lstride + e * estride].
// A line is cut at the 16-byte addresses: slot 0 is the head in front of the first one, the last slot the tail.
template <class T, class Src>
__device__ __forceinline__ void stage_lines(typename T::elem* dst, int nlines, int n, int lstride, int estride, Src src) {
  typedef typename T::elem E;
  constexpr int V = T::V;
  const int slots = (n + V - 1) / V + 1;
  for (int i = threadIdx.x; i < nlines * slots; i += kThreads) {
    const int l = i / slots, v = i - l * slots;
    const E* p = src(l);
    const int a = (int)((reinterpret_cast<uintptr_t>(p) / sizeof(E)) & (V - 1));
    const int e0 = ((V - a) & (V - 1)) + (v - 1) * V;
    E* d = dst + l * lstride;
    if (e0 >= 0 && e0 + V <= n) {
      E r[V];
      ld16_raw<T>(p + e0, r);
#pragma unroll
      for (int j = 0; j < V; ++j) d[(e0 + j) * estride] = r[j];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int e = e0 + j;
        if (e >= 0 && e < n) d[e * estride] = p[e];
      }
    }
  }
}

// channels c0 .. c0 + cc - 1 at pixels pos0 .. pos0 + n - 1 of image `img` -> sF[c * pitch + x]; zeros for x in n .. X - 1
template <class T>
__device__ __forceinline__ void stage(const GramArgs& a, const typename T::elem* img, typename T::elem* sF, int c0, int cc,
                                      int64_t pos0, int n) {
  typedef typename T::elem E;
  auto pixel = [&](int64_t pos) -> int64_t {
    const int64_t h = pos / a.W;
    return h * a.sh + (pos - h * a.W) * a.sw;
  };
  if (a.mode == 1) {
    const E* base = img + pos0 * a.ps;
    stage_lines<T>(sF, cc, n, a.pitch, 1, [&](int l) { return base + (int64_t)(c0 + l) * a.sc; });
  } else if (a.mode == 2) {
    stage_lines<T>(sF, n, cc, 1, a.pitch, [&](int l) { return img + pixel(pos0 + l) + c0; });
  } else {
    for (int i = threadIdx.x; i < cc * n; i += kThreads) {
      const int c = i / n, x = i - c * n;
      sF[c * a.pitch + x] = img[(int64_t)(c0 + c) * a.sc + pixel(pos0 + x)];
    }
  }
  if (n < a.X) {
    const int z = a.X - n;
    for (int i = threadIdx.x; i < cc * z; i += kThreads) {
      const int c = i / z;
      sF[c * a.pitch + n + (i - c * z)] = E(0);
    }
  }
}

// PC: the number of powers when it is known at compile time (10, the detector's default), 0 = a.P at run time
template <class T, int PC>
__global__ __launch_bounds__(kThreads) void gram_tile_kernel(GramArgs a) {
  typedef typename T::elem E;
  constexpr int PB = PC ? PC : kMaxP, KCH = kKch;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int P = PC ? PC : a.P;
  const int X = a.X, tid = threadIdx.x;
  E* sF = reinterpret_cast<E*>(smem);
  float* sS = reinterpret_cast<float*>(smem + a.stage_bytes);  // [P][X]
  float* red = sS + P * X;                                                                         // [wave][P][X]

  const int64_t b = blockIdx.x / a.ntw, j = blockIdx.x - b * a.ntw;
  const E* img = static_cast<const E*>(a.x) + b * a.sb;
  float* part = a.part + (int64_t)blockIdx.x * P * a.C;

  const int xa = tid & (X - 1), slice = tid >> a.lx, nslice = kThreads >> a.lx;  // pass A
  const int g = tid & (a.gb - 1), slot = tid / a.gb, nslot = kThreads / a.gb;     // pass B
  const int quads = X >> 2;

  float acc[KCH][PB];
#pragma unroll
  for (int k = 0; k < KCH; ++k)
#pragma unroll
    for (int p = 0; p < PB; ++p) acc[k][p] = 0.f;

  // the lanes of a channel add up; lane 0 of the group stores channel c0 + slot + k * nslot
  auto flush = [&](int c0, int cc) {
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
      const int c = slot + k * nslot;
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        if (PC || p < P) {
          float s = acc[k][p];
          for (int o = a.gb >> 1; o; o >>= 1) s += __shfl_xor(s, o);
          if (g == 0 && c < cc) part[(int64_t)p * a.C + c0 + c] = s;
          acc[k][p] = 0.f;
        }
      }
    }
  };

  for (int tile = 0; tile < a.tpw; ++tile) {
    const int64_t pos0 = (j * a.tpw + tile) * X;
    if (pos0 >= a.HW) break;
    const int n = a.HW - pos0 < X ? (int)(a.HW - pos0) : X;

    // ---- pass A: S_p[x] over all channels
    float s[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) s[p] = 0.f;
    for (int ch = 0; ch < a.nchunk; ++ch) {
      const int c0 = ch * a.chunk, cc = a.C - c0 < a.chunk ? a.C - c0 : a.chunk;
      __syncthreads();  // the previous readers of the stage are done
      stage<T>(a, img, sF, c0, cc, pos0, n);
      __syncthreads();
      for (int c = slice; c < cc; c += nslice) {
        const float f = widen(T{}, sF[c * a.pitch + xa]);
        float pw = f;
#pragma unroll
        for (int p = 0; p < PB; ++p) {
          if (PC || p < P) {
            s[p] += pw;
            pw *= f;
          }
        }
      }
    }
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      if (PC || p < P) {
        float v = s[p];
        for (int o = X; o < 64; o <<= 1) v += __shfl_xor(v, o);
        if ((tid & 63) < X) red[((tid >> 6) * P + p) * X + (tid & 63)] = v;
      }
    }
    __syncthreads();
    for (int i = tid; i < P * X; i += kThreads) {
      float v = red[i];
      for (int w = 1; w < kWaves; ++w) v += red[w * P * X + i];
      sS[i] = v;
    }
    __syncthreads();

    // ---- pass B: t[p][c] += sum_x F^p S_p over this tile
    for (int ch = 0; ch < a.nchunk; ++ch) {
      const int c0 = ch * a.chunk, cc = a.C - c0 < a.chunk ? a.C - c0 : a.chunk;
      if (a.nchunk > 1) {
        __syncthreads();
        stage<T>(a, img, sF, c0, cc, pos0, n);
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < KCH; ++k) {
        const int c = slot + k * nslot;
        if (c < cc) {
          const E* row = sF + c * a.pitch;
          for (int q = g; q < quads; q += a.gb) {
            const float f0 = widen(T{}, row[4 * q]), f1 = widen(T{}, row[4 * q + 1]);
            const float f2 = widen(T{}, row[4 * q + 2]), f3 = widen(T{}, row[4 * q + 3]);
            float w0 = f0, w1 = f1, w2 = f2, w3 = f3;
#pragma unroll
            for (int p = 0; p < PB; ++p) {
              if (PC || p < P) {
                const float4 sp = *reinterpret_cast<const float4*>(sS + p * X + 4 * q);
                float t = acc[k][p];
                t = fmaf(w0, sp.x, t);
                t = fmaf(w1, sp.y, t);
                t = fmaf(w2, sp.z, t);
                t = fmaf(w3, sp.w, t);
                acc[k][p] = t;
                w0 *= f0; w1 *= f1; w2 *= f2; w3 *= f3;
              }
            }
          }
        }
      }
      if (a.nchunk > 1) flush(c0, cc);
    }
  }
  if (a.nchunk == 1) flush(0, a.C);
}

// ---- finish ------------------------------------------------------------------------------------------------------------------
struct FinishArgs {
  const float* part;
  const void* labels;
  float* out;           // STATS: (B, P, C);  SCORE: (B)
  uint32_t *kmin, *kmax;  // FIT: ordered keys [K][P][C]
  const float *mins, *maxs;  // SCORE: [K][P][C]
  int64_t ntw, B, K;
  int C, P, label64;
};

__device__ __forceinline__ float signed_root(float t, int p) {
  const float a = fabsf(t);
  float r;
  switch (p) {
    case 1: r = a; break;
    case 2: r = sqrtf(a); break;
    case 4: r = sqrtf(sqrtf(a)); break;
    case 8: r = sqrtf(sqrtf(sqrtf(a))); break;
    case 16: r = sqrtf(sqrtf(sqrtf(sqrtf(a)))); break;
    default: r = __builtin_amdgcn_exp2f(log2_nonneg(a) / (float)p);  // (|.| >= 2^(-149/3): never a denormal result)
  }
  return copysignf(r, t);
}

__device__ __forceinline__ float gram_value(const FinishArgs& a, int64_t b, int p, int c) {
  const float* q = a.part + ((b * a.ntw) * a.P + p) * a.C + c;
  float t = q[0];
  for (int64_t j = 1; j < a.ntw; ++j) t += q[j * a.P * a.C];
  return signed_root(t, p + 1);
}

__device__ __forceinline__ int64_t label_of(const FinishArgs& a, int64_t b) {
  return a.label64 ? static_cast<const int64_t*>(a.labels)[b] : (int64_t) static_cast<const int32_t*>(a.labels)[b];
}

template <int MODE>  // RUNIA_GRAM_STATS or RUNIA_GRAM_FIT: thread = (image, channel)
__global__ __launch_bounds__(256) void gram_finish_kernel(FinishArgs a, int cblocks) {
  const int64_t b = blockIdx.x / cblocks;
  const int c = (int)(blockIdx.x - b * cblocks) * 256 + threadIdx.x;
  if (c >= a.C) return;
  int64_t k = 0;
  if (MODE == RUNIA_GRAM_FIT) {
    k = label_of(a, b);
    if (k < 0 || k >= a.K) return;  // an image of no class fits nothing
  }
  for (int p = 0; p < a.P; ++p) {
    const float v = gram_value(a, b, p, c);
    if (MODE == RUNIA_GRAM_STATS) {
      a.out[(b * a.P + p) * a.C + c] = v;
    } else {
      const int64_t at = (k * a.P + p) * a.C + c;
      const uint32_t key = asc_key(v);
      atomicMin(a.kmin + at, key);
      atomicMax(a.kmax + at, key);
    }
  }
}

__global__ __launch_bounds__(kScoreThreads) void gram_score_kernel(FinishArgs a) {
  __shared__ float wsum[kScoreWaves];
  const int64_t b = blockIdx.x, k = label_of(a, b);
  const int tid = threadIdx.x;
  const bool inside = k >= 0 && k < a.K;  // (uniform over the workgroup)
  float dev = 0.f;
  int unfitted = 0;
  if (inside) {
    const int items = a.P * a.C;
    const float* mn = a.mins + k * items;
    const float* mx = a.maxs + k * items;
    for (int i = tid; i < items; i += kScoreThreads) {
      const int p = i / a.C, c = i - p * a.C;
      const float v = gram_value(a, b, p, c), lo = mn[i], hi = mx[i];
      unfitted |= lo > hi;
      const float below = fmaxf(lo - v, 0.f) / fabsf(lo + 1e-6f), above = fmaxf(v - hi, 0.f) / fabsf(hi + 1e-6f);
      dev += below + above;
    }
  }
  unfitted = __syncthreads_or(unfitted);
  dev = wave_sum(dev);
  if ((tid & 63) == 0) wsum[tid >> 6] = dev;
  __syncthreads();
  if (tid == 0) {
    float s = wsum[0];
    for (int w = 1; w < kScoreWaves; ++w) s += wsum[w];
    a.out[b] = (!inside || unfitted) ? __builtin_inff() : s;
  }
}

__global__ __launch_bounds__(256) void gram_fill_kernel(uint32_t* p, int64_t n, uint32_t v) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}

bool sizes_ok(int dtype, int64_t B, int64_t C, int64_t H, int64_t W, int P) {
  const int64_t lim = 0x7fffffffll;
  return elem_dtype_ok(dtype) && B >= 0 && B <= lim && C >= 1 && C <= lim && H >= 1 && W >= 1 && H <= lim && W <= lim &&
         H * W <= lim && P >= 1 && P <= kMaxP && (int64_t)P * C <= lim;
}

template <class T, int PC>
int launch_tiles(const GramArgs& a, const GramPlan& g, int64_t blocks, hipStream_t s) {
  static std::atomic<uint64_t> done{0};
  if (runia_allow_dynamic_lds((const void*)gram_tile_kernel<T, PC>, 160 * 1024, done) != RUNIA_OK) return RUNIA_E_LAUNCH;
  RUNIA_LAUNCH_TIMED((gram_tile_kernel<T, PC>), (unsigned)blocks, kThreads, g.lds, s, a);
  return runia_check_launch();
}

}  // namespace

extern "C" int64_t runia_gram_tile_width(int dtype, int64_t C) {
  if (!elem_dtype_ok(dtype) || C < 1 || C > 0x7fffffffll) return 0;
  return make_plan(dtype, C, 1, 1, 1, 1, 1, 1).X;
}

extern "C" int64_t runia_gram_chunk_channels(int dtype, int64_t C) {
  if (!elem_dtype_ok(dtype) || C < 1 || C > 0x7fffffffll) return 0;
  return make_plan(dtype, C, 1, 1, 1, 1, 1, 1).chunk;
}

extern "C" int64_t runia_gram_workspace_bytes(int dtype, int64_t B, int64_t C, int64_t H, int64_t W, int P) {
  if (!sizes_ok(dtype, B, C, H, W, P) || B == 0) return 0;
  const GramPlan g = make_plan(dtype, C, H, W, 1, 1, 1, P);
  return (int64_t)ws_bytes([&](WsWalk& w) { w.take<float>((size_t)B * g.ntw * P * C, 16); });
}

extern "C" int runia_gram_table_init(uint32_t* kmin, uint32_t* kmax, int64_t n, runia_stream_t stream) {
  if (n < 0 || (n > 0 && (!kmin || !kmax))) return RUNIA_E_INVALID;
  if (n == 0) return RUNIA_OK;
  hipStream_t s = as_stream(stream);
  gram_fill_kernel<<<runia_stream_grid(n, 256), 256, 0, s>>>(kmin, n, asc_key(__builtin_inff()));
  gram_fill_kernel<<<runia_stream_grid(n, 256), 256, 0, s>>>(kmax, n, asc_key(-__builtin_inff()));
  return runia_check_launch();
}

extern "C" int runia_gram_layer(const void* x, int dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t sb, int64_t sc,
                                int64_t sh, int64_t sw, int P, int mode, const void* labels, int label64, int64_t K,
                                void* mins, void* maxs, float* out, void* workspace, size_t workspace_bytes,
                                runia_stream_t stream) {
  if (!sizes_ok(dtype, B, C, H, W, P) || sb < 0 || sc < 0 || sh < 0 || sw < 0 || mode < RUNIA_GRAM_STATS ||
      mode > RUNIA_GRAM_SCORE)
    return RUNIA_E_INVALID;
  if (mode != RUNIA_GRAM_STATS && (K < 1 || K > 0x7fffffffll)) return RUNIA_E_INVALID;
  if (B == 0) return RUNIA_OK;
  if (!x || (mode != RUNIA_GRAM_FIT && !out) || (mode != RUNIA_GRAM_STATS && (!labels || !mins || !maxs)))
    return RUNIA_E_INVALID;
  const GramPlan g = make_plan(dtype, C, H, W, sc, sh, sw, P);
  const int64_t blocks = B * g.ntw;
  if (blocks > 0x7fffffffll || g.lds > 160 * 1024) return RUNIA_E_INVALID;
  const size_t need = (size_t)runia_gram_workspace_bytes(dtype, B, C, H, W, P);
  if (ws_refused(workspace, workspace_bytes, need, 16)) return RUNIA_E_WORKSPACE;
  WsWalk walk(workspace);
  float* part = walk.take<float>((size_t)blocks * P * C, 16);
  hipStream_t s = as_stream(stream);

  GramArgs a;
  a.x = x; a.part = part;
  a.sb = sb; a.sc = sc; a.sh = sh; a.sw = sw; a.ps = g.ps;
  a.C = (int)C; a.H = (int)H; a.W = (int)W; a.P = P;
  a.X = g.X; a.lx = g.lx; a.pitch = g.pitch; a.chunk = g.chunk; a.nchunk = g.nchunk; a.tpw = g.tpw; a.gb = g.gb;
  a.mode = g.mode;
  a.stage_bytes = (int)round_up((size_t)g.chunk * g.pitch * (dtype == kF32 ? 4 : 2), 16);
  a.ntw = g.ntw; a.HW = H * W;
  const int rc = dispatch_elem(dtype, [&](auto t) {
    typedef decltype(t) T;
    return P == 10 ? launch_tiles<T, 10>(a, g, blocks, s) : launch_tiles<T, 0>(a, g, blocks, s);
  });
  if (rc != RUNIA_OK) return rc;

  FinishArgs f;
  f.part = part; f.labels = labels; f.out = out;
  f.kmin = static_cast<uint32_t*>(mins); f.kmax = static_cast<uint32_t*>(maxs);
  f.mins = static_cast<const float*>(mins); f.maxs = static_cast<const float*>(maxs);
  f.ntw = g.ntw; f.B = B; f.K = K;
  f.C = (int)C; f.P = P; f.label64 = label64;
  if (mode == RUNIA_GRAM_SCORE) {
    gram_score_kernel<<<(unsigned)B, kScoreThreads, 0, s>>>(f);
    return runia_check_launch();
  }
  const int cblocks = (int)((C + 255) / 256);
  if (B * cblocks > 0x7fffffffll) return RUNIA_E_INVALID;
  if (mode == RUNIA_GRAM_STATS) gram_finish_kernel<RUNIA_GRAM_STATS><<<(unsigned)(B * cblocks), 256, 0, s>>>(f, cblocks);
  else gram_finish_kernel<RUNIA_GRAM_FIT><<<(unsigned)(B * cblocks), 256, 0, s>>>(f, cblocks);
  return runia_check_launch();
}
