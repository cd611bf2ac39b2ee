// Standardized Max Logits (Jung et al., ICCV 2021) of a segmentation head from its (G, C, H, W) logits read where the model
// left them, and the two map post-processing steps that go with it:
//   runia_pixel_sml_accumulate       ONE pass that ADDS the exact integer moments of every pixel's max logit, by predicted class,
//                                    into a small integer device record (the fit streams a training set batch by batch)
//   runia_pixel_sml_maps             ONE launch: sml = (m - mean[label]) * inv_std[label], label, optionally the raw max logit
//   runia_pixel_boundary_smooth_f32  iterative boundary suppression, then a dilated Gaussian smoothing, of any f32 (G, H, W) map
//
// The first two walk the class planes of a pixel inside one lane, as pixel_calibration.hip does, in its three load forms
// (pixel_map.hpp: kLoadVec / kLoadCLast / kLoadElem, picked on the host) and its two kernels: the register form for C <= 24 (every
// load of a lane's pixels is issued before the first compare) and the general form for any C <= 1024 (one walk: only the running
// maximum is kept).  The maximum is torch.max(dim=1)'s: the first NaN wins, ties go to the lowest index.
//
// Fit.  A used pixel (valid, m finite, |m| < 2^14) adds q = rint(m * 2^16), |q| < 2^30, as count += 1, sum_q += q and
// q * q = hi * 2^30 + lo into sq_hi, sq_lo.  A lane merges runs of equal labels, the workgroup's table is in LDS (28 bytes a
// class), the workgroups flush with 64-bit integer atomics into the record.  Integer adds only: any order, any split into
// batches and any number of GPUs give the same record.  hi < 2^30 and lo < 2^30: 2^34 pixels cannot overflow a uint64.
//
// Post-processing.  Two launches, the suppressed map in the caller's workspace between them.  A workgroup owns a
// RUNIA_PIXSML_TILE_H x RUNIA_PIXSML_TILE_W output tile of ONE image (no row of another image is ever a neighbour).
//   suppression  stages the scores with a halo of I pixels, builds the boundary flags with a halo of I + Wb - 1 from the labels
//                (halo I + Wb), the capped Chebyshev distance as bytes (row min-filter, then column min-filter), and runs the I
//                iterates ping-pong in LDS, each on the region that the later ones still read
//   smoothing    separable: the row pass of the K taps from global memory into LDS for the TILE_H + d (K - 1) rows the tile
//                reads, then the column pass from LDS
// One launch for both would need a halo of I + d (K - 1) / 2 = 22 score pixels at the defaults: two 76 x 108 f32 buffers and the
// byte maps are 92 KB for a 32 x 64 tile, more than the 80 KB at which two workgroups share a CU; a 32 x 32 tile fits (65 KB) but
// 82 % of what it stages and iterates is halo.  The two launches cost 8 bytes a pixel (one write, one read of the iterate).
// Every output pixel is computed by one thread in a fixed order: the same calls give the same bits.
#include "common.hpp"
#include "elem.hpp"
#include "pixel_map.hpp"

#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kRegC = 24;                  // widest head of the register form
constexpr int kItemsPerThread = 2;         // lane items of a workgroup's range, per thread, while the grid is below its cap
constexpr int kMaxBlocks = 2048;
constexpr int kHead = RUNIA_PIXSML_HEAD_SLOTS;
constexpr int64_t kMaxPixels = (int64_t)1 << 34;
constexpr float kQ = 65536.f;              // 2^16: the grid of the fit
constexpr float kMaxAbs = 16384.f;         // 2^14: |m| of a used pixel stays below it

// torch.max(dim=1) over ascending classes: a NaN is taken once and kept, a tie keeps the lower index
__device__ __forceinline__ void max_take(float& m, int& bi, float v, int c) {
  if (m == m && (v > m || v != v)) {
    m = v;
    bi = c;
  }
}

// m and its index for the PPL pixels of a lane; p: class 0 of the first pixel, sc: the class stride
// CMAX > 0: the register form (C <= CMAX; EXACT: C == CMAX, the heads of 19 and 21); CMAX == 0: the general form
template <class T, int LOAD, int CMAX, bool EXACT, int PPL>
__device__ __forceinline__ void pixel_max(const typename T::elem* p, int64_t sc, int C, float (&m)[PPL], int (&bi)[PPL]) {
  if constexpr (CMAX > 0) {
    float v[CMAX][PPL];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {  // every load is issued; a class past C re-reads the last plane and is masked
      const int cc = (EXACT || c < C) ? c : C - 1;
      load_px<T, LOAD>(p + cc * sc, v[c]);
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      m[j] = v[0][j];
      bi[j] = 0;
    }
#pragma unroll
    for (int c = 1; c < CMAX; ++c) {
      if (EXACT || c < C) {
#pragma unroll
        for (int j = 0; j < PPL; ++j) max_take(m[j], bi[j], v[c][j], c);
      }
    }
  } else {
    load_px<T, LOAD>(p, m);
#pragma unroll
    for (int j = 0; j < PPL; ++j) bi[j] = 0;
#pragma unroll 8
    for (int c = 1; c < C; ++c) {
      float x[PPL];
      load_px<T, LOAD>(p + c * sc, x);
#pragma unroll
      for (int j = 0; j < PPL; ++j) max_take(m[j], bi[j], x[j], c);
    }
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

bool sizes_ok(int64_t G, int64_t C, int64_t H, int64_t W) {
  if (G < 0 || H < 0 || W < 0 || C < 1 || C > RUNIA_PIXSML_MAX_CLASSES || G > kLim || H > kLim || W > kLim) return false;
  return G == 0 || H * W == 0 || G * H * W <= kMaxPixels;
}

// ---- the fit ------------------------------------------------------------------------------------------------------------------
struct AccArgs {
  MapView v;
  const uint8_t* valid;  // (G, H, W) contiguous, or null: every pixel
  int64_t items, items_per_block;
  unsigned long long* rec;  // head | count[C] | sum_q[C] | sq_hi[C] | sq_lo[C]
};

struct MomRun {  // what a lane has for one class, not yet in LDS
  int label;
  unsigned n;
  long long sum;
  unsigned long long hi, lo;
};

// the table of one workgroup in LDS: the 64-bit sums first, then the 32-bit counts (a workgroup walks fewer than 2^32 pixels)
struct MomTable {
  unsigned long long *sum, *hi, *lo;
  unsigned* cnt;
};
__host__ __device__ inline size_t moment_lds_bytes(int C) { return (size_t)C * 28; }

__device__ __forceinline__ void flush_run(const MomTable& t, MomRun& r) {
  if (r.n) {
    atomicAdd(&t.cnt[r.label], r.n);
    atomicAdd(&t.sum[r.label], (unsigned long long)r.sum);  // (two's complement: the sum of the words is the word of the sum)
    atomicAdd(&t.hi[r.label], r.hi);
    atomicAdd(&t.lo[r.label], r.lo);
  }
  r.n = 0u;
  r.sum = 0;
  r.hi = r.lo = 0ull;
}

template <class T, int LOAD, int CMAX, bool EXACT>
__global__ __launch_bounds__(kThreads) void pixsml_accumulate_kernel(AccArgs a) {
  constexpr int PPL = LOAD == kLoadVec ? 4 : 1;
  typedef typename T::elem E;
  extern __shared__ unsigned long long lds64[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int C = a.v.C;
  const int64_t sc = LOAD == kLoadCLast ? 1 : a.v.sc;

  MomTable t;
  t.sum = lds64;
  t.hi = t.sum + C;
  t.lo = t.hi + C;
  t.cnt = reinterpret_cast<unsigned*>(t.lo + C);
  for (int i = tid; i < 7 * C; i += kThreads) reinterpret_cast<unsigned*>(lds64)[i] = 0u;
  __syncthreads();

  MomRun run = {0, 0u, 0, 0ull, 0ull};
  unsigned n_used = 0u, n_masked = 0u, n_bad = 0u;
  const int64_t t0 = (int64_t)blockIdx.x * a.items_per_block;
  const int64_t t1 = (t0 + a.items_per_block < a.items) ? t0 + a.items_per_block : a.items;
  for (int64_t it = t0 + tid; it < t1; it += kThreads) {
    const int64_t pix0 = it * PPL;  // (vector form: the joined row is a multiple of four pixels, no group is cut)
    const E* p = static_cast<const E*>(a.v.x) + pixel_offset(a.v, pix0);
    float m[PPL];
    int bi[PPL];
    pixel_max<T, LOAD, CMAX, EXACT, PPL>(p, sc, C, m, bi);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const bool valid = !a.valid || a.valid[pix0 + j] != 0;
      const bool used = valid && fabsf(m[j]) < kMaxAbs;  // (false for a NaN and for +-inf)
      n_masked += valid ? 0u : 1u;
      n_bad += (valid && !used) ? 1u : 0u;
      if (!used) continue;
      n_used += 1u;
      const long long q = (long long)rintf(m[j] * kQ);  // the product is exact: |q| < 2^30
      const unsigned long long qq = (unsigned long long)(q * q);
      if (bi[j] != run.label) {
        flush_run(t, run);
        run.label = bi[j];
      }
      run.n += 1u;
      run.sum += q;
      run.hi += qq >> 30;
      run.lo += qq & 0x3fffffffull;
    }
  }
  flush_run(t, run);
  n_used = wave_sum(n_used);
  n_masked = wave_sum(n_masked);
  n_bad = wave_sum(n_bad);
  if (lane == 0) {
    if (n_used) atomicAdd(a.rec + 0, (unsigned long long)n_used);
    if (n_masked) atomicAdd(a.rec + 1, (unsigned long long)n_masked);
    if (n_bad) atomicAdd(a.rec + 2, (unsigned long long)n_bad);
  }
  __syncthreads();  // every LDS atomic of the workgroup is done
  // whatever the workgroup counted, straight into the record (integer adds: any order gives the same sums)
  unsigned long long* g = a.rec + kHead;
  for (int i = tid; i < C; i += kThreads) {
    const unsigned n = t.cnt[i];
    if (n) {
      atomicAdd(g + i, (unsigned long long)n);
      atomicAdd(g + C + i, t.sum[i]);
      atomicAdd(g + 2 * C + i, t.hi[i]);
      atomicAdd(g + 3 * C + i, t.lo[i]);
    }
  }
}

template <class T, int LOAD>
int launch_accumulate(const AccArgs& a, unsigned grid, hipStream_t s) {
  const size_t lds = moment_lds_bytes(a.v.C);
  if (a.v.C == 19) pixsml_accumulate_kernel<T, LOAD, 19, true><<<grid, kThreads, lds, s>>>(a);
  else if (a.v.C == 21) pixsml_accumulate_kernel<T, LOAD, 21, true><<<grid, kThreads, lds, s>>>(a);
  else if (a.v.C <= kRegC) pixsml_accumulate_kernel<T, LOAD, kRegC, false><<<grid, kThreads, lds, s>>>(a);
  else pixsml_accumulate_kernel<T, LOAD, 0, false><<<grid, kThreads, lds, s>>>(a);
  return runia_check_launch();
}

// ---- the score ------------------------------------------------------------------------------------------------------------------
struct MapArgs {
  MapView v;
  const float *mean, *inv_std;
  int64_t items;
  float *sml, *max_logit;
  int32_t* label;
  int vec_store;  // every map that is given is 16-byte aligned
};

template <class T, int LOAD, int CMAX, bool EXACT>
__global__ __launch_bounds__(kThreads) void pixsml_maps_kernel(MapArgs a) {
  constexpr int PPL = LOAD == kLoadVec ? 4 : 1;
  typedef typename T::elem E;
  const int C = a.v.C;
  const int64_t sc = LOAD == kLoadCLast ? 1 : a.v.sc;
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < a.items; it += (int64_t)gridDim.x * kThreads) {
    const int64_t pix0 = it * PPL;
    const E* p = static_cast<const E*>(a.v.x) + pixel_offset(a.v, pix0);
    float m[PPL], z[PPL];
    int bi[PPL];
    pixel_max<T, LOAD, CMAX, EXACT, PPL>(p, sc, C, m, bi);
#pragma unroll
    for (int j = 0; j < PPL; ++j) z[j] = a.sml ? (m[j] - a.mean[bi[j]]) * a.inv_std[bi[j]] : 0.f;
    if constexpr (PPL == 4) {
      if (a.vec_store) {
        if (a.sml) *reinterpret_cast<float4*>(a.sml + pix0) = make_float4(z[0], z[1], z[2], z[3]);
        if (a.label) *reinterpret_cast<int4*>(a.label + pix0) = make_int4(bi[0], bi[1], bi[2], bi[3]);
        if (a.max_logit) *reinterpret_cast<float4*>(a.max_logit + pix0) = make_float4(m[0], m[1], m[2], m[3]);
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      if (a.sml) a.sml[pix0 + j] = z[j];
      if (a.label) a.label[pix0 + j] = bi[j];
      if (a.max_logit) a.max_logit[pix0 + j] = m[j];
    }
  }
}

template <class T, int LOAD>
int launch_maps(const MapArgs& a, hipStream_t s) {
  const unsigned grid = runia_stream_grid(a.items, kThreads);
  if (a.v.C == 19) pixsml_maps_kernel<T, LOAD, 19, true><<<grid, kThreads, 0, s>>>(a);
  else if (a.v.C == 21) pixsml_maps_kernel<T, LOAD, 21, true><<<grid, kThreads, 0, s>>>(a);
  else if (a.v.C <= kRegC) pixsml_maps_kernel<T, LOAD, kRegC, false><<<grid, kThreads, 0, s>>>(a);
  else pixsml_maps_kernel<T, LOAD, 0, false><<<grid, kThreads, 0, s>>>(a);
  return runia_check_launch();
}

// f(tag, load form, lane items) for the view of one launch
template <class F>
int dispatch_view(int dtype, const MapView& v, int64_t G, int64_t H, F f) {
  return dispatch_elem(dtype, [&](auto tag) {
    typedef decltype(tag) T;
    if (view_allows_vec(v, G, H, T::kBytes)) return f(tag, std::integral_constant<int, kLoadVec>{}, v.P / 4);
    if (v.sc == 1 && v.C > 1) return f(tag, std::integral_constant<int, kLoadCLast>{}, v.P);
    return f(tag, std::integral_constant<int, kLoadElem>{}, v.P);
  });
}

// ---- boundary suppression and dilated smoothing ------------------------------------------------------------------------------------
constexpr int kTH = RUNIA_PIXSML_TILE_H, kTW = RUNIA_PIXSML_TILE_W;
constexpr int kMaxWb = RUNIA_PIXSML_MAX_WIDTH, kMaxDil = RUNIA_PIXSML_MAX_DILATION, kMaxK = RUNIA_PIXSML_MAX_KERNEL;
constexpr int kMaxHaloS = kMaxWb;                   // score halo of the suppression: I <= Wb
constexpr int kMaxHaloB = 2 * kMaxWb - 1;           // boundary-flag halo: I + Wb - 1
constexpr int kMaxHaloG = kMaxDil * (kMaxK - 1) / 2;  // row halo of the smoothing
constexpr int kScoreCells = (kTH + 2 * kMaxHaloS) * (kTW + 2 * kMaxHaloS);
constexpr int kFlagCells = (kTH + 2 * kMaxHaloB) * (kTW + 2 * kMaxHaloB);

struct TileArgs {
  const float* x;
  const int32_t* lab;
  float* out;
  int64_t HW;
  int H, W, tiles_x, tiles_y;
  int Wb, I;        // suppression
  int K, d;         // smoothing
  float g[kMaxK];
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the tile of a workgroup: image, first row, first column
__device__ __forceinline__ void tile_of(const TileArgs& a, int64_t& img, int& y0, int& x0) {
  const int64_t b = blockIdx.x;
  const int64_t per = (int64_t)a.tiles_x * a.tiles_y;
  img = b / per;
  const int r = (int)(b - img * per);
  y0 = (r / a.tiles_x) * kTH;
  x0 = (r % a.tiles_x) * kTW;
}

__global__ __launch_bounds__(kThreads) void pixsml_suppress_kernel(TileArgs a) {
  __shared__ float buf[2][kScoreCells];
  __shared__ uint8_t flag[kFlagCells];   // 1: boundary pixel
  __shared__ uint8_t rowd[kFlagCells];   // distance to the nearest boundary pixel of the row, capped at Wb
  __shared__ uint8_t dist[kScoreCells];  // Chebyshev distance to the nearest boundary pixel, capped at Wb
  const int tid = threadIdx.x;
  int64_t img;
  int y0, x0;
  tile_of(a, img, y0, x0);
  const float* x = a.x + img * a.HW;
  const int32_t* lab = a.lab + img * a.HW;
  const int H = a.H, W = a.W, Wb = a.Wb, I = a.I;
  const int hs = I, hb = I + Wb - 1;
  const int RH = kTH + 2 * hs, RW = kTW + 2 * hs;  // the score region
  const int BH = kTH + 2 * hb, BW = kTW + 2 * hb;  // the flag region

  for (int i = tid; i < RH * RW; i += kThreads) {
    const int yy = y0 - hs + i / RW, xx = x0 - hs + i % RW;
    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
    buf[0][i] = in ? x[(int64_t)yy * W + xx] : 0.f;  // (a cell outside the image is never read)
  }
  for (int i = tid; i < BH * BW; i += kThreads) {
    const int yy = y0 - hb + i / BW, xx = x0 - hb + i % BW;
    uint8_t f = 0;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const int64_t o = (int64_t)yy * W + xx;
      const int32_t l = lab[o];
      const bool up = yy > 0 && lab[o - W] != l, dn = yy + 1 < H && lab[o + W] != l;
      const bool lf = xx > 0 && lab[o - 1] != l, rt = xx + 1 < W && lab[o + 1] != l;
      f = (up || dn || lf || rt) ? 1 : 0;
    }
    flag[i] = f;
  }
  __syncthreads();
  for (int i = tid; i < BH * BW; i += kThreads) {  // row min-filter
    const int r = i / BW, c = i % BW;
    int best = Wb;
    for (int k = -(Wb - 1); k <= Wb - 1; ++k) {
      const int cc = c + k;
      const int ak = k < 0 ? -k : k;
      if (cc >= 0 && cc < BW && flag[r * BW + cc] && ak < best) best = ak;
    }
    rowd[i] = (uint8_t)best;
  }
  __syncthreads();
  for (int i = tid; i < RH * RW; i += kThreads) {  // column min-filter: min over dy of max(|dy|, rowd)
    const int r = i / RW + (hb - hs), c = i % RW + (hb - hs);
    int best = Wb;
    for (int k = -(Wb - 1); k <= Wb - 1; ++k) {
      const int rr = r + k;  // (inside the flag region: hb - hs = Wb - 1)
      const int ak = k < 0 ? -k : k;
      const int v = rowd[rr * BW + c];
      const int mx = v > ak ? v : ak;
      best = mx < best ? mx : best;
    }
    dist[i] = (uint8_t)best;
  }
  __syncthreads();

  const int step = Wb / I;
  int cur = 0;
  for (int t = 0; t < I; ++t) {
    const int rt = (t == I - 1) ? 0 : Wb - step * t - 1;  // the last iterate touches the boundary pixels alone
    const int sh = t + 1;  // iterate t + 1 is needed on the region shrunk by t + 1
    const int SH = RH - 2 * sh, SW = RW - 2 * sh;
    const float* src = buf[cur];
    float* dst = buf[cur ^ 1];
    for (int i = tid; i < SH * SW; i += kThreads) {
      const int r = sh + i / SW, c = sh + i % SW;
      const int yy = y0 - hs + r, xx = x0 - hs + c;
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const int o = r * RW + c;
      float v = src[o];
      if (dist[o] <= rt) {
        float sum = 0.f;
        int n = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          const int rr = clampi(yy + dy, H - 1) - (y0 - hs);
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int cc = clampi(xx + dx, W - 1) - (x0 - hs);
            const int oo = rr * RW + cc;
            if (dist[oo] > rt) {  // selected, not multiplied: a NaN under the mask does not spread
              sum += src[oo];
              n += 1;
            }
          }
        }
        if (n > 0) v = sum / (float)n;
      }
      dst[o] = v;
    }
    cur ^= 1;
    __syncthreads();
  }
  float* out = a.out + img * a.HW;
  for (int i = tid; i < kTH * kTW; i += kThreads) {
    const int r = i / kTW, c = i % kTW;
    const int yy = y0 + r, xx = x0 + c;
    if (yy < H && xx < W) out[(int64_t)yy * W + xx] = buf[cur][(r + hs) * RW + c + hs];
  }
}

__global__ __launch_bounds__(kThreads) void pixsml_smooth_kernel(TileArgs a) {
  __shared__ float rows[(kTH + 2 * kMaxHaloG) * kTW];
  const int tid = threadIdx.x;
  int64_t img;
  int y0, x0;
  tile_of(a, img, y0, x0);
  const float* x = a.x + img * a.HW;
  const int H = a.H, W = a.W, K = a.K, d = a.d;
  const int h = d * (K - 1) / 2;
  const int RH = kTH + 2 * h;
  for (int i = tid; i < RH * kTW; i += kThreads) {  // the row pass, taps in ascending order
    const int r = i / kTW, c = i % kTW;
    const int yy = clampi(y0 - h + r, H - 1), xx = x0 + c;
    const float* row = x + (int64_t)yy * W;
    float s = 0.f;
    for (int b = 0; b < K; ++b) s += a.g[b] * row[clampi(xx + b * d - h, W - 1)];
    rows[i] = s;
  }
  __syncthreads();
  float* out = a.out + img * a.HW;
  for (int i = tid; i < kTH * kTW; i += kThreads) {  // the column pass
    const int r = i / kTW, c = i % kTW;
    const int yy = y0 + r, xx = x0 + c;
    if (yy >= H || xx >= W) continue;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += a.g[k] * rows[(r + k * d) * kTW + c];
    out[(int64_t)yy * W + xx] = s;
  }
}

bool suppress_on(int Wb, int I) { return Wb > 0 && I > 0; }

// the workspace of runia_pixel_boundary_smooth_f32 when both steps run: the suppressed map, between the two launches
float* plan_iterate(WsWalk& w, int64_t P) { return w.take<float>((size_t)P); }

// 0 ok; the parameters of runia_pixel_boundary_smooth_f32 and its workspace query
bool smooth_params_ok(int64_t G, int64_t H, int64_t W, int Wb, int I, int K, int d) {
  if (G < 0 || H < 0 || W < 0 || G > kLim || H > kLim || W > kLim) return false;
  if (G > 0 && H * W > 0 && G * H * W > kMaxPixels) return false;
  if (Wb < 0 || Wb > kMaxWb || I < 0 || I > kMaxWb) return false;
  if (suppress_on(Wb, I) && Wb % I != 0) return false;
  if (K != 0 && K != 3 && K != 5 && K != 7) return false;
  if (K != 0 && (d < 1 || d > kMaxDil)) return false;
  if (G > 0 && H * W > 0) {
    const int64_t tiles = G * ((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW);
    if (tiles > kLim) return false;
  }
  return true;
}

}  // namespace

extern "C" int runia_pixel_sml_accumulate(const void* logits, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn,
                                          int64_t sc, int64_t sh, int64_t sw, const void* valid, void* record,
                                          runia_stream_t stream) {
  if (!elem_dtype_ok(dtype) || !sizes_ok(G, C, H, W) || !view_ok(G, C, H, W, sn, sc, sh, sw)) return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;  // nothing to add
  if (!logits || !record || reinterpret_cast<uintptr_t>(record) % 8 != 0) return RUNIA_E_INVALID;
  AccArgs a;
  a.v = make_view(logits, G, C, H, W, sn, sc, sh, sw);
  a.valid = static_cast<const uint8_t*>(valid);
  a.rec = static_cast<unsigned long long*>(record);
  hipStream_t s = as_stream(stream);
  return dispatch_view(dtype, a.v, G, H, [&](auto tag, auto load, int64_t items) {
    int64_t blocks;
    a.items = items;
    grid_of(items, blocks, a.items_per_block);
    return launch_accumulate<decltype(tag), decltype(load)::value>(a, (unsigned)blocks, s);
  });
}

extern "C" int runia_pixel_sml_maps(const void* logits, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn,
                                    int64_t sc, int64_t sh, int64_t sw, const float* mean, const float* inv_std, float* sml,
                                    int32_t* label, float* max_logit, runia_stream_t stream) {
  if (!elem_dtype_ok(dtype) || !sizes_ok(G, C, H, W) || !view_ok(G, C, H, W, sn, sc, sh, sw)) return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;
  if (!logits || (!sml && !label && !max_logit) || (sml && (!mean || !inv_std))) return RUNIA_E_INVALID;
  MapArgs a;
  a.v = make_view(logits, G, C, H, W, sn, sc, sh, sw);
  a.mean = mean;
  a.inv_std = inv_std;
  a.sml = sml;
  a.label = label;
  a.max_logit = max_logit;
  a.vec_store = (reinterpret_cast<uintptr_t>(sml) % 16 == 0 && reinterpret_cast<uintptr_t>(label) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(max_logit) % 16 == 0) ? 1 : 0;
  hipStream_t s = as_stream(stream);
  return dispatch_view(dtype, a.v, G, H, [&](auto tag, auto load, int64_t items) {
    a.items = items;
    return launch_maps<decltype(tag), decltype(load)::value>(a, s);
  });
}

extern "C" int64_t runia_pixel_boundary_smooth_workspace_bytes(int64_t G, int64_t H, int64_t W, int boundary_width,
                                                               int boundary_iterations, int kernel_size) {
  if (!smooth_params_ok(G, H, W, boundary_width, boundary_iterations, kernel_size, 1) || G == 0 || H * W == 0) return 0;
  if (!suppress_on(boundary_width, boundary_iterations) || kernel_size == 0) return 0;  // one step: straight into `out`
  return (int64_t)ws_bytes([&](WsWalk& w) { plan_iterate(w, G * H * W); });
}

extern "C" int runia_pixel_boundary_smooth_f32(const float* score, const int32_t* label, int64_t G, int64_t H, int64_t W,
                                               int boundary_width, int boundary_iterations, int kernel_size, int dilation,
                                               const float* taps, float* out, void* workspace, size_t workspace_bytes,
                                               runia_stream_t stream) {
  if (!smooth_params_ok(G, H, W, boundary_width, boundary_iterations, kernel_size, dilation)) return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;
  const bool sup = suppress_on(boundary_width, boundary_iterations), smooth = kernel_size != 0;
  if (!score || !out || score == out || (sup && !label) || (smooth && !taps)) return RUNIA_E_INVALID;
  const size_t need = (size_t)runia_pixel_boundary_smooth_workspace_bytes(G, H, W, boundary_width, boundary_iterations, kernel_size);
  if (need > 0 && ws_refused(workspace, workspace_bytes, need, 4)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  if (!sup && !smooth) {
    return hipMemcpyAsync(out, score, (size_t)(G * H * W) * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess
               ? RUNIA_OK : RUNIA_E_LAUNCH;
  }
  TileArgs a;
  a.lab = label;
  a.HW = H * W;
  a.H = (int)H;
  a.W = (int)W;
  a.tiles_x = (int)((W + kTW - 1) / kTW);
  a.tiles_y = (int)((H + kTH - 1) / kTH);
  a.Wb = boundary_width;
  a.I = boundary_iterations;
  a.K = kernel_size;
  a.d = dilation;
  for (int k = 0; k < kMaxK; ++k) a.g[k] = (smooth && k < kernel_size) ? taps[k] : 0.f;
  const unsigned grid = (unsigned)(G * a.tiles_x * a.tiles_y);
  const float* src = score;
  if (sup) {
    WsWalk walk(workspace);
    a.x = score;
    a.out = smooth ? plan_iterate(walk, G * H * W) : out;
    pixsml_suppress_kernel<<<grid, kThreads, 0, s>>>(a);
    if (int rc = runia_check_launch()) return rc;
    src = a.out;
  }
  if (smooth) {
    a.x = src;
    a.out = out;
    pixsml_smooth_kernel<<<grid, kThreads, 0, s>>>(a);
    return runia_check_launch();
  }
  return RUNIA_OK;
}
