// Per-pixel class-Gaussian log densities (pixel DDU: Mukhoti et al., "Deep Deterministic Uncertainty for Semantic
// Segmentation", 2021) from the feature maps of a segmentation decoder, read where the model left them:
//   runia_pixdens_score   ONE launch over G maps of (C, h, w) features in f32 / f16 / bf16 (NCHW, channels_last or any strided
//                         view): lp_c = consts[c] - 0.5 |W_c (x - mu_c)|^2 with a lower-triangular W_c = L_c^-1 of its own per
//                         class, their logsumexp, its argmax and all K terms.
//
// The pooled-covariance kernel (pixel_features.hip) multiplies every pixel ONCE and streams the pixels past a resident W.
// Here the product differs per class, so the roles are swapped: the workgroup's pixel tile is widened once and stays in LDS
// as Xs[channel][pixel] for the whole launch (the map is read from HBM once), and the K triangular matrices stream past it,
// 128 rows x 32 columns at a time through Ws[row][34], the next chunk's loads in flight while the matrix cores consume this
// one - across the block and class boundaries too: (class, row block, chunk) is ONE flat sequence of steps.  The staged
// chunks - K sum_j0 128 min(j0 + 128, C) floats, 3/4 K C^2 at C = 256: 3.7 MB at K = 19 - are shared by every workgroup: an
// L2 / Infinity-Cache stream.
//
// On v_mfma_f32_32x32x2_f32 W_c is the A operand (rows j) and x - mu_c the B operand (columns = pixels): the difference is
// formed in f32 as the operand leaves LDS (Xs holds x itself; mu_c sits beside it as mus[channel]), so a lane holds ONE pixel
// (lane & 31) and 16 of the 32 rows of a tile, and |z|^2 is summed inside the lane: 64 squares per block in f32 on four
// chains, the blocks and the two lane halves in f64 (the row kernel gmm_tril.hip: f32 products, f64 sums), then
// lp_c = (float)(consts[c] - 0.5 d) and an online (max, sum) logsumexp over the classes in ascending order, in f64, in the
// lane that holds the pixel.  Nothing (pixels, C) or (pixels, K) is written unless class_log_densities is asked for.
//
// W_c is lower triangular: row block j0 needs the chunks up to its own last row only, and inside the diagonal block a
// 32-row tile stops at its own last row (36 of the 48 tile-chunks of a dense product at C = 256).
//
// Tile width.  The resident tile must fit the 160 KB of LDS next to Ws (17 KB), mus and the cross-wave sums:
//   C <=  256   128 pixels, pitch 132: wave v owns pixels 32 v .. + 31 and all 128 rows of a block (4 tiles)   <= 153 600 B
//   C <=  512    64 pixels, pitch  68: waves (v & 1) share the pixels, (v >> 1) the halves of a block (2 tiles)  <= 159 744 B
//   C <= 1024    32 pixels, pitch  32: every wave owns 32 rows of a block for the same 32 pixels (1 tile)        <= 153 600 B
// The LDS of a launch follows C (round_up(C, chunk) rows), so narrow maps keep several workgroups on a compute unit.  Where
// waves share pixels their f64 sums of a class meet in LDS and are added in wave order.
// The tile is read in one of the three ways of pixel_map.hpp (vector, channels_last, element); all fill the same Xs, every
// sum runs in one fixed order and there are no atomics: results are bit identical from run to run, on the three load paths,
// and wherever in the batch a pixel sits.
//
// A pixel with a NaN or infinite feature (found by one pass over its resident column) has NaN in every output, nearest 0; a
// pixel is a column of the B operand, nothing of it reaches another column.  A finite pixel so far out that its squares
// overflow has d = +inf for that class: lp_c = -inf (all classes: log_density -inf, nearest 0).
// consts[c] = -inf excludes class c: lp_c = -inf, it never wins; all excluded: log_density = -inf, nearest 0.
#include "common.hpp"
#include "elem.hpp"
#include "pixel_map.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTJ = 128;  // rows of W_c per block
constexpr int kMaxK = 256;
constexpr int kMaxLds = 160 * 1024;

constexpr int tile_pitch(int tp) { return tp == 32 ? 32 : tp + 4; }
// pixel-tile width for C channels: the switch points of the header comment
int tile_pixels(int64_t C) { return C <= 256 ? 128 : (C <= 512 ? 64 : 32); }
int padded_channels(int64_t C, int tp) { return (int)round_up((size_t)C, (size_t)(4096 / tp)); }
size_t lds_bytes(int cpad, int tp) {
  return sizeof(float) * ((size_t)cpad * tile_pitch(tp) + (size_t)kTJ * kWP + cpad) + (tp < 128 ? sizeof(double) * 128 : 0);
}

struct DensArgs {
  MapView v;
  int K, vecw, cpad;
  const float *mu, *W;
  const double* consts;
  float* ld;
  int* nearest;
  float* cld;
};

// one staged chunk (32 k) of the tiles TMIN .. NT - 1 of this wave: tiles below TMIN lie above the diagonal for this chunk
template <int NT, int TMIN, int XP>
__device__ __forceinline__ void mma_chunk(const float (*Xs)[XP], const float (*Ws)[kWP], const float* mus, int k0, int row0,
                                          int pix, int li, int lh, f32x16 (&acc)[NT]) {
#pragma unroll
  for (int s = 0; s < kKCh / 4; ++s) {
    const int k = k0 + 4 * s + 2 * lh;
    const float2 m = *reinterpret_cast<const float2*>(&mus[k]);
    const float bx = Xs[k][pix] - m.x, by = Xs[k + 1][pix] - m.y;
    float2 av[NT];
#pragma unroll
    for (int t = TMIN; t < NT; ++t) av[t] = *reinterpret_cast<const float2*>(&Ws[row0 + t * 32 + li][4 * s + 2 * lh]);
#pragma unroll
    for (int t = TMIN; t < NT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].x, bx, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].y, by, acc[t], 0, 0, 0);
    }
  }
}

template <class T, int LOAD, int TP>
__global__ __launch_bounds__(256) void pixdens_score_kernel(DensArgs a) {
  constexpr bool VEC = LOAD == kLoadVec;
  constexpr int XP = tile_pitch(TP);
  constexpr int NT = TP / 32;     // accumulator tiles of a wave = waves side by side along the pixels
  constexpr int NJ = 4 / NT;      // waves that share a pixel group: each owns 128 / NJ rows of a block
  constexpr int KCX = 4096 / TP;  // channels of one staged chunk of the tile
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float (*Xs)[XP] = reinterpret_cast<float (*)[XP]>(lds);                            // [cpad][XP]  x, widened
  float (*Ws)[kWP] = reinterpret_cast<float (*)[kWP]>(lds + (size_t)a.cpad * XP);    // [128][34]   chunk of W_c
  float* mus = lds + (size_t)a.cpad * XP + kTJ * kWP;                                // [cpad]      mu_c, 0 past C
  double* red = reinterpret_cast<double*>(mus + a.cpad);                             // [NJ][TP]    (NJ > 1)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int pg = wave % NT, js = wave / NT;
  const int pix = pg * 32 + li, row0 = js * NT * 32;
  const int C = a.v.C, K = a.K, cpad = a.cpad;
  const int64_t p0 = (int64_t)blockIdx.x * TP;

  // the tile: read once, resident for all K classes
  {
    int64_t off[4];
    const int nv = staged_pixels<LOAD, TP>(a.v, p0, tid, off);
    float xr[16];
    for (int k0 = 0; k0 < cpad; k0 += KCX) {
      if constexpr (LOAD == kLoadCLast) {
        load_x_cl<T, TP>(a.v, off[0], nv > 0, k0, tid, xr);
        store_x_cl<TP, false>(xr, Xs + k0, nullptr, 0, tid);
      } else {
        load_x<T, VEC, TP>(a.v, off, nv, k0, tid, xr);
        store_x<TP, false>(xr, Xs + k0, nullptr, 0, tid);
      }
    }
  }
  // the pixel whose sums this lane holds
  const int64_t pm = p0 + pix;
  const bool mine = pm < a.v.P;
  const int64_t gm = mine ? pm / a.v.HW : 0, qm = mine ? pm - gm * a.v.HW : 0;
  const bool writer = mine && lh == 0 && js == 0;
  // is any feature of this lane's pixel NaN or infinite?  One pass over the resident column, the two lane halves on
  // alternate channels: a sum that merely overflows (a finite outlier) is told apart from an invalid pixel below
  __syncthreads();
  bool badx = false;
  for (int k = lh; k < cpad; k += 2) badx = badx || !(fabsf(Xs[k][pix]) < INFINITY);
  badx = __shfl_xor((int)badx, 32, 64) != 0 || badx;

  double mx = -kInfD(), sum = 0.0, tot = 0.0;
  float best = -INFINITY;
  int bi = 0;
  bool bad = false;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  float wr[16], mr[kMaxC / 256];
  auto load_mu = [&](int c) {
#pragma unroll
    for (int i = 0; i < kMaxC / 256; ++i) {
      const int k = tid + 256 * i;
      mr[i] = k < C ? a.mu[(int64_t)c * C + k] : 0.f;
    }
  };
  load_w(a.W, C, C, 0, 0, tid, a.vecw != 0, wr);
  load_mu(0);
  int c = 0, j0 = 0, k0 = 0;
  while (c < K) {
    const int kend = j0 + kTJ < C ? j0 + kTJ : C;  // W_c[j, k] = 0 for k > j: nothing right of the block's last row
    __syncthreads();  // every wave has finished reading the previous chunk (and, at a class's first step, its mean)
    store_w(wr, Ws, tid);
    if (j0 == 0 && k0 == 0) {
#pragma unroll
      for (int i = 0; i < kMaxC / 256; ++i)
        if (tid + 256 * i < cpad) mus[tid + 256 * i] = mr[i];
    }
    __syncthreads();
    int nc = c, nj = j0, nk = k0 + kKCh;
    if (nk >= kend) {
      nk = 0;
      nj += kTJ;
      if (nj >= C) {
        nj = 0;
        ++nc;
      }
    }
    if (nc < K) {  // the next step's loads fly while the matrix cores consume this one
      load_w(a.W + (int64_t)nc * C * C, C, C, nj, nk, tid, a.vecw != 0, wr);
      if (nj == 0 && nk == 0) load_mu(nc);
    }
    {
      // tile t of this wave holds rows j0 + row0 + 32 t .. + 31: it needs the chunks up to k0 = j0 + row0 + 32 t
      const int tmin = (k0 - j0 - row0) / 32;  // (<= 0 below the diagonal block: every tile)
      constexpr int T1 = NT < 2 ? 0 : 1, T2 = NT < 3 ? 0 : 2, T3 = NT < 4 ? 0 : 3;  // (clamped: tmin < NT where it is taken)
      if (tmin <= 0) mma_chunk<NT, 0>(Xs, Ws, mus, k0, row0, pix, li, lh, acc);
      else if (tmin == 1 && T1) mma_chunk<NT, T1>(Xs, Ws, mus, k0, row0, pix, li, lh, acc);
      else if (tmin == 2 && T2) mma_chunk<NT, T2>(Xs, Ws, mus, k0, row0, pix, li, lh, acc);
      else if (tmin == 3 && T3) mma_chunk<NT, T3>(Xs, Ws, mus, k0, row0, pix, li, lh, acc);
    }
    if (nk == 0) {
      // the block is complete: acc[t][r] = z[j0 + row0 + 32 t + (r & 3) + 8 (r >> 2) + 4 lh] of pixel `pix`
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
          s0 = fmaf(acc[t][r], acc[t][r], s0);
          s1 = fmaf(acc[t][r + 1], acc[t][r + 1], s1);
          s2 = fmaf(acc[t][r + 2], acc[t][r + 2], s2);
          s3 = fmaf(acc[t][r + 3], acc[t][r + 3], s3);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      }
      tot += (double)((s0 + s1) + (s2 + s3));
      if (nj == 0) {  // the class is complete
        double d = tot + shfl_xor_f64(tot, 32);
        tot = 0.0;
        if constexpr (NJ > 1) {
          if (lh == 0) red[js * TP + pix] = d;
          __syncthreads();  // (the next write follows a later step's barriers)
          d = red[pix];
#pragma unroll
          for (int j = 1; j < NJ; ++j) d += red[j * TP + pix];
        }
        if (badx) d = __builtin_nan("");
        else if (!(d < kInfD())) d = kInfD();  // finite features whose squares overflow: lp_c = -inf
        const float lp = (float)(a.consts[c] - 0.5 * d);
        if (a.cld && writer) a.cld[(gm * K + c) * a.v.HW + qm] = lp;
        if (lp > best) {
          best = lp;
          bi = c;
        }
        const double v = (double)lp;
        if (v != v) bad = true;
        if (v > mx) {
          sum = (mx == -kInfD()) ? 1.0 : fma(sum, exp(mx - v), 1.0);
          mx = v;
        } else if (v == v && v > -kInfD()) {
          sum += exp(v - mx);
        }
      }
    }
    c = nc;
    j0 = nj;
    k0 = nk;
  }
  if (writer) {
    if (a.ld) a.ld[pm] = bad ? __builtin_nanf("") : (mx == -kInfD() || mx == kInfD() ? (float)mx : (float)(mx + log(sum)));
    if (a.nearest) a.nearest[pm] = bad ? 0 : bi;
  }
}

template <class T, int TP>
int launch_score(const DensArgs& a, int64_t G, int64_t H, hipStream_t s) {
  static std::atomic<uint64_t> allowed[3];
  const int64_t tiles = (a.v.P + TP - 1) / TP;
  if (tiles > kLim) return RUNIA_E_INVALID;  // (2^37 pixels in 32-pixel tiles: more workgroups than a grid holds)
  const unsigned grid = (unsigned)tiles;
  const size_t lds = lds_bytes(a.cpad, TP);
  auto go = [&](auto kernel, std::atomic<uint64_t>& done) {
    const int rc = runia_allow_dynamic_lds(reinterpret_cast<const void*>(kernel), kMaxLds, done);
    if (rc != RUNIA_OK) return rc;
    kernel<<<grid, 256, lds, s>>>(a);
    return runia_check_launch();
  };
  if (view_allows_vec(a.v, G, H, T::kBytes)) return go(pixdens_score_kernel<T, kLoadVec, TP>, allowed[0]);
  if (view_allows_clast(a.v, G, H, T::V)) return go(pixdens_score_kernel<T, kLoadCLast, TP>, allowed[1]);
  return go(pixdens_score_kernel<T, kLoadElem, TP>, allowed[2]);
}

}  // namespace

extern "C" int64_t runia_pixdens_tile_pixels(int64_t C) { return C >= 1 && C <= kMaxC ? tile_pixels(C) : 0; }

extern "C" int64_t runia_pixdens_workspace_bytes(int64_t C, int64_t K) {
  (void)C;
  (void)K;
  return 0;  // the tile, the sums and the running logsumexp live in LDS and registers: nothing scales with the pixels
}

extern "C" int runia_pixdens_score(const void* features, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn,
                                   int64_t sc, int64_t sh, int64_t sw, const float* means, const float* w_tril,
                                   const double* consts, int64_t K, float* log_density, int32_t* nearest,
                                   float* class_log_densities, void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  (void)workspace;
  (void)workspace_bytes;
  if (C < 1 || C > kMaxC || K < 1 || K > kMaxK || !elem_dtype_ok(dtype) || !view_ok(G, C, H, W, sn, sc, sh, sw))
    return RUNIA_E_INVALID;
  if (G == 0 || H * W == 0) return RUNIA_OK;
  if (!features || !means || !w_tril || !consts || (!log_density && !nearest && !class_log_densities)) return RUNIA_E_INVALID;
  DensArgs a;
  a.v = make_view(features, G, C, H, W, sn, sc, sh, sw);
  a.K = (int)K;
  a.vecw = (C % 4 == 0 && reinterpret_cast<uintptr_t>(w_tril) % 16 == 0) ? 1 : 0;
  const int tp = tile_pixels(C);
  a.cpad = padded_channels(C, tp);
  a.mu = means; a.W = w_tril; a.consts = consts;
  a.ld = log_density; a.nearest = nearest; a.cld = class_log_densities;
  hipStream_t s = as_stream(stream);
  return dispatch_elem(dtype, [&](auto t) {
    typedef decltype(t) T;
    if (tp == 128) return launch_score<T, 128>(a, G, H, s);
    if (tp == 64) return launch_score<T, 64>(a, G, H, s);
    return launch_score<T, 32>(a, G, H, s);
  });
}
