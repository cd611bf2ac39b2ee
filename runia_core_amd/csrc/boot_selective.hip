// Bootstrap replicates of the selective-prediction summaries (evaluation/selective_bootstrap.py): AURC, AUGRC and
// the risk at full coverage of B Poisson(1) resamples of one confidence / loss table, without anything of size B x N in memory.
// A replicate is the tie-aware definition of selective.hip on the table with every row physically repeated w times, w the
// weight of boot_weights.hpp (a pure function of seed, replicate and row / group id: the resample runia_boot_metrics draws).
//   * The ordered table is that of runia_sel_keys_* (keys int64 ascending = descending confidence, rows int32).
//   * runia_boot_sel_metrics: the shape of bootstrap.hip's walk.  One workgroup (512 threads) per Philox block of FOUR
//     replicates walks the whole table in tiles of 4096 rows; a thread owns kItems consecutive rows.  It draws the rows' weights
//     in registers and gathers their losses (f64) once for the four replicates; the workgroup scans, per replicate, the weight
//     count (integer), the weighted loss sum w l (f64, Hillis-Steele inside a wave, then the waves in order) and the last run
//     end at or before every thread, whose cumulative weight and loss are parked in LDS.  Every thread then walks its rows
//     with (e, L_e) running and (s, L_s) of the run end in front of them.  The carries across tiles - cumulative weight and
//     loss, and those at the last run end so far - are the same numbers for every thread: a run over many tiles and a tile
//     without a run end take the same path.  One walk: n' enters once at the end.
//   * Where the registers go.  The run terms below are heavy (a division loop, log1p), so the walk's row loop is a real loop
//     over the rows' weight words and losses, parked in LDS by their owner (32 inlined copies of the run terms spilled), and
//     the carries live in LDS once instead of in every thread's registers: 219 VGPRs at two waves per SIMD, no scratch.
//   * A run of equal keys with m = e - s > 0 copies adds, in closed form (no loop over the copies of a long run),
//         sum_{k = s+1 .. e} Lbar_k     = m L_s + d (m + 1) / 2                       d = L_e - L_s
//         sum_{k = s+1 .. e} Lbar_k / k = L_s dH + (d / m)(m - s dH)                   dH = sum_{k = s+1 .. e} 1 / k
//     m <= 32: the per-copy terms (L_s + j d / m) / (s + j) themselves.  m > 32: dH = [sum_{k = s+1 .. 32} 1 / k] +
//     log1p((e - s0) / s0) + t(e) - t(s0), s0 = max(s, 32), t(x) = 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6) - the next term
//     of the series is 1 / (240 x^8) < 4e-15 at x = 32.
//   * The cumulative loss at a sorted position is ALWAYS formed as base + (start of the thread + the thread's running sum),
//     whoever asks for it, so a carried L_s has the bits its owner gave it; with integer-valued losses every sum is exact.
//     f64 sums in an order fixed by n alone, no atomics, no communication between workgroups: the same bits from call to call
//     and for any split of the replicates into calls.
#include "common.hpp"
#include "boot_weights.hpp"

namespace {

constexpr int kThreads = 512;  // one workgroup per CU at B = 1000: two waves per SIMD
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;      // consecutive rows of a tile per thread
constexpr int kTile = kThreads * kItems;
constexpr int kDirect = 32;    // runs of up to this many copies are summed copy by copy; also s0 of the closed form
static_assert(kThreads % 64 == 0 && kThreads <= 1024, "whole waves");

typedef unsigned long long u64;

// The carries across tiles: the same numbers for every thread, so they live in LDS once (two copies: thread 0 writes the next
// tile's while the others may still read this tile's).
struct Carry {
  u64 base_w[4], prev_w[4];        // cumulative weight in front of the tile / at the last run end in front of it
  double base_l[4], prev_l[4];     // the weighted loss likewise
};

struct BsShared {
  uint32_t wtot[kWaves][4];     // [wave][replicate]: the wave's weight
  double ltot[kWaves][4];       // ... and weighted loss
  int wend[kWaves];             // the last thread of the wave (and before) that holds a run end, -1: none
  uint32_t endw[kThreads][4];   // cumulative weight inside the tile at the thread's last run end
  double endl[kThreads][4];     // ... and weighted loss
  uint32_t wp[kItems][kThreads];  // per row of the thread: four 4-bit weights | run end << 16 (read back by its owner alone:
  double v[kItems][kThreads];     // the walk's row loop stays a loop) and the row's loss
  Carry carry[2];
};

// What a thread knows of its rows of a tile after the workgroup's scan.
struct Front {
  uint32_t start_w[4];  // weight of the tile's rows in front of the thread's first row
  double start_l[4];    // ... and weighted loss
  u64 base_w[4], pw[4];     // cumulative weight in front of the tile / at the last run end in front of the thread's rows
  double base_l[4], pl[4];  // the weighted loss likewise
};

__device__ __forceinline__ double bs_load(const void* p, int is_f64, int64_t i) {
  return is_f64 ? reinterpret_cast<const double*>(p)[i] : (double)reinterpret_cast<const float*>(p)[i];
}

__device__ __forceinline__ void bs_front(const int64_t* __restrict__ keys, const int32_t* __restrict__ rows,
                                         const void* __restrict__ loss, int loss_f64, const int32_t* __restrict__ grp, int64_t n,
                                         uint64_t seed, uint32_t quad, int64_t tile, BsShared& sh, Front& f) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = tile * kTile + (int64_t)tid * kItems;
  int64_t k[kItems + 1];
  uint32_t id[kItems];
  double v[kItems];
#pragma unroll
  for (int c = 0; c < kItems; ++c) {
    const int64_t i = i0 + c;
    k[c] = (i < n) ? keys[i] : 0;
    int32_t row = (i < n) ? rows[i] : 0;
    row = row < 0 ? 0 : (row >= (int32_t)n ? (int32_t)n - 1 : row);  // (a caller's bad row id must not become a bad address)
    v[c] = (i < n) ? bs_load(loss, loss_f64, row) : 0.0;
    id[c] = grp ? (uint32_t)grp[row] : (uint32_t)row;
  }
  k[kItems] = (i0 + kItems < n) ? keys[i0 + kItems] : 0;
  uint32_t accw[4] = {0u, 0u, 0u, 0u}, lastw[4] = {0u, 0u, 0u, 0u};
  double accl[4] = {0.0, 0.0, 0.0, 0.0}, lastl[4] = {0.0, 0.0, 0.0, 0.0};
  uint32_t wp[kItems];
  bool has_end = false;
#pragma unroll
  for (int c = 0; c < kItems; ++c) {
    const int64_t i = i0 + c;
    const bool valid = i < n;
    const bool end = valid && (i == n - 1 || k[c] != k[c + 1]);
    const uint32_t w = valid ? runia_boot::quad_weights(seed, quad, id[c]) : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t wj = (w >> (4 * j)) & 15u;
      accw[j] += wj;
      accl[j] += (double)wj * v[c];  // (the walk repeats exactly this sum)
    }
    wp[c] = w | ((end ? 1u : 0u) << 16);
    if (end) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { lastw[j] = accw[j]; lastl[j] = accl[j]; }
      has_end = true;
    }
  }
  // weighted loss and weight up to and with the thread; the last thread with a run end
  struct Run { double l[4]; uint32_t w[4]; int m; } run;
#pragma unroll
  for (int j = 0; j < 4; ++j) { run.w[j] = accw[j]; run.l[j] = accl[j]; }
  run.m = has_end ? tid : -1;
  run = wave_scan_incl(run, [](const Run& lower, Run own) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { own.w[j] += lower.w[j]; own.l[j] = lower.l[j] + own.l[j]; }
    own.m = max(own.m, lower.m);
    return own;
  });
  const uint32_t(&xw)[4] = run.w;
  const double(&xl)[4] = run.l;
  const int m = run.m;
  // exclusive values of the lane
  uint32_t ew[4];
  double el[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ew[j] = lane_up(xw[j], 1);
    el[j] = lane_up(xl[j], 1);
    if (lane == 0) { ew[j] = 0u; el[j] = 0.0; }
  }
  int pe = lane_up(m, 1);
  if (lane == 0) pe = -1;
  __syncthreads();  // the previous tile's reads of `sh` are over
#pragma unroll
  for (int c = 0; c < kItems; ++c) { sh.wp[c][tid] = wp[c]; sh.v[c][tid] = v[c]; }
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { sh.wtot[wave][j] = xw[j]; sh.ltot[wave][j] = xl[j]; }
    sh.wend[wave] = m;
  }
  __syncthreads();
  uint32_t offw[4] = {0u, 0u, 0u, 0u}, totw[4] = {0u, 0u, 0u, 0u};
  double offl[4] = {0.0, 0.0, 0.0, 0.0}, totl[4] = {0.0, 0.0, 0.0, 0.0};
  int before = -1, all = -1;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t tw = sh.wtot[w][j];
      const double tl = sh.ltot[w][j];
      if (w < wave) { offw[j] += tw; offl[j] += tl; }
      totw[j] += tw;
      totl[j] += tl;
    }
    const int e = sh.wend[w];
    if (w < wave) before = max(before, e);
    all = max(all, e);
  }
  pe = max(pe, before);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f.start_w[j] = offw[j] + ew[j];
    f.start_l[j] = offl[j] + el[j];
  }
  if (has_end) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sh.endw[tid][j] = f.start_w[j] + lastw[j];
      sh.endl[tid][j] = f.start_l[j] + lastl[j];
    }
  }
  __syncthreads();
  const Carry& cy = sh.carry[tile & 1];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f.base_w[j] = cy.base_w[j];
    f.base_l[j] = cy.base_l[j];
    f.pw[j] = pe >= 0 ? f.base_w[j] + sh.endw[pe][j] : cy.prev_w[j];
    f.pl[j] = pe >= 0 ? f.base_l[j] + sh.endl[pe][j] : cy.prev_l[j];
  }
  if (tid == 0) {
    Carry& nx = sh.carry[(tile + 1) & 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nx.prev_w[j] = all >= 0 ? f.base_w[j] + sh.endw[all][j] : cy.prev_w[j];
      nx.prev_l[j] = all >= 0 ? f.base_l[j] + sh.endl[all][j] : cy.prev_l[j];
      nx.base_w[j] = f.base_w[j] + totw[j];
      nx.base_l[j] = f.base_l[j] + totl[j];
    }
  }
}

// t(x) of the header comment: H_x = log x + gamma + t(x) + O(x^-8)
__device__ __forceinline__ double bs_tail(double x) {
  const double r = 1.0 / x, r2 = r * r;
  return r * (0.5 - r * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0))));
}

// sum_{k = s+1 .. e} 1 / k for e - s > kDirect
__device__ __forceinline__ double bs_delta_h(u64 s, u64 e) {
  double h = 0.0;
  u64 s0 = s;
  if (s < (u64)kDirect) {  // (e > s + kDirect >= kDirect)
    for (int k = (int)s + 1; k <= kDirect; ++k) h += 1.0 / (double)k;
    s0 = (u64)kDirect;
  }
  const double x0 = (double)s0, xe = (double)e;
  return h + (log1p((xe - x0) / x0) + (bs_tail(xe) - bs_tail(x0)));
}

// the terms of one run with m = e - s > 0 copies: -> sum Lbar_k / k, sum Lbar_k
__device__ __forceinline__ void bs_run_terms(u64 s, u64 e, double ls, double le, double& a, double& g) {
  const u64 m = e - s;
  const double md = (double)m, sd = (double)s, d = le - ls, slope = d / md;
  g += md * ls + d * (md + 1.0) * 0.5;
  if (m <= (u64)kDirect) {
    double t = 0.0;
    for (int j = 1; j <= (int)m; ++j) t += (ls + (double)j * slope) / (sd + (double)j);
    a += t;
  } else {
    const double dh = bs_delta_h(s, e);
    a += ls * dh + slope * (md - sd * dh);
  }
}

__global__ __launch_bounds__(kThreads) void boot_sel_kernel(const int64_t* __restrict__ keys, const int32_t* __restrict__ rows,
                                                            const void* __restrict__ loss, int loss_f64,
                                                            const int32_t* __restrict__ grp, int64_t n, uint64_t seed,
                                                            int64_t first, int64_t n_boot, uint32_t quad0,
                                                            double* __restrict__ out, int64_t ntiles) {
  __shared__ BsShared sh;
  __shared__ double sa[kWaves][4], sg[kWaves][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t quad = quad0 + blockIdx.x;

  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sh.carry[0].base_w[j] = 0ull; sh.carry[0].prev_w[j] = 0ull;
      sh.carry[0].base_l[j] = 0.0; sh.carry[0].prev_l[j] = 0.0;
    }
  }
  double sum_a[4] = {0.0, 0.0, 0.0, 0.0}, sum_g[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t tile = 0; tile < ntiles; ++tile) {
    Front f;
    bs_front(keys, rows, loss, loss_f64, grp, n, seed, quad, tile, sh, f);
    uint32_t tw[4];   // weight inside the tile up to the row
    double run[4];    // the thread's running weighted loss
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tw[j] = f.start_w[j];
      run[j] = 0.0;
    }
#pragma unroll 1
    for (int c = 0; c < kItems; ++c) {
      const uint32_t wp = sh.wp[c][tid];
      const double v = sh.v[c][tid];
      const bool end = (wp >> 16) & 1u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t wj = (wp >> (4 * j)) & 15u;
        tw[j] += wj;
        run[j] += (double)wj * v;
        if (end) {
          const u64 cw = f.base_w[j] + tw[j];
          const double cl = f.base_l[j] + (f.start_l[j] + run[j]);
          if (cw > f.pw[j]) bs_run_terms(f.pw[j], cw, f.pl[j], cl, sum_a[j], sum_g[j]);
          f.pw[j] = cw;
          f.pl[j] = cl;
        }
      }
    }
  }
  // the sums of the workgroup, in a fixed order
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sum_a[j] = wave_sum(sum_a[j]);
    sum_g[j] = wave_sum(sum_g[j]);
    if (lane == 0) { sa[wave][j] = sum_a[j]; sg[wave][j] = sum_g[j]; }
  }
  __syncthreads();
  if (tid == 0) {
    const Carry& cy = sh.carry[ntiles & 1];  // (what the last tile left)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t b = (int64_t)quad * 4 + j;
      if (b < first || b >= first + n_boot) continue;
      double* o = out + (b - first) * 4;
      const double np = (double)cy.base_w[j];
      o[3] = np;
      if (cy.base_w[j] == 0ull) {  // an empty replicate: every row drew 0
        o[0] = NAN; o[1] = NAN; o[2] = NAN;
        continue;
      }
      double a = sa[0][j], g = sg[0][j];
      for (int w = 1; w < kWaves; ++w) { a += sa[w][j]; g += sg[w][j]; }  // (the waves in order)
      o[0] = a / np;
      o[1] = g / (np * np);
      o[2] = cy.base_l[j] / np;
    }
  }
}

}  // namespace

extern "C" int runia_boot_sel_tile_rows(void) { return kTile; }

extern "C" int runia_boot_sel_metrics(const int64_t* sorted_keys, const int32_t* sorted_rows, const void* loss, int loss_f64,
                                      int64_t n, const int32_t* group_of_row, uint64_t seed, int64_t first_replicate,
                                      int64_t n_boot, double* out, runia_stream_t stream) {
  if (n < 1 || n >= (1ll << 31)) return RUNIA_E_INVALID;
  if (n_boot < 1 || first_replicate < 0 || n_boot > (1ll << 31) || first_replicate > (1ll << 31) - n_boot) return RUNIA_E_INVALID;
  if (!sorted_keys || !sorted_rows || !loss || !out) return RUNIA_E_INVALID;
  const int64_t q0 = first_replicate >> 2, q1 = (first_replicate + n_boot - 1) >> 2, ntiles = (n + kTile - 1) / kTile;
  boot_sel_kernel<<<(unsigned)(q1 - q0 + 1), kThreads, 0, as_stream(stream)>>>(
      sorted_keys, sorted_rows, loss, loss_f64, group_of_row, n, seed, first_replicate, n_boot, (uint32_t)q0, out, ntiles);
  return runia_check_launch();
}
