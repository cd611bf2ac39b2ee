// Bootstrap replicates of the OoD metrics (evaluation/bootstrap.py): AUROC / FPR@95 / AUPR of B Poisson(1)
// resamples of one InD / OoD score table, without anything of size B x N in memory.
//   * runia_boot_keys_*: the metrics.hip key of every score (sigmoid in the scores' dtype when any score lies outside [0, 1] or
//     is NaN, f64 sortable key, ties = equal keys) as int64 whose ascending signed order is the descending score order.  The
//     caller orders them once per method (a device sort of 8-byte keys: plumbing).
//   * runia_boot_metrics: one workgroup (512 threads) per Philox block of FOUR replicates walks the whole sorted table in tiles
//     of 4096 rows.  A thread owns kItems consecutive rows of a tile: it draws the rows' weights (boot_weights.hpp: a pure function of seed, replicate
//     and row / group id) in registers, the workgroup scans the per-thread weight sums (InD and OoD weight of a replicate packed
//     into the halves of one 32-bit word: a tile holds at most 13 * 4096 < 2^16 of either), and every thread then walks its rows
//     with the cumulative weights and the cumulative weights at the run end before it.  The carries across tiles - cumulative
//     weights, and those at the last run end so far - are the same in every thread's registers.  No atomics on global memory,
//     no communication between workgroups: the same bits from call to call and for any split of the replicates into calls.
//   * FPR@95 needs the replicate's total InD weight P, known only after the walk: the walk leaves the cumulative weights at
//     every tile end in the workspace (64 bytes per tile and workgroup), the first tile whose end reaches 19 P / 20 is found
//     from them, and the walk is repeated from there until the first run end that reaches it (one or two tiles unless a tie
//     run is longer).
#include "common.hpp"
#include "boot_weights.hpp"

namespace {

#ifndef BOOT_THREADS
#define BOOT_THREADS 512
#endif
#ifndef BOOT_ITEMS
#define BOOT_ITEMS 8
#endif
constexpr int kThreads = BOOT_THREADS;     // one workgroup per CU at B = 1000: 512 threads are two waves per SIMD
constexpr int kWaves = kThreads / 64;
constexpr int kItems = BOOT_ITEMS;         // consecutive rows of a tile per thread
constexpr int kBootTile = kThreads * kItems;
static_assert(kThreads % 64 == 0 && kThreads <= 1024 && kItems >= 1, "whole waves");
static_assert(runia_boot::kMaxWeight * kBootTile < 65536, "a tile's InD / OoD weight fits half a 32-bit word");

typedef unsigned long long u64;

// ---- keys -----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void boot_probe_kernel(const T* __restrict__ ind, int64_t n_ind, const T* __restrict__ ood,
                                                         int64_t n_ood, unsigned* __restrict__ any_outside) {
  const int64_t n = n_ind + n_ood;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const T v = (i < n_ind) ? ind[i] : ood[i - n_ind];
    bad = bad || !(v >= (T)0 && v <= (T)1);
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) *any_outside = 1u;  // (cleared in front of the launch; every writer writes 1)
}

template <typename T>
__global__ __launch_bounds__(256) void boot_keys_kernel(const T* __restrict__ ind, int64_t n_ind, const T* __restrict__ ood,
                                                        int64_t n_ood, const unsigned* __restrict__ any_outside,
                                                        int64_t* __restrict__ keys) {
  const int64_t n = n_ind + n_ood;
  const bool squash = *any_outside != 0u;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    keys[i] = signed_view(score_key<T>((i < n_ind) ? ind[i] : ood[i - n_ind], squash));  // the key of metrics.hip, for a sort of int64
}

template <typename T>
int boot_keys(const T* ind, int64_t n_ind, const T* ood, int64_t n_ood, int64_t* keys, unsigned* any_outside,
              runia_stream_t stream) {
  if (n_ind < 1 || n_ood < 1 || n_ind + n_ood >= (1ll << 31)) return RUNIA_E_INVALID;
  if (!ind || !ood || !keys || !any_outside) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(any_outside, 0, sizeof(unsigned), s) != hipSuccess) return RUNIA_E_LAUNCH;
  const unsigned grid = runia_stream_grid(n_ind + n_ood, 256);
  boot_probe_kernel<T><<<grid < 1024u ? grid : 1024u, 256, 0, s>>>(ind, n_ind, ood, n_ood, any_outside);
  boot_keys_kernel<T><<<grid, 256, 0, s>>>(ind, n_ind, ood, n_ood, any_outside, keys);
  return runia_check_launch();
}

// ---- replicates -----------------------------------------------------------------------------------------------------------
struct TileRec { u64 tp[4], fp[4]; };  // cumulative InD / OoD weight of the four replicates at the end of a tile

struct BootShared {
  uint32_t wtot[kWaves][4];  // [wave][replicate]: the wave's packed weight
  int wend[kWaves];          // the last thread of the wave (and before) that holds a run end, -1: none
  uint32_t endval[kThreads][4];  // packed cumulative weight inside the tile at the thread's last run end
};

// What a thread knows of its rows of a tile after the workgroup's scan.  Packed words: InD weight in the low half, OoD weight in
// the high half, counted from the start of the tile.
struct Front {
  uint32_t wp[kItems];  // per row: four 4-bit weights | InD << 16 | run end << 17
  uint32_t start[4];    // before the thread's first row
  uint32_t pend[4];     // at the last run end of the tile before the thread's first row (has_pend)
  uint32_t last[4];     // at the tile's last run end (has_last)
  uint32_t total[4];    // of the whole tile
  bool has_pend, has_last;
};

__device__ __forceinline__ void boot_front(const int64_t* __restrict__ keys, const int32_t* __restrict__ rows,
                                           const int32_t* __restrict__ grp, int64_t n, int64_t n_ind, uint64_t seed,
                                           uint32_t quad, int64_t tile, BootShared& sh, Front& f) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = tile * kBootTile + (int64_t)tid * kItems;
  int64_t k[kItems + 1];
  int32_t r[kItems];
#pragma unroll
  for (int c = 0; c < kItems; ++c) {
    const int64_t i = i0 + c;
    k[c] = (i < n) ? keys[i] : 0;
    int32_t row = (i < n) ? rows[i] : 0;
    row = row < 0 ? 0 : (row >= (int32_t)n ? (int32_t)n - 1 : row);  // (a caller's bad row id must not become a bad address)
    r[c] = row;
  }
  k[kItems] = (i0 + kItems < n) ? keys[i0 + kItems] : 0;
  uint32_t id[kItems];
#pragma unroll
  for (int c = 0; c < kItems; ++c) id[c] = grp ? (uint32_t)grp[r[c]] : (uint32_t)r[c];
  uint32_t acc[4] = {0u, 0u, 0u, 0u}, lastend[4] = {0u, 0u, 0u, 0u};
  bool has_end = false;
#pragma unroll
  for (int c = 0; c < kItems; ++c) {
    const int64_t i = i0 + c;
    const bool valid = i < n;
    const bool end = valid && (i == n - 1 || k[c] != k[c + 1]);
    const uint32_t w = valid ? runia_boot::quad_weights(seed, quad, id[c]) : 0u;
    const bool is_ind = r[c] < n_ind;
    const int sh16 = is_ind ? 0 : 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += ((w >> (4 * j)) & 15u) << sh16;
    f.wp[c] = w | ((is_ind ? 1u : 0u) << 16) | ((end ? 1u : 0u) << 17);
    if (end) {
#pragma unroll
      for (int j = 0; j < 4; ++j) lastend[j] = acc[j];
      has_end = true;
    }
  }
  struct Run { uint32_t x[4]; int m; } run;  // packed weights up to and with the thread; the last thread with a run end
#pragma unroll
  for (int j = 0; j < 4; ++j) run.x[j] = acc[j];
  run.m = has_end ? tid : -1;
  run = wave_scan_incl(run, [](const Run& lower, Run own) {
#pragma unroll
    for (int j = 0; j < 4; ++j) own.x[j] += lower.x[j];
    own.m = max(own.m, lower.m);
    return own;
  });
  const uint32_t(&x)[4] = run.x;
  const int m = run.m;
  __syncthreads();  // the previous tile's reads of `sh` are over
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < 4; ++j) sh.wtot[wave][j] = x[j];
    sh.wend[wave] = m;
  }
  __syncthreads();
  uint32_t off[4] = {0u, 0u, 0u, 0u};
  int before = -1, all = -1;
#pragma unroll
  for (int j = 0; j < 4; ++j) f.total[j] = 0u;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t t = sh.wtot[w][j];
      if (w < wave) off[j] += t;
      f.total[j] += t;
    }
    const int e = sh.wend[w];
    if (w < wave) before = max(before, e);
    all = max(all, e);
  }
  int pe = lane_up(m, 1);
  if (lane == 0) pe = -1;
  pe = max(pe, before);
#pragma unroll
  for (int j = 0; j < 4; ++j) f.start[j] = off[j] + x[j] - acc[j];
  if (has_end) {
#pragma unroll
    for (int j = 0; j < 4; ++j) sh.endval[tid][j] = f.start[j] + lastend[j];
  }
  __syncthreads();
  f.has_pend = pe >= 0;
  f.has_last = all >= 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f.pend[j] = f.has_pend ? sh.endval[pe][j] : 0u;
    f.last[j] = f.has_last ? sh.endval[all][j] : 0u;
  }
}

// precision at a curve point; 1 where nothing has been counted yet (the curve's closing point, rows that all drew 0)
__device__ __forceinline__ double boot_precision(u64 tp, u64 fp) {
  return (tp + fp == 0ull) ? 1.0 : (double)tp / (double)(tp + fp);
}

__global__ __launch_bounds__(kThreads) void boot_replicates_kernel(const int64_t* __restrict__ keys,
                                                                   const int32_t* __restrict__ rows,
                                                                   const int32_t* __restrict__ grp, int64_t n, int64_t n_ind,
                                                                   uint64_t seed, int64_t first, int64_t n_boot, uint32_t quad0,
                                                                   double* __restrict__ out, TileRec* recs,
                                                                   int64_t ntiles) {
  __shared__ BootShared sh;
  __shared__ u64 sroc[kWaves][4];
  __shared__ double spr[kWaves][4];
  __shared__ int tstart_s;  // (fewer than 2^20 tiles)
  __shared__ unsigned hit_tid[4];
  __shared__ u64 hit_fp[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t quad = quad0 + blockIdx.x;
  TileRec* rec = recs + (size_t)blockIdx.x * (size_t)ntiles;

  // ---- the walk: AUROC and AUPR sums, the tile-end records ----
  u64 base_tp[4] = {0, 0, 0, 0}, base_fp[4] = {0, 0, 0, 0};  // cumulative weight in front of the tile
  u64 prev_tp[4] = {0, 0, 0, 0}, prev_fp[4] = {0, 0, 0, 0};  // ... at the last run end in front of the tile
  u64 roc[4] = {0, 0, 0, 0};
  double pr[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t tile = 0; tile < ntiles; ++tile) {
    Front f;
    boot_front(keys, rows, grp, n, n_ind, seed, quad, tile, sh, f);
    u64 tp[4], fp[4], ptp[4], pfp[4];
    double pprec[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tp[j] = base_tp[j] + (f.start[j] & 0xffffu);
      fp[j] = base_fp[j] + (f.start[j] >> 16);
      ptp[j] = f.has_pend ? base_tp[j] + (f.pend[j] & 0xffffu) : prev_tp[j];
      pfp[j] = f.has_pend ? base_fp[j] + (f.pend[j] >> 16) : prev_fp[j];
      pprec[j] = boot_precision(ptp[j], pfp[j]);
    }
#pragma unroll
    for (int c = 0; c < kItems; ++c) {
      const uint32_t wp = f.wp[c];
      const bool is_ind = (wp >> 16) & 1u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u64 w = (wp >> (4 * j)) & 15u;
        tp[j] += is_ind ? w : 0ull;
        fp[j] += is_ind ? 0ull : w;
      }
      if ((wp >> 17) & 1u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          roc[j] += (fp[j] - pfp[j]) * (tp[j] + ptp[j]);
          const double prec = boot_precision(tp[j], fp[j]);
          pr[j] += (double)(tp[j] - ptp[j]) * (prec + pprec[j]);
          ptp[j] = tp[j]; pfp[j] = fp[j]; pprec[j] = prec;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (f.has_last) {
        prev_tp[j] = base_tp[j] + (f.last[j] & 0xffffu);
        prev_fp[j] = base_fp[j] + (f.last[j] >> 16);
      }
      base_tp[j] += f.total[j] & 0xffffu;
      base_fp[j] += f.total[j] >> 16;
    }
    if (tid == 0) {
      TileRec t;
#pragma unroll
      for (int j = 0; j < 4; ++j) { t.tp[j] = base_tp[j]; t.fp[j] = base_fp[j]; }
      rec[tile] = t;
    }
  }
  // the sums of the workgroup, in a fixed order
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    roc[j] = wave_sum(roc[j]);
    pr[j] = wave_sum(pr[j]);
    if (lane == 0) { sroc[wave][j] = roc[j]; spr[wave][j] = pr[j]; }
  }
  if (tid == 0) tstart_s = (int)ntiles;
  __syncthreads();  // (also: the tile records are visible to the workgroup)

  // ---- FPR@95: the first run end with 20 TP >= 19 P ----
  u64 P[4], N[4];
  bool found[4];
  u64 fpr_fp[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    P[j] = base_tp[j];
    N[j] = base_fp[j];
    const int64_t b = (int64_t)quad * 4 + j;
    found[j] = !(b >= first && b < first + n_boot && P[j] > 0ull && N[j] > 0ull);  // nothing to find
  }
  {
    int tmin = (int)ntiles;
    for (int64_t t = tid; t < ntiles && tmin == (int)ntiles; t += kThreads) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!found[j] && 20ull * rec[t].tp[j] >= 19ull * P[j]) tmin = (int)t;
    }
    if (tmin < (int)ntiles) atomicMin(&tstart_s, tmin);  // (LDS, integer)
  }
  __syncthreads();
  for (int64_t tile = tstart_s; tile < ntiles && !(found[0] && found[1] && found[2] && found[3]); ++tile) {
    Front f;
    boot_front(keys, rows, grp, n, n_ind, seed, quad, tile, sh, f);
    if (tid < 4) hit_tid[tid] = ~0u;
    u64 tp[4], fp[4], my_fp[4] = {0, 0, 0, 0};
    bool hit[4] = {false, false, false, false};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u64 btp = tile > 0 ? rec[tile - 1].tp[j] : 0ull, bfp = tile > 0 ? rec[tile - 1].fp[j] : 0ull;
      tp[j] = btp + (f.start[j] & 0xffffu);
      fp[j] = bfp + (f.start[j] >> 16);
    }
#pragma unroll
    for (int c = 0; c < kItems; ++c) {
      const uint32_t wp = f.wp[c];
      const bool is_ind = (wp >> 16) & 1u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u64 w = (wp >> (4 * j)) & 15u;
        tp[j] += is_ind ? w : 0ull;
        fp[j] += is_ind ? 0ull : w;
        if (((wp >> 17) & 1u) && !found[j] && !hit[j] && 20ull * tp[j] >= 19ull * P[j]) { hit[j] = true; my_fp[j] = fp[j]; }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (hit[j]) atomicMin(&hit_tid[j], (unsigned)tid);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (hit[j] && hit_tid[j] == (unsigned)tid) hit_fp[j] = my_fp[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (!found[j] && hit_tid[j] != ~0u) { found[j] = true; fpr_fp[j] = hit_fp[j]; }
    __syncthreads();  // (hit_tid / hit_fp are rewritten by the next tile)
  }

  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t b = (int64_t)quad * 4 + j;
      if (b < first || b >= first + n_boot) continue;
      double* o = out + (b - first) * 3;
      if (P[j] == 0ull || N[j] == 0ull) {  // a degenerate replicate: one side drew nothing
        o[0] = NAN; o[1] = NAN; o[2] = NAN;
        continue;
      }
      u64 r = sroc[0][j];
      double q = spr[0][j];
      for (int w = 1; w < kWaves; ++w) { r += sroc[w][j]; q += spr[w][j]; }  // (the waves in order)
      o[0] = (double)r / (double)(2ull * P[j] * N[j]);
      o[1] = (double)fpr_fp[j] / (double)N[j];
      o[2] = 0.5 * q / (double)P[j];
    }
  }
}

int64_t boot_tiles(int64_t n) { return (n + kBootTile - 1) / kBootTile; }
int64_t boot_max_quads(int64_t n_boot) { return (n_boot + 3) / 4 + 1; }  // a range that starts inside a block touches one more

}  // namespace

extern "C" int runia_boot_tile_rows(void) { return kBootTile; }

extern "C" int runia_boot_keys_f32(const float* ind_scores, int64_t n_ind, const float* ood_scores, int64_t n_ood, int64_t* keys,
                                   unsigned* any_outside, runia_stream_t stream) {
  return boot_keys<float>(ind_scores, n_ind, ood_scores, n_ood, keys, any_outside, stream);
}

extern "C" int runia_boot_keys_f64(const double* ind_scores, int64_t n_ind, const double* ood_scores, int64_t n_ood, int64_t* keys,
                                   unsigned* any_outside, runia_stream_t stream) {
  return boot_keys<double>(ind_scores, n_ind, ood_scores, n_ood, keys, any_outside, stream);
}

// one record per tile and workgroup (a workgroup = four replicates)
static size_t boot_records_bytes(int64_t quads, int64_t n) { return (size_t)quads * (size_t)boot_tiles(n) * sizeof(TileRec); }
extern "C" size_t runia_boot_workspace_bytes(int64_t n, int64_t n_boot) {
  if (n <= 0 || n_boot <= 0) return 0;
  return boot_records_bytes(boot_max_quads(n_boot), n);
}

extern "C" int runia_boot_metrics(const int64_t* sorted_keys, const int32_t* sorted_rows, int64_t n, int64_t n_ind,
                                  const int32_t* group_of_row, uint64_t seed, int64_t first_replicate, int64_t n_boot, double* out,
                                  void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  // sizes first: the AUROC sum is at most 13^2 * 2 * n_ind * n_ood, which has to stay below 2^64
  if (n < 2 || n >= (1ll << 31) || n_ind < 1 || n_ind >= n) return RUNIA_E_INVALID;
  if (n_ind * (n - n_ind) >= (1ll << 55)) return RUNIA_E_INVALID;  // (both factors are below 2^31)
  if (n_boot < 1 || first_replicate < 0 || n_boot > (1ll << 31) || first_replicate > (1ll << 31) - n_boot) return RUNIA_E_INVALID;
  if (!sorted_keys || !sorted_rows || !out) return RUNIA_E_INVALID;
  const int64_t q0 = first_replicate >> 2, q1 = (first_replicate + n_boot - 1) >> 2, ntiles = boot_tiles(n);
  if (ws_refused(workspace, workspace_bytes, boot_records_bytes(q1 - q0 + 1, n), 8)) return RUNIA_E_WORKSPACE;
  boot_replicates_kernel<<<(unsigned)(q1 - q0 + 1), kThreads, 0, as_stream(stream)>>>(
      sorted_keys, sorted_rows, group_of_row, n, n_ind, seed, first_replicate, n_boot, (uint32_t)q0, out,
      reinterpret_cast<TileRec*>(workspace), ntiles);
  return runia_check_launch();
}

extern "C" int runia_boot_weight_of_word_host(uint32_t word) { return (int)runia_boot::weight_of_word(word); }

extern "C" int runia_boot_weights_host(uint64_t seed, int64_t first_replicate, int64_t n_boot, const int32_t* ids, int64_t n,
                                       uint8_t* out) {
  if (n_boot < 1 || n < 1 || first_replicate < 0 || !ids || !out) return RUNIA_E_INVALID;
  if (n_boot > (1ll << 31) || first_replicate > (1ll << 31) - n_boot) return RUNIA_E_INVALID;
  for (int64_t r = 0; r < n_boot; ++r)
    for (int64_t i = 0; i < n; ++i)
      out[r * n + i] = (uint8_t)runia_boot::weight(seed, (uint64_t)(first_replicate + r), (uint32_t)ids[i]);
  return RUNIA_OK;
}
