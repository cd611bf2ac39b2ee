// Selective prediction (evaluation/selective.py): the risk-coverage curve of a confidence / loss table and its
// summaries - AURC, AUGRC, risk at a coverage, coverage at a risk, equal-mass bins - with ties treated as ties.
//   * runia_sel_keys_*: the f64 sortable key of every confidence as int64 whose ascending signed order is the descending
//     confidence order (f32 widened exactly, -0.0 and +0.0 one key, +-inf ordinary); a device word records a NaN.  The caller
//     orders the keys once (a device sort of 8-byte keys: plumbing, as for runia_boot_keys_*).
//   * runia_sel_curve: the two-level tile scan of metrics.hip over the ordered table, tiles of 2048 rows, a thread owns kItems
//     consecutive rows.
//       pass 1 (one workgroup per tile): gathers the loss through the rows (f64, left in the workspace in sorted order so the
//         gather happens once) and takes the confidence back out of the key - the key is the f64 value, one to one, so the
//         confidences themselves are never read again - scans both inside the tile and leaves the tile's sums, its first and
//         last run end and the sums up to those;
//       pass 2 (one workgroup): prefix sums over the tile records in an order fixed by the number of tiles, and for every tile
//         the run end in front of it (s, L_s) and the first run end behind it (e, L_e) - the carries of a run that covers many
//         tiles, in both directions;
//       pass 3 (one workgroup per tile): the same scan again; every row k then knows s, L_s, e, L_e of its run from the tile's
//         own run ends or the carries, forms Lbar_k = L_s + (k - s)(L_e - L_s) / (e - s) (L_e itself at k = e) and adds
//         Lbar_k / k and Lbar_k; run ends are compacted into the curve.  No thread loops over a run: an all-tied table costs
//         what an all-distinct one costs;
//       pass 4 (one workgroup): the tile sums in a fixed order -> aurc, augrc.
//     The cumulative sum at sorted position i is ALWAYS formed as base[tile] + (start of the thread + the thread's running sum),
//     whichever pass or tile asks for it, so a carried L_s has the bits the owning tile gives it.  Every sum is f64 in an order
//     fixed by n alone, no floating-point atomics: the same inputs give the same bits.  Cumulative sums of integer-valued
//     losses (the 0/1 error) are exact, so L_s, L_e, s, e of a row depend on the multiset of (confidence, loss) pairs only and
//     EVERY output is bit-identical under any permutation of the input rows.
//   * runia_sel_query: from the compacted curve.  The run of a position (a coverage target, a bin boundary) is found by binary
//     search in run_end; the coverage at a risk is a maximum over ALL run ends (the curve is not monotone): integer atomicMax
//     on the run end, order-independent.
#include "common.hpp"

namespace {

constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelItems = 8;  // consecutive rows of a tile per thread
constexpr int kSelTile = kSelThreads * kSelItems;
constexpr int kNoEnd = 0x7fffffff;
constexpr int kMaxGrid = 64, kMaxBins = 512;

// ---- keys -----------------------------------------------------------------------------------------------------------------
// descending, as a signed number; -0.0 and +0.0 share a key
__host__ __device__ inline int64_t sel_key(double v) { return signed_view(desc_key(fold_zero(v))); }

// the confidence a key stands for, as f64 (-0.0 comes back as +0.0: the same term of a sum)
__device__ __forceinline__ double sel_conf_of_key(int64_t key) { return desc_value(unsigned_view(key)); }

template <typename T>
__global__ __launch_bounds__(256) void sel_keys_kernel(const T* __restrict__ conf, int64_t n, int64_t* __restrict__ keys,
                                                       unsigned* __restrict__ bad) {
  bool nan = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double v = (double)conf[i];
    nan = nan || v != v;
    keys[i] = sel_key(v);
  }
  if (__syncthreads_or(nan) && threadIdx.x == 0) *bad = 1u;  // (cleared in front of the launch; every writer writes 1)
}

template <typename T>
int sel_keys(const T* conf, int64_t n, int64_t* keys, unsigned* bad, runia_stream_t stream) {
  if (n < 1 || n >= (1ll << 31)) return RUNIA_E_INVALID;
  if (!conf || !keys || !bad) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(bad, 0, sizeof(unsigned), s) != hipSuccess) return RUNIA_E_LAUNCH;
  sel_keys_kernel<T><<<runia_stream_grid(n, 256), 256, 0, s>>>(conf, n, keys, bad);
  return runia_check_launch();
}

// ---- the tile scan --------------------------------------------------------------------------------------------------------
struct TileSum {    // pass 1 -> pass 2; sums are relative to the start of the tile
  double tot_l, tot_s;      // of the whole tile (= the sums at its last row)
  double first_l, first_s;  // at the tile's first run end
  double last_l, last_s;    // at its last run end
  int first, last;          // their places inside the tile; kNoEnd / -1: the tile holds no run end
  int cnt, pad;             // run ends in the tile
};
struct TileCarry {  // pass 2 -> pass 3
  double base_l, base_s;  // cumulative sums in front of the tile
  double prev_l, next_l;  // cumulative loss at the last run end in front of the tile / the first run end behind it
  int prev_pos, next_pos; // their 1-based sorted positions (0: no run end in front; the last row always ends a run)
  int base_pts, pad;      // run ends in front of the tile
};
static_assert(sizeof(TileSum) == 64 && sizeof(TileCarry) == 48, "workspace layout");

struct SelShared {
  double wl[kSelWaves], ws[kSelWaves];
  int wcnt[kSelWaves], wlast[kSelWaves], wfirst[kSelWaves];
};

struct Scan {
  double start_l, start_s;  // sums of the tile's rows in front of the thread's first row
  int cnt0;                 // run ends in front of it
  int p, q;                 // last run end in front of the thread's rows / first run end behind them (-1 / kNoEnd: none)
  int tile_first, tile_last, tile_cnt;
};

// One scan of the workgroup over per-thread (loss sum, confidence sum, run ends, last / first run end); called once per kernel.
// The order of the additions depends on nothing but the thread's place.
__device__ __forceinline__ void sel_block_scan(double al, double as, int cnt, int last, int first, SelShared& sh, Scan& o) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double xl = al, xs = as;
  int xc = cnt, xm = last, xf = first;
#pragma unroll  // (hand-written: a forward scan of four fields paired with the backward scan of xf)
  for (int d = 1; d < 64; d <<= 1) {
    const double yl = lane_up(xl, d), ys = lane_up(xs, d);
    const int yc = lane_up(xc, d), ym = lane_up(xm, d), yf = lane_down(xf, d);
    if (lane >= d) { xl = yl + xl; xs = ys + xs; xc += yc; xm = max(xm, ym); }
    if (lane + d < 64) xf = min(xf, yf);
  }
  if (lane == 63) { sh.wl[wave] = xl; sh.ws[wave] = xs; sh.wcnt[wave] = xc; sh.wlast[wave] = xm; }
  if (lane == 0) sh.wfirst[wave] = xf;
  // exclusive values of the lane
  double el = lane_up(xl, 1), es = lane_up(xs, 1);
  int ec = lane_up(xc, 1), em = lane_up(xm, 1), ef = lane_down(xf, 1);
  if (lane == 0) { el = 0.0; es = 0.0; ec = 0; em = -1; }
  if (lane == 63) ef = kNoEnd;
  __syncthreads();
  double offl = 0.0, offs = 0.0;
  int offc = 0, before = -1, after = kNoEnd, tfirst = kNoEnd, tlast = -1, tcnt = 0;
#pragma unroll
  for (int w = 0; w < kSelWaves; ++w) {
    if (w < wave) { offl += sh.wl[w]; offs += sh.ws[w]; offc += sh.wcnt[w]; before = max(before, sh.wlast[w]); }
    if (w > wave) after = min(after, sh.wfirst[w]);
    tfirst = min(tfirst, sh.wfirst[w]);
    tlast = max(tlast, sh.wlast[w]);
    tcnt += sh.wcnt[w];
  }
  o.start_l = offl + el;
  o.start_s = offs + es;
  o.cnt0 = offc + ec;
  o.p = max(before, em);
  o.q = min(after, ef);
  o.tile_first = tfirst; o.tile_last = tlast; o.tile_cnt = tcnt;
}

// The thread's rows of a tile: run-end flags and the confidences from the keys, the running sums, and the scan.  rl[c] / rs[c]:
// the sums of the tile's rows up to and including row c of the thread.
struct Rows {
  double rl[kSelItems], rs[kSelItems];
  unsigned ends;  // bit c: row c ends a run
  Scan sc;
};

__device__ __forceinline__ void sel_rows(const int64_t* __restrict__ keys, int64_t n, int64_t i0, const double* vl, SelShared& sh,
                                         Rows& r) {
  const int tid = threadIdx.x;
  int64_t k[kSelItems + 1];
  if (i0 + kSelItems < n) {  // every tile but the last: loads without a guard, which the compiler can widen
#pragma unroll
    for (int c = 0; c <= kSelItems; ++c) k[c] = keys[i0 + c];
  } else {
#pragma unroll
    for (int c = 0; c <= kSelItems; ++c) k[c] = (i0 + c < n) ? keys[i0 + c] : 0;
  }
  double al = 0.0, as = 0.0;
  int cnt = 0, last = -1, first = kNoEnd;
  r.ends = 0u;
#pragma unroll
  for (int c = 0; c < kSelItems; ++c) {
    const int64_t i = i0 + c;
    const bool end = i < n && (i == n - 1 || k[c] != k[c + 1]);
    al = (c == 0) ? vl[0] : al + vl[c];
    const double vs = i < n ? sel_conf_of_key(k[c]) : 0.0;
    as = (c == 0) ? vs : as + vs;
    r.rl[c] = al;
    r.rs[c] = as;
    if (end) {
      r.ends |= 1u << c;
      ++cnt;
      last = tid * kSelItems + c;
      if (first == kNoEnd) first = tid * kSelItems + c;
    }
  }
  sel_block_scan(al, as, cnt, last, first, sh, r.sc);
#pragma unroll
  for (int c = 0; c < kSelItems; ++c) {
    r.rl[c] = r.sc.start_l + r.rl[c];
    r.rs[c] = r.sc.start_s + r.rs[c];
  }
}

__device__ __forceinline__ double sel_load(const void* p, int is_f64, int64_t i) {
  return is_f64 ? reinterpret_cast<const double*>(p)[i] : (double)reinterpret_cast<const float*>(p)[i];
}

// pass 1
__global__ __launch_bounds__(kSelThreads) void sel_summary_kernel(const int64_t* __restrict__ keys, const int32_t* __restrict__ rows,
                                                                  const void* __restrict__ loss, int loss_f64, int64_t n,
                                                                  double* __restrict__ gl, TileSum* __restrict__ sums) {
  __shared__ SelShared sh;
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kSelTile, i0 = t0 + (int64_t)tid * kSelItems;
  double vl[kSelItems];
  int32_t row[kSelItems];
  const bool whole = i0 + kSelItems <= n;
  if (whole) {
#pragma unroll
    for (int c = 0; c < kSelItems; ++c) row[c] = rows[i0 + c];
  } else {
#pragma unroll
    for (int c = 0; c < kSelItems; ++c) row[c] = (i0 + c < n) ? rows[i0 + c] : 0;
  }
#pragma unroll
  for (int c = 0; c < kSelItems; ++c) {
    const int32_t r = row[c] < 0 ? 0 : (row[c] >= (int32_t)n ? (int32_t)n - 1 : row[c]);  // (a bad row id must not become a bad address)
    vl[c] = (i0 + c < n) ? sel_load(loss, loss_f64, r) : 0.0;
  }
  if (whole) {
#pragma unroll
    for (int c = 0; c < kSelItems; ++c) gl[i0 + c] = vl[c];
  } else {
#pragma unroll
    for (int c = 0; c < kSelItems; ++c)
      if (i0 + c < n) gl[i0 + c] = vl[c];
  }
  Rows r;
  sel_rows(keys, n, i0, vl, sh, r);
  TileSum* out = sums + blockIdx.x;
  const int64_t tile_rows = (n - t0 < kSelTile) ? n - t0 : kSelTile;  // >= 1
#pragma unroll
  for (int c = 0; c < kSelItems; ++c) {
    const int at = tid * kSelItems + c;
    if (at == r.sc.tile_first) { out->first_l = r.rl[c]; out->first_s = r.rs[c]; }
    if (at == r.sc.tile_last) { out->last_l = r.rl[c]; out->last_s = r.rs[c]; }
    if (at == (int)tile_rows - 1) { out->tot_l = r.rl[c]; out->tot_s = r.rs[c]; }
  }
  if (tid == 0) {
    out->first = r.sc.tile_first;
    out->last = r.sc.tile_last;
    out->cnt = r.sc.tile_cnt;
    out->pad = 0;
    if (r.sc.tile_cnt == 0) { out->first_l = 0.0; out->first_s = 0.0; out->last_l = 0.0; out->last_s = 0.0; }
  }
}

// pass 2: thread t takes the tiles [t * per, (t + 1) * per); the threads' sums are then added in thread order
__global__ __launch_bounds__(kSelThreads) void sel_tiles_kernel(const TileSum* __restrict__ sums, TileCarry* __restrict__ carry,
                                                                int64_t ntiles, int64_t n, double* __restrict__ record,
                                                                int64_t* __restrict__ n_points) {
  __shared__ double sl[kSelThreads], ss[kSelThreads];
  __shared__ int64_t sc[kSelThreads], slast[kSelThreads], sfirst[kSelThreads];
  const int tid = threadIdx.x;
  const int64_t per = (ntiles + kSelThreads - 1) / kSelThreads;
  const int64_t a = (int64_t)tid * per < ntiles ? (int64_t)tid * per : ntiles, b = a + per < ntiles ? a + per : ntiles;
  {
    double l = 0.0, s = 0.0;
    int64_t c = 0, last = -1, first = ntiles;
    for (int64_t t = a; t < b; ++t) {
      l += sums[t].tot_l;
      s += sums[t].tot_s;
      c += sums[t].cnt;
      if (sums[t].cnt > 0) {
        last = t;
        if (first == ntiles) first = t;
      }
    }
    sl[tid] = l; ss[tid] = s; sc[tid] = c; slast[tid] = last; sfirst[tid] = first;
  }
  __syncthreads();
  double l = 0.0, s = 0.0;
  int64_t c = 0, prev = -1, next = ntiles;
  for (int u = 0; u < tid; ++u) {
    l += sl[u]; s += ss[u]; c += sc[u];
    prev = slast[u] > prev ? slast[u] : prev;
  }
  for (int u = kSelThreads - 1; u > tid; --u) next = sfirst[u] < next ? sfirst[u] : next;
  for (int64_t t = a; t < b; ++t) {
    carry[t].base_l = l;
    carry[t].base_s = s;
    carry[t].base_pts = (int)c;
    carry[t].pad = 0;
    l += sums[t].tot_l;
    s += sums[t].tot_s;
    c += sums[t].cnt;
  }
  if (b == ntiles && a < b) {  // the thread of the last tile
    record[0] = (double)c;
    record[1] = l;
    record[2] = s;
    if (n_points) *n_points = c;
  }
  __syncthreads();  // every base is written
  for (int64_t t = a; t < b; ++t) {
    carry[t].prev_pos = prev >= 0 ? (int)(prev * kSelTile + sums[prev].last + 1) : 0;
    carry[t].prev_l = prev >= 0 ? carry[prev].base_l + sums[prev].last_l : 0.0;
    if (sums[t].cnt > 0) prev = t;
  }
  for (int64_t t = b - 1; t >= a; --t) {
    // (the table's last row ends a run, so only the last tile has nothing behind it, and there nothing asks)
    carry[t].next_pos = next < ntiles ? (int)(next * kSelTile + sums[next].first + 1) : (int)n;
    carry[t].next_l = next < ntiles ? carry[next].base_l + sums[next].first_l : 0.0;
    if (sums[t].cnt > 0) next = t;
  }
}

// pass 3
__device__ __forceinline__ int sel_lds(int at) { return at + at / kSelItems; }  // threads 72 bytes apart: no bank shared by a half wave
__global__ __launch_bounds__(kSelThreads) void sel_final_kernel(const int64_t* __restrict__ keys, const double* __restrict__ gl,
                                                                int64_t n,
                                                                const TileCarry* __restrict__ carry, int32_t* __restrict__ run_end,
                                                                double* __restrict__ cum_loss, double* __restrict__ cum_conf,
                                                                double* __restrict__ partial) {
  __shared__ SelShared sh;
  __shared__ double lsh[kSelTile + kSelTile / kSelItems];  // cumulative loss at every row of the tile (a thread's rows + 1 pad)
  __shared__ double wa[kSelWaves], wg[kSelWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * kSelTile, i0 = t0 + (int64_t)tid * kSelItems;
  const TileCarry cy = carry[blockIdx.x];
  double vl[kSelItems];
  if (i0 + kSelItems <= n) {
#pragma unroll
    for (int c = 0; c < kSelItems; ++c) vl[c] = gl[i0 + c];
  } else {
#pragma unroll
    for (int c = 0; c < kSelItems; ++c) vl[c] = (i0 + c < n) ? gl[i0 + c] : 0.0;
  }
  Rows r;
  sel_rows(keys, n, i0, vl, sh, r);
#pragma unroll
  for (int c = 0; c < kSelItems; ++c) {
    r.rl[c] = cy.base_l + r.rl[c];
    lsh[sel_lds(tid * kSelItems + c)] = r.rl[c];
  }
  __syncthreads();
  // the first run end at or behind every row of the thread
  int q[kSelItems];
  {
    int cur = r.sc.q;
#pragma unroll
    for (int c = kSelItems - 1; c >= 0; --c) {
      if ((r.ends >> c) & 1u) cur = tid * kSelItems + c;
      q[c] = cur;
    }
  }
  int p = r.sc.p, pt = cy.base_pts + r.sc.cnt0;
  double sum_a = 0.0, sum_g = 0.0;
#pragma unroll
  for (int c = 0; c < kSelItems; ++c) {
    const int64_t i = i0 + c;
    if (i < n) {
      const double k = (double)(i + 1);
      const double s = p >= 0 ? (double)(t0 + p + 1) : (double)cy.prev_pos;
      const double ls = p >= 0 ? lsh[sel_lds(p)] : cy.prev_l;
      const double e = q[c] != kNoEnd ? (double)(t0 + q[c] + 1) : (double)cy.next_pos;
      const double le = q[c] != kNoEnd ? lsh[sel_lds(q[c])] : cy.next_l;
      const bool end = (r.ends >> c) & 1u;
      const double lbar = end ? r.rl[c] : ls + ((k - s) * (le - ls)) / (e - s);
      sum_a += lbar / k;
      sum_g += lbar;
      if (end) {
        if (run_end) {
          run_end[pt] = (int32_t)(i + 1);
          cum_loss[pt] = r.rl[c];
          cum_conf[pt] = cy.base_s + r.rs[c];
        }
        ++pt;
        p = tid * kSelItems + c;
      }
    }
  }
  sum_a = wave_sum(sum_a);
  sum_g = wave_sum(sum_g);
  if (lane == 0) { wa[wave] = sum_a; wg[wave] = sum_g; }
  __syncthreads();
  if (tid == 0) {
    double x = wa[0], y = wg[0];
    for (int w = 1; w < kSelWaves; ++w) { x += wa[w]; y += wg[w]; }  // (the waves in order)
    partial[2 * (int64_t)blockIdx.x] = x;
    partial[2 * (int64_t)blockIdx.x + 1] = y;
  }
}

// pass 4
__global__ __launch_bounds__(kSelThreads) void sel_finish_kernel(const double* __restrict__ partial, int64_t ntiles, int64_t n,
                                                                 double* __restrict__ record) {
  __shared__ double sa[kSelThreads], sg[kSelThreads];
  const int tid = threadIdx.x;
  const int64_t per = (ntiles + kSelThreads - 1) / kSelThreads;
  const int64_t a = (int64_t)tid * per < ntiles ? (int64_t)tid * per : ntiles, b = a + per < ntiles ? a + per : ntiles;
  double x = 0.0, y = 0.0;
  for (int64_t t = a; t < b; ++t) { x += partial[2 * t]; y += partial[2 * t + 1]; }
  sa[tid] = x; sg[tid] = y;
  __syncthreads();
  if (tid == 0) {
    x = sa[0]; y = sg[0];
    for (int u = 1; u < kSelThreads; ++u) { x += sa[u]; y += sg[u]; }
    record[3] = x / (double)n;
    record[4] = y / ((double)n * (double)n);
  }
}

int64_t sel_tiles(int64_t n) { return (n + kSelTile - 1) / kSelTile; }
constexpr size_t kBestBytes = 256;  // slot of runia_sel_query's 64 run ends

// ---- queries --------------------------------------------------------------------------------------------------------------
constexpr int kQItems = 8;

__global__ __launch_bounds__(256) void sel_best_kernel(const int32_t* __restrict__ run_end, const double* __restrict__ cum_loss,
                                                       const int64_t* __restrict__ n_points, int64_t n,
                                                       const double* __restrict__ risks, int R, int* __restrict__ best) {
  __shared__ int sbest[kMaxGrid];
  const int tid = threadIdx.x, lane = tid & 63;
  int64_t m = *n_points;
  m = m < 0 ? 0 : (m > n ? n : m);  // (the arrays hold n entries at most)
  if (tid < kMaxGrid) sbest[tid] = 0;
  __syncthreads();
  // (whole workgroups enter a trip: the wave reduction below needs every lane)
  for (int64_t g0 = (int64_t)blockIdx.x * 256 * kQItems; g0 < m; g0 += (int64_t)gridDim.x * 256 * kQItems) {
    const int64_t c0 = g0 + (int64_t)tid * kQItems;
    double e[kQItems], l[kQItems];
#pragma unroll
    for (int c = 0; c < kQItems; ++c) {
      const bool in = c0 + c < m;
      e[c] = in ? (double)run_end[c0 + c] : 0.0;
      l[c] = in ? cum_loss[c0 + c] : 1.0;  // (1 <= r * 0 is false for every finite r; a NaN r compares false as well)
    }
    for (int j = 0; j < R; ++j) {
      const double rj = risks[j];
      int b = 0;
#pragma unroll
      for (int c = 0; c < kQItems; ++c)
        if (e[c] > 0.0 && l[c] <= rj * e[c]) b = (int)e[c];  // (run ends ascend with c)
      b = wave_max(b);
      if (lane == 0 && b > 0) atomicMax(&sbest[j], b);
    }
  }
  __syncthreads();
  if (tid < R && sbest[tid] > 0) atomicMax(&best[tid], sbest[tid]);
}

// the first curve point whose run end is >= k (1 <= k <= n: the last run end is n)
__device__ __forceinline__ int64_t sel_point_of(const int32_t* __restrict__ run_end, int64_t m, int64_t k) {
  int64_t lo = 0, hi = m - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)run_end[mid] >= k) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sel_query_kernel(const int32_t* __restrict__ run_end, const double* __restrict__ cum_loss,
                                                        const double* __restrict__ cum_conf, const int64_t* __restrict__ n_points,
                                                        int64_t n, const int64_t* __restrict__ targets, int Q, int R, int n_bins,
                                                        const int* __restrict__ best, double* __restrict__ risk_at,
                                                        double* __restrict__ cov_at, double* __restrict__ cov_at_risk,
                                                        double* __restrict__ bins) {
  __shared__ double bl[kMaxBins + 1], bs[kMaxBins + 1];
  const int tid = threadIdx.x;
  int64_t m = *n_points;
  m = m < 1 ? 1 : (m > n ? n : m);
  if (tid < Q) {
    int64_t k = targets[tid];
    k = k < 1 ? 1 : (k > n ? n : k);
    const int64_t at = sel_point_of(run_end, m, k);
    const double e = (double)run_end[at];
    risk_at[tid] = cum_loss[at] / e;
    cov_at[tid] = e / (double)n;
  }
  if (tid < R) cov_at_risk[tid] = (double)best[tid] / (double)n;
  if (n_bins < 1) return;
  // Lbar and Sbar at the boundaries: ascending position floor(b n / B) is sorted position k = n - floor(b n / B)
  for (int b = tid; b <= n_bins; b += 256) {
    const int64_t k = n - ((int64_t)b * n) / n_bins;
    double l = 0.0, s = 0.0;
    if (k >= 1) {
      const int64_t at = sel_point_of(run_end, m, k);
      const double e = (double)run_end[at], st = at > 0 ? (double)run_end[at - 1] : 0.0;
      const double le = cum_loss[at], ls = at > 0 ? cum_loss[at - 1] : 0.0;
      const double se = cum_conf[at], ss = at > 0 ? cum_conf[at - 1] : 0.0;
      const bool end = (int64_t)run_end[at] == k;
      l = end ? le : ls + (((double)k - st) * (le - ls)) / (e - st);
      s = end ? se : ss + (((double)k - st) * (se - ss)) / (e - st);
    }
    bl[b] = l;
    bs[b] = s;
  }
  __syncthreads();
  for (int b = tid; b < n_bins; b += 256) {
    const int64_t j0 = ((int64_t)b * n) / n_bins, j1 = ((int64_t)(b + 1) * n) / n_bins;
    bins[3 * b] = (double)(j1 - j0);
    bins[3 * b + 1] = j1 > j0 ? bl[b] - bl[b + 1] : 0.0;
    bins[3 * b + 2] = j1 > j0 ? bs[b] - bs[b + 1] : 0.0;
  }
}

}  // namespace

extern "C" int runia_sel_tile_rows(void) { return kSelTile; }

extern "C" int runia_sel_keys_f32(const float* conf, int64_t n, int64_t* keys, unsigned* bad, runia_stream_t stream) {
  return sel_keys<float>(conf, n, keys, bad, stream);
}

extern "C" int runia_sel_keys_f64(const double* conf, int64_t n, int64_t* keys, unsigned* bad, runia_stream_t stream) {
  return sel_keys<double>(conf, n, keys, bad, stream);
}

extern "C" int64_t runia_sel_key_of_f64_host(double conf) { return sel_key(conf); }

struct SelPlan {
  int* best;  // runia_sel_query's 64 run ends, at the front of the workspace
  double* gl;
  TileSum* sums;
  TileCarry* carry;
  double* partial;
};
static SelPlan sel_plan(WsWalk& w, int64_t n) {
  const size_t t = (size_t)sel_tiles(n);
  SelPlan p;
  p.best = w.take<int>(64, kBestBytes);
  p.gl = w.take<double>(n);
  p.sums = w.take<TileSum>(t);
  p.carry = w.take<TileCarry>(t);
  p.partial = w.take<double>(2 * t);
  return p;
}

extern "C" size_t runia_sel_workspace_bytes(int64_t n) {
  if (n < 1 || n >= (1ll << 31)) return 0;
  return ws_bytes([&](WsWalk& w) { sel_plan(w, n); });
}

extern "C" int runia_sel_curve(const int64_t* sorted_keys, const int32_t* sorted_rows, const void* loss, int loss_f64, int64_t n,
                               double* record, int32_t* run_end, double* cum_loss, double* cum_conf, int64_t* n_points,
                               void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (n < 1 || n >= (1ll << 31)) return RUNIA_E_INVALID;
  if (!sorted_keys || !sorted_rows || !loss || !record) return RUNIA_E_INVALID;
  if ((run_end != nullptr) != (cum_loss != nullptr) || (run_end != nullptr) != (cum_conf != nullptr)) return RUNIA_E_INVALID;
  if (run_end && !n_points) return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const SelPlan plan = sel_plan(w, n);
  if (ws_refused(workspace, workspace_bytes, w.used(), 8)) return RUNIA_E_WORKSPACE;
  const int64_t ntiles = sel_tiles(n);
  double *gl = plan.gl, *partial = plan.partial;
  TileSum* sums = plan.sums;
  TileCarry* carry = plan.carry;
  hipStream_t s = as_stream(stream);
  sel_summary_kernel<<<(unsigned)ntiles, kSelThreads, 0, s>>>(sorted_keys, sorted_rows, loss, loss_f64, n, gl, sums);
  sel_tiles_kernel<<<1, kSelThreads, 0, s>>>(sums, carry, ntiles, n, record, n_points);
  sel_final_kernel<<<(unsigned)ntiles, kSelThreads, 0, s>>>(sorted_keys, gl, n, carry, run_end, cum_loss, cum_conf, partial);
  sel_finish_kernel<<<1, kSelThreads, 0, s>>>(partial, ntiles, n, record);
  return runia_check_launch();
}

extern "C" int runia_sel_query(const int32_t* run_end, const double* cum_loss, const double* cum_conf, const int64_t* n_points,
                               int64_t n, const int64_t* targets, int n_targets, const double* risks, int n_risks, int n_bins,
                               double* risk_at, double* coverage_at, double* coverage_at_risk, double* bins, void* workspace,
                               size_t workspace_bytes, runia_stream_t stream) {
  if (n < 1 || n >= (1ll << 31)) return RUNIA_E_INVALID;
  if (n_targets < 0 || n_targets > kMaxGrid || n_risks < 0 || n_risks > kMaxGrid) return RUNIA_E_INVALID;
  if (n_bins < 0 || n_bins > kMaxBins) return RUNIA_E_INVALID;
  if (!run_end || !cum_loss || !cum_conf || !n_points) return RUNIA_E_INVALID;
  if ((n_targets && (!targets || !risk_at || !coverage_at)) || (n_risks && (!risks || !coverage_at_risk)) || (n_bins && !bins))
    return RUNIA_E_INVALID;
  if (ws_refused(workspace, workspace_bytes, kBestBytes, 8)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  int* best = reinterpret_cast<int*>(workspace);
  if (n_risks) {
    if (hipMemsetAsync(best, 0, kBestBytes, s) != hipSuccess) return RUNIA_E_LAUNCH;
    int64_t grid = (n + 256 * kQItems - 1) / (256 * kQItems);
    grid = grid > 1024 ? 1024 : grid;
    sel_best_kernel<<<(unsigned)grid, 256, 0, s>>>(run_end, cum_loss, n_points, n, risks, n_risks, best);
  }
  sel_query_kernel<<<1, 256, 0, s>>>(run_end, cum_loss, cum_conf, n_points, n, targets, n_targets, n_risks, n_bins, best, risk_at,
                                     coverage_at, coverage_at_risk, bins);
  return runia_check_launch();
}
