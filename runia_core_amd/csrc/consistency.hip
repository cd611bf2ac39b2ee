// Sample-consistency scores of LLM generations from the sampled token ids alone (black box): pairwise ROUGE-L / Jaccard
// counts (Fomicheva et al. 2020) and the graph scores NumSet / Deg / Ecc / EigV over a pairwise similarity (Lin, Trivedi
// and Sun 2023).  Rows are prompt-major: group g = rows g*k .. g*k+k-1 of the ids of generate(num_return_sequences=k),
// read where they lie (int32 or int64, any row and column stride).  The content of a row is its ids up to the first eos
// id (excluded) and up to lengths[row]; n_i = its length (0 allowed).
//
// runia_cons_pairs - integer tables, no atomics, every entry a function of its own two rows:
//   len      one wave per row: 64 columns per trip, the first eos by ballot.  Writes len and the diagonal lcs[i, i] = n_i.
//   lcs      one wave per unordered pair.  The LONGER content lies across the lanes, C consecutive columns per lane in
//            registers (C = the power of two with 64 C >= T, chosen per launch), the DP row in C more registers; the
//            shorter one is walked serially: 64 ids per trip sit one per lane and come out wave-uniform by v_readlane.
//            Per step cand_j = (b_j == a_i) ? prev_{j-1} + 1 : prev_j, row = inclusive prefix-max(cand) - valid because DP
//            rows are non-decreasing: a serial pass over the lane's own columns, one wave_scan_incl (max) of the lane
//            totals, one pass to fold the lanes before.  Columns past the content are never read back: a prefix only
//            flows to the right.  int64 ids are compared on all 64 bits.
//   sort     one workgroup per row: the content as int64 in LDS (32 KB), padded to a power of two with INT64_MAX (an id
//            of that value ties with the padding; only the first n sorted slots are read) and sorted by the LDS sort of
//            order.hpp; duplicates are dropped by a block scan of the
//            "differs from its left neighbour" flags.  The distinct ids go to the workspace in ascending order; writes
//            uniq and the diagonal inter[i, i].
//   inter    one wave per unordered pair: the lanes take the distinct ids of the smaller set and search the larger one
//            (binary search in the workspace rows), counts summed by wave_sum.
//
// runia_cons_graph - one workgroup of 256 threads per group, W [k, k] f64 (upper triangle read, diagonal taken as 1):
//   degrees, adjacency masks (64-bit, closed by six squaring steps: paths of up to 64 edges), the normalised Laplacian
//   L = I - D^-1/2 W D^-1/2 in LDS, then the cyclic Jacobi in LDS of jacobi.hpp (jacobi_lds_sweeps: eigenvalue form of the
//   threshold; NaN after 30 sweeps) with the rotations also applied to V (eigenvectors in its columns).  Ecc is
//   formed as the norm of the centred rows of the selected eigenvectors - equal to the projector form P_ii - 2 (P 1)_i / k +
//   1'P1 / k^2 but without its cancellation (an s_i^2 of 0 would otherwise come out as 1e-17 and its root as 3e-9).
//   LDS: two 32 KB matrices + 8 KB of vectors (dynamic, above the 64 KB static limit).  Every sum runs in index order.
#include <math.h>

#include "common.hpp"
#include "jacobi.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = RUNIA_CONS_MAX_K;
constexpr int kMaxT = RUNIA_CONS_MAX_T;
static_assert((kMaxT & (kMaxT - 1)) == 0, "cons_sort_kernel pads a row to a power of two inside kMaxT slots");
constexpr int kMaxSweeps = 30;

// lane s of the wave (s wave-uniform) as a scalar
__device__ __forceinline__ int32_t lane_value(int32_t v, int s) { return __builtin_amdgcn_readlane(v, s); }
__device__ __forceinline__ int64_t lane_value(int64_t v, int s) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, s);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), s);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// unordered pair number rem (0 <= rem < k (k - 1) / 2, row-major over i < j) -> (i, j)
__device__ __forceinline__ void pair_of(int k, int rem, int& i, int& j) {
  i = 0;
  while (rem >= k - 1 - i) { rem -= k - 1 - i; ++i; }
  j = i + 1 + rem;
}

// ---- content lengths ----------------------------------------------------------------------------------------------------
template <class Id>
__global__ __launch_bounds__(kThreads) void cons_len_kernel(const Id* __restrict__ ids, int64_t rows, int k, int T,
                                                            int64_t rs, int64_t cs, const int64_t* __restrict__ eos,
                                                            int n_eos, const int64_t* __restrict__ lengths,
                                                            int32_t* __restrict__ len, int32_t* __restrict__ lcs) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= rows) return;
  int n = T;
  if (lengths) {
    const int64_t v = lengths[row];
    n = v < 0 ? 0 : (v < (int64_t)T ? (int)v : T);
  }
  const Id* r = ids + row * rs;
  int cut = n;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int c = c0 + lane;
    bool hit = false;
    if (c < n) {
      const int64_t v = (int64_t)r[(int64_t)c * cs];
      for (int e = 0; e < n_eos; ++e) hit |= (v == eos[e]);
    }
    const unsigned long long m = __ballot(hit);
    if (m) {
      cut = c0 + __ffsll(m) - 1;
      break;
    }
  }
  if (lane == 0) {
    len[row] = cut;
    if (lcs) {
      const int64_t g = row / k;
      const int i = (int)(row - g * k);
      lcs[(g * k + i) * k + i] = cut;
    }
  }
}

// ---- longest common subsequence of every pair ---------------------------------------------------------------------------
template <class Id, int C>
__global__ __launch_bounds__(kThreads) void cons_lcs_kernel(const Id* __restrict__ ids, int64_t groups, int k, int64_t rs,
                                                            int64_t cs, const int32_t* __restrict__ len,
                                                            int32_t* __restrict__ lcs) {
  const int lane = threadIdx.x & 63;
  const int P = k * (k - 1) / 2;
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w >= groups * P) return;
  const int64_t g = w / P;
  int i, j;
  pair_of(k, (int)(w - g * P), i, j);
  const int64_t ra = g * k + i, rb = g * k + j;
  int na = len[ra], nb = len[rb];
  const Id* a = ids + ra * rs;
  const Id* b = ids + rb * rs;
  if (na > nb) {  // b: the longer content, across the lanes
    const Id* p = a; a = b; b = p;
    const int n = na; na = nb; nb = n;
  }
  int res = 0;
  if (na > 0) {
    Id bv[C];
    int row[C];
#pragma unroll
    for (int t = 0; t < C; ++t) {
      const int col = lane * C + t;
      bv[t] = col < nb ? b[(int64_t)col * cs] : Id(0);
      row[t] = 0;
    }
    for (int c0 = 0; c0 < na; c0 += 64) {
      const int c = c0 + lane;
      const Id av = c < na ? a[(int64_t)c * cs] : Id(0);
      const int steps = na - c0 < 64 ? na - c0 : 64;
      for (int s = 0; s < steps; ++s) {
        const Id ai = lane_value(av, s);
        int left = lane_up(row[C - 1], 1);  // the previous row at column lane * C - 1
        if (lane == 0) left = 0;
        int run = 0;
#pragma unroll
        for (int t = 0; t < C; ++t) {
          const int up = row[t];
          const int cand = (bv[t] == ai) ? left + 1 : up;
          left = up;
          run = cand > run ? cand : run;
          row[t] = run;
        }
        const int inc = wave_scan_incl(run, [](int x, int y) { return x > y ? x : y; });
        int before = lane_up(inc, 1);
        if (lane == 0) before = 0;
#pragma unroll
        for (int t = 0; t < C; ++t) row[t] = row[t] > before ? row[t] : before;
      }
    }
    const int last = nb - 1;  // the row's value at the content's last column
    int v = 0;
#pragma unroll
    for (int t = 0; t < C; ++t) v = (t == last % C) ? row[t] : v;
    res = __shfl(v, last / C, 64);
  }
  if (lane == 0) {
    lcs[(g * k + i) * k + j] = res;
    lcs[(g * k + j) * k + i] = res;
  }
}

// ---- distinct ids of every row, ascending -------------------------------------------------------------------------------
template <class Id>
__global__ __launch_bounds__(kThreads) void cons_sort_kernel(const Id* __restrict__ ids, int k, int T, int64_t rs,
                                                             int64_t cs, const int32_t* __restrict__ len,
                                                             int64_t* __restrict__ sorted, int32_t* __restrict__ uniq,
                                                             int32_t* __restrict__ inter) {
  __shared__ int64_t a[kMaxT];
  __shared__ int wave_totals[kWaves];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int n = len[row];
  const Id* r = ids + row * rs;
  int N = 1;
  while (N < n) N <<= 1;  // <= kMaxT, a power of two
  for (int c = tid; c < N; c += kThreads) a[c] = c < n ? (int64_t)r[(int64_t)c * cs] : INT64_MAX;  // the padding sorts last
  __syncthreads();
  lds_bitonic_sort(a, N, tid, kThreads);
  const int per = (n + kThreads - 1) / kThreads;
  const int first = tid * per < n ? tid * per : n;
  const int end = first + per < n ? first + per : n;
  int count = 0;
  for (int x = first; x < end; ++x) count += (x == 0 || a[x] != a[x - 1]) ? 1 : 0;
  int total;
  int pos = block_scan_excl<kThreads>(count, wave_totals, total);
  int64_t* out = sorted + row * T;
  for (int x = first; x < end; ++x)
    if (x == 0 || a[x] != a[x - 1]) out[pos++] = a[x];
  if (tid == 0) {
    uniq[row] = total;
    const int64_t g = row / k;
    const int i = (int)(row - g * k);
    inter[(g * k + i) * k + i] = total;
  }
}

__global__ __launch_bounds__(kThreads) void cons_inter_kernel(const int64_t* __restrict__ sorted, int64_t groups, int k, int T,
                                                              const int32_t* __restrict__ uniq,
                                                              int32_t* __restrict__ inter) {
  const int lane = threadIdx.x & 63;
  const int P = k * (k - 1) / 2;
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w >= groups * P) return;
  const int64_t g = w / P;
  int i, j;
  pair_of(k, (int)(w - g * P), i, j);
  int64_t rs_ = g * k + i, rl = g * k + j;
  int ns = uniq[rs_], nl = uniq[rl];
  if (ns > nl) {
    const int64_t r = rs_; rs_ = rl; rl = r;
    const int n = ns; ns = nl; nl = n;
  }
  const int64_t* S = sorted + rs_ * T;
  const int64_t* L = sorted + rl * T;
  int cnt = 0;
  for (int x = lane; x < ns; x += 64) {
    const int64_t v = S[x];
    int lo = 0, hi = nl;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (L[mid] < v) lo = mid + 1; else hi = mid;
    }
    cnt += (lo < nl && L[lo] == v) ? 1 : 0;
  }
  cnt = wave_sum(cnt);
  if (lane == 0) {
    inter[(g * k + i) * k + j] = cnt;
    inter[(g * k + j) * k + i] = cnt;
  }
}

// ---- graph scores -------------------------------------------------------------------------------------------------------
constexpr int kMat = kMaxK * kMaxK;  // doubles per LDS matrix
constexpr int kVec = 1024;           // doubles of vectors behind the two matrices
constexpr int kGraphLdsBytes = (2 * kMat + kVec) * 8;

__global__ __launch_bounds__(kThreads) void cons_graph_kernel(const double* __restrict__ W, int k, double eigv_thr,
                                                              double set_thr, double* __restrict__ eigenvalues,
                                                              double* __restrict__ u_deg, double* __restrict__ u_eigv,
                                                              double* __restrict__ u_ecc, double* __restrict__ lexsim,
                                                              double* __restrict__ c_deg, double* __restrict__ c_ecc,
                                                              int32_t* __restrict__ num_sets) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* G = lds;         // [k, k] row-major: W, then the Laplacian, diagonalised in place
  double* V = lds + kMat;  // [k, k] row-major: eigenvectors in the columns
  double* x = lds + 2 * kMat;
  double* rot = x;           // [64]: cosines, sines of the step's rotations
  double* part = x + 64;     // [256]: Frobenius norm partials
  double* deg = x + 320;     // [64]
  double* dinv = x + 384;    // [64]
  double* lam = x + 448;     // [64]: eigenvalues in ascending order
  double* csum = x + 512;    // [64]: column sums of V
  double* ssq = x + 576;     // [64]: s_i^2
  double* upper = x + 640;   // [64]: sum of w_ij over j > i
  unsigned long long* adj = reinterpret_cast<unsigned long long*>(x + 704);  // [64]
  int* order = reinterpret_cast<int*>(x + 768);                              // [64]: column of V of the r-th eigenvalue
  int* flag = reinterpret_cast<int*>(x + 800);                               // rotated, NaN eigenvalue, non-finite input
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;
  const double* Wg = W + g * k * k;
  const double nan = __builtin_nan("");

  if (tid == 0) { flag[1] = 0; flag[2] = 0; }
  __syncthreads();
  for (int idx = tid; idx < k * k; idx += kThreads) {
    const int i = idx / k, j = idx - i * k;
    double w = 1.0;
    if (i != j) {
      w = Wg[(i < j ? i : j) * k + (i < j ? j : i)];
      if (!__builtin_isfinite(w)) flag[2] = 1;
    }
    G[idx] = w;
    V[idx] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  if (flag[2]) {  // a non-finite entry: the group has no scores
    if (tid < k) {
      eigenvalues[g * k + tid] = nan;
      c_deg[g * k + tid] = nan;
      c_ecc[g * k + tid] = nan;
    }
    if (tid == 0) {
      u_deg[g] = nan; u_eigv[g] = nan; u_ecc[g] = nan; lexsim[g] = nan;
      num_sets[g] = -1;
    }
    return;
  }

  // ---- degrees, adjacency ------------------------------------------------------------------------------------------------
  if (tid < k) {
    double d = 0.0, u = 0.0;
    unsigned long long m = 0;
    for (int j = 0; j < k; ++j) {
      const double w = G[tid * k + j];
      d += w;
      if (j > tid) u += w;
      if (j == tid || w >= set_thr) m |= 1ull << j;
    }
    deg[tid] = d;
    upper[tid] = u;
    dinv[tid] = 1.0 / sqrt(d);
    adj[tid] = m;
  }
  __syncthreads();
  for (int it = 0; it < 6; ++it) {  // reach doubles per step: 2^6 >= k - 1 edges
    unsigned long long m = 0;
    if (tid < k) {
      m = adj[tid];
      unsigned long long bits = m;
      while (bits) {
        const int j = __ffsll(bits) - 1;
        bits &= bits - 1;
        m |= adj[j];
      }
    }
    __syncthreads();
    if (tid < k) adj[tid] = m;
    __syncthreads();
  }

  // ---- normalised Laplacian ----------------------------------------------------------------------------------------------
  for (int idx = tid; idx < k * k; idx += kThreads) {
    const int i = idx / k, j = idx - i * k;
    G[idx] = (i == j ? 1.0 : 0.0) - G[idx] * (dinv[i] * dinv[j]);  // dinv_i dinv_j commutes: G stays exactly symmetric
  }
  __syncthreads();

  // ---- cyclic Jacobi on G, rotations accumulated in V -----------------------------------------------------------------------
  const bool converged = jacobi_lds_sweeps<kThreads, true>(G, V, k, kMaxSweeps, rot, part, flag);

  // ---- scores -------------------------------------------------------------------------------------------------------------
  if (tid < k) {
    const double v = G[tid * k + tid];
    if (isnan(v)) {
      flag[1] = 1;
    } else {
      int rank = 0;
      for (int j = 0; j < k; ++j) {
        const double u = G[j * k + j];
        rank += (u < v || (u == v && j < tid)) ? 1 : 0;
      }
      lam[rank] = v;
      order[rank] = tid;
    }
    double s = 0.0;
    for (int r = 0; r < k; ++r) s += V[r * k + tid];
    csum[tid] = s;
  }
  __syncthreads();
  const bool spectral = converged && !flag[1];
  if (tid < k) {
    double ss = 0.0;
    if (spectral) {
      for (int r = 0; r < k; ++r) {
        if (!(lam[r] < eigv_thr)) break;  // ascending: the selected eigenvalues come first
        const int c = order[r];
        const double d = V[tid * k + c] - csum[c] / (double)k;
        ss += d * d;
      }
    }
    ssq[tid] = ss;
    eigenvalues[g * k + tid] = spectral ? lam[tid] : nan;
    c_deg[g * k + tid] = deg[tid] / (double)k;
    c_ecc[g * k + tid] = spectral ? -sqrt(ss) : nan;
  }
  __syncthreads();
  if (tid == 0) {
    double dsum = 0.0, usum = 0.0, ev = 0.0, ecc = 0.0;
    int sets = 0;
    for (int i = 0; i < k; ++i) {
      dsum += deg[i];
      usum += upper[i];
      ecc += ssq[i];
      sets += (__ffsll(adj[i]) - 1 == i) ? 1 : 0;  // a component is counted at its lowest member
    }
    if (spectral)
      for (int r = 0; r < k; ++r) ev += fmax(0.0, 1.0 - lam[r]);
    u_deg[g] = 1.0 - dsum / ((double)k * (double)k);
    lexsim[g] = usum / (0.5 * (double)k * (double)(k - 1));
    u_eigv[g] = spectral ? ev : nan;
    u_ecc[g] = spectral ? sqrt(ecc) : nan;
    num_sets[g] = sets;
  }
}

bool pairs_shape_ok(int64_t groups, int64_t k, int64_t T) {
  return groups >= 1 && k >= 2 && k <= kMaxK && groups * k * k <= 0x7fffffffll && T >= 0 && T <= kMaxT;
}

void sorted_layout(WsWalk& w, int64_t rows, int64_t T, int64_t*& sorted) { sorted = w.take<int64_t>((size_t)(rows * T), 16); }

template <class Id, int C>
void launch_lcs(const void* ids, int64_t groups, int k, int64_t rs, int64_t cs, const int32_t* len, int32_t* lcs,
                hipStream_t s) {
  const int64_t waves = groups * (k * (k - 1) / 2);
  cons_lcs_kernel<Id, C><<<(unsigned)((waves + kWaves - 1) / kWaves), kThreads, 0, s>>>(static_cast<const Id*>(ids), groups, k,
                                                                                       rs, cs, len, lcs);
}

template <class Id>
void launch_pairs(const void* ids, int64_t groups, int k, int T, int64_t rs, int64_t cs, const int64_t* eos, int n_eos,
                  const int64_t* lengths, int what, int32_t* len, int32_t* lcs, int32_t* uniq, int32_t* inter,
                  int64_t* sorted, hipStream_t s) {
  const Id* p = static_cast<const Id*>(ids);
  const int64_t rows = groups * k;
  const bool want_lcs = what & RUNIA_CONS_LCS;
  cons_len_kernel<Id><<<(unsigned)((rows + kWaves - 1) / kWaves), kThreads, 0, s>>>(p, rows, k, T, rs, cs, eos, n_eos, lengths,
                                                                                   len, want_lcs ? lcs : nullptr);
  if (want_lcs) {
    int c = 1;
    while (c * 64 < T) c <<= 1;
    switch (c) {
      case 1: launch_lcs<Id, 1>(ids, groups, k, rs, cs, len, lcs, s); break;
      case 2: launch_lcs<Id, 2>(ids, groups, k, rs, cs, len, lcs, s); break;
      case 4: launch_lcs<Id, 4>(ids, groups, k, rs, cs, len, lcs, s); break;
      case 8: launch_lcs<Id, 8>(ids, groups, k, rs, cs, len, lcs, s); break;
      case 16: launch_lcs<Id, 16>(ids, groups, k, rs, cs, len, lcs, s); break;
      case 32: launch_lcs<Id, 32>(ids, groups, k, rs, cs, len, lcs, s); break;
      default: launch_lcs<Id, 64>(ids, groups, k, rs, cs, len, lcs, s); break;
    }
  }
  if (what & RUNIA_CONS_JACCARD) {
    cons_sort_kernel<Id><<<(unsigned)rows, kThreads, 0, s>>>(p, k, T, rs, cs, len, sorted, uniq, inter);
    const int64_t waves = groups * (k * (k - 1) / 2);
    cons_inter_kernel<<<(unsigned)((waves + kWaves - 1) / kWaves), kThreads, 0, s>>>(sorted, groups, k, T, uniq, inter);
  }
}

}  // namespace

extern "C" int64_t runia_cons_pairs_workspace_bytes(int64_t groups, int64_t k, int64_t T, int what) {
  if (!pairs_shape_ok(groups, k, T) || !(what & RUNIA_CONS_JACCARD)) return 0;
  return (int64_t)ws_bytes([&](WsWalk& w) { int64_t* sorted; sorted_layout(w, groups * k, T, sorted); });
}

extern "C" int runia_cons_pairs(const void* ids, int id_bytes, int64_t groups, int64_t k, int64_t T, int64_t row_stride,
                                int64_t col_stride, const int64_t* eos, int n_eos, const int64_t* lengths, int what,
                                int32_t* len, int32_t* lcs, int32_t* uniq, int32_t* inter, void* workspace,
                                size_t workspace_bytes, runia_stream_t stream) {
  const bool want_lcs = what & RUNIA_CONS_LCS, want_jac = what & RUNIA_CONS_JACCARD;
  if (!pairs_shape_ok(groups, k, T) || (id_bytes != 4 && id_bytes != 8) || (!ids && T > 0) || row_stride < 0 ||
      col_stride < 0 || n_eos < 0 || n_eos > RUNIA_CONS_MAX_EOS || (n_eos > 0 && !eos) || what < 1 || what > 3 || !len ||
      (want_lcs && !lcs) || (want_jac && (!uniq || !inter)))
    return RUNIA_E_INVALID;
  int64_t* sorted = nullptr;
  if (want_jac) {
    const size_t need = (size_t)runia_cons_pairs_workspace_bytes(groups, k, T, what);
    if (need > 0 && ws_refused(workspace, workspace_bytes, need, 8)) return RUNIA_E_WORKSPACE;
    WsWalk w(workspace);
    sorted_layout(w, groups * k, T, sorted);
  }
  hipStream_t s = as_stream(stream);
  if (id_bytes == 4)
    launch_pairs<int32_t>(ids, groups, (int)k, (int)T, row_stride, col_stride, eos, n_eos, lengths, what, len, lcs, uniq, inter,
                          sorted, s);
  else
    launch_pairs<int64_t>(ids, groups, (int)k, (int)T, row_stride, col_stride, eos, n_eos, lengths, what, len, lcs, uniq, inter,
                          sorted, s);
  return runia_check_launch();
}

extern "C" int runia_cons_graph(const double* W, int64_t groups, int64_t k, double eigv_threshold, double set_threshold,
                                double* eigenvalues, double* u_deg, double* u_eigv, double* u_ecc, double* lexsim,
                                double* c_deg, double* c_ecc, int32_t* num_sets, runia_stream_t stream) {
  if (!W || !eigenvalues || !u_deg || !u_eigv || !u_ecc || !lexsim || !c_deg || !c_ecc || !num_sets || groups < 1 ||
      groups > 0x7fffffffll || k < 2 || k > kMaxK)
    return RUNIA_E_INVALID;
  static std::atomic<uint64_t> lds_ok{0};
  if (runia_allow_dynamic_lds(reinterpret_cast<const void*>(cons_graph_kernel), kGraphLdsBytes, lds_ok) != RUNIA_OK)
    return RUNIA_E_LAUNCH;
  cons_graph_kernel<<<(unsigned)groups, kThreads, kGraphLdsBytes, as_stream(stream)>>>(
      W, (int)k, eigv_threshold, set_threshold, eigenvalues, u_deg, u_eigv, u_ecc, lexsim, c_deg, c_ecc, num_sets);
  return runia_check_launch();
}
