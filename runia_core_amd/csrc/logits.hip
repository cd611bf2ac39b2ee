// Per-token scores of an LLM generation from its logits (HuggingFace `generate(output_scores=True).scores`): log-sum-exp,
// the normalised transition score x[tok] - lse (HF compute_transition_scores(normalize_logits=True), reference
// llm_uncertainty/scores.py:452-456, 495-499) and the normalised token entropy of generation_entropy (reference
// scores.py:135-152, utils.py:83-99), for every (row b, step t) in one pass over the T x B x V logits.
//
// The steps are read where they lie: a device table of n_steps descriptors {pointer to row 0, row stride in elements}
// (the vocabulary axis has unit stride), so the caller's tensors are neither stacked nor copied.  Three kernels:
//   partial   one workgroup per (row, chunk of kChunk = 4096 logits): the chunk's online-softmax partial {m, s', u, bad}
//             with m the chunk max, s' = sum e^(x-m) without the max's own term, u = sum e^(x-m) (m - x), bad = a NaN or
//             +inf was seen.  16-byte loads when the row start is 16-byte aligned; the element -> lane map and the
//             summation order depend on the element index only, so a row gives the same bits at any address.
//   finish    one thread per (row, step): merges the row's partials in chunk order in f64, writes lse, log_prob, entropy
//   sequence  one workgroup, one wave per row: f64 means over the steps (generation entropy, perplexity, the mean of the
//             finite log-probs) and normalized_entropy over the rows in row order
// No atomics: every reduction has a fixed order, so repeated calls are bitwise equal, and a row's outputs depend on its
// own V logits only (not on B, T or the other rows).
//
// Numerics.  With S = 1 + s' the softmax denominator relative to the max,
//   lse = m + log1p(s'),   H = -sum p log p = log1p(s') + u / (1 + s'),
// both terms >= 0, so there is no cancellation and peaked rows keep their accuracy.  A -inf logit contributes nothing
// (its e^(x-m) (m-x) = 0 * inf term is skipped explicitly), and neither does a finite one so far below the max that
// m - x, or (m - x) (1 + s') in the f32 lane merges, leaves the f32 range (bf16 / f32 rows holding both signs of
// ~3e38, or torch.finfo(dtype).min as a logits processor's mask value): its weight e^(x-m) is 0 and the same
// 0 * inf is skipped.  log_prob is (x[tok] - m) - log1p(s') in f64, so it keeps the log term whatever the size of m;
// the lse output is m + log1p(s') rounded to f32 and equals m once |m| >= 2^24 log1p(s') (no f32 holds more).
// The reference clamps p at 1e-12 before the log; that moves H by at most V e^-1 1e-12 (4.7e-8 nats, 4e-9 after the
// division by log V at V = 128 256) and is dropped here.  A row that holds NaN or +inf, or only -inf, gives NaN in
// all three outputs, as torch's softmax does; a token whose logit is -inf gets log_prob = -inf exactly.
#include "common.hpp"
#include "elem.hpp"

namespace {

constexpr int kChunk = 4096;  // logits per partial: 256 lanes x 16
constexpr int kThreads = 256;
constexpr int kPerLane = kChunk / kThreads;

struct Partial {  // 16 bytes, one per (row, chunk) in the workspace
  float m, s, u;
  int bad;
};

// p <- p (+) q: the partial of the union of two disjoint element sets.  hi is the partial with the larger max; the lower
// one's terms are rescaled by r = e^(lo.m - hi.m) and its max's own term (1) joins the sum.
template <class T, class P>
__device__ __forceinline__ void merge(T& m, T& s, T& u, int& bad, const P& q) {
  bad |= q.bad;
  const T qm = q.m, qs = q.s, qu = q.u;
  if (!(qm > -(T)__builtin_inff())) return;  // q is empty or all -inf (NaN max: q.bad is set)
  if (!(m > -(T)__builtin_inff())) { m = qm; s = qs; u = qu; return; }
  T hm = m, hs = s, hu = u, ls = qs, lu = qu, lm = qm;
  if (qm > m) { hm = qm; hs = qs; hu = qu; lm = m; ls = s; lu = u; }
  const T d = hm - lm;
  const T r = exp(-d);
  const T l1 = (T)1 + ls;
  m = hm;
  s = hs + r * l1;
  // r = 0 (d past ~104 in f32): the lower partial has no weight left; d, or d * l1 in f32, may be inf there (0 * inf)
  u = hu + (r > (T)0 ? r * (lu + d * l1) : (T)0);
}

// ---- partial -----------------------------------------------------------------------------------------------------------
// block = (row r = t * B + b, chunk c); lane i holds elements c*kChunk + (k*256 + i)*W + e of the row, k < kPerLane / W
template <class T>
__global__ __launch_bounds__(kThreads) void partial_kernel(const StepDesc* __restrict__ tab, int64_t B, int64_t V, int nc,
                                                           Partial* __restrict__ part) {
  constexpr int W = T::V;
  const int64_t blk = blockIdx.x;
  const int64_t r = blk / nc;
  const int c = (int)(blk - r * nc);
  const int64_t t = r / B, b = r - t * B;
  const StepDesc sd = tab[t];
  const char* row = step_row<T>(sd, b);
  const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int lane = threadIdx.x;
  const int64_t c0 = (int64_t)c * kChunk;

  float x[kPerLane];
#pragma unroll
  for (int k = 0; k < kPerLane / W; ++k) load_vec<T>(row, c0 + ((int64_t)k * kThreads + lane) * W, V, aligned, x + k * W);

  float m = -__builtin_inff();
  int bad = 0;
#pragma unroll
  for (int e = 0; e < kPerLane; ++e) {
    m = fmaxf(m, x[e]);
    bad |= (x[e] != x[e]) | (x[e] == __builtin_inff());
  }
  float s = 0.f, u = 0.f;
  if (m > -__builtin_inff()) {
    bool skipped = false;  // the first element equal to the max is the max's own term (1), kept out of s
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
      const bool own = !skipped && x[e] == m;
      skipped |= own;
      const float gap = m - x[e];
      // x = -inf, or finite and more than FLT_MAX below the max: e^(x-m) = 0 and (m - x) = inf, no 0 * inf
      const bool live = !own && gap < __builtin_inff();
      const float d = live ? gap : 0.f;
      // v_exp_f32 of -d log2(e): the rounded product moves e^-d by at most d 2^-24 relative, so s' and u move by at
      // most 6e-8 H relative (H the entropy, <= log V) - 1e-6 of lse at V = 128 256; the accurate expf made the kernel
      // ALU-bound (bf16 as slow as f32)
      const float ex = live ? __builtin_amdgcn_exp2f(d * -1.44269504088896341f) : 0.f;
      s += ex;
      u += ex * d;
    }
  }
  // fixed-order reduction: butterfly in the wave, then the four waves in order
  Partial p{m, s, u, bad};
#pragma unroll  // (hand-written: the butterfly runs from 1 up, wave_reduce merges from the widest step down)
  for (int o = 1; o < 64; o <<= 1) {
    const Partial q = lane_xor(p, o);
    merge(p.m, p.s, p.u, p.bad, q);
  }
  __shared__ Partial waves[kThreads / 64];
  if ((lane & 63) == 0) waves[lane >> 6] = p;
  __syncthreads();
  if (lane == 0) {
    Partial a = waves[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) merge(a.m, a.s, a.u, a.bad, waves[w]);
    part[blk] = a;
  }
}

// ---- finish ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void finish_kernel(const StepDesc* __restrict__ tab, int64_t B, int64_t n_steps, int64_t V,
                                                     int nc, const Partial* __restrict__ part,
                                                     const int64_t* __restrict__ tokens, int64_t token_stride, int normalize,
                                                     float* __restrict__ lse, float* __restrict__ log_prob,
                                                     float* __restrict__ entropy) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // t * B + b
  if (r >= B * n_steps) return;
  const int64_t t = r / B, b = r - t * B;
  double m = -__builtin_inf(), s = 0.0, u = 0.0;
  int bad = 0;
  const Partial* p = part + r * nc;
  for (int c = 0; c < nc; ++c) merge(m, s, u, bad, p[c]);
  const bool nan_row = bad || !(m > -__builtin_inf());
  const double l1p = log1p(s);
  const double row_lse = nan_row ? __builtin_nan("") : m + l1p;
  const int64_t o = b * n_steps + t;
  if (lse) lse[o] = (float)row_lse;
  if (entropy) entropy[o] = nan_row ? __builtin_nanf("") : (float)((l1p + u / (1.0 + s)) / log((double)V));
  if (log_prob) {
    const float xt = ld1<T>(elem_at<T>(step_row<T>(tab[t], b), tokens[b * token_stride + t]));
    // (x - m) - log1p(s'), not x - lse: m + log1p(s') drops the log term in f64 once |m| passes 2^53 (bf16 1e30)
    // x = -inf stays -inf exactly; a NaN row gives NaN whatever the token
    log_prob[o] = !normalize ? xt : nan_row ? __builtin_nanf("") : (float)(((double)xt - m) - l1p);
  }
}

// ---- sequence ----------------------------------------------------------------------------------------------------------
// seq [3B + 1] f64: generation entropy mean_t entropy[b, t], perplexity -mean_t log_prob[b, t], the mean of row b's
// log-probs that are not -inf (NaN when there is none), and normalized_entropy = -mean_b of those means.
__global__ __launch_bounds__(1024) void sequence_kernel(const float* __restrict__ log_prob, const float* __restrict__ entropy,
                                                        int64_t B, int64_t T, double* __restrict__ seq) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  for (int64_t b = wave; b < B; b += waves) {
    double se = 0.0, sl = 0.0, sv = 0.0, nv = 0.0;
    for (int64_t t = lane; t < T; t += 64) {
      const float lp = log_prob[b * T + t];
      se += (double)entropy[b * T + t];
      sl += (double)lp;
      if (lp != -__builtin_inff()) { sv += (double)lp; nv += 1.0; }
    }
    se = wave_sum(se);
    sl = wave_sum(sl);
    sv = wave_sum(sv);
    nv = wave_sum(nv);
    if (lane == 0) {
      seq[b] = se / (double)T;
      seq[B + b] = -sl / (double)T;
      seq[2 * B + b] = sv / nv;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int64_t b = 0; b < B; ++b) acc += seq[2 * B + b];
    seq[3 * B] = -acc / (double)B;
  }
}

int64_t n_chunks(int64_t V) { return (V + kChunk - 1) / kChunk; }

constexpr int64_t kMaxRows = 1ll << 26;  // B * n_steps
constexpr int64_t kMaxV = 1ll << 28;

bool dims_ok(int64_t n_steps, int64_t B, int64_t V) {
  return n_steps >= 1 && B >= 1 && V >= 1 && V <= kMaxV && B <= kMaxRows && n_steps <= kMaxRows / B &&
         B * n_steps * n_chunks(V) < 0x7fffffffll;
}

}  // namespace

extern "C" size_t runia_logit_stats_workspace_bytes(int64_t n_steps, int64_t B, int64_t V) {
  if (!dims_ok(n_steps, B, V)) return 0;
  return (size_t)(B * n_steps * n_chunks(V)) * sizeof(Partial);
}

extern "C" int runia_logit_stats(const void* table, int dtype, int64_t n_steps, int64_t B, int64_t V, const int64_t* tokens,
                                 int64_t token_stride, int normalize, float* lse, float* log_prob, float* entropy,
                                 double* seq, void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (!table || !elem_dtype_ok(dtype) || !dims_ok(n_steps, B, V)) return RUNIA_E_INVALID;
  if (!lse && !log_prob && !entropy && !seq) return RUNIA_E_INVALID;
  if (log_prob && (!tokens || (B > 1 && token_stride < n_steps))) return RUNIA_E_INVALID;
  if (seq && (!log_prob || !entropy)) return RUNIA_E_INVALID;
  const size_t need = runia_logit_stats_workspace_bytes(n_steps, B, V);
  if (ws_refused(workspace, workspace_bytes, need, 16)) return RUNIA_E_WORKSPACE;
  const int nc = (int)n_chunks(V);
  const int64_t rows = B * n_steps;
  const StepDesc* tab = reinterpret_cast<const StepDesc*>(table);
  Partial* part = reinterpret_cast<Partial*>(workspace);
  const hipStream_t s = as_stream(stream);
  dispatch_elem(dtype, [&](auto t) {
    typedef decltype(t) T;
    partial_kernel<T><<<(unsigned)(rows * nc), kThreads, 0, s>>>(tab, B, V, nc, part);
    finish_kernel<T><<<(unsigned)((rows + 255) / 256), 256, 0, s>>>(tab, B, n_steps, V, nc, part, tokens, token_stride,
                                                                     normalize, lse, log_prob, entropy);
  });
  const int rc = runia_check_launch();
  if (rc != RUNIA_OK || !seq) return rc;
  sequence_kernel<<<1, 1024, 0, s>>>(log_prob, entropy, B, n_steps, seq);
  return runia_check_launch();
}
