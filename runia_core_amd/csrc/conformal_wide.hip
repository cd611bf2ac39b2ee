// Conformal prediction sets of rows of any width (llm_uncertainty/conformal.py): the next-token sets of an LLM
// generation, V of 32 k to 256 k, read in place through the step table of runia_logit_stats.  The definitions are those of
// conformal.hip; the row is never ordered.  For aps and raps the score is non-decreasing along the order (descending logit,
// equal logits by lower index), so a row's set is a prefix of the order and the kernel finds the cut: a key value and the
// number j of the classes with that key that are in.  One workgroup of 256 threads per row; the row is read again from L2 /
// the Infinity Cache in every pass:
//   0. maximum m and the NaN / +inf flag
//   1-3. radix descent over descending_key(x), digits of 11 / 11 / 10 bits from the top.  The classes whose higher digits match
//      the prefix found so far add 1 to cnt[digit] and e * 2^40 (e = exp(beta (x - m)), an integer) to mass[digit] in LDS.
//      Integer sums are exact in any order: no float atomics, the same bits every run.  S0 is the total of pass 1.  A scan
//      over the bins gives every bin the count and mass ordered before it; the bin taken is the first one with
//      B_end + penalty(rank of its last class) > qhat, B_end the mass up to the bin's end over S0 (every class of a bin before
//      it has s <= B_end + penalty <= qhat: it is in), or the last bin that holds a class where there is none.
//   cut. after three digits the bin is one key value: its g classes share one p and enter by index, so the j of them that are
//      in follow from the monotone score by a binary search (every thread runs it: no broadcast)
//   4. output in index order, coalesced: class c is in iff key_c < cut key, or key_c == cut key with fewer than j equal-key
//      classes at lower indices - a running count carried across chunks, formed only when 0 < j < g.  A thread's bits are
//      joined to 32-class words inside the wave; size is the population count, covered the label's bit.
// lac needs no order (1 - p_c <= qhat): pass 0, a pass for S0, the output pass.  qhat < 0 (every score is >= 0) and
// qhat = +inf are settled after pass 0, a qhat above every score of the row after pass 1.  LDS: 24 KiB of bins
// (2048 x (8 + 4) bytes) and 96 bytes of hand-over.
// 16-byte loads where the row start is 16-byte aligned, element loads otherwise and at the row's end; the element -> lane map
// depends on the element index alone, so a row gives the same bits at any address, in any batch, in any dtype that widens to
// the same f32 values.
#include "common.hpp"
#include "elem.hpp"
#include "conformal_core.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kLoads = 4;                     // 16-byte loads a thread has in flight
constexpr int kMaxBins = 2048;                // the 11-bit digits
constexpr int64_t kMaxWideV = 1ll << 20;      // V e 2^40 < 2^61: the masses of a row fit 64 bits
constexpr int64_t kMaxWideRows = 1ll << 26;   // B * n_steps
constexpr float kFix = 1099511627776.f;       // 2^40

struct Bin {  // the bin the descent takes: count and mass ordered before it, its own count and mass
  uint32_t before, count;
  u64 mass_before, mass;
};

// f(index, logit) for every class of the row; thread i of load q takes elements c0 + (q * 256 + i) * T::V ..
template <class T, class F>
__device__ __forceinline__ void sweep(const char* row, int V, bool aligned, F f) {
  constexpr int W = T::V;
  for (int c0 = 0; c0 < V; c0 += kThreads * W * kLoads) {
    float v[kLoads][W];
#pragma unroll
    for (int q = 0; q < kLoads; ++q) {
      const int j = c0 + (q * kThreads + (int)threadIdx.x) * W;
      if (j < V) {
        load_vec<T>(row, j, V, aligned, v[q]);
      } else {
#pragma unroll
        for (int e = 0; e < W; ++e) v[q][e] = -INFINITY;
      }
    }
#pragma unroll
    for (int q = 0; q < kLoads; ++q) {
      const int j = c0 + (q * kThreads + (int)threadIdx.x) * W;
#pragma unroll
      for (int e = 0; e < W; ++e) {
        if (j + e < V) f(j + e, v[q][e]);
      }
    }
  }
}

// The workgroup's reductions: every thread calls them, every thread gets the result; `red` is free again on return.
struct Red {
  u64 m[kThreads / 64];
  uint32_t c[kThreads / 64];
  float f[kThreads / 64];
};

__device__ __forceinline__ void block_max_flag(float& m, int& bad, Red& red) {
  m = wave_max_f32(m);
  bad = wave_or(bad);
  if ((threadIdx.x & 63) == 0) {
    red.f[threadIdx.x >> 6] = m;
    red.c[threadIdx.x >> 6] = (uint32_t)bad;
  }
  __syncthreads();
  m = fmaxf(fmaxf(red.f[0], red.f[1]), fmaxf(red.f[2], red.f[3]));
  bad = (int)(red.c[0] | red.c[1] | red.c[2] | red.c[3]);
  __syncthreads();
}

__device__ __forceinline__ void block_sum(uint32_t& c, u64& m, Red& red) {
  c = wave_sum(c);
  m = wave_sum(m);
  if ((threadIdx.x & 63) == 0) {
    red.c[threadIdx.x >> 6] = c;
    red.m[threadIdx.x >> 6] = m;
  }
  __syncthreads();
  c = red.c[0] + red.c[1] + red.c[2] + red.c[3];
  m = red.m[0] + red.m[1] + red.m[2] + red.m[3];
  __syncthreads();
}

// (c, m) <- their sums over the threads before this one; (tc, tm) <- over all threads
__device__ __forceinline__ void block_exclusive_scan(uint32_t& c, u64& m, uint32_t& tc, u64& tm, Red& red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t ic = wave_scan_incl(c);
  const u64 im = wave_scan_incl(m);
  if (lane == 63) {
    red.c[wave] = ic;
    red.m[wave] = im;
  }
  __syncthreads();
  uint32_t oc = 0, ac = 0;
  u64 om = 0, am = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    if (w == wave) {
      oc = ac;
      om = am;
    }
    ac += red.c[w];
    am += red.m[w];
  }
  __syncthreads();
  c = oc + ic - c;
  m = om + im - m;
  tc = ac;
  tm = am;
}

template <class T>
__global__ __launch_bounds__(kThreads) void conformal_sets_wide_kernel(const StepDesc* __restrict__ tab, int64_t n_steps,
                                                                       int64_t rows, int V, Labels L, int64_t label_stride,
                                                                       const float* __restrict__ u, Method M, float qhat,
                                                                       int32_t* __restrict__ size,
                                                                       int32_t* __restrict__ members,
                                                                       uint8_t* __restrict__ covered) {
  constexpr int W = T::V;        // classes per load
  constexpr int LPW = 32 / W;    // lanes that hold one word of members
  __shared__ u64 mass[kMaxBins];
  __shared__ uint32_t cnt[kMaxBins];
  __shared__ Red red;
  __shared__ Bin taken;
  __shared__ int first_over, last_held, label_in;
  const int tid = threadIdx.x;
  const int words = (V + 31) >> 5;
  const uint32_t key_ninf = descending_key(-INFINITY);
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {  // r = b * n_steps + t: the output row
    const int64_t b = r / n_steps, t = r - b * n_steps;
    const StepDesc sd = tab[t];
    const char* row = step_row<T>(sd, b);
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    bool used;
    const int y = row_class(L, b * label_stride + t, V, used);
    if (tid == 0) label_in = 0;

    // 0. the maximum and the flag
    float m = -INFINITY;
    int bad = 0;
    sweep<T>(row, V, aligned, [&](int, float x) {
      m = fmaxf(m, x);
      bad |= (x != x) | (x == INFINITY);
    });
    block_max_flag(m, bad, red);  // (its barriers also order label_in = 0 before the output pass)
    if (bad || !(m > -INFINITY) || qhat < 0.f) {  // no softmax, or no score that low: the empty set
      if (members) {
        for (int w = tid; w < words; w += kThreads) members[r * words + w] = 0;
      }
      if (tid == 0) {
        size[r] = 0;
        if (covered) covered[r] = 0;
      }
      continue;
    }

    // the cut: class c is in iff key_c < cut_key, or key_c == cut_key and fewer than j equal-key classes lie before it
    uint32_t cut_key = 0xffffffffu;  // qhat = +inf: every class (the key of -inf is below it)
    uint32_t j = 0, group = 0;
    bool lac = false;
    float r_s0 = 0.f;
    if (qhat < INFINITY && M.kind == kLac) {
      lac = true;
      uint32_t none = 0;
      u64 s0 = 0;
      sweep<T>(row, V, aligned, [&](int, float x) { s0 += (u64)(softmax_term(x, m, M.beta) * kFix); });
      block_sum(none, s0, red);
      r_s0 = (float)((double)kFix / (double)s0);
    } else if (qhat < INFINITY) {
      const float ur = u ? u[r] : 1.f;
      uint32_t prefix = 0, before = 0;
      u64 mass_before = 0;
      double inv = 0.0;
      for (int level = 0; level < 3; ++level) {
        const int shift = level == 0 ? 21 : level == 1 ? 10 : 0;
        const int nb = level == 2 ? 1024 : 2048;
        const uint32_t above = level == 0 ? 0u : ~0u << (level == 1 ? 21 : 10);  // the digits already fixed
        for (int i = tid; i < nb; i += kThreads) {
          cnt[i] = 0;
          mass[i] = 0;
        }
        if (tid == 0) {
          first_over = nb;
          last_held = -1;
        }
        __syncthreads();
        uint32_t n_ninf = 0;  // classes at -inf (a top-k warper leaves most of the row there): counted in a register
        sweep<T>(row, V, aligned, [&](int, float x) {
          if (x == -INFINITY) {
            n_ninf += 1;
            return;
          }
          const uint32_t k = descending_key(x);
          if ((k & above) != prefix) return;
          const int bin = (int)((k >> shift) & (uint32_t)(nb - 1));
          atomicAdd(&cnt[bin], 1u);
          const u64 e = (u64)(softmax_term(x, m, M.beta) * kFix);
          if (e) atomicAdd(&mass[bin], e);
        });
        if (n_ninf && (key_ninf & above) == prefix) atomicAdd(&cnt[(key_ninf >> shift) & (uint32_t)(nb - 1)], n_ninf);
        __syncthreads();
        // a thread owns nb / 256 consecutive bins
        const int per = nb / kThreads, bin0 = tid * per;
        uint32_t c_run = 0, c_all;
        u64 m_run = 0, m_all;
        for (int i = 0; i < per; ++i) {
          c_run += cnt[bin0 + i];
          m_run += mass[bin0 + i];
        }
        block_exclusive_scan(c_run, m_run, c_all, m_all, red);
        if (level == 0) inv = 1.0 / (double)m_all;  // S0 >= 2^40: the maximum's own term
        c_run += before;
        m_run += mass_before;
        int my_over = -1, my_held = -1;
        Bin over = {0, 0, 0, 0}, held = {0, 0, 0, 0};
        for (int i = 0; i < per; ++i) {
          const uint32_t c = cnt[bin0 + i];
          const u64 ms = mass[bin0 + i];
          if (c == 0) continue;
          const Bin here = {c_run, c, m_run, ms};
          c_run += c;
          m_run += ms;
          const float b_end = (float)((double)m_run * inv);
          if (my_over < 0 && score_of(M, 0.f, b_end, 0.f, (int)c_run) > qhat) {
            my_over = bin0 + i;
            over = here;
          }
          my_held = bin0 + i;
          held = here;
        }
        if (my_over >= 0) atomicMin(&first_over, my_over);
        if (my_held >= 0) atomicMax(&last_held, my_held);
        __syncthreads();
        if (level == 0 && first_over >= nb) {  // qhat is above every score: the cut is fixed, every class is in
          group = 0;
          break;  // (the same in every thread; nothing of this level is read after the barrier above)
        }
        const int bin = first_over < nb ? first_over : last_held;
        if (first_over < nb) {
          if (bin == my_over) taken = over;
        } else if (bin == my_held) {
          taken = held;
        }
        __syncthreads();
        before = taken.before;
        mass_before = taken.mass_before;
        group = taken.count;
        prefix |= (uint32_t)bin << shift;
        __syncthreads();  // (taken, first_over and the bins are written again from here)
      }
      // the bin is one key: g classes of one p, entering by index.  j = the largest i in [0, g] with s_i <= qhat
      if (group) cut_key = prefix;
      const float e = softmax_term(key_logit(cut_key), m, M.beta);
      const u64 e_fix = (u64)(e * kFix);
      const float p = e * (float)((double)kFix * inv);
      uint32_t lo = 0, hi = group;
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        const float b_mid = (float)((double)(mass_before + (u64)(mid - 1) * e_fix) * inv);
        if (score_of(M, p, b_mid, ur, (int)(before + mid)) <= qhat) lo = mid;
        else hi = mid - 1;
      }
      j = lo;
    }

    // 4. the output pass
    const bool whole = j >= group;        // the equal-key group is in as a whole (or, with j = 0 = g, there is none)
    const bool tie = j > 0 && j < group;  // the cut falls inside it: the running count of equal keys
    uint32_t run = 0, n_in = 0;
    int hit = 0;
    for (int c0 = 0; c0 < V; c0 += kThreads * W * kLoads) {
      float v[kLoads][W];
#pragma unroll
      for (int q = 0; q < kLoads; ++q) {
        const int j0 = c0 + (q * kThreads + tid) * W;
        if (j0 < V) {
          load_vec<T>(row, j0, V, aligned, v[q]);
        } else {
#pragma unroll
          for (int e = 0; e < W; ++e) v[q][e] = -INFINITY;
        }
      }
#pragma unroll
      for (int q = 0; q < kLoads; ++q) {
        const int j0 = c0 + (q * kThreads + tid) * W;
        uint32_t in = 0, eq = 0;
#pragma unroll
        for (int e = 0; e < W; ++e) {
          if (j0 + e >= V) continue;
          if (lac) {
            in |= (score_of(M, softmax_term(v[q][e], m, M.beta) * r_s0, 0.f, 0.f, 0) <= qhat ? 1u : 0u) << e;
          } else {
            const uint32_t k = descending_key(v[q][e]);
            in |= (k < cut_key ? 1u : 0u) << e;
            eq |= (k == cut_key ? 1u : 0u) << e;
          }
        }
        if (whole) in |= eq;
        if (tie) {  // (the same in every thread of the workgroup)
          uint32_t pos = (uint32_t)__popc(eq), total;
          u64 none = 0, none_all;
          block_exclusive_scan(pos, none, total, none_all, red);
          pos += run;
          run += total;
#pragma unroll
          for (int e = 0; e < W; ++e) {
            if ((eq >> e) & 1u) {
              in |= (pos < j ? 1u : 0u) << e;
              pos += 1;
            }
          }
        }
        n_in += (uint32_t)__popc(in);
        if (used && y >= j0 && y < j0 + W) hit = (int)((in >> (y - j0)) & 1u);
        uint32_t word = in << ((tid & (LPW - 1)) * W);
#pragma unroll
        for (int o = 1; o < LPW; o <<= 1) word |= __shfl_xor(word, o, 64);
        const int w = j0 >> 5;
        if (members && (tid & (LPW - 1)) == 0 && w < words) members[r * words + w] = (int32_t)word;
      }
    }
    if (hit) label_in = 1;
    u64 none = 0;
    block_sum(n_in, none, red);  // (its barriers: label_in is written before thread 0 reads it, and read before the next row)
    if (tid == 0) {
      size[r] = (int32_t)n_in;
      if (covered) covered[r] = label_in ? 1 : 0;
    }
  }
}

}  // namespace

extern "C" int runia_conformal_sets_wide(const void* table, int dtype, int64_t n_steps, int64_t B, int64_t V, const void* labels,
                                         int labels_i64, int64_t label_stride, int has_ignore, int64_t ignore_index,
                                         const float* u, int method, float beta, float lam, int k_reg, float qhat, int32_t* size,
                                         int32_t* members, uint8_t* covered, runia_stream_t stream) {
  if (!elem_dtype_ok(dtype) || n_steps < 1 || B < 1 || V < 1 || V > kMaxWideV || B > kMaxWideRows ||
      n_steps > kMaxWideRows / B || !method_ok(method, beta, lam, k_reg) || qhat != qhat)
    return RUNIA_E_INVALID;
  if (!table || !size || (covered && !labels) || (labels && B > 1 && label_stride < n_steps)) return RUNIA_E_INVALID;
  const Labels L = {labels, labels_i64 != 0, has_ignore != 0, ignore_index};
  const Method M = {method, beta, lam, k_reg};
  const int64_t rows = B * n_steps;
  const unsigned grid = (unsigned)(rows < (1ll << 20) ? rows : (1ll << 20));
  hipStream_t s = as_stream(stream);
  dispatch_elem(dtype, [&](auto tag) {
    conformal_sets_wide_kernel<decltype(tag)><<<grid, kThreads, 0, s>>>(static_cast<const StepDesc*>(table), n_steps, rows,
                                                                        (int)V, L, label_stride, u, M, qhat, size, members,
                                                                        covered);
  });
  return runia_check_launch();
}
