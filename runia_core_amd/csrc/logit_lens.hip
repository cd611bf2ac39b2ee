// Logit lens: what an intermediate layer would have predicted, DESIGN 4.60.  A table of state rows (the chosen layers' window
// states after the final norm, [planes, N, d]) is multiplied with the unembedding W [V, d] on the matrix cores, and the few
// numbers wanted per row - log-sum-exp, entropy, the target's logit, the arg-max, the divergence of the final layer's
// distribution from the row's - are taken as online reductions over the vocabulary while the logits are still in
// accumulator registers.  Nothing of size N x V is ever written.
//
// Orientation.  The product is W-tile x states-tile^T: vocabulary ids are the ROWS of a 32 x 32 MFMA result, state rows its
// columns.  Lane l of a wave owns state column l & 31; the 16 accumulator registers of a tile are 16 vocabulary ids of that
// state (id (r & 3) + 8 (r >> 2) + 4 (l >> 5), ascending in r), so the running statistics are a serial per-lane update with
// no cross-lane work in the vocabulary loop.  The two lane halves and the two vocabulary waves meet once, in LDS, at the end.
//
// Workgroup: 256 threads, one vocabulary CHUNK (lens_steps_per_chunk(V) steps of kStep = 128 ids) of one block of 32 positions for
// one GROUP of kSlots = 4 planes: a 128-id x 128-column tile, 4 waves of 64 x 64 (2 x 2 MFMA tiles; four fragment reads feed
// four matrix instructions of the 16-bit forms).  Wave w: vocabulary half w & 1, plane pair w >> 1.  With a final plane, slot 0
// of EVERY group is the final plane and the other three slots take the remaining planes in order: the wave that holds slot 0
// puts its logits of the step into LDS ([vocabulary half][tile][register][lane] f32, 16 KB), and every wave reads the final
// logit of its own (vocabulary id, position) back at its own lane and register index - no permutes, no second product inside a
// group.  Groups past the first recompute the final plane (the same instructions on the same data: the same bits); what that
// costs is stated in DESIGN 4.60.
//
// K runs over d in stages of 64 bytes per row (32 k of a 16-bit type, 16 k of f32), fetched global -> registers one stage
// ahead and written to one of two LDS buffers (pitch 80 bytes: 16 consecutive rows fall into the 16 different 16-byte bank
// groups), one barrier per stage.  Rows past V or N, planes a group does not have and the d tail are staged as zeros; a padded
// vocabulary id is masked to -inf before it can enter a maximum or a sum.  The state tile is restaged from L2 for every
// step; W streams from HBM once per position block and group.
//
// Per lane and slot: m, s = sum e^(z-m), u = sum e^(z-m) (z-m) (entropy = log s - u / s: no cancellation against |z|), the
// first arg-max id, the target's logit, and with a final plane c = sum e^(y-m_y) (z-m) with the final row's m_y, s_y over the
// same ids.  A step's maximum is taken first, everything is rescaled once per step, then the step's 32 ids are added.
//
// Vocabulary split.  V is cut into S = S(V) <= RUNIA_LENS_MAX_SPLIT chunks - S depends on V alone, so a position's bits do
// not depend on N or on the other rows of the call.  Each (chunk, plane, position) leaves one 32-byte record; lens_merge_kernel
// folds the S records in ascending chunk order in f64 and writes the outputs.  No atomics.
//
// A NaN or infinite state value is noticed while the state tile is staged (every workgroup sees all d values of its columns
// during its first step) and turns the column's record into NaN: the matrix cores keep a column's NaN inside the column, the
// flag makes the row's outputs NaN whatever the arithmetic would have left (inf - inf, comparisons that drop a NaN).
#include "common.hpp"
#include "elem.hpp"

#include <type_traits>

namespace {

constexpr int kTile = RUNIA_LENS_VOCAB_TILE;  // 32: one MFMA tile of vocabulary ids
constexpr int kStep = RUNIA_LENS_VOCAB_STEP;  // 128: ids per workgroup step
constexpr int kMaxSplit = RUNIA_LENS_MAX_SPLIT;
constexpr int kSlots = RUNIA_LENS_GROUP_PLANES;  // plane slots of a group
constexpr int kPos = 32;                          // positions per workgroup
constexpr int kCols = kSlots * kPos;              // 128 state columns
constexpr int kPitch = 5;                         // uint4 per staged row: 64 bytes of k + 16 of padding
constexpr int kStageVec = (kStep + kCols) * kPitch;
static_assert(kTile == 32 && kStep == 128 && kSlots == 4, "the wave layout below is written for these");

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct Rec { float m, s, u, c, ztok; int top; float pad0, pad1; };  // one (chunk, plane, position); m = NaN: a bad state row
static_assert(sizeof(Rec) == 32, "two 16-byte stores");

__host__ __device__ inline int64_t lens_steps(int64_t V) { return (V + kStep - 1) / kStep; }
__host__ __device__ inline int64_t lens_steps_per_chunk(int64_t V) { return (lens_steps(V) + kMaxSplit - 1) / kMaxSplit; }
__host__ __device__ inline int64_t lens_split(int64_t V) {
  const int64_t t = lens_steps_per_chunk(V);
  return (lens_steps(V) + t - 1) / t;
}
__host__ __device__ inline int64_t lens_groups(int64_t planes, int64_t final_plane) {
  if (final_plane < 0) return (planes + kSlots - 1) / kSlots;
  const int64_t g = (planes - 1 + kSlots - 2) / (kSlots - 1);
  return g < 1 ? 1 : g;
}
// the plane of slot j of group g, or -1
__device__ __forceinline__ int64_t slot_plane(int64_t g, int j, int64_t planes, int64_t fp) {
  if (fp < 0) {
    const int64_t p = g * kSlots + j;
    return p < planes ? p : -1;
  }
  if (j == 0) return fp;
  const int64_t i = g * (kSlots - 1) + (j - 1), p = i < fp ? i : i + 1;
  return p < planes ? p : -1;
}

template <class T>
__device__ __forceinline__ bool any_nonfinite(uint4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (T::kBytes == 4) {
      bad |= (w[i] & 0x7f800000u) == 0x7f800000u;
    } else {
      constexpr uint32_t e = std::is_same<T, F16>::value ? 0x7c00u : 0x7f80u;
      bad |= (w[i] & e) == e || ((w[i] >> 16) & e) == e;
    }
  }
  return bad;
}

// 16 bytes of a row from element k (a multiple of T::V), zero past d: one vector load where the row allows it
template <class T>
__device__ __forceinline__ uint4 load_slot(const typename T::elem* row, int64_t k, int64_t d, bool aligned) {
  if (!row || k >= d) return make_uint4(0u, 0u, 0u, 0u);
  if (aligned && k + T::V <= d) return *reinterpret_cast<const uint4*>(row + k);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if constexpr (T::kBytes == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < d) w[e] = __float_as_uint(row[k + e]);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < d) w[e >> 1] |= (uint32_t)row[k + e] << (16 * (e & 1));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// one 16-byte fragment pair -> the matrix instruction(s) of its k range (f32: four of two k each, the same k order in both
// operands)
template <class T>
__device__ __forceinline__ void mma(f32x16& acc, uint4 a, uint4 b) {
  if constexpr (std::is_same<T, BF16>::value) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  } else if constexpr (std::is_same<T, F16>::value) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
}

constexpr float kLog2e = 1.44269504088896341f;
// e^t of a clamped t in [-200, 0]: the product's rounding moves a term by <= |t| 2^-24 of itself, and a term weighs e^t
__device__ __forceinline__ float exp_term(float t) { return __builtin_amdgcn_exp2f(t * kLog2e); }
__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

// what one holder (a lane, a workgroup, a chunk) knows of a row over its share of the vocabulary; m = -inf: nothing yet
template <class F>
struct Part {
  F m, s, u, c, ym, ys;
  int top;
};

// `p` (ids above those of `t` or not: the arg-max takes the lower id on a tie) folded into `t`
template <class F>
__device__ __forceinline__ void fold(Part<F>& t, const Part<F>& p) {
  const F ninf = -(F)__builtin_inff();
  if (p.m != p.m || t.m != t.m) {  // a bad state row
    t.m = (F)__builtin_nanf("");
    return;
  }
  if (p.m == ninf) return;
  if (t.m == ninf) {
    t = p;
    return;
  }
  if (p.m > t.m || (p.m == t.m && p.top < t.top)) t.top = p.top;
  const F M = p.m > t.m ? p.m : t.m, dt = t.m - M, dp = p.m - M;
  const F ym = p.ym > t.ym ? p.ym : t.ym;
  const F at = exp(dt), ap = exp(dp);
  // (without a final plane ym stays -inf on both sides: the y terms are not used then)
  const F yt = t.ym == ninf ? (F)0 : exp(t.ym - ym), yp = p.ym == ninf ? (F)0 : exp(p.ym - ym);
  t.u = at * (t.u + dt * t.s) + ap * (p.u + dp * p.s);
  t.c = yt * (t.c + dt * t.ys) + yp * (p.c + dp * p.ys);
  t.s = at * t.s + ap * p.s;
  t.ys = yt * t.ys + yp * p.ys;
  t.m = M;
  t.ym = ym;
}

template <class T>
__global__ __launch_bounds__(256) void lens_kernel(const typename T::elem* __restrict__ states,
                                                   const typename T::elem* __restrict__ weight, int64_t wstride,
                                                   int64_t planes, int64_t N, int64_t V, int64_t d,
                                                   const int64_t* __restrict__ tokens, int64_t fp, int64_t groups,
                                                   int64_t npb, Rec* __restrict__ recs) {
  __shared__ __attribute__((aligned(16))) uint4 stage[2 * kStageVec];  // 2 x (128 W rows + 128 state columns) x 80 bytes
  __shared__ float ylds[2 * 2 * 16 * 64];                              // the final plane's logits of the step
  __shared__ int bad[kCols];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wv = wave & 1, wp = wave >> 1;
  const int64_t g = blockIdx.x % groups, pb = (blockIdx.x / groups) % npb, chunk = blockIdx.x / (groups * npb);
  const int64_t n0 = pb * kPos;
  const int64_t spc = lens_steps_per_chunk(V), nsteps = lens_steps(V);
  const int64_t step0 = chunk * spc, step1 = step0 + spc < nsteps ? step0 + spc : nsteps;
  const bool has_final = fp >= 0;  // (uniform)

  // staging: thread t moves 16-byte slot t & 3 of W rows / state columns t >> 2 and (t >> 2) + 64
  const int srow = tid >> 2, sq = tid & 3;
  const bool w_al = (reinterpret_cast<uintptr_t>(weight) & 15) == 0 && ((wstride * T::kBytes) & 15) == 0;
  const bool s_al = (reinterpret_cast<uintptr_t>(states) & 15) == 0 && ((d * T::kBytes) & 15) == 0;
  const typename T::elem* srows[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int col = srow + 64 * h;
    const int64_t p = slot_plane(g, col >> 5, planes, fp), n = n0 + (col & 31);
    srows[h] = (p >= 0 && n < N) ? states + (p * N + n) * d : nullptr;
  }
  if (tid < kCols) bad[tid] = 0;
  __syncthreads();

  // the slots of this wave (2 wp, 2 wp + 1) and what this lane tracks for them
  bool valid[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) valid[b] = slot_plane(g, 2 * wp + b, planes, fp) >= 0;  // (uniform)
  const int64_t npos = n0 + li;
  const int64_t tok = (tokens && npos < N) ? tokens[npos] : -1;
  Part<float> st[2];
  float ztok[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    st[b].m = st[b].ym = neg_inf();
    st[b].s = st[b].u = st[b].c = st[b].ys = 0.f;
    st[b].top = 0;
    ztok[b] = __builtin_nanf("");
  }

  constexpr int kPerStage = 4 * T::V;  // k per stage: 4 slots of T::V elements
  const int64_t nstage = (d + kPerStage - 1) / kPerStage;
  for (int64_t step = step0; step < step1; ++step) {
    const int64_t v0 = step * kStep;
    const typename T::elem* wrows[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t v = v0 + srow + 64 * h;
      wrows[h] = v < V ? weight + v * wstride : nullptr;
    }
    const bool check = step == step0;  // (uniform)
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    uint4 fw[2], fs[2];
    auto fetch = [&](int64_t sg) {
      const int64_t k = sg * kPerStage + sq * T::V;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        fw[h] = load_slot<T>(wrows[h], k, d, w_al);
        fs[h] = load_slot<T>(srows[h], k, d, s_al);
      }
    };
    auto store = [&](int buf) {
      uint4* base = stage + buf * kStageVec;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        base[(srow + 64 * h) * kPitch + sq] = fw[h];
        base[(kStep + srow + 64 * h) * kPitch + sq] = fs[h];
        if (check && any_nonfinite<T>(fs[h])) bad[srow + 64 * h] = 1;
      }
    };
    fetch(0);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int64_t sg = 0; sg < nstage; ++sg) {
      const bool more = sg + 1 < nstage;  // (uniform)
      if (more) fetch(sg + 1);
      const uint4* pa = stage + buf * kStageVec + (wv * 64 + li) * kPitch + lh;
      const uint4* pbs = stage + buf * kStageVec + (kStep + wp * 64 + li) * kPitch + lh;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint4 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) fa[a] = pa[a * 32 * kPitch + 2 * s];
#pragma unroll
        for (int b = 0; b < 2; ++b) fb[b] = pbs[b * 32 * kPitch + 2 * s];
#pragma unroll
        for (int b = 0; b < 2; ++b)
          if (valid[b]) {
#pragma unroll
            for (int a = 0; a < 2; ++a) mma<T>(acc[a][b], fa[a], fb[b]);
          }
      }
      __builtin_amdgcn_sched_barrier(0);  // (the fetched values are first touched here)
      if (more) store(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }

    // ---- the step's 64 ids of this lane, per slot ----
    if (has_final) {
      if (wp == 0) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int r = 0; r < 16; ++r) ylds[((wv * 2 + a) * 16 + r) * 64 + lane] = acc[a][0][r];
      }
      __syncthreads();  // (the next write is behind the barriers of the next step's stages)
    }
    const int64_t vlane = v0 + wv * 64 + 4 * lh;  // id of (a, r): vlane + 32 a + (r & 3) + 8 (r >> 2)
    float y[2][16];
    float ym_new = st[0].ym;
    if (has_final) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t v = vlane + 32 * a + (r & 3) + 8 * (r >> 2);
          const float t = ylds[((wv * 2 + a) * 16 + r) * 64 + lane];
          y[a][r] = v < V ? t : neg_inf();
          ym_new = y[a][r] > ym_new ? y[a][r] : ym_new;
        }
    }
    const float ymref = ym_new == neg_inf() ? 0.f : ym_new;
    const bool y_first = st[0].ym == neg_inf();
    const float y_scale = y_first ? 0.f : exp_term(st[0].ym - ym_new);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (!valid[b]) continue;
      float m_new = st[b].m;
      int top = st[b].top;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t v = vlane + 32 * a + (r & 3) + 8 * (r >> 2);
          const float z = v < V ? acc[a][b][r] : neg_inf();
          acc[a][b][r] = z;
          if (z > m_new) {  // strict: the first id that attains the maximum (ids ascend with a, r and the step)
            m_new = z;
            top = (int)v;
          }
          if (v == tok) ztok[b] = z;
        }
      const bool first = st[b].m == neg_inf();
      const float mref = m_new == neg_inf() ? 0.f : m_new;
      const float dm = first ? 0.f : st[b].m - m_new;
      const float scale = first ? 0.f : exp_term(dm);
      float s = scale * st[b].s, u = scale * (st[b].u + dm * st[b].s);
      float c = y_scale * (st[b].c + dm * st[b].ys);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float t = fmaxf(acc[a][b][r] - mref, -200.f);  // (a masked id: e = 0, e t = 0)
          const float e = exp_term(t);
          s += e;
          u += e * t;
          if (has_final) c += exp_term(fmaxf(y[a][r] - ymref, -200.f)) * t;
        }
      st[b].m = m_new;
      st[b].top = top;
      st[b].s = s;
      st[b].u = u;
      st[b].c = c;
    }
    if (has_final) {  // the final row's own sum over this lane's ids (one per lane: both slots see the same positions)
      float ys = y_scale * st[0].ys;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) ys += exp_term(fmaxf(y[a][r] - ymref, -200.f));
      st[0].ys = st[1].ys = ys;
      st[0].ym = st[1].ym = ym_new;
    }
  }

  // ---- the four holders of a (slot, position) meet: lane halves and vocabulary waves, ascending ids ----
  __syncthreads();  // the stage buffers are free
  Part<float>* parts = reinterpret_cast<Part<float>*>(stage);  // [slot][holder = 2 wv + lh][position]
  float* zt = reinterpret_cast<float*>(parts + kSlots * 4 * kPos);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int at = ((2 * wp + b) * 4 + 2 * wv + lh) * kPos + li;
    parts[at] = st[b];
    zt[at] = ztok[b];
  }
  __syncthreads();
  if (tid < kCols) {
    const int j = tid >> 5, pos = tid & 31;
    const int64_t p = slot_plane(g, j, planes, fp), n = n0 + pos;
    if (p >= 0 && n < N && !(has_final && j == 0 && g > 0)) {  // (a recomputed final plane is group 0's to write)
      Part<float> t = parts[(j * 4) * kPos + pos];
      float z = zt[(j * 4) * kPos + pos];
#pragma unroll
      for (int h = 1; h < 4; ++h) {
        fold(t, parts[(j * 4 + h) * kPos + pos]);
        const float zh = zt[(j * 4 + h) * kPos + pos];
        z = z == z ? z : zh;
      }
      Rec r;
      r.m = bad[tid] ? __builtin_nanf("") : t.m;
      r.s = t.s, r.u = t.u, r.c = t.c, r.ztok = z, r.top = t.top, r.pad0 = r.pad1 = 0.f;
      float4* out = reinterpret_cast<float4*>(recs + (chunk * planes + p) * N + n);
      out[0] = make_float4(r.m, r.s, r.u, r.c);
      out[1] = make_float4(r.ztok, __int_as_float(r.top), 0.f, 0.f);
    }
  }
}

// the S records of a (plane, position) in ascending chunk order, f64; one thread per row
__global__ __launch_bounds__(256) void lens_merge_kernel(const Rec* __restrict__ recs, int64_t planes, int64_t N, int64_t V,
                                                         int64_t S, const int64_t* __restrict__ tokens, int64_t fp,
                                                         float* __restrict__ lse, float* __restrict__ entropy,
                                                         float* __restrict__ log_prob, float* __restrict__ top_log_prob,
                                                         int32_t* __restrict__ top_token, float* __restrict__ kl_final) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= planes * N) return;
  const int64_t p = i / N, n = i % N;
  const double ninf = -__builtin_inf(), nan = __builtin_nan("");
  Part<double> t;
  t.m = t.ym = ninf;
  t.s = t.u = t.c = t.ys = 0.0;
  t.top = 0;
  Part<double> ty = t;  // the final row's own m, s, u, folded alongside
  const int64_t tok = tokens ? tokens[n] : -1;
  const bool has_tok = tok >= 0 && tok < V;
  const int64_t tok_chunk = has_tok ? (tok / kStep) / lens_steps_per_chunk(V) : -1;
  double ztok = nan;
  for (int64_t c = 0; c < S; ++c) {
    const Rec r = recs[(c * planes + p) * N + n];
    Part<double> q;
    q.m = r.m, q.s = r.s, q.u = r.u, q.c = r.c, q.top = r.top;
    q.ym = ninf, q.ys = 0.0;
    if (fp >= 0) {
      const Rec f = recs[(c * planes + fp) * N + n];
      q.ym = f.m, q.ys = f.s;
      Part<double> qy;
      qy.m = f.m, qy.s = f.s, qy.u = f.u, qy.c = 0.0, qy.ym = ninf, qy.ys = 0.0, qy.top = f.top;
      fold(ty, qy);
    }
    if (c == tok_chunk) ztok = r.ztok;
    fold(t, q);
  }
  const bool bad = t.m != t.m;
  const double ls = log(t.s), l = t.m + ls;
  if (lse) lse[i] = bad ? (float)nan : (float)l;
  if (entropy) entropy[i] = bad ? (float)nan : (float)(ls - t.u / t.s);
  if (log_prob) log_prob[i] = (bad || !has_tok) ? (float)nan : (float)(ztok - l);
  if (top_log_prob) top_log_prob[i] = bad ? (float)nan : (float)(-ls);
  if (top_token) top_token[i] = bad ? -1 : t.top;
  if (kl_final) {
    double kl = nan;
    if (fp >= 0 && !bad && ty.m == ty.m) kl = (ty.u - t.c) / ty.s - log(ty.s) + ls;
    kl_final[i] = (float)kl;
  }
}

struct Plan {
  Rec* recs;  // [min(steps, max split)][planes][N]
};
// the records of every chunk the split can have at this V: through S alone does V enter
Plan make_plan(WsWalk& w, int64_t planes, int64_t N, int64_t V) {
  const int64_t cap = lens_steps(V) < kMaxSplit ? lens_steps(V) : kMaxSplit;
  Plan p;
  p.recs = w.take<Rec>((size_t)(cap * planes * N), 16);
  return p;
}

bool dims_ok(int64_t planes, int64_t N, int64_t V, int64_t d) {
  return planes >= 1 && N >= 1 && V >= 1 && d >= 1 && V <= RUNIA_LENS_MAX_VOCAB && planes <= (1 << 20) &&
         N <= ((int64_t)1 << 31) / planes && d <= ((int64_t)1 << 31);
}

}  // namespace

extern "C" int64_t runia_lens_workspace_bytes(int64_t planes, int64_t N, int64_t V, int64_t d) {
  if (!dims_ok(planes, N, V, d)) return 0;
  return (int64_t)ws_bytes([&](WsWalk& w) { make_plan(w, planes, N, V); });
}

extern "C" int runia_lens_scores(const void* states, const void* weight, int64_t weight_row_stride, int dtype, int64_t planes,
                                 int64_t N, int64_t V, int64_t d, const int64_t* tokens, int64_t final_plane, float* lse,
                                 float* entropy, float* log_prob, float* top_log_prob, int32_t* top_token, float* kl_final,
                                 void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (!states || !weight || !elem_dtype_ok(dtype) || !dims_ok(planes, N, V, d) || final_plane < -1 || final_plane >= planes ||
      (weight_row_stride < d && V > 1) || weight_row_stride < 0)
    return RUNIA_E_INVALID;
  const int64_t groups = lens_groups(planes, final_plane), npb = (N + kPos - 1) / kPos, S = lens_split(V);
  if (groups * npb > ((int64_t)1 << 31) / S - 1) return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const Plan plan = make_plan(w, planes, N, V);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  hipStream_t s = as_stream(stream);
  dispatch_elem(dtype, [&](auto tag) {
    using T = decltype(tag);
    RUNIA_LAUNCH_TIMED(lens_kernel<T>, (unsigned)(S * npb * groups), 256, 0, s, static_cast<const typename T::elem*>(states),
                       static_cast<const typename T::elem*>(weight), weight_row_stride, planes, N, V, d, tokens, final_plane,
                       groups, npb, plan.recs);
    return 0;
  });
  RUNIA_LAUNCH_TIMED(lens_merge_kernel, (unsigned)((planes * N + 255) / 256), 256, 0, s, plan.recs, planes, N, V, S, tokens,
                     final_plane, lse, entropy, log_prob, top_log_prob, top_token, kl_final);
  return runia_check_launch();
}
