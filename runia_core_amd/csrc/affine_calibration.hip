// Per-class calibration maps fitted on the device (evaluation/affine_calibration.py): vector scaling and matrix scaling (Guo et
// al. 2017) and Dirichlet calibration with the ODIR regulariser (Kull et al. 2019).
//   runia_affcal_eval: ONE evaluation of the objective and its gradient from ONE read of the logits, nothing N x C written.
// A row has logits x in R^C and a label y.  Its input u and parameter block W are
//   vector     (kind 0)  u = x                                          W = diag(w), w in R^C
//   matrix     (kind 1)  u = x                                          W full C x C
//   dirichlet  (kind 2)  u_k = max(log_softmax(x)_k, log FLT_MIN)       W full C x C      (log FLT_MIN = -87.33654...)
// and z = W u + b, q = softmax(z).  Over the rows whose label is not ignore_index (n of them) the call sums
//   nll = -log q_y        dW = (q - e_y) u^T  (its diagonal for `vector`)        db = q - e_y
// in a fixed order; the 1 / n and the regulariser terms of the objective are the host's.  A non-finite logit of `vector` /
// `matrix`, or a NaN anywhere, makes the row's nll (and so the sum) NaN.
//
// The matrix-core form (affcal_full_kernel; matrix and dirichlet, C <= 256).  C is padded to CP in {32, 64, 128, 256} inside
// the kernel; a padded class has u = 0, z = -inf, q = 0 and is never read from the caller's memory.  A workgroup of W waves
// walks tiles of R rows (Plan<CP>); per tile, between barriers,
//   A  a wave per row: the row is widened into registers, log-softmax and floor applied there for dirichlet (two wave
//      reductions), and written to the tile U [R][CP + 2] in LDS
//   B  Z = U W^T on v_mfma_f32_32x32x2_f32: every wave owns one 32 x 32 block of Z, its A fragments are 8-byte LDS reads, its
//      W fragments come from global memory (W is at most 256 KB: L2-resident); z + b goes to the tile Z [R][CP + 2] in LDS
//   C  2 CP / 32 lanes per row: first argmax, maximum, sum, the row's outputs, and Z is overwritten with R = Q - onehot (0 for
//      a row that is not scored, whose U row is zeroed as well)
//   D  G += R^T U on the same instruction: every wave owns 1, 1, 1 x 2 or 2 x 4 blocks of G (16 to 128 accumulator registers),
//      which stay in registers across all tiles of the workgroup; the column sums of R are the first C threads'
// Blocks of Z and G that lie wholly in the padding are skipped.  Waves 1 / 4 / 8 / 8, rows of a tile 32 / 64 / 64 / 32,
// LDS 2 R (CP + 2) floats + 20 R bytes: 8.9 / 34 / 67 / 66 KB, so two workgroups of the wide forms share a compute unit.
//
// The wave-per-row form (affcal_vector_kernel; vector, C <= 4096): there is no matrix product in z_k = w_k u_k + b_k, so a
// wave holds a row in registers (lane l: classes l, l + 64, ...), w and b in LDS; maximum and sum first, then the residual
// r_k = q_k - [k = y], added into per-lane column sums of r_k u_k and r_k that live in registers across the wave's rows.  The
// waves of a workgroup add theirs in wave order through LDS.
//
// Either form leaves per-workgroup partials in the workspace (n, sum nll in f64; the gradient sums in f32), and
// affcal_final_kernel adds them in workgroup order in f64: no floating-point atomics, the grid and the tile-to-workgroup map
// depend on (N, C) alone, the same inputs give the same bits.
#include "common.hpp"
#include "elem.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr float kLogFltMin = -87.336544750553109f;
constexpr int kVector = RUNIA_AFFCAL_KIND_VECTOR, kDirichlet = RUNIA_AFFCAL_KIND_DIRICHLET;

struct Labels {
  const void* p;  // int32 or int64 [N]; NULL: no labels (pred, conf, log q only)
  int is_i64, has_ignore;
  int64_t ignore;
};

struct RowOut {
  int32_t* pred;
  float *conf, *nll, *brier, *logq;
};

struct Args {
  const void* x;
  int64_t row_stride, N;
  int C, dirichlet;
  Labels L;
  const float *W, *b;
  RowOut o;
  double* head;  // [blocks][2]: n_used, sum nll; NULL: no record (no gradient work)
  float* part;   // [blocks][slots]
};

// the class whose z the row needs (0 for a row without one) and whether the row is scored against a label
__device__ __forceinline__ int row_class(const Labels& L, int64_t row, int64_t C, bool& used) {
  used = false;
  if (!L.p) return 0;
  const int64_t y = L.is_i64 ? static_cast<const int64_t*>(L.p)[row] : (int64_t) static_cast<const int32_t*>(L.p)[row];
  used = y >= 0 && y < C && !(L.has_ignore && y == L.ignore);
  return used ? (int)y : 0;
}

__device__ __forceinline__ void write_row(const RowOut& o, int64_t row, int bi, float conf, float nll, float brier,
                                          bool labelled, bool used) {
  const float nan = __builtin_nanf("");
  if (o.pred) o.pred[row] = (bi == kNoIndex) ? 0 : bi;
  if (o.conf) o.conf[row] = (!labelled || used) ? conf : nan;
  if (o.nll) o.nll[row] = used ? nll : nan;
  if (o.brier) o.brier[row] = used ? brier : nan;
}

// ---- the matrix-core form ------------------------------------------------------------------------------------------------
template <int CP>
struct Plan {
  static constexpr int NT = CP / 32;                      // 32-class blocks per side
  static constexpr int W = NT * NT < 8 ? NT * NT : 8;     // waves: 1, 4, 8, 8
  static constexpr int R = 32 * W / NT;                   // rows of a tile: every wave owns one 32 x 32 block of Z (32, 64, 64, 32)
  static constexpr int SI = CP == 256 ? 2 : 1;            // a wave owns SI x SJ blocks of G: 1 x 1, 1 x 1, 1 x 2, 2 x 4
  static constexpr int SJ = NT * NT / (W * SI);
  static constexpr int NB = NT / SJ;                      // wave -> (w / NB, w % NB) of those groups
  static constexpr int P = CP + 2;                        // row pitch of both tiles (8-byte reads of two k)
  static constexpr int TPR = 64 * W / R;                  // lanes per row of the softmax step: 2, 4, 8, 16 (16 classes each)
  static constexpr int CPT = CP / TPR;
  static constexpr int NL = CP < 64 ? 1 : CP / 64;        // loads per lane of a widened row
  static constexpr int CAP = CP == 32 ? 1024 : (CP == 64 ? 512 : 256);  // workgroups (a partial is up to 257 KB)
  static constexpr size_t LDS = (size_t)2 * R * P * sizeof(float) + (size_t)R * (2 * sizeof(double) + sizeof(int));
  static_assert(CPT == 16 && R * TPR == 64 * W && SJ * NB == NT && SI * (W / NB) == NT, "the plan");
};

template <class T, int CP>
__global__ __launch_bounds__(64 * Plan<CP>::W) void affcal_full_kernel(Args a) {
  using PL = Plan<CP>;
  constexpr int R = PL::R, P = PL::P, W = PL::W, SI = PL::SI, SJ = PL::SJ, TPR = PL::TPR;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Us = lds;
  float* Zs = lds + R * P;
  double* dsum = reinterpret_cast<double*>(Zs + R * P);  // [2][R]
  int* bad = reinterpret_cast<int*>(dsum + 2 * R);       // [R]
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.C;
  const typename T::elem* x = static_cast<const typename T::elem*>(a.x);
  const int64_t tiles = (a.N + R - 1) / R;
  const bool grad = a.head != nullptr;
  const int gi = SI * (wave / PL::NB), gj = SJ * (wave % PL::NB);  // first block of the wave's SI x SJ group of G
  const bool g_live = grad && 32 * gi < C && 32 * gj < C;
  const int zr = wave / PL::NT, zc = wave % PL::NT;  // block of Z
  const int srow = tid / TPR, sub = tid % TPR;       // softmax step: row of the tile, lane of the row

  f32x16 acc[SI][SJ];
#pragma unroll
  for (int p = 0; p < SI; ++p)
#pragma unroll
    for (int q = 0; q < SJ; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[p][q][r] = 0.f;
  float db = 0.f;
  double nll_sum = 0.0, n_sum = 0.0;

  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * R;
    // A: rows into LDS
    for (int r = wave; r < R; r += W) {
      const int64_t row = r0 + r;
      const bool in = row < a.N;
      const typename T::elem* xr = x + (in ? row : 0) * a.row_stride;
      float v[PL::NL];
      bool odd = false;
#pragma unroll
      for (int c = 0; c < PL::NL; ++c) {
        const int col = lane + 64 * c;
        const bool ok = in && col < C;
        v[c] = ok ? ld1<T>(xr + col) : (a.dirichlet ? -INFINITY : 0.f);
        odd |= ok && !(fabsf(v[c]) < INFINITY);
      }
      if (a.dirichlet) {
        float m = v[0];
#pragma unroll
        for (int c = 1; c < PL::NL; ++c) m = fmaxf(m, v[c]);
        m = wave_max_f32(m);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < PL::NL; ++c) s += exp_nonpos(v[c] - m);  // (a NaN logit: NaN; a row of -inf: -inf - -inf)
        const float ls = log_nonneg(wave_sum_f32(s));
#pragma unroll
        for (int c = 0; c < PL::NL; ++c) {
          const float u = (v[c] - m) - ls;
          v[c] = (in && lane + 64 * c < C) ? ((u < kLogFltMin) ? kLogFltMin : u) : 0.f;  // (a NaN stays)
        }
      }
      const bool any_odd = __ballot(odd) != 0;
      if (lane == 0) bad[r] = (!a.dirichlet && any_odd) ? 1 : 0;
#pragma unroll
      for (int c = 0; c < PL::NL; ++c)
        if (lane + 64 * c < CP) Us[r * P + lane + 64 * c] = v[c];
    }
    __syncthreads();
    // B: Z = U W^T + b
    {
      const int j = zc * 32 + li;
      const bool jok = j < C;
      f32x16 z;
#pragma unroll
      for (int r = 0; r < 16; ++r) z[r] = 0.f;
      if (zc * 32 < C) {
        const float* wr = a.W + (size_t)(jok ? j : 0) * C;
        const float* ur = Us + (zr * 32 + li) * P;
        const int kend = (C + 3) & ~3;
        // 32 classes per chain, the chains added in order: the rounding of z grows with 32 + C / 32 terms, not with C (one
        // chain over 255 classes left conf 2.6e-6 from float64 where a blocked f32 product stays below 1e-6)
        for (int kc = 0; kc < kend; kc += 32) {
          f32x16 zc32;
#pragma unroll
          for (int r = 0; r < 16; ++r) zc32[r] = 0.f;
          const int kstop = kc + 32 < kend ? kc + 32 : kend;
          for (int k0 = kc; k0 < kstop; k0 += 4) {
            const int k = k0 + 2 * lh;
            const float2 u2 = *reinterpret_cast<const float2*>(ur + k);
            const float w0 = (jok && k < C) ? wr[k] : 0.f;
            const float w1 = (jok && k + 1 < C) ? wr[k + 1] : 0.f;
            zc32 = __builtin_amdgcn_mfma_f32_32x32x2f32(u2.x, w0, zc32, 0, 0, 0);
            zc32 = __builtin_amdgcn_mfma_f32_32x32x2f32(u2.y, w1, zc32, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) z[r] += zc32[r];
        }
      }
      const float bj = jok ? a.b[j] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {  // C[row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][col = lane & 31]
        const int row = zr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        Zs[row * P + j] = jok ? z[r] + bj : -INFINITY;
      }
    }
    __syncthreads();
    // C: the row softmax; Z becomes R = Q - onehot
    {
      const int64_t row = r0 + srow;
      const bool in = row < a.N;
      float* zrow = Zs + srow * P;
      float z[PL::CPT];
      float m = -INFINITY;
      int bi = kNoIndex;
#pragma unroll
      for (int i = 0; i < PL::CPT; ++i) {
        z[i] = zrow[sub + TPR * i];
        best_take(m, bi, z[i], sub + TPR * i);
      }
#pragma unroll
      for (int o = TPR / 2; o > 0; o >>= 1) {
        const float v = lane_xor(m, o);
        const int i = lane_xor(bi, o);
        best_take(m, bi, v, i);
      }
      bool used = false;
      const int y = in ? row_class(a.L, row, C, used) : 0;
      float s = 0.f, zy = -INFINITY;
#pragma unroll
      for (int i = 0; i < PL::CPT; ++i) {
        zy = (sub + TPR * i == y) ? z[i] : zy;
        z[i] = z[i] - m;
        s += (z[i] == -INFINITY) ? 0.f : exp_nonpos(z[i]);
      }
      s = wave_sum<TPR>(s);
      zy = wave_reduce<TPR>(zy, [](float p, float q) { return fmaxf(p, q); });
      if (bad[srow]) s = __builtin_nanf("");
      const float rs = 1.f / s, ls = log_nonneg(s);
      float q2 = 0.f;
#pragma unroll
      for (int i = 0; i < PL::CPT; ++i) {
        const int col = sub + TPR * i;
        const float e = (z[i] == -INFINITY) ? 0.f : exp_nonpos(z[i]);
        const float q = div_by_rcp(e, s, rs);
        q2 += q * q;
        zrow[col] = used ? q - (col == y ? 1.f : 0.f) : 0.f;
        if (!used) Us[srow * P + col] = 0.f;
        if (a.o.logq && in && col < C) a.o.logq[row * C + col] = z[i] - ls;
      }
      q2 = wave_sum<TPR>(q2);
      if (sub == 0 && in) {
        const float nll = ls - (zy - m);
        const float qy = div_by_rcp(exp_nonpos(zy - m), s, rs);
        write_row(a.o, row, bi, rs, nll, q2 - 2.f * qy + 1.f, a.L.p != nullptr, used);
        if (used) {
          nll_sum += (double)nll;
          n_sum += 1.0;
        }
      }
    }
    __syncthreads();
    // D: G += R^T U, db += column sums of R
    if (g_live) {
      for (int k0 = 0; k0 < R; k0 += 2) {
        const float* rr = Zs + (k0 + lh) * P + 32 * gi + li;
        const float* ur = Us + (k0 + lh) * P + 32 * gj + li;
        float rv[SI], uv[SJ];
#pragma unroll
        for (int p = 0; p < SI; ++p) rv[p] = rr[32 * p];
#pragma unroll
        for (int q = 0; q < SJ; ++q) uv[q] = ur[32 * q];
#pragma unroll
        for (int p = 0; p < SI; ++p)
#pragma unroll
          for (int q = 0; q < SJ; ++q)
            if (32 * (gi + p) < C && 32 * (gj + q) < C)  // (wave-uniform: a block in the padding stays zero)
              acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(rv[p], uv[q], acc[p][q], 0, 0, 0);
      }
    }
    if (grad && tid < C) {
      for (int r = 0; r < R; ++r) db += Zs[r * P + tid];
    }
    __syncthreads();
  }
  if (!grad) return;
  // the workgroup's partials
  if (sub == 0) {
    dsum[srow] = n_sum;
    dsum[R + srow] = nll_sum;
  }
  __syncthreads();
  if (tid < 2) {
    double v = 0.0;
    for (int r = 0; r < R; ++r) v += dsum[tid * R + r];
    a.head[(size_t)blockIdx.x * 2 + tid] = v;
  }
  float* part = a.part + (size_t)blockIdx.x * ((size_t)C * C + C);
  if (g_live) {
#pragma unroll
    for (int p = 0; p < SI; ++p)
#pragma unroll
      for (int q = 0; q < SJ; ++q) {
        const int j = 32 * (gj + q) + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 32 * (gi + p) + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (i < C && j < C) part[(size_t)i * C + j] = acc[p][q][r];
        }
      }
  }
  if (tid < C) part[(size_t)C * C + tid] = db;
}

// ---- the wave-per-row form -----------------------------------------------------------------------------------------------
constexpr int kVecWaves = 4;
static inline int vector_nc(int64_t C) { return C <= 64 ? 1 : (C <= 256 ? 4 : (C <= 1024 ? 16 : 64)); }
static inline int64_t vector_cap(int nc) { return nc <= 4 ? 1024 : (nc == 16 ? 512 : 256); }

template <class T, int NC>
__global__ __launch_bounds__(64 * kVecWaves) void affcal_vector_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) float wb[];  // w [C] | b [C]; at the end the workgroup's sums
  __shared__ double dsum[2][kVecWaves];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.C;
  const typename T::elem* x = static_cast<const typename T::elem*>(a.x);
  const bool grad = a.head != nullptr;
  for (int i = tid; i < C; i += 64 * kVecWaves) {
    wb[i] = a.W[i];
    wb[C + i] = a.b[i];
  }
  __syncthreads();
  float gw[NC], gb[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) gw[c] = gb[c] = 0.f;
  double nll_sum = 0.0, n_sum = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * kVecWaves + wave; row < a.N; row += (int64_t)gridDim.x * kVecWaves) {
    const typename T::elem* xr = x + row * a.row_stride;
    float u[NC];
    bool odd = false;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = lane + 64 * c;
      u[c] = col < C ? ld1<T>(xr + col) : 0.f;
      odd |= !(fabsf(u[c]) < INFINITY);
    }
    const bool any_odd = __ballot(odd) != 0;
    bool used;
    const int y = row_class(a.L, row, C, used);
    float m = -INFINITY;
    int bi = kNoIndex;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = lane + 64 * c;
      if (col < C) best_take(m, bi, fmaf(wb[col], u[c], wb[C + col]), col);
    }
    wave_best(m, bi);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = lane + 64 * c;
      if (col < C) {
        const float d = fmaf(wb[col], u[c], wb[C + col]) - m;
        s += (d == -INFINITY) ? 0.f : exp_nonpos(d);
      }
    }
    s = any_odd ? __builtin_nanf("") : wave_sum_f32(s);
    const float rs = 1.f / s, ls = log_nonneg(s);
    float q2 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = lane + 64 * c;
      if (col < C) {
        const float d = fmaf(wb[col], u[c], wb[C + col]) - m;
        const float q = div_by_rcp((d == -INFINITY) ? 0.f : exp_nonpos(d), s, rs);
        q2 += q * q;
        if (used && grad) {
          const float r = q - (col == y ? 1.f : 0.f);
          gw[c] += r * u[c];
          gb[c] += r;
        }
        if (a.o.logq) a.o.logq[row * C + col] = d - ls;
      }
    }
    q2 = wave_sum_f32(q2);
    if (lane == 0) {
      const float dy = fmaf(wb[y], ld1<T>(xr + y), wb[C + y]) - m;
      const float nll = ls - dy;
      const float qy = div_by_rcp((dy == -INFINITY) ? 0.f : exp_nonpos(dy), s, rs);
      write_row(a.o, row, bi, rs, nll, q2 - 2.f * qy + 1.f, a.L.p != nullptr, used);
      if (used) {
        nll_sum += (double)nll;
        n_sum += 1.0;
      }
    }
  }
  if (!grad) return;
  if (lane == 0) {
    dsum[0][wave] = n_sum;
    dsum[1][wave] = nll_sum;
  }
  __syncthreads();  // (w and b are no longer read)
  for (int w = 0; w < kVecWaves; ++w) {  // the waves' column sums, in wave order
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = lane + 64 * c;
        if (col < C) {
          wb[col] = (w == 0) ? gw[c] : wb[col] + gw[c];
          wb[C + col] = (w == 0) ? gb[c] : wb[C + col] + gb[c];
        }
      }
    }
    __syncthreads();
  }
  if (tid < 2) {
    double v = 0.0;
    for (int w = 0; w < kVecWaves; ++w) v += dsum[tid][w];
    a.head[(size_t)blockIdx.x * 2 + tid] = v;
  }
  float* part = a.part + (size_t)blockIdx.x * 2 * C;
  for (int i = tid; i < 2 * C; i += 64 * kVecWaves) part[i] = wb[i];
}

// ---- the ordered add: one thread per slot of the record, the workgroups' partials in order ----------------------------------
__global__ __launch_bounds__(256) void affcal_final_kernel(const double* __restrict__ head, const float* __restrict__ part,
                                                           int64_t blocks, int64_t slots, double* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= 2 + slots) return;
  double v = 0.0;
  if (s < 2) {
    for (int64_t b = 0; b < blocks; ++b) v += head[b * 2 + s];
  } else {
    for (int64_t b = 0; b < blocks; ++b) v += (double)part[b * slots + (s - 2)];
  }
  out[s] = v;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static inline int full_cp(int64_t C) { return C <= 32 ? 32 : (C <= 64 ? 64 : (C <= 128 ? 128 : 256)); }

static inline bool shape_ok(int64_t N, int64_t C, int kind) {
  if (N < 0 || C < 1 || kind < kVector || kind > kDirichlet) return false;
  return C <= (kind == kVector ? RUNIA_AFFCAL_MAX_VECTOR : RUNIA_AFFCAL_MAX_FULL);
}

// rows that the workgroups' first trip covers
static inline int64_t round_rows(int64_t C, int kind) {
  if (kind == kVector) return vector_cap(vector_nc(C)) * kVecWaves;
  switch (full_cp(C)) {
    case 32: return (int64_t)Plan<32>::CAP * Plan<32>::R;
    case 64: return (int64_t)Plan<64>::CAP * Plan<64>::R;
    case 128: return (int64_t)Plan<128>::CAP * Plan<128>::R;
    default: return (int64_t)Plan<256>::CAP * Plan<256>::R;
  }
}

static inline int64_t plan_blocks(int64_t N, int64_t C, int kind) {
  int64_t per = kVecWaves, cap = 0;
  if (kind == kVector) {
    cap = vector_cap(vector_nc(C));
  } else {
    switch (full_cp(C)) {
      case 32: per = Plan<32>::R, cap = Plan<32>::CAP; break;
      case 64: per = Plan<64>::R, cap = Plan<64>::CAP; break;
      case 128: per = Plan<128>::R, cap = Plan<128>::CAP; break;
      default: per = Plan<256>::R, cap = Plan<256>::CAP; break;
    }
  }
  const int64_t b = (N + per - 1) / per;
  return b < cap ? b : cap;
}

static inline int64_t record_slots(int64_t C, int kind) { return kind == kVector ? 2 * C : C * C + C; }

struct Workspace {
  double* head;
  float* part;
};
static Workspace layout(WsWalk& w, int64_t N, int64_t C, int kind) {
  const int64_t blocks = plan_blocks(N, C, kind);
  Workspace ws;
  ws.head = w.take<double>((size_t)blocks * 2);
  ws.part = w.take<float>((size_t)blocks * record_slots(C, kind));
  return ws;
}

template <class T, int CP>
int launch_full(const Args& a, unsigned grid, hipStream_t s) {
  static std::atomic<uint64_t> lds_ok{0};
  if (int rc = runia_allow_dynamic_lds(reinterpret_cast<const void*>(affcal_full_kernel<T, CP>), 160 * 1024, lds_ok)) return rc;
  affcal_full_kernel<T, CP><<<grid, 64 * Plan<CP>::W, Plan<CP>::LDS, s>>>(a);
  return runia_check_launch();
}

template <class T>
int launch_eval(const Args& a, int kind, unsigned grid, hipStream_t s) {
  if (kind == kVector) {
    const size_t lds = (size_t)2 * a.C * sizeof(float);
    switch (vector_nc(a.C)) {
      case 1: affcal_vector_kernel<T, 1><<<grid, 64 * kVecWaves, lds, s>>>(a); break;
      case 4: affcal_vector_kernel<T, 4><<<grid, 64 * kVecWaves, lds, s>>>(a); break;
      case 16: affcal_vector_kernel<T, 16><<<grid, 64 * kVecWaves, lds, s>>>(a); break;
      default: affcal_vector_kernel<T, 64><<<grid, 64 * kVecWaves, lds, s>>>(a); break;
    }
    return runia_check_launch();
  }
  switch (full_cp(a.C)) {
    case 32: return launch_full<T, 32>(a, grid, s);
    case 64: return launch_full<T, 64>(a, grid, s);
    case 128: return launch_full<T, 128>(a, grid, s);
    default: return launch_full<T, 256>(a, grid, s);
  }
}

}  // namespace

extern "C" int64_t runia_affcal_round_rows(int64_t C, int kind) { return shape_ok(0, C, kind) ? round_rows(C, kind) : 0; }

extern "C" int64_t runia_affcal_workspace_bytes(int64_t N, int64_t C, int kind) {
  if (!shape_ok(N, C, kind) || N == 0) return 0;
  return (int64_t)ws_bytes([&](WsWalk& w) { layout(w, N, C, kind); });
}

extern "C" int runia_affcal_eval(const void* logits, int dtype, int64_t row_stride, const void* labels, int labels_i64,
                                 int has_ignore, int64_t ignore_index, int kind, const float* W, const float* b, void* record,
                                 int32_t* pred, float* conf, float* nll, float* brier, float* logq, int64_t N, int64_t C,
                                 void* workspace, size_t workspace_bytes, runia_stream_t stream) {
  if (!elem_dtype_ok(dtype) || !shape_ok(N, C, kind) || row_stride < C || !W || !b) return RUNIA_E_INVALID;
  if (!record && !pred && !conf && !nll && !brier && !logq) return RUNIA_E_INVALID;
  hipStream_t s = as_stream(stream);
  const int64_t slots = record_slots(C, kind);
  const unsigned final_grid = (unsigned)((2 + slots + 255) / 256);
  if (N == 0) {
    if (record) affcal_final_kernel<<<final_grid, 256, 0, s>>>(nullptr, nullptr, 0, slots, static_cast<double*>(record));
    return runia_check_launch();
  }
  if (!logits || (!labels && (record || nll || brier))) return RUNIA_E_INVALID;
  Workspace ws = {nullptr, nullptr};
  if (record) {
    if (ws_refused(workspace, workspace_bytes, (size_t)runia_affcal_workspace_bytes(N, C, kind), 8)) return RUNIA_E_WORKSPACE;
    WsWalk w(workspace);
    ws = layout(w, N, C, kind);
  }
  const Args a = {logits, row_stride, N, (int)C, kind == kDirichlet, {labels, labels_i64 != 0, has_ignore != 0, ignore_index},
                  W, b, {pred, conf, nll, brier, logq}, ws.head, ws.part};
  const int64_t blocks = plan_blocks(N, C, kind);
  const int rc = dispatch_elem(dtype, [&](auto tag) { return launch_eval<decltype(tag)>(a, kind, (unsigned)blocks, s); });
  if (rc != RUNIA_OK || !record) return rc;
  affcal_final_kernel<<<final_grid, 256, 0, s>>>(ws.head, ws.part, blocks, slots, static_cast<double*>(record));
  return runia_check_launch();
}
