// K2 / K2' of the fused LaREM row pipeline: the score launches behind K1 (the pipeline: head of mc_sampler.hip).
#include "common.hpp"
#include "mfma_f64_tile.hpp"
#include "trap_order.hpp"

namespace {
using namespace runia_mfma;

// ------------------------------------------------------------------------------------------
// K2: H -> PCA (optional) -> LaREM score.  One workgroup = BM rows; both contractions on f64 MFMA.
// Packed weights layout: see gemm_f64.hip.
// ------------------------------------------------------------------------------------------
struct PcaMdArgs {
  const double* h;         // [N, D]
  const double* packed_ct; // pack(C.T [D, n]) or null (no PCA: n == D)
  const double* bias;      // [n]
  const double* scale;     // [n] or null
  const double* md_mean;   // [n]
  const double* packed_p;  // pack(P [n, n])
  double* score;           // [N]
  double* y_out;           // optional [N, n]: the projected rows (tests)
  int64_t N, D, n;
};

template <int RT>  // row tiles of 16 per workgroup (BM = 16*RT)
__global__ __launch_bounds__(256) void pca_md_kernel(PcaMdArgs g) {
  constexpr int BM = 16 * RT;
  extern __shared__ double lds[];
  // layout: lds_a [2][BM][APITCH] | lds_y [BM][ypitch] | part [4][BM]
  const int64_t n_pad = n_padded(g.n);
  const int ypitch = (int)n_pad + 2;  // == 2 mod 32 -> conflict-free A-fragment reads
  double* lds_a = lds;
  double* lds_y = lds + 2 * BM * APITCH;
  double* part = lds_y + (size_t)BM * ypitch;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int64_t NT = n_pad / 16;
  const int64_t r0 = (int64_t)blockIdx.x * BM;

  // ---------------- phase A: d = (H C^T - bias) / scale - md_mean  -> lds_y ----------------
  if (g.packed_ct) {
    const int64_t nchunks = k_padded(g.D) / KC;
    constexpr int PER_T = BM * KC / 256;  // doubles staged per thread per chunk (4 or 2)
    for (int64_t cb = 0; cb < n_pad / BN; ++cb) {
      const int64_t ctbase = cb * 16 + wave * 4;
      d4 acc[RT][4];
#pragma unroll
      for (int a = 0; a < RT; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = (d4){0.0, 0.0, 0.0, 0.0};
      const double2* bp = reinterpret_cast<const double2*>(g.packed_ct) + ctbase * 64 + lane;
      double2 b0[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) b0[c] = bp[c * 64];
      double areg[PER_T];
      const int srow = (tid * PER_T) / KC, skk = (tid * PER_T) % KC;
      auto load_a = [&](int64_t kc) {
        const int64_t gr = r0 + srow;
#pragma unroll
        for (int q = 0; q < PER_T; ++q) {
          const int64_t gk = kc + skk + q;
          areg[q] = (gr < g.N && gk < g.D) ? g.h[gr * g.D + gk] : 0.0;
        }
      };
      load_a(0);
      int buf = 0;
      for (int64_t ch = 0; ch < nchunks; ++ch) {
#pragma unroll
        for (int q = 0; q < PER_T; ++q) lds_a[(buf * BM + srow) * APITCH + skk + q] = areg[q];
        __syncthreads();
        if (ch + 1 < nchunks) load_a((ch + 1) * KC);
        mfma_chunk<RT>(acc, lds_a + buf * BM * APITCH, APITCH, li, lg, bp + ch * 4 * NT * 64, NT * 64, b0);
        buf ^= 1;
      }
      // epilogue: sklearn transform then the LaREM centring, kept in LDS
#pragma unroll
      for (int a = 0; a < RT; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int64_t col = (ctbase + c) * 16 + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * a + lg + 4 * r;
            double d = 0.0;
            if (col < g.n) {
              double y = acc[a][c][r] - g.bias[col];
              if (g.scale) y = y / g.scale[col];
              if (g.y_out && r0 + row < g.N) g.y_out[(r0 + row) * g.n + col] = y;
              d = y - g.md_mean[col];
            }
            lds_y[row * ypitch + col] = d;  // zero padding beyond n keeps phase B exact
          }
        }
      __syncthreads();
    }
  } else {
    // no PCA: d = h - md_mean straight into lds_y (n == D)
    for (int i = tid; i < BM * (int)n_pad; i += 256) {
      const int row = i / (int)n_pad, col = i - row * (int)n_pad;
      double d = 0.0;
      if (r0 + row < g.N && col < g.n) d = g.h[(r0 + row) * g.D + col] - g.md_mean[col];
      lds_y[row * ypitch + col] = d;
    }
    __syncthreads();
  }

  // ---------------- phase B: score = -sum_j (d P)_j d_j, A fragments straight from lds_y ------
  double rowdot[RT][4];
#pragma unroll
  for (int a = 0; a < RT; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) rowdot[a][r] = 0.0;
  const int64_t kchunks = k_padded(g.n) / KC;
  for (int64_t cb = 0; cb < n_pad / BN; ++cb) {
    const int64_t ctbase = cb * 16 + wave * 4;
    d4 acc[RT][4];
#pragma unroll
    for (int a = 0; a < RT; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = (d4){0.0, 0.0, 0.0, 0.0};
    const double2* bp = reinterpret_cast<const double2*>(g.packed_p) + ctbase * 64 + lane;
    double2 b0[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) b0[c] = bp[c * 64];
    for (int64_t ch = 0; ch < kchunks; ++ch)
      mfma_chunk<RT>(acc, lds_y + ch * KC, ypitch, li, lg, bp + ch * 4 * NT * 64, NT * 64, b0);
#pragma unroll
    for (int a = 0; a < RT; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = (int)((ctbase + c) * 16) + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) rowdot[a][r] += acc[a][c][r] * lds_y[(16 * a + lg + 4 * r) * ypitch + col];
      }
  }
#pragma unroll
  for (int a = 0; a < RT; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = rowdot[a][r];
      v += shfl_xor_f64(v, 1);
      v += shfl_xor_f64(v, 2);
      v += shfl_xor_f64(v, 4);
      v += shfl_xor_f64(v, 8);
      if (li == 0) part[wave * BM + 16 * a + lg + 4 * r] = v;
    }
  __syncthreads();
  if (tid < BM) {
    const int64_t row = r0 + tid;
    if (row < g.N) g.score[row] = -(((part[tid] + part[BM + tid]) + part[2 * BM + tid]) + part[3 * BM + tid]);
  }
}

// ------------------------------------------------------------------------------------------
// K2': the same score as K2 from ONE contraction.  With d = A h + b (A = diag(1/scale) C, b = -bias/scale - mu) and
// P = W^T W (W = diag(1/sqrt(s)) U^T over the eigenpairs pinvh kept),  -d^T P d = -|| (W A) h + W b ||^2, so the
// 512->256 projection, the whitening, the centring and the 256x256 quadratic form collapse into M = W A (r x D) and
// c = W b, folded once at setup.  2*D*r FLOP per row instead of 2*D*n + 2*n^2; no LDS round trip for the projection.
// ------------------------------------------------------------------------------------------
struct ProjSqArgs {
  const double* h;        // [N, D]
  const double* packed_m; // pack(M^T [D, r])
  const double* c;        // [r]
  double* score;          // [N]            (column split 1)
  double* partial;        // [2, N] row sums (column split 2; proj_sq_combine_kernel finishes)
  int64_t N, D, r;
};

// NCT column tiles per wave: 4 = the workgroup covers every 256-column block whole (grid.y = 1); 2 = two
// workgroups share a row tile, each taking one 128-column half of every block (grid.y = 2) and leaving its row
// sums of squares in `partial`.  The split halves the unit of work: at N = 10 000 the 625 row tiles are 2.44 per
// CU (3 on some, 2 on most: 19 % of the matrix pipes idle at the end); 1250 half tiles finish within 3 %.
// Few components (the reference's default is nro_components = 16): SPLIT = false with NCT = 1 covers r <= 64 (each wave
// one 16-column tile), with NCT = 2 r <= 128 - the zero-padded column tiles beyond r are simply not computed (the
// 256-column forms spend the same 45-50 us on r = 16 as on r = 256).
// 16-row forms: 96 vector registers = 5 waves per SIMD, so the 1 250 workgroups of 10 000 rows are all resident at once
// (98 registers = 4 waves left 226 workgroups for a second, thinly occupied round: 45.5 -> 44.5 us)
#ifndef K2_WAVES
#define K2_WAVES 5
#endif
#ifndef K2_DMA
#define K2_DMA 1
#endif
#ifndef K2_WAVES_DMA
#define K2_WAVES_DMA 5  // (the DMA form needs 74 vector registers, but 6 waves per SIMD measured 2 % slower than 5)
#endif
// TRAP: the caller promises an upper-trapezoidal M (M[j][k] = 0 for k < j; runia_qr_trapezoid_f64 makes one at setup: the
// score does not change under an orthogonal factor from the left).  Column tile t of M^T then holds only zeros in its
// rows k < 16 t, and the products with them are 0.0 * h: adding them changes nothing for finite h, so the K loop may start
// behind them.  With r = 256, D = 512 and the column split, the wave that owns 32-column group q = 0..7 can skip q of the
// 16 chunks: 100 of 128 chunk-waves are left, 0.78 of the matrix instructions and weight-fragment loads (the parameter
// count of a rank-256 form on 512 dimensions allows 0.75).  Column tile 0 skips nothing, so a row with a NaN h still
// scores NaN, and a row with an infinite h never scores a finite value (NaN like the dense form wherever a computed
// column meets the infinity with a zero; -inf instead of NaN only for +-inf exactly at k = 32 q - 1 under TRAP = 2).
//   TRAP = 0  dense: the code of the plain entry points, unchanged
//   TRAP = 1  workgroup-uniform skip: the chunk loop of a workgroup starts at the first chunk in which any of its columns
//             is non-zero (chunk 4 for column half 1 of the case above: 0.875 of the work; nothing for the unsplit forms
//             below 256 columns); DMA prologue and B ring start there
//   TRAP = 2  per-wave skip (16-row DMA forms; the others fall back to TRAP = 1): below its own first live chunk a wave
//             only issues its share of the row DMA and joins the barrier.  Which wave owns which 32-column group rotates
//             between the workgroups that share a CU (`grp`) - the four waves of a workgroup sit on the four SIMDs of a CU, and with a fixed assignment
//             the SIMD of the wave that skips least would set the pace; `part` is indexed by group, so the summation
//             order below is the documented one whichever wave computed a group.
#ifndef K2_TRAP_FORM
#define K2_TRAP_FORM 2  // the form behind runia_proj_sq_*_trap_f64
#endif
// K2_TRAP_ROT: how the owner of a column group rotates under TRAP = 2.  Workgroup ids go round-robin over the 8 XCDs
// (bits 0-2), so `tile & 3` (= id & 3) is one value per XCD and rotates nothing inside a CU; which higher bits separate
// the workgroups of one CU is the dispatcher's business.  Measured, accumulate form, N = 10 000, trap / dense: id bits
// 4-5 + 8-9 0.958, bits 8-9 alone 0.964 (one session); `tile & 3` 0.933 in an earlier session on its own - not
// compared side by side, and none near the 0.78 of the instruction count: SIMD balance is not what holds the kernel back.
#ifndef K2_TRAP_ROT
#define K2_TRAP_ROT 2  // 0 none, 1 tile & 3, 2 id bits 4-5 + 8-9, 3 id bits 8-9
#endif
//   TRAP = 3  TRAP = 2 for an R whose 32-row blocks stand in the balanced order of trap_order.hpp (runia_trap_balance_rows_f64;
//             the runia_proj_sq_*_btrap_f64 entry points): a group's first live chunk comes from trap_balanced_first_k
//             instead of its own position, the workgroup's start is the minimum over its groups.  Both column halves then
//             keep 50 of their 64 chunk-waves (58 and 42 under TRAP = 2) - and both run 16 and 15 chunk STEPS (row DMA +
//             barrier, paid by all four waves) where TRAP = 2 runs 16 and 12.  Measured, the steps are what costs: 40.15 us
//             against 40.33 (TRAP = 2) and 41.56 (dense) at N = 10 000, nothing in the step.  Not the pipeline's default.
// K2_TRAP_HALFMAP: which of the two ids of a row tile (i, i ^ 8: same XCD, one dispatch round apart) takes which column
// half.  0: half = bit 0 of j = id >> 3, the index of the workgroup inside its XCD.  A dispatcher that deals an XCD's
// workgroups round-robin over its 32 CUs then gives every CU workgroups of ONE half only, and under TRAP the half-0 CUs
// (16 chunk steps, 58 of 64 chunk-waves) set the kernel's time while the half-1 CUs (12 steps, 42 of 64) idle at the end.
// 1: the halves swap in every second group of 32 dispatch rounds, so a CU holds both kinds.  Measured at N = 10 000,
// accumulate form, trap / dense: 0.970 with 0, 0.889 with 1 (36.97 us); dense itself does not move (41.56 / 41.61).  The
// mapping only changes which workgroup computes which half - never a bit of the result - and where workgroups land is the
// dispatcher's business: on another placement it is worth what 0 is worth.  (profiles/README.md, "K2' column halves per CU")
#ifndef K2_TRAP_HALFMAP
#define K2_TRAP_HALFMAP 1
#endif
template <int RT, int NCT, bool ACCUMULATE, bool SPLIT, bool DMA, int TRAP = 0>
__global__ __launch_bounds__(256, (RT == 1 && NCT <= 2) ? (DMA ? K2_WAVES_DMA : K2_WAVES) : 1) void proj_sq_kernel(ProjSqArgs g) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass only needs the launch stub; the body uses device-only buffer builtins)
  constexpr int BM = 16 * RT;
  constexpr bool WAVE_SKIP = TRAP >= 2 && DMA && RT == 1;
  __shared__ double lds_a[DMA ? 1 : 2 * BM * APITCH];
  // the DMA form's two chunk buffers are separate objects: the compiler orders a ds_read behind every LDS DMA it cannot
  // prove disjoint (one array: `s_waitcnt vmcnt(0)` in front of each chunk's first read, the DMA of the NEXT chunk included)
  __shared__ __attribute__((aligned(16))) double lds_d0[DMA ? BM * KC : 2];
  __shared__ __attribute__((aligned(16))) double lds_d1[DMA ? BM * KC : 2];
  constexpr int NG = (NCT + 1) / 2;  // 32-column groups per wave: the unit of the (launch-independent) summation order
  __shared__ double part[4 * NG * BM];
  const int64_t n_pad = n_padded(g.r);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int64_t NT = n_pad / 16;
  // Column split (NCT == 2): a 1-D grid whose ids i and i + 8 are the two column halves of one row tile.  Consecutive
  // workgroup ids go round-robin over the 8 XCDs, so the two halves run on the SAME XCD one dispatch round apart and the
  // second one finds the row tile in that XCD's L2 (with a (tile, half) 2-D grid they sat 625 ids apart: both read the
  // tile from HBM, 90.9 MB fetched for 42 MB of rows).
  int64_t tile = blockIdx.x;
  int half = 0;
  if constexpr (SPLIT) {
    tile = (int64_t)(blockIdx.x >> 4) * 8 + (blockIdx.x & 7);
    const unsigned j = blockIdx.x >> 3;
    half = (int)((K2_TRAP_HALFMAP ? j ^ (j >> 5) : j) & 1);
    if (tile * BM >= g.N) return;  // padding of the last group of 8 tiles (uniform over the workgroup)
  }
  const int64_t r0 = tile * BM;
  const int nchunks = (int)(k_padded(g.D) / KC);
  // The 32 * NG-column group of every block this wave owns; under WAVE_SKIP the owner rotates from workgroup to workgroup
  // (K2_TRAP_ROT, measured above).
  const int rot = K2_TRAP_ROT == 1 ? (int)(tile & 3)
                  : K2_TRAP_ROT == 2 ? (int)(((blockIdx.x >> 4) + (blockIdx.x >> 8)) & 3)
                  : K2_TRAP_ROT == 3 ? (int)((blockIdx.x >> 8) & 3) : 0;
  const int grp = WAVE_SKIP ? (wave + rot) & 3 : wave;
  constexpr int PER_T = BM * KC / 256;
  double rowsq[NG][RT][4];
#pragma unroll
  for (int q = 0; q < NG; ++q)
#pragma unroll
    for (int a = 0; a < RT; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) rowsq[q][a][r] = 0.0;
  for (int64_t cb = 0; cb < n_pad / BN; ++cb) {
    const int64_t ctbase = cb * 16 + (int64_t)half * (4 * NCT) + grp * NCT;
    // first chunk with a non-zero column of this workgroup (ch0) and of this wave (ws); never past the last chunk, so the
    // row DMA stays inside the rows (all-zero padding columns beyond r just run that one chunk)
    int64_t wg_chunk = (cb * 16 + (int64_t)half * (4 * NCT)) * 16 / KC, wave_chunk = ctbase * 16 / KC;
    if constexpr (TRAP == 3) {
      // balanced order: the 2 * NCT groups of this workgroup and the NG groups of this wave, by 32-column position
      const int64_t wg_pos = (cb * 16 + (int64_t)half * (4 * NCT)) / 2, wave_pos = ctbase / 2;
      wg_chunk = trap_balanced_first_k(wg_pos, g.r) / KC;
#pragma unroll
      for (int i = 1; i < 2 * NCT; ++i) {
        const int64_t f = trap_balanced_first_k(wg_pos + i, g.r) / KC;
        wg_chunk = f < wg_chunk ? f : wg_chunk;
      }
      wave_chunk = trap_balanced_first_k(wave_pos, g.r) / KC;
#pragma unroll
      for (int q = 1; q < NG; ++q) {
        const int64_t f = trap_balanced_first_k(wave_pos + q, g.r) / KC;
        wave_chunk = f < wave_chunk ? f : wave_chunk;
      }
    }
    const int ch0 = TRAP ? (int)(wg_chunk < nchunks - 1 ? wg_chunk : nchunks - 1) : 0;
    [[maybe_unused]] const int ws = WAVE_SKIP ? (int)(wave_chunk < nchunks - 1 ? wave_chunk : nchunks - 1) : ch0;
    d4 acc[RT][NCT];
#pragma unroll
    for (int a = 0; a < RT; ++a)
#pragma unroll
      for (int c = 0; c < NCT; ++c) acc[a][c] = (d4){0.0, 0.0, 0.0, 0.0};
    double2 bring[4][NCT];  // B fragments three k-step pairs ahead
    if constexpr (DMA) {
      // DMA form (whole chunks of a matrix below 4 GiB, the usual case; proj_sq_dma_ok): per chunk and wave ONE buffer_load ... lds for
      // the rows (no staging registers, no ds_write), B fragments through a scalar offset, the LDS buffer a compile-time
      // constant (chunks are taken two at a time): the vector ALU issues the matrix instructions and nothing else.
      const __amdgpu_buffer_rsrc_t brsrc = buffer_of(g.packed_m, (unsigned)(packed_elems(g.D, g.r) * 8));
      const int64_t rows_here = (g.N - r0 < BM) ? g.N - r0 : BM;  // rows past N read as zero (range check)
      const __amdgpu_buffer_rsrc_t arsrc = buffer_of(g.h + r0 * g.D, (unsigned)(rows_here * g.D * 8));
      const unsigned lane_bytes = (unsigned)lane * 16u;
      const unsigned pair_stride_bytes = (unsigned)NT * 1024u;
      const unsigned ct_bytes = (unsigned)ctbase * 1024u;
      // DMA instruction j of a chunk fills slots 64j .. 64j+63: slot = kpair * BM + row
      constexpr int NDMA = BM / 4 / 4;  // per wave (BM / 4 instructions per chunk over 4 waves)
      unsigned a_lane_bytes[NDMA];
#pragma unroll
      for (int i = 0; i < NDMA; ++i) {
        const int slot = 64 * (wave + 4 * i) + lane;
        a_lane_bytes[i] = (unsigned)(((slot % BM) * g.D + 2 * (slot / BM)) * 8);
      }
      auto dma_rows = [&](int bufc, int kc) {
#pragma unroll
        for (int i = 0; i < NDMA; ++i)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(
              arsrc, (__attribute__((address_space(3))) void*)((bufc ? lds_d1 : lds_d0) + 128 * (wave + 4 * i)), 16,
              a_lane_bytes[i], (unsigned)kc * 8u, 0, 0);
        asm volatile("" ::: "memory");  // the B loads of the chunk stay behind the DMA in program order (the wait below counts them)
      };
      auto body = [&](auto buf_tag, int ch) {
        constexpr int bufc = decltype(buf_tag)::value;
        // this wave's DMA of chunk ch is older than at least 3 * NCT B loads (four pairs in the loop, three in the prologue):
        // once at most that many loads are outstanding it has landed (loads retire in order); the barrier then publishes
        // all four waves' parts.  The oldest of those B loads is needed by the first matrix instruction anyway.
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * NCT) : "memory");
        __syncthreads();
        // (no branch: the last chunk fetches itself again into the idle buffer - with the DMA under a condition the loop
        // is several basic blocks and the compiler's own wait at their join is vmcnt(0))
        dma_rows(bufc ^ 1, ((ch + 1 < nchunks) ? ch + 1 : ch) * KC);
        mfma_chunk_dma<RT, NCT, BM>(acc, bufc ? lds_d1 : lds_d0, li, lg, brsrc, lane_bytes,
                                    ct_bytes + (unsigned)ch * 4u * pair_stride_bytes, pair_stride_bytes, bring);
      };
      // prologue in the loop's own order - DMA first, then the three ring pairs - so the count in body() holds for chunk 0
      // too (and the compiler's own wait for its DMA -> ds_read dependence merges to the same vmcnt(3 * NCT) at the loop
      // header instead of vmcnt(0))
      dma_rows(0, ch0 * KC);
      int ch = ch0;
      if constexpr (WAVE_SKIP) {
        // chunks below this wave's first live one: its quarter of the rows and the barrier, no B load, no matrix
        // instruction.  No load of this wave is younger than its DMA here, so no count above zero says the DMA has landed:
        // vmcnt(0).  The next DMA goes out behind the barrier like in body(); the last one of this loop (chunk ws) is
        // followed by the ring prologue, so body(ws) finds its DMA older than 3 * NCT B loads again.
        for (; ch < ws; ++ch) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          dma_rows((ch + 1 - ch0) & 1, (ch + 1) * KC);
        }
      }
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < NCT; ++c)
          bring[j][c] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(
                                                        brsrc, lane_bytes + c * 1024u,
                                                        ct_bytes + (unsigned)(4 * ch + j) * pair_stride_bytes, 0));
      if constexpr (WAVE_SKIP) {
        // an odd number of skipped chunks leaves chunk ws in buffer 1
        if ((ch - ch0) & 1) {
          body(std::integral_constant<int, 1>{}, ch);
          ++ch;
        }
      }
      for (; ch + 1 < nchunks; ch += 2) {
        body(std::integral_constant<int, 0>{}, ch);
        body(std::integral_constant<int, 1>{}, ch + 1);
      }
      if (ch < nchunks) body(std::integral_constant<int, 0>{}, ch);
    } else {
      const double2* bp = reinterpret_cast<const double2*>(g.packed_m) + ctbase * 64 + lane + (int64_t)ch0 * 4 * NT * 64;
    #pragma unroll
      for (int j = 0; j < 3; ++j)
  #pragma unroll
        for (int c = 0; c < NCT; ++c) bring[j][c] = bp[j * NT * 64 + c * 64];
      // staging: element q*256 + tid of the BM x KC chunk (a wave covers two 256-byte row segments per pass)
      double areg[PER_T];
      const int srow = tid / KC, skk = tid % KC;  // + 256/KC rows per q
      // interior row tile of a matrix whose width is a whole number of chunks (uniform over the workgroup): plain loads off
      // one running pointer - predicated loads and 64-bit index arithmetic are vector instructions the matrix pipe waits for
      const bool interior = (r0 + BM <= g.N) && (g.D % KC == 0);
      const double* pa = g.h + (r0 + srow) * g.D + skk;
      auto load_a = [&](int64_t kc) {
        if (interior) {
  #pragma unroll
          for (int q = 0; q < PER_T; ++q) areg[q] = pa[(int64_t)q * (256 / KC) * g.D + kc];
          return;
        }
        const int64_t gk = kc + skk;
  #pragma unroll
        for (int q = 0; q < PER_T; ++q) {
          const int64_t gr = r0 + srow + q * (256 / KC);
          areg[q] = (gr < g.N && gk < g.D) ? g.h[gr * g.D + gk] : 0.0;
        }
      };
      load_a((int64_t)ch0 * KC);
      int buf = 0;
      for (int64_t ch = ch0; ch < nchunks; ++ch) {
  #pragma unroll
        for (int q = 0; q < PER_T; ++q) lds_a[(buf * BM + srow + q * (256 / KC)) * APITCH + skk] = areg[q];
        __syncthreads();
        if (ch + 1 < nchunks) load_a((ch + 1) * KC);
        mfma_chunk_ring<RT, NCT>(acc, lds_a + buf * BM * APITCH, APITCH, li, lg, bp + (ch - ch0) * 4 * NT * 64, NT * 64, bring);
        buf ^= 1;
      }
    }
#pragma unroll
    for (int a = 0; a < RT; ++a)
#pragma unroll
      for (int c = 0; c < NCT; ++c) {
        const int64_t col = (ctbase + c) * 16 + li;
        const double cc = (col < g.r) ? g.c[col] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = acc[a][c][r] + cc;  // zero-padded columns contribute 0
          rowsq[c / 2][a][r] = fma(v, v, rowsq[c / 2][a][r]);
        }
      }
    __syncthreads();
  }
  // A row's sum of squares is added up in ONE order whatever the launch shape (so a batch scores the same bits
  // sharded, chunked or whole): 32-column groups g = 0..7 of every 256-column block, each accumulated over the
  // blocks and its 16 lanes, then ((g0+g1)+g2)+g3 and ((g4+g5)+g6)+g7, then the sum of the two halves.
#pragma unroll
  for (int q = 0; q < NG; ++q)
#pragma unroll
    for (int a = 0; a < RT; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double v = rowsq[q][a][r];
        v += shfl_xor_f64(v, 1);
        v += shfl_xor_f64(v, 2);
        v += shfl_xor_f64(v, 4);
        v += shfl_xor_f64(v, 8);
        if (li == 0) part[(grp * NG + q) * BM + 16 * a + lg + 4 * r] = v;
      }
  __syncthreads();
  if (tid < BM) {
    const int64_t row = r0 + tid;
    if (row < g.N) {
      const double lo = ((part[tid] + part[BM + tid]) + part[2 * BM + tid]) + part[3 * BM + tid];
      if constexpr (NCT == 4) {
        const double hi = ((part[4 * BM + tid] + part[5 * BM + tid]) + part[6 * BM + tid]) + part[7 * BM + tid];
        g.score[row] = -(lo + hi);
      } else if constexpr (!SPLIT) {  // this workgroup holds the whole row (r <= 64 * NCT)
        if constexpr (ACCUMULATE) unsafeAtomicAdd(&g.score[row], -lo);
        else g.score[row] = -lo;
      } else if constexpr (ACCUMULATE) {
        // score was zeroed earlier in the stream: two addends per row, and 0 + a + b = 0 + b + a bit for bit
        unsafeAtomicAdd(&g.score[row], -lo);
      } else {
        g.partial[(int64_t)half * g.N + row] = lo;
      }
    }
  }
#endif
}

__global__ void proj_sq_combine_kernel(const double* __restrict__ partial, double* __restrict__ score, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) score[i] = -(partial[i] + partial[N + i]);
}

template <int RT>
int launch_pca_md(const PcaMdArgs& g, hipStream_t s) {
  constexpr int BM = 16 * RT;
  const int64_t n_pad = n_padded(g.n);
  const size_t shmem = ((size_t)2 * BM * APITCH + (size_t)BM * (n_pad + 2) + 4 * BM) * sizeof(double);
  if (shmem > 160 * 1024) return RUNIA_E_INVALID;
  static std::atomic<uint64_t> lds_ok{0};
  if (runia_allow_dynamic_lds(reinterpret_cast<const void*>(pca_md_kernel<RT>), 160 * 1024, lds_ok) != RUNIA_OK)
    return RUNIA_E_LAUNCH;
  const int64_t tiles = (g.N + BM - 1) / BM;
  pca_md_kernel<RT><<<(unsigned)tiles, 256, shmem, s>>>(g);
  return runia_check_launch();
}

}  // namespace

extern "C" int runia_pca_md_score_f64(const double* h, const double* packed_ct, const double* bias,
                                      const double* scale, const double* md_mean, const double* packed_p,
                                      double* score, double* y_out, int64_t N, int64_t D, int64_t n,
                                      runia_stream_t stream) {
  if (N < 0 || D <= 0 || n <= 0) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!h || !md_mean || !packed_p || !score) return RUNIA_E_INVALID;
  if (packed_ct ? !bias : (n != D)) return RUNIA_E_INVALID;
  PcaMdArgs g{h, packed_ct, bias, scale, md_mean, packed_p, score, y_out, N, D, n};
  // 32-row tiles halve the L2 traffic of the packed weights but need >= ~4 tiles per CU to balance
  const int64_t tiles32 = (N + 31) / 32;
  const int64_t n_pad = n_padded(n);
  const bool fits32 = ((size_t)2 * 32 * APITCH + (size_t)32 * (n_pad + 2) + 128) * 8 <= 160 * 1024;
  if (tiles32 >= 1024 && fits32) return launch_pca_md<2>(g, as_stream(stream));
  return launch_pca_md<1>(g, as_stream(stream));
}

// The DMA form addresses the rows and the packed matrix through 32-bit buffer offsets and stages whole 32-deep chunks.
// Measured against the register-staged form (tools/ablate/run_proj_acc.py, us per launch, D = 512, r = 256):
//   N = 2 000 / 5 000 / 8 000 / 10 000: 20.9 / 26.1 / 33.9 / 41.4 vs 23.0 / 27.9 / 35.8 / 43.5 (every workgroup resident
//   at once: 5 per CU); 12 000 / 15 000 / 20 000: 56.8 / 69.7 / 86.2 vs 52.0 / 67.5 / 83.7 (a second, partial round of
//   16-row workgroups: slower); 32 x 256 tiles at 40 000 / 100 000: 158.8 / 410.3 vs 167.3 / 426.3.
static bool proj_sq_dma_ok(int64_t D, int64_t r) {
  return K2_DMA && D % KC == 0 && D < (1 << 23) && packed_elems(D, r) < ((int64_t)1 << 29);
}
static bool proj_sq_one_round(unsigned grid) { return (int64_t)grid <= (int64_t)K2_WAVES_DMA * runia_cu_count(); }
// TRAP here: 0 dense, 1 upper-trapezoidal M (kernel form K2_TRAP_FORM), 2 its row blocks in balanced order (kernel form 3)
template <int TRAP, int RT, int NCT, bool ACCUMULATE, bool SPLIT>
static void launch_proj_sq(unsigned grid, hipStream_t s, const ProjSqArgs& g, bool dma) {
  const bool use_dma = dma && (RT > 1 || proj_sq_one_round(grid));
  if constexpr (TRAP) {
    constexpr int FORM = TRAP == 2 ? 3 : K2_TRAP_FORM;
    // The register-staged 16-row forms stay dense (same bits): with the start chunk to carry they spill 12-20 bytes of scratch at
    // the 96 of 5 waves per SIMD and measured 85.3 us against 83.5 us dense at N = 20 000.
    if (use_dma) proj_sq_kernel<RT, NCT, ACCUMULATE, SPLIT, true, FORM><<<grid, 256, 0, s>>>(g);
    else if constexpr (RT > 1) proj_sq_kernel<RT, NCT, ACCUMULATE, SPLIT, false, FORM><<<grid, 256, 0, s>>>(g);
    else proj_sq_kernel<RT, NCT, ACCUMULATE, SPLIT, false><<<grid, 256, 0, s>>>(g);
  } else {
    if (use_dma) proj_sq_kernel<RT, NCT, ACCUMULATE, SPLIT, true><<<grid, 256, 0, s>>>(g);
    else proj_sq_kernel<RT, NCT, ACCUMULATE, SPLIT, false><<<grid, 256, 0, s>>>(g);
  }
}

// 32 x 256 tiles (fewer re-reads of M, 65 TFLOP/s when they fill the chip evenly) or 16 x 128 half tiles (62 TFLOP/s,
// whatever the batch)?  The large tile only pays when its last round of workgroups is nearly full: N = 20 000 is 625
// large tiles = 2.44 rounds on 256 CUs and ran at 51 TFLOP/s; 16 384 / 32 768 / 65 536 rows (whole rounds) at 63-65.
static bool proj_sq_large_tiles(int64_t N, int64_t cus) {
  const int64_t tiles32 = (N + 31) / 32;
  const int64_t rounds = (tiles32 + cus - 1) / cus;
  return tiles32 >= 2 * cus && 100 * tiles32 >= 93 * rounds * cus;
}

template <int TRAP>
static int proj_sq_accumulate(const double* h, const double* packed_m, const double* c, double* score, int64_t N, int64_t D,
                              int64_t r, runia_stream_t stream) {
  if (N < 0 || D <= 0 || r <= 0) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!h || !packed_m || !c || !score) return RUNIA_E_INVALID;
  ProjSqArgs g{h, packed_m, c, score, nullptr, N, D, r};
  hipStream_t s = as_stream(stream);
  const int64_t tiles16 = (N + 15) / 16, cus = runia_cu_count();
  const bool dma = proj_sq_dma_ok(D, r);
  if (r <= 64) launch_proj_sq<TRAP, 1, 1, true, false>((unsigned)tiles16, s, g, dma);
  else if (r <= 128) launch_proj_sq<TRAP, 1, 2, true, false>((unsigned)tiles16, s, g, dma);
  else if (proj_sq_large_tiles(N, cus)) launch_proj_sq<TRAP, 2, 4, false, false>((unsigned)((N + 31) / 32), s, g, dma);
  else if (tiles16 > cus / 2) launch_proj_sq<TRAP, 1, 2, true, true>((unsigned)((tiles16 + 7) / 8 * 16), s, g, dma);
  else launch_proj_sq<TRAP, 1, 4, false, false>((unsigned)tiles16, s, g, dma);
  return runia_check_launch();
}

extern "C" int runia_proj_sq_accumulate_f64(const double* h, const double* packed_m, const double* c, double* score,
                                            int64_t N, int64_t D, int64_t r, runia_stream_t stream) {
  return proj_sq_accumulate<0>(h, packed_m, c, score, N, D, r, stream);
}
// the caller promises M[j][k] = 0 for k < j (r <= D): same bits as the plain entry point on that matrix, fewer chunks
extern "C" int runia_proj_sq_accumulate_trap_f64(const double* h, const double* packed_m, const double* c, double* score,
                                                 int64_t N, int64_t D, int64_t r, runia_stream_t stream) {
  if (r > D) return RUNIA_E_INVALID;
  return proj_sq_accumulate<1>(h, packed_m, c, score, N, D, r, stream);
}
// the caller promises that M with its 32-row blocks in the balanced order of trap_order.hpp (runia_trap_balance_rows_f64)
extern "C" int runia_proj_sq_accumulate_btrap_f64(const double* h, const double* packed_m, const double* c, double* score,
                                                  int64_t N, int64_t D, int64_t r, runia_stream_t stream) {
  if (r > D) return RUNIA_E_INVALID;
  return proj_sq_accumulate<2>(h, packed_m, c, score, N, D, r, stream);
}

extern "C" size_t runia_proj_sq_workspace_bytes(int64_t N) { return N > 0 ? (size_t)N * 2 * sizeof(double) : 0; }

template <int TRAP>
static int proj_sq_score(const double* h, const double* packed_m, const double* c, double* score, void* workspace,
                         size_t workspace_bytes, int64_t N, int64_t D, int64_t r, runia_stream_t stream) {
  if (N < 0 || D <= 0 || r <= 0) return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!h || !packed_m || !c || !score) return RUNIA_E_INVALID;
  ProjSqArgs g{h, packed_m, c, score, reinterpret_cast<double*>(workspace), N, D, r};
  hipStream_t s = as_stream(stream);
  const int64_t tiles16 = (N + 15) / 16, cus = runia_cu_count();
  const bool dma = proj_sq_dma_ok(D, r);
  if (r <= 64) {
    launch_proj_sq<TRAP, 1, 1, false, false>((unsigned)tiles16, s, g, dma);
  } else if (r <= 128) {
    launch_proj_sq<TRAP, 1, 2, false, false>((unsigned)tiles16, s, g, dma);
  } else if (proj_sq_large_tiles(N, cus)) {
    launch_proj_sq<TRAP, 2, 4, false, false>((unsigned)((N + 31) / 32), s, g, dma);
  } else if (tiles16 > cus / 2 && workspace && workspace_bytes >= runia_proj_sq_workspace_bytes(N)) {
    // (32-, 48- and 64-row tiles with the same column split measured 64, 64 and 78 us against 59 us)
    launch_proj_sq<TRAP, 1, 2, false, true>((unsigned)((tiles16 + 7) / 8 * 16), s, g, dma);
    proj_sq_combine_kernel<<<(unsigned)((N + 255) / 256), 256, 0, s>>>(g.partial, score, N);
  } else {
    launch_proj_sq<TRAP, 1, 4, false, false>((unsigned)tiles16, s, g, dma);
  }
  return runia_check_launch();
}

extern "C" int runia_proj_sq_score_f64(const double* h, const double* packed_m, const double* c, double* score,
                                       void* workspace, size_t workspace_bytes, int64_t N, int64_t D, int64_t r,
                                       runia_stream_t stream) {
  return proj_sq_score<0>(h, packed_m, c, score, workspace, workspace_bytes, N, D, r, stream);
}
extern "C" int runia_proj_sq_score_trap_f64(const double* h, const double* packed_m, const double* c, double* score,
                                            void* workspace, size_t workspace_bytes, int64_t N, int64_t D, int64_t r,
                                            runia_stream_t stream) {
  if (r > D) return RUNIA_E_INVALID;
  return proj_sq_score<1>(h, packed_m, c, score, workspace, workspace_bytes, N, D, r, stream);
}
extern "C" int runia_proj_sq_score_btrap_f64(const double* h, const double* packed_m, const double* c, double* score,
                                             void* workspace, size_t workspace_bytes, int64_t N, int64_t D, int64_t r,
                                             runia_stream_t stream) {
  if (r > D) return RUNIA_E_INVALID;
  return proj_sq_score<2>(h, packed_m, c, score, workspace, workspace_bytes, N, D, r, stream);
}
