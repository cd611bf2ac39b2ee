// Fused LaREM row pipeline (a11): LaRExInference.get_score after the backbone
// (reference inference/image_level.py:115-119) as three launches per batch instead of
// ~100 tiny ones per image:
//
//   K0  mc_mask      DropBlock draws (N,n_mc,H,W) -> per-image keep-flag table (the DropBlock2D masks of
//                    feature_extraction/abstract_classes.py:91-96 as 0/1 floats, drop layers sorted by mask sum).
//                    Bit arithmetic on one 64-bit word per drop layer; ~9 us per 10 000 images.  Not launched in the
//                    product case (4x4, 16 drop layers, explicit draws): there K1 reads the draws itself and looks the
//                    layers' flags up in a geometry table (mc_entropy_lut_kernel) - two launches per batch.
//   K1  mc_entropy   hooked latent maps (N,C,H,W) + table -> per-dimension entropies H (N,C) f64
//                    = MCSamplerModule.forward (feature_extraction/abstract_classes.py:81-101) fused with
//                      the per-dimension loop of get_dl_h_z (evaluation/entropy.py:77-82).  One thread owns
//                      one (image, channel): its H*W map stays in VGPRs, the n_mc MC samples are produced,
//                      sorted and reduced to one entropy without ever leaving registers.  VALU-issue-bound.
//   K2' proj_sq      H (N,D) f64 -> LaREM score (N) = apply_pca_transform (dimensionality_reduction.py:86)
//                    + MDLatentSpace.postprocess (inference/postprocessors.py:241-242) folded into ONE contraction
//                    on the f64 matrix cores (K2 pca_md is the two-contraction form, kept for non-PSD precisions).
//
// Sample order inside an image is irrelevant to the entropy (order statistics), so K1 visits the drop
// layers sorted by their mask sum and recomputes the per-element quotients (x*numel)/sum only when the sum
// changes (wave-uniform branch): same bits as the upstream op order.
// K1 (vector ALU) and K2' (f64 matrix instructions) share the SIMD's issue port on gfx950 and do not overlap
// (tools/microbench/mfma_valu_overlap.hip); they run back to back on one stream.
#include <type_traits>

#include "common.hpp"
#include "entropy_core.hpp"
#include "philox.hpp"
#include "div_consts.hpp"
#include "roi_source.hpp"

namespace {

using namespace runia_entropy;

constexpr int kMaxMC = 64;
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

// K0_NT_STORE / K1_NT_STORE: K0's table and K1's entropies leave as streaming (non-temporal) stores instead of ordinary
// write-back ones.  Both measured and left off (profiles/README.md, "K1 without the z_out branches").
#ifndef K0_NT_STORE
#define K0_NT_STORE 0
#endif
#ifndef K1_NT_STORE
#define K1_NT_STORE 0
#endif
template <int NT, typename T>
__device__ __forceinline__ void store_out(T* p, T v) {
  if constexpr (NT != 0) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// Keep-flag table of one image (K0 -> K1), n_mc*(HW+2) floats:
//   n_mc records of HW floats: 0.0 where the drop layer removes the position, 2^-a where it keeps it, with the layer's
//     mask sum written as sum = 2^a * m (m odd).  The DropBlock rescale x * numel / sum = (x * numel / m) * 2^-a and a
//     power-of-two factor commutes with every rounding that follows (products, row sums, means), so it rides on the
//     flags for free;  positions in K1's operand order (mask_slot);
//   n_mc floats zh = RN(1/m) and n_mc floats zl = RN(1/m - zh): the layer's quotients are q = fma(u, zh, u * zl),
//     the correctly rounded u / m in two instructions (div_consts.hpp, proven by tools/verify_div_constants.py).
//     A layer that drops the whole map has zh = NaN (0 * numel / 0 upstream).
// Drop layers are sorted by m (layers that share m share their quotients; m = 1 - sums 1, 2, 4, 8, 16, ... - needs none).
__device__ __forceinline__ void layer_consts(int cnt, int& m, float& flag, float& zh, float& zl) {
  const int a = cnt ? __ffs(cnt) - 1 : 0;
  m = cnt >> a;
  flag = __uint_as_float((unsigned)(127 - a) << 23);  // 2^-a
  zh = cnt ? __uint_as_float(runia_div::kDivHi[(m - 1) >> 1]) : NAN;
  zl = cnt ? __uint_as_float(runia_div::kDivLo[(m - 1) >> 1]) : 0.f;
}

__device__ __forceinline__ float add_f32(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ float div_newton(float u, float den, float r) {
  const float q = u * r;
  const float e = fmaf(-den, q, u);
  return fmaf(e, r, q);
}

// position p of the map -> slot of its keep flag in a table record (K1's operand order)
template <int HT, int WT>
__host__ __device__ constexpr int mask_slot(int p) {
  // even H: rows 2k and 2k+1 are interleaved so that one 64-bit scalar operand feeds a packed FMA
  if constexpr (HT % 2 == 0) {
    const int y = p / WT, xw = p - y * WT;
    return ((y >> 1) * WT + xw) * 2 + (y & 1);
  } else {
    return p;
  }
}

// K0 for maps of at most 64 positions (2x2, 4x4, 7x7, 8x8 ...): a drop layer is one 64-bit word and
// the whole derivation is bit arithmetic in registers - no LDS, no barrier, one HBM round trip.
//   seeds   : lane = (layer, position); `draw < gamma` -> ballot -> 64/HW layers per word
//   dilation: lane = layer; separable OR of the seed word shifted over the block window (columns, then rows)
//   sort    : rank by popcount through readlane broadcasts; each lane stores its own table record
// (The LDS kernel this one replaced spent ~110 instructions per (layer, position) and 17-18 us per 10 000 images whatever
// its workgroup shape; an empty launch of the same grid takes 5 us; profiles/README.md.)
template <int HT, int WT>
__host__ __device__ constexpr int slot_position(int slot) {  // inverse of mask_slot
  if constexpr (HT % 2 == 0) {
    const int e = slot & 1, t = slot >> 1;
    const int k = t / WT, xw = t - k * WT;
    return (2 * k + e) * WT + xw;
  } else {
    return slot;
  }
}

template <int HT, int WT>
__device__ __forceinline__ unsigned long long columns_below(int k) {  // positions (y, x) with x < k
  unsigned long long row = (k >= 64) ? ~0ull : ((1ull << k) - 1ull), m = 0ull;
#pragma unroll
  for (int y = 0; y < HT; ++y) m |= row << (y * WT);
  return m;
}

constexpr int kMaskBitsWaves = 4;  // images per workgroup (independent waves)

template <int HT, int WT, int NP, bool REDRAW = false>
__global__ __launch_bounds__(64 * kMaskBitsWaves) void mc_mask_bits_kernel(const float* __restrict__ rnd,
                                                                           int64_t rand_stride,
                                                                           float* __restrict__ table, int64_t N,
                                                                           int n_mc, float gamma, int block_size,
                                                                           int identity, int sort_layers,
                                                                           uint64_t rng_seed, int64_t first_image) {
  constexpr int HW = HT * WT;
  static_assert(HW <= 64 && NP <= 64, "one drop layer per 64-bit word");
  // draw i = layer * HW + position sits in bit i % 64 of ballot word i / 64.  Map sizes that divide 64 (2x2, 4x4, 8x8)
  // keep whole layers inside a word; any other size (7x7: 49 bits) lets a layer straddle two words, and the lane that
  // owns the layer stitches its bits together from them.
  constexpr bool DIV = (64 % HW == 0);
  constexpr int WORDS = (NP * HW + 63) / 64;
  constexpr unsigned long long FULL = (HW == 64) ? ~0ull : ((1ull << HW) - 1ull);
  const int lane = threadIdx.x & 63;
  const int64_t img = (int64_t)blockIdx.x * kMaskBitsWaves + (threadIdx.x >> 6);
  if (img >= N) return;  // wave-uniform
  const int bit0 = lane * HW, word0 = bit0 >> 6, off = bit0 & 63;  // where this lane's layer (lane = layer) starts
  const int pad = block_size / 2;

  // seed word of this lane's layer from attempt `attempt` of the draws (attempt > 0: counter mode only)
  auto seeds_of = [&](unsigned attempt) -> unsigned long long {
    float d[WORDS];
    if (rnd) {
      const float* r = rnd + img * rand_stride;
#pragma unroll
      for (int t = 0; t < WORDS; ++t) {
        const int i = lane + 64 * t;
        d[t] = (i < n_mc * HW) ? r[i] : 1.0f;
      }
    } else {  // counter mode (philox.hpp): this lane's words 4q .. 4q+3 are the four components of one Philox block
#pragma unroll
      for (int q = 0; q < (WORDS + 3) / 4; ++q) {
        const runia_philox::u4 b = runia_philox::lane_block(rng_seed, (uint64_t)(first_image + img), lane, q, attempt);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = 4 * q + j;
          if (t < WORDS) d[t] = (lane + 64 * t < n_mc * HW) ? runia_philox::component(b, j) : 1.0f;
        }
      }
    }
    unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
    for (int t = 0; t < WORDS; ++t) {
      const unsigned long long w = __ballot(d[t] < gamma);
      if (t == word0) lo = w;
      if (!DIV && t == word0 + 1) hi = w;
    }
    unsigned long long sd = lo >> off;
    if (!DIV && off + HW > 64) sd |= hi << (64 - off);
    return sd & FULL;
  };
  auto keep_of = [&](unsigned long long seed) -> unsigned long long {
    unsigned long long hx = 0ull;
    for (int dx = 0; dx < block_size; ++dx) {  // dropped(y, x) |= seed(y, x + ox)
      const int ox = dx - pad;
      if (ox >= WT || -ox >= WT) continue;
      hx |= (ox >= 0) ? ((seed >> ox) & columns_below<HT, WT>(WT - ox))
                      : ((seed << -ox) & ~columns_below<HT, WT>(-ox) & FULL);
    }
    unsigned long long dropped = 0ull;
    for (int dy = 0; dy < block_size; ++dy) {  // ... |= hx(y + oy, x)
      const int oy = dy - pad;
      if (oy >= HT || -oy >= HT) continue;
      dropped |= (oy >= 0) ? (hx >> (oy * WT)) : ((hx << (-oy * WT)) & FULL);
    }
    return ~dropped & FULL;
  };

  unsigned long long keep = identity ? FULL : keep_of(seeds_of(0u));
  if (REDRAW && !identity && !rnd) {
    // throughput mode, opt-in: a drop layer that removed the whole map (0 * numel / 0 = NaN upstream) draws again from
    // the next counter block of the same image - a bounded, wave-uniform loop that only images with such a layer enter
    for (unsigned attempt = 1; attempt <= 16u; ++attempt) {
      if (__ballot(lane < n_mc && keep == 0ull) == 0ull) break;
      const unsigned long long again = keep_of(seeds_of(attempt));
      if (keep == 0ull) keep = again;
    }
  }
  const int cnt = __popcll(keep);
  int m;
  float flag, zh, zl;
  layer_consts(cnt, m, flag, zh, zl);
  const int key = m ? m : 127;  // fully dropped maps last
  int rank = 0;  // stable counting sort of the drop layers by the odd part of their mask sum
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int o = __shfl(key, j, 64);
    rank += (j < n_mc) && ((o < key) || (o == key && j < lane));
  }
  if (!sort_layers) rank = lane;  // table in the order of the draws (runia_mc_stack_table_f32)
  if (lane >= n_mc) return;
  float* out = table + img * (int64_t)(n_mc * (HW + 2));
  float* rec = out + rank * HW;
  if constexpr (HW % 4 == 0) {
#pragma unroll
    for (int c = 0; c < HW / 4; ++c) {
      f4 v;
      v.x = ((keep >> slot_position<HT, WT>(4 * c)) & 1ull) ? flag : 0.f;
      v.y = ((keep >> slot_position<HT, WT>(4 * c + 1)) & 1ull) ? flag : 0.f;
      v.z = ((keep >> slot_position<HT, WT>(4 * c + 2)) & 1ull) ? flag : 0.f;
      v.w = ((keep >> slot_position<HT, WT>(4 * c + 3)) & 1ull) ? flag : 0.f;
      store_out<K0_NT_STORE>(reinterpret_cast<f4*>(rec) + c, v);
    }
  } else {
#pragma unroll
    for (int q = 0; q < HW; ++q)
      store_out<K0_NT_STORE>(rec + q, ((keep >> slot_position<HT, WT>(q)) & 1ull) ? flag : 0.f);
  }
  store_out<K0_NT_STORE>(out + n_mc * HW + rank, zh);
  store_out<K0_NT_STORE>(out + n_mc * (HW + 1) + rank, zl);
}

// ---- geometry table: what K0 derives from a layer's seed bits, for every seed word -------------------------------------
// Between the ballot and the table record K0 computes a pure function of (H, W, block_size): neither the data nor gamma
// enters.  For maps of 16 positions there are 65 536 seed words, so the function is a table built once on the host:
// record `key` = the 16 keep flags (2^-a or 0, mask_slot order), zh, zl - exactly K0's record of a layer whose seed word is
// `key` - and in the padding a sort word and the odd part m (0: the layer drops the whole map).
//   sort word = class << 27 | key * 80: class = (m - 1) / 2, 8 for a fully dropped layer; the kernel ORs the layer index
//   in at bit 23, so that an ascending sort is K0's order (by m, dead layers last, ties by layer) and the low 23 bits are
//   the record's byte offset.  With gamma = 0.125 99 % of the layers have at most 5 seeds: 6 885 records, 550 KB.
constexpr int kLutRecDwords = 20, kLutSortDword = 18, kLutOddDword = 19;
constexpr int kLutLayerShift = 23, kLutClassShift = 27;
constexpr unsigned kLutOffsetMask = (1u << kLutLayerShift) - 1u;
constexpr size_t kLutKeys = 65536;
static_assert((kLutKeys - 1) * kLutRecDwords * 4 <= kLutOffsetMask, "a record's byte offset fits below the layer index");
// The table is padded with zero records up to the largest offset the mask lets through: whatever the words a caller's
// table holds, the kernel's reads stay inside the lut_bytes the entry point has checked.
constexpr size_t kLutRecords = (kLutOffsetMask + 1) / (kLutRecDwords * 4) + 2;
static_assert(kLutRecords * kLutRecDwords * 4 >= kLutOffsetMask + 1 + kLutRecDwords * 4, "every masked offset reads inside the table");

void flag_lut_fill_4x4(uint32_t* out, int block_size) {
  constexpr int HT = 4, WT = 4, HW = 16;
  const int pad = block_size / 2;
  for (size_t i = kLutKeys * kLutRecDwords; i < kLutRecords * kLutRecDwords; ++i) out[i] = 0u;
  for (unsigned key = 0; key < kLutKeys; ++key) {
    unsigned keep = 0;
    for (int y = 0; y < HT; ++y)
      for (int xw = 0; xw < WT; ++xw) {
        bool dropped = false;  // a seed inside the block window of (y, x), as keep_of of K0
        for (int yy = 0; yy < HT; ++yy)
          for (int xx = 0; xx < WT; ++xx)
            if (((key >> (yy * WT + xx)) & 1u) && yy - y >= -pad && yy - y < block_size - pad && xx - xw >= -pad &&
                xx - xw < block_size - pad)
              dropped = true;
        if (!dropped) keep |= 1u << (y * WT + xw);
      }
    const int cnt = __builtin_popcount(keep);
    const int a = cnt ? __builtin_ctz((unsigned)cnt) : 0;  // layer_consts on the host
    const int m = cnt >> a;
    const uint32_t flag = (uint32_t)(127 - a) << 23;  // 2^-a
    uint32_t* rec = out + (size_t)key * kLutRecDwords;
    for (int slot = 0; slot < HW; ++slot) rec[slot] = ((keep >> slot_position<HT, WT>(slot)) & 1u) ? flag : 0u;
    rec[HW] = cnt ? runia_div::kDivHiC[(m - 1) >> 1] : 0x7fc00000u;  // NaN: 0 * numel / 0 upstream
    rec[HW + 1] = cnt ? runia_div::kDivLoC[(m - 1) >> 1] : 0u;
    const unsigned cls = cnt ? (unsigned)(m - 1) >> 1 : 8u;
    rec[kLutSortDword] = (cls << kLutClassShift) | (key * (unsigned)(kLutRecDwords * 4));
    rec[kLutOddDword] = (uint32_t)m;
  }
}

// Ascending sort of 16 wave-uniform words (Batcher's odd-even merge sort, 63 compare-exchanges): s_min_u32 + s_max_u32 each,
// no vector instruction.
__device__ __forceinline__ void sort16_uniform(unsigned (&v)[16]) {
#pragma unroll
  for (int p = 1; p < 16; p <<= 1) {
#pragma unroll
    for (int k = p; k >= 1; k >>= 1) {
#pragma unroll
      for (int j = k % p; j + k < 16; j += 2 * k) {
#pragma unroll
        for (int i = 0; i < k; ++i) {
          if (i + j + k < 16 && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            const unsigned lo = v[i + j] < v[i + j + k] ? v[i + j] : v[i + j + k];
            const unsigned hi = v[i + j] < v[i + j + k] ? v[i + j + k] : v[i + j];
            v[i + j] = lo;
            v[i + j + k] = hi;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// K1: latent map -> MC samples -> entropy.   one workgroup = (image, block of kK1Block channels); no LDS, no barrier.
// The mask table is wave-uniform: it arrives through the scalar cache (s_load) and enters the arithmetic as
// SGPR operands.  A drop layer is acc = fma(q, keep, acc) over the map in the upstream summation order
// (keep = 1: the add of the reference; keep = 0: acc unchanged), two rows per v_pk_fma_f32.
// ------------------------------------------------------------------------------------------
#ifndef K1_BLOCK
#define K1_BLOCK 128
#endif
constexpr int kK1Block = K1_BLOCK;  // channels (threads) per workgroup: 185 us vs 199 us with 256 at N = 10 000

// ---- ROI source of K1 (BASELINE config 4, reference feature_extraction/object_level.py:340-349 + 312-367): instead of a
// (K, C, PH, PW) tensor that roi_align wrote, a thread builds its PH x PW map in registers from the feature map itself.
// `x` of the kernel then points at a RoiSource (written by roi_sample_table_kernel, roi.hip): the feature map in NHWC
// (channel = lane: every bilinear tap of a wave is one contiguous 4 * 64-byte run) and, per ROI, a SEPARABLE table of its
// bilinear samples - per sample row (ph, iy): byte offsets of the two map rows and the weights hy, ly; per sample column
// (pw, ix): byte offsets of the two map columns and hx, lx; two bit masks of the rows / columns
// more than a pixel outside the map (their samples contribute 0) - 480 bytes for 7x7 bins of 2x2 samples,
// wave-uniform, read through the scalar cache.  (A table of all 196 samples with their four offsets and four products,
// 6.3 KB per ROI, kept every vector instruction out of the weights but streamed 376 MB per 60 000 ROIs through the scalar
// cache: 7 of the 11 ms the launch took.)  A bin is the sum of its G x G samples in (iy, ix) order, each
// (hy hx) v1 + (hy lx) v2 + (ly hx) v3 + (ly lx) v4, divided by G * G: the arithmetic of roi_align_kernel, same bits
// (tests/test_api_gpu.py).  The taps are buffer loads with the sample's offset as the scalar operand: no vector instruction
// goes into addressing.  How it got to 3.6 ms per 60 000 ROIs x 256 channels x 7x7 bins (roi_align 9.4 + K1 1.1 as two
// launches): a table of all 196 samples (offsets and products, 6.3 KB per ROI) streamed 376 MB through the scalar cache -
// 11.2 ms, 7 of them scalar-cache misses; the separable table 8.7 ms, every sample's four loads followed by a wait (four
// loads in flight per wave, ~380 ns each); all 56 taps of a sample row requested before the first is used: 3.6 ms, the
// vector L1 path now at ~18 TB/s of taps.  (The four taps of a sample as ONE 16-byte load from a map of quads
// (f[y][x], f[y][x+1], f[y+1][x], f[y+1][x+1]): the same bytes, a quarter of the instructions, no reuse left for the L1 -
// 11.1 ms in the unpipelined form, not kept.)  The struct itself: roi_source.hpp.

template <int HT, int WT, int G>
__device__ __forceinline__ void roi_load_map(float (&u)[HT * WT], const RoiSource* __restrict__ src, int64_t roi, int c) {
  // the table is read through the constant address space: loads the compiler may keep on the scalar unit (through a
  // plain pointer loaded from memory it reads the wave-uniform entries with vector loads and wraps every tap in a
  // readfirstlane loop)
  typedef const __attribute__((address_space(4))) unsigned* cptr;
  cptr tab = (cptr)(src->table + roi * (int64_t)src->roi_dwords);  // wave-uniform
  const unsigned image = tab[0];
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(src->nhwc) + (int64_t)image * (src->image_bytes / 4), 0, (int)src->image_bytes, 0x00020000);
  const int voff = c * 4;
  cptr rows = tab + 8, cols = tab + 8 + 4 * (HT * G);
  constexpr float count = (float)(G * G);
  // The column entries first (offsets stay in scalar registers, the weights move to vector registers: a vector multiply
  // takes one scalar operand, the row's), then per sample row ALL its taps are requested before the first is used: left
  // to the compiler every sample's four loads were followed by a wait - four loads in flight per wave, 380 ns each,
  // 8.7 ms per 60 000 ROIs x 256 channels with the load path a sixth busy.
  constexpr int SX = WT * G, SY = HT * G;
  unsigned ox_lo[SX], ox_hi[SX];
  float hx[SX], lx[SX];
#pragma unroll
  for (int sx = 0; sx < SX; ++sx) {
    ox_lo[sx] = cols[4 * sx];
    ox_hi[sx] = cols[4 * sx + 1];
    hx[sx] = __uint_as_float(cols[4 * sx + 2]);
    lx[sx] = __uint_as_float(cols[4 * sx + 3]);
  }
  float acc[HT * WT];
#pragma unroll
  for (int p = 0; p < HT * WT; ++p) acc[p] = 0.f;
  // The two pixel rows of a sample row stay in registers: sample rows are 1/G of a bin apart, so on a box of fewer than
  // 2 * SY feature rows the next sample row uses the same two pixel rows again (no load) or the upper one becomes the lower
  // (SX * 2 loads instead of SX * 4).  Which of the three it is depends on the table alone (wave-uniform), and a pixel read
  // once is the pixel read twice: the same bits as one load per tap.
  float tl[SX][2], th[SX][2];
  unsigned cur_lo = 0xffffffffu, cur_hi = 0xffffffffu;  // (no pixel row starts at this byte offset)
#pragma unroll
  for (int sy = 0; sy < SY; ++sy) {
    const unsigned oy_lo = rows[4 * sy], oy_hi = rows[4 * sy + 1];
    const float hy = __uint_as_float(rows[4 * sy + 2]), ly = __uint_as_float(rows[4 * sy + 3]);
    if (oy_lo != cur_lo || oy_hi != cur_hi) {
      if (oy_lo == cur_hi) {
#pragma unroll
        for (int sx = 0; sx < SX; ++sx) { tl[sx][0] = th[sx][0]; tl[sx][1] = th[sx][1]; }
      } else {
#pragma unroll
        for (int sx = 0; sx < SX; ++sx) {
          tl[sx][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (int)(oy_lo + ox_lo[sx]), 0));
          tl[sx][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (int)(oy_lo + ox_hi[sx]), 0));
        }
      }
#pragma unroll
      for (int sx = 0; sx < SX; ++sx) {
        th[sx][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (int)(oy_hi + ox_lo[sx]), 0));
        th[sx][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (int)(oy_hi + ox_hi[sx]), 0));
      }
      cur_lo = oy_lo;
      cur_hi = oy_hi;
    }
    __builtin_amdgcn_sched_barrier(0);  // (the loads above stay above)
#pragma unroll
    for (int sx = 0; sx < SX; ++sx) {
      // (a sample outside the map: zero weights and taps beyond the buffer, which read as 0 - the table sees to both)
      const float w1 = hy * hx[sx], w2 = hy * lx[sx], w3 = ly * hx[sx], w4 = ly * lx[sx];
      const float val = w1 * tl[sx][0] + w2 * tl[sx][1] + w3 * th[sx][0] + w4 * th[sx][1];
      float& bin = acc[(sy / G) * WT + (sx / G)];
      bin += val;  // a bin receives its samples in (iy, ix) order
      // added NOW: left alone the compiler keeps all SY * SX sample values in registers to add them in pairs at the end
      // (247 vector registers, two waves per SIMD; the loader needs the bins, two pixel rows and little else)
      asm volatile("" : "+v"(bin));
    }
  }
#pragma unroll
  for (int p = 0; p < HT * WT; ++p) u[p] = acc[p] / count;
}

#ifndef K1_IMGS
#define K1_IMGS 1  // images per workgroup, one after the other (timing experiments: fewer, longer waves)
#endif
// ZOUT: the launch also writes the MC samples to z_out (the sampler-only entry point and the tests); the product launch
// passes no z_out and takes the instantiation without the stores, whose drop layers are then free of branches on it.
// LUT: `table` is the geometry table (flag_lut_fill_4x4 above) and the launch reads the draws itself: no K0, no per-image table.
//   A wave forms its image's seed bits with four ballots (the draws as K0 reads them, bit i = layer * HW + position), takes
//   each layer's 16-bit seed word as the key of its table record, and orders the 16 layers as K0 does - by the odd part of the
//   mask sum, then by layer - with a sorting network over the records' sort words on the scalar unit.  Everything after that
//   is the table form; only the address of a layer's operands differs.
template <int HT, int WT, int NP, int K, bool FULL, bool ENTROPY, int ROI_G, bool ZOUT, bool LUT = false>
__device__ __forceinline__ void mc_entropy_item(const float* __restrict__ x, const float* __restrict__ table,
                                                double* __restrict__ h, float* __restrict__ z_out,
                                                double* __restrict__ zero_fill, int64_t N, int C, int n_mc_rt,
                                                double min_dist, double const_term, double inv_n, int64_t img, int c,
                                                const float* __restrict__ rnd = nullptr, int64_t rand_stride = 0,
                                                float gamma = 0.f) {
  constexpr int HW = HT * WT;
  constexpr bool PAIRS = (HT % 2 == 0);
  const int n_mc = FULL ? NP : n_mc_rt;
  if (img >= N) return;
  // the ballots come before any lane leaves: a wave with fewer than 64 live channels still needs all 64 draws of a word
  unsigned long long seedw[LUT ? NP * HW / 64 : 1];
  if constexpr (LUT) {
    static_assert(!LUT || (HW == 16 && NP == 16 && FULL && !ZOUT && ROI_G == 0), "the geometry table is for 4x4 x 16 layers");
    const float* r = rnd + img * rand_stride + (threadIdx.x & 63);
#pragma unroll
    for (int t = 0; t < NP * HW / 64; ++t) seedw[t] = __ballot(r[64 * t] < gamma);
  }
  if (zero_fill && c == 0) zero_fill[img] = 0.0;  // the accumulator of the score launch that follows (optional)
  if (c >= C) return;
  typedef const __attribute__((address_space(4))) unsigned* lut_ptr;  // constant address space: scalar loads
  const lut_ptr lut = (lut_ptr) reinterpret_cast<const unsigned*>(table);
  unsigned sv[LUT ? NP : 1];  // LUT: the layers' sort words (class, layer, byte offset of the record), ascending
  if constexpr (LUT) {
#pragma unroll
    for (int s = 0; s < NP; ++s) {
      const unsigned key = (unsigned)(seedw[s >> 2] >> (16 * (s & 3))) & 0xffffu;
      sv[s] = lut[key * kLutRecDwords + kLutSortDword] | ((unsigned)s << kLutLayerShift);
    }
    sort16_uniform(sv);
  }
  const float* mk = table + img * (int64_t)(n_mc * (HW + 2));  // wave-uniform
  const float* zhs = mk + n_mc * HW;
  const float* zls = zhs + n_mc;
  float u[HW];
  if constexpr (ROI_G > 0) {
    roi_load_map<HT, WT, ROI_G>(u, reinterpret_cast<const RoiSource*>(x), img, c);
  } else {
    // 16-byte loads at a 4*HW-byte lane stride: measured faster than staging the block's contiguous run
    // through LDS (214 vs 271 us at N = 10 000, profiles/README.md) - the kernel is VALU-bound, not HBM-bound
    const float* xc = x + (img * C + c) * (int64_t)HW;
    if constexpr (HW % 4 == 0) {
#pragma unroll
      for (int p = 0; p < HW / 4; ++p) {
        const float4 v = reinterpret_cast<const float4*>(xc)[p];
        u[4 * p] = v.x; u[4 * p + 1] = v.y; u[4 * p + 2] = v.z; u[4 * p + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int p = 0; p < HW; ++p) u[p] = xc[p];
    }
  }
  constexpr bool w_pow2 = (WT & (WT - 1)) == 0, h_pow2 = (HT & (HT - 1)) == 0;
  // Power-of-two scalings are exact and commute with rounding (no overflow / underflow at feature-map magnitudes),
  // so they are moved to where they cost nothing: with sum(bm) = 2^a * m, (x*numel)/sum = (x*numel/m) * 2^-a, the
  // factor 2^-a sits on the keep flags (K0), and when numel = H*W is a power of two it cancels against the 1/(H*W) of
  // mean_H(mean_W(.)): the sample is the plain sum of the quotients x/m over the kept positions, in upstream order.
  constexpr bool hw_pow2 = w_pow2 && h_pow2;
  if constexpr (!hw_pow2) {
#pragma unroll
    for (int p = 0; p < HW; ++p) u[p] *= (float)HW;
  }
  const float rW = 1.0f / (float)WT, rH = 1.0f / (float)HT;
  float z[NP];
  float q[PAIRS ? 1 : HW];   // quotients (x*numel)/sum ...
  f2 q2[PAIRS ? HW / 2 : 1];  // ... as row pairs in mask_slot order when H is even
  // quotients start out as x / 1 (the m = 1 group comes first in the sorted table).  The divisor in use is tracked by its
  // BIT PATTERN: both values sit in scalar registers, and gfx950 compares scalar integers on the scalar unit but floats only
  // on the vector unit (v_mov + v_cmp per drop layer: 32 of the kernel's 772 vector instructions)
  unsigned cur_zh_bits = __float_as_uint(1.0f);
#pragma unroll
  for (int p = 0; p < HW; ++p) {
    if constexpr (PAIRS) q2[mask_slot<HT, WT>(p) >> 1][mask_slot<HT, WT>(p) & 1] = u[p];
    else q[p] = u[p];
  }
  // G drop layers per trip of a rolled loop: G*HW keep flags live in SGPRs at a time (a fully unrolled loop
  // lets the compiler hoist all n_mc*HW scalar loads and spill them).  z is a shift register: constant indices
  // only, and the sample order is irrelevant to the sort that follows.
#ifndef K1_GCAP
#define K1_GCAP 128
#endif
  // (a run-time n_mc adds the clamped indices to the scalar side: with 8 layers per trip that instantiation spilled
  // scalar registers to vector lanes - 254 v_readlane / v_writelane; 4 per trip do not)
  constexpr int GCAP = FULL ? K1_GCAP : K1_GCAP / 2;
  constexpr int G = (GCAP / HW < 1) ? 1 : ((GCAP / HW > NP) ? NP : GCAP / HW);
  // the +inf fill only matters when fewer than NP samples are produced (FULL writes every slot: NP / G whole trips)
  if constexpr (!(FULL && NP % G == 0)) {
#pragma unroll
    for (int s = 0; s < NP; ++s) z[s] = INFINITY;
  }
#ifndef K1_TRIP_UNROLL
#define K1_TRIP_UNROLL 1
#endif
#pragma unroll K1_TRIP_UNROLL
  for (int s0 = 0; s0 < NP; s0 += G) {
    float znew[G];
    // The scalar operands of this trip.  They are NOT all requested here in the emitted code: G * HW flags do not fit the
    // scalar registers, so the compiler loads each drop layer's 16 flags into the same registers in front of that layer's
    // arithmetic and waits there.  Requesting layer g + 1's set ahead of layer g's arithmetic (a second register set,
    // scheduling barriers) measured slower in this loop: profiles/README.md, "K1 without the z_out branches".
    float dg[G], rg[G], mg[G][HW];
    // FULL: one base pointer per trip and constant offsets from it (the scalar loads then carry the layer's offset as an
    // immediate; with sc = s0 + g inside the index the compiler kept one 64-bit address per drop layer in scalar registers)
    const float* mk_t = mk + (FULL ? s0 * HW : 0);
    const float* zhs_t = zhs + (FULL ? s0 : 0);
    const float* zls_t = zls + (FULL ? s0 : 0);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if constexpr (LUT) {  // this trip's layers are sv[0 .. G-1]: constant indices, the array moves down after the trip
        const lut_ptr rec = lut + (sv[g] & kLutOffsetMask) / 4u;
        dg[g] = __uint_as_float(rec[HW]);
        rg[g] = __uint_as_float(rec[HW + 1]);
#pragma unroll
        for (int p = 0; p < HW; ++p) mg[g][p] = __uint_as_float(rec[p]);
      } else {
        const int sc = FULL ? g : ((s0 + g < n_mc) ? s0 + g : n_mc - 1);
        dg[g] = zhs_t[sc];
        rg[g] = zls_t[sc];
#pragma unroll
        for (int p = 0; p < HW; ++p) mg[g][p] = mk_t[sc * HW + p];
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int s = s0 + g;
      znew[g] = INFINITY;
      if (FULL || s < n_mc) {
        const float zh = dg[g], zl = rg[g];
        if (__float_as_uint(zh) != cur_zh_bits) {  // wave-uniform: every thread of the block works on the same image
#pragma unroll
          for (int p = 0; p < HW; ++p) {
            const float qv = fmaf(u[p], zh, u[p] * zl);  // u / m, correctly rounded (div_consts.hpp)
            if constexpr (PAIRS) q2[mask_slot<HT, WT>(p) >> 1][mask_slot<HT, WT>(p) & 1] = qv;
            else q[p] = qv;
          }
          cur_zh_bits = __float_as_uint(zh);
        }
        const float* m = mg[g];
        float col;
        if constexpr (PAIRS) {
          float rows[HT];
#pragma unroll
          for (int k2 = 0; k2 < HT / 2; ++k2) {
            const f2* qq = q2 + k2 * WT;
            const float* mm = m + 2 * k2 * WT;
            f2 acc = qq[0] * (f2){mm[0], mm[1]};  // torch_chain<WT>(0) == 0
#pragma unroll
            for (int xi = 1; xi < WT; ++xi) {  // the row in torch's CPU summation order (common.hpp)
              const int xw = torch_chain<WT>(xi);
              acc = __builtin_elementwise_fma(qq[xw], (f2){mm[2 * xw], mm[2 * xw + 1]}, acc);
            }
            if constexpr (hw_pow2) {
              // scaled once below
            } else if constexpr (w_pow2) {
              acc = acc * (f2){rW, rW};
            } else {
              acc = (f2){div_newton(acc.x, (float)WT, rW), div_newton(acc.y, (float)WT, rW)};
            }
            rows[2 * k2] = acc.x;
            rows[2 * k2 + 1] = acc.y;
          }
          // plain v_add_f32: left to itself the compiler adds the halves of the row-pair registers with v_pk_add_f32 and
          // op_sel, one useful add per packed instruction (4.2 issue cycles instead of 2.5)
          col = rows[0];
#pragma unroll
          for (int yi = 1; yi < HT; ++yi) col = add_f32(col, rows[torch_chain<HT>(yi)]);
        } else {
          float rm[HT];
#pragma unroll
          for (int y = 0; y < HT; ++y) {
            float rowsum = q[y * WT] * m[y * WT];
#pragma unroll
            for (int xi = 1; xi < WT; ++xi) {
              const int xw = torch_chain<WT>(xi);
              rowsum = fmaf(q[y * WT + xw], m[y * WT + xw], rowsum);
            }
            rm[y] = w_pow2 ? rowsum * rW : div_newton(rowsum, (float)WT, rW);
          }
          col = rm[0];
#pragma unroll
          for (int yi = 1; yi < HT; ++yi) col += rm[torch_chain<HT>(yi)];
        }
        if constexpr (hw_pow2 && PAIRS) znew[g] = col;
        else znew[g] = h_pow2 ? col * rH : div_newton(col, (float)HT, rH);
        // copy of the MC samples (drop-layer order is the table's; the sampler-only entry point and the tests).  Still a
        // run-time test inside the ZOUT instantiation: it parts the drop layers, and with a bare store the compiler
        // requests several layers' flags at once and spills scalar registers to vector lanes (4x4: 140 lane moves)
        if constexpr (ZOUT) {
          if (z_out) z_out[(img * n_mc + s) * (int64_t)C + c] = znew[g];
        }
      }
    }
#pragma unroll
    for (int i = NP - 1; i >= G; --i) z[i] = z[i - G];
#pragma unroll
    for (int g = 0; g < G; ++g) z[g] = znew[g];
    if constexpr (LUT) {
#pragma unroll
      for (int g = 0; g + G < NP; ++g) sv[g] = sv[g + G];
    }
  }
  if constexpr (ENTROPY) {
    // A NaN sample - a fully dropped map (0*numel/0 upstream), a NaN or infinite activation - makes the entropy NaN
    // upstream; the min/max sort below would silently drop it, so it is caught here: a sum is NaN iff a term is
    // (+inf pads of a short column cannot cancel: the samples are finite otherwise).
    float nan_probe = z[0];
#pragma unroll
    for (int s = 1; s < NP; ++s) nan_probe += z[s];
    const bool bad = nan_probe != nan_probe;
    sort_asc<NP>(z);
    double res = const_term + inv_n * column_log_sum<NP, K, FULL>(z, n_mc, min_dist);
    if (bad) res = NAN;
    store_out<K1_NT_STORE>(h + (img * C + c), res);
  }
}

template <int HT, int WT, int NP, int K, bool FULL, bool ENTROPY, int ROI_G, bool ZOUT>
#ifdef K1_WAVES
__attribute__((amdgpu_waves_per_eu(K1_WAVES, 8)))
#endif
__global__ __launch_bounds__(kK1Block) void mc_entropy_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ table,
                                                          double* __restrict__ h, float* __restrict__ z_out,
                                                          double* __restrict__ zero_fill, int64_t N, int C,
                                                          int n_mc_rt, double min_dist, double const_term,
                                                          double inv_n) {
  // XCD-aware order: consecutive workgroup ids go round-robin over the 8 XCDs (each with its own L2), so the
  // channel blocks of one image are given ids that are congruent mod 8 - the image's keep-flag table is then
  // fetched into ONE L2 (with the plain (block, image) grid up to 4 XCDs fetched it: +35 MB per 10 000 images).
  // (The product launch, mc_entropy_lut_kernel below, has no per-image table: the same order keeps the image's draws there.)
  const unsigned chunks = (unsigned)(C + kK1Block - 1) / kK1Block;
  const unsigned slot = blockIdx.x >> 3;
  const int c = (int)(slot % chunks) * kK1Block + threadIdx.x;
#pragma unroll 1
  for (int rep = 0; rep < K1_IMGS; ++rep) {
    const int64_t img = ((int64_t)(slot / chunks) * K1_IMGS + rep) * 8 + (blockIdx.x & 7);
    mc_entropy_item<HT, WT, NP, K, FULL, ENTROPY, ROI_G, ZOUT>(x, table, h, z_out, zero_fill, N, C, n_mc_rt, min_dist,
                                                              const_term, inv_n, img, c);
  }
}

// K1 from the draws and the geometry table (no K0 launch): the workgroup order of mc_entropy_kernel, which here keeps an
// image's 1 KB of draws in one L2 - each of the image's waves reads them and derives the same operands on its own.
// (six waves per SIMD as the table form: left alone the register allocator took 87 vector registers here, for the same code
// behind the drop layers that takes 75 there)
template <int HT, int WT, int NP, int K>
__attribute__((amdgpu_waves_per_eu(6, 8)))
__global__ __launch_bounds__(kK1Block) void mc_entropy_lut_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ rnd, int64_t rand_stride,
                                                              const float* __restrict__ lut, float gamma,
                                                              double* __restrict__ h, double* __restrict__ zero_fill,
                                                              int64_t N, int C, double min_dist, double const_term,
                                                              double inv_n) {
  const unsigned chunks = (unsigned)(C + kK1Block - 1) / kK1Block;
  const unsigned slot = blockIdx.x >> 3;
  const int c = (int)(slot % chunks) * kK1Block + threadIdx.x;
#pragma unroll 1
  for (int rep = 0; rep < K1_IMGS; ++rep) {
    const int64_t img = ((int64_t)(slot / chunks) * K1_IMGS + rep) * 8 + (blockIdx.x & 7);
    mc_entropy_item<HT, WT, NP, K, true, true, 0, false, true>(x, lut, h, nullptr, zero_fill, N, C, NP, min_dist, const_term,
                                                               inv_n, img, c, rnd, rand_stride, gamma);
  }
}

// The entropy launch.  The 4x4 maps have an instantiation without the z_out stores, taken when the caller passes no
// z_out (the product path).  The other maps keep the one kernel with its run-time test, which their code needs between
// the drop layers: without it the 7x7 form held two layers' quotients (200 vector registers, 64 scalar registers spilled
// to lanes) and the 2x2 x 32 form, one trip of 32 layers, requested all its flags at once (228 lane moves).
template <int HT, int WT, int NP, int K, bool FULL, int ROI_G>
void launch_mc_entropy(unsigned grid, hipStream_t s, const float* x, const float* table, double* h, float* z_out,
                       double* zero_fill, int64_t N, int C, int n_mc, double min_dist, double ct, double inv_n) {
  auto go = [&](auto kernel) {
    if constexpr (ROI_G == 0)
      RUNIA_LAUNCH_TIMED(kernel, grid, kK1Block, 0, s, x, table, h, z_out, zero_fill, N, C, n_mc, min_dist, ct, inv_n);
    else
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kK1Block), 0, s, x, table, h, z_out, zero_fill, N, C, n_mc, min_dist, ct,
                         inv_n);
  };
  if constexpr (HT == 4 && WT == 4) {
    if (!z_out) return go(mc_entropy_kernel<HT, WT, NP, K, FULL, true, ROI_G, false>);
  }
  go(mc_entropy_kernel<HT, WT, NP, K, FULL, true, ROI_G, true>);
}

template <int HH, int WW, int NPP>
void launch_mask(const float* rnd, int64_t rand_image_stride, float* table, int64_t N, int n_mc, float gamma,
                 int block_size, int identity, int sort_layers, uint64_t seed, int64_t first_image, int redraw,
                 hipStream_t s) {
  static_assert(HH * WW <= 64, "mc_mask_bits_kernel holds a drop layer in one 64-bit word");
  const unsigned grid = (unsigned)((N + kMaskBitsWaves - 1) / kMaskBitsWaves);
  if (redraw)  // throughput mode, opt-in: its own instantiation, so that the common launch carries neither the check nor the code
    mc_mask_bits_kernel<HH, WW, NPP, true><<<grid, 64 * kMaskBitsWaves, 0, s>>>(rnd, rand_image_stride, table, N, n_mc, gamma,
                                                                              block_size, identity, sort_layers, seed, first_image);
  else
    mc_mask_bits_kernel<HH, WW, NPP, false><<<grid, 64 * kMaskBitsWaves, 0, s>>>(rnd, rand_image_stride, table, N, n_mc, gamma,
                                                                               block_size, identity, sort_layers, seed, first_image);
}

// explicit draws of the counter generator, [N, n_mc, H, W] (tests; callers that want the values themselves)
__global__ void mc_draws_kernel(float* __restrict__ out, int64_t N, int per_image, uint64_t seed, int64_t first_image) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * per_image) return;
  const int64_t img = i / per_image;
  out[i] = runia_philox::draw(seed, (uint64_t)(first_image + img), (int)(i - img * per_image));
}
}  // namespace

extern "C" size_t runia_mc_entropy_workspace_bytes(int64_t N, int H, int W, int n_mc) {
  if (N <= 0 || H <= 0 || W <= 0 || n_mc <= 0) return 0;
  return (size_t)N * (size_t)n_mc * (size_t)(H * W + 2) * sizeof(float);
}

// K1's grid (the workgroup order of mc_entropy_kernel): groups of 8 images, K1_IMGS per workgroup, x the channel blocks
static unsigned k1_grid(int64_t N, int C) {
  return (unsigned)((((N + 7) / 8 + K1_IMGS - 1) / K1_IMGS) * 8 * ((C + kK1Block - 1) / kK1Block));
}

// ---- shapes.  The sampler exists for exactly these (H, W, register samples NP, k).  n_mc in (NP/2, NP] takes the NP
// instantiation: the FULL one when n_mc == NP, else the one with a run-time n_mc.  The list feeds the shape query and every
// dispatch, so `supported` can never promise a shape an entry point has no kernel for.
#define RUNIA_MCE_SHAPES(F) \
  F(4, 4, 16, 5) F(4, 4, 32, 5) F(4, 4, 8, 5) F(2, 2, 16, 5) F(2, 2, 32, 5) F(7, 7, 16, 5) F(7, 7, 32, 5) F(8, 8, 16, 5) F(8, 8, 32, 5)

// The same for roi_align folded into K1's load, with the samples per bin side G (= sampling_ratio).  Everything else
// (adaptive sampling - ratio <= 0 - has a per-ROI sample count; 4x4 / 8x8 bins with one sample; n_mc <= 8) goes through
// runia_roi_align_f32 + runia_mc_entropy_f32, same bits.
#define RUNIA_ROI_MCE_SHAPES(X)                                                                                    \
  X(7, 7, 16, 5, 2) X(7, 7, 32, 5, 2) X(7, 7, 16, 5, 1) X(7, 7, 32, 5, 1)                                          \
  X(4, 4, 16, 5, 2) X(4, 4, 32, 5, 2) X(8, 8, 16, 5, 2) X(8, 8, 32, 5, 2)

template <int V> using int_c = std::integral_constant<int, V>;

// f(H, W, NP, K, full) for the list entry that holds the shape - its numbers as int_c constants, full = std::bool_constant<
// n_mc == NP> - and 1; no call and 0 when no entry does.  any_k: for K0, which has no k and takes the entry of (H, W, n_mc)
// whatever its k (a flag, not a value of k: the shape query has to answer for every int).
template <class F>
int mc_for_shape(int H, int W, int n_mc, int k, F&& f, bool any_k = false) {
#define RUNIA_MCE(HH, WW, NPP, KK)                                                                 \
  if (H == HH && W == WW && n_mc <= NPP && n_mc > NPP / 2 && (k == KK || any_k)) {                \
    if (n_mc == NPP) f(int_c<HH>{}, int_c<WW>{}, int_c<NPP>{}, int_c<KK>{}, std::true_type{});     \
    else f(int_c<HH>{}, int_c<WW>{}, int_c<NPP>{}, int_c<KK>{}, std::false_type{});                \
    return 1;                                                                                      \
  }
  RUNIA_MCE_SHAPES(RUNIA_MCE)
#undef RUNIA_MCE
  return 0;
}

template <class F>  // f(PH, PW, NP, K, G, full)
int roi_mc_for_shape(int PH, int PW, int n_mc, int k, int sampling_ratio, F&& f) {
#define RUNIA_ROI_MCE(HH, WW, NPP, KK, GG)                                                                    \
  if (PH == HH && PW == WW && n_mc <= NPP && n_mc > NPP / 2 && k == KK && sampling_ratio == GG) {             \
    if (n_mc == NPP) f(int_c<HH>{}, int_c<WW>{}, int_c<NPP>{}, int_c<KK>{}, int_c<GG>{}, std::true_type{});   \
    else f(int_c<HH>{}, int_c<WW>{}, int_c<NPP>{}, int_c<KK>{}, int_c<GG>{}, std::false_type{});              \
    return 1;                                                                                                 \
  }
  RUNIA_ROI_MCE_SHAPES(RUNIA_ROI_MCE)
#undef RUNIA_ROI_MCE
  return 0;
}

// 4x4 maps with 6 ... 32 samples; 9 ... 32 samples (32 = the reference's default mcd_samples_nro, evaluation/entropy.py:41)
// on the maps RoI-align produces (7x7), 8x8 and 2x2; the k-th neighbour needs k < n_mc
extern "C" int runia_mc_entropy_supported(int H, int W, int n_mc, int k) {
  return k < n_mc && mc_for_shape(H, W, n_mc, k, [](auto...) {});
}

extern "C" int runia_roi_mc_entropy_supported(int PH, int PW, int n_mc, int k, int sampling_ratio) {
  return  // (the ROIs' keep-flag table comes from the plain sampler's launch)
      runia_mc_entropy_supported(PH, PW, n_mc, k) && roi_mc_for_shape(PH, PW, n_mc, k, sampling_ratio, [](auto...) {});
}

// ---- refusals: two checks.  Which code wins when two things are wrong at once is part of each entry point's contract
// (tests/test_sampler_host_contract.py): the entry points that build their own table answer an unsupported shape before they
// look at the workspace (they leave it to the table launch), the ones that are handed a workspace look at it first.
constexpr int64_t kMaxImages = 65535;  // images (ROIs) of one call; callers slice above it
constexpr int kNoArg = 1;              // what an entry point without a C, block_size or k passes for it

// (1) The scalar arguments and, for N > 0 and if `has_ws`, room for the keep-flag table in the workspace.  N == 0 is RUNIA_OK
// here and an early return for the caller.
static int mc_args_ok(int64_t N, int C, int H, int W, int n_mc, int block_size, int k, bool has_ws = false,
                      const void* ws = nullptr, size_t ws_bytes = 0) {
  if (N < 0 || N > kMaxImages || C <= 0 || H <= 0 || W <= 0 || n_mc < 2 || n_mc > kMaxMC || block_size < 1 || k < 1 || k >= n_mc)
    return RUNIA_E_INVALID;
  const bool refused = ws_refused(ws, ws_bytes, runia_mc_entropy_workspace_bytes(N, H, W, n_mc), 16);
  return (N > 0 && has_ws && refused) ? RUNIA_E_WORKSPACE : RUNIA_OK;
}

// (2) The operands of a K1 launch on N > 0 maps: input and output, a shape with a kernel, and x on 16 bytes where a map is
// read with 16-byte loads.  Callers without these: runia_mc_stack_f32 + runia_kl_entropy_per_dim_f32.
static bool k1_operands_ok(const float* x, const void* out, int H, int W, int n_mc, int k) {
  return x && out && runia_mc_entropy_supported(H, W, n_mc, k) && ((((uintptr_t)x) & 15) == 0 || (H * W) % 4 != 0);
}

static int mc_mask_table(const float* rnd, int64_t rand_image_stride, void* workspace, size_t workspace_bytes,
                         int64_t N, int H, int W, int n_mc, double drop_prob, int block_size, int sort_layers,
                         runia_stream_t stream, bool counter = false, uint64_t seed = 0, int64_t first_image = 0,
                         int redraw = 0) {
  if (int rc = mc_args_ok(N, kNoArg, H, W, n_mc, block_size, kNoArg, true, workspace, workspace_bytes)) return rc;
  if (N == 0) return RUNIA_OK;
  const int identity = (drop_prob == 0.0);
  if (!identity && !rnd && !counter) return RUNIA_E_INVALID;
  if (counter) rnd = nullptr;
  float* table = reinterpret_cast<float*>(workspace);
  const float gamma = (float)(drop_prob / (double)(block_size * block_size));
  hipStream_t s = as_stream(stream);
  if (!mc_for_shape(H, W, n_mc, 0, [&](auto hh, auto ww, auto np, auto, auto) {
        launch_mask<hh, ww, np>(rnd, rand_image_stride, table, N, n_mc, gamma, block_size, identity, sort_layers, seed,
                                first_image, redraw, s);
      }, /*any_k=*/true))
    return RUNIA_E_INVALID;
  return runia_check_launch();
}

extern "C" int runia_mc_mask_table_f32(const float* rnd, int64_t rand_image_stride, void* workspace,
                                       size_t workspace_bytes, int64_t N, int H, int W, int n_mc, double drop_prob,
                                       int block_size, runia_stream_t stream) {
  return mc_mask_table(rnd, rand_image_stride, workspace, workspace_bytes, N, H, W, n_mc, drop_prob, block_size, 1,
                       stream);
}

// MCSamplerModule.forward alone (the samples, in the order of the draws) on the table path: the keep-flag table is
// left unsorted and K1 stops after the sampler.  Same bits as runia_mc_stack_f32.
extern "C" int runia_mc_stack_table_f32(const float* x, const float* rnd, int64_t rand_image_stride, float* z,
                                        void* workspace, size_t workspace_bytes, int64_t N, int C, int H, int W,
                                        int n_mc, double drop_prob, int block_size, runia_stream_t stream) {
  if (int rc = mc_args_ok(N, C, H, W, n_mc, kNoArg, kNoArg, true, workspace, workspace_bytes)) return rc;  // block_size: below
  if (N == 0) return RUNIA_OK;
  if (!k1_operands_ok(x, z, H, W, n_mc, 5)) return RUNIA_E_INVALID;
  if (int rc = mc_mask_table(rnd, rand_image_stride, workspace, workspace_bytes, N, H, W, n_mc, drop_prob,
                             block_size, 0, stream))
    return rc;
  const float* table = reinterpret_cast<const float*>(workspace);
  hipStream_t s = as_stream(stream);
  if (!mc_for_shape(H, W, n_mc, 5, [&](auto hh, auto ww, auto np, auto kk, auto full) {
        mc_entropy_kernel<hh, ww, np, kk, full, false, 0, true><<<k1_grid(N, C), kK1Block, 0, s>>>(
            x, table, nullptr, z, nullptr, N, C, n_mc, 0.0, 0.0, 0.0);
      }))
    return RUNIA_E_INVALID;
  return runia_check_launch();
}

extern "C" int runia_mc_entropy_from_table_f32(const float* x, const void* workspace, size_t workspace_bytes,
                                               double* h, float* z_out, double* zero_fill, int64_t N, int C,
                                               int H, int W, int n_mc, int k, double min_dist,
                                               runia_stream_t stream) {
  if (int rc = mc_args_ok(N, C, H, W, n_mc, kNoArg, k, true, workspace, workspace_bytes)) return rc;
  if (N == 0) return RUNIA_OK;
  if (!k1_operands_ok(x, h, H, W, n_mc, k)) return RUNIA_E_INVALID;
  const float* table = reinterpret_cast<const float*>(workspace);
  const double ct = digamma_diff(n_mc, k), inv_n = 1.0 / (double)n_mc;
  hipStream_t s = as_stream(stream);
  if (!mc_for_shape(H, W, n_mc, k, [&](auto hh, auto ww, auto np, auto kk, auto full) {
        launch_mc_entropy<hh, ww, np, kk, full, 0>(k1_grid(N, C), s, x, table, h, z_out, zero_fill, N, C, n_mc, min_dist, ct,
                                                   inv_n);
      }))
    return RUNIA_E_INVALID;
  return runia_check_launch();
}

extern "C" int runia_mc_entropy_f32(const float* x, const float* rnd, int64_t rand_image_stride, double* h,
                                    float* z_out, double* zero_fill, void* workspace, size_t workspace_bytes,
                                    int64_t N, int C, int H, int W, int n_mc, double drop_prob, int block_size,
                                    int k, double min_dist, runia_stream_t stream) {
  // everything that does not need the workspace is refused before anything is launched; the table launch checks the rest
  if (int rc = mc_args_ok(N, C, H, W, n_mc, block_size, k)) return rc;
  if (N == 0) return RUNIA_OK;
  if (!k1_operands_ok(x, h, H, W, n_mc, k)) return RUNIA_E_INVALID;
  if (drop_prob != 0.0 && !rnd) return RUNIA_E_INVALID;
  if (int rc = runia_mc_mask_table_f32(rnd, rand_image_stride, workspace, workspace_bytes, N, H, W, n_mc, drop_prob,
                                       block_size, stream))
    return rc;
  return runia_mc_entropy_from_table_f32(x, workspace, workspace_bytes, h, z_out, zero_fill, N, C, H, W, n_mc, k,
                                         min_dist, stream);
}

// ---- the product launch without K0: draws + geometry table -> entropies ------------------------------------------------
extern "C" size_t runia_mc_flag_lut_bytes(int H, int W, int block_size) {
  if (H != 4 || W != 4 || block_size < 1) return 0;
  return kLutRecords * kLutRecDwords * sizeof(uint32_t);
}

extern "C" int runia_mc_flag_lut_fill(void* host_out, size_t bytes, int H, int W, int block_size) {
  const size_t need = runia_mc_flag_lut_bytes(H, W, block_size);
  if (need == 0 || !host_out || (((uintptr_t)host_out) & 3) != 0) return RUNIA_E_INVALID;
  if (bytes < need) return RUNIA_E_WORKSPACE;
  flag_lut_fill_4x4(reinterpret_cast<uint32_t*>(host_out), block_size);
  return RUNIA_OK;
}

extern "C" int runia_mc_entropy_lut_supported(int H, int W, int n_mc, int k, int block_size) {
  return H == 4 && W == 4 && n_mc == 16 && k == 5 && block_size >= 1;
}

extern "C" int runia_mc_entropy_lut_f32(const float* x, const float* rnd, int64_t rand_image_stride, const void* lut,
                                        size_t lut_bytes, double* h, double* zero_fill, int64_t N, int C, int H, int W,
                                        int n_mc, double drop_prob, int block_size, int k, double min_dist,
                                        runia_stream_t stream) {
  if (rand_image_stride < 0 || !runia_mc_entropy_lut_supported(H, W, n_mc, k, block_size)) return RUNIA_E_INVALID;
  if (!(drop_prob > 0.0)) return RUNIA_E_INVALID;  // no drop layers: the identity table of runia_mc_entropy_f32
  if (int rc = mc_args_ok(N, C, H, W, n_mc, block_size, k)) return rc;
  if (N == 0) return RUNIA_OK;
  if (!rnd || !k1_operands_ok(x, h, H, W, n_mc, k)) return RUNIA_E_INVALID;
  if (ws_refused(lut, lut_bytes, runia_mc_flag_lut_bytes(H, W, block_size), 4)) return RUNIA_E_WORKSPACE;
  const float gamma = (float)(drop_prob / (double)(block_size * block_size));
  const double ct = digamma_diff(n_mc, k), inv_n = 1.0 / (double)n_mc;
  RUNIA_LAUNCH_TIMED((mc_entropy_lut_kernel<4, 4, 16, 5>), k1_grid(N, C), kK1Block, 0, as_stream(stream), x, rnd,
                     rand_image_stride, reinterpret_cast<const float*>(lut), gamma, h, zero_fill, N, C, min_dist, ct, inv_n);
  return runia_check_launch();
}

// ---- ROI source (config 4): roi_align folded into K1's load ------------------------------------------------------------
struct RoiMcPlan { float* masks; size_t masks_bytes; char* tab; };  // the ROIs' keep-flag table (256-byte slot) | their sample table
static RoiMcPlan roi_mc_plan(WsWalk& w, int64_t K, int PH, int PW, int n_mc, int sampling_ratio) {
  RoiMcPlan p;
  p.masks = w.take<float>(runia_mc_entropy_workspace_bytes(K, PH, PW, n_mc) / sizeof(float), 256);
  p.masks_bytes = w.used();
  p.tab = w.take<char>(runia_roi_sample_table_bytes(K, PH, PW, sampling_ratio));
  return p;
}
extern "C" size_t runia_roi_mc_entropy_workspace_bytes(int64_t K, int PH, int PW, int n_mc, int sampling_ratio) {
  if (K <= 0 || sampling_ratio < 1) return 0;
  return ws_bytes([&](WsWalk& w) { roi_mc_plan(w, K, PH, PW, n_mc, sampling_ratio); });
}
extern "C" int runia_roi_mc_entropy_f32(const float* feat_nhwc, const float* boxes, const int* batch_idx, const float* rnd,
                                        int64_t rand_image_stride, double* h, float* z_out, void* workspace,
                                        size_t workspace_bytes, int64_t K, int64_t B, int C, int H, int W, int PH, int PW,
                                        double spatial_scale, int sampling_ratio, int aligned, int n_mc, double drop_prob,
                                        int block_size, int k, double min_dist, runia_stream_t stream) {
  if (B <= 0) return RUNIA_E_INVALID;
  if (int rc = mc_args_ok(K, C, H, W, n_mc, block_size, k)) return rc;  // (H, W: the feature map's here)
  if (K == 0) return RUNIA_OK;
  if (!feat_nhwc || !boxes || !h || (B > 1 && !batch_idx)) return RUNIA_E_INVALID;
  if (!runia_roi_mc_entropy_supported(PH, PW, n_mc, k, sampling_ratio)) return RUNIA_E_INVALID;
  if ((int64_t)H * W * C * 4 >= ((int64_t)1 << 30)) return RUNIA_E_INVALID;  // one image's map behind a 32-bit buffer (RUNIA_ROI_FUSED_MAX_IMAGE_BYTES)
  if (drop_prob != 0.0 && !rnd) return RUNIA_E_INVALID;
  WsWalk w(workspace);
  const RoiMcPlan plan = roi_mc_plan(w, K, PH, PW, n_mc, sampling_ratio);
  if (ws_refused(workspace, workspace_bytes, w.used(), 16)) return RUNIA_E_WORKSPACE;
  const size_t masks = plan.masks_bytes;
  if (int rc = runia_mc_mask_table_f32(rnd, rand_image_stride, workspace, masks, K, PH, PW, n_mc, drop_prob, block_size, stream))
    return rc;
  char* tab = plan.tab;
  hipStream_t s = as_stream(stream);
  if (int rc = runia_roi_sample_table(feat_nhwc, boxes, batch_idx, tab, workspace_bytes - masks, K, B, C, H, W, PH, PW,
                                      spatial_scale, sampling_ratio, aligned, s))
    return rc;
  const float* table = plan.masks;
  const float* src = reinterpret_cast<const float*>(tab);  // the RoiSource at the head of the sample table
  const double ct = digamma_diff(n_mc, k), inv_n = 1.0 / (double)n_mc;
  if (!roi_mc_for_shape(PH, PW, n_mc, k, sampling_ratio, [&](auto hh, auto ww, auto np, auto kk, auto gg, auto full) {
        launch_mc_entropy<hh, ww, np, kk, full, gg>(k1_grid(K, C), s, src, table, h, z_out, nullptr, K, C, n_mc, min_dist, ct,
                                                    inv_n);
      }))
    return RUNIA_E_INVALID;
  return runia_check_launch();
}

// ---- throughput mode: the DropBlock draws come from the counter generator inside K0 (philox.hpp) ----------------
extern "C" int runia_mc_draws_f32(float* out, int64_t N, int n_mc, int H, int W, uint64_t seed, int64_t first_image,
                                  runia_stream_t stream) {
  if (N < 0 || n_mc < 1 || H <= 0 || W <= 0 || first_image < 0 || (int64_t)n_mc * H * W > (1 << 20))
    return RUNIA_E_INVALID;
  if (N == 0) return RUNIA_OK;
  if (!out) return RUNIA_E_INVALID;
  const int64_t total = N * n_mc * H * W;
  if ((total + 255) / 256 > 0x7fffffffLL) return RUNIA_E_INVALID;
  mc_draws_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(out, N, n_mc * H * W, seed,
                                                                                first_image);
  return runia_check_launch();
}

extern "C" int runia_mc_mask_table_counter_f32(uint64_t seed, int64_t first_image, void* workspace,
                                               size_t workspace_bytes, int64_t N, int H, int W, int n_mc,
                                               double drop_prob, int block_size, int redraw_dead_layers,
                                               runia_stream_t stream) {
  if (first_image < 0) return RUNIA_E_INVALID;
  return mc_mask_table(nullptr, 0, workspace, workspace_bytes, N, H, W, n_mc, drop_prob, block_size, 1, stream, true,
                       seed, first_image, redraw_dead_layers ? 1 : 0);
}

extern "C" int runia_mc_entropy_counter_f32(const float* x, uint64_t seed, int64_t first_image, double* h,
                                            float* z_out, double* zero_fill, void* workspace, size_t workspace_bytes,
                                            int64_t N, int C, int H, int W, int n_mc, double drop_prob,
                                            int block_size, int k, double min_dist, int redraw_dead_layers,
                                            runia_stream_t stream) {
  if (first_image < 0) return RUNIA_E_INVALID;
  if (int rc = mc_args_ok(N, C, H, W, n_mc, block_size, k)) return rc;
  if (N == 0) return RUNIA_OK;
  if (!k1_operands_ok(x, h, H, W, n_mc, k)) return RUNIA_E_INVALID;  // before anything is launched
  if (int rc = runia_mc_mask_table_counter_f32(seed, first_image, workspace, workspace_bytes, N, H, W, n_mc,
                                               drop_prob, block_size, redraw_dead_layers, stream))
    return rc;
  return runia_mc_entropy_from_table_f32(x, workspace, workspace_bytes, h, z_out, zero_fill, N, C, H, W, n_mc, k,
                                         min_dist, stream);
}
