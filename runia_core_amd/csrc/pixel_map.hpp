// A (G, C, h, w) feature map read where the model left it, for the kernels that multiply 128 consecutive pixels of the
// flattened G * h * w axis with a matrix on the f32 matrix cores (pixel_features.hip: the whitening matrix; pixel_knn.hip: the
// bank): the view through the strides, and the staging of a 32-channel x 128-pixel chunk of x - centre into LDS as
// Xs[channel][pixel] by a 256-thread workgroup, in one of three load forms that fill the same Xs with the same bits, and the
// staging of 128 rows x 32 columns of the matrix as Ws[row][34].
// Include after common.hpp and elem.hpp.
#pragma once

namespace {

constexpr int kTP = 128;    // pixels per workgroup
constexpr int kKCh = 32;    // channels per staged chunk
constexpr int kXP = 132;    // pitch of Xs: rows stay 16-byte aligned
constexpr int kWP = 34;     // pitch of Ws (nt_tile_f32.hpp's KP)
constexpr int kMaxC = 1024;

struct MapView {  // a (G, C, h, w) map through its strides; rows that follow one another are one long row (Wr = h * w)
  const void* x;
  int64_t sn, sc, sh, sw, HW, Wr, P;
  int C;
};

__device__ __forceinline__ int64_t pixel_offset(const MapView& v, int64_t p) {
  const int64_t g = p / v.HW, q = p - g * v.HW, hh = q / v.Wr, ww = q - hh * v.Wr;
  return g * v.sn + hh * v.sh + ww * v.sw;
}

// ---- staging ------------------------------------------------------------------------------------------------------------------
// How a workgroup reads its 32-channel x 128-pixel chunk (one per launch, picked on the host from the strides):
//   kLoadVec    w has unit stride (NCHW): four neighbouring pixels of a channel plane per 16- / 8-byte load
//   kLoadCLast  the channels have unit stride (channels_last): 16 neighbouring channels of a pixel per thread, 16-byte loads
//   kLoadElem   anything else (crops, odd bases): element loads through the strides
enum { kLoadVec = 0, kLoadElem = 1, kLoadCLast = 2 };

// X chunk: thread t owns the pixel group t & 31 (four neighbouring pixels) of the channel rows (t >> 5) + 8 i, i = 0 .. 3
template <class T, bool VEC>
__device__ __forceinline__ void load_x(const MapView& v, const int64_t (&off)[4], int nv, int k0, int tid, float (&xr)[16]) {
  typedef typename T::elem E;
  const E* x = static_cast<const E*>(v.x);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = k0 + i * 8 + (tid >> 5);
    const bool in = c < v.C && nv > 0;
    const int cc = c < v.C ? c : v.C - 1;  // (every load is issued: a row past C re-reads the last plane and is masked)
    float t[4];
    if constexpr (VEC) {
      const E* p = x + off[0] + (int64_t)cc * v.sc;
      if (nv > 0) {
        if constexpr (T::kBytes == 4) ld16<T>(p, t);
        else ld8<T>(p, t);
      } else {
        t[0] = t[1] = t[2] = t[3] = 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = j < nv ? widen(T{}, x[off[j] + (int64_t)cc * v.sc]) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) xr[4 * i + j] = (in && j < nv) ? t[j] : 0.f;
  }
}

__device__ __forceinline__ void store_x(const float (&xr)[16], float (*Xs)[kXP], const float* m0s, int k0, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i * 8 + (tid >> 5);
    const float m = m0s[k0 + row];  // 0 past C: the padding stays 0
    *reinterpret_cast<float4*>(&Xs[row][4 * (tid & 31)]) =
        make_float4(xr[4 * i] - m, xr[4 * i + 1] - m, xr[4 * i + 2] - m, xr[4 * i + 3] - m);
  }
}

// channels_last: thread t owns channels 16 (t & 1) .. + 15 of the chunk for pixel t >> 1
template <class T>
__device__ __forceinline__ void load_x_cl(const MapView& v, int64_t off, bool valid, int k0, int tid, float (&xr)[16]) {
  typedef typename T::elem E;
  const int kb = k0 + (tid & 1) * 16;
  const int kc = kb < v.C ? kb : 0;  // (a half past C reads nothing)
  const E* p = static_cast<const E*>(v.x) + off + kc;
  if (valid && kb + 16 <= v.C) {
#pragma unroll
    for (int i = 0; i < 16 / T::V; ++i) ld16<T>(p + i * T::V, xr + i * T::V);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) xr[i] = (valid && kb + i < v.C) ? widen(T{}, p[i]) : 0.f;
  }
}

__device__ __forceinline__ void store_x_cl(const float (&xr)[16], float (*Xs)[kXP], const float* m0s, int k0, int tid) {
  const int pix = tid >> 1, r0 = (tid & 1) * 16;
#pragma unroll
  for (int i = 0; i < 16; ++i) Xs[r0 + i][pix] = xr[i] - m0s[k0 + r0 + i];
}

// W chunk: rows j0 .. j0 + 127, columns k0 .. k0 + 31 of a row-major [rows, C] matrix, zero outside it
__device__ __forceinline__ void load_w(const float* __restrict__ W, int rows, int C, int j0, int k0, int tid, bool vec,
                                       float (&wr)[16]) {
  const int row = tid >> 1, half = tid & 1;
  const int j = j0 + row, kb = k0 + half * 16;
  const float* p = W + (int64_t)j * C + kb;
  if (j < rows && vec && kb + 16 <= C) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 t = reinterpret_cast<const float4*>(p)[i];
      wr[4 * i] = t.x; wr[4 * i + 1] = t.y; wr[4 * i + 2] = t.z; wr[4 * i + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) wr[i] = (j < rows && kb + i < C) ? p[i] : 0.f;
  }
}

__device__ __forceinline__ void store_w(const float (&wr)[16], float (*Ws)[kWP], int tid) {
  const int row = tid >> 1, half = tid & 1;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    *reinterpret_cast<float2*>(&Ws[row][half * 16 + 2 * i]) = make_float2(wr[2 * i], wr[2 * i + 1]);
}

// the four pixels (channels_last: the one pixel) thread `tid` of the workgroup at pixel p0 stages -> the number of them
// inside the map, their element offsets in `off`
template <int LOAD>
__device__ __forceinline__ int staged_pixels(const MapView& v, int64_t p0, int tid, int64_t (&off)[4]) {
  off[0] = off[1] = off[2] = off[3] = 0;
  if constexpr (LOAD == kLoadCLast) {
    const int64_t ps = p0 + (tid >> 1);
    const int nv = ps < v.P ? 1 : 0;
    off[0] = nv ? pixel_offset(v, ps) : 0;
    return nv;
  } else {
    const int64_t ps = p0 + 4 * (tid & 31);
    const int64_t left = v.P - ps;
    const int nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) off[j] = (LOAD == kLoadVec ? j == 0 && nv > 0 : j < nv) ? pixel_offset(v, ps + j) : 0;
    return nv;
  }
}

// ---- one lane, one class plane (pixel_calibration.hip, pixel_sml.hip) -----------------------------------------------------------
// the logits of class plane p for a lane's pixels: four neighbouring pixels in the vector form, one otherwise
template <class T, int LOAD>
__device__ __forceinline__ void load_px(const typename T::elem* p, float* x) {
  if constexpr (LOAD == kLoadVec) {
    if constexpr (T::kBytes == 4) ld16<T>(p, x);
    else ld8<T>(p, x);
  } else {
    x[0] = ld1<T>(p);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
constexpr int64_t kLim = 0x7fffffffll;

bool view_ok(int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc, int64_t sh, int64_t sw) {
  return G >= 0 && H >= 0 && W >= 0 && C >= 1 && G <= kLim && H <= kLim && W <= kLim && sn >= 0 && sc >= 0 && sh >= 0 &&
         sw >= 0 && (G == 0 || H * W == 0 || G * H * W <= (kLim << 6));
}

MapView make_view(const void* x, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc, int64_t sh, int64_t sw) {
  MapView v;
  v.x = x;
  v.sn = sn; v.sc = sc; v.sh = sh; v.sw = sw;
  v.HW = H * W;
  v.P = G * v.HW;
  v.C = (int)C;
  const bool flat = H == 1 || sh == W * sw;
  v.Wr = flat ? v.HW : W;
  if (flat) v.sh = 0;  // (hh is always 0)
  return v;
}

// four neighbouring pixels from a multiple of four of the flat pixel axis are one aligned load
bool view_allows_vec(const MapView& v, int64_t G, int64_t H, int elem_bytes) {
  auto ok = [](int64_t stride, int64_t extent) { return extent <= 1 || stride % 4 == 0; };
  const bool flat = v.Wr == v.HW;
  return v.sw == 1 && v.Wr % 4 == 0 && (flat || ok(v.sh, H)) && ok(v.sc, v.C) && ok(v.sn, G) &&
         reinterpret_cast<uintptr_t>(v.x) % (4 * elem_bytes) == 0;
}

// 16 neighbouring channels of a pixel are aligned 16-byte loads (T::V elements each)
bool view_allows_clast(const MapView& v, int64_t G, int64_t H, int elems_per_16) {
  auto ok = [&](int64_t stride, int64_t extent) { return extent <= 1 || stride % elems_per_16 == 0; };
  const bool flat = v.Wr == v.HW;
  return v.sc == 1 && v.C >= 16 && ok(v.sw, v.Wr) && (flat || ok(v.sh, H)) && ok(v.sn, G) &&
         reinterpret_cast<uintptr_t>(v.x) % 16 == 0;
}

}  // namespace
