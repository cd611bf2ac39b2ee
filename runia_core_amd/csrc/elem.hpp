// The element layer of the kernels that read the caller's tensors where they lie, in f32, f16 or bf16: the dtype codes
// of the C ABI, one tag type per element type, the exact widening to f32, the rounding back (to nearest even, as torch's
// casts), the aligned 8- and 16-byte loads, the rows of a step table, and the host-side step from a run-time code to a
// tag.  A kernel is written once as `template <class T>` over the tags.  Include after common.hpp.
#pragma once

enum { kF32 = 0, kF16 = 1, kBF16 = 2 };  // `dtype` of runia_hip.h; _hip.ELEM_DTYPE_CODES on the Python side

static inline bool elem_dtype_ok(int dtype) { return dtype >= kF32 && dtype <= kBF16; }

// elem: the type in memory; V: elements per 16 bytes
struct F32 { typedef float elem; static constexpr int kBytes = 4, V = 4; };
struct F16 { typedef uint16_t elem; static constexpr int kBytes = 2, V = 8; };
struct BF16 { typedef uint16_t elem; static constexpr int kBytes = 2, V = 8; };

__device__ __forceinline__ float widen(F32, float v) { return v; }
__device__ __forceinline__ float widen(F16, uint16_t v) {
  _Float16 h;
  __builtin_memcpy(&h, &v, 2);
  return (float)h;
}
__device__ __forceinline__ float widen(BF16, uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

__device__ __forceinline__ float narrow(F32, float f) { return f; }
__device__ __forceinline__ uint16_t narrow(F16, float f) {  // round to nearest even (v_cvt_f16_f32)
  const _Float16 h = (_Float16)f;
  uint16_t v;
  __builtin_memcpy(&v, &h, 2);
  return v;
}
// the bits of a non-NaN f32 rounded to nearest even at bit 16: the bf16 value in the upper half
__device__ __forceinline__ uint32_t bf16_round_bits(uint32_t u) { return u + 0x7fffu + ((u >> 16) & 1u); }
__device__ __forceinline__ uint16_t narrow(BF16, float f) {  // round to nearest even; NaN -> the quiet NaN torch writes
  if (f != f) return 0x7fc0;
  return (uint16_t)(bf16_round_bits(__float_as_uint(f)) >> 16);
}

template <class T>
__device__ __forceinline__ float ld1(const typename T::elem* p) { return widen(T{}, *p); }

// 16 aligned bytes -> v[T::V]
template <class T>
__device__ __forceinline__ void ld16(const typename T::elem* p, float* v) {
  const uint4 r = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  if constexpr (T::V == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(w[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = widen(T{}, (uint16_t)(w[j] & 0xffffu));
      v[2 * j + 1] = widen(T{}, (uint16_t)(w[j] >> 16));
    }
  }
}

// 8 aligned bytes of a 16-bit type -> v[4]
template <class T>
__device__ __forceinline__ void ld8(const typename T::elem* p, float* v) {
  static_assert(T::kBytes == 2, "four elements in 8 bytes");
  const uint2 r = *reinterpret_cast<const uint2*>(p);
  v[0] = widen(T{}, (uint16_t)(r.x & 0xffffu));
  v[1] = widen(T{}, (uint16_t)(r.x >> 16));
  v[2] = widen(T{}, (uint16_t)(r.y & 0xffffu));
  v[3] = widen(T{}, (uint16_t)(r.y >> 16));
}

// ---- rows behind a step table (logits.hip, conformal_wide.hip) ----------------------------------------------------------------
struct StepDesc {  // one generation step: row b of it starts at ptr + b * row_stride elements
  int64_t ptr, row_stride;
};

// row b of a step (rows are addressed in bytes: `aligned` below is a property of the address), and element j of a row
template <class T>
__device__ __forceinline__ const char* step_row(const StepDesc& sd, int64_t b) {
  return reinterpret_cast<const char*>(sd.ptr) + b * sd.row_stride * T::kBytes;
}
template <class T>
__device__ __forceinline__ const typename T::elem* elem_at(const char* row, int64_t j) {
  return reinterpret_cast<const typename T::elem*>(row) + j;
}

// T::V consecutive logits from element j: one 16-byte load when the row is 16-byte aligned and all of them lie inside the
// row, element loads otherwise (-inf past V)
template <class T>
__device__ __forceinline__ void load_vec(const char* row, int64_t j, int64_t V, bool aligned, float* out) {
  if (aligned && j + T::V <= V) {
    ld16<T>(elem_at<T>(row, j), out);
  } else {
#pragma unroll
    for (int e = 0; e < T::V; ++e) out[e] = j + e < V ? ld1<T>(elem_at<T>(row, j + e)) : -__builtin_inff();
  }
}

// f(tag) for a code that elem_dtype_ok() accepted
template <class F>
static inline auto dispatch_elem(int dtype, F f) {
  switch (dtype) {
    case kF32: return f(F32{});
    case kF16: return f(F16{});
    default: return f(BF16{});
  }
}
