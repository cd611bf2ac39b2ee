// Ordering shared by the kernels: the integer image of a float whose unsigned order is the float's order, and the bitonic sort
// of a power-of-two array in LDS.  Plain templates; the key part also runs on the host (lib.hip, selective.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

// ---- ordered keys: f32 <-> uint32_t, f64 <-> uint64_t ------------------------------------------------------------------------
template <class T> using order_key_t = std::conditional_t<sizeof(T) == 4, uint32_t, uint64_t>;
template <class T> using order_value_t = std::conditional_t<sizeof(T) == 4, float, double>;

// ascending: negative -> all bits flipped, else the sign bit set.  By the bits alone: -0 directly below +0, a NaN with the sign
// bit clear above +inf, one with it set below -inf.  asc_value is the inverse.
template <class F>
__host__ __device__ __forceinline__ order_key_t<F> asc_key(F v) {
  typedef order_key_t<F> K;
  const K top = K(1) << (8 * sizeof(K) - 1), b = __builtin_bit_cast(K, v);
  return (b & top) ? ~b : (b | top);
}
template <class K>
__host__ __device__ __forceinline__ order_value_t<K> asc_value(K k) {
  constexpr K top = K(1) << (8 * sizeof(K) - 1);
  return __builtin_bit_cast(order_value_t<K>, (k & top) ? (k ^ top) : ~k);
}
// descending: the complement (larger value, smaller key)
template <class F> __host__ __device__ __forceinline__ order_key_t<F> desc_key(F v) { return ~asc_key(v); }
template <class K> __host__ __device__ __forceinline__ order_value_t<K> desc_value(K k) { return asc_value((K)~k); }
// asc_key of a value known to be >= +0 (a probability, a squared distance) skips the sign test; its inverse
__host__ __device__ __forceinline__ uint32_t asc_key_nonneg(float v) { return __builtin_bit_cast(uint32_t, v) | 0x80000000u; }
__host__ __device__ __forceinline__ float asc_value_nonneg(uint32_t k) { return __builtin_bit_cast(float, k & 0x7fffffffu); }

// -0 -> +0 for the sites where the two zeros are one value.  f32: every other value, a NaN's payload included, keeps its bits.
// f64: the add that these sites have always used; it also quiets a signalling NaN, and their keys reach the caller.
__host__ __device__ __forceinline__ float fold_zero(float v) { return v == 0.f ? 0.f : v; }
__host__ __device__ __forceinline__ double fold_zero(double v) { return v + 0.0; }
// a 64-bit key as a signed number of the same order (for a sort of int64), and back
__host__ __device__ __forceinline__ int64_t signed_view(uint64_t k) { return (int64_t)(k ^ 0x8000000000000000ull); }
__host__ __device__ __forceinline__ uint64_t unsigned_view(int64_t k) { return (uint64_t)k ^ 0x8000000000000000ull; }

// Descending f64 key of a score: the zeros folded, and every NaN - either sign, any payload - on ONE key, that of the positive
// quiet NaN: the smallest key in use, in front of +inf's.
constexpr uint64_t kNanKey = 0x0007ffffffffffffull;  // desc_key of 0x7ff8000000000000
__host__ __device__ __forceinline__ uint64_t desc_key_one_nan(double v) { return v != v ? kNanKey : desc_key(fold_zero(v)); }
// ... of a score of the OoD metrics (metrics.hip; bootstrap.hip sorts its signed view), through torch.sigmoid in its dtype first
template <typename T>
__device__ __forceinline__ uint64_t score_key(T v, bool squash) {
  if (squash) v = (T)1 / ((T)1 + exp(-v));
  return desc_key_one_nan((double)v);
}

// ---- bitonic sort of np2 (a power of two) slots in LDS by the nt threads of a group, this one being thread t of them ----------
// cx(lo, hi, up) compares slots lo < hi and leaves them ascending when `up`, descending otherwise.  Each of the np2 / 2 pairs of
// a step belongs to one thread; ONE __syncthreads() closes every step, so every thread of the workgroup makes the call with the
// same np2 (smaller groups sort their arrays side by side), after the caller's barrier behind filling the slots.  Elements
// must be totally ordered by cx: the network is not stable.
template <class CX>
__device__ __forceinline__ void lds_bitonic_sort(int np2, int t, int nt, CX cx) {
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int h = t; h < (np2 >> 1); h += nt) {
        const int lo = ((h & ~(j - 1)) << 1) | (h & (j - 1));
        cx(lo, lo | j, (lo & k) == 0);
      }
      __syncthreads();
    }
}
template <class W>  // one array of words compared by <
__device__ __forceinline__ void lds_bitonic_sort(W* s, int np2, int t, int nt) {
  lds_bitonic_sort(np2, t, nt, [s](int lo, int hi, bool up) {
    const W a = s[lo], b = s[hi];
    if ((a > b) == up) { s[lo] = b; s[hi] = a; }
  });
}
