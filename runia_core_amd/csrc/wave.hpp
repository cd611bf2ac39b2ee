// Wave-level (64 lanes) shuffle, reduce and scan primitives shared by the kernels.  Plain templates over the __shfl_*
// builtins; a payload of several fields travels as one small struct with one combining lambda.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

// ---- shuffles of any trivially copyable T of whole 32-bit words (double, uint64_t, small structs), word by word ----------
#define RUNIA_LANE_SHUFFLE(name, builtin)                                                                              \
  template <class T>                                                                                                   \
  __device__ __forceinline__ T name(const T& v, int o) {                                                               \
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "whole 32-bit words");                   \
    uint32_t w[sizeof(T) / 4];                                                                                         \
    __builtin_memcpy(w, &v, sizeof(T));                                                                                \
    _Pragma("unroll") for (unsigned i = 0; i < sizeof(T) / 4; ++i) w[i] = builtin(w[i], o, 64);                        \
    T r;                                                                                                               \
    __builtin_memcpy(&r, w, sizeof(T));                                                                                \
    return r;                                                                                                          \
  }
RUNIA_LANE_SHUFFLE(lane_xor, __shfl_xor)    // the value of lane ^ o
RUNIA_LANE_SHUFFLE(lane_up, __shfl_up)      // the value of lane - o (the lane's own below o)
RUNIA_LANE_SHUFFLE(lane_down, __shfl_down)  // the value of lane + o (the lane's own from 64 - o on)
#undef RUNIA_LANE_SHUFFLE

// ---- butterfly reduction: every lane of an aligned WIDTH-lane group gets op over the group --------------------------------
// The steps run from WIDTH / 2 down to 1 and form op(own, other): a floating-point site that adds in another order
// stays hand-written.
template <int WIDTH = 64, class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
  static_assert(WIDTH >= 1 && WIDTH <= 64 && (WIDTH & (WIDTH - 1)) == 0, "power-of-two group within the wave");
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v = op(v, lane_xor(v, o));
  return v;
}
template <int WIDTH = 64, class T>
__device__ __forceinline__ T wave_sum(T v) {
  return wave_reduce<WIDTH>(v, [](T a, T b) { return a + b; });
}
template <int WIDTH = 64, class T>
__device__ __forceinline__ T wave_max(T v) {
  return wave_reduce<WIDTH>(v, [](T a, T b) { return a > b ? a : b; });
}
template <int WIDTH = 64, class T>
__device__ __forceinline__ T wave_or(T v) {
  return wave_reduce<WIDTH>(v, [](T a, T b) { return a | b; });
}

__device__ __forceinline__ float wave_max_f32(float v) {  // fmaxf: a NaN entry is dropped
  return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); });
}
__device__ __forceinline__ float wave_sum_f32(float v) { return wave_sum(v); }
__device__ __forceinline__ double shfl_xor_f64(double v, int o) { return lane_xor(v, o); }

// (value, index) of a row maximum, first index on ties (np.argmax); a NaN entry never wins (fmaxf drops it as well)
constexpr int kNoIndex = 0x7fffffff;
__device__ __forceinline__ void best_take(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}
__device__ __forceinline__ void wave_best(float& bv, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v = lane_xor(bv, o);
    const int i = lane_xor(bi, o);
    best_take(bv, bi, v, i);
  }
}

// ---- inclusive Hillis-Steele scan over the wave's lanes: lane l gets op(v[0], ..., v[l]), combined as op(lower, own) ------
template <class T, class Op>
__device__ __forceinline__ T wave_scan_incl(T v, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = lane_up(v, o);
    if (lane >= o) v = op(y, v);
  }
  return v;
}

template <class T>  // the running sum of an arithmetic T
__device__ __forceinline__ T wave_scan_incl(T v) {
  return wave_scan_incl(v, [](T a, T b) { return a + b; });
}

// ---- exclusive scan over the THREADS threads of a (one-dimensional) workgroup, in thread order ---------------------------
// Returns op over the threads before this one (`identity` for thread 0) and, in `total`, op over all of them.  Every
// thread calls it.  wave_totals holds THREADS / 64 slots; there is exactly ONE barrier inside, between writing and
// reading them.  The caller owns the barrier that makes wave_totals reusable: one must lie between the return of a call
// and the next write of the same slots (the next call included).
template <int THREADS, class T, class Op>
__device__ __forceinline__ T block_scan_excl(T v, Op op, T identity, T* wave_totals, T& total) {
  static_assert(THREADS % 64 == 0, "whole waves");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_scan_incl(v, op);
  if (lane == 63) wave_totals[wave] = inc;
  T before = lane_up(inc, 1);  // the wave's own lanes below this one
  if (lane == 0) before = identity;
  __syncthreads();
  T waves_before = identity, all = identity;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const T t = wave_totals[w];
    if (w < wave) waves_before = op(waves_before, t);
    all = op(all, t);
  }
  total = all;
  return op(waves_before, before);
}
template <int THREADS, class T>  // the sum of an arithmetic T
__device__ __forceinline__ T block_scan_excl(T v, T* wave_totals, T& total) {
  return block_scan_excl<THREADS>(v, [](T a, T b) { return a + b; }, T(0), wave_totals, total);
}

// ---- sum over the THREADS threads of a (one-dimensional) workgroup by the LDS tree: part [THREADS] ------------------------
// Every thread calls it; the sum is in part[0] for every thread on return (a barrier closes every halving step).  The
// order is fixed - thread i adds thread i + o, o = THREADS / 2 down to 1 - so a sum has the same bits on every run.
template <int THREADS, class T>
__device__ __forceinline__ void block_tree_sum(T v, T* part) {
  static_assert((THREADS & (THREADS - 1)) == 0, "halving steps");
  T* mine = part + threadIdx.x;  // both reads of a step from one address: they stay one ds_read2_b64 down to o = 1
  *mine = v;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) *mine += mine[o];
    __syncthreads();
  }
}
