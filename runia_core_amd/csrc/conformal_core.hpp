// What the conformal kernels share (conformal.hip: label scores, narrow sets, reduce; conformal_wide.hip: sets of rows of any
// width): the method and label descriptors, the softmax term, the score of a class from its normalised parts, and the 32-bit key
// whose ascending order is the order of the definitions.  Include after common.hpp.
#pragma once

namespace {

enum { kLac = 0, kAps = 1, kRaps = 2 };

struct Labels {
  const void* p;   // int32 or int64 [N]; NULL: no labels
  int is_i64, has_ignore;
  int64_t ignore;
};

struct Method {
  int kind;
  float beta, lam;
  int k_reg;
};

__device__ __forceinline__ int64_t label_at(const Labels& L, int64_t row) {
  return L.is_i64 ? static_cast<const int64_t*>(L.p)[row] : (int64_t) static_cast<const int32_t*>(L.p)[row];
}

// the class whose logit the row needs (0 for a row without one) and whether the row is scored against a label
__device__ __forceinline__ int row_class(const Labels& L, int64_t row, int64_t C, bool& used) {
  used = false;
  if (!L.p) return 0;
  const int64_t y = label_at(L, row);
  used = y >= 0 && y < C && !(L.has_ignore && y == L.ignore);
  return used ? (int)y : 0;
}

__device__ __forceinline__ float softmax_term(float x, float m, float beta) {
  return (x == -INFINITY) ? 0.f : exp_nonpos(beta * (x - m));
}

// s from the row's normalised parts: p of the class, B the mass ordered before it, rank 1-based
__device__ __forceinline__ float score_of(const Method& M, float p, float B, float u, int rank) {
  if (M.kind == kLac) return 1.f - p;
  const float s = B + u * p;
  if (M.kind == kAps) return s;
  const int over = rank - M.k_reg;
  return s + M.lam * (float)(over > 0 ? over : 0);
}

// uint32 key of a logit: ascending key order is descending logit order; -0 and +0 are equal logits
__device__ __forceinline__ uint32_t descending_key(float x) { return desc_key(fold_zero(x)); }
__device__ __forceinline__ float key_logit(uint32_t k) { return desc_value(k); }

static inline bool method_ok(int method, float beta, float lam, int k_reg) {
  return method >= kLac && method <= kRaps && beta > 0.f && beta < INFINITY && lam >= 0.f && lam < INFINITY && k_reg >= 0;
}

}  // namespace
