// The arithmetic of one softmax row at a temperature 1 / beta, shared by the row pass (calibration.hip: a row is class-
// contiguous) and the pixel pass (pixel_calibration.hip: a row is the classes of one pixel, H * W elements apart).
// With m the row maximum, d_k = x_k - m and e_k = exp(beta d_k), a row is the four sums
//   S0 = sum e_k   S1 = sum e_k d_k   S2 = sum e_k d_k^2   Q = sum e_k^2          (p_k = e_k / S0)
// and the label's d_y:  conf = 1 / S0,  nll = log S0 - beta d_y,  brier = Q / S0^2 - 2 p_y + 1,  g = S1 / S0 - d_y,
// h = max(0, S2 / S0 - (S1 / S0)^2).  A class at -inf adds nothing; a NaN logit makes the row's outputs NaN.
// Include after common.hpp.
#pragma once

namespace {

struct Sums { float s0, s1, s2, q; };

struct RowVals { float conf, nll, brier, g, h; };  // conf = 1 / S0; the other four NaN for a row that is not scored

// e_k of one logit under the row maximum m (0 for a class at -inf)
__device__ __forceinline__ float class_exp(float x, float m, float beta) {
  return (x == -INFINITY) ? 0.f : exp_nonpos(beta * (x - m));
}

__device__ __forceinline__ void term(float x, float m, float beta, Sums& a) {
  const float d = x - m;
  const float e = (x == -INFINITY) ? 0.f : exp_nonpos(beta * d);
  a.s0 += e;
  a.q += e * e;
  const bool some = e != 0.f;  // (a NaN passes; e == 0 with d = -inf would be 0 * inf)
  const float ed = some ? e * d : 0.f;
  a.s1 += ed;
  a.s2 += some ? ed * d : 0.f;
}

// the sums of a maximum that moved up by delta > 0:  d' = d - delta,  e' = e exp(-beta delta).  No term cancels: S1 <= 0 <= S0, S2.
__device__ __forceinline__ void rescale(Sums& a, float delta, float beta) {
  const float f = exp_nonpos(-beta * delta);
  const float s1 = a.s1 - delta * a.s0;
  a.s2 = f * (a.s2 - 2.f * delta * a.s1 + delta * delta * a.s0);
  a.s1 = f * s1;
  a.s0 *= f;
  a.q *= f * f;
}

// the finished row: xy the label's logit (read only when `used`)
__device__ __forceinline__ RowVals finish_vals(float beta, float m, Sums a, float xy, bool used) {
  const float nan = __builtin_nanf("");
  if (a.s0 == 0.f) a.s0 = nan;  // a row of -inf has no softmax (torch: NaN)
  const float r = 1.f / a.s0;
  RowVals o = {r, nan, nan, nan, nan};
  if (used) {
    const float dy = xy - m, ay = beta * dy;
    const float py = (xy == -INFINITY) ? 0.f : exp_nonpos(ay) * r;
    const float mu = a.s1 * r, var = a.s2 * r - mu * mu;
    o.nll = logf(a.s0) - ay;
    o.brier = a.q * r * r - 2.f * py + 1.f;
    o.g = mu - dy;
    o.h = (var > 0.f || var != var) ? var : 0.f;
  }
  return o;
}

// b = clamp((int)ceilf(conf * (float)n_bins) - 1, 0, n_bins - 1); a NaN goes to bin 0 (and makes its conf_sum NaN)
__device__ __forceinline__ int conf_bin(float conf, int n_bins) {
  const float t = ceilf(conf * (float)n_bins);
  int b = (t == t) ? (int)fminf(fmaxf(t, -1.f), (float)n_bins) - 1 : 0;
  b = b < 0 ? 0 : b;
  return b > n_bins - 1 ? n_bins - 1 : b;
}

}  // namespace
