// The building blocks shared by the two-sided cyclic Jacobi eigen-solvers (eigh.hip, eigh_block.hip, eigen_score.hip,
// consistency.hip): the round-robin pairing, the rotation of one pair with its two threshold rules, the 2 x 2 block update
// and the whole sweep loop of a matrix that lives in LDS.  Plain functions; every one keeps the order of its
// floating-point operations fixed (the build has -ffp-contract=off), so a kernel's bits do not depend on which of them it
// is built from.  J = [[c, s], [-s, c]] in the (p, q) plane; identity = (1, 0).
#pragma once
#include "wave.hpp"

// pair j (0 <= j < m/2) of round t (0 <= t < m-1) of the circle method on m (even) players, p < q
__device__ __forceinline__ void tournament_pair(int m, int t, int j, int& p, int& q) {
  if (j == 0) {
    p = m - 1;
    q = t;
  } else {
    p = (t + j) % (m - 1);
    q = (t - j + (m - 1)) % (m - 1);
  }
  if (p > q) { const int s = p; p = q; q = s; }
}

// ---- rotation thresholds: a pair is rotated when |apq| > thr ------------------------------------------------------------
// Eigenvector form (eigh.hip).  Rotate when |apq| > 1e-17 sqrt|app aqq|: the relative rule, under which the small
// eigenvalues of a graded matrix AND their eigenvectors come out accurately (Demmel & Veselic 1992).  The absolute floor
// 1e-19 |A|_F joins it only where a diagonal entry of the pair is itself rounding noise (<= 1e-16 |A|_F: zero diagonals,
// the null space of a rank-deficient matrix - below the pinvh cut-off n eps max|w|), where the relative rule alone would
// chase noise.  With the floor on EVERY pair the eigenvalues stayed accurate (an off-diagonal entry enters them squared)
// but two small eigenvalues w kept a residue of 1e-19 |A|_F between them, their vectors mixed by that over their gap, and
// U diag(1/w) U^T of a matrix scaled over ten decades was off by 3e-10 where 1e-14 is to be had.
// (eigh_block.hip keeps this rule in its own squared form with a wider relative bound; the reason stands there.)
__device__ __forceinline__ double jacobi_thr_vectors(double app, double aqq, double anorm) {
  const double rel = 1e-17 * sqrt(fabs(app * aqq));
  const bool noise = fmin(fabs(app), fabs(aqq)) <= 1e-16 * anorm;
  return noise ? fmax(1e-19 * anorm, rel) : rel;
}
// Eigenvalue form (eigen_score.hip, consistency.hip): max(1e-19 |A|_F, 1e-17 sqrt|app aqq|) on every pair.  Only the
// eigenvalues are wanted to full accuracy there, and an entry left under the absolute floor enters them squared
// (consistency.hip accumulates its eigenvectors under this same rule).
__device__ __forceinline__ double jacobi_thr_values(double app, double aqq, double anorm) {
  return fmax(1e-19 * anorm, 1e-17 * sqrt(fabs(app * aqq)));
}

// (c, s) that annihilate apq; identity and `false` unless |apq| > thr (a NaN apq never rotates)
__device__ __forceinline__ bool jacobi_rotation(double app, double aqq, double apq, double thr, double& c, double& s) {
  if (fabs(apq) > thr) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(tt * tt + 1.0);
    s = tt * c;
    return true;
  }
  c = 1.0;
  s = 0.0;
  return false;
}

// N = J_a^T B J_b of the 2 x 2 block B = A[{pa, qa}, {pb, qb}]; `diagonal` (a == b): the rotated pair is annihilated by
// construction
__device__ __forceinline__ void jacobi_block(double ca, double sa, double cb, double sb, double b00, double b01, double b10,
                                             double b11, bool diagonal, double& n00, double& n01, double& n10,
                                             double& n11) {
  const double t00 = ca * b00 - sa * b10, t01 = ca * b01 - sa * b11;  // J_a^T B
  const double t10 = sa * b00 + ca * b10, t11 = sa * b01 + ca * b11;
  n00 = t00 * cb - t01 * sb;  // (J_a^T B) J_b
  n01 = t00 * sb + t01 * cb;
  n10 = t10 * cb - t11 * sb;
  n11 = t10 * sb + t11 * cb;
  if (diagonal) { n01 = 0.0; n10 = 0.0; }
}

// ---- cyclic Jacobi on G [k, k] (row-major, symmetric, k <= 64) in LDS, by the THREADS threads of the workgroup ------------
// Up to max_sweeps sweeps of m - 1 steps (m = k rounded up to even; the bye index of odd k leaves its partner untouched).
// A step: the first m/2 threads form the rotations of the step's pairs (eigenvalue form of the threshold, |G|_F taken once
// on entry), barrier, G <- J^T G J on the upper triangle of 2 x 2 pair blocks mirrored (G stays exactly symmetric) and,
// WITH_V, V <- V J on V [k, k] behind it without a barrier in between (the two passes touch different arrays), barrier.
// The loop stops after the first sweep that applies no rotation; returns whether it did so within max_sweeps.
// LDS of the caller: rot [64] (32 cosines, 32 sines), part [THREADS], flag [1].  G must be visible to all threads on entry.
template <int THREADS, bool WITH_V>
__device__ __forceinline__ bool jacobi_lds_sweeps(double* G, double* V, int k, int max_sweeps, double* rot, double* part,
                                                  int* flag) {
  const int tid = threadIdx.x;
  double* rot_c = rot;
  double* rot_s = rot + 32;
  double sq = 0.0;
  for (int idx = tid; idx < k * k; idx += THREADS) sq += G[idx] * G[idx];
  block_tree_sum<THREADS>(sq, part);
  const double anorm = sqrt(part[0]);
  const int m = (k + 1) & ~1, half = m / 2;
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    if (tid == 0) flag[0] = 0;
    __syncthreads();
    for (int t = 0; t < m - 1; ++t) {
      if (tid < half) {
        int p, q;
        tournament_pair(m, t, tid, p, q);
        double c = 1.0, s = 0.0;
        if (q < k) {
          const double app = G[p * k + p], aqq = G[q * k + q], apq = G[p * k + q];
          if (jacobi_rotation(app, aqq, apq, jacobi_thr_values(app, aqq, anorm), c, s)) flag[0] = 1;
        }
        rot_c[tid] = c;
        rot_s[tid] = s;
      }
      __syncthreads();
      for (int idx = tid; idx < half * half; idx += THREADS) {
        const int ka = idx / half, kb = idx - ka * half;
        if (ka > kb) continue;
        const double rac = rot_c[ka], ras = rot_s[ka], rbc = rot_c[kb], rbs = rot_s[kb];
        if (ras == 0.0 && rbs == 0.0) continue;
        int pa, qa, pb, qb;
        tournament_pair(m, t, ka, pa, qa);
        tournament_pair(m, t, kb, pb, qb);
        const bool qa_ok = qa < k, qb_ok = qb < k;
        const double b00 = G[pa * k + pb];
        const double b01 = qb_ok ? G[pa * k + qb] : 0.0;
        const double b10 = qa_ok ? G[qa * k + pb] : 0.0;
        const double b11 = (qa_ok && qb_ok) ? G[qa * k + qb] : 0.0;
        double n00, n01, n10, n11;
        jacobi_block(rac, ras, rbc, rbs, b00, b01, b10, b11, ka == kb, n00, n01, n10, n11);
        G[pa * k + pb] = n00;
        G[pb * k + pa] = n00;
        if (qb_ok) { G[pa * k + qb] = n01; G[qb * k + pa] = n01; }
        if (qa_ok) { G[qa * k + pb] = n10; G[pb * k + qa] = n10; }
        if (qa_ok && qb_ok) { G[qa * k + qb] = n11; G[qb * k + qa] = n11; }
      }
      if (WITH_V) {  // columns p and q of every row
        for (int idx = tid; idx < half * k; idx += THREADS) {
          const int ka = idx / k, r = idx - ka * k;
          const double c = rot_c[ka], s = rot_s[ka];
          if (s == 0.0) continue;
          int p, q;
          tournament_pair(m, t, ka, p, q);
          const double vp = V[r * k + p], vq = V[r * k + q];
          V[r * k + p] = c * vp - s * vq;
          V[r * k + q] = s * vp + c * vq;
        }
      }
      __syncthreads();
    }
    const int any = flag[0];
    __syncthreads();  // every thread has read the flag before thread 0 clears it for the next sweep
    if (!any) return true;
  }
  return false;
}
