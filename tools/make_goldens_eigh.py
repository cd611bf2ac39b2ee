#!/usr/bin/env python3
"""Graded symmetric positive definite matrices with 60-digit eigenvalues: the fixture of the relative-accuracy tests of the
Jacobi eigen-solvers (csrc/eigh.hip, csrc/eigh_block.hip) and of ``device_fit.pinvh_device``.

``A = D H D``: ``H = X X^T / 3n`` (X standard normal (n, 3n), seeded) rescaled to unit diagonal - cond(H) is about 12 - and
``D = diag(10^(-5 perm(n) / (n - 1)))``, so the diagonal of A spans ten decades in a shuffled order; A is symmetrised.
Such a matrix is what unnormalised features of very different scale give as a covariance: badly conditioned (1e10 and
more) only through its scaling.  Demmel and Veselic (1992): Jacobi with a relative stopping rule finds EVERY eigenvalue
of such a matrix to ``O(n eps cond(H))`` relative accuracy, where a tridiagonalising solver is accurate relative to the
largest one only.

Every operation of the builder is an IEEE operation in a fixed order or is rounded correctly (math.fsum for the Gram
sums, mpmath for the powers of ten), so the matrices do not depend on the BLAS or the libm of the machine.

The references are computed by mpmath at 60 digits ON THE f64 MATRIX (whose entries are exact there) and rounded to f64:
``eigsy`` for the eigenvalues, ``inverse`` for the inverse of the n = 72 matrix.

Writes tests/golden/eigh_graded.npz (data only, loads with allow_pickle=False):
  a{n}  (n, n) f64   the matrix, n = 40 and 72 (72 pads to 128 in the blocked solver: four blocks, one of them all zero)
  w{n}  (n,)   f64   its eigenvalues, ascending
  inv72 (72, 72) f64 the inverse of a72

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_eigh.py
"""
from __future__ import annotations

import math
import os
import sys

sys.dont_write_bytecode = True

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "eigh_graded.npz")
SIZES = (40, 72)
INVERSE_OF = 72
SEED = 20240  # + n
DIGITS = 60


def graded_spd(n):
    """-> (A, H, d): A = diag(d) H diag(d) symmetrised, H with unit diagonal, d the shuffled scales 1 .. 1e-5."""
    import mpmath

    rng = np.random.default_rng(SEED + n)
    x = rng.standard_normal((n, 3 * n))
    perm = rng.permutation(n)
    h = np.empty((n, n))
    for i in range(n):
        for j in range(i, n):
            h[i, j] = h[j, i] = math.fsum(x[i] * x[j]) / (3 * n)
    s = np.sqrt(np.diag(h))
    h = h / s[:, None] / s[None, :]
    np.fill_diagonal(h, 1.0)
    h = (h + h.T) * 0.5
    with mpmath.workdps(DIGITS):
        d = np.array([float(mpmath.mpf(10) ** (mpmath.mpf(-5 * int(p)) / (n - 1))) for p in perm])
    a = d[:, None] * h * d[None, :]
    return (a + a.T) * 0.5, h, d


def _to_mp(a):
    import mpmath

    return mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in a])


def eigenvalues_60(a):
    import mpmath

    with mpmath.workdps(DIGITS):
        w = mpmath.eigsy(_to_mp(a), eigvals_only=True)
        return np.sort(np.array([float(v) for v in w]))


def inverse_60(a):
    import mpmath

    n = a.shape[0]
    with mpmath.workdps(DIGITS):
        inv = mpmath.inverse(_to_mp(a))
        return np.array([[float(inv[i, j]) for j in range(n)] for i in range(n)])


def build():
    out = {}
    for n in SIZES:
        a, _, _ = graded_spd(n)
        out[f"a{n}"] = a
        out[f"w{n}"] = eigenvalues_60(a)
        if n == INVERSE_OF:
            out[f"inv{n}"] = inverse_60(a)
    return out


if __name__ == "__main__":
    arrays = build()
    np.savez(OUT, **arrays)
    for k, v in arrays.items():
        print(k, v.shape, v.dtype)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
