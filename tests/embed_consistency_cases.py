"""Inputs, the f64 restatement and the derived error bound of the embedding-consistency tests.

Inputs: a shared offset (about 3 per feature) plus unit-scale noise, rounded to the tested dtype; the reference reads those
exact values, so no centred norm is small.  The bound of a coverage entry is derived from the kernel's arithmetic, not measured:
    2 u + (d + 32) 2^-24 + 2^-22 max |x| / min |x - m|
- 2 u: what a relative error of u in every element of both operands moves a product of unit vectors by (sum_k |a_k b_k| <= 1);
  u = 2^-9 bf16, 2^-12 f16, 2^-24 f32.  One rounding to a 16-bit type errs by up to TWICE these u, so the kernel carries every
  16-bit operand as hi + lo and stays far inside;
- (d + 32) 2^-24: the f32 accumulation of d exact products in any order (d 2^-24), and in front of the rounding three f32
  roundings per operand - the subtraction, the inverse norm, the scaling - with room to spare (logit_lens_cases.py: the same forms);
- the centring term: the mean is used rounded to f32, which moves a centred token by <= 2^-24 |m| <= 2^-24 max |x|, its direction
  by twice that over its norm, and a cosine by the sum over its two operands; 0 with center=False.
A maximum moves by at most what its entries move, a mean of maxima likewise; ``|dw| <= 2 max(|dP|, |dR|)`` doubles it for the
similarity.
"""
import numpy as np
import torch

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
UNIT = {"f32": 2.0 ** -24, "f16": 2.0 ** -12, "bf16": 2.0 ** -9}


def coverage_ref(contents, center=True):
    """``(K, K)`` f64 coverage of one group's contents (a list of ``(n_i, d)`` f64 arrays) and the largest |x| / smallest
    non-zero |x - m| over its tokens."""
    k = len(contents)
    every = np.concatenate(contents)
    if np.isnan(every).any():
        return np.full((k, k), np.nan), 0.0
    m = every.mean(0) if center and len(every) else 0.0
    unit, ratio = [], 0.0
    for x in contents:
        c = x - m
        norm = np.linalg.norm(c, axis=1)
        unit.append(c / np.where(norm == 0, 1.0, norm)[:, None])
        if center and (norm > 0).any():
            ratio = max(ratio, 1.0 / norm[norm > 0].min())
    ratio *= max([np.linalg.norm(x, axis=1).max() for x in contents if len(x)], default=0.0)
    cov = np.empty((k, k))
    for i in range(k):
        for j in range(k):
            if len(unit[i]) == 0 or len(unit[j]) == 0:
                cov[i, j] = float(len(unit[i]) == len(unit[j]))
            else:
                cov[i, j] = (unit[i] @ unit[j].T).max(1).mean()
    return cov, ratio


def similarity_ref(cov):
    r = np.maximum(cov, 0.0)
    p = r.T
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(p + r == 0, 0.0, 2 * p * r / (p + r))
    if not np.isnan(cov).any():
        np.fill_diagonal(w, 1.0)
    return w


def reference(x, windows, k, dtype, center=True):
    """``coverage``, ``similarity`` ``(G, K, K)`` and ``bound`` ``(G,)`` (of a coverage entry) of host states x (G K, T, d)."""
    xs, d = x.double().numpy(), x.shape[-1]
    rows = [xs[r, s:s + n] for r, (s, n) in enumerate(windows)]
    cov, sim, bound = [], [], []
    for g in range(len(rows) // k):
        c, ratio = coverage_ref(rows[g * k:(g + 1) * k], center)
        cov.append(c)
        sim.append(similarity_ref(c))
        bound.append(2 * UNIT[dtype] + (d + 32) * 2.0 ** -24 + 2.0 ** -22 * ratio)
    return {"coverage": np.stack(cov), "similarity": np.stack(sim), "bound": np.array(bound)}


def make(seed, groups, k, n, d, dtype="bf16", ragged=True):
    """``(x, windows)``: host states ``(G K, T, d)`` of ``dtype`` and every row's ``[start, length]``; with ``ragged`` rows
    1 mod 4 hold half of ``n`` (at least one token) and rows 2 mod 4 none."""
    rng = np.random.default_rng([seed, groups, k, n, d])
    batch = groups * k
    ns = [(max(1, n // 2) if r % 4 == 1 else 0 if r % 4 == 2 else n) if ragged else n for r in range(batch)]
    x = rng.standard_normal((batch, n + 3, d)) + 3.0 * rng.standard_normal(d)
    return torch.from_numpy(x).to(DTYPES[dtype]), [[r % 3, v] for r, v in enumerate(ns)]


def worst_ratio(got, ref):
    """max |error| / bound over coverage and similarity (the latter against twice the bound); inf where only one is NaN."""
    worst = 0.0
    for name, scale in (("coverage", 1.0), ("similarity", 2.0)):
        g, r = got[name], ref[name]
        if (np.isnan(g) != np.isnan(r)).any():
            return np.inf
        err = np.where(np.isnan(r), 0.0, np.abs(g - r)) / (scale * ref["bound"][:, None, None])
        worst = max(worst, float(err.max()))
    return worst
