"""Seeded cases, the f64 restatement and the f32 yardstick of the per-pixel Mahalanobis maps (csrc/pixel_features.hip,
runia_core_amd.inference.pixel_features).  No GPU is touched here: the yardstick is CPU torch, so that it is independent
of the GPU libraries.

A case is a feature map (G, C, h, w) whose pixels are drawn from K class Gaussians with one shared covariance: class
means offset from zero (+3: the expanded form |z|^2 - 2 z.mz + |mz|^2 cancels there), correlated noise with a chosen
condition number of the covariance, random labels with some ignore_index pixels, and a separate set of training rows from
the same generator on which the restatement fits the parameters the kernel is handed."""
from functools import lru_cache

import numpy as np
import scipy.linalg
import torch

IGNORE = 255
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

# (C, K, G, h, w): the tile (128 pixels), chunk (32 channels) and column-block (128 channels) edges, tiles that straddle
# images (3 x 129 pixels), more classes than one register group (33)
SCORE_SHAPES = ((1, 1, 1, 1, 1), (3, 2, 2, 5, 7), (31, 19, 1, 1, 127), (32, 19, 1, 1, 128), (33, 21, 3, 3, 43),
                (65, 33, 1, 16, 17), (96, 19, 1, 31, 67), (128, 2, 1, 8, 16), (256, 19, 1, 16, 24), (304, 33, 1, 8, 20))
CONDITIONS = (1e2, 1e6)


def store_exactly(x: np.ndarray, dt: str) -> np.ndarray:
    """f32 values that the narrower type holds exactly (f32: unchanged)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(TORCH_DT[dt]).to(torch.float32).numpy()


def fit_restatement(rows: np.ndarray, labels: np.ndarray, n_classes: int, ridge: float = 0.0) -> dict:
    """The definition in f64 NumPy: class means, pooled within-class covariance (divided by n, as sklearn's
    EmpiricalCovariance of the centred rows), its Cholesky factor L, W = L^-1, the centre m0 = global mean rounded to f32,
    mz_c = W (mu_c - m0).  A class without rows has NaN means and +inf offsets."""
    x = np.asarray(rows, dtype=np.float64)
    n, c = x.shape
    means = np.full((n_classes, c), np.nan)
    cov = np.zeros((c, c))
    for k in range(n_classes):
        xk = x[labels == k]
        if len(xk):
            means[k] = xk.mean(axis=0)
            d = xk - means[k]
            cov += d.T @ d
    cov /= n
    if ridge > 0.0:
        cov = cov + ridge * np.trace(cov) / c * np.eye(c)
    chol = np.linalg.cholesky(cov)
    w = scipy.linalg.solve_triangular(chol, np.eye(c), lower=True)
    m0 = x.mean(axis=0).astype(np.float32).astype(np.float64)
    mz = np.where(np.isnan(means), 0.0, means - m0) @ w.T
    mz[np.isnan(means).any(axis=1)] = np.inf
    return {"means": means, "cov": cov, "chol": chol, "W": w, "m0": m0, "mz": mz}


def f64_distances(features: np.ndarray, fit: dict) -> np.ndarray:
    """All K distances of every pixel in f64: (G, C, h, w) -> (G, K, h, w)."""
    g, c, h, w = features.shape
    x = np.asarray(features, dtype=np.float64).transpose(0, 2, 3, 1).reshape(-1, c)
    z = (x - fit["m0"]) @ fit["W"].T
    k = fit["mz"].shape[0]
    d = np.empty((x.shape[0], k))
    for cl in range(k):
        d[:, cl] = np.inf if np.isinf(fit["mz"][cl, 0]) else ((z - fit["mz"][cl]) ** 2).sum(axis=1)
    return d.reshape(g, h, w, k).transpose(0, 3, 1, 2)


def f32_composition(features: torch.Tensor, fit: dict) -> np.ndarray:
    """The yardstick: what a user composes from torch in f32 on the CPU - permute to rows, (x.float() - m0) @ W32.T, the
    difference form, (the caller takes the min) -> (G, K, h, w) f32."""
    g, c, h, w = features.shape
    m0 = torch.from_numpy(fit["m0"].astype(np.float32))
    w32 = torch.from_numpy(fit["W"].astype(np.float32))
    mz = torch.from_numpy(np.where(np.isinf(fit["mz"]), 0.0, fit["mz"]).astype(np.float32))
    x = features.cpu().float().permute(0, 2, 3, 1).reshape(-1, c)
    z = (x - m0) @ w32.T
    d = ((z[:, None, :] - mz[None]) ** 2).sum(-1)
    d[:, torch.from_numpy(np.isinf(fit["mz"][:, 0]))] = float("inf")
    return d.reshape(g, h, w, -1).permute(0, 3, 1, 2).contiguous().numpy()


def _generator(rng, c, k, cond):
    means = 3.0 + rng.standard_normal((k, c))
    q, _ = np.linalg.qr(rng.standard_normal((c, c)))
    s = np.logspace(0.0, -0.5 * np.log10(cond), c) if c > 1 else np.ones(1)  # singular values: cov has condition `cond`
    return means, (q * s) @ q.T


@lru_cache(maxsize=None)
def make_case(c, k, g, h, w, cond, dt="f32", seed=0):
    """-> dict: features (G, C, h, w) f32 holding values exact in `dt`, labels (G, h, w) int64 with ~5 % IGNORE, fit (the
    restatement on separate training rows), d64 (G, K, h, w), yard (G, K, h, w) f32.  Cached: computed once, shared, and
    not to be written to."""
    rng = np.random.default_rng(1000003 * seed + 7919 * c + 31 * k + g * h * w + int(np.log10(cond)))
    means, a = _generator(rng, c, k, cond)
    n_train = max(4 * c, 2000)
    tl = np.arange(n_train) % k
    train = means[tl] + rng.standard_normal((n_train, c)) @ a
    labels = rng.integers(0, k, size=(g, h, w))
    x = means[labels] + rng.standard_normal((g, h, w, c)) @ a
    labels = np.where(rng.random((g, h, w)) < 0.05, IGNORE, labels).astype(np.int64)
    features = store_exactly(x.transpose(0, 3, 1, 2), dt)
    fit = fit_restatement(train, tl, k)
    ft = torch.from_numpy(features)
    case = {"features": features, "labels": labels, "fit": fit, "d64": f64_distances(features, fit),
            "yard": f32_composition(ft, fit), "dtype": dt}
    return case


def nearest_with_gap(d64: np.ndarray):
    """f64 argmin over the classes and the relative gap between the two nearest classes (inf with one class)."""
    k = d64.shape[1]
    near = d64.argmin(axis=1)
    if k == 1:
        return near, np.full(near.shape, np.inf)
    two = np.sort(d64, axis=1)[:, :2]
    return near, (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)
