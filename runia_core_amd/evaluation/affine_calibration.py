"""Per-class calibration maps of a classifier fitted on the device: vector scaling and matrix scaling (Guo et al. 2017) and
Dirichlet calibration with the ODIR regulariser (Kull et al. 2019) - what a user reaches for when one temperature leaves the
class-wise calibration error high.

A row has logits ``x`` and a label ``y``; the map is ``q = softmax(W u + b)`` with

    vector     u = x                                        W = diag(w)
    matrix     u = x                                        W full C x C
    dirichlet  u = max(log_softmax(x), log FLT_MIN)         W full C x C

and the fit minimises the convex objective

    L(W, b) = mean_rows -log q_y + lam / (C (C - 1)) sum_{i != j} W_ij^2 + mu / C sum_j b_j^2

(the off-diagonal term is absent for ``vector`` and for ``C == 1``).  Everything that touches the ``[N, C]`` logits is one HIP
kernel (``csrc/affine_calibration.hip``): an evaluation of the objective and its gradient reads the logits once, runs both
small-C matrix products on the f32 matrix cores and writes nothing ``N x C``.  The optimiser is a plain L-BFGS in float64 on the
host, whose iteration is one parameter upload, one evaluation and one read-back of the small record.  There is no host
implementation: without a GPU the calls raise.  The definitions are restated in float64 in ``tests/affine_calibration_cases.py``.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .calibration import CalibrationResult, _logits_to_device, _prepare, _result_from_rows

__all__ = ["AffineCalibrator", "fit_affine_calibration", "lbfgs_minimize"]


def lbfgs_minimize(fun: Callable[[np.ndarray], Tuple[float, np.ndarray]], x0: np.ndarray, max_iter: int = 200, tol: float = 1e-6,
                   history: int = 10) -> Tuple[np.ndarray, float, int]:
    """Plain L-BFGS in float64 around ``fun(x) -> (f, grad)``: two-loop recursion over the last ``history`` pairs, Armijo
    backtracking (c1 = 1e-4, halving from a unit step; the first step is scaled to length <= 1).  It stops at
    ``max |grad| <= tol``, after ``max_iter`` iterations, or when no step along the direction gives a representable decrease.
    Returns ``(x, f, iterations)``.  A non-finite ``f`` at the start raises ``ValueError``."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    if not np.isfinite(f):
        raise ValueError("the objective is not finite at the starting point")
    pairs = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        if np.max(np.abs(g)) <= tol:
            n_iter -= 1
            break
        d = -g
        alphas = []
        for s, y, rho in reversed(pairs):
            a = rho * s.dot(d)
            alphas.append(a)
            d -= a * y
        if pairs:
            s, y, _ = pairs[-1]
            d *= s.dot(y) / y.dot(y)
        for (s, y, rho), a in zip(pairs, reversed(alphas)):
            d += (a - rho * y.dot(d)) * s
        slope = g.dot(d)
        if not slope < 0:  # (rounding in the pairs: fall back to the gradient)
            d, slope, pairs = -g, -g.dot(g), []
        t = 1.0 if pairs else 1.0 / max(1.0, float(np.linalg.norm(d)))
        moved = False
        for _ in range(60):
            x_new = x + t * d
            if np.array_equal(x_new, x):
                break
            f_new, g_new = fun(x_new)
            if np.isfinite(f_new) and f_new <= f + 1e-4 * t * slope and f_new < f:
                moved = True
                break
            t *= 0.5
        if not moved:
            n_iter -= 1
            break
        s, y = x_new - x, g_new - g
        sy = s.dot(y)
        if sy > 1e-10 * np.linalg.norm(s) * np.linalg.norm(y):
            pairs = (pairs + [(s, y, 1.0 / sy)])[-history:]
        x, f, g = x_new, f_new, g_new
    return x, float(f), n_iter


def regulariser(kind: str, W: np.ndarray, b: np.ndarray, lam: float, mu: float):
    """The ODIR terms of the objective and their gradients ``(value, dW, db)`` in float64."""
    c = b.shape[0]
    value, dW = mu / c * float(b.dot(b)), np.zeros_like(W)
    if kind != "vector" and c > 1:
        off = W - np.diag(np.diag(W))
        value += lam / (c * (c - 1)) * float((off * off).sum())
        dW = 2.0 * lam / (c * (c - 1)) * off
    return value, dW, 2.0 * mu / c * b


def _split(theta: np.ndarray, kind: str, c: int):
    nw = c if kind == "vector" else c * c
    return theta[:nw].reshape((c,) if kind == "vector" else (c, c)), theta[nw:]


def identity_parameters(kind: str, c: int) -> np.ndarray:
    """``W = I, b = 0`` as one parameter vector: the uncalibrated model (for ``dirichlet``: up to the floor)."""
    W = np.ones(c) if kind == "vector" else np.eye(c)
    return np.concatenate([W.ravel(), np.zeros(c)])


class AffineCalibrator:
    """A fitted map ``q = softmax(W u + b)``: ``W`` ([C] for ``vector``, [C, C] otherwise) and ``b`` [C] as float32 host arrays
    (what the kernel reads), ``kind``, the objective ``loss`` at them and the ``n_iter`` L-BFGS iterations taken.  It pickles as
    those host arrays; the device copies are made on use."""

    def __init__(self, kind: str, W, b, loss: float = float("nan"), n_iter: int = 0, ignore_index: Optional[int] = None):
        self.kind, self.W, self.b = kind, np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)
        _hip.affine_calibration_check(self.b.shape[0], kind, self.W, self.b)
        self.loss, self.n_iter, self.ignore_index = float(loss), int(n_iter), ignore_index

    def _eval(self, x: Tensor, y, want):
        if x.shape[1] != self.b.shape[0]:
            raise ValueError(f"fitted for {self.b.shape[0]} classes, got logits {tuple(x.shape)}")
        dev = x.device
        return _hip.affine_calibration_eval(x, y, self.kind, torch.from_numpy(self.W).to(dev), torch.from_numpy(self.b).to(dev),
                                            self.ignore_index, want=want)

    def metrics(self, logits, labels, n_bins: int = 15) -> CalibrationResult:
        """Accuracy, NLL, Brier score, ECE, MCE and the reliability table of the calibrated probabilities against ``labels``
        (the per-row outputs of the kernel, then the reduce of ``calibration_metrics``); ``temperature`` is reported as 1."""
        if not isinstance(n_bins, (int, np.integer)) or n_bins < 1 or n_bins > 512:
            raise ValueError(f"n_bins must be an integer in 1 .. 512, got {n_bins!r}")
        x, y = _prepare(logits, labels, self.ignore_index)
        rows = self._eval(x, y, ("pred", "conf", "nll", "brier")).rows
        return _result_from_rows(rows, y, 1.0, int(n_bins), self.ignore_index)

    def log_probabilities_device(self, logits) -> Tensor:
        """``log q`` [N, C] float32 on the device."""
        if logits.ndim != 2:
            raise ValueError(f"logits must be [N, C], got shape {tuple(logits.shape)}")
        return self._eval(_logits_to_device(logits), None, ("logq",)).logq

    def probabilities_device(self, logits) -> Tensor:
        return self.log_probabilities_device(logits).exp_()


def fit_affine_calibration(logits, labels, kind: str = "dirichlet", lam: float = 0.0, mu: float = 0.0,
                           ignore_index: Optional[int] = None, max_iter: int = 200, tol: float = 1e-6) -> AffineCalibrator:
    """Fit ``kind`` in ``("dirichlet", "matrix", "vector")`` to ``logits`` [N, C] and ``labels`` [N] (host arrays or device
    tensors; float32 / float16 / bfloat16 device logits are read in place) by L-BFGS from ``W = I, b = 0``.  ``lam`` and ``mu``
    weigh the off-diagonal and the bias regulariser.  Rows labelled ``ignore_index`` are left out; any other label outside
    ``[0, C)`` raises.  ``matrix`` and ``dirichlet`` serve ``C <= 256``, ``vector`` ``C <= 4096``; a wider head raises
    ``ValueError``.  A non-finite objective (a NaN logit; an infinite one for ``vector`` / ``matrix``) raises as well."""
    if logits.ndim != 2 or logits.shape[1] < 1:
        raise ValueError(f"logits must be [N, C] with C >= 1, got shape {tuple(logits.shape)}")
    c = int(logits.shape[1])
    _hip.affine_calibration_check(c, kind)
    if not (lam >= 0 and mu >= 0 and np.isfinite(lam) and np.isfinite(mu)):
        raise ValueError(f"lam and mu must be non-negative and finite, got {lam!r}, {mu!r}")
    if not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not (tol > 0):
        raise ValueError(f"tol must be positive, got {tol!r}")
    x, y = _prepare(logits, labels, ignore_index)
    started = []

    def objective(theta):
        W, b = _split(theta, kind, c)
        Wd = torch.from_numpy(W.astype(np.float32)).to(x.device)
        bd = torch.from_numpy(b.astype(np.float32)).to(x.device)
        rec = _hip.to_host(_hip.affine_calibration_eval(x, y, kind, Wd, bd, ignore_index, want=("record",)).record)
        n = rec[0]
        if n == 0:
            raise ValueError("fit_affine_calibration: no labelled row (labels is empty or all ignore_index)")
        if not np.isfinite(rec[1]) and not started:  # (later: a trial step that overflowed, which the line search shortens)
            raise ValueError("fit_affine_calibration: the likelihood is not finite (a NaN or infinite logit, or a label "
                             "whose probability is 0)")
        started.append(True)
        reg, dW, db = regulariser(kind, W, b, lam, mu)
        grad = rec[2:] / n
        grad[:W.size] += dW.ravel()
        grad[W.size:] += db
        return rec[1] / n + reg, grad

    theta, loss, n_iter = lbfgs_minimize(objective, identity_parameters(kind, c), int(max_iter), float(tol))
    W, b = _split(theta, kind, c)
    return AffineCalibrator(kind, W, b, loss, n_iter, ignore_index)
