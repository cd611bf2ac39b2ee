"""Conformal prediction sets of a classifier from its logits: calibrate one threshold ``qhat`` on held-out rows, return for every
test row a set of classes that holds the true label with probability at least ``1 - alpha`` (split conformal prediction; LAC:
Sadinle et al. 2019, APS: Romano et al. 2020, RAPS: Angelopoulos et al. 2021).  The set size is a per-row uncertainty score.  The
reference has none of this; the definitions are restated in float64 in ``tests/conformal_cases.py``.

Per row, with ``p = softmax(logits / temperature)``, the classes ordered by logit (descending, equal logits by lower index first),
``r_c`` the 1-based rank of class ``c`` and ``B_c`` the sum of ``p`` over the classes ordered before it:

    lac   s_c = 1 - p_c
    aps   s_c = B_c + u p_c
    raps  s_c = B_c + u p_c + lam * max(0, r_c - k_reg)

``u`` is one number in [0, 1] per row (1 without randomisation).  ``qhat`` is the ``ceil((n + 1)(1 - alpha))``-th smallest of the
``n`` calibration scores ``s_y`` - an exact order statistic, +inf when that rank exceeds ``n`` - and a row's set is
``{c : s_c <= qhat}``.

Everything that touches the ``[N, C]`` logits runs as HIP kernels (``csrc/conformal.hip``): the label scores in one pass without
a sort, the sets with the row ordered inside the workgroup, a small integer reduce for the evaluation record.  No ``[N, C]``
temporary is made, and there is no host implementation: without a GPU the calls raise.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .calibration import _check_logits, _logits_to_device, _prepare

__all__ = ["ConformalClassifier", "ConformalResult", "PredictionSets", "conformal_quantile", "conformal_scores"]


class PredictionSets(NamedTuple):
    """``size`` [N] int32 and ``members`` [N, ceil(C / 32)] int32 on the device (bit ``c % 32`` of word ``c // 32`` is class
    ``c``; None when not asked for), the threshold they were cut at and the number of classes."""

    size: Tensor
    members: Optional[Tensor]
    qhat: float
    n_classes: int

    def to_bool(self) -> Tensor:
        """The sets as a [N, C] bool tensor on the device (plain torch: for inspection, not a hot path)."""
        if self.members is None:
            raise ValueError("these sets were predicted with return_members=False")
        shifts = torch.arange(32, dtype=torch.int32, device=self.members.device)
        bits = (self.members.unsqueeze(-1) >> shifts) & 1
        return bits.reshape(self.members.shape[0], -1)[:, :self.n_classes].to(torch.bool)

    def classes(self, i: int) -> np.ndarray:
        """The classes of row ``i``'s set, ascending (host int64)."""
        if self.members is None:
            raise ValueError("these sets were predicted with return_members=False")
        words = self.members[i].cpu().numpy().view(np.uint32)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.n_classes]
        return np.flatnonzero(bits).astype(np.int64)


class ConformalResult(NamedTuple):
    coverage: float                 # share of the rows whose set holds the label
    mean_size: float
    size_histogram: np.ndarray      # int64 [min(C + 1, 512)]: rows per set size; the last slot counts that size or more
    class_coverage: np.ndarray      # float64 [C], NaN for a class without rows
    class_count: np.ndarray         # int64 [C]
    n: int                          # rows scored (rows labelled ignore_index are left out)
    qhat: float


def _check_method(method, temperature, lam, k_reg) -> None:
    if method not in _hip.CONFORMAL_METHODS:
        raise ValueError(f"method must be one of {tuple(_hip.CONFORMAL_METHODS)}, got {method!r}")
    if not (temperature > 0) or not np.isfinite(temperature):
        raise ValueError(f"temperature must be positive and finite, got {temperature!r}")
    if not (lam >= 0) or not np.isfinite(lam):
        raise ValueError(f"lam must be non-negative and finite, got {lam!r}")
    if not isinstance(k_reg, (int, np.integer)) or k_reg < 0:
        raise ValueError(f"k_reg must be a non-negative integer, got {k_reg!r}")


def _check_width(c: int) -> None:
    limit = _hip.conformal_max_classes()
    if c > limit:
        raise ValueError(f"prediction sets are built for at most {limit} classes, got C = {c}")


def _row_numbers(u, n: int, method: str, randomized: bool, seed: int, device) -> Optional[Tensor]:
    """The per-row ``u`` on the device: None (u = 1) without randomisation and for lac (which has no ``u``: a caller's is
    checked and then unused), the caller's, or ``torch.rand`` from a device generator seeded by ``seed``."""
    if not randomized:
        if u is not None:
            raise ValueError("u was given with randomized=False (u = 1 there)")
        return None
    if u is None:
        if method == "lac":
            return None
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        return torch.rand((n,), generator=gen, dtype=torch.float32, device=device)
    if not isinstance(u, Tensor):
        u = np.asarray(u)
        if u.dtype.kind not in "fiu":
            raise ValueError(f"u must hold numbers, got dtype {u.dtype}")
    if u.ndim != 1 or u.shape[0] != n:
        raise ValueError(f"u must hold one number per row of logits ({n}), got shape {tuple(u.shape)}")
    u = u.detach().to(device=device, dtype=torch.float32) if isinstance(u, Tensor) else _hip.to_device(u, torch.float32)
    if n and not bool(((u >= 0) & (u <= 1)).all()):
        raise ValueError("u must lie in [0, 1]")
    return None if method == "lac" else u


def conformal_quantile(scores: Tensor, alpha: float) -> float:
    """The ``ceil((n + 1)(1 - alpha))``-th smallest of the ``n`` float32 device scores, exactly (a radix select, no
    interpolation); +inf when that rank exceeds ``n``.  A NaN score raises."""
    if not (0 < alpha < 1):
        raise ValueError(f"alpha must lie in (0, 1), got {alpha!r}")
    n = scores.numel()
    if n and bool(torch.isnan(scores).any()):
        raise ValueError("a calibration score is NaN (a NaN logit, or a row without a finite logit)")
    k = math.ceil((n + 1) * (1 - alpha))
    if k > n:
        return math.inf
    return _hip.kth_smallest_flat(scores, [k - 1])[0]


def _label_scores(x: Tensor, y: Tensor, method, temperature, u, lam, k_reg, ignore_index) -> Tensor:
    return _hip.conformal_label_scores(x, y, method, 1.0 / temperature, u, lam, k_reg, ignore_index)[0]


def conformal_scores(logits, labels, method: str = "aps", temperature: float = 1.0, randomized: bool = True, u=None,
                     lam: float = 0.0, k_reg: int = 0, seed: int = 0, ignore_index: Optional[int] = None) -> Tensor:
    """The conformal score ``s_y`` of every row's label, float32 [N] on the device (NaN for a row labelled ``ignore_index`` and
    for a row without a softmax).  ``logits`` [N, C] and ``labels`` [N] are host arrays or device tensors (float32 / float16 /
    bfloat16 device logits, row-sliced views included, are read in place).  Sums in a fixed order: the same bits every run."""
    _check_method(method, temperature, lam, k_reg)
    x, y = _prepare(logits, labels, ignore_index)
    u = _row_numbers(u, x.shape[0], method, randomized, seed, x.device)
    return _label_scores(x, y, method, float(temperature), u, float(lam), int(k_reg), ignore_index)


class ConformalClassifier:
    """Split conformal prediction as an object: ``calibrate`` finds ``qhat_`` on a held-out split, ``predict`` returns the sets of
    a batch, ``evaluate`` their coverage and sizes against labels.  The state is host scalars only (it pickles).  A fitted
    ``TemperatureScaler`` composes by passing its ``temperature``.  Where ``u`` is drawn, calibration uses the generator seeded by
    ``seed`` and every ``predict`` / ``evaluate`` call a fresh one seeded by ``seed + 1``: a call is reproducible, and row ``i`` of
    every batch gets the same ``u``.  The guarantee is per row and holds; a caller who wants independent draws across batches
    passes ``u``."""

    def __init__(self, method: str = "aps", alpha: float = 0.1, temperature: float = 1.0, randomized: bool = True,
                 lam: float = 0.0, k_reg: int = 0, seed: int = 0):
        _check_method(method, temperature, lam, k_reg)
        if not (0 < alpha < 1):
            raise ValueError(f"alpha must lie in (0, 1), got {alpha!r}")
        self.method = method
        self.alpha = float(alpha)
        self.temperature = float(temperature)
        self.randomized = bool(randomized)
        self.lam = float(lam)
        self.k_reg = int(k_reg)
        self.seed = int(seed)
        self.qhat_: Optional[float] = None
        self.n_calibration_: Optional[int] = None

    def calibrate(self, logits, labels, ignore_index: Optional[int] = None, u=None) -> "ConformalClassifier":
        _check_logits(logits)
        _check_width(logits.shape[1])
        x, y = _prepare(logits, labels, ignore_index)
        u = _row_numbers(u, x.shape[0], self.method, self.randomized, self.seed, x.device)
        s = _label_scores(x, y, self.method, self.temperature, u, self.lam, self.k_reg, ignore_index)
        if ignore_index is not None:
            s = s[y != int(ignore_index)]
        if s.numel() == 0:
            raise ValueError("calibrate: no labelled row (labels is empty or all ignore_index)")
        self.qhat_ = conformal_quantile(s, self.alpha)
        self.n_calibration_ = int(s.numel())
        return self

    def _sets(self, logits, labels, u, ignore_index, want_members):
        if self.qhat_ is None:
            raise ValueError("calibrate the classifier first")
        _check_logits(logits)
        _check_width(logits.shape[1])
        x, y = (_logits_to_device(logits), None) if labels is None else _prepare(logits, labels, ignore_index)
        u = _row_numbers(u, x.shape[0], self.method, self.randomized, self.seed + 1, x.device)
        return x, y, _hip.conformal_sets(x, self.qhat_, self.method, 1.0 / self.temperature, u, self.lam, self.k_reg, y,
                                         ignore_index, want_members)

    def predict(self, logits, u=None, return_members: bool = True) -> PredictionSets:
        x, _, sets = self._sets(logits, None, u, None, return_members)
        return PredictionSets(sets.size, sets.members, self.qhat_, int(x.shape[1]))

    def evaluate(self, logits, labels, u=None, ignore_index: Optional[int] = None) -> ConformalResult:
        x, y, sets = self._sets(logits, labels, u, ignore_index, False)
        c = int(x.shape[1])
        rec = _hip.conformal_record(_hip.to_host(_hip.conformal_reduce(sets, y, c, ignore_index)), c)
        n = rec["n_used"]
        count, hit = rec["class_count"], rec["class_covered"]
        with np.errstate(invalid="ignore", divide="ignore"):
            class_coverage = np.where(count > 0, hit / count, np.nan)
        nan = float("nan")
        return ConformalResult(rec["n_covered"] / n if n else nan, rec["size_sum"] / n if n else nan, rec["hist"], class_coverage,
                               count, n, self.qhat_)
