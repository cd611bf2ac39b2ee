"""Per-feature Kolmogorov-Smirnov drift tests with a max-T permutation null on the device (no counterpart in the reference).

:mod:`.shift` says WHETHER a batch of latent rows has drifted from the InD reference; this module says WHICH features moved: one
univariate two-sample KS test per feature, the recipe "Failing Loudly" (Rabanser et al., NeurIPS 2019) found strongest, combined
over the features by the Westfall-Young max-T permutation adjustment (Ge, Dudoit & Speed 2003), which controls the family-wise
error under any dependence between the features, or by Bonferroni over the asymptotic p-values as in the paper.

Definitions (``csrc/ks_perm.hip``).  Two row tables ``X [n, D]``, ``Y [m, D]`` of one dtype, pooled ``Z = [X; Y]``,
``N = n + m``.  For feature ``d`` and permutation ``p``: walk the pooled values of column ``d`` in ascending order, start ``v = 0``,
add ``m`` for a member of the first set of permutation ``p`` and subtract ``n`` otherwise; at the last position of every run of
equal values take ``|v|``; ``T[p, d]`` is the largest of those, an exact integer ``<= n m``, and the KS statistic is
``T[p, d] / (n m)`` (``scipy.stats.ks_2samp`` to the last bit of the division).

* Order: values compare as numbers; f16 / bf16 are widened exactly; ``-0.0 == +0.0``; ``+-inf`` are ordinary extreme values.
* A column holding any NaN is invalid: ``T[:, d] = -1``, NaN statistic and p-values, left out of every family maximum and of the
  Bonferroni count ``K`` (the number of valid features).
* Memberships are those of :mod:`.shift` (``csrc/shift_perm.hpp``): ``p = 0`` is the observed split (rows ``i < n``), ``p >= 1``
  has exactly ``n`` members, a pure function of ``(seed, p, i, n, N)``.
* Raw permutation p-value: ``p_d = (1 + #{p >= 1: T[p, d] >= T[0, d]}) / (1 + n_perm)``.
* Single-step max-T (``adjust="maxT"``): ``M_p = max over valid d of T[p, d]``,
  ``p~_d = (1 + #{p >= 1: M_p >= T[0, d]}) / (1 + n_perm)``.
* Step-down max-T (``adjust="stepdown"``): order the valid features by ``T[0, d]`` descending, ties by feature index ascending,
  ``r_1 .. r_K``; ``u_{p,k} = max_{l >= k} T[p, r_l]``; ``p~_{r_k} = (1 + #{p >= 1: u_{p,k} >= T[0, r_k]}) / (1 + n_perm)``, then
  the running maximum over ``k``.
* Asymptotic: ``p_asym_d = min(1, 2 sum_{k >= 1} (-1)^(k-1) exp(-2 k^2 lambda^2))``, ``lambda = sqrt(n m / N) T[0, d] / (n m)``, in
  f64 on the host, 1 where the statistic is 0; ``adjust="bonferroni"`` is ``min(1, K p_asym_d)``, the only mode ``n_perm = 0``
  allows (the permutation p-values are then NaN and ``null_max`` is empty).
* Global test: statistic ``M_0 / (n m)``, p-value ``(1 + #{p >= 1: M_p >= M_0}) / (1 + n_perm)``; NaN when no feature is valid.

All comparisons are integer comparisons and every output is the same bits from call to call.  There is no CPU path for the table:
without a GPU :func:`ks_test` raises, after its argument checks.  :func:`maxt_adjust` is bookkeeping on ``(1 + n_perm) x D``
integers in plain torch ops and runs wherever its table lives.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .shift import _device_rows, _pair, _shape2

__all__ = ["UnivariateShiftResult", "MaxTAdjustment", "ks_test", "ks_asymptotic_p", "maxt_adjust", "UnivariateShiftDetector"]

ADJUSTMENTS = ("maxT", "stepdown", "bonferroni")


@dataclass
class UnivariateShiftResult:
    """``statistic``, ``p_value`` (raw permutation), ``p_adjusted`` (by ``adjust``), ``p_asymptotic``: device tensors ``(D,)`` f64,
    NaN in an invalid feature; ``global_statistic`` / ``global_p_value``: the max-T test of "any feature drifted";  ``drifted``:
    host int array of the features with ``p_adjusted <= alpha``, strongest first (smallest adjusted p-value, then largest
    statistic, then lowest index); ``null_max``: device tensor ``(n_perm,)`` f64 of the permuted family maxima ``M_p / (n m)``."""

    statistic: Tensor
    p_value: Tensor
    p_adjusted: Tensor
    p_asymptotic: Tensor
    global_statistic: float
    global_p_value: float
    drifted: np.ndarray
    null_max: Tensor
    adjust: str
    n_x: int
    n_y: int
    n_perm: int
    seed: int


def _ratio(num: Tensor, den: int) -> Tensor:
    """``num / den`` as ONE correctly rounded f64 division per element: the divisor is a tensor, because torch turns a division by
    a scalar on the device into a multiplication by its reciprocal, which is an ulp off for some counts."""
    num = num.to(torch.float64)
    return num / torch.full_like(num, float(den))


class MaxTAdjustment(NamedTuple):
    """Outputs of :func:`maxt_adjust` on the table's device: ``p_value``, ``p_single_step``, ``p_step_down`` f64 ``(D,)`` (NaN in an
    invalid column), ``p_adjusted`` the one ``method`` names, ``maxima`` int64 ``(1 + n_perm,)`` = ``M_p`` (-1 when no column is
    valid)."""

    p_value: Tensor
    p_single_step: Tensor
    p_step_down: Tensor
    p_adjusted: Tensor
    maxima: Tensor


def maxt_adjust(table: Tensor, valid: Tensor, method: str = "maxT") -> MaxTAdjustment:
    """Raw, single-step and step-down max-T p-values from an integer table ``[1 + n_perm, D]`` (row 0: the observed split) and the
    per-column ``valid`` flags.  Integer comparisons throughout; ``(1 + count) / (1 + n_perm)`` is one f64 division."""
    if method not in ("maxT", "stepdown"):
        raise ValueError(f"method must be 'maxT' or 'stepdown', not {method!r}")
    if table.dim() != 2 or table.shape[0] < 1 or valid.shape != (table.shape[1],):
        raise ValueError("table must be [1 + n_perm, D] with one valid flag per column")
    table = table.to(torch.int64)
    ok = valid.to(device=table.device) != 0
    rows, d = table.shape
    tab = torch.where(ok[None, :], table, torch.full_like(table, -1))  # an invalid column never raises a maximum
    t0 = tab[0]
    nan = torch.full((d,), float("nan"), dtype=torch.float64, device=table.device)

    def p_of(count: Tensor) -> Tensor:
        return _ratio(1 + count, rows)

    raw = torch.where(ok, p_of((tab[1:] >= t0[None, :]).sum(dim=0)), nan)
    maxima = tab.max(dim=1).values if d > 0 else torch.full((rows,), -1, dtype=torch.int64, device=table.device)
    single = torch.where(ok, p_of((maxima[1:, None] >= t0[None, :]).sum(dim=0)), nan)
    # step-down: columns by t0 descending, ties by index ascending (a stable sort); invalid columns (-1) come last
    order = torch.sort(t0, descending=True, stable=True).indices
    srt = tab[:, order]
    succ = torch.flip(torch.cummax(torch.flip(srt, [1]), dim=1).values, [1])  # u[p, k] = max over l >= k
    down = torch.cummax(p_of((succ[1:] >= srt[0][None, :]).sum(dim=0)), dim=0).values
    step = torch.empty_like(nan)
    step[order] = down
    step = torch.where(ok, step, nan)
    return MaxTAdjustment(raw, single, step, single if method == "maxT" else step, maxima)


def ks_asymptotic_p(statistic, n: int, m: int) -> np.ndarray:
    """The asymptotic two-sided p-value of KS statistics between samples of ``n`` and ``m`` rows, host f64:
    ``min(1, 2 sum_{k >= 1} (-1)^(k-1) exp(-2 k^2 lambda^2))`` with ``lambda = sqrt(n m / (n + m)) statistic``.  Below
    ``lambda = 1`` the series is summed in its Jacobi-theta form ``1 - sqrt(2 pi) / lambda sum_k exp(-(2 k - 1)^2 pi^2 / (8
    lambda^2))``, the same function, whose terms fall off where the alternating ones cancel.  1 at statistic 0, NaN at NaN."""
    if isinstance(statistic, Tensor):
        statistic = _hip.to_host(statistic)
    stat = np.asarray(statistic, dtype=np.float64)
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError("n and m must be positive")
    lam = np.sqrt(n * m / (n + m)) * stat
    k = np.arange(1, 9, dtype=np.float64).reshape((-1,) + (1,) * lam.ndim)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        big = 2.0 * np.sum((-1.0) ** (k - 1.0) * np.exp(-2.0 * k * k * lam * lam), axis=0)
        small = 1.0 - np.sqrt(2.0 * np.pi) / lam * np.sum(np.exp(-((2.0 * k - 1.0) ** 2) * np.pi**2 / (8.0 * lam * lam)), axis=0)
    p = np.where(lam >= 1.0, big, small)
    p = np.where(lam <= 0.0, 1.0, p)
    return np.where(np.isnan(stat), np.nan, np.clip(p, 0.0, 1.0))


def _check(x, y, n_perm, seed, adjust: str, alpha) -> None:
    if adjust not in ADJUSTMENTS:
        raise ValueError(f"adjust must be one of {list(ADJUSTMENTS)}, not {adjust!r}")
    if int(n_perm) != n_perm or int(n_perm) < 0 or int(n_perm) > _hip.KS_MAX_PERM:
        raise ValueError(f"n_perm must be an integer in 0 .. 2^20 - 1, not {n_perm!r}")
    if int(n_perm) == 0 and adjust != "bonferroni":
        raise ValueError(f"n_perm = 0 leaves no permutation null: adjust={adjust!r} needs n_perm >= 1 (only 'bonferroni' does not)")
    if int(seed) != seed:
        raise ValueError(f"seed must be an integer, not {seed!r}")
    if not (0.0 < float(alpha) < 1.0):
        raise ValueError(f"alpha must lie strictly between 0 and 1, not {alpha!r}")
    if x is None:
        return
    (n, dx), (m, dy) = _shape2(x), _shape2(y)
    if dx != dy:
        raise ValueError(f"the two tables differ in width: {dx} and {dy}")
    if dx < 1 or n < 1 or m < 1:
        raise ValueError("both tables need at least one row and one feature")
    cap = _hip.ks_max_rows()
    if n + m > cap:
        raise ValueError(f"n + m = {n + m} exceeds the cap of {cap} pooled rows of one KS test: subsample the reference")


def _run(xd: Tensor, yd: Tensor, n_perm: int, seed: int, adjust: str, alpha: float) -> UnivariateShiftResult:
    n, m = int(xd.shape[0]), int(yd.shape[0])
    table, valid = _hip.ks_perm_table(xd, yd, n_perm, seed)
    adj = maxt_adjust(table, valid, "stepdown" if adjust == "stepdown" else "maxT")
    ok = valid != 0
    nan = torch.full_like(adj.p_value, float("nan"))
    scale = n * m
    statistic = torch.where(ok, _ratio(table[0], scale), nan)
    stat_host = _hip.to_host(statistic)
    asym_host = ks_asymptotic_p(stat_host, n, m)
    k_valid = int(np.count_nonzero(~np.isnan(stat_host)))
    p_asym = torch.from_numpy(asym_host).to(statistic.device)
    if adjust == "bonferroni":
        p_adj = torch.from_numpy(np.where(np.isnan(asym_host), np.nan, np.minimum(1.0, k_valid * asym_host))).to(statistic.device)
    else:
        p_adj = adj.p_adjusted
    p_raw = adj.p_value if n_perm > 0 else nan
    maxima = _hip.to_host(adj.maxima)
    if k_valid == 0:
        g_stat = g_p = float("nan")
    else:
        g_stat = float(maxima[0]) / scale
        g_p = (1 + int(np.sum(maxima[1:] >= maxima[0]))) / (1 + n_perm) if n_perm > 0 else float("nan")
    p_host = _hip.to_host(p_adj)
    hit = np.nonzero(p_host <= float(alpha))[0]  # (NaN compares false)
    drifted = hit[np.lexsort((hit, -stat_host[hit], p_host[hit]))].astype(np.int64)
    null_max = _ratio(adj.maxima[1:], scale)
    return UnivariateShiftResult(statistic, p_raw, p_adj, p_asym, g_stat, g_p, drifted, null_max, adjust, n, m, int(n_perm),
                                 int(seed))


def ks_test(x, y, *, n_perm: int = 1000, seed: int = 0, adjust: str = "maxT", alpha: float = 0.05) -> UnivariateShiftResult:
    """One two-sample KS test per feature of ``x`` (n, D) against ``y`` (m, D), with permutation p-values adjusted over the
    features: CUDA tensors (f32 / f16 / bf16, strided row views read in place) or host arrays, as :func:`~.shift.mmd_test`.
    ``adjust``: ``"maxT"`` (single-step Westfall-Young), ``"stepdown"`` or ``"bonferroni"`` (asymptotic p-values times the
    number of valid features; the only mode ``n_perm = 0`` allows).  ``ValueError`` for tables of different width, an empty
    table, more pooled rows than ``runia_ks_max_rows()`` (subsample the reference), a bad ``n_perm``, ``adjust`` or ``alpha``."""
    _check(x, y, n_perm, seed, adjust, alpha)
    xd, yd = _pair(x, y)
    return _run(xd, yd, int(n_perm), int(seed), adjust, float(alpha))


class UnivariateShiftDetector:
    """``fit(reference)`` keeps the reference rows; ``test(batch)`` is :func:`ks_test` of the reference against the batch.

    The fitted state is a host array (``reference_``); the device copy is a cache that is rebuilt on first use, so a pickle holds
    no GPU tensor and loads on a host without a GPU (as :class:`~.shift.ShiftDetector`)."""

    _device_cache_attrs = ("_dev",)

    def __init__(self, *, n_perm: int = 1000, adjust: str = "maxT", alpha: float = 0.05, seed: int = 0):
        _check(None, None, n_perm, seed, adjust, alpha)
        self.n_perm, self.adjust, self.alpha, self.seed = int(n_perm), adjust, float(alpha), int(seed)
        self.reference_ = None
        self._ref_dtype = "float32"  # bf16 rows are kept widened on the host (exactly) and narrowed again on upload
        self._dev = None

    def __getstate__(self):
        state = dict(self.__dict__)
        for name in self._device_cache_attrs:
            if name in state:
                state[name] = None
        return state

    def fit(self, reference) -> "UnivariateShiftDetector":
        n, d = _shape2(reference)
        if n < 1 or d < 1:
            raise ValueError("the reference needs at least one row and one feature")
        cap = _hip.ks_max_rows()
        if n >= cap:
            raise ValueError(f"the reference has {n} rows: no room for a batch within the cap of {cap} pooled rows of one KS test: "
                             "subsample the reference")
        ref = _device_rows(reference)
        ref = ref if ref.is_contiguous() else ref.contiguous()
        host = _hip.to_host(ref.float() if ref.dtype == torch.bfloat16 else ref)
        self.reference_ = np.array(host, copy=True)
        self._ref_dtype = str(ref.dtype).replace("torch.", "")
        self._dev = ref
        return self

    def _reference_device(self) -> Tensor:
        if self.reference_ is None:
            raise RuntimeError("UnivariateShiftDetector.test before fit")
        if self._dev is None:
            self._dev = _hip.to_device(self.reference_, getattr(torch, self._ref_dtype))
        return self._dev

    def test(self, batch, *, seed: Optional[int] = None) -> UnivariateShiftResult:
        if self.reference_ is None:
            raise RuntimeError("UnivariateShiftDetector.test before fit")
        seed = self.seed if seed is None else seed
        _check(self.reference_, batch, self.n_perm, seed, self.adjust, self.alpha)
        xd, yd = _pair(self._reference_device(), batch)
        return _run(xd, yd, self.n_perm, int(seed), self.adjust, self.alpha)
