"""Kernel two-sample tests for distribution shift on the device (no counterpart in the reference).

The postprocessors score one row at a time; this module answers whether a whole batch of rows - LaREx entropies, PCA rows,
penultimate features - has drifted from an InD reference table: the kernel MMD permutation test of Gretton et al. (JMLR 2012),
as used in "Failing Loudly" (Rabanser et al., NeurIPS 2019), and the energy distance (Szekely & Rizzo).

Definitions (``csrc/shift.hip``, ``csrc/shift_perm.hpp``).  Pooled rows ``Z = [X; Y]``, ``N = n + m``, centred by the
pooled column mean unless the kernel is ``linear``.  Kernels: ``rbf`` ``k = sum_b exp(-d^2 / (2 sigma_b^2))``, ``energy``
``k = -d``, ``linear`` ``k = z_i . z_j``.  Permutation ``p`` (``p = 0``: the observed split) has exactly ``n`` members, a pure
function of ``(seed, p, i, n, N)``.  With ``K = k(Z, Z)`` the device forms ``t_p = a_p' K a_p``, ``u_p = a_p' K 1`` and
``S = 1' K 1`` without ever storing ``K``; ``AA = t``, ``AB = u - t``, ``BB = S - 2 u + t`` give the biased statistic
``AA / n^2 + BB / m^2 - 2 AB / (n m)`` or the unbiased one (diagonal removed), and
``p_value = (1 + #{p >= 1: stat_p >= stat_0}) / (1 + n_perm)``.  Any non-finite input makes ``statistic`` and ``p_value`` NaN.

There is no CPU path: without a GPU the functions raise, after their argument checks.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _hip

__all__ = ["ShiftTestResult", "mmd_test", "energy_test", "ShiftDetector", "shift_power_table", "median_bandwidth"]

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@dataclass
class ShiftTestResult:
    """``statistic``: the observed statistic; ``p_value``: the permutation p-value; ``null``: device tensor ``(n_perm,)`` f64 of
    the permuted statistics; ``bandwidths``: the sigmas used (empty for ``energy`` / ``linear``)."""

    statistic: float
    p_value: float
    null: Tensor
    bandwidths: Tuple[float, ...]
    kernel: str
    estimator: str
    n_x: int
    n_y: int
    n_perm: int
    seed: int


def _shape2(a) -> Tuple[int, int]:
    shape = tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape
    if len(shape) != 2:
        raise ValueError(f"rows must be a 2-D table (rows, features), got shape {shape}")
    return int(shape[0]), int(shape[1])


def _check_tables(x, y, estimator: str) -> None:
    (n, dx), (m, dy) = _shape2(x), _shape2(y)
    if dx != dy:
        raise ValueError(f"the two tables differ in width: {dx} and {dy}")
    if dx < 1 or n < 1 or m < 1:
        raise ValueError("both tables need at least one row and one feature")
    if estimator == "unbiased" and (n < 2 or m < 2):
        raise ValueError(f"the unbiased estimator needs n >= 2 and m >= 2, got {n} and {m}")
    if n + m > _hip.SHIFT_MAX_ROWS:
        raise ValueError(f"n + m = {n + m} exceeds 2^18 pooled rows")


def _check_common(kernel: str, estimator: str, n_perm, seed) -> None:
    if kernel not in _hip.SHIFT_KERNELS:
        raise ValueError(f"kernel must be one of {sorted(_hip.SHIFT_KERNELS)}, not {kernel!r}")
    if estimator not in _hip.SHIFT_ESTIMATORS:
        raise ValueError(f"estimator must be 'unbiased' or 'biased', not {estimator!r}")
    if int(n_perm) != n_perm or int(n_perm) < 1:
        raise ValueError(f"n_perm must be a positive integer, not {n_perm!r}")
    if int(seed) != seed:
        raise ValueError(f"seed must be an integer, not {seed!r}")


def _explicit_bandwidths(bandwidths) -> Tuple[float, ...]:
    bw = np.atleast_1d(np.asarray(bandwidths, dtype=np.float64))
    if bw.ndim != 1 or bw.size < 1:
        raise ValueError("bandwidths must be 'median', a number or a sequence of numbers")
    if bw.size > _hip.SHIFT_MAX_BANDWIDTHS:
        raise ValueError(f"at most {_hip.SHIFT_MAX_BANDWIDTHS} bandwidths, got {bw.size}")
    if not np.all(bw > 0.0):
        raise ValueError(f"every bandwidth must be positive, got {bw.tolist()}")
    return tuple(float(b) for b in bw)


def _check_bandwidth_args(kernel: str, bandwidths, scales) -> None:
    """Everything about the bandwidths that can be refused without looking at the rows."""
    if kernel != "rbf":
        return
    if isinstance(bandwidths, str):
        if bandwidths != "median":
            raise ValueError(f"bandwidths must be 'median', a number or a sequence of numbers, not {bandwidths!r}")
        _explicit_bandwidths(scales)  # (count and sign of the scales are those of the bandwidths)
    else:
        _explicit_bandwidths(bandwidths)


def _device_rows(a, dtype: Optional[torch.dtype] = None) -> Tensor:
    """CUDA tensors stay where and as they are (strided row views included); host arrays go through ``to_device``."""
    if isinstance(a, Tensor) and a.is_cuda:
        if a.dtype not in _DTYPES:
            raise ValueError(f"rows must be float32, float16 or bfloat16, not {a.dtype}")
        return a.detach()
    if isinstance(a, Tensor):
        want = a.dtype if a.dtype in _DTYPES else torch.float32
    else:
        a = np.asarray(a)
        want = torch.float16 if a.dtype == np.float16 else torch.float32
    return _hip.to_device(a, dtype or want)


def _pair(x, y) -> Tuple[Tensor, Tensor]:
    xd = _device_rows(x)
    yd = _device_rows(y, xd.dtype) if not (isinstance(y, Tensor) and y.is_cuda) else _device_rows(y)
    if xd.dtype != yd.dtype:
        raise ValueError(f"the two tables differ in dtype: {xd.dtype} and {yd.dtype}")
    return xd, yd


def median_bandwidth(x, y) -> float:
    """The median distance between the rows of the bandwidth sample of the pooled table ``[x; y]``: at most 2048 pooled rows at
    evenly spaced indices (``floor(k N / M)``), all pairs ``k < l``, the median as ``numpy.median`` takes it.  NaN when a sampled row
    is not finite."""
    _check_tables(x, y, "biased")
    xd, yd = _pair(x, y)
    if xd.shape[0] + yd.shape[0] < 2:
        raise ValueError("the median distance needs two pooled rows")
    dist = _hip.shift_pairwise_sample(xd, yd)
    if not bool(torch.isfinite(dist).all()):
        return float("nan")
    cnt = dist.numel()
    lo, hi = _hip.kth_smallest_flat(dist, [(cnt - 1) // 2, cnt // 2])
    return 0.5 * (lo + hi)


def _resolve_bandwidths(kernel: str, bandwidths, scales, xd: Tensor, yd: Tensor) -> Tuple[float, ...]:
    if kernel != "rbf":
        return ()
    if isinstance(bandwidths, str):
        med = median_bandwidth(xd, yd)
        if med != med:
            return tuple(float("nan") for _ in _explicit_bandwidths(scales))  # non-finite rows: the test itself reports NaN
        if not med > 0.0:
            raise ValueError("the median distance of the sample is 0: no positive bandwidth (pass bandwidths explicitly)")
        return tuple(med * s for s in _explicit_bandwidths(scales))
    return _explicit_bandwidths(bandwidths)


def _run(xd: Tensor, yd: Tensor, kernel: str, bw: Tuple[float, ...], n_perm: int, seed: int, estimator: str) -> ShiftTestResult:
    sums = _hip.shift_mmd(xd, yd, kernel, bw if kernel == "rbf" else (1.0,), estimator, int(n_perm), int(seed))
    head = _hip.to_host(torch.stack((sums.stats[0], sums.p_value[0])))
    return ShiftTestResult(float(head[0]), float(head[1]), sums.stats[1:], tuple(bw), kernel, estimator, int(xd.shape[0]),
                           int(yd.shape[0]), int(n_perm), int(seed))


def mmd_test(x, y, *, kernel: str = "rbf", bandwidths: Union[str, float, Sequence[float]] = "median",
             scales: Sequence[float] = (0.25, 0.5, 1, 2, 4), n_perm: int = 1000, seed: int = 0,
             estimator: str = "unbiased") -> ShiftTestResult:
    """The kernel MMD permutation test of ``x`` (n, D) against ``y`` (m, D): CUDA tensors (f32 / f16 / bf16, strided row views read
    in place) or host arrays.  ``bandwidths="median"``: sigma = the sample's median distance (:func:`median_bandwidth`) times each
    of ``scales``; a number or a sequence of at most 8 is taken as is.  ``ValueError`` for tables of different width, fewer than two
    rows a side with the unbiased estimator, more than 8 or non-positive bandwidths, more than 2^18 pooled rows, ``n_perm < 1``."""
    _check_common(kernel, estimator, n_perm, seed)
    _check_tables(x, y, estimator)
    _check_bandwidth_args(kernel, bandwidths, scales)
    xd, yd = _pair(x, y)
    return _run(xd, yd, kernel, _resolve_bandwidths(kernel, bandwidths, scales, xd, yd), n_perm, seed, estimator)


def energy_test(x, y, *, n_perm: int = 1000, seed: int = 0, estimator: str = "biased") -> ShiftTestResult:
    """The energy-distance permutation test: the same launch with ``k = -d``; the biased (V-statistic) form is
    ``2 E|X - Y| - E|X - X'| - E|Y - Y'|`` over all pairs."""
    return mmd_test(x, y, kernel="energy", n_perm=n_perm, seed=seed, estimator=estimator)


class ShiftDetector:
    """``fit(reference)`` keeps the reference rows on the device and fixes the bandwidths (for ``bandwidths="median"``: from the
    reference alone); ``test(batch)`` is :func:`mmd_test` of the reference against the batch with those bandwidths.

    The fitted state is host arrays (``reference_``, ``bandwidths_``); the device copy is a cache that is rebuilt on first use, so a
    pickle holds no GPU tensor and loads on a host without a GPU."""

    _device_cache_attrs = ("_dev",)

    def __init__(self, *, kernel: str = "rbf", bandwidths: Union[str, float, Sequence[float]] = "median",
                 scales: Sequence[float] = (0.25, 0.5, 1, 2, 4), n_perm: int = 1000, seed: int = 0, estimator: str = "unbiased"):
        _check_common(kernel, estimator, n_perm, seed)
        _check_bandwidth_args(kernel, bandwidths, scales)
        self.kernel, self.bandwidths, self.scales = kernel, bandwidths, tuple(scales)
        self.n_perm, self.seed, self.estimator = int(n_perm), int(seed), estimator
        self.reference_ = None
        self.bandwidths_ = None
        self._ref_dtype = "float32"  # bf16 rows are kept widened on the host (exactly) and narrowed again on upload
        self._dev = None

    def __getstate__(self):
        state = dict(self.__dict__)
        for name in self._device_cache_attrs:
            if name in state:
                state[name] = None
        return state

    def fit(self, reference) -> "ShiftDetector":
        n, d = _shape2(reference)
        if n < 2 or d < 1:
            raise ValueError("the reference needs at least two rows and one feature")
        if n >= _hip.SHIFT_MAX_ROWS:
            raise ValueError(f"the reference has {n} rows: no room for a batch within 2^18 pooled rows")
        ref = _device_rows(reference)
        ref = ref if ref.is_contiguous() else ref.contiguous()
        if self.kernel == "rbf" and isinstance(self.bandwidths, str):
            half = n // 2  # the sample of the pooled table [first half; second half] is the sample of the reference
            self.bandwidths_ = _resolve_bandwidths("rbf", "median", self.scales, ref[:half], ref[half:])
        else:
            self.bandwidths_ = _resolve_bandwidths(self.kernel, self.bandwidths, self.scales, ref, ref)
        host = _hip.to_host(ref.float() if ref.dtype == torch.bfloat16 else ref)
        self.reference_ = np.array(host, copy=True)
        self._ref_dtype = str(ref.dtype).replace("torch.", "")
        self._dev = ref
        return self

    def _reference_device(self) -> Tensor:
        if self.reference_ is None:
            raise RuntimeError("ShiftDetector.test before fit")
        if self._dev is None:
            self._dev = _hip.to_device(self.reference_, getattr(torch, self._ref_dtype))
        return self._dev

    def test(self, batch, *, seed: Optional[int] = None) -> ShiftTestResult:
        ref = self._reference_device()
        seed = self.seed if seed is None else seed
        _check_common(self.kernel, self.estimator, self.n_perm, seed)
        _check_tables(ref, batch, self.estimator)
        xd, yd = _pair(ref, batch)
        return _run(xd, yd, self.kernel, self.bandwidths_, self.n_perm, seed, self.estimator)


def shift_power_table(ind_rows, ood_dict: Dict[str, object], *, sample_sizes: Sequence[int], n_trials: int, alpha: float = 0.05,
                      test: str = "mmd", n_perm: int = 200, seed: int = 0, **test_kwargs) -> Dict[str, Dict[int, float]]:
    """Detection rate at level ``alpha`` per OoD set and per sample size: ``{name: {size: rate}}``, with the control row
    ``"InD"`` (InD against InD, disjoint subsets) first.  A trial draws ``size`` reference rows and ``size`` batch rows without
    replacement from a generator seeded by ``(seed, size, trial)`` and runs :func:`mmd_test` (``test="mmd"``, ``test_kwargs``
    passed on) or :func:`energy_test` (``test="energy"``); a rejection is ``p_value <= alpha``.  A thin host loop."""
    if test not in ("mmd", "energy"):
        raise ValueError(f"test must be 'mmd' or 'energy', not {test!r}")
    if not (0.0 < float(alpha) < 1.0):
        raise ValueError(f"alpha must lie strictly between 0 and 1, not {alpha!r}")
    if int(n_trials) != n_trials or int(n_trials) < 1:
        raise ValueError(f"n_trials must be a positive integer, not {n_trials!r}")
    sizes = [int(s) for s in sample_sizes]
    n_ind = _shape2(ind_rows)[0]
    for s in sizes:
        if s < 2 or 2 * s > n_ind:
            raise ValueError(f"sample size {s}: 2 <= size and 2 * size <= {n_ind} InD rows are required (reference and control)")
    for name, rows in ood_dict.items():
        if _shape2(rows)[0] < max(sizes, default=0):
            raise ValueError(f"OoD set {name!r} has fewer rows than the largest sample size")
        if name == "InD":
            raise ValueError("'InD' names the control row")
    run = mmd_test if test == "mmd" else energy_test
    ind = _device_rows(ind_rows)
    sets = {name: _device_rows(rows, ind.dtype) for name, rows in ood_dict.items()}
    table: Dict[str, Dict[int, float]] = {name: {} for name in ["InD", *sets]}
    for s in sizes:
        hits = {name: 0 for name in table}
        for trial in range(int(n_trials)):
            rng = np.random.default_rng([int(seed), s, trial])
            pick = torch.from_numpy(rng.permutation(n_ind)[: 2 * s]).to(ind.device)
            ref = ind.index_select(0, pick[:s])
            batches = {"InD": ind.index_select(0, pick[s:])}
            for name, rows in sets.items():
                sub = torch.from_numpy(rng.permutation(rows.shape[0])[:s]).to(rows.device)
                batches[name] = rows.index_select(0, sub)
            for name, batch in batches.items():
                res = run(ref, batch, n_perm=n_perm, seed=int(seed) + trial, **test_kwargs)
                hits[name] += int(res.p_value <= alpha)
        for name in table:
            table[name][s] = hits[name] / int(n_trials)
    return table
