"""Per-pixel k-nearest-neighbour anomaly maps from the feature maps of a segmentation decoder: the distance of every
pixel's feature vector to its k-th nearest row of a memory bank of in-distribution pixel features - "deep nearest
neighbours" as SegmentMeIfYouCan, RoadAnomaly and Fishyscapes report it next to the Mahalanobis baseline, and the scoring
half of a PatchCore-style bank.  It is the non-parametric counterpart of ``pixel_features.PixelMahalanobis``: it needs no
labels and works where class Gaussians do not (multi-modal classes).

The maps are made by one launch of ``csrc/pixel_knn.hip`` that reads the ``(G, C, h, w)`` features where the model left them
(NCHW, ``channels_last`` or any view; f32 / f16 / bf16): no permute into a ``(G h w, C)`` table, no f32 copy, no
pixels x bank distance matrix.  The bank is a greedy k-center coreset (farthest-point selection, on the device) of a
deterministic subsample of the training pixels, gathered on the device by ``pixel_feature_rows``.  All distances are
SQUARED Euclidean distances.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from .pixel_features import (_check_features, _check_labels, _check_outputs, _hook_of, _hooked_map, pixel_feature_rows)

__all__ = ["PixelKNN", "kcenter_greedy", "get_pixel_knn_maps", "fit_pixel_knn", "PIXEL_KNN_OUTPUTS"]

PIXEL_KNN_OUTPUTS = _hip.PIXKNN_OUTPUTS
_SELECTIONS = ("kcenter", "random")
_MASKED = 255  # the label of a masked pixel in the one-class label map handed to pixel_feature_rows


def kcenter_greedy(rows, n_pick: int, first: int = 0):
    """Greedy k-center (farthest-point) selection on the device: pick 0 is row ``first`` of ``rows`` ``(N, D)``, pick
    ``t + 1`` the row with the largest squared distance to its nearest picked row (lowest index on ties).

    Returns ``(picked int64 (n,), radius f32 (n,))`` as host arrays: ``radius[t]`` is that largest distance at the moment of
    pick ``t`` (``radius[0]`` is ``+inf``; non-increasing).  ``n <= n_pick``: the selection ends early when every remaining
    row duplicates a picked one.  The picks are the same from run to run."""
    if isinstance(rows, Tensor):
        if rows.dim() != 2 or rows.dtype != torch.float32:
            raise ValueError(f"rows must be a float32 (N, D) table, got {tuple(rows.shape)} {rows.dtype}")
    else:
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.dtype != np.float32:
            raise ValueError(f"rows must be a float32 (N, D) table, got {rows.shape} {rows.dtype}")
    n, d = (int(v) for v in rows.shape)
    if n < 1 or d < 1 or d > _hip.KCENTER_MAX_COLUMNS:
        raise ValueError(f"rows are {n} x {d}: at least one row and 1 .. {_hip.KCENTER_MAX_COLUMNS} columns are supported")
    if not isinstance(n_pick, (int, np.integer)) or n_pick < 1:
        raise ValueError(f"n_pick must be a positive integer, got {n_pick!r}")
    if not isinstance(first, (int, np.integer)) or first < 0 or first >= n:
        raise ValueError(f"first must be a row index in 0 .. {n - 1}, got {first!r}")
    device = _hip.require_gpu()
    table = rows.detach() if isinstance(rows, Tensor) else torch.from_numpy(np.ascontiguousarray(rows))
    table = (table if table.is_cuda else table.to(device)).contiguous()
    picked, radius, n_picked = _hip.kcenter_greedy(table, min(int(n_pick), n), int(first))
    n_out = int(n_picked.item())
    return (np.array(_hip.to_host(picked[:n_out]), dtype=np.int64), np.array(_hip.to_host(radius[:n_out]), dtype=np.float32))


class PixelKNN:
    """A memory bank of in-distribution pixel features and the k-nearest-neighbour maps against it.

    ``partial_fit(features, labels=None)`` takes a batch of maps ``(G, C, h, w)``: a pixel is valid where ``labels``
    ``(G, h, w)`` differs from ``ignore_index`` (all pixels without labels); each valid pixel is kept with probability
    ``min(1, rows_per_batch / valid)`` by the counter draw of ``pixel_feature_rows`` (image ids run on over the batches, so
    two half batches keep the rows of one whole batch when the probability is the same).  ``finalize()`` sets the centre
    (``center="mean"``: the mean of the candidates rounded to f32; ``None``: zeros; or a given ``(C,)`` vector), and selects
    ``bank_size`` candidates (all of them if there are fewer): ``selection="kcenter"`` by ``kcenter_greedy`` on the centred
    candidates, started at the candidate farthest from the centre (lowest index on ties); ``"random"`` takes the first
    ``bank_size`` candidates, which the counter draw already thinned at random.

    ``score_maps(features, outputs)`` returns device tensors: ``"kth_distance"`` f32 ``(G, h, w)`` (the anomaly score),
    ``"mean_distance"`` f32 ``(G, h, w)`` (mean of the k), ``"distances"`` f32 ``(G, k, h, w)`` ascending and ``"indices"``
    int32 ``(G, k, h, w)`` into ``bank_`` (lower index first on equal distances).  Distances are squared.  A pixel with a
    NaN or infinite feature has NaN distances and index -1; no other pixel is touched by it.  Results are bit-identical from
    run to run and do not depend on a pixel's position in the batch.

    The fitted state is host arrays: ``bank_`` f64 ``(M, C)`` (the selected rows as they were), ``bank_rows_`` int64 ``(M,)``
    (their indices among the candidates), ``center_`` f64 ``(C,)``, ``coverage_radius_`` (the largest Euclidean distance of
    a candidate to its nearest bank row) and ``n_channels_``.  The kernel's operands - the centred bank ``bank_ - center_``
    and its squared row norms, formed in f64 and rounded to f32 once, the norms from the rounded rows - are a device cache
    that is rebuilt on first use, so a pickle loads on a host without a GPU."""

    _device_cache_attrs = ("_dev",)

    def __init__(self, k: int = 3, bank_size: int = 8192, rows_per_batch: int = 16384, selection: str = "kcenter",
                 center="mean", ignore_index: int = 255, seed: int = 0):
        if not isinstance(k, (int, np.integer)) or k < 1 or k > _hip.PIXKNN_MAX_K:
            raise ValueError(f"k must be an integer in 1 .. {_hip.PIXKNN_MAX_K}, got {k!r}")
        if not isinstance(bank_size, (int, np.integer)) or bank_size < 1 or bank_size > _hip.PIXKNN_MAX_BANK:
            raise ValueError(f"bank_size must be an integer in 1 .. {_hip.PIXKNN_MAX_BANK}, got {bank_size!r}")
        if not isinstance(rows_per_batch, (int, np.integer)) or rows_per_batch < 1:
            raise ValueError(f"rows_per_batch must be a positive integer, got {rows_per_batch!r}")
        if selection not in _SELECTIONS:
            raise ValueError(f"unknown selection {selection!r}: one of {_SELECTIONS}")
        if center is not None and not (isinstance(center, str) and center == "mean"):
            center = np.array(center, dtype=np.float64)
            if center.ndim != 1 or not np.isfinite(center).all():
                raise ValueError("center must be 'mean', None or a finite (C,) vector")
        self.k = int(k)
        self.bank_size = int(bank_size)
        self.rows_per_batch = int(rows_per_batch)
        self.selection = selection
        self.center = center
        self.ignore_index = int(ignore_index)
        self.seed = int(seed)
        self._reset()

    def _reset(self) -> None:
        self._rows = []  # kept rows per batch, host f32 (n_b, C)
        self._images_seen = 0
        self.valid_pixels_ = 0  # valid pixels seen
        self.n_channels_ = None
        self.bank_ = self.bank_rows_ = self.center_ = self.coverage_radius_ = None
        self._dev = None

    def __getstate__(self):
        state = dict(self.__dict__)
        for name in self._device_cache_attrs:
            if name in state:
                state[name] = None
        return state

    # ---- fitting ----------------------------------------------------------------------------------------------------------------
    def partial_fit(self, features: Tensor, labels: Optional[Tensor] = None) -> "PixelKNN":
        _check_features(features, self.n_channels_)
        if labels is not None:
            _check_labels(labels, features)
        device = _hip.require_gpu()
        f = features.detach() if features.is_cuda else features.detach().to(device)
        g, c, h, w = (int(v) for v in f.shape)
        one_class = torch.zeros((g, h, w), dtype=torch.uint8, device=f.device)
        if labels is not None:
            one_class[labels.detach().to(f.device) == self.ignore_index] = _MASKED
        valid = int((one_class == 0).sum().item())
        keep = min(1.0, self.rows_per_batch / max(valid, 1))
        rows, _ = pixel_feature_rows(f, one_class, [keep], _MASKED, self.seed, self._images_seen)
        self._images_seen += g
        self.n_channels_ = c
        self.valid_pixels_ += valid
        if rows.shape[0]:
            self._rows.append(np.array(_hip.to_host(rows), dtype=np.float32))
        self.bank_ = self.bank_rows_ = self.center_ = self.coverage_radius_ = None
        self._dev = None
        return self

    def finalize(self) -> "PixelKNN":
        if not self._rows:
            raise ValueError("finalize() before any valid pixel was seen: call partial_fit first")
        cand = np.concatenate(self._rows, axis=0).astype(np.float64)
        n, c = cand.shape
        if n < self.k:
            raise ValueError(f"k = {self.k} neighbours were asked for but only {n} pixels were kept for the bank")
        if self.center is None:
            center = np.zeros(c)
        elif isinstance(self.center, str):
            center = cand.mean(axis=0)
        else:
            if self.center.shape != (c,):
                raise ValueError(f"center has shape {self.center.shape}, the features have {c} channels")
            center = self.center
        center = center.astype(np.float32).astype(np.float64)  # the f32 centre the kernel subtracts, kept as it is used
        m = min(self.bank_size, n)
        if m < self.k:
            raise ValueError(f"k = {self.k} neighbours were asked for but the bank has {m} rows")
        device = _hip.require_gpu()
        if self.selection == "kcenter":
            centred = (cand - center).astype(np.float32)
            far = (centred.astype(np.float64) ** 2).sum(axis=1)
            picked, _ = kcenter_greedy(centred, m, int(np.argmax(far)))  # (np.argmax: the lowest index on ties)
            if picked.shape[0] < self.k:
                raise ValueError(f"k = {self.k} neighbours were asked for but the candidates hold only {picked.shape[0]} "
                                 "distinct rows")
        else:
            picked = np.arange(m, dtype=np.int64)
        self.bank_rows_ = picked
        self.bank_ = np.ascontiguousarray(cand[picked])
        self.center_ = center
        self._dev = None
        # how well the bank covers the candidates: their nearest-row distances, by the scoring kernel itself on the
        # candidate table taken as a (1, C, 1, n) map
        rows32 = torch.from_numpy(np.ascontiguousarray(cand.astype(np.float32))).to(device)
        nearest = _hip.pixknn_score(rows32.t()[None, :, None, :], *self._device_params(device), 1, ("kth_distance",))
        self.coverage_radius_ = float(np.sqrt(float(nearest["kth_distance"].max().item())))
        return self

    def fit(self, features: Tensor, labels: Optional[Tensor] = None) -> "PixelKNN":
        self._reset()
        return self.partial_fit(features, labels).finalize()

    # ---- scoring ----------------------------------------------------------------------------------------------------------------
    def _device_params(self, device):
        dev = self._dev
        if dev is None or dev[0] != device:
            bank32 = np.ascontiguousarray((self.bank_ - self.center_).astype(np.float32))
            bank_sq = (bank32.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)  # of the rows the kernel multiplies
            dev = (device, torch.from_numpy(self.center_.astype(np.float32)).to(device), torch.from_numpy(bank32).to(device),
                   torch.from_numpy(bank_sq).to(device))
            self._dev = dev
        return dev[1:]

    def score_maps(self, features: Tensor, outputs: Union[str, Sequence[str]] = ("kth_distance",)) -> Dict[str, Tensor]:
        outputs = _check_outputs(outputs, PIXEL_KNN_OUTPUTS)
        if self.bank_ is None:
            raise ValueError("the detector is not fitted: call fit(), or partial_fit() and finalize()")
        _check_features(features, self.n_channels_)
        device = _hip.require_gpu()
        f = features.detach() if features.is_cuda else features.detach().to(device)
        return _hip.pixknn_score(f, *self._device_params(f.device), self.k, outputs)


def get_pixel_knn_maps(dnn_model: torch.nn.Module, input_dataloader, hooked_layer, detector: PixelKNN,
                       outputs: Union[str, Sequence[str]] = ("kth_distance",)) -> Dict[str, Tensor]:
    """The dataloader form (the loop of ``get_pixel_mahalanobis_maps``): one forward pass of ``dnn_model`` per batch of
    ``input_dataloader`` (batches of ``(image, target)``), the feature map caught by ``hooked_layer`` (a ``Hook``, or the
    module to hook) scored by ``detector`` where the model left it, the maps concatenated over the batches -> dict of device
    tensors at the resolution of the hooked layer."""
    outputs = _check_outputs(outputs, PIXEL_KNN_OUTPUTS)
    device = _hip.require_gpu()
    hook, own = _hook_of(hooked_layer)
    parts = []
    try:
        with torch.no_grad():
            for image, _ in input_dataloader:
                dnn_model(image.to(device))
                parts.append(detector.score_maps(_hooked_map(hook), outputs))
    finally:
        if own:
            hook.close()
    if not parts:
        raise ValueError("the dataloader gave no batch")
    return {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}


def fit_pixel_knn(dnn_model: torch.nn.Module, dataloader, hooked_layer, label_stride: int = 1,
                  **detector_kwargs) -> PixelKNN:
    """Fit a ``PixelKNN`` on the feature maps ``hooked_layer`` catches over ``dataloader`` (batches of ``(image, labels)``
    with ``labels`` ``(B, H, W)`` or ``None``).  Labels are brought to the resolution of the features as
    ``labels[..., ::s, ::s]`` with ``s = label_stride``; they only mask pixels out (``ignore_index``).  ``detector_kwargs`` go
    to ``PixelKNN``."""
    if not isinstance(label_stride, (int, np.integer)) or label_stride < 1:
        raise ValueError(f"label_stride must be a positive integer, got {label_stride!r}")
    detector = PixelKNN(**detector_kwargs)
    device = _hip.require_gpu()
    hook, own = _hook_of(hooked_layer)
    try:
        with torch.no_grad():
            for image, labels in dataloader:
                dnn_model(image.to(device))
                s = int(label_stride)
                detector.partial_fit(_hooked_map(hook), None if labels is None else labels[..., ::s, ::s])
    finally:
        if own:
            hook.close()
    return detector.finalize()
