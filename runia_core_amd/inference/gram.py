"""The Gram-matrix out-of-distribution detector of Sastry & Oore, "Detecting Out-of-Distribution Examples with Gram
Matrices" (ICML 2020) - the ``gram`` row of the OpenOOD tables - scored from the hooked feature maps of several layers.

For a layer's map ``F`` (C channels, HW positions) and a power ``p`` the paper forms ``G_p = F^p (F^p)^T``, takes the
``p``-th root and sums each row; the minimum and maximum of every such value over the training images of a (predicted)
class are recorded, and a test image's deviation from those ranges, normalised per layer by its mean on held-out
in-distribution data, is the score.  The row sum never needs the ``(C, C)`` matrix::

    t[b, p, c] = sum_x F[b, c, x]^p * S_p[b, x]      S_p[b, x] = sum_j F[b, j, x]^p      v = sign(t) |t|^(1/p)

``csrc/gram.hip`` computes it with one read of the map where the model left it (NCHW, ``channels_last``, any view; f32 /
f16 / bf16) and folds or scores it in the same call.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ..feature_extraction.utils import Hook

__all__ = ["GramDetector", "gram_statistics", "fit_gram_detector", "get_gram_scores"]

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_LABEL_DTYPES = (torch.int32, torch.int64)


def _check_powers(powers) -> int:
    if not isinstance(powers, (int, np.integer)) or isinstance(powers, bool) or not 1 <= powers <= _hip.GRAM_MAX_POWERS:
        raise ValueError(f"powers must be an integer in 1 .. {_hip.GRAM_MAX_POWERS}, got {powers!r}")
    return int(powers)


def _check_map(fmap, name: str = "fmap") -> None:
    if not isinstance(fmap, Tensor) or fmap.dim() not in (2, 4):
        raise ValueError(f"{name} must be a (B, C, H, W) or (B, F) tensor, got shape {tuple(getattr(fmap, 'shape', ()))}")
    if fmap.dtype not in _DTYPES:
        raise ValueError(f"unsupported {name} dtype {fmap.dtype} (float32, float16, bfloat16)")
    if any(int(s) < 1 for s in fmap.shape[1:]):
        raise ValueError(f"{name} of shape {tuple(fmap.shape)} has an empty dimension")


def _on_device(t: Tensor, device) -> Tensor:
    t = t.detach()
    return t if t.is_cuda else t.to(device)


def gram_statistics(fmap: Tensor, powers: int = 10) -> Tensor:
    """The Gram statistics ``v[b, p - 1, c] = sign(t) |t|^(1/p)``, ``t = sum_j G_p[c, j]``, ``p = 1 .. powers``, of one hooked
    map ``(B, C, H, W)`` or ``(B, F)`` (``H = W = 1``) -> f32 device tensor ``(B, powers, C)``.  The map is read in place."""
    powers = _check_powers(powers)
    _check_map(fmap)
    device = _hip.require_gpu()
    return _hip.gram_layer_stats(_on_device(fmap, device), powers)


class GramDetector:
    """Per-class, per-layer ranges of the Gram statistics, and the deviation of new images from them.

    ``fit_batch(maps, labels)`` takes one map per hooked layer and the model's predicted labels and widens the ranges
    ``mins_[l]`` / ``maxs_[l]`` (f32 ``(n_classes, powers, C_l)``) of the rows ``labels[b]``; a training set is streamed
    through it batch by batch, in any order - min and max do not depend on it.  ``calibrate_batch(maps, labels)`` adds the
    layer deviations of held-out in-distribution images to ``dev_sum_`` / ``dev_count_``; the paper normalises every layer
    by that mean.  ``layer_deviations`` returns ``(B, L)``::

        dev_l[b] = sum_{p,c} relu(mins - v) / |mins + 1e-6| + relu(v - maxs) / |maxs + 1e-6|      at row labels[b]

    ``score`` returns ``-sum_l dev_l / mean_val_dev_l``: HIGHER MEANS IN-DISTRIBUTION, as everywhere else in this library;
    the paper's total deviation is ``-score``.  An image of a class nothing was fitted to, or with a label outside
    ``[0, n_classes)``, has infinite deviations and scores ``-inf``.

    The fitted state is host arrays (``mins_``, ``maxs_``: lists of f32 arrays; ``dev_sum_`` f64, ``dev_count_``); the
    device tables are a cache, so a pickle loads on a host without a GPU."""

    def __init__(self, n_classes: int, powers: int = 10):
        if not isinstance(n_classes, (int, np.integer)) or isinstance(n_classes, bool) or n_classes < 1:
            raise ValueError(f"n_classes must be a positive integer, got {n_classes!r}")
        self.n_classes = int(n_classes)
        self.powers = _check_powers(powers)
        self._mins: Optional[List[np.ndarray]] = None
        self._maxs: Optional[List[np.ndarray]] = None
        self.dev_sum_: Optional[np.ndarray] = None
        self.dev_count_ = 0
        self._keys = None   # device (kmin, kmax) per layer while fitting; the host arrays are then behind
        self._dev = None    # (device, [(mins, maxs) f32 per layer])
        self._cal = None    # device (sum f64 (L,), count) not yet added to dev_sum_ / dev_count_

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def _pull(self) -> None:
        if self._keys is not None:
            self._mins = [np.array(_hip.to_host(_hip.gram_keys_to_values(a)), dtype=np.float32) for a, _ in self._keys]
            self._maxs = [np.array(_hip.to_host(_hip.gram_keys_to_values(b)), dtype=np.float32) for _, b in self._keys]
            self._keys = None
        if self._cal is not None:
            s, n = self._cal
            self.dev_sum_ = (0.0 if self.dev_sum_ is None else self.dev_sum_) + np.array(_hip.to_host(s), dtype=np.float64)
            self.dev_count_ += n
            self._cal = None

    def _set_tables(self, name: str, tables) -> None:
        self._pull()
        tables = None if tables is None else [np.ascontiguousarray(t, dtype=np.float32) for t in tables]
        for t in tables or ():
            if t.ndim != 3 or t.shape[:2] != (self.n_classes, self.powers):
                raise ValueError(f"{name}: one ({self.n_classes}, {self.powers}, C) array per layer, got {t.shape}")
        setattr(self, "_" + name, tables)
        self._dev = None

    mins_ = property(lambda self: (self._pull(), self._mins)[1], lambda self, v: self._set_tables("mins", v))
    maxs_ = property(lambda self: (self._pull(), self._maxs)[1], lambda self, v: self._set_tables("maxs", v))

    def __getstate__(self):
        self._pull()
        state = dict(self.__dict__)
        state["_keys"] = state["_dev"] = state["_cal"] = None
        return state

    @property
    def mean_deviations_(self) -> np.ndarray:
        """``E_val[dev_l]`` per layer, f64 ``(L,)``."""
        self._pull()
        if self.dev_sum_ is None or self.dev_count_ < 1:
            raise ValueError("the detector is not calibrated: call calibrate_batch on held-out in-distribution data")
        return self.dev_sum_ / float(self.dev_count_)

    # ---- checks -----------------------------------------------------------------------------------------------------------------
    def _inputs(self, maps, labels, channels=None):
        if isinstance(maps, Tensor) or not isinstance(maps, Sequence) or len(maps) == 0:
            raise ValueError("maps must be a non-empty sequence of tensors, one per hooked layer")
        for i, m in enumerate(maps):
            _check_map(m, f"maps[{i}]")
        b = int(maps[0].shape[0])
        if any(int(m.shape[0]) != b for m in maps):
            raise ValueError(f"the maps have different batch sizes: {[int(m.shape[0]) for m in maps]}")
        if not isinstance(labels, Tensor) or labels.dtype not in _LABEL_DTYPES or tuple(labels.shape) != (b,):
            raise ValueError(f"labels must be an int32 or int64 tensor of shape ({b},), got "
                             f"{tuple(getattr(labels, 'shape', ()))} {getattr(labels, 'dtype', type(labels).__name__)}")
        if channels is not None and [int(m.shape[1]) for m in maps] != channels:
            raise ValueError(f"the maps have {[int(m.shape[1]) for m in maps]} channels, the detector was fitted on {channels}")
        device = _hip.require_gpu()
        maps = [_on_device(m, device) for m in maps]
        return maps, labels.detach().to(maps[0].device)

    # ---- fitting ----------------------------------------------------------------------------------------------------------------
    def fit_batch(self, maps: Sequence[Tensor], labels: Tensor) -> "GramDetector":
        have = self._keys is not None or self._mins is not None
        channels = None
        if self._keys is not None:
            channels = [int(a.shape[2]) for a, _ in self._keys]
        elif self._mins is not None:
            channels = [int(a.shape[2]) for a in self._mins]
        maps, labels = self._inputs(maps, labels, channels)
        device = maps[0].device
        if self._keys is None or self._keys[0][0].device != device:
            self._pull()
            if have:
                f32 = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
                self._keys = [(_hip.gram_values_to_keys(f32(a)), _hip.gram_values_to_keys(f32(b)))
                              for a, b in zip(self._mins, self._maxs)]
            else:
                self._keys = [_hip.gram_key_tables(self.n_classes, self.powers, int(m.shape[1]), device) for m in maps]
        for m, (kmin, kmax) in zip(maps, self._keys):
            _hip.gram_layer_fit(m, labels, kmin, kmax)
        self._dev = None
        return self

    # ---- scoring ----------------------------------------------------------------------------------------------------------------
    def _tables(self, device):
        self._pull()
        if self._mins is None or self._maxs is None:
            raise ValueError("the detector is not fitted: call fit_batch first")
        if self._dev is None or self._dev[0] != device:
            f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)  # noqa: E731
            self._dev = (device, [(f32(a), f32(b)) for a, b in zip(self._mins, self._maxs)])
        return self._dev[1]

    def layer_deviations(self, maps: Sequence[Tensor], labels: Tensor) -> Tensor:
        """f32 device tensor ``(B, L)``: the deviation of every image from the fitted ranges of its class, per layer."""
        self._pull()
        channels = None if self._mins is None else [int(a.shape[2]) for a in self._mins]
        maps, labels = self._inputs(maps, labels, channels)
        tables = self._tables(maps[0].device)
        return torch.stack([_hip.gram_layer_deviation(m, labels, lo, hi) for m, (lo, hi) in zip(maps, tables)], dim=1)

    def calibrate_batch(self, maps: Sequence[Tensor], labels: Tensor) -> "GramDetector":
        dev = self.layer_deviations(maps, labels)
        s, n = dev.to(torch.float64).sum(dim=0), int(dev.shape[0])
        self._cal = (s, n) if self._cal is None else (self._cal[0] + s, self._cal[1] + n)
        return self

    def score(self, maps: Sequence[Tensor], labels: Tensor) -> Tensor:
        """f32 device tensor ``(B,)``: ``-sum_l dev_l / mean_val_dev_l``.  Higher means in-distribution; the total deviation
        of the paper is ``-score``."""
        mean = self.mean_deviations_
        dev = self.layer_deviations(maps, labels)
        inv = torch.from_numpy((1.0 / mean).astype(np.float32)).to(dev.device)
        return -(dev * inv).sum(dim=1)


def _hooks_of(hooked_layers):
    if isinstance(hooked_layers, (Hook, torch.nn.Module)) or len(hooked_layers) == 0:
        raise ValueError("hooked_layers must be a non-empty sequence of Hooks or of the modules to hook")
    hooks, own = [], []
    for layer in hooked_layers:
        if isinstance(layer, Hook):
            hooks.append(layer)
        elif isinstance(layer, torch.nn.Module):
            hooks.append(Hook(layer))
            own.append(hooks[-1])
        else:
            for h in own:
                h.close()
            raise ValueError(f"hooked_layers holds a {type(layer).__name__}: a Hook or the module to hook is needed")
    return hooks, own


def _forward(dnn_model, hooks, image, device):
    """One forward pass: ``(hooked maps, predicted labels)``, the labels being the model's argmax taken on the device."""
    out = dnn_model(image.to(device))
    if isinstance(out, dict) and "out" in out:
        out = out["out"]
    return [h.output for h in hooks], out.argmax(dim=1)


def fit_gram_detector(dnn_model: torch.nn.Module, train_loader, val_loader, hooked_layers, n_classes: int,
                      powers: int = 10) -> GramDetector:
    """Fit a ``GramDetector`` on the maps ``hooked_layers`` (Hooks, or the modules to hook) catch over ``train_loader``, then
    calibrate its per-layer normalisation over ``val_loader`` (held-out in-distribution data).  Both give batches of
    ``(image, target)``; the targets are not used: the classes are the model's own predictions."""
    detector = GramDetector(n_classes, powers)
    hooks, own = _hooks_of(hooked_layers)
    device = _hip.require_gpu()
    try:
        with torch.no_grad():
            for image, _ in train_loader:
                detector.fit_batch(*_forward(dnn_model, hooks, image, device))
            for image, _ in val_loader:
                detector.calibrate_batch(*_forward(dnn_model, hooks, image, device))
    finally:
        for h in own:
            h.close()
    detector._pull()
    return detector


def get_gram_scores(dnn_model: torch.nn.Module, loader, hooked_layers, detector: GramDetector) -> Tensor:
    """``detector.score`` of every image of ``loader`` (batches of ``(image, target)``), concatenated: f32 device tensor."""
    hooks, own = _hooks_of(hooked_layers)
    device = _hip.require_gpu()
    parts = []
    try:
        with torch.no_grad():
            for image, _ in loader:
                parts.append(detector.score(*_forward(dnn_model, hooks, image, device)))
    finally:
        for h in own:
            h.close()
    if not parts:
        raise ValueError("the dataloader gave no batch")
    return torch.cat(parts, dim=0)
