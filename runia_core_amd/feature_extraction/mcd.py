"""The classic MC-dropout extractor (reference ``runia_core/feature_extraction/image_level.py:252-410`` and its two
deprecated function forms, ``:580-694``): ``mcd_nro_samples`` stochastic forward passes of the USER'S model per batch, the
hooked activation reduced after every pass.

The passes are the model's own (PyTorch-ROCm).  What follows each pass is one ``runia_mcd_reduce_rows`` launch
(csrc/mcd_reduce.hip): the hooked activation of the whole batch - in the dtype and memory layout the model produced - is
reduced (``fullmean`` / ``mean`` / ``avgpool`` / the FC copy) straight into the pass's rows of one ``(B * mcd, D)`` f32
block per batch, and the blocks are concatenated once at the end.  No per-pass tensor, no host round trip; the samples stay
on the device, as with ``FastMCDSamplesExtractor``.

Row order: every image owns ``mcd_nro_samples`` consecutive rows (image-major), which is what ``get_dl_h_z`` and
``LaRExInference`` read.  With one image per batch that is the reference's table, row for row.  With larger batches the
reference's ``reshape(1, -1)`` folds the batch into the row width; here every image keeps rows of its own.

These names are not part of ``feature_extraction.image_level`` here (that module mirrors the in-scope names of the
reference's file); they are exported from ``runia_core_amd.feature_extraction`` and from the package.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union
from warnings import warn

import torch
from torch import Tensor
from torch.utils.data import DataLoader

from .. import _hip
from .utils import Hook

__all__ = ["MCDSamplesExtractor", "deeplabv3p_get_ls_mcd_samples", "get_latent_representation_mcd_samples"]


def _as_map(latent: Tensor) -> Tensor:
    """The hooked activation as the (B, C, H, W) or (B, F) view the kernel reads."""
    if isinstance(latent, (tuple, list)):
        latent = latent[0]
    assert isinstance(latent, Tensor), "the hooked layer did not produce a tensor"
    if latent.dim() in (2, 4):
        return latent
    if latent.dim() == 3:  # (B, C, L): a 1-D map
        return latent.unsqueeze(2)
    raise ValueError(f"cannot reduce a hooked activation of shape {tuple(latent.shape)}")


class _RowBlock:
    """The (B * mcd, D) block of one batch: allocated when D is first known, filled pass after pass."""

    def __init__(self, mcd: int):
        self.mcd, self.table = mcd, None

    def write(self, latent: Tensor, s: int, mode: str, pooling=None) -> None:
        if not latent.is_cuda:
            raise _hip.RuniaHipError("MC-dropout extraction runs on the device only: the hooked activation is on "
                                     f"{latent.device} (move the model to the GPU)")
        if self.table is None:
            d = _hip.mcd_row_width(latent.shape, mode, pooling)
            self.table = torch.empty((latent.shape[0] * self.mcd, d), dtype=torch.float32, device=latent.device)
        _hip.mcd_reduce_rows(latent, self.table, mode, row0=s, row_step=self.mcd, avg_pooling_parameters=pooling)


def _mcd_loop(forward, read_hook, data_loader, device, mcd: int, mode: str, pooling=None, keep_predictions: bool = False):
    """The shared loop: per batch ``mcd`` calls of ``forward(image)``, each followed by one launch into the batch's
    block.  Returns (blocks, predictions per batch or None)."""
    blocks, predictions = [], [] if keep_predictions else None
    with torch.no_grad():
        for image, _ in data_loader:
            image = image.to(device)
            block = _RowBlock(mcd)
            passes = []
            for s in range(mcd):
                pred = forward(image)
                if keep_predictions:
                    passes.append(pred)
                block.write(read_hook(), s, mode, pooling)
            if block.table is not None:
                blocks.append(block.table)
            if keep_predictions:
                predictions.append(torch.cat(passes, dim=0))
    return blocks, predictions


class MCDSamplesExtractor:
    """Monte-Carlo samples from any torch model with Dropout / DropBlock layers of its own: the classic MCD algorithm,
    ``mcd_nro_samples`` inferences per batch.  Constructor, attributes and ``get_ls_samples`` as the reference's class
    (``return_stds``, ``dropblock_probs`` and ``dropblock_sizes`` are accepted and, as there, not used)."""

    def __init__(
        self,
        model: torch.nn.Module,
        hooked_layers: List[Hook],
        device: torch.device,
        layer_type: str,
        reduction_method: str,
        return_raw_predictions: bool = False,
        return_stds: bool = False,
        mcd_nro_samples: int = 1,
        hook_layer_output: bool = True,
        dropblock_probs: Union[float, List] = 0.0,
        dropblock_sizes: Union[int, List] = 0,
        avg_pooling_parameters: Union[Tuple, List, None] = None,
    ):
        self.model = model
        self.hooked_layers = hooked_layers
        self.device = device
        self.return_raw_predictions = return_raw_predictions
        self.return_stds = return_stds
        self.mcd_nro_samples = mcd_nro_samples
        self.hook_layer_output = hook_layer_output
        self.dropblock_probs = dropblock_probs
        self.dropblock_sizes = dropblock_sizes
        self.hooked_layer = self.hooked_layers[0]
        assert layer_type in ("FC", "Conv"), "Layer type must be either 'FC' or 'Conv'"
        assert reduction_method in (
            "mean",
            "fullmean",
            "avgpool",
        ), "Only mean, fullmean and avg pool reduction methods supported"
        if avg_pooling_parameters is not None:
            assert len(avg_pooling_parameters) == 3, "Three parameters are needed for average pooling"
        self.layer_type = layer_type
        self.reduction_method = reduction_method
        self.avg_pooling_parameters = avg_pooling_parameters

    def _mode(self) -> str:
        # FC: "it is already a 1d tensor" - the activation is flattened as it is
        return "copy" if self.layer_type == "FC" else self.reduction_method

    def get_ls_samples(self, data_loader: DataLoader, **kwargs) -> Union[Tuple[Tensor, Tensor], Tensor]:
        """MC-dropout inference over a dataloader -> ``(N * mcd_nro_samples, D)`` f32 samples on the device, image-major;
        with ``return_raw_predictions`` also the raw predictions, in the shape the reference returns them.  As in the
        reference, ``**kwargs`` reach the model only when the raw predictions are requested."""
        assert isinstance(data_loader, DataLoader)
        pass_kwargs = kwargs if self.return_raw_predictions else {}
        pooling = self.avg_pooling_parameters if self._mode() == "avgpool" else None
        blocks, predictions = _mcd_loop(
            lambda image: self.model(image, **pass_kwargs),
            lambda: _as_map(self.hooked_layer.output),  # the reference reads .output whatever hook_layer_output says
            data_loader, self.device, self.mcd_nro_samples, self._mode(), pooling, self.return_raw_predictions)
        samples = torch.cat(blocks, dim=0)
        print("MCD N_samples: ", samples.shape[1])
        if not self.return_raw_predictions:
            return samples
        # the reference extends a list with the (B * mcd, ...) predictions of every batch - that iterates their first
        # dimension - and concatenates the pieces along dim 0: the first two dimensions end up merged
        raw = torch.cat(predictions, dim=0)
        raw = raw.flatten(0, 1) if raw.dim() >= 2 else torch.cat(list(raw.unbind(0)), dim=0)
        return samples, raw


def deeplabv3p_get_ls_mcd_samples(model_module, dataloader: DataLoader, mcd_nro_samples: int,
                                  hook_dropout_layer: Hook) -> Tensor:
    """Deprecated function form for a Deeplabv3+ Lightning module: ``model_module.deeplab_v3plus_model`` is run
    ``mcd_nro_samples`` times per batch, the hooked map reduced by its full mean."""
    warn("This method is deprecated. Use one of the Extractor classes instead", DeprecationWarning, stacklevel=2)
    assert isinstance(model_module, torch.nn.Module), "model_module must be a pytorch model"
    assert isinstance(dataloader, DataLoader), "dataloader must be a DataLoader"
    assert isinstance(mcd_nro_samples, int), "mcd_nro_samples must be an integer"
    assert isinstance(hook_dropout_layer, Hook), "hook_dropout_layer must be an Hook"
    device = _hip.require_gpu()
    blocks, _ = _mcd_loop(model_module.deeplab_v3plus_model, lambda: _as_map(hook_dropout_layer.output), dataloader,
                          device, mcd_nro_samples, "fullmean")
    return torch.cat(blocks, dim=0)


def _fc_rows_as_map(latent: Tensor) -> Tensor:
    """Deprecated FC branch: ``torch.mean(latent, dim=1).reshape(1, -1)`` of a (rows, F) activation is ONE row of
    ``rows`` values - the full mean of a (1, rows, 1, F) view."""
    if isinstance(latent, (tuple, list)):
        latent = latent[0]
    if latent.dim() != 2:
        raise ValueError(f"the deprecated FC form reduces a (rows, features) activation, got {tuple(latent.shape)}")
    return latent[None, :, None, :]


def get_latent_representation_mcd_samples(dnn_model: torch.nn.Module, dataloader: DataLoader, mcd_nro_samples: int,
                                          layer_hook: Hook, layer_type: str) -> Tensor:
    """Deprecated function form: ``Conv`` -> full mean of the hooked map; ``FC`` -> mean over dim 1 of the hooked
    (rows, features) activation, one row per pass."""
    warn("This method is deprecated. Use one of the Extractor classes instead", DeprecationWarning, stacklevel=2)
    assert isinstance(dnn_model, torch.nn.Module), "dnn_model must be a pytorch model"
    assert isinstance(dataloader, DataLoader), "dataloader must be a DataLoader"
    assert isinstance(mcd_nro_samples, int), "mcd_nro_samples must be an integer"
    assert isinstance(layer_hook, Hook), "layer_hook must be an Hook"
    assert layer_type in ("FC", "Conv"), "Layer type must be either 'FC' or 'Conv'"
    device = _hip.require_gpu()
    read = (lambda: _as_map(layer_hook.output)) if layer_type == "Conv" else (lambda: _fc_rows_as_map(layer_hook.output))
    blocks, _ = _mcd_loop(dnn_model, read, dataloader, device, mcd_nro_samples, "fullmean")
    return torch.cat(blocks, dim=0)
