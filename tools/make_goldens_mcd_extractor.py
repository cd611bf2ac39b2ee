#!/usr/bin/env python3
"""Fixtures of the reference's classic MC-dropout extractor, generated from its own ``feature_extraction/image_level.py`` ->
``tests/golden/ref_mcd_extractor.npz``: ``MCDSamplesExtractor.get_ls_samples`` (``fullmean``, ``mean``, three ``avgpool``
settings, the ``FC`` form, the raw-prediction return) and the two deprecated function forms
(``get_latent_representation_mcd_samples`` with ``Conv`` and ``FC``, ``deeplabv3p_get_ls_mcd_samples``).

Same by-path import recipe and stand-ins as ``tools/make_goldens_box_extraction.py``.  A model's dropout stream on the
device can never equal the CPU's, so the passes are made deterministic: a seeded table of hooked activations
``(images, mcd, C, H, W)`` and a replay stub whose hooked layer emits entry ``(image, pass)`` on its k-th call
(``k = image * mcd + pass`` with one image per batch, which is what the reference's ``reshape(1, -1)`` assumes).

Only DATA is written (the activation tables, the stub's predictions, the reference's results); the same bytes on every run.

Usage (from the repository root, with the reference's source tree where ``make_goldens_r2.REF`` names it):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_mcd_extractor.py
"""
from __future__ import annotations

import io
import os
import sys
import warnings
import zipfile

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

import make_goldens_box_extraction as mbe  # noqa: E402
import make_goldens_r2 as r2  # noqa: E402

OUT = r2.OUT
N_IMAGES, MCD = 4, 5
C, H, W = 6, 10, 7  # odd sizes: W not a multiple of 4, H != W
AVGPOOL_SETTINGS = [(3, 2, 1), (4, 3, 0), (4, 3, 2)]  # (kernel, stride, padding); H and W are not multiples of 3
FC_FEATURES, DEP_FC_ROWS, N_PRED = 23, 9, 3
PRED_SCALE = 2.0  # keyword argument of the stub's forward: reaches the model only with return_raw_predictions


class _Emit(torch.nn.Module):
    def forward(self, x):
        return x


class ReplayModel(torch.nn.Module):
    """The hooked layer emits ``acts[image, pass]`` on the k-th forward call (batches of ``batch`` images: the images of
    batch ``k // mcd``, pass ``k % mcd``); the prediction is ``preds[image, pass] * scale``."""

    def __init__(self, acts, preds=None, batch=1, drop_batch_dim=False):
        super().__init__()
        self.hooked = _Emit()
        self.register_buffer("acts", torch.as_tensor(np.asarray(acts)))
        self.register_buffer("preds", None if preds is None else torch.as_tensor(np.asarray(preds)))
        self.batch, self.drop_batch_dim, self.calls = batch, drop_batch_dim, 0

    def forward(self, image, scale=1.0):
        bi, s = divmod(self.calls, self.acts.shape[1])
        self.calls += 1
        lo = bi * self.batch
        self.hooked(self.acts[lo, s] if self.drop_batch_dim else self.acts[lo:lo + image.shape[0], s])
        return image if self.preds is None else self.preds[lo:lo + image.shape[0], s] * scale


def _loader():
    return DataLoader(TensorDataset(torch.zeros(N_IMAGES, 1), torch.zeros(N_IMAGES)), batch_size=1)


def main():
    mbe._stubs()
    import runia_core.feature_extraction.image_level as fil
    from runia_core.feature_extraction.utils import Hook

    g = np.random.default_rng(20261016)
    relu = lambda shape: (np.maximum(g.standard_normal(shape), 0) + 0.25 * g.random(shape)).astype(np.float32)  # noqa: E731
    cases = {
        "acts": relu((N_IMAGES, MCD, C, H, W)),
        "acts_fc": relu((N_IMAGES, MCD, FC_FEATURES)),
        "acts_dep_fc": relu((N_IMAGES, MCD, DEP_FC_ROWS, FC_FEATURES)),
        "preds": g.standard_normal((N_IMAGES, MCD, N_PRED)).astype(np.float32),
        "pred_scale": np.array([PRED_SCALE], np.float64),
        "avgpool_settings": np.array(AVGPOOL_SETTINGS, np.int64),
    }
    cpu = torch.device("cpu")

    def extract(acts, preds=None, **kw):
        model = ReplayModel(acts, preds)
        hook = Hook(model.hooked)
        ext = fil.MCDSamplesExtractor(model=model, hooked_layers=[hook], device=cpu, mcd_nro_samples=MCD, **kw)
        out = ext.get_ls_samples(_loader(), **({"scale": PRED_SCALE} if preds is not None else {}))
        hook.close()
        return out

    for method in ("fullmean", "mean"):
        cases[f"ref_{method}"] = extract(cases["acts"], layer_type="Conv", reduction_method=method).numpy()
    for k, s, p in AVGPOOL_SETTINGS:
        cases[f"ref_avgpool_{k}_{s}_{p}"] = extract(cases["acts"], layer_type="Conv", reduction_method="avgpool",
                                                     avg_pooling_parameters=(k, s, p)).numpy()
    cases["ref_fc"] = extract(cases["acts_fc"], layer_type="FC", reduction_method="fullmean").numpy()
    samples, raw = extract(cases["acts"], cases["preds"], layer_type="Conv", reduction_method="fullmean",
                           return_raw_predictions=True)
    cases["ref_raw_samples"], cases["ref_raw_preds"] = samples.numpy(), raw.numpy()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for acts, layer_type, key, drop in ((cases["acts"], "Conv", "ref_dep_conv", False),
                                            (cases["acts_dep_fc"], "FC", "ref_dep_fc", True)):
            model = ReplayModel(acts, drop_batch_dim=drop)
            hook = Hook(model.hooked)
            cases[key] = fil.get_latent_representation_mcd_samples(model, _loader(), MCD, hook, layer_type).numpy()
            hook.close()
        module = torch.nn.Module()
        module.deeplab_v3plus_model = ReplayModel(cases["acts"])
        hook = Hook(module.deeplab_v3plus_model.hooked)
        cases["ref_dep_deeplab"] = fil.deeplabv3p_get_ls_mcd_samples(module, _loader(), MCD, hook).numpy()
        hook.close()
    for key in sorted(cases):
        print(f"  {key}: {cases[key].shape} {cases[key].dtype}")

    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(cases):
            arr = io.BytesIO()
            np.save(arr, np.ascontiguousarray(cases[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, arr.getvalue())
    path = os.path.join(OUT, "ref_mcd_extractor.npz")
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {os.path.abspath(path)} ({len(buf.getvalue())} bytes)")


if __name__ == "__main__":
    main()
