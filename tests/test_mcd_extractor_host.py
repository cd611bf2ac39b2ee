"""``MCDSamplesExtractor`` and ``runia_mcd_reduce_rows`` without a GPU: where the names live, the constructor's and the
deprecated functions' assertions, the ABI entry, the wrapper's refusals (all before any launch) and the fixture's own
consistency (tests/golden/ref_mcd_extractor.npz against an f64 NumPy reduction of its activation tables)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from conftest import ROOT, load_npz, rel_err
from runia_core_amd import _hip
from runia_core_amd.feature_extraction import (
    Hook,
    MCDSamplesExtractor,
    deeplabv3p_get_ls_mcd_samples,
    get_latent_representation_mcd_samples,
)

TOL = 1e-5  # |d| <= TOL * max(1, |ref|), BASELINE.md section 5
AVGPOOL_SETTINGS = [(3, 2, 1), (4, 3, 0), (4, 3, 2)]  # as tools/make_goldens_mcd_extractor.py


class _Emit(torch.nn.Module):
    def forward(self, x):
        return x


class ReplayModel(torch.nn.Module):
    """The stub of tools/make_goldens_mcd_extractor.py: the hooked layer emits ``acts[image, pass]`` on the k-th forward
    call (batches of ``batch`` images: the images of batch ``k // mcd``, pass ``k % mcd``); the prediction is
    ``preds[image, pass] * scale``."""

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


def np_reduce(x, mode, params=None):
    """f64 host reduction of maps x (N, C, H, W) -> (N, D): what one pass writes per image."""
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    if mode == "fullmean":
        return x.mean(axis=(2, 3))
    if mode == "mean":
        return x.mean(axis=3).reshape(n, c * h)
    if mode == "copy":
        return x.reshape(n, -1)
    k, st, p = params
    xp = np.zeros((n, c, h + 2 * p, w + 2 * p))
    xp[:, :, p:p + h, p:p + w] = x
    ho, wo = (h + 2 * p - k) // st + 1, (w + 2 * p - k) // st + 1
    out = np.empty((n, c, ho, wo))
    for i in range(ho):
        for j in range(wo):
            out[:, :, i, j] = xp[:, :, i * st:i * st + k, j * st:j * st + k].sum(axis=(2, 3)) / (k * k)
    return out.reshape(n, -1)


def _model():
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Dropout2d(0.5))


def _loader(n=2):
    return DataLoader(TensorDataset(torch.zeros(n, 1), torch.zeros(n)), batch_size=1)


def test_names_live_in_the_package_and_not_in_the_mirrored_module():
    import runia_core_amd
    import runia_core_amd.feature_extraction as fe
    import runia_core_amd.feature_extraction.image_level as il

    for name in ("MCDSamplesExtractor", "deeplabv3p_get_ls_mcd_samples", "get_latent_representation_mcd_samples"):
        assert hasattr(fe, name) and getattr(runia_core_amd, name) is getattr(fe, name)
        assert not hasattr(il, name)


def test_constructor_defaults_attributes_and_assertions():
    m = _model()
    hook = Hook(m[1])
    ext = MCDSamplesExtractor(m, [hook], torch.device("cpu"), "Conv", "avgpool", avg_pooling_parameters=(3, 2, 1))
    assert ext.hooked_layer is hook and ext.layer_type == "Conv" and ext.reduction_method == "avgpool"
    assert ext.avg_pooling_parameters == (3, 2, 1) and ext.mcd_nro_samples == 1
    assert ext.return_raw_predictions is False and ext.return_stds is False and ext.hook_layer_output is True
    assert ext.dropblock_probs == 0.0 and ext.dropblock_sizes == 0
    with pytest.raises(AssertionError, match="Layer type must be either 'FC' or 'Conv'"):
        MCDSamplesExtractor(m, [hook], torch.device("cpu"), "RPN", "mean")
    with pytest.raises(AssertionError, match="Only mean, fullmean and avg pool reduction methods supported"):
        MCDSamplesExtractor(m, [hook], torch.device("cpu"), "Conv", "std")
    for bad in ((3, 2), (3, 2, 1, 0)):
        with pytest.raises(AssertionError, match="Three parameters are needed for average pooling"):
            MCDSamplesExtractor(m, [hook], torch.device("cpu"), "Conv", "avgpool", avg_pooling_parameters=bad)
    with pytest.raises(AssertionError):
        ext.get_ls_samples([(torch.zeros(1, 3, 8, 8), 0)])  # not a DataLoader
    hook.close()


def test_deprecated_functions_warn_and_assert_on_their_argument_types():
    m = _model()
    hook = Hook(m[1])
    bad_calls = [
        (get_latent_representation_mcd_samples, ("model", _loader(), 2, hook, "Conv"), "dnn_model must be a pytorch model"),
        (get_latent_representation_mcd_samples, (m, [1, 2], 2, hook, "Conv"), "dataloader must be a DataLoader"),
        (get_latent_representation_mcd_samples, (m, _loader(), 2.0, hook, "Conv"), "mcd_nro_samples must be an integer"),
        (get_latent_representation_mcd_samples, (m, _loader(), 2, m[1], "Conv"), "layer_hook must be an Hook"),
        (get_latent_representation_mcd_samples, (m, _loader(), 2, hook, "RPN"), "Layer type must be either 'FC' or 'Conv'"),
        (deeplabv3p_get_ls_mcd_samples, ("model", _loader(), 2, hook), "model_module must be a pytorch model"),
        (deeplabv3p_get_ls_mcd_samples, (m, [1, 2], 2, hook), "dataloader must be a DataLoader"),
        (deeplabv3p_get_ls_mcd_samples, (m, _loader(), "2", hook), "mcd_nro_samples must be an integer"),
        (deeplabv3p_get_ls_mcd_samples, (m, _loader(), 2, None), "hook_dropout_layer must be an Hook"),
    ]
    for fn, args, message in bad_calls:
        with pytest.warns(DeprecationWarning, match="This method is deprecated"):
            with pytest.raises(AssertionError, match=re.escape(message)):
                fn(*args)
    hook.close()


def test_entry_point_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "runia_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+runia_mcd_reduce_rows\s*\(", header)
    for mode in ("FULLMEAN", "MEAN", "AVGPOOL", "COPY"):
        assert f"RUNIA_MCD_{mode}" in header
    assert "runia_mcd_reduce_rows" in _hip.exported_symbols()
    lib = ctypes.CDLL(os.path.join(ROOT, "runia_core_amd", "librunia_hip.so"))
    assert hasattr(lib, "runia_mcd_reduce_rows")
    assert _hip.load_library().runia_abi_version() == 6  # the entry is additive


def test_wrapper_refuses_bad_arguments_before_any_launch(monkeypatch):
    def no_library(*a, **k):
        raise RuntimeError("the library was reached")

    monkeypatch.setattr(_hip, "load_library", no_library)
    x = torch.zeros(2, 3, 4, 5)
    with pytest.raises(AssertionError, match="must be a device tensor"):
        _hip.mcd_reduce_rows(x, torch.zeros(2, 3), "fullmean")
    for dtype in (torch.float64, torch.int32):
        with pytest.raises(AssertionError, match="unsupported activation dtype"):
            _hip.mcd_reduce_rows(x.to(dtype), torch.zeros(2, 3), "fullmean")
    with pytest.raises(AssertionError, match="row-major float32 matrix"):
        _hip.mcd_reduce_rows(x, torch.zeros(2, 3, dtype=torch.float64), "fullmean")
    for mode, params, d in (("fullmean", None, 3), ("mean", None, 12), ("copy", None, 60), ("avgpool", (3, 2, 1), 18)):
        assert _hip.mcd_row_width(x.shape, mode, params) == d
        with pytest.raises(AssertionError, match="too narrow"):
            _hip.mcd_reduce_rows(x, torch.zeros(2, d - 1), mode, avg_pooling_parameters=params)
    with pytest.raises(AssertionError, match="leave the table"):
        _hip.mcd_reduce_rows(x, torch.zeros(8, 3), "fullmean", row0=4, row_step=4)  # image 1 -> row 8
    with pytest.raises(AssertionError, match="leave the table"):
        _hip.mcd_reduce_rows(x, torch.zeros(8, 3), "fullmean", row0=-1, row_step=4)
    with pytest.raises(AssertionError, match="Three parameters"):
        _hip.mcd_reduce_rows(x, torch.zeros(2, 60), "avgpool", avg_pooling_parameters=(3, 2))
    with pytest.raises(AssertionError, match="mode must be"):
        _hip.mcd_reduce_rows(x, torch.zeros(2, 60), "std")


def test_golden_tables_agree_with_an_f64_reduction_of_their_own_activations():
    g = load_npz("ref_mcd_extractor.npz")
    acts = g["acts"]
    n, mcd, c, h, w = acts.shape
    assert w % 4 != 0 and h != w
    assert [tuple(int(v) for v in r) for r in g["avgpool_settings"]] == AVGPOOL_SETTINGS
    flat = acts.reshape(n * mcd, c, h, w)  # image-major, the reference's row order with one image per batch
    cases = [("ref_fullmean", "fullmean", None), ("ref_mean", "mean", None), ("ref_raw_samples", "fullmean", None),
             ("ref_dep_conv", "fullmean", None), ("ref_dep_deeplab", "fullmean", None)]
    cases += [(f"ref_avgpool_{k}_{s}_{p}", "avgpool", (k, s, p)) for k, s, p in AVGPOOL_SETTINGS]
    for key, mode, params in cases:
        ref = np_reduce(flat, mode, params)
        assert g[key].shape == ref.shape and g[key].dtype == np.float32, key
        assert rel_err(g[key], ref) <= TOL, key
    assert any(g[f"ref_avgpool_{k}_{s}_{p}"].shape[1] > c and (h % s or w % s) for k, s, p in AVGPOOL_SETTINGS)
    fc = g["acts_fc"]
    np.testing.assert_array_equal(g["ref_fc"], fc.reshape(n * mcd, -1))
    dep = g["acts_dep_fc"].astype(np.float64)  # (images, mcd, rows, F): mean over F, one row of `rows` values per pass
    assert rel_err(g["ref_dep_fc"], dep.mean(axis=3).reshape(n * mcd, -1)) <= TOL
    # the raw predictions: (mcd, K) per image, the first two dimensions merged by the reference's extend + cat
    np.testing.assert_array_equal(g["ref_raw_preds"], (g["preds"] * np.float32(g["pred_scale"][0])).reshape(-1))
