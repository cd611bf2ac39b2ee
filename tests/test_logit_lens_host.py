"""The logit lens without a GPU: every refusal comes before the device is touched, the ABI, and the reference itself."""
import ctypes
import types

import numpy as np
import pytest
import torch

import logit_lens_cases as cases
from runia_core_amd import _hip
from runia_core_amd.llm_uncertainty import compute_uncertainties, logit_lens

HS = tuple(torch.randn(2, 6, 8) for _ in range(3))
W = torch.randn(11, 8)
SEQ = torch.zeros((2, 7), dtype=torch.int64)


@pytest.mark.parametrize("args,kw,error", [
    ((HS, W.half(), [1]), dict(input_length=3), TypeError),                                            # mixed dtypes
    ((tuple(h.to(torch.int32) for h in HS), W, [1]), dict(input_length=3), TypeError),                # integer states
    ((HS, W, [1]), dict(input_length=3, attention_mask=torch.tensor([[1] * 6, [0] * 4 + [1] * 2])), ValueError),  # padding
    ((HS, W, [1]), dict(input_length=3, sequences=SEQ[:, :5]), ValueError),                            # sequences too short
    ((HS, W, [1]), dict(), ValueError),                                                                # no window start
])
def test_error_paths_raise_before_the_device(monkeypatch, args, kw, error):
    monkeypatch.setattr(_hip, "require_gpu", lambda: pytest.fail("the device was touched"))
    with pytest.raises(error):
        logit_lens(*args, **kw)


@pytest.mark.parametrize("head,config", [(types.SimpleNamespace(weight=W, bias=torch.zeros(11)), types.SimpleNamespace()),
                                         (types.SimpleNamespace(weight=W), types.SimpleNamespace(final_logit_softcapping=30.0)),
                                         (types.SimpleNamespace(weight=W), types.SimpleNamespace(logit_scale=0.0625))])
def test_pipeline_refuses_heads_the_kernel_does_not_model(head, config):
    model = types.SimpleNamespace(get_output_embeddings=lambda: head, config=config)  # (no tokenizer, no device: refused first)
    with pytest.raises(ValueError, match="logit lens"):
        compute_uncertainties(model, None, "1 2", [{"method_name": "lens_kl"}])


def test_valid_call_without_a_gpu_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.RuniaHipError):
        logit_lens(HS, W, [1], input_length=3, sequences=SEQ)


def test_library_exports_the_header_signatures():
    lib = _hip.load_library()
    res, args = _hip._SIGNATURES["runia_lens_scores"]
    assert res is ctypes.c_int and len(args) == 19 and args[2] is ctypes.c_int64 and args[-1] is ctypes.c_void_p
    assert _hip._SIGNATURES["runia_lens_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64] * 4)
    assert lib.runia_lens_scores.argtypes == args
    big = lib.runia_lens_workspace_bytes(5, 4096, 128256, 4096)
    assert big == lib.runia_lens_workspace_bytes(5, 4096, 1 << 20, 4096) == 64 * 5 * 4096 * 32  # nothing N x V
    assert lib.runia_lens_workspace_bytes(5, 4096, (1 << 24) + 1, 4096) == 0 == lib.runia_lens_workspace_bytes(0, 1, 1, 1)
    assert lib.runia_lens_scores(None, None, 8, 2, 1, 1, 1, 8, None, -1, *([None] * 6), None, 0, None) == _hip._HEADER_MACROS["RUNIA_E_INVALID"]


def test_reference_agrees_with_torch_log_softmax():
    x, w, tok, ref = cases.make(3, 2, 5, 40, 12, final=1)
    logp = torch.log_softmax(x.double() @ w.double().T, -1)
    assert np.allclose(ref["log_prob"], logp[:, torch.arange(5), tok].numpy(), rtol=0, atol=1e-12)
    assert np.allclose(ref["entropy"], -(logp.exp() * logp).sum(-1).numpy(), rtol=0, atol=1e-12)
    kl = (logp[1].exp() * (logp[1] - logp)).sum(-1).numpy()
    assert np.allclose(ref["kl_final"], kl, rtol=0, atol=1e-12) and (ref["top_token"] == logp.argmax(-1).numpy()).all()
