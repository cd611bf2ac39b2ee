"""Embedding consistency without a GPU: every refusal comes before the device is touched, the request keys, the ABI, and the
restatement itself against a brute-force double loop."""
import numpy as np
import pytest
import torch

import embed_consistency_cases as cases
from runia_core_amd import _hip
from runia_core_amd.llm_uncertainty import embedding_similarity
from runia_core_amd.llm_uncertainty.pipeline import _score_name

HS = tuple(torch.randn(6, 9, 8) for _ in range(3))
LONG = (torch.zeros(2, 1030, 4),)


@pytest.mark.parametrize("args,kw,error", [
    ((tuple(h[:, :, None] for h in HS), 3, 1), dict(), ValueError),                                   # 4-d states
    ((tuple(h.to(torch.int32) for h in HS), 3, 1), dict(), TypeError),                                # integer states
    ((tuple(h.double() for h in HS), 3, 1), dict(), TypeError),                                       # f64 states
    ((HS, 1, 1), dict(), ValueError),                                                                 # one sample per group
    ((HS, 65, 1), dict(), ValueError),                                                                # beyond RUNIA_CONS_MAX_K
    ((HS, 4, 1), dict(), ValueError),                                                                 # 6 rows, groups of 4
    ((HS, 3, 1), dict(windows=[[1, 4]] * 6, attention_mask=torch.tensor([[0, 0] + [1] * 7] * 6)), ValueError),  # padding
    ((HS, 3, 1), dict(windows=[[5, 5]] * 6), ValueError),                                             # leaves the positions
    ((LONG, 2, 0), dict(), ValueError),                                                               # n > 1024
])
def test_error_paths_raise_before_the_device(monkeypatch, args, kw, error):
    monkeypatch.setattr(_hip, "require_gpu", lambda: pytest.fail("the device was touched"))
    with pytest.raises(error):
        embedding_similarity(*args, **kw)


def test_valid_call_without_a_gpu_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.RuniaHipError):
        embedding_similarity(HS, 3, 1)


@pytest.mark.parametrize("req,key", [({"similarity": "embedding"}, "deg_embedding"),
                                     ({"similarity": "embedding", "layer": 15}, "deg_embedding"),
                                     ({"similarity": "embedding", "layer": 3}, "deg_embedding_3"),
                                     ({"similarity": "jaccard", "layer": 3}, "deg_jaccard"), ({}, "deg")])
def test_request_keys(req, key):
    assert _score_name({"method_name": "deg", **req}) == key


def test_entry_point_refusal_and_size_query():
    lib = _hip.load_library()
    assert lib.runia_cons_embed(None, None, None, 2, 1, 2, 1, 1, 8, 1, None, None, 0, None) == _hip._HEADER_MACROS["RUNIA_E_INVALID"] == -1
    size = lib.runia_cons_embed_workspace_bytes
    for bad in ((0, 2, 1, 1), (-1, 2, 1, 1), (1, 1, 1, 1), (1, 65, 1, 1), (1, 2, -1, 1), (1, 2, 1025, 1), (1, 2, 1, 0)):
        assert size(*bad) == 0, bad
    # means (d to 32) + flag + inverse norms per row + 8 bytes per pair and token slot (T to 128): nothing T x T or N x d
    assert size(64, 10, 256, 4096) == 64 * (4096 * 4 + 4 + 10 * 256 * 4 + 55 * 256 * 8)
    assert size(1, 2, 0, 1) == size(1, 2, 128, 32) == 32 * 4 + 16 + 2 * 128 * 4 + 3 * 128 * 8


def test_restatement_equals_a_double_loop():
    x, windows = cases.make(1, 2, 3, 5, 7, "f32")
    ref = cases.reference(x, windows, 3, "f32")
    xs = x.double().numpy()
    for g in range(2):
        rows = [xs[r, s:s + n] for r, (s, n) in list(enumerate(windows))[3 * g:3 * g + 3]]
        m = np.concatenate(rows).mean(0)
        for i, a in enumerate(rows):
            for j, b in enumerate(rows):
                if len(a) == 0 or len(b) == 0:
                    want = float(len(a) == len(b))
                else:
                    want = np.mean([max(np.dot(u - m, v - m) / np.linalg.norm(u - m) / np.linalg.norm(v - m) for v in b) for u in a])
                assert abs(ref["coverage"][g, i, j] - want) <= 1e-12
    w, c = ref["similarity"], np.maximum(ref["coverage"], 0)
    assert np.allclose(w, w.transpose(0, 2, 1)) and (np.diagonal(w, axis1=1, axis2=2) == 1).all()
    assert abs(w[0, 0, 1] - 2 * c[0, 0, 1] * c[0, 1, 0] / (c[0, 0, 1] + c[0, 1, 0])) <= 1e-15 and w[0, 0, 2] == 0 == w[0, 2, 1]
