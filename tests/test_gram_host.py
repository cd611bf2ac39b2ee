"""The Gram detector without a GPU: refusals, the pickle of a detector whose state is set from arrays, and the float64
restatement of tests/gram_cases.py against the published matmul recipe."""
import pickle

import numpy as np
import pytest
import torch

import gram_cases as cases
from runia_core_amd import _hip
from runia_core_amd.inference import GramDetector, fit_gram_detector, gram_statistics


def test_restatement_equals_the_matmul_recipe():
    f = cases.make_map((2, 5, 3, 4), "signed", seed=7).astype(np.float64)
    t, a, v = cases.statistics(f, 6)
    assert np.abs(v - cases.matmul_recipe(f, 6)).max() <= 1e-12 and (a >= np.abs(t)).all()
    bound, ok = cases.bound_v(f.astype(np.float32), 6)
    assert bound.shape == v.shape and (bound[ok] >= 0).all()
    lo, hi = (v.min(axis=0, keepdims=True) + 0.01).astype(np.float32), (v.max(axis=0, keepdims=True) - 0.01).astype(np.float32)
    dev = cases.deviation(v, np.concatenate([lo, np.full_like(lo, np.inf)]), np.concatenate([hi, np.full_like(hi, -np.inf)]),
                          np.array([0, 1]))
    assert dev[0] > 0 and np.isposinf(dev[1])


@pytest.mark.parametrize("call, message", [
    (lambda: gram_statistics(torch.zeros(2, 3, 4)), r"\(B, C, H, W\) or \(B, F\)"),
    (lambda: gram_statistics(torch.zeros(2, 3, dtype=torch.float64)), "unsupported fmap dtype"),
    (lambda: gram_statistics(torch.zeros(2, 3), powers=17), r"powers must be an integer in 1 \.\. 16"),
    (lambda: gram_statistics(torch.zeros(2, 3), powers=0), r"powers must be an integer in 1 \.\. 16"),
    (lambda: GramDetector(0), "n_classes must be a positive integer"),
    (lambda: GramDetector(3).fit_batch(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)), "non-empty sequence of tensors"),
    (lambda: GramDetector(3).fit_batch([torch.zeros(2, 3)], torch.zeros(2)), r"labels must be an int32 or int64 tensor of shape \(2,\)"),
    (lambda: GramDetector(3).fit_batch([torch.zeros(2, 3), torch.zeros(3, 3)], torch.zeros(2, dtype=torch.int64)),
     "different batch sizes"),
    (lambda: GramDetector(3).score([torch.zeros(2, 3)], torch.zeros(2, dtype=torch.int64)), "not calibrated"),
    (lambda: fit_gram_detector(torch.nn.Identity(), [], [], [], 3), "hooked_layers must be a non-empty sequence"),
])
def test_refusals_name_the_argument(call, message):
    with pytest.raises(ValueError, match=message):
        call()


def test_wrapper_refusals_and_the_abi():
    assert _hip.GRAM_MAX_POWERS == 16 and {"runia_gram_layer", "runia_gram_workspace_bytes"} <= set(_hip.exported_symbols())
    x = torch.zeros(2, 3)
    for call, message in ((lambda: _hip.gram_layer_stats(x.double()), "unsupported activation dtype"),
                          (lambda: _hip.gram_layer_stats(x[0]), r"\(B, F\) or \(B, C, H, W\)"),
                          (lambda: _hip.gram_layer_stats(x), "must be a device tensor"),
                          (lambda: _hip.gram_layer_deviation(x, torch.zeros(2), torch.zeros(1, 10, 3), torch.zeros(1, 10, 3)),
                           "labels must be an int32 or int64"),
                          (lambda: _hip.gram_layer_deviation(x, torch.zeros(2, dtype=torch.int32), torch.zeros(1, 10, 4),
                                                             torch.zeros(1, 10, 4)), r"table of shape \(K, 10, 3\)")):
        with pytest.raises(AssertionError, match=message):
            call()
    # host queries: the tile width and the staged channels follow from C and the element type alone
    assert _hip.gram_tile_width(65) in (8, 16, 32) and _hip.gram_chunk_channels(65, torch.bfloat16) == 65
    vals = torch.tensor([float("-inf"), -2.5, -0.0, 0.0, 1.5, float("inf")])
    k = _hip.gram_values_to_keys(vals)
    assert torch.equal(_hip.gram_keys_to_values(k).view(torch.int32), vals.view(torch.int32))
    assert (np.diff(k.numpy().astype(np.int64) & 0xffffffff) > 0).all()   # the unsigned order of the keys is the floats' order


def test_pickle_round_trip_of_a_detector_set_from_arrays():
    det = GramDetector(2, 3)
    rng = np.random.default_rng(0)
    det.mins_ = [rng.standard_normal((2, 3, 5)), rng.standard_normal((2, 3, 7))]
    det.maxs_ = [m + 1 for m in det.mins_]
    det.dev_sum_, det.dev_count_ = np.array([2.0, 6.0]), 4
    twin = pickle.loads(pickle.dumps(det))
    assert twin.n_classes == 2 and twin.powers == 3 and twin.dev_count_ == 4
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(twin.mins_ + twin.maxs_, det.mins_ + det.maxs_))
    assert np.array_equal(twin.mean_deviations_, [0.5, 1.5])
    with pytest.raises(ValueError, match=r"one \(2, 3, C\) array per layer"):
        det.mins_ = [np.zeros((2, 4, 5))]
