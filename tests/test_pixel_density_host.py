"""Per-pixel class-Gaussian densities, the part that needs no GPU: the C boundary (header, binding table, library, argument
checks before any HIP call), the refusals of the public functions and the pickle of a detector set from arrays."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from runia_core_amd import _hip
from runia_core_amd.inference import PixelGaussianDensity, PixelMahalanobis, fit_pixel_density, get_pixel_density_maps

ENTRIES = ("runia_pixdens_tile_pixels", "runia_pixdens_workspace_bytes", "runia_pixdens_score")
INVALID, P = -1, 4096  # P: any non-null address, never dereferenced on these paths


def test_header_binding_and_library_list_the_entries():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    lib = _hip.load_library()
    for name in ENTRIES:
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl, f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols() and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_hip._SIGNATURES[name][1]), name
    assert {s for s in _hip.exported_symbols() if s.startswith("runia_pixdens_")} == set(ENTRIES)
    assert [_hip.pixdens_tile_pixels(c) for c in (0, 1, 256, 257, 512, 513, 1024, 1025)] == [0, 128, 128, 64, 64, 32, 32, 0]


def _score(lib, features=P, dtype=0, G=2, C=19, H=4, W=8, sn=608, sc=32, sh=8, sw=1, means=P, wt=P, consts=P, K=5, ld=P):
    return lib.runia_pixdens_score(features, dtype, G, C, H, W, sn, sc, sh, sw, means, wt, consts, K, ld, None, None, None, 0, None)


def test_score_argument_checks_come_before_any_hip_call():
    lib = _hip.load_library()
    assert all(_score(lib, **kw) == INVALID for kw in ({"C": 1025}, {"C": 0}, {"K": 257}, {"K": 0}))
    assert _score(lib, dtype=3) == INVALID and _score(lib, G=-1) == INVALID and _score(lib, sw=-1) == INVALID
    assert _score(lib, G=0) == 0 and _score(lib, H=0) == 0 and _score(lib, W=0) == 0  # nothing to do: no launch
    assert all(_score(lib, **{name: None}) == INVALID for name in ("features", "means", "wt", "consts", "ld"))  # ld: no output
    assert _score(lib, C=1025, G=0) == INVALID                                        # the limits come first


@pytest.mark.parametrize("call, message", [
    (lambda: PixelGaussianDensity(0), "n_classes must be an integer in 1 .. 256"),
    (lambda: PixelGaussianDensity(3, weights="prior"), "weights must be one of"),
    (lambda: PixelGaussianDensity(3).finalize(), "before any labelled pixel was seen"),
    (lambda: PixelGaussianDensity(3).score_maps(torch.zeros(1, 4, 2, 2)), "not fitted"),
    (lambda: PixelGaussianDensity(3).score_maps(torch.zeros(1, 4, 2, 2), "distance"), "unknown output 'distance'"),
    (lambda: _hip.pixdens_score(torch.zeros(1, 4, 2, 2), torch.zeros(3, 4), torch.zeros(3, 4, 5), torch.zeros(3)), "w_tril must be"),
    (lambda: PixelGaussianDensity(3).partial_fit(torch.zeros(1, 1025, 2, 2), torch.zeros(1, 2, 2).long()), "1025 channels"),
    (lambda: fit_pixel_density(torch.nn.Identity(), [], torch.nn.Identity(), 3, label_stride=0), "label_stride"),
    (lambda: get_pixel_density_maps(torch.nn.Identity(), [], torch.nn.Identity(), None, ()), "nothing requested"),
])
def test_refusals_name_the_argument(call, message):
    with pytest.raises((ValueError, AssertionError), match=message):
        call()


def test_pickle_drops_the_device_cache_and_mahalanobis_keeps_its_state_names():
    det = PixelGaussianDensity(2, weights="empirical")
    det.n_channels_, det.class_means_, det.whitenings_ = 3, np.arange(6.0).reshape(2, 3), np.tril(np.ones((2, 3, 3)))
    det.covariances_, det.log_norms_, det.log_weights_ = np.zeros((2, 3, 3)), np.array([-1.0, -2.0]), np.log([0.25, 0.75])
    det._dev = ("cuda:0", "stale")
    twin = pickle.loads(pickle.dumps(det))
    assert twin._dev is None and det._dev is not None and twin.weights == "empirical" and twin.ridge == 1e-6
    assert all(np.array_equal(getattr(twin, n), getattr(det, n)) for n in det._fitted_attrs)
    assert {"class_means_", "covariance_", "center_", "whitening_", "class_offsets_", "_dev"} <= set(PixelMahalanobis(3).__getstate__())
