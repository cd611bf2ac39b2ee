"""Per-pixel Mahalanobis maps, the part that needs no GPU: the f64 restatement against scipy / sklearn, the C boundary
(header, binding table, library, Makefile, argument checks before any HIP call) and the refusals of the public functions."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import pixel_feature_cases as cases
from conftest import ROOT
from runia_core_amd import _hip
from runia_core_amd import inference
from runia_core_amd.inference import pixel_features as pf

ENTRIES = ("runia_pixfeat_workspace_bytes", "runia_pixfeat_score", "runia_pixfeat_label_hist",
           "runia_pixfeat_gather_workspace_bytes", "runia_pixfeat_gather_rows")
INVALID, WORKSPACE = -1, -4
P = 4096  # any non-null address: never dereferenced on these paths


def test_restatement_agrees_with_scipy_and_sklearn():
    from scipy.spatial.distance import mahalanobis
    from sklearn.covariance import EmpiricalCovariance

    rng = np.random.default_rng(5)
    k, c, n = 3, 6, 400
    labels = np.arange(n) % k
    means = 3.0 + rng.standard_normal((k, c))
    rows = means[labels] + rng.standard_normal((n, c)) @ rng.standard_normal((c, c))
    fit = cases.fit_restatement(rows, labels, k)
    centred = rows - fit["means"][labels]
    ec = EmpiricalCovariance(assume_centered=True).fit(centred)
    assert np.allclose(fit["cov"], ec.covariance_, rtol=1e-12, atol=1e-12)
    assert np.allclose(fit["W"] @ fit["chol"], np.eye(c), atol=1e-10)
    x = 3.0 + rng.standard_normal((2, c, 3, 4))
    d = cases.f64_distances(x, fit)
    vi = np.linalg.inv(fit["cov"])
    for g, hh, ww, cl in ((0, 0, 0, 0), (1, 2, 3, 2), (0, 1, 2, 1)):
        want = mahalanobis(x[g, :, hh, ww], fit["means"][cl], vi) ** 2
        assert abs(d[g, cl, hh, ww] - want) <= 1e-9 * want
    rows_x = x.transpose(0, 2, 3, 1).reshape(-1, c)
    for cl in range(k):
        want = ec.mahalanobis(rows_x - fit["means"][cl])  # squared distances
        assert np.allclose(d[:, cl].reshape(-1), want, rtol=1e-9)


def test_yardstick_is_close_to_f64_and_the_expanded_form_is_not():
    """Why the kernel's epilogue is the difference form: with the means at +3 the expanded form loses the result in f32."""
    case = cases.make_case(96, 19, 1, 31, 67, 1e6)
    d64 = case["d64"]
    err = np.max(np.abs(case["yard"] - d64) / np.maximum(1.0, d64))
    assert err < 1e-2
    fit = case["fit"]
    x = torch.from_numpy(case["features"]).permute(0, 2, 3, 1).reshape(-1, 96)
    w32, m0 = torch.from_numpy(fit["W"].astype(np.float32)), torch.from_numpy(fit["m0"].astype(np.float32))
    mz = torch.from_numpy(fit["mz"].astype(np.float32))
    z = (x - m0) @ w32.T
    expanded = (z * z).sum(1, keepdim=True) - 2.0 * z @ mz.T + (mz * mz).sum(1)[None]
    diff = ((z[:, None] - mz[None]) ** 2).sum(-1)
    ref = torch.from_numpy(d64).permute(0, 2, 3, 1).reshape(-1, 19)
    e_exp = float(((expanded.double() - ref).abs() / ref.clamp(min=1.0)).max())
    e_diff = float(((diff.double() - ref).abs() / ref.clamp(min=1.0)).max())
    assert e_diff <= e_exp


def test_cases_store_half_values_exactly_and_are_shared():
    for dt in ("f16", "bf16"):
        case = cases.make_case(33, 21, 3, 3, 43, 1e2, dt)
        t = torch.from_numpy(case["features"])
        assert torch.equal(t.to(cases.TORCH_DT[dt]).float(), t)
        assert cases.make_case(33, 21, 3, 3, 43, 1e2, dt) is case
        assert (case["labels"] == cases.IGNORE).any()


def test_header_binding_library_and_makefile_list_the_entries():
    header = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load_library()
    for name in ENTRIES:
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl, f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols() and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_hip._SIGNATURES[name][1]), name
    assert {s for s in _hip.exported_symbols() if s.startswith("runia_pixfeat_")} == set(ENTRIES)
    makefile = open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpixel_features\.hip\b", makefile, flags=re.M)
    assert lib.runia_abi_version() == 6  # additive entries


def test_workspace_query_knows_nothing_of_the_pixels():
    lib = _hip.load_library()
    assert _hip._SIGNATURES["runia_pixfeat_workspace_bytes"][1] == [_hip.c_int64, _hip.c_int64]  # (C, K): no G, h, w
    sizes = {(c, k): int(lib.runia_pixfeat_workspace_bytes(c, k)) for c in (1, 256, 1024) for k in (1, 19, 256)}
    assert all(v >= 0 and v < 1 << 30 for v in sizes.values())
    assert int(lib.runia_pixfeat_gather_workspace_bytes(0)) == 0
    assert int(lib.runia_pixfeat_gather_workspace_bytes(1)) == 8
    assert int(lib.runia_pixfeat_gather_workspace_bytes(1024)) == 8
    assert int(lib.runia_pixfeat_gather_workspace_bytes(1025)) == 16


def _score(lib, features=P, dtype=0, G=2, C=19, H=4, W=8, sn=608, sc=32, sh=8, sw=1, m0=P, Wm=P, mz=P, K=5, dist=P,
           nearest=None, cd=None):
    return lib.runia_pixfeat_score(features, dtype, G, C, H, W, sn, sc, sh, sw, m0, Wm, mz, K, dist, nearest, cd, None, 0, None)


def test_score_argument_checks_come_before_any_hip_call():
    lib = _hip.load_library()
    assert _score(lib, C=1025) == INVALID and _score(lib, C=0) == INVALID
    assert _score(lib, K=257) == INVALID and _score(lib, K=0) == INVALID
    assert _score(lib, dtype=3) == INVALID and _score(lib, dtype=-1) == INVALID
    assert _score(lib, G=-1) == INVALID and _score(lib, H=-1) == INVALID and _score(lib, sw=-1) == INVALID
    assert _score(lib, G=1 << 31) == INVALID
    assert _score(lib, G=1 << 20, H=1 << 10, W=1 << 10) == INVALID           # 2^40 pixels
    assert _score(lib, G=0) == 0 and _score(lib, H=0) == 0 and _score(lib, W=0) == 0  # nothing to do: no launch
    assert _score(lib, G=0, features=None, dist=None) == 0
    assert _score(lib, features=None) == INVALID and _score(lib, m0=None) == INVALID
    assert _score(lib, Wm=None) == INVALID and _score(lib, mz=None) == INVALID
    assert _score(lib, dist=None) == INVALID                                 # no output asked for
    assert _score(lib, C=1025, G=0) == INVALID                               # the limits come first


def test_hist_and_gather_argument_checks_come_before_any_hip_call():
    lib = _hip.load_library()
    hist = lib.runia_pixfeat_label_hist
    assert hist(P, 0, 10, 257, 255, P, P, None) == INVALID and hist(P, 0, 10, 0, 255, P, P, None) == INVALID
    assert hist(P, 3, 10, 5, 255, P, P, None) == INVALID and hist(P, 0, -1, 5, 255, P, P, None) == INVALID
    assert hist(P, 0, 10, 5, 255, None, P, None) == INVALID and hist(None, 0, 10, 5, 255, P, P, None) == INVALID

    def gather(features=P, dtype=0, G=2, C=19, H=4, W=8, labels=P, ldt=0, K=5, keep=P, off=0, rows=None, rl=None, cap=0,
               n_out=P, ws=P, ws_bytes=8):
        return lib.runia_pixfeat_gather_rows(features, dtype, G, C, H, W, 608, 32, 8, 1, labels, ldt, K, 255, keep, 7, off,
                                             rows, rl, cap, n_out, ws, ws_bytes, None)

    assert gather(C=1025) == INVALID and gather(K=257) == INVALID and gather(dtype=5) == INVALID and gather(ldt=3) == INVALID
    assert gather(off=-1) == INVALID and gather(n_out=None) == INVALID and gather(keep=None) == INVALID
    assert gather(rows=P) == INVALID and gather(rl=P) == INVALID             # both or neither
    assert gather(features=None) == INVALID and gather(labels=None) == INVALID
    assert gather(ws=None) == WORKSPACE and gather(ws_bytes=0) == WORKSPACE and gather(ws=P + 4) == WORKSPACE


def test_exports_and_refusals_of_the_public_functions():
    for name in ("PixelMahalanobis", "pixel_feature_rows", "get_pixel_mahalanobis_maps", "fit_pixel_mahalanobis"):
        assert name in pf.__all__ and getattr(inference, name) is getattr(pf, name)
    with pytest.raises(ValueError):
        pf.PixelMahalanobis(0)
    with pytest.raises(ValueError):
        pf.PixelMahalanobis(257)
    with pytest.raises(ValueError):
        pf.PixelMahalanobis(3, rows_per_class_per_batch=0)
    with pytest.raises(ValueError):
        pf.PixelMahalanobis(3, ridge=-1.0)
    det = pf.PixelMahalanobis(3)
    x = torch.zeros(1, 4, 2, 2)
    with pytest.raises(ValueError, match="not fitted"):
        det.score_maps(x)
    with pytest.raises(ValueError, match="unknown output"):
        det.score_maps(x, outputs=("distance", "z"))
    with pytest.raises(ValueError):
        det.partial_fit(x, torch.zeros(1, 3, 2, dtype=torch.int64))          # labels at another resolution
    with pytest.raises(ValueError):
        det.partial_fit(x.double(), torch.zeros(1, 2, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        det.partial_fit(x, torch.zeros(1, 2, 2, dtype=torch.float32))
    with pytest.raises(ValueError):
        det.finalize()
    with pytest.raises(ValueError):
        pf.pixel_feature_rows(x, torch.zeros(1, 2, 2, dtype=torch.int64), [0.5, 1.5])
    with pytest.raises(ValueError):
        pf.fit_pixel_mahalanobis(torch.nn.Identity(), [], torch.nn.Identity(), 3, label_stride=0)


def test_a_fitted_state_is_host_arrays_and_pickles_without_its_device_cache():
    det = pf.PixelMahalanobis(2)
    fit = cases.fit_restatement(np.random.default_rng(0).standard_normal((50, 3)), np.arange(50) % 2, 2)
    det.n_channels_, det.center_, det.whitening_, det.class_offsets_ = 3, fit["m0"], fit["W"], fit["mz"]
    det._dev = ("placeholder of the device copies",)
    back = pickle.loads(pickle.dumps(det))
    assert back._dev is None and det._dev is not None
    assert np.array_equal(back.whitening_, det.whitening_) and back.whitening_.dtype == np.float64
    assert not any(isinstance(v, torch.Tensor) for v in back.__dict__.values())
