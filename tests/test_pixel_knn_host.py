"""Per-pixel kNN maps and the k-center coreset, the part that needs no GPU: the restatements against scipy and a direct loop,
the C boundary (header, binding table, library, Makefile, argument checks before any HIP call) and the refusals of the public
functions."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import pixel_knn_cases as cases
from conftest import ROOT
from runia_core_amd import _hip
from runia_core_amd import inference
from runia_core_amd.inference import pixel_knn as pk

ENTRIES = {"runia_pixknn_": ("runia_pixknn_workspace_bytes", "runia_pixknn_score"),
           "runia_kcenter_": ("runia_kcenter_workspace_bytes", "runia_kcenter_greedy_f32")}
INVALID, WORKSPACE = -1, -4
P = 4096  # any non-null address: never dereferenced on these paths


def test_restatement_agrees_with_scipy_and_a_stable_argsort():
    from scipy.spatial.distance import cdist

    rng = np.random.default_rng(3)
    x, b = 3.0 + rng.standard_normal((50, 7)), 3.0 + rng.standard_normal((90, 7))
    b[40:45] = b[10:15]                                                     # ties
    dist, idx, full = cases.knn_restatement(x, b, 6)
    want = cdist(x, b, "sqeuclidean")
    assert np.allclose(full, want, rtol=1e-12, atol=1e-12)
    assert np.array_equal(idx, np.argsort(full, axis=1, kind="stable")[:, :6])
    assert np.array_equal(dist, np.take_along_axis(full, idx, axis=1)) and (np.diff(dist, axis=1) >= 0).all()
    tied = np.diff(dist, axis=1) == 0
    assert tied.any() and (np.diff(idx, axis=1)[tied] > 0).all()            # the lower index first
    g, c, h, w = 2, 7, 3, 4
    maps = rng.standard_normal((g, c, h, w))
    rows = cases.pixel_rows(maps)
    assert np.array_equal(rows[1 * 12 + 2 * 4 + 3], maps[1, :, 2, 3])
    assert np.array_equal(cases.as_maps(rows, g, h, w), maps)


def test_kcenter_restatement_agrees_with_a_direct_loop():
    for rows in (cases.kcenter_int_table(257, 33), cases.kcenter_int_table(40, 1), cases.kcenter_float_table()[0][:90]):
        n = rows.shape[0]
        picked, radius, _ = cases.kcenter_restatement(rows, 25, 3)
        x = rows.astype(np.float64)
        mine, rad = [3], [np.inf]
        while len(mine) < 25:
            best, arg = -1.0, -1
            for i in range(n):
                near = min(float(((x[i] - x[j]) ** 2).sum()) for j in mine)
                if near > best:                                             # strictly: the lowest index on ties
                    best, arg = near, i
            if best <= 0.0:
                break
            mine.append(arg)
            rad.append(best)
        assert picked.tolist() == mine and np.allclose(radius, rad, rtol=1e-12)
        assert (np.diff(radius[1:]) <= 0).all()
    picked, _, _ = cases.kcenter_restatement(cases.kcenter_int_table(40, 1), 40, 0)
    assert len(picked) == len(np.unique(cases.kcenter_int_table(40, 1))) < 40  # ends when only duplicates are left


def test_exact_cases_are_exact_in_every_dtype_and_shared():
    for dt in ("f16", "bf16"):
        case = cases.exact_case(33, 129, 1, 3, 3, 43, dt)
        t = torch.from_numpy(case["features"])
        assert torch.equal(t.to(cases.TORCH_DT[dt]).float(), t)
        assert cases.exact_case(33, 129, 1, 3, 3, 43, dt) is case
    case = cases.tie_case()
    d, i = case["distances"], case["indices"]
    tied = np.diff(d, axis=1) == 0
    assert tied.mean() >= 0.4 and (np.diff(i, axis=1)[tied] > 0).all()       # every row twice: the lower index first
    assert (i[:, 1] == i[:, 0] + 150).mean() > 0.9                           # (the twin of the nearest row comes second)
    for kind in cases.PLACEMENTS:
        cases.placement_case(kind)
    cases.monotone_case(True), cases.monotone_case(False)
    c32, b32, bsq = cases.kernel_operands(case["bank"], case["center"])
    assert np.array_equal(b32, (case["bank"] - case["center"]).astype(np.float32))
    assert np.array_equal(bsq, (b32.astype(np.float64) ** 2).sum(1).astype(np.float32)) and c32.dtype == np.float32


def test_float_yardstick_is_the_uncentred_expanded_form_and_the_margin_of_the_kcenter_table_holds():
    case = cases.float_case(40, 300, 8, 3, 6, 22, 3.0)
    err = np.max(np.abs(case["yard"] - case["d64"]) / np.maximum(1.0, case["d64"]))
    assert 0 < err < 1e-4
    assert np.array_equal(case["d64"], np.sort(case["all64"], axis=1)[:, :8])
    rows, picked, radius = cases.kcenter_float_table()
    assert rows.shape == (700, 48) and len(picked) == 32 and len(set(picked.tolist())) == 32


def test_header_binding_library_and_makefile_list_the_entries():
    header = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load_library()
    for prefix, names in ENTRIES.items():
        for name in names:
            decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
            assert decl, f"{name} is not declared in include/runia_hip.h"
            assert name in _hip.exported_symbols() and hasattr(lib, name)
            assert len(decl.group(1).split(",")) == len(_hip._SIGNATURES[name][1]), name
        assert {s for s in _hip.exported_symbols() if s.startswith(prefix)} == set(names)
    for name in ("runia_pixknn_score", "runia_kcenter_greedy_f32"):
        assert _hip._SIGNATURES[name][1][-1] is _hip.c_void_p and "runia_stream_t stream" in re.search(
            rf"\b{name}\s*\(([^)]*)\)", code).group(1).split(",")[-1]
    makefile = open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpixel_knn\.hip\b", makefile, flags=re.M)
    assert lib.runia_abi_version() == 6  # additive entries


def test_workspace_queries():
    lib = _hip.load_library()
    assert _hip._SIGNATURES["runia_pixknn_workspace_bytes"][1] == [_hip.c_int64] * 3     # (C, M, k): no G, h, w
    assert all(0 <= int(lib.runia_pixknn_workspace_bytes(c, m, k)) < 1 << 30
               for c in (1, 256, 1024) for m in (16, 1 << 22) for k in (1, 16))
    small, large = int(lib.runia_kcenter_workspace_bytes(1, 1)), int(lib.runia_kcenter_workspace_bytes(65536, 256))
    assert 0 < small < large and large >= 65536 * 4
    assert int(lib.runia_kcenter_workspace_bytes(0, 4)) == 0 and int(lib.runia_kcenter_workspace_bytes(4, 1025)) == 0


def _score(lib, features=P, dtype=0, G=2, C=19, H=4, W=8, sn=608, sc=32, sh=8, sw=1, center=P, bank=P, bank_sq=P, M=50, k=3,
           dist=P, idx=None, kth=None, mean=None):
    return lib.runia_pixknn_score(features, dtype, G, C, H, W, sn, sc, sh, sw, center, bank, bank_sq, M, k, dist, idx, kth,
                                  mean, None, 0, None)


def test_score_argument_checks_come_before_any_hip_call():
    lib = _hip.load_library()
    assert _score(lib, C=1025) == INVALID and _score(lib, C=0) == INVALID
    assert _score(lib, k=17) == INVALID and _score(lib, k=0) == INVALID
    assert _score(lib, M=2) == INVALID and _score(lib, M=(1 << 22) + 1) == INVALID    # k <= M <= 2^22
    assert _score(lib, dtype=3) == INVALID and _score(lib, dtype=-1) == INVALID
    assert _score(lib, G=-1) == INVALID and _score(lib, H=-1) == INVALID and _score(lib, sw=-1) == INVALID
    assert _score(lib, G=1 << 31) == INVALID
    assert _score(lib, G=1 << 11, H=1 << 10, W=1 << 10) == INVALID                    # 2^31 pixels
    assert _score(lib, G=0) == 0 and _score(lib, H=0) == 0 and _score(lib, W=0) == 0  # nothing to do: no launch
    assert _score(lib, G=0, features=None, dist=None) == 0
    assert _score(lib, features=None) == INVALID and _score(lib, center=None) == INVALID
    assert _score(lib, bank=None) == INVALID and _score(lib, bank_sq=None) == INVALID
    assert _score(lib, dist=None) == INVALID                                          # no output asked for
    for limit in (dict(C=1025), dict(k=17), dict(M=2), dict(M=(1 << 22) + 1), dict(dtype=3)):
        assert _score(lib, G=0, **limit) == INVALID                                   # the limits come first


def test_kcenter_argument_checks_come_before_any_hip_call():
    lib = _hip.load_library()

    def greedy(rows=P, N=100, D=8, first=0, n_pick=10, picked=P, radius=P, n_picked=P, ws=P, ws_bytes=1 << 30):
        return lib.runia_kcenter_greedy_f32(rows, N, D, first, n_pick, picked, radius, n_picked, ws, ws_bytes, None)

    assert greedy(N=0) == INVALID and greedy(N=1 << 31) == INVALID
    assert greedy(D=0) == INVALID and greedy(D=1025) == INVALID
    assert greedy(first=-1) == INVALID and greedy(first=100) == INVALID
    assert greedy(n_pick=0) == INVALID
    assert greedy(rows=None) == INVALID and greedy(picked=None) == INVALID
    assert greedy(radius=None) == INVALID and greedy(n_picked=None) == INVALID
    need = int(lib.runia_kcenter_workspace_bytes(100, 8))
    assert greedy(ws=None) == WORKSPACE and greedy(ws_bytes=need - 1) == WORKSPACE and greedy(ws=P + 4) == WORKSPACE
    assert greedy(ws=None, N=0) == INVALID                                            # the limits come first


def test_exports_and_refusals_of_the_public_functions():
    for name in ("PixelKNN", "kcenter_greedy", "get_pixel_knn_maps", "fit_pixel_knn"):
        assert name in pk.__all__ and getattr(inference, name) is getattr(pk, name)
    assert "PIXEL_KNN_OUTPUTS" in pk.__all__
    assert pk.PIXEL_KNN_OUTPUTS == ("kth_distance", "mean_distance", "distances", "indices")
    for bad in (dict(k=0), dict(k=17), dict(bank_size=0), dict(rows_per_batch=0), dict(selection="furthest"),
                dict(center=[[1.0, 2.0]]), dict(center=[float("nan")])):
        with pytest.raises(ValueError):
            pk.PixelKNN(**bad)
    det = pk.PixelKNN()
    assert (det.k, det.bank_size, det.rows_per_batch, det.selection, det.center, det.ignore_index, det.seed) == \
        (3, 8192, 16384, "kcenter", "mean", 255, 0)
    x = torch.zeros(1, 4, 2, 2)
    with pytest.raises(ValueError, match="not fitted"):
        det.score_maps(x)
    with pytest.raises(ValueError, match="unknown output"):
        det.score_maps(x, outputs=("kth_distance", "distance"))
    with pytest.raises(ValueError, match="named twice"):
        det.score_maps(x, outputs=("indices", "indices"))
    with pytest.raises(ValueError, match="empty"):
        det.score_maps(x, outputs=())
    with pytest.raises(ValueError):
        det.partial_fit(x, torch.zeros(1, 3, 2, dtype=torch.int64))          # labels at another resolution
    with pytest.raises(ValueError):
        det.partial_fit(x.double())
    with pytest.raises(ValueError):
        det.partial_fit(x[0])
    with pytest.raises(ValueError):
        det.partial_fit(x, torch.zeros(1, 2, 2, dtype=torch.float32))
    with pytest.raises(ValueError):
        det.finalize()
    det._rows = [np.zeros((2, 4), dtype=np.float32)]                          # two candidates, k = 3
    with pytest.raises(ValueError, match="k = 3"):
        det.finalize()
    fitted = _fitted()
    with pytest.raises(ValueError, match="channels"):
        fitted.score_maps(torch.zeros(1, 4, 2, 2))
    with pytest.raises(ValueError):
        fitted.score_maps(torch.zeros(1, 3, 2, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        pk.kcenter_greedy(np.zeros((4, 3)), 2)                               # f64
    with pytest.raises(ValueError):
        pk.kcenter_greedy(np.zeros((4, 3), dtype=np.float32), 0)
    with pytest.raises(ValueError):
        pk.kcenter_greedy(np.zeros((4, 3), dtype=np.float32), 2, first=4)
    with pytest.raises(ValueError):
        pk.kcenter_greedy(np.zeros((4, 1025), dtype=np.float32), 2)
    with pytest.raises(ValueError):
        pk.fit_pixel_knn(torch.nn.Identity(), [], torch.nn.Identity(), label_stride=0)
    with pytest.raises(ValueError):
        pk.get_pixel_knn_maps(torch.nn.Identity(), [], torch.nn.Identity(), fitted, outputs=("nearest",))


def _fitted():
    det = pk.PixelKNN(k=2)
    rng = np.random.default_rng(0)
    det.n_channels_, det.bank_, det.center_ = 3, rng.standard_normal((5, 3)), rng.standard_normal(3)
    det.bank_rows_, det.coverage_radius_ = np.arange(5), 1.0
    return det


def test_a_fitted_state_is_host_arrays_and_pickles_without_its_device_cache():
    det = _fitted()
    det._rows = [np.zeros((5, 3), dtype=np.float32)]
    det._dev = ("placeholder of the device copies",)
    back = pickle.loads(pickle.dumps(det))
    assert back._dev is None and det._dev is not None
    assert np.array_equal(back.bank_, det.bank_) and back.bank_.dtype == np.float64
    assert np.array_equal(back.center_, det.center_) and np.array_equal(back.bank_rows_, det.bank_rows_)

    def tensors(v):
        if isinstance(v, torch.Tensor):
            return True
        return isinstance(v, (list, tuple)) and any(tensors(i) for i in v)

    assert not any(tensors(v) for v in back.__dict__.values())
