"""Per-pixel uncertainty maps, the part that needs no GPU: the fixture, the C boundary (header, binding table, Makefile,
argument checks before any launch), the refusals of the public functions and their export."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_npz
from runia_core_amd import _hip

CASE_KEYS = ("logits", "nmc", "dtype", "pred_h", "mi", "energy", "msp", "label", "gap")
NEW_ENTRIES = ("runia_pixel_maps_workspace_bytes", "runia_pixel_uncertainty_maps", "runia_pixel_map_reduce_f32")


def test_fixture_loads_and_has_the_keys_the_gpu_test_walks():
    g = load_npz("ref_pixel_maps.npz")  # allow_pickle=False is np.load's default: arrays only
    names = [str(n) for n in g["case_names"]]
    assert len(names) >= 10 and len(set(names)) == len(names)
    classes, samples, images, halves = set(), set(), set(), set()
    for name in names:
        for k in CASE_KEYS:
            assert f"{name}_{k}" in g.files, f"{name}_{k}"
        x, n_mc = g[f"{name}_logits"], int(g[f"{name}_nmc"])
        assert x.dtype == np.float32 and x.ndim == 4 and x.shape[0] % n_mc == 0
        assert np.abs(x).max() <= 20.0
        shape = (x.shape[0] // n_mc, x.shape[2], x.shape[3])
        for k in ("pred_h", "mi", "energy", "msp", "gap"):
            assert g[f"{name}_{k}"].shape == shape and g[f"{name}_{k}"].dtype == np.float32
            assert np.isfinite(g[f"{name}_{k}"]).all()
        assert g[f"{name}_label"].shape == shape and g[f"{name}_label"].dtype == np.int32
        assert float((g[f"{name}_gap"] <= 1e-6).mean()) <= 0.01
        dt = str(g[f"{name}_dtype"])
        if dt != "f32":  # half inputs are stored as their exact f32 values
            t = torch.from_numpy(x)
            assert torch.equal(t.to(torch.bfloat16 if dt == "bf16" else torch.float16).to(torch.float32), t)
        classes.add(x.shape[1]); samples.add(n_mc); images.add(shape[0]); halves.add(dt)
    assert classes == {1, 2, 19, 21, 150, 257} and samples == {1, 2, 5, 16} and images == {1, 3}
    assert halves == {"f32", "f16", "bf16"}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_pixel_maps.npz")) < 1 << 20


def test_header_binding_and_makefile_list_the_new_entries():
    header = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols()
    makefile = open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bpixel_maps\.hip\b", makefile, flags=re.M)
    lib = _hip.load_library()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name)
    assert lib.runia_abi_version() == 6  # additive entries


def test_argument_checks_come_before_any_launch():
    lib = _hip.load_library()
    P = 4096  # any non-null address: never dereferenced on these paths
    INVALID, WORKSPACE = -1, -4

    def maps(table=P, single=1, dtype=0, G=2, n_mc=2, C=19, H=4, W=8, sn=608, sc=32, sh=8, sw=1, pred_h=P, mi=None,
             msp=None, energy=None, max_logit=None, label=None, mean_probs=None, ws=None, ws_bytes=0):
        return lib.runia_pixel_uncertainty_maps(table, single, dtype, G, n_mc, C, H, W, sn, sc, sh, sw, pred_h, mi, msp,
                                                energy, max_logit, label, mean_probs, ws, ws_bytes, None)

    assert maps(G=0) == 0 and maps(H=0) == 0 and maps(W=0) == 0          # nothing to do: no launch
    assert maps(G=0, table=None, pred_h=None) == 0
    assert maps(G=-1) == INVALID and maps(C=0) == INVALID and maps(n_mc=0) == INVALID and maps(H=-1) == INVALID
    assert maps(dtype=3) == INVALID and maps(dtype=-1) == INVALID and maps(single=2) == INVALID
    assert maps(sn=-1) == INVALID and maps(sc=-1) == INVALID and maps(sh=-1) == INVALID and maps(sw=-1) == INVALID
    assert maps(G=1 << 31) == INVALID and maps(C=1 << 31) == INVALID
    assert maps(table=None) == INVALID
    assert maps(pred_h=None) == INVALID                                   # at least one output
    # row statistics beyond LDS (n_mc > 21, two-pass kernel) need the caller's workspace
    need = lib.runia_pixel_maps_workspace_bytes(2, 150, 4, 8, 32, 0)
    assert need == 32 * 3 * (2 * 4 * 8) * 4
    assert lib.runia_pixel_maps_workspace_bytes(2, 19, 4, 8, 32, 0) == 0  # register kernel
    assert lib.runia_pixel_maps_workspace_bytes(2, 19, 4, 8, 32, 1) == need  # max_logit goes to the two-pass kernel
    assert lib.runia_pixel_maps_workspace_bytes(2, 150, 4, 8, 21, 0) == 0 and lib.runia_pixel_maps_workspace_bytes(2, 150, 4, 8, 22, 0) > 0
    assert maps(C=150, n_mc=32, sn=4800) == WORKSPACE
    assert maps(C=150, n_mc=32, sn=4800, ws=P, ws_bytes=need - 4) == WORKSPACE
    assert maps(C=150, n_mc=32, sn=4800, ws=P + 2, ws_bytes=need) == WORKSPACE  # misaligned

    def reduce(m=P, valid=None, G=2, HW=32, mean=P, mx=None, cnt=None):
        return lib.runia_pixel_map_reduce_f32(m, valid, G, HW, mean, mx, cnt, None)

    assert reduce(G=0) == 0 and reduce(G=0, m=None, mean=None) == 0
    assert reduce(G=-1) == INVALID and reduce(HW=-1) == INVALID and reduce(G=1 << 31) == INVALID
    assert reduce(m=None) == INVALID and reduce(mean=None) == INVALID


def test_public_refusals_name_the_offending_value():
    from runia_core_amd.inference import pixel_level as pl

    x = torch.zeros(6, 3, 4, 5)
    with pytest.raises(ValueError, match=r"unknown score 'entropy'"):
        pl.pixel_uncertainty_maps(x, 2, scores=("pred_h", "entropy"))
    with pytest.raises(ValueError, match=r"first dimension of the logits \(6\) is not divisible by mcd_nro_samples \(4\)"):
        pl.pixel_uncertainty_maps(x, 4)
    with pytest.raises(ValueError, match=r"got shape \(6, 3\)"):
        pl.pixel_uncertainty_maps(torch.zeros(6, 3), 2)
    with pytest.raises(ValueError, match="torch.float64"):
        pl.pixel_uncertainty_maps(x.double(), 2)
    with pytest.raises(ValueError, match="mcd_nro_samples must be a positive integer, got 0"):
        pl.pixel_uncertainty_maps(x, 0)
    a = torch.zeros(2, 3, 4, 5)
    with pytest.raises(ValueError, match=r"list holds 2 passes, mcd_nro_samples is 3"):
        pl.pixel_uncertainty_maps([a, a], 3)
    with pytest.raises(ValueError, match=r"pass 1 has shape \(2, 3, 4, 6\)"):
        pl.pixel_uncertainty_maps([a, torch.zeros(2, 3, 4, 6)], 2)
    with pytest.raises(ValueError, match="pass 1 has dtype torch.float16"):
        pl.pixel_uncertainty_maps([a, a.half()], 2)
    with pytest.raises(ValueError, match=r"pass 1 has strides \(60, 1, 15, 3\)"):
        pl.pixel_uncertainty_maps([a, a.contiguous(memory_format=torch.channels_last)], 2)
    with pytest.raises(ValueError, match="nothing requested"):
        pl.pixel_uncertainty_maps(x, 2, scores=())
    with pytest.raises(ValueError, match="reduction must be 'mean' or 'max', got 'sum'"):
        pl.image_scores_from_maps(torch.zeros(2, 4, 5), reduction="sum")
    with pytest.raises(ValueError, match=r"valid has shape \(2, 4, 4\)"):
        pl.image_scores_from_maps(torch.zeros(2, 4, 5), valid=torch.ones(2, 4, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"ood_mask has shape \(2, 4\)"):
        pl.pixel_ood_metrics(torch.zeros(2, 4, 5), torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="unknown score 'h'"):
        pl.get_pixel_mcd_uncertainty_maps(torch.nn.Identity(), [], 2, scores=("h",))
    # existing behaviour kept: the row function still refuses 4-D logits through its own checks
    with pytest.raises(AssertionError, match="divisible by the mcd_nro_samples"):
        from runia_core_amd.inference import get_predictive_uncertainty_score
        get_predictive_uncertainty_score(torch.zeros(7, 3), 2)


def test_public_names_are_exported():
    import runia_core_amd.inference as inf
    from runia_core_amd.inference import pixel_level as pl

    names = ("pixel_uncertainty_maps", "get_pixel_mcd_uncertainty_maps", "image_scores_from_maps", "pixel_ood_metrics")
    for n in names:
        assert n in pl.__all__ and callable(getattr(pl, n))
        assert getattr(inf, n) is getattr(pl, n)
    assert pl.PIXEL_MAP_SCORES == ("pred_h", "mi", "msp", "energy", "max_logit")
    doc = pl.pixel_uncertainty_maps.__doc__
    assert "0 * log 0" in doc and "NaN" in doc


def test_no_cpu_fallback(monkeypatch):
    from runia_core_amd.inference import pixel_level as pl

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.RuniaHipError, match="no CPU fallback"):
        pl.pixel_uncertainty_maps(torch.zeros(2, 3, 4, 5), 2)
    with pytest.raises(_hip.RuniaHipError):
        pl.image_scores_from_maps(torch.zeros(2, 4, 5))
    with pytest.raises(_hip.RuniaHipError):
        pl.get_pixel_mcd_uncertainty_maps(torch.nn.Identity(), [(torch.zeros(1, 3, 4, 5), 0)], 2)
