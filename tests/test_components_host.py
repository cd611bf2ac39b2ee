"""Component-level metrics, the part that needs no GPU: the float64 restatement against the worked example and the two
identities, the C boundary (header, binding table, Makefile, argument checks before any launch), the refusals of the public
functions and the additivity of ``ComponentResult``."""
import os
import re

import numpy as np
import pytest
import torch

import component_cases as cc
from conftest import ROOT
from runia_core_amd import _hip
from runia_core_amd.evaluation import ComponentResult, component_metrics, label_components

NEW_ENTRIES = ("runia_cc_tile_h", "runia_cc_tile_w", "runia_cc_label_workspace_bytes", "runia_cc_label", "runia_cc_overlap",
               "runia_cc_relabel")


def test_restatement_reproduces_the_worked_example():
    c8 = cc.image_components(cc.EXAMPLE_GT, cc.EXAMPLE_PRED, 8)
    assert c8["siou"].tolist() == [2 / 6, 1 / 6] and c8["ppv"].tolist() == [3 / 5, 0.0]
    assert c8["gt_size"].tolist() == [4, 4] and c8["pred_size"].tolist() == [5, 2]
    score = cc.EXAMPLE_PRED.astype(np.float32)[None]
    r = cc.dataset_metrics(score, cc.EXAMPLE_GT[None], [0.5], connectivity=8)
    assert (r["tp"][0, 0], r["fn"][0, 0], r["fp"][0, 0]) == (1, 1, 1) and r["f1"][0, 0] == 0.5
    c4 = cc.image_components(cc.EXAMPLE_GT, cc.EXAMPLE_PRED, 4)
    assert c4["pred_size"].tolist() == [5, 1, 1] and c4["ppv"].tolist() == [3 / 5, 0.0, 0.0]
    assert c4["siou"].tolist() == [2 / 6, 1 / 6]


def test_restatement_special_cases():
    c = cc.image_components(cc.SPECIAL_GT, cc.SPECIAL_PRED, 8)
    assert c["siou"][0] == 0.25                      # X: exactly tau = 0.25 -> a false negative there
    assert c["gt_inter"].tolist() == [1, 4, 2, 1] and c["pred_size"].tolist() == [1, 2, 2, 4]
    assert c["gt_union"].tolist() == [4, 5, 5, 3]    # Z and W share one predicted component with one background pixel
    r = cc.dataset_metrics(cc.SPECIAL_PRED.astype(np.float32)[None], cc.SPECIAL_GT[None], [0.5])
    assert r["tp"][0, 0] == 3 and r["fn"][0, 0] == 1


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_two_identities_hold_on_random_masks(connectivity):
    rng = np.random.default_rng(connectivity)
    for i in range(100):
        h, w = rng.integers(3, 14), rng.integers(3, 18)
        gt, pred = rng.random((h, w)) < rng.uniform(0.1, 0.6), rng.random((h, w)) < rng.uniform(0.1, 0.6)
        valid = rng.random((h, w)) < 0.9 if i % 3 == 0 else None
        c = cc.image_components(gt, pred, connectivity, min_size=int(i % 4 == 1) * 3, valid=valid)
        assert np.array_equal(c["gt_inter"], c["inter_id"]) and np.array_equal(c["gt_union"], c["union_id"])


def test_min_size_and_valid_in_the_restatement():
    c = cc.image_components(cc.EXAMPLE_GT, cc.EXAMPLE_PRED, 8, min_size=3)
    assert c["pred_size"].tolist() == [5]
    valid = np.ones_like(cc.EXAMPLE_GT)
    valid[:, 3] = False  # cuts the predicted bar in two
    c = cc.image_components(cc.EXAMPLE_GT, cc.EXAMPLE_PRED, 8, valid=valid)
    assert c["pred_size"].tolist() == [2, 2, 2] and c["siou"].tolist() == [2 / 4, 1 / 5]


def test_header_binding_and_makefile_list_the_new_entries():
    header = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load_library()
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/runia_hip.h"
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    makefile = open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bcomponents\.hip\b", makefile, flags=re.M)
    th = int(re.search(r"#define RUNIA_CC_TILE_H (\d+)", code).group(1))
    tw = int(re.search(r"#define RUNIA_CC_TILE_W (\d+)", code).group(1))
    assert _hip.CC_TILE == (th, tw) == (lib.runia_cc_tile_h(), lib.runia_cc_tile_w())
    assert lib.runia_abi_version() == 6  # additive entries
    assert b"step cap" in lib.runia_error_string(-5)


def test_argument_checks_come_before_any_launch():
    lib = _hip.load_library()
    P = 4096  # any non-null address: never dereferenced on these paths
    INVALID, WORKSPACE = -1, -4

    def lab(mask=P, score=None, thr=None, T=1, less=0, valid=None, G=2, H=8, W=8, conn=8, labels=P, counts=P, ws=P, ws_bytes=1 << 20):
        return lib.runia_cc_label(mask, score, thr, T, less, valid, G, H, W, conn, labels, counts, ws, ws_bytes, None)

    assert lab(G=0) == 0 and lab(H=0) == 0 and lab(W=0) == 0 and lab(mask=None, score=P, thr=P, T=0) == 0
    assert lab(conn=6) == INVALID and lab(G=-1) == INVALID and lab(H=-1) == INVALID
    assert lab(mask=None) == INVALID and lab(score=P, thr=P) == INVALID and lab(T=2) == INVALID
    assert lab(mask=None, score=P, thr=None, T=2) == INVALID and lab(labels=None) == INVALID and lab(counts=None) == INVALID
    assert lab(G=1, H=1 << 16, W=1 << 15) == INVALID                      # 2^31 pixels: parents are int32
    assert lab(mask=None, score=P, thr=P, T=1 << 11, G=1, H=1 << 10, W=1 << 10) == INVALID
    assert lab(ws=None) == WORKSPACE and lab(ws_bytes=8) == WORKSPACE and lab(ws=P + 4) == WORKSPACE
    assert lib.runia_cc_label_workspace_bytes(0, 8, 8) == 0
    assert lib.runia_cc_label_workspace_bytes(3, 33, 64) == 16 + 2 * 3 * 3 * 4   # three 1024-pixel chunks per image

    def ov(gt=P, goff=P, pred=P, poff=P, G=2, T=2, H=8, W=8, Kg=3, gs=P, gi=P, ps=P, pi=P, keys=None, cap=0, nk=P, stats=1):
        return lib.runia_cc_overlap(gt, goff, pred, poff, G, T, H, W, Kg, gs, gi, ps, pi, keys, cap, nk, stats, None)

    assert ov(G=0) == 0 and ov(H=0) == 0 and ov(T=0) == 0
    assert ov(G=-1) == INVALID and ov(gt=None, pred=None) == INVALID and ov(goff=None) == INVALID and ov(poff=None) == INVALID
    assert ov(ps=None) == INVALID and ov(gi=None) == INVALID and ov(keys=P, nk=None) == INVALID
    assert ov(G=1, T=1 << 11, H=1 << 10, W=1 << 10) == INVALID
    assert lib.runia_cc_relabel(P, P, P, 0, 8, 8, None) == 0 and lib.runia_cc_relabel(None, P, P, 1, 8, 8, None) == INVALID


def test_refusals_are_raised_before_the_gpu_is_required():
    s, m = torch.zeros((2, 4, 5)), torch.zeros((2, 4, 5), dtype=torch.bool)
    with pytest.raises(ValueError, match="connectivity"):
        component_metrics(s, m, 0.5, connectivity=6)
    with pytest.raises(ValueError, match="connectivity"):
        label_components(m, connectivity=6)
    with pytest.raises(ValueError, match="anomaly_if"):
        component_metrics(s, m, 0.5, anomaly_if="higher")
    with pytest.raises(ValueError, match="ood_mask has shape"):
        component_metrics(s, m[:1], 0.5)
    with pytest.raises(ValueError, match="valid has shape"):
        component_metrics(s, m, 0.5, valid=m[:, :2])
    with pytest.raises(ValueError, match="valid has shape"):
        label_components(m, valid=m[0])
    with pytest.raises(ValueError, match="bool or uint8"):
        component_metrics(s, m.float(), 0.5)
    with pytest.raises(ValueError, match="score_map must be"):
        component_metrics(s[0], m[0], 0.5)
    with pytest.raises(ValueError, match="dtype"):
        component_metrics(s.double(), m, 0.5)
    with pytest.raises(ValueError, match="finite"):
        component_metrics(s, m, [0.1, float("nan")])
    with pytest.raises(ValueError, match="finite"):
        component_metrics(s, m, float("inf"))
    with pytest.raises(ValueError, match="1-D"):
        component_metrics(s, m, [[0.1, 0.2]])
    with pytest.raises(ValueError, match="finite"):
        component_metrics(s, m, 0.5, iou_thresholds=[float("nan")])
    with pytest.raises(ValueError, match="min_component_size"):
        component_metrics(s, m, 0.5, min_component_size=-1)
    with pytest.raises(ValueError, match="min_component_size"):
        component_metrics(s, m, 0.5, min_component_size=1.5)
    with pytest.raises(ValueError, match="mask must be"):
        label_components(m[None])


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_cpu_fallback():
    s, m = torch.zeros((2, 4, 5)), torch.zeros((2, 4, 5), dtype=torch.bool)
    with pytest.raises(_hip.RuniaHipError):
        component_metrics(s, m, 0.5)
    with pytest.raises(_hip.RuniaHipError):
        label_components(m)


def _as_result(r, thresholds, taus):
    return ComponentResult(np.asarray(thresholds, np.float64), np.asarray(taus, np.float64), r["n_gt"], r["n_pred"],
                           r["sum_siou"], r["sum_ppv"], r["tp"], r["fn"], r["fp"], dict(r["components"]))


def test_component_result_adds_two_halves_to_the_whole():
    score, gt = cc.blob_images(4, 20, 30, seed=5)
    thr, taus = [0.25, 0.5, 0.75], cc.DEFAULT_TAUS
    whole = _as_result(cc.dataset_metrics(score, gt, thr), thr, taus)
    a = _as_result(cc.dataset_metrics(score[:2], gt[:2], thr), thr, taus)
    b = _as_result(cc.dataset_metrics(score[2:], gt[2:], thr), thr, taus)
    s = a + b
    assert whole.n_gt.min() > 0 and whole.n_pred.min() > 0
    for k in ("n_gt", "n_pred", "tp", "fn", "fp"):
        assert np.array_equal(getattr(s, k), getattr(whole, k)), k
    for k in ("sum_siou", "sum_ppv", "mean_siou", "mean_ppv", "f1_star"):
        assert np.allclose(getattr(s, k), getattr(whole, k), rtol=1e-13, atol=0), k
    assert np.array_equal(s.f1, whole.f1, equal_nan=True)
    # the tables are concatenated with the right operand's images numbered on: the same multiset of rows as the whole
    def rows(res, keys):
        return sorted(zip(*(res.components[k].tolist() for k in keys)))
    assert rows(s, ("gt_threshold", "gt_image", "gt_size", "gt_inter", "siou")) == \
        rows(whole, ("gt_threshold", "gt_image", "gt_size", "gt_inter", "siou"))
    assert rows(s, ("pred_threshold", "pred_image", "pred_size", "pred_inter", "ppv")) == \
        rows(whole, ("pred_threshold", "pred_image", "pred_size", "pred_inter", "ppv"))
    with pytest.raises(ValueError, match="different"):
        a + _as_result(cc.dataset_metrics(score[2:], gt[2:], [0.3]), [0.3], taus)
    # properties of an empty result: NaN means, NaN F1
    e = ComponentResult(np.zeros(1), np.asarray(taus), np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1), np.zeros(1),
                        *(np.zeros((1, len(taus)), np.int64) for _ in range(3)))
    assert np.isnan(e.mean_siou).all() and np.isnan(e.mean_ppv).all() and np.isnan(e.f1).all() and np.isnan(e.f1_star).all()
