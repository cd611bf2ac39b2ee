"""MaxLogit / KL-Matching / fDBD / Relative Mahalanobis without a GPU: the float64 restatements of
tests/extended_baseline_cases.py against independent forms, the second registry, argument errors, pickling and the header."""
import os
import pickle
import re

import numpy as np
import pytest

import extended_baseline_cases as cases
from conftest import ROOT


def test_klm_restatement_matches_rel_entr_double_loop():
    from scipy.special import rel_entr, softmax

    g = np.random.default_rng(0)
    logits = g.standard_normal((7, 5)) * 2.0
    q = softmax(g.standard_normal((5, 5)) * 1.5, axis=1)
    valid = np.array([1, 1, 0, 1, 1], dtype=np.int32)
    p = softmax(logits, axis=1)
    want = np.empty(7)
    for n in range(7):
        kls = []
        for c in range(5):
            if valid[c]:
                kls.append(sum(rel_entr(p[n, k], q[c, k]) for k in range(5)))
        want[n] = -min(kls)
    got = cases.klm_scores_f64(logits, np.log(q), valid)
    assert np.max(np.abs(got - want)) < 1e-12
    assert np.all(got <= 1e-12)  # a KL divergence is never negative


def test_klm_fit_restatement_groups_by_prediction():
    from scipy.special import softmax

    g = np.random.default_rng(1)
    logits = g.standard_normal((50, 4))
    logits[:, 3] -= 20.0  # class 3 is never predicted
    q, valid = cases.klm_fit_f64(logits, 4)
    assert valid.tolist() == [1, 1, 1, 0]
    p, pred = softmax(logits, axis=1), logits.argmax(1)
    for c in range(3):
        assert np.allclose(q[c], np.mean([p[n] for n in range(50) if pred[n] == c], axis=0), rtol=1e-13, atol=0)
    assert np.all(q[3] == 0)


def test_row_stats_restatement():
    from scipy.special import entr, logsumexp, softmax

    x = cases.logits_with_ties(9, 12, 2).astype(np.float64)
    x[0, 5] = -np.inf
    m, lse, ne, am = cases.row_stats_f64(x)
    assert np.array_equal(m, x.max(1)) and np.array_equal(am, np.argmax(x, 1))
    assert np.allclose(lse, logsumexp(x, axis=1), rtol=1e-14)
    assert np.allclose(ne, -entr(softmax(x, axis=1)).sum(1), rtol=1e-12) and np.all(np.isfinite(ne))


def test_fdbd_restatement_matches_row_loop():
    g = np.random.default_rng(3)
    w, b = cases.fc_layer(6, 8, 4)
    w[4] = w[1]  # two identical weight rows: their pair has no boundary and adds 0
    feats = g.standard_normal((11, 8))
    mu = g.standard_normal(8) * 0.1
    want = np.empty(11)
    for n in range(11):
        logits = [float(np.dot(w[c].astype(np.float64), feats[n]) + b[c]) for c in range(6)]
        top = int(np.argmax(logits))
        total = 0.0
        for k in range(6):
            norm = float(np.linalg.norm(w[top].astype(np.float64) - w[k].astype(np.float64)))
            if k != top and norm > 0:
                total += abs(logits[top] - logits[k]) / norm
        want[n] = total / (5 * np.linalg.norm(feats[n] - mu))
    assert np.max(np.abs(cases.fdbd_scores_f64(feats, w, b, mu) - want)) < 1e-12
    table = cases.fdbd_table_f64(w)
    assert table[1, 4] == 0 and table[4, 1] == 0 and np.all(np.diag(table) == 0) and np.array_equal(table, table.T)


def test_fdbd_inverse_distances_against_f64_table():
    from runia_core_amd.inference.extended_postprocessors import fdbd_inverse_distances

    w, _ = cases.fc_layer(65, 96, 5)
    w[7] = w[60]
    w[9] = w[8] * np.float32(1.0 + 1e-5)  # a pair whose squared distance cancels in the Gram form
    got = fdbd_inverse_distances(w)
    want = cases.fdbd_table_f64(w)
    assert got.dtype == np.float32 and got[7, 60] == 0 and np.all(np.diag(got) == 0)
    assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)) <= 1e-6


def test_rmds_restatement_is_minus_min_of_distance_differences():
    g = np.random.default_rng(6)
    x = g.standard_normal((20, 5))
    means = g.standard_normal((3, 5))
    a, b2 = g.standard_normal((5, 5)), g.standard_normal((5, 5))
    prec, bg_prec = a @ a.T + np.eye(5), b2 @ b2.T + np.eye(5)
    bg_mean = g.standard_normal((1, 5))
    d = cases.mahalanobis_distances_f64(x, means, prec)
    d0 = cases.mahalanobis_distances_f64(x, bg_mean, bg_prec)[:, 0]
    factor = 1.0  # the project's Mahalanobis score is max_k -(x - mu_k) P (x - mu_k)^T: no 1/2
    want = -factor * np.min(d - d0[:, None], axis=1)
    assert np.max(np.abs(cases.rmds_scores_f64(x, means, prec, bg_mean, bg_prec) - want)) < 1e-10
    z = x[0] - means[1]
    assert abs(d[0, 1] - z @ prec @ z) < 1e-10


def test_second_registry_extends_the_reference_registry():
    from runia_core_amd.inference import (FDBD, KLMatching, MaxLogit, RelativeMahalanobis, extended_postprocessor_input_dict,
                                          extended_postprocessors_dict, postprocessor_input_dict, postprocessors_dict)
    from runia_core_amd.inference.abstract_classes import OodPostprocessor

    assert len(postprocessors_dict) == 16 and len(extended_postprocessors_dict) == 20
    for key, cls in postprocessors_dict.items():
        assert extended_postprocessors_dict[key] is cls
        assert extended_postprocessor_input_dict[key] == postprocessor_input_dict[key]
    new = {"mls": (MaxLogit, ["logits"]), "klm": (KLMatching, ["logits"]), "fdbd": (FDBD, ["features"]),
           "rmds": (RelativeMahalanobis, ["features"])}
    for key, (cls, inputs) in new.items():
        assert extended_postprocessors_dict[key] is cls and issubclass(cls, OodPostprocessor)
        assert extended_postprocessor_input_dict[key] == inputs and key not in postprocessors_dict
    assert set(extended_postprocessor_input_dict) == set(extended_postprocessors_dict)


def test_argument_errors_name_the_keyword():
    from runia_core_amd.inference import FDBD, KLMatching, RelativeMahalanobis

    for bad in (0, -3, 2.5, None):
        with pytest.raises(ValueError, match="num_classes"):
            KLMatching(flip_sign=False, num_classes=bad)
        with pytest.raises(ValueError, match="num_classes"):
            RelativeMahalanobis(flip_sign=False, num_classes=bad)
    x = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="num_classes"):
        KLMatching(flip_sign=False, num_classes=5).setup(x)
    with pytest.raises(AssertionError, match="final_linear_layer_params"):
        FDBD(flip_sign=False).setup(x, valid_feats=x)
    with pytest.raises(AssertionError, match="valid_feats"):
        FDBD(flip_sign=False).setup(x, final_linear_layer_params={"weight": x, "bias": x[0]})
    with pytest.raises(ValueError, match="final_linear_layer_params"):
        FDBD(flip_sign=False).setup(x, valid_feats=x, final_linear_layer_params={"weight": x[:1], "bias": x[0, :1]})
    with pytest.raises(AssertionError, match="train_labels"):
        RelativeMahalanobis(flip_sign=False, num_classes=2).setup(x, valid_feats=x)
    with pytest.raises(AssertionError, match="valid_feats"):
        RelativeMahalanobis(flip_sign=False, num_classes=2).setup(x, train_labels=np.zeros(4, dtype=int))
    with pytest.raises(AssertionError, match="setup"):
        KLMatching(flip_sign=False, num_classes=3).postprocess(x)


def test_pickle_round_trip_of_objects_given_their_arrays():
    from runia_core_amd.inference import FDBD, KLMatching, MaxLogit, RelativeMahalanobis, fdbd_inverse_distances

    g = np.random.default_rng(8)
    klm = KLMatching(flip_sign=True, num_classes=4)
    klm.log_q, klm.valid = np.log(g.random((4, 4)).astype(np.float32)), np.array([1, 0, 1, 1], dtype=np.int32)
    klm.set_threshold(g.standard_normal(10))
    klm._dev = {"a device cache": object}
    fd = FDBD(flip_sign=False)
    fd.w, fd.b = cases.fc_layer(5, 8, 9)
    fd.train_mean, fd.inv_dist = g.standard_normal(8).astype(np.float32), fdbd_inverse_distances(fd.w)
    fd.set_threshold(g.standard_normal(10))
    fd._dev = {"a device cache": object}
    rm = RelativeMahalanobis(flip_sign=False, num_classes=3)
    rm.class_mean, rm.precision = g.standard_normal((3, 6)), np.eye(6)
    rm.background_mean, rm.background_precision = g.standard_normal((1, 6)), 2.0 * np.eye(6)
    rm.set_threshold(g.standard_normal(10))
    rm._state = ("device", "copies")
    ml = MaxLogit(flip_sign=False)
    ml.set_threshold(g.standard_normal(10))
    for obj in (klm, fd, rm, ml):
        back = pickle.loads(pickle.dumps(obj))
        assert type(back) is type(obj) and back._setup_flag and back.threshold == obj.threshold
        assert back.flip_sign == obj.flip_sign
        for name, value in obj.__dict__.items():
            if name in obj._device_cache_attrs:
                assert getattr(back, name) is None  # device copies are rebuilt on first use
            elif isinstance(value, np.ndarray):
                assert np.array_equal(getattr(back, name), value) and getattr(back, name).dtype == value.dtype


def test_header_declares_the_new_symbols():
    from runia_core_amd import _hip

    new = ["runia_row_logit_stats_f32", "runia_klm_score_f32", "runia_fdbd_score_f32", "runia_row_dist_f32"]
    with open(os.path.join(ROOT, "include", "runia_hip.h")) as f:
        header = f.read()
    lib = _hip.load_library()
    for name in new:
        assert name in _hip.exported_symbols() and hasattr(lib, name)
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/runia_hip.h"
        assert len(decl.group(1).split(",")) == len(_hip._SIGNATURES[name][1])
    assert lib.runia_abi_version() == 6


def test_harness_refuses_missing_logits_by_name():
    from runia_core_amd.evaluation.extended_baselines import calculate_extended_baselines, extended_baseline_names

    assert extended_baseline_names == ("mls", "klm", "fdbd", "rmds")
    with pytest.raises(KeyError, match="train logits"):
        calculate_extended_baselines(["mls"], {}, {}, None, {"ood_datasets": []}, 10)
    ind, ood, scores = calculate_extended_baselines(["energy"], {}, {}, None, {"ood_datasets": ["a"]}, 10)
    assert scores == {} and ind == {} and ood == {}
