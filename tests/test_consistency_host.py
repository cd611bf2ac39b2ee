"""Sample-consistency scores without a GPU: the NumPy statement (tests/consistency_cases.py) against hand-worked values, the
prefix-max row recurrence against the textbook DP, the two forms of Ecc, the guards of the shared cases, word_ids, the ABI
table, the pipeline's key names and the argument errors of every public function."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

import consistency_cases as cc
import runia_core_amd.llm_uncertainty as L
from runia_core_amd import _hip
from runia_core_amd.llm_uncertainty import consistency as C
from test_llm_pipeline_host import _Model, _Tok, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the statement itself ---------------------------------------------------------------------------------------------------
def test_pair_matrix_has_the_closed_form_spectrum():
    w, exp = cc.hand_matrices()["pair"]
    s = cc.graph_scores(w)
    assert np.allclose(s["eigenvalues"], exp["eigenvalues"], atol=1e-15)
    assert s["lexical_similarity"] == pytest.approx(0.3, abs=1e-16)
    assert s["u_deg"] == pytest.approx(1 - (2 + 0.6) / 4, abs=1e-16)
    assert np.allclose(s["c_deg"], [0.65, 0.65], atol=1e-16)
    assert s["num_sets"] == 2 and cc.graph_scores(w, set_threshold=0.3)["num_sets"] == 1


@pytest.mark.parametrize("k", [2, 3, 6, 17])
def test_hand_worked_matrices(k):
    h = cc.hand_matrices(k)
    s = cc.graph_scores(h["ones"][0])
    assert np.allclose(s["eigenvalues"], [0.0] + [1.0] * (k - 1), atol=1e-14)
    assert s["u_eigv"] == pytest.approx(1.0, abs=1e-13) and s["u_deg"] == pytest.approx(0.0, abs=1e-15)
    assert s["num_sets"] == 1 and s["lexical_similarity"] == 1.0 and s["u_ecc"] == pytest.approx(0.0, abs=1e-14)
    s = cc.graph_scores(h["identity"][0])
    assert np.allclose(s["eigenvalues"], 0.0, atol=1e-15) and s["u_eigv"] == pytest.approx(float(k), abs=1e-14)
    assert s["u_ecc"] == pytest.approx(np.sqrt(k - 1), abs=1e-14) and s["num_sets"] == k
    assert np.allclose(s["c_ecc"], -np.sqrt(1 - 1 / k), atol=1e-14) and np.allclose(s["c_deg"], 1 / k, atol=1e-16)
    if k >= 4:
        s = cc.graph_scores(h["two_blocks"][0])
        assert s["u_eigv"] == pytest.approx(2.0, abs=1e-13) and s["num_sets"] == 2
        assert np.allclose(s["eigenvalues"][:2], 0.0, atol=1e-14) and np.allclose(s["eigenvalues"][2:], 1.0, atol=1e-14)


def test_lower_triangle_and_diagonal_are_not_read():
    w = cc.rouge_w(5, cc.SPECTRAL_SEEDS[5])
    g = w.copy()
    g[np.tril_indices(5, -1)] = np.nan
    np.fill_diagonal(g, 7.0)
    a, b = cc.graph_scores(w), cc.graph_scores(g)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def test_non_finite_entry_gives_nan_and_minus_one():
    w = cc.rouge_w(3, cc.SPECTRAL_SEEDS[3]).copy()
    w[0, 2] = np.inf
    s = cc.graph_scores(w)
    assert s["num_sets"] == -1 and np.isnan(s["u_eigv"]) and np.isnan(s["eigenvalues"]).all() and np.isnan(s["c_deg"]).all()


def test_prefix_max_recurrence_equals_the_dp():
    rng = np.random.default_rng(5)
    for trial in range(300):
        na, nb = rng.integers(0, 40, size=2)
        vocab = int(rng.integers(2, 8))
        a, b = rng.integers(0, vocab, size=na), rng.integers(0, vocab, size=nb)
        assert cc.lcs_scan(a, b) == cc.lcs_dp(a, b) == cc.lcs_dp(b, a), (a, b)
    assert cc.lcs_dp([1, 2, 3, 4, 1], [3, 4, 1, 2, 1, 3]) == 3  # "3 4 1"
    assert cc.lcs_dp([], [1]) == 0 and cc.lcs_scan([], [1]) == 0


def test_counts_and_similarities_by_hand():
    ids, eos = cc.eos_group()
    ln, lcs, uq, it = cc.pair_counts(ids, 4, eos=eos)
    assert ln.tolist() == [0, 3, 3, 8] and uq.tolist() == [0, 3, 3, 7]
    assert lcs[0, 1, 2] == 3 and lcs[0, 1, 3] == 3 and lcs[0, 0, 1] == 0 and np.array_equal(np.diagonal(lcs[0]), ln)
    assert it[0, 1, 2] == 3 and it[0, 1, 3] == 3 and it[0, 0, 3] == 0
    w = cc.similarity(ln, lcs, uq, it, "rouge_l")[0]
    assert w[1, 2] == 1.0 and w[0, 1] == 0.0 and w[1, 3] == pytest.approx(6 / 11) and np.array_equal(np.diagonal(w), np.ones(4))
    j = cc.similarity(ln, lcs, uq, it, "jaccard")[0]
    assert j[1, 3] == pytest.approx(3 / 7) and j[0, 0] == 1.0 and j[0, 2] == 0.0
    # both empty: 1
    ln, lcs, uq, it = cc.pair_counts(np.array([[1, 2], [1, 3]]), 2, eos=(1,))
    assert cc.similarity(ln, lcs, uq, it, "rouge_l")[0, 0, 1] == 1.0 and cc.similarity(ln, lcs, uq, it, "jaccard")[0, 0, 1] == 1.0
    # lengths and start
    ln, lcs, _, _ = cc.pair_counts(np.array([[9, 2, 3, 4], [9, 2, 4, 4]]), 2, start=1, lengths=[3, 2])
    assert ln.tolist() == [3, 2] and lcs[0, 0, 1] == 2


def test_both_ecc_forms_agree():
    for k in cc.SPECTRAL_KS:
        w = cc.rouge_w(k, cc.SPECTRAL_SEEDS[k])
        lam, vec = np.linalg.eigh(cc.laplacian(w)[0])
        sel = vec[:, lam < cc.EIGV_THRESHOLD]
        assert sel.shape[1] >= 1
        assert np.allclose(cc.ecc_centred(sel) ** 2, cc.ecc_projector(sel), atol=1e-13)
    for w, _ in cc.hand_matrices().values():
        lam, vec = np.linalg.eigh(cc.laplacian(w)[0])
        sel = vec[:, lam < cc.EIGV_THRESHOLD]
        assert np.allclose(cc.ecc_centred(sel) ** 2, cc.ecc_projector(sel), atol=1e-13)


def test_shared_cases_keep_their_distance_from_the_thresholds():
    for k in cc.SPECTRAL_KS:
        cc.guard(cc.rouge_w(k, cc.SPECTRAL_SEEDS[k]), set_threshold=cc.RANDOM_SET_THRESHOLD)
    for w, _ in cc.hand_matrices().values():
        cc.guard(w)
    with pytest.raises(AssertionError):
        cc.guard(np.array([[1.0, 0.5], [0.5, 1.0]]))


def test_case_builders_have_the_sizes_they_promise():
    ids, lengths = cc.length_mix_group()
    assert tuple(lengths) == cc.LENGTH_MIX and ids.shape == (8, 129)
    ids, lengths = cc.max_t_pair()
    assert ids.shape == (2, cc.MAX_T) and lengths.tolist() == [cc.MAX_T, cc.MAX_T - 1]
    hb = cc.high_bit_pair()
    assert np.array_equal(hb.astype(np.int32)[0], hb.astype(np.int32)[1]) and not np.array_equal(hb[0], hb[1])
    _, lcs, _, it = cc.pair_counts(hb, 3)
    assert lcs[0, 0, 1] == 0 and lcs[0, 0, 2] == 6 and it[0, 0, 1] == 0
    ids, lengths, k = cc.jaccard_groups()["uniq_64_65"]
    _, _, uq, it = cc.pair_counts(ids, k, lengths=lengths)
    assert uq.tolist() == [64, 65, 65] and it[0, 1, 2] == 65 and it[0, 0, 1] == 64
    p = cc.pattern_groups()
    ln, lcs, _, it = cc.pair_counts(p["identical"], 2)
    assert lcs[0, 0, 1] == ln[0]
    assert cc.pair_counts(p["disjoint"], 2)[1][0, 0, 1] == 0 and cc.pair_counts(p["one_id"], 2)[1][0, 0, 1] == 70


# ---- word_ids -----------------------------------------------------------------------------------------------------------------
def test_word_ids_punctuation_case_and_empty_strings():
    ids, lengths = L.word_ids(["The cat, the CAT!", "", "cat-the 42nd", "...", "Ünï the"])
    assert ids.dtype == torch.int64 and lengths.dtype == torch.int64 and ids.shape == (5, 4)
    assert lengths.tolist() == [4, 0, 3, 0, 2]  # "Ünï" keeps its ASCII run "n": the split is [a-z0-9]+ after lower()
    assert ids[0].tolist() == [1, 2, 1, 2] and ids[1].tolist() == [0, 0, 0, 0]
    assert ids[2].tolist() == [2, 1, 3, 0] and ids[3].tolist() == [0, 0, 0, 0]
    assert ids[4].tolist() == [4, 1, 0, 0]
    ids, lengths = L.word_ids(["", ""])
    assert ids.shape == (2, 1) and lengths.tolist() == [0, 0]
    with pytest.raises(TypeError):
        L.word_ids("one string")
    with pytest.raises(TypeError):
        L.word_ids(["a", 3])


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_header_table_and_the_library_with_the_stream_last():
    lib = _hip.load_library()
    text = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    for name in ("runia_cons_pairs", "runia_cons_graph"):
        assert name in _hip.exported_symbols() and hasattr(lib, name)
        res, args = _hip._SIGNATURES[name]
        assert res is _hip.c_int and args[-1] is _hip.c_void_p
        decl = re.search(rf"\b{name}\s*\(([^()]*)\)\s*;", text).group(1)
        assert decl.split(",")[-1].split() == ["runia_stream_t", "stream"]
    assert "runia_cons_pairs_workspace_bytes" in _hip.exported_symbols()
    assert _hip._SIGNATURES["runia_cons_pairs_workspace_bytes"][0] is _hip.c_int64  # (every size_t query is pinned in a table)
    assert (_hip.CONS_MAX_K, _hip.CONS_MAX_T) == (cc.MAX_K, cc.MAX_T) == (64, 4096)
    assert lib.runia_abi_version() == 6  # additive entries
    assert "consistency.hip" in open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    # the sizing query and the refusals need no device
    assert lib.runia_cons_pairs_workspace_bytes(3, 4, 100, 3) == 3 * 4 * 100 * 8
    assert lib.runia_cons_pairs_workspace_bytes(3, 4, 100, 1) == 0 and lib.runia_cons_pairs_workspace_bytes(3, 65, 100, 3) == 0
    assert lib.runia_cons_pairs(None, 4, 1, 2, 8, 8, 1, None, 0, None, 1, None, None, None, None, None, 0, None) == -1
    assert lib.runia_cons_graph(None, 1, 2, 0.9, 0.5, None, None, None, None, None, None, None, None, None) == -1


def test_package_exports_the_new_names():
    for n in ("PairCounts", "ConsistencyScores", "pairwise_counts", "pairwise_similarity", "graph_scores", "consistency_scores",
              "word_ids"):
        assert n in L.__all__ and hasattr(L, n) and n in C.__all__
    assert C.ConsistencyScores._fields == ("eigenvalues", "u_deg", "u_eigv", "u_ecc", "lexical_similarity", "c_deg", "c_ecc",
                                           "num_sets", "similarity")
    assert C.PairCounts._fields == ("len", "lcs", "uniq", "inter")


# ---- pipeline -----------------------------------------------------------------------------------------------------------------
NAMES = ("lexical_similarity", "deg", "ecc", "eigv", "num_sets")


def test_pipeline_key_names():
    from runia_core_amd.llm_uncertainty.pipeline import _NEEDS_SAMPLING, _score_name

    for m in NAMES:
        assert _NEEDS_SAMPLING[m] is True
        assert _score_name({"method_name": m}) == m == _score_name({"method_name": m, "similarity": "rouge_l"})
        assert _score_name({"method_name": m, "similarity": "jaccard"}) == f"{m}_jaccard"
        with pytest.raises(KeyError):
            _score_name({"method_name": m, "similarity": "bleu"})
    assert _score_name({"method_name": "perplexity", "similarity": "bleu"}) == "perplexity"  # not a consistency request


def test_unknown_similarity_raises_key_error_before_generating():
    for f, prompt in ((L.compute_uncertainties, "a b"), (L.compute_uncertainties_batch, ["a b", "c"])):
        m = _Model()
        with pytest.raises(KeyError):
            f(m, _Tok(), prompt, [{"method_name": "deg"}, {"method_name": "eigv", "similarity": "cosine"}])
        assert m.calls == []


@pytest.mark.parametrize("fn", ["compute_uncertainties", "compute_uncertainties_batch"])
def test_consistency_requests_sample(fn):
    prompt = "the cat sat" if fn == "compute_uncertainties" else ["the cat sat", "a dog"]
    for name in NAMES:
        m = _Model()
        _run(getattr(L, fn), m, _Tok(), prompt, [{"method_name": name}], None, 3)
        assert len(m.calls) == 2 and m.calls[1]["num_return_sequences"] == 3


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_id_functions_refuse_bad_arguments_before_the_device():
    ok = torch.zeros(6, 5, dtype=torch.int64)
    for f in (L.pairwise_counts, L.pairwise_similarity, L.consistency_scores):
        with pytest.raises(ValueError):
            f(torch.zeros(6, dtype=torch.int64), 3)          # not 2-D
        with pytest.raises(ValueError):
            f(ok.numpy(), 3)                                 # not a tensor
        with pytest.raises(TypeError):
            f(ok.float(), 3)
        with pytest.raises(TypeError):
            f(ok.to(torch.int16), 3)
        with pytest.raises(ValueError):
            f(ok, 4)                                         # 6 rows, groups of 4
        with pytest.raises(ValueError):
            f(ok, 1)
        with pytest.raises(ValueError):
            f(torch.zeros(130, 5, dtype=torch.int64), 65)    # K above the limit
        with pytest.raises(ValueError):
            f(torch.zeros(2, cc.MAX_T + 1, dtype=torch.int32), 2)
        with pytest.raises(ValueError):
            f(ok, 3, start=6)
        with pytest.raises(ValueError):
            f(ok, 3, start=-1)
        with pytest.raises(ValueError):
            f(ok, 3, lengths=torch.zeros(5, dtype=torch.int64))
        with pytest.raises(TypeError):
            f(ok, 3, lengths=torch.zeros(6))
        with pytest.raises(ValueError):
            f(ok, 3, eos_token_id=list(range(17)))
    with pytest.raises(ValueError):
        L.pairwise_counts(ok, 3, jaccard=False, lcs=False)
    for f in (L.pairwise_similarity, L.consistency_scores):
        with pytest.raises(ValueError):
            f(ok, 3, kind="bleu")
    # a width within the limit after `start` passes the checks (and then needs the device)
    view, k, lengths = C._checked_ids(torch.zeros(2, cc.MAX_T + 3, dtype=torch.int32), 2, 3, [1, 2])
    assert view.shape == (2, cc.MAX_T) and k == 2 and lengths.dtype == torch.int64


def test_graph_scores_refuses_bad_arguments_before_the_device():
    with pytest.raises(ValueError):
        L.graph_scores(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        L.graph_scores(torch.zeros(2, 3, 3, 3))
    with pytest.raises(ValueError):
        L.graph_scores(np.eye(3))
    with pytest.raises(TypeError):
        L.graph_scores(torch.eye(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        L.graph_scores(torch.eye(1))
    with pytest.raises(ValueError):
        L.graph_scores(torch.zeros(2, 65, 65))
    with pytest.raises(ValueError):
        L.graph_scores(torch.zeros(0, 3, 3))
    with pytest.raises(ValueError):
        L.graph_scores(torch.eye(3), eigv_threshold=float("nan"))


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_host_fallback():
    ids = torch.randint(2, 9, (6, 5))
    with pytest.raises(_hip.RuniaHipError):
        L.pairwise_counts(ids, 3)
    with pytest.raises(_hip.RuniaHipError):
        L.consistency_scores(ids, 3, kind="jaccard")
    with pytest.raises(_hip.RuniaHipError):
        L.graph_scores(torch.eye(4))
