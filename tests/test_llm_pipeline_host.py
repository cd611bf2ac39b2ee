"""compute_uncertainties / compute_uncertainties_batch / eigen_scores without a GPU: the fixture of the reference's own
compute_uncertainties (tests/golden/ref_llm_pipeline.npz, tools/make_goldens_llm_pipeline.py), the exported names, the
result keys and errors, the generate() calls, and the ABI table."""
from __future__ import annotations

import json
import os
import re
import types

import numpy as np
import pytest
import torch

import runia_core_amd.llm_uncertainty as L
from runia_core_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_llm_pipeline.npz")


def load():
    return np.load(FIXTURE, allow_pickle=False)


def log_softmax(x):
    x = x.astype(np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def test_fixture_loads_without_pickle_and_is_small():
    d = load()
    assert os.path.getsize(FIXTURE) < 400 * 1024
    cases = list(d["cases"])
    assert cases == ["all_methods", "eos_early"]
    for c in cases:
        reqs = json.loads(str(d[f"{c}__requests"]))
        modes = {(r["token_aggregation"], r["head_aggregation"]) for r in reqs if r["method_name"] == "RAUQ"}
        assert len(modes) == 6 and any(r.get("ablation") for r in reqs)
        assert d[f"{c}__samp__hidden"].shape == (5, 1, 32)
        assert d[f"{c}__det__att_0"].shape[0] == 16  # 16 layers
    eos = json.loads(str(d["eos_early__gen_config"]))["eos_token_id"]
    gen = d["eos_early__samp__sequences"][:, -d["eos_early__samp__scores"].shape[0]:]
    ended = (gen == eos).any(axis=1)
    assert ended.any() and not ended.all(), "the eos case must end some samples early"


@pytest.mark.parametrize("case", ["all_methods", "eos_early"])
def test_numpy_restatement_matches_reference_scores(case):
    """perplexity / generation_entropy of the deterministic scores and normalized_entropy of the sampled ones, in
    NumPy f64 from the recorded logits, against the reference's numbers."""
    d = load()
    p = f"{case}__"
    x = d[p + "det__scores"][:, 0, :]
    T = x.shape[0]
    tok = d[p + "det__sequences"][0, -T:]
    lp = log_softmax(x)[np.arange(T), tok]
    assert abs(-lp.mean() - float(d[p + "score__perplexity"])) < 1e-6
    pr = np.exp(log_softmax(x))
    ent = -(pr * np.log(np.maximum(pr, 1e-12))).sum(-1) / np.log(x.shape[-1])
    assert abs(ent.mean() - float(d[p + "score__generation_entropy"])) < 1e-6
    xs = d[p + "samp__scores"]  # (T, K, V)
    toks = d[p + "samp__sequences"][:, -xs.shape[0]:]
    lps = np.take_along_axis(log_softmax(xs).transpose(1, 0, 2), toks[:, :, None], axis=2)[..., 0]
    rows = [r[np.isfinite(r)].mean() for r in lps]
    assert abs(-np.mean(rows) - float(d[p + "score__normalized_entropy"])) < 1e-6
    # eigen_score restated on the recorded hidden states (the reference's own formula, f64)
    e = d[p + "samp__hidden"][:, 0, :].astype(np.float64)
    sv = np.linalg.svd(np.cov(e.T) + 1e-3 * np.eye(e.shape[1]), compute_uv=False)
    assert abs(np.mean(np.log(sv)) - float(d[p + "score__eigen_score"])) < 1e-6


def test_package_exports_the_new_names_outside_scores():
    import runia_core_amd.llm_uncertainty.pipeline as pl
    import runia_core_amd.llm_uncertainty.scores as sc

    for n in ("compute_uncertainties", "compute_uncertainties_batch", "eigen_scores"):
        assert n in L.__all__ and callable(getattr(L, n)) and n in pl.__all__
        assert not hasattr(sc, n)
    assert sc.__all__ == ["eigen_score", "normalized_entropy", "semantic_entropy", "perplexity", "generation_entropy"]


def test_header_and_binding_tables_agree():
    text = open(os.path.join(ROOT, "include", "runia_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(runia_[a-z0-9_]+)\s*\(", text)))
    assert "runia_eigen_score_batch" in syms
    assert sorted(_hip.exported_symbols()) == syms
    src = open(os.path.join(ROOT, "runia_core_amd", "csrc", "Makefile")).read()
    assert "eigen_score.hip" in src


# ---- a stub model that records its generate() calls --------------------------------------------------------------------
class _Tok:
    """Whitespace tokenizer over a fixed vocabulary (ids from 3; pad 0, eos 1)."""

    def __init__(self):
        self.padding_side, self.pad_token, self.eos_token = "right", None, "<eos>"
        self.calls = []

    def __call__(self, text, return_tensors=None, padding=False):
        from transformers import BatchEncoding

        self.calls.append((text, self.padding_side, self.pad_token, padding))
        texts = [text] if isinstance(text, str) else list(text)
        ids = [[3 + (sum(map(ord, w)) % 20) for w in t.split()] for t in texts]
        n = max(len(i) for i in ids)
        rows = [[0] * (n - len(i)) + i for i in ids]
        mask = [[0] * (n - len(i)) + [1] * len(i) for i in ids]
        return BatchEncoding({"input_ids": torch.tensor(rows), "attention_mask": torch.tensor(mask)})

    def batch_decode(self, seqs, skip_special_tokens=True):
        return [" ".join(f"w{int(t)}" for t in row if int(t) > 1) for row in seqs]


def fake_output(rows, in_len, T, V=24, L_=2, H=2, hidden=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(2, V, (rows, in_len + T), generator=g)
    scores = tuple(torch.randn(rows, V, generator=g) for _ in range(T))
    att = []
    for s in range(T):
        q, k = (in_len, in_len) if s == 0 else (1, in_len + s)
        att.append(tuple(torch.softmax(torch.randn(rows, H, q, k, generator=g), -1) for _ in range(L_)))
    hs = tuple(tuple(torch.randn(rows, in_len if s == 0 else 1, hidden, generator=g) for _ in range(17)) for s in range(T))
    return types.SimpleNamespace(sequences=seq, scores=scores, attentions=tuple(att), hidden_states=hs)


class _Model:
    device = torch.device("cpu")

    def __init__(self, T=4):
        self.calls, self.T = [], T
        self.generation_config = types.SimpleNamespace(eos_token_id=None)

    def generate(self, **kw):
        self.calls.append(kw)
        rows = kw["input_ids"].shape[0] * kw.get("num_return_sequences", 1)
        return fake_output(rows, kw["input_ids"].shape[1], self.T, seed=len(self.calls))


def _run(fn, *a, **k):
    """The call on this host: it runs to the end on a GPU host and raises RuniaHipError at the first device score
    without one; the generate() calls are made either way."""
    try:
        return fn(*a, **k)
    except _hip.RuniaHipError:
        return None


DET_KW = {"generation_config", "output_attentions", "output_hidden_states", "output_scores", "return_dict_in_generate",
          "tokenizer", "input_ids", "attention_mask"}
SAMP_KW = {"do_sample", "temperature", "num_return_sequences", "generation_config", "output_attentions",
           "output_hidden_states", "output_scores", "return_dict_in_generate", "input_ids", "attention_mask"}


@pytest.mark.parametrize("fn", ["compute_uncertainties", "compute_uncertainties_batch"])
def test_sampled_generate_only_when_a_request_needs_it(fn):
    f = getattr(L, fn)
    prompt = "the cat sat" if fn == "compute_uncertainties" else ["the cat sat", "a dog"]
    cfg = object()
    for reqs, sampled in (([{"method_name": "perplexity"}, {"method_name": "generation_entropy"}], False),
                          ([{"method_name": "RAUQ", "token_aggregation": "original", "head_aggregation": "mean_heads"}], False),
                          ([{"method_name": "perplexity"}, {"method_name": "eigen_score"}], True),
                          ([{"method_name": "normalized_entropy"}], True)):
        m, tok = _Model(), _Tok()
        _run(f, m, tok, prompt, reqs, cfg, 3)
        assert len(m.calls) == (2 if sampled else 1), reqs
        det = m.calls[0]
        assert set(det) == DET_KW and det["generation_config"] is cfg and det["tokenizer"] is tok
        assert all(det[k] is True for k in ("output_attentions", "output_hidden_states", "output_scores",
                                            "return_dict_in_generate"))
        if sampled:
            s = m.calls[1]
            assert set(s) == SAMP_KW and s["generation_config"] is cfg
            assert s["do_sample"] is True and s["temperature"] == 1.0 and s["num_return_sequences"] == 3
            assert torch.equal(s["input_ids"], det["input_ids"])


def test_batch_tokenizes_left_padded_and_restores_the_tokenizer():
    m, tok = _Model(), _Tok()
    _run(L.compute_uncertainties_batch, m, tok, ["a b c d", "e"], [{"method_name": "perplexity"}])
    assert tok.calls == [(["a b c d", "e"], "left", "<eos>", True)]
    assert tok.padding_side == "right" and tok.pad_token is None
    ids = m.calls[0]["input_ids"]
    assert ids.shape == (2, 4) and m.calls[0]["attention_mask"].tolist() == [[1, 1, 1, 1], [0, 0, 0, 1]]


def test_unknown_method_and_incomplete_rauq_raise_key_error_before_generating():
    for reqs in ([{"method_name": "entropy"}], [{"method_name": "RAUQ", "head_aggregation": "rollout"}],
                 [{"method_name": "RAUQ", "token_aggregation": "original"}], [{"alphas": [0.2]}]):
        for f, prompt in ((L.compute_uncertainties, "a b"), (L.compute_uncertainties_batch, ["a b"])):
            m = _Model()
            with pytest.raises(KeyError):
                f(m, _Tok(), prompt, reqs)
            assert m.calls == []


def test_key_names_follow_the_reference():
    from runia_core_amd.llm_uncertainty.pipeline import _score_name

    assert _score_name({"method_name": "RAUQ", "token_aggregation": "original", "head_aggregation": "rollout"}) == \
        "RAUQ_original_rollout"
    assert _score_name({"method_name": "RAUQ", "token_aggregation": 1, "head_aggregation": None}) == "RAUQ_1_None"
    for m in ("eigen_score", "normalized_entropy", "semantic_entropy", "perplexity", "generation_entropy"):
        assert _score_name({"method_name": m, "token_aggregation": "x"}) == m


def test_semantic_entropy_only_runs_on_the_host_with_given_entailment():
    """semantic_entropy is the host function: with an NLI model given, the call needs no device."""

    class NLI:
        device = torch.device("cpu")

        def __call__(self, input_ids=None, **kw):
            return types.SimpleNamespace(logits=torch.tensor([[0.0, 0.0, 1.0]]).repeat(input_ids.shape[0], 1))

    class PairTok:
        def __call__(self, a, b, return_tensors=None, padding=False):
            return {"input_ids": torch.zeros(len(a), 3, dtype=torch.int64)}

    m = _Model()
    text, scores = L.compute_uncertainties(m, _Tok(), "a b", [{"method_name": "semantic_entropy"}], num_samples=4,
                                           entailment=(NLI(), PairTok()))
    assert isinstance(text, list) and len(text) == 1 and scores["semantic_entropy"] == 0.0
    assert set(scores) == {"semantic_entropy", "clusters"} and set(scores["clusters"].values()) == {0}
    texts, bs = L.compute_uncertainties_batch(_Model(), _Tok(), ["a b", "c"], [{"method_name": "semantic_entropy"}],
                                              num_samples=3, entailment=(NLI(), PairTok()))
    assert len(texts) == 2 and bs["semantic_entropy"].dtype == torch.float64 and bs["semantic_entropy"].tolist() == [0.0, 0.0]
    assert isinstance(bs["clusters"], list) and len(bs["clusters"]) == 2


def test_eigen_scores_validates_shapes_before_the_device():
    hs = ((torch.zeros(6, 2, 4),) * 16,)
    with pytest.raises(ValueError):
        L.eigen_scores(hs, 3)
    hs = ((torch.zeros(6, 1, 4),) * 16,)
    with pytest.raises(ValueError):
        L.eigen_scores(hs, 4)  # 6 rows, groups of 4
    with pytest.raises(ValueError):
        L.eigen_scores(hs, 1)
    with pytest.raises(ValueError):
        L.eigen_scores(((torch.zeros(6, 4),) * 16,), 3)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_eigen_scores_needs_a_gpu():
    with pytest.raises(_hip.RuniaHipError):
        L.eigen_scores(((torch.randn(6, 1, 4),) * 16,), 3)
    with pytest.raises(_hip.RuniaHipError):
        L.eigen_scores(((torch.randn(1, 6, 4),) * 16,), 2)
