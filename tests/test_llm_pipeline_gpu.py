"""eigen_scores (one launch of runia_eigen_score_batch), compute_uncertainties and compute_uncertainties_batch on the
device: against eigen_score and the f64 definition, on the replayed generations of the reference's own
compute_uncertainties (tests/golden/ref_llm_pipeline.npz), and against the one-prompt functions on real tiny-Llama
generations."""
from __future__ import annotations

import json
import math
import os
import types

import numpy as np
import pytest
import torch

from runia_core_amd.llm_uncertainty import (RAUQ, compute_uncertainties, compute_uncertainties_batch, eigen_score,
                                            eigen_scores, generated_lengths, generation_scores, rauq_batch)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_llm_pipeline.npz")


def hs_of(e2d):
    """hidden_states whose [-1][15] is e2d viewed as (N, 1, H)."""
    return ((e2d[:, None, :],) * 16,)


def one(e2d, alpha=1e-3):
    return eigen_score(((e2d[None],) * 16,), alpha)


# ---- eigen_scores ---------------------------------------------------------------------------------------------------------
def test_eigen_scores_reference_mock():
    """unit_test_llm_uncertainty.py:69-92: (1, 10, 768) hidden states, golden -6.775187082486514."""
    np.random.seed(42)
    torch.manual_seed(42)
    hs = tuple(tuple(torch.randn(1, 10, 768) for _ in range(20)) for _ in range(5))
    s = eigen_scores(hs, 10, alpha=1e-3)
    assert s.shape == (1,) and s.dtype == torch.float64 and not s.is_cuda
    assert abs(float(s[0]) - (-6.775187082486514)) < 1e-6


@pytest.mark.parametrize("k", [2, 5, 10, 32, 64])
@pytest.mark.parametrize("hidden", [32, 768, 4096])
def test_eigen_scores_equal_eigen_score_per_group(k, hidden):
    g = torch.Generator().manual_seed(k * 7919 + hidden)
    G = 3
    e = torch.randn(G * k, hidden, generator=g) * (0.5 + torch.rand(hidden, generator=g))
    want = [one(e[i * k:(i + 1) * k]) for i in range(G)]
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x = e.to(dt)
        want_dt = want if dt == torch.float32 else [one(x[i * k:(i + 1) * k].float()) for i in range(G)]
        for src in (x, x.cuda()):
            got = eigen_scores(hs_of(src), k)
            assert got.is_cuda == src.is_cuda
            got = got.cpu()
            for i in range(G):
                assert abs(float(got[i]) - want_dt[i]) <= 1e-10, (k, hidden, dt, src.is_cuda, i)


def test_eigen_scores_strided_rows_and_k_above_hidden():
    g = torch.Generator().manual_seed(5)
    base = torch.randn(4 * 40, 2 * 96, generator=g).cuda()
    view = base[:, 7:7 + 32]  # row stride 192, k = 40 > hidden = 32
    assert view.stride() == (192, 1)
    got = eigen_scores(hs_of(view), 40).cpu()
    for i in range(4):
        assert abs(float(got[i]) - one(view[i * 40:(i + 1) * 40].cpu())) <= 1e-10
    bf = torch.randn(2 * 10, 3 * 768, generator=g).bfloat16().cuda()[:, ::3]  # column stride 3: made contiguous
    got = eigen_scores(hs_of(bf), 10).cpu()
    for i in range(2):
        assert abs(float(got[i]) - one(bf[i * 10:(i + 1) * 10].float().cpu())) <= 1e-10
    rows = torch.randn(3 * 5, 2, 64, generator=g).cuda()[:, 1, :]  # (1, N, H) layout through the (N, H) view
    got = eigen_scores(((rows[None],) * 16,), 5).cpu()
    for i in range(3):
        assert abs(float(got[i]) - one(rows[i * 5:(i + 1) * 5].cpu())) <= 1e-10


def test_eigen_scores_llama_width_against_f64_definition():
    torch.manual_seed(7)
    e = torch.randn(10, 4096) * (0.5 + torch.rand(4096))
    for alpha in (1e-3, 1e-2):
        got = float(eigen_scores(hs_of(e.cuda()), 10, alpha)[0])
        x = e.double().numpy()
        sv = np.linalg.svd(np.cov(x.T) + alpha * np.eye(4096), compute_uv=False)
        assert abs(got - float(np.mean(np.log(sv)))) < 2e-6


def test_eigen_scores_group_bits_do_not_depend_on_the_batch():
    g = torch.Generator().manual_seed(11)
    k = 10
    e = (torch.randn(256 * k, 768, generator=g)).bfloat16().cuda()
    all_ = eigen_scores(hs_of(e), k)
    for i in (0, 1, 77, 255):
        alone = eigen_scores(hs_of(e[i * k:(i + 1) * k]), k)
        assert torch.equal(alone, all_[i:i + 1]), i
    assert torch.equal(eigen_scores(hs_of(e), k), all_)


def test_eigen_scores_degenerate_and_limits():
    row = torch.randn(1, 64)
    same = row.expand(6, 64).contiguous()
    assert abs(float(eigen_scores(hs_of(same.cuda()), 6, 1e-3)[0]) - math.log(1e-3)) < 1e-12
    e = torch.randn(2 * 65, 48)
    got = eigen_scores(hs_of(e), 65)  # beyond the kernel's 64: the eigen_score path per group
    for i in range(2):
        assert float(got[i]) == one(e[i * 65:(i + 1) * 65])
    with pytest.raises(ValueError):
        eigen_scores(hs_of(torch.randn(4, 8).cuda()), 1)
    from runia_core_amd import _hip

    with pytest.raises(ValueError):
        _hip.eigen_scores(torch.randn(65, 8).cuda(), 65)


# ---- replay of the reference's generations -------------------------------------------------------------------------------
def fixture():
    return np.load(FIXTURE, allow_pickle=False)


def make_tokenizer(words):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    tk = Tokenizer(models.WordLevel({w: i for i, w in enumerate(words)}, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tk.decoder = decoders.WordPiece(prefix="##", cleanup=False)
    return PreTrainedTokenizerFast(tokenizer_object=tk, pad_token="<pad>", eos_token="<eos>", unk_token="<unk>")


def make_nli(d):
    from transformers import BertConfig, BertForSequenceClassification

    cfg = BertConfig.from_dict(json.loads(str(d["nli__config"])))
    model = BertForSequenceClassification(cfg).eval()
    state = {k[len("nli__w__"):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("nli__w__")}
    model.load_state_dict(state)
    return model


def replay_output(d, p, which):
    """The recorded generate() output on the GPU (hidden states: only [-1][15] is read)."""
    seq = torch.from_numpy(d[p + which + "__sequences"]).cuda()
    scores = tuple(s.cuda() for s in torch.from_numpy(d[p + which + "__scores"]))
    out = types.SimpleNamespace(sequences=seq, scores=scores)
    if which == "det":
        n = scores.__len__()
        out.attentions = tuple(tuple(torch.from_numpy(d[p + f"det__att_{g}"]).cuda().unbind(0)) for g in range(n))
    else:
        h = torch.from_numpy(d[p + "samp__hidden"]).cuda()
        out.hidden_states = ((None,) * 15 + (h,),)
    return out


class ReplayModel:
    device = torch.device("cuda")

    def __init__(self, det, samp, eos=None):
        self.det, self.samp, self.calls = det, samp, []
        self.generation_config = types.SimpleNamespace(eos_token_id=eos)

    def generate(self, **kw):
        self.calls.append(kw)
        return self.samp if kw.get("do_sample") else self.det


@pytest.mark.parametrize("case", ["all_methods", "eos_early"])
def test_compute_uncertainties_replays_the_reference(case):
    from transformers import GenerationConfig

    d = fixture()
    p = f"{case}__"
    tok = make_tokenizer([str(w) for w in d["vocab"]])
    assert tok(str(d[p + "prompt"]), return_tensors="pt")["input_ids"].tolist() == d[p + "input_ids"].tolist()
    reqs = json.loads(str(d[p + "requests"]))
    cfg = GenerationConfig(**json.loads(str(d[p + "gen_config"])))
    model = ReplayModel(replay_output(d, p, "det"), replay_output(d, p, "samp"))
    text, scores = compute_uncertainties(model, tok, str(d[p + "prompt"]), reqs, cfg, int(d[p + "num_samples"]),
                                         entailment=(make_nli(d), tok))
    assert len(model.calls) == 2
    assert text == [str(t) for t in d[p + "text"]]
    keys = {k[len(p + "score__"):] for k in d.files if k.startswith(p + "score__")}
    assert set(scores) == keys | {"clusters"}
    assert scores["clusters"] == dict(zip([str(t) for t in d[p + "clusters_text"]], d[p + "clusters_id"].tolist()))
    assert scores["semantic_entropy"] == float(d[p + "score__semantic_entropy"])
    for k in ("perplexity", "generation_entropy", "normalized_entropy", "eigen_score"):
        assert isinstance(scores[k], float) and abs(scores[k] - float(d[p + "score__" + k])) < 1e-6, k
    for r in reqs:
        if r["method_name"] != "RAUQ":
            continue
        key = f"RAUQ_{r['token_aggregation']}_{r['head_aggregation']}"
        want = d[p + "score__" + key]
        got = np.asarray(scores[key], dtype=np.float64)
        assert isinstance(scores[key], list) == bool(r.get("ablation")), key
        tol = 1e-5 if r["head_aggregation"] == "rollout" else 1e-6
        assert np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))), (key, got, want)


# ---- real tiny Llama on the GPU ----------------------------------------------------------------------------------------------
def tiny_llama(eos, seed=23, vocab=48):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(seed)
    cfg = transformers.LlamaConfig(vocab_size=vocab, hidden_size=32, intermediate_size=64, num_hidden_layers=16,
                                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256,
                                   attn_implementation="eager", pad_token_id=0, eos_token_id=eos, bos_token_id=None)
    model = transformers.LlamaForCausalLM(cfg).cuda().eval()
    with torch.no_grad():
        model.lm_head.weight.mul_(10.0)
    return model


class RecordingModel:
    """A real model whose generate() outputs are kept (they are the inputs the one-prompt functions are compared on)."""

    def __init__(self, model):
        self.model, self.outs = model, []
        self.device = model.device
        self.generation_config = model.generation_config

    def generate(self, **kw):
        with torch.no_grad():
            out = self.model.generate(**kw)
        self.outs.append(out)
        return out


class IdTok:
    """Prompts are space-separated token ids; decode prints ids (eos 1 and pad 0 are special)."""

    padding_side, pad_token, eos_token = "right", None, "<eos>"

    def __call__(self, text, return_tensors=None, padding=False):
        from transformers import BatchEncoding

        texts = [text] if isinstance(text, str) else list(text)
        ids = [[int(w) for w in t.split()] for t in texts]
        n = max(len(i) for i in ids)
        left = self.padding_side == "left"
        rows = [([0] * (n - len(i)) + i) if left else (i + [0] * (n - len(i))) for i in ids]
        mask = [([0] * (n - len(i)) + [1] * len(i)) if left else ([1] * len(i) + [0] * (n - len(i))) for i in ids]
        return BatchEncoding({"input_ids": torch.tensor(rows), "attention_mask": torch.tensor(mask)})

    def batch_decode(self, seqs, skip_special_tokens=True):
        return [" ".join(str(int(t)) for t in row if int(t) > 1) for row in seqs]


ALL_REQS = ([{"method_name": m} for m in ("perplexity", "generation_entropy", "normalized_entropy", "eigen_score")] +
            [{"method_name": "RAUQ", "token_aggregation": t, "head_aggregation": h, "alphas": [0.2, 0.6], "ablation": True}
             for h in ("original", "mean_heads", "rollout") for t in ("original", "mean_all_tokens")])


def test_compute_uncertainties_real_llama_equals_the_score_functions():
    from transformers import GenerationConfig

    model = RecordingModel(tiny_llama(eos=None))
    cfg = GenerationConfig(max_new_tokens=7, pad_token_id=0)
    torch.manual_seed(3)
    text, scores = compute_uncertainties(model, IdTok(), "5 9 14 3 22 31", ALL_REQS, cfg, 6)
    det, samp = model.outs
    in_len = 6
    gs = generation_scores(det.sequences, det.scores)
    assert scores["perplexity"] == float(gs.perplexity[0])
    assert scores["generation_entropy"] == float(gs.generation_entropy[0])
    assert scores["normalized_entropy"] == generation_scores(samp.sequences, samp.scores).normalized_entropy
    assert scores["eigen_score"] == float(eigen_scores(samp.hidden_states, 6)[0])
    assert abs(scores["eigen_score"] - eigen_score(samp.hidden_states)) <= 1e-10
    for r in ALL_REQS[4:]:
        key = f"RAUQ_{r['token_aggregation']}_{r['head_aggregation']}"
        assert scores[key] == RAUQ(gs.log_probs, det.attentions, in_len, r["token_aggregation"], r["head_aggregation"],
                                   r["alphas"], True)
    assert text == IdTok().batch_decode(det.sequences[:, in_len:])


PROMPTS = ["5 9 14 3 22 31 7 12", "17 4", "8 8 30 2 11", "40 21 6 9 13 27", "33"]


def _slice_output(out, rows, steps):
    return types.SimpleNamespace(sequences=out.sequences[rows], scores=tuple(s[rows] for s in out.scores[:steps]))


def test_compute_uncertainties_batch_equals_the_one_prompt_functions():
    from transformers import GenerationConfig

    eos = [5, 6, 7]
    model = RecordingModel(tiny_llama(eos=eos, seed=29))
    cfg = GenerationConfig(max_new_tokens=10, pad_token_id=0, eos_token_id=eos)
    torch.manual_seed(4)
    K, B = 4, len(PROMPTS)
    texts, scores = compute_uncertainties_batch(model, IdTok(), PROMPTS, ALL_REQS, cfg, K)
    det, samp = model.outs
    in_len = int(det.sequences.shape[1] - len(det.scores))
    assert det.sequences.shape[0] == B and samp.sequences.shape[0] == B * K
    lengths = generated_lengths(det.sequences, in_len, eos)
    assert (lengths < len(det.scores)).any(), "eos must end some deterministic rows early"
    mask = IdTok()
    mask.padding_side = "left"
    am = mask(PROMPTS)["attention_mask"].cuda()
    lp_all = generation_scores(det.sequences, det.scores).log_probs
    for b in range(B):
        n = int(lengths[b])
        one_det = generation_scores(det.sequences[b:b + 1, :in_len + n], tuple(s[b:b + 1] for s in det.scores[:n]))
        assert abs(float(scores["perplexity"][b]) - float(one_det.perplexity[0])) <= 1e-12
        assert abs(float(scores["generation_entropy"][b]) - float(one_det.generation_entropy[0])) <= 1e-12
        rows = slice(b * K, (b + 1) * K)
        one_s = generation_scores(samp.sequences[rows], tuple(s[rows] for s in samp.scores))
        assert abs(float(scores["normalized_entropy"][b]) - one_s.normalized_entropy) <= 1e-12
        hs = ((None,) * 15 + (samp.hidden_states[-1][15][rows],),)
        assert float(scores["eigen_score"][b]) == float(eigen_scores((hs[0],), K)[0])
    for r in ALL_REQS[4:]:
        key = f"RAUQ_{r['token_aggregation']}_{r['head_aggregation']}"
        want = rauq_batch(lp_all, det.attentions, in_len, r["token_aggregation"], r["head_aggregation"], r["alphas"], am,
                          lengths).double().cpu()
        got = scores[key]
        assert got.shape == (B, 2) and bool(((got == want) | (got.isnan() & want.isnan())).all()), key
    assert all(s.dtype == torch.float64 and not s.is_cuda for k, s in scores.items())
    assert texts == IdTok().batch_decode(det.sequences[:, in_len:])


def test_batch_of_one_equals_compute_uncertainties_on_the_same_generation():
    d = fixture()
    p = "eos_early__"
    from transformers import GenerationConfig

    tok = make_tokenizer([str(w) for w in d["vocab"]])
    reqs = json.loads(str(d[p + "requests"]))
    cfg = GenerationConfig(**json.loads(str(d[p + "gen_config"])))
    nli = (make_nli(d), tok)
    prompt = str(d[p + "prompt"])
    m1 = ReplayModel(replay_output(d, p, "det"), replay_output(d, p, "samp"))
    _, one_ = compute_uncertainties(m1, tok, prompt, reqs, cfg, 5, entailment=nli)
    m2 = ReplayModel(replay_output(d, p, "det"), replay_output(d, p, "samp"))
    texts, bat = compute_uncertainties_batch(m2, tok, [prompt], reqs, cfg, 5, entailment=nli)
    assert texts == [str(t) for t in d[p + "text"]]
    assert bat["clusters"] == [one_["clusters"]]
    for k, v in one_.items():
        if k == "clusters":
            continue
        got = bat[k][0]
        want = torch.tensor(v, dtype=torch.float64)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), (k, got, want)
