"""``compute_uncertainties``: generate and score in one call, with the reference's signature, defaults, keys and return
types (``runia_core/llm_uncertainty/scores.py:347-524``), and its batched form for many prompts.

The reference makes two ``generate()`` calls - a deterministic one, and a sampled one with ``num_return_sequences =
num_samples`` only when a request needs samples - then scores them with host-style torch.  Here the same two calls are
made with the same keyword arguments and every score comes from this package's device code:

- ``perplexity``, ``generation_entropy``: ``generation_scores`` of the deterministic output (one pass over its logits);
- ``RAUQ``: the deterministic log-probs of that pass and the attention maps, read in place (``RAUQ`` / ``rauq_batch``);
- ``normalized_entropy``: ``generation_scores`` of the sampled output;
- ``eigen_score``: ``eigen_scores`` (one launch of ``runia_eigen_score_batch`` for every prompt's sample group);
- ``semantic_entropy``: the host function of ``.scores`` with the NLI model (its forward passes are the cost);
- ``lexical_similarity``, ``deg``, ``ecc``, ``eigv``, ``num_sets``: the sample-consistency scores of ``.consistency`` from the
  sampled ids alone (one ``runia_cons_pairs`` call and one ``runia_cons_graph`` launch per call, shared by the requests).

``model.compute_transition_scores`` is not called.  ``entailment=(nli_model, nli_tokenizer)`` is this package's
addition: without it a ``semantic_entropy`` request loads ``microsoft/deberta-v2-xxlarge-mnli`` by name, as the
reference does.  Without a GPU the device scores raise ``RuniaHipError``: there is no host fallback.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from .. import _hip
from .consistency import SIMILARITIES, scores_by_kind
from .logits import generation_scores
from .rauq import RAUQ, generated_lengths, rauq_batch
from .scores import eigen_score, semantic_entropy

__all__ = ["eigen_scores", "compute_uncertainties", "compute_uncertainties_batch"]

_NEEDS_SAMPLING = {"eigen_score": True, "normalized_entropy": True, "semantic_entropy": True, "perplexity": False,
                   "generation_entropy": False, "RAUQ": False, "lexical_similarity": True, "deg": True, "ecc": True,
                   "eigv": True, "num_sets": True}
# request name -> field of ConsistencyScores
_CONSISTENCY = {"lexical_similarity": "lexical_similarity", "deg": "u_deg", "ecc": "u_ecc", "eigv": "u_eigv",
                "num_sets": "num_sets"}
_NLI_MODEL = "microsoft/deberta-v2-xxlarge-mnli"


def eigen_scores(hidden_states, num_samples: int, alpha: float = 1e-3, token_index: int = -1,
                 layer_index: int = 15) -> torch.Tensor:
    """``(G,)`` f64 eigen scores, one per group of ``num_samples`` consecutive rows of
    ``hidden_states[token_index][layer_index]`` (HF ``generate(num_return_sequences=num_samples)`` on G prompts: rows are
    prompt-major).  ``(N, 1, H)`` and ``(1, N, H)`` are both read as ``(N, H)``, as the reference's ``.squeeze()`` leaves
    them; f32, f16 or bf16, host or one GPU, read in place.  Group g is ``eigen_score`` of rows ``g*k .. g*k+k-1``; all
    groups go through one kernel launch.  Groups of more than 64 samples (beyond the kernel's LDS budget) take the
    ``eigen_score`` path, one group at a time.  The result lies where the hidden states do."""
    e = hidden_states[token_index][layer_index]
    if not isinstance(e, torch.Tensor) or e.dim() != 3 or (e.shape[1] != 1 and e.shape[0] != 1):
        shape = tuple(e.shape) if isinstance(e, torch.Tensor) else type(e).__name__
        raise ValueError(f"hidden states of one token must be (N, 1, H) or (1, N, H), got {shape}")
    e2 = e[:, 0, :] if e.shape[1] == 1 else e[0]
    k = int(num_samples)
    n = int(e2.shape[0])
    if k < 2:
        raise ValueError(f"eigen_score needs at least two samples per group, got num_samples={num_samples}")
    if n == 0 or n % k:
        raise ValueError(f"{n} rows do not form groups of num_samples={k}")
    if k <= _hip.EIGEN_SCORE_MAX_K:
        return _hip.eigen_scores(e2, k, alpha)
    vals = [eigen_score(((e2[g * k:(g + 1) * k].unsqueeze(0),) * 16,), alpha) for g in range(n // k)]
    return torch.tensor(vals, dtype=torch.float64, device=e2.device)


def _score_name(req: Dict[str, Any]) -> str:
    """The reference's result key (KeyError for an unknown method or a RAUQ request without its two aggregations)."""
    method = req["method_name"]
    if method not in _NEEDS_SAMPLING:
        raise KeyError(method)
    if method == "RAUQ":
        return f"RAUQ_{req['token_aggregation']}_{req['head_aggregation']}"
    if method in _CONSISTENCY:
        similarity = req.get("similarity", SIMILARITIES[0])
        if similarity not in SIMILARITIES:
            raise KeyError(similarity)
        return method if similarity == SIMILARITIES[0] else f"{method}_{similarity}"
    return method


def _consistency(requests, samp, input_length: int, num_samples: int, eos):
    """``{similarity: ConsistencyScores}`` of the sampled rows for every similarity the requests name: one count call and
    one graph launch, whatever the number of requests."""
    kinds = [req.get("similarity", SIMILARITIES[0]) for req in requests if req["method_name"] in _CONSISTENCY]
    return scores_by_kind(samp.sequences[:, input_length:], num_samples, kinds, eos_token_id=eos)


def _entailment_models(entailment, requests):
    if not any(req["method_name"] == "semantic_entropy" for req in requests):
        return None, None
    if entailment is not None:
        return entailment
    from transformers import AutoModelForSequenceClassification, AutoTokenizer

    return (AutoModelForSequenceClassification.from_pretrained(_NLI_MODEL, device_map="auto"),
            AutoTokenizer.from_pretrained(_NLI_MODEL))


def _generate(model, tokenizer, inputs, gen_config, num_samples: int, sample: bool):
    """The reference's two ``generate()`` calls, keyword for keyword."""
    if not sample:
        return model.generate(**inputs, generation_config=gen_config, output_attentions=True, output_hidden_states=True,
                              output_scores=True, return_dict_in_generate=True, tokenizer=tokenizer)
    return model.generate(**inputs, do_sample=True, temperature=1.0, num_return_sequences=num_samples,
                          generation_config=gen_config, output_attentions=True, output_hidden_states=True,
                          output_scores=True, return_dict_in_generate=True)


def _rauq_args(req):
    return (req.get("token_aggregation", "mean_all_tokens"), req.get("head_aggregation", "rollout"),
            req.get("alphas", [0.3]), req.get("ablation", False))


def compute_uncertainties(model, tokenizer, prompt: str, uncertainty_requests: List[Dict[str, Any]], gen_config=None,
                          num_samples: int = 5, *, entailment: Optional[Tuple[Any, Any]] = None
                          ) -> Tuple[List[str], Dict[str, Any]]:
    """Generate for ``prompt`` and compute the requested uncertainty scores (reference ``compute_uncertainties``).

    ``uncertainty_requests``: dicts with ``method_name`` in eigen_score, normalized_entropy, semantic_entropy, perplexity,
    generation_entropy, RAUQ, lexical_similarity, deg, ecc, eigv, num_sets (the last five: sample consistency of the sampled
    ids, ``.consistency``; an optional ``"similarity"`` of ``"rouge_l"`` (default) or ``"jaccard"``, which is appended to the
    key when it is not the default; ``num_sets`` is an int); a RAUQ request also names ``token_aggregation`` and
    ``head_aggregation`` and may give ``alphas`` (default [0.3]) and ``ablation`` (default False).  Returns ``(deterministic_text, scores)``: the text as
    the reference returns it (a list of one string) and ``{key: score}`` with keys ``method_name`` or
    ``RAUQ_<token_aggregation>_<head_aggregation>``, Python floats (a list for RAUQ with ``ablation=True``), plus
    ``"clusters"`` = ``{text: cluster}`` when semantic entropy is requested.  ``entailment``: the NLI ``(model,
    tokenizer)`` for semantic entropy (default: ``microsoft/deberta-v2-xxlarge-mnli`` by name)."""
    names = [_score_name(req) for req in uncertainty_requests]
    inputs = tokenizer(prompt, return_tensors="pt").to(model.device)
    input_length = int(inputs["input_ids"].shape[1])
    nli_model, nli_tokenizer = _entailment_models(entailment, uncertainty_requests)

    det = _generate(model, tokenizer, inputs, gen_config, num_samples, sample=False)
    deterministic_text = tokenizer.batch_decode(det.sequences[:, input_length:], skip_special_tokens=True)
    samp, sampled_texts = None, None
    if any(_NEEDS_SAMPLING[req["method_name"]] for req in uncertainty_requests):
        samp = _generate(model, tokenizer, inputs, gen_config, num_samples, sample=True)
        sampled_texts = tokenizer.batch_decode(samp.sequences[:, input_length:], skip_special_tokens=True)

    cache: Dict[str, Any] = {}

    def det_scores():
        if "det" not in cache:
            cache["det"] = generation_scores(det.sequences, det.scores)
        return cache["det"]

    scores: Dict[str, Any] = {}
    for name, req in zip(names, uncertainty_requests):
        method = req["method_name"]
        if method == "perplexity":
            scores[name] = float(det_scores().perplexity[0])
        elif method == "generation_entropy":
            scores[name] = float(det_scores().generation_entropy[0])
        elif method == "RAUQ":
            tok, head, alphas, ablation = _rauq_args(req)
            scores[name] = RAUQ(det_scores().log_probs, det.attentions, input_length, tok, head, alphas, ablation)
        elif method == "normalized_entropy":
            scores[name] = generation_scores(samp.sequences, samp.scores).normalized_entropy
        elif method == "eigen_score":
            scores[name] = float(eigen_scores(samp.hidden_states, num_samples)[0])
        elif method in _CONSISTENCY:
            if "cons" not in cache:
                cache["cons"] = _consistency(uncertainty_requests, samp, input_length, num_samples,
                                             _eos_ids(model, gen_config))
            value = getattr(cache["cons"][req.get("similarity", SIMILARITIES[0])], _CONSISTENCY[method])[0]
            scores[name] = int(value) if method == "num_sets" else float(value)
        else:  # semantic_entropy
            entropy, clusters = semantic_entropy(nli_model, nli_tokenizer, sampled_texts)
            scores["clusters"] = {sampled_texts[i]: c for c, members in clusters.items() for i in members}
            scores[name] = float(entropy)
    return deterministic_text, scores


def _eos_ids(model, gen_config):
    for cfg in (gen_config, getattr(model, "generation_config", None)):
        eos = getattr(cfg, "eos_token_id", None) if cfg is not None else None
        if eos is not None:
            return [int(eos)] if isinstance(eos, int) else [int(v) for v in eos]
    return None


def _masked_mean(values: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """(B,) f64 mean of every row's first lengths[b] values, on the values' device."""
    steps = torch.arange(values.shape[1], device=values.device)
    keep = steps[None, :] < lengths.to(values.device)[:, None]
    total = torch.where(keep, values.double(), torch.zeros((), dtype=torch.float64, device=values.device)).sum(dim=1)
    return total / lengths.to(device=values.device, dtype=torch.float64)


def compute_uncertainties_batch(model, tokenizer, prompts: Sequence[str], uncertainty_requests: List[Dict[str, Any]],
                                gen_config=None, num_samples: int = 5, *, entailment: Optional[Tuple[Any, Any]] = None
                                ) -> Tuple[List[str], Dict[str, Any]]:
    """``compute_uncertainties`` for B prompts with one deterministic and one sampled ``generate()`` (B * num_samples
    rows) on the left-padded batch.  Returns ``(texts, scores)``: B deterministic texts, ``(B,)`` f64 host tensors
    (``(B, n_alpha)`` for RAUQ with ``ablation=True``) and ``"clusters"`` as a list of B ``{text: cluster}`` dicts.

    Prompt b's numbers are the one-prompt functions applied to prompt b's slices of the two generations: the
    deterministic row b cut at its ``generated_lengths`` (through the first eos of ``gen_config`` or
    ``model.generation_config``; every step without one) for perplexity, generation entropy (masked means on the device)
    and RAUQ (``rauq_batch`` with the attention mask), and sample rows ``b*K .. b*K+K-1`` for normalized entropy, eigen
    score (one ``eigen_scores`` call for all prompts), semantic entropy and the sample-consistency scores (one count call and
    one graph launch for all prompts; ``num_sets`` comes back as int64).  A batch is not promised to equal B separate
    ``compute_uncertainties`` calls: left padding changes what the model generates."""
    prompts = list(prompts)
    if not prompts or not all(isinstance(p, str) for p in prompts):
        raise ValueError("prompts must be a non-empty sequence of strings")
    names = [_score_name(req) for req in uncertainty_requests]
    B, K = len(prompts), int(num_samples)
    side, pad = tokenizer.padding_side, tokenizer.pad_token
    try:
        tokenizer.padding_side = "left"
        if pad is None:
            tokenizer.pad_token = tokenizer.eos_token
        inputs = tokenizer(prompts, return_tensors="pt", padding=True).to(model.device)
    finally:
        tokenizer.padding_side = side
        if pad is None:
            tokenizer.pad_token = pad
    input_length = int(inputs["input_ids"].shape[1])
    nli_model, nli_tokenizer = _entailment_models(entailment, uncertainty_requests)

    det = _generate(model, tokenizer, inputs, gen_config, K, sample=False)
    texts = tokenizer.batch_decode(det.sequences[:, input_length:], skip_special_tokens=True)
    samp, sampled_texts = None, None
    if any(_NEEDS_SAMPLING[req["method_name"]] for req in uncertainty_requests):
        samp = _generate(model, tokenizer, inputs, gen_config, K, sample=True)
        sampled_texts = tokenizer.batch_decode(samp.sequences[:, input_length:], skip_special_tokens=True)

    cache: Dict[str, Any] = {}

    def det_scores():
        if "det" not in cache:
            gs = generation_scores(det.sequences, det.scores)
            eos = _eos_ids(model, gen_config)
            T = len(det.scores)
            lengths = (generated_lengths(det.sequences, input_length, eos) if eos is not None
                       else torch.full((B,), T, dtype=torch.int64))
            cache["det"] = (gs, lengths.clamp_max(T))
        return cache["det"]

    def samp_scores():
        if "samp" not in cache:
            cache["samp"] = generation_scores(samp.sequences, samp.scores)
        return cache["samp"]

    scores: Dict[str, Any] = {}
    for name, req in zip(names, uncertainty_requests):
        method = req["method_name"]
        if method == "perplexity":
            gs, lengths = det_scores()
            scores[name] = (-_masked_mean(gs.log_probs, lengths)).cpu()
        elif method == "generation_entropy":
            gs, lengths = det_scores()
            scores[name] = _masked_mean(gs.token_entropy, lengths).cpu()
        elif method == "RAUQ":
            tok, head, alphas, ablation = _rauq_args(req)
            gs, lengths = det_scores()
            r = rauq_batch(gs.log_probs, det.attentions, input_length, tok, head, alphas, inputs["attention_mask"],
                           lengths).double().cpu()
            scores[name] = r if ablation else r[:, 0]
        elif method == "normalized_entropy":
            # per sample row the mean of its finite log-probs (-inf = padding), then -mean over the prompt's K rows
            lp = samp_scores().log_probs
            finite = lp != -float("inf")
            zero = torch.zeros((), dtype=torch.float64, device=lp.device)
            rows = torch.where(finite, lp.double(), zero).sum(dim=1) / finite.sum(dim=1).double()
            scores[name] = (-rows.view(B, K).mean(dim=1)).cpu()
        elif method == "eigen_score":
            scores[name] = eigen_scores(samp.hidden_states, K).cpu()
        elif method in _CONSISTENCY:
            if "cons" not in cache:
                cache["cons"] = _consistency(uncertainty_requests, samp, input_length, K, _eos_ids(model, gen_config))
            value = getattr(cache["cons"][req.get("similarity", SIMILARITIES[0])], _CONSISTENCY[method]).cpu()
            scores[name] = value.to(torch.int64) if method == "num_sets" else value
        else:  # semantic_entropy
            ent, groups = [], []
            for b in range(B):
                part = sampled_texts[b * K:(b + 1) * K]
                entropy, clusters = semantic_entropy(nli_model, nli_tokenizer, part)
                ent.append(float(entropy))
                groups.append({part[i]: c for c, members in clusters.items() for i in members})
            scores["clusters"] = groups
            scores[name] = torch.tensor(ent, dtype=torch.float64)
    return texts, scores
