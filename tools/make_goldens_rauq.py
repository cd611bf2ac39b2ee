#!/usr/bin/env python3
"""RAUQ fixture: the reference's ``rauq_uncertainty``, ``rauq_uncertainty_mean_heads`` and ``rauq_uncertainty_rollout``
(runia_core/llm_uncertainty/scores.py:155-344, imported by path as in tools/make_goldens.py) on

- the mocks of its own tests (tests/unit_test_llm_uncertainty.py:371-556, SEED = 42): one softmax row per step, so the
  rollout broadcasts step 0's single query row over the prompt block;
- causal f32 mocks (a lower-triangular prompt block, as HuggingFace ``generate`` returns it);
- a bf16 and an f16 greedy generation of a seeded random-init eager ``LlamaForCausalLM`` (nothing downloaded), on the CPU;
- edge cases: n_gen = 2, alphas [0, 0.5, 1], 2-D log-probs for the per-head modes.

Writes tests/golden/ref_rauq.npz (data only, loads with allow_pickle=False).  Per case ``c``:
  c__step{g}   (L, H, q, k) f32 - the maps of step g, batch 0 (bf16 / f16 values are exact in f32), c__dtype the tag,
  c__lp        the log-probs as the per-head modes got them (1-D, or (1, n) when c__lp2d), rollout gets them as (1, n),
  c__in        input_length, c__alphas,
  c__{head}__{token}  the scores the reference returns with ablation=True (head: original / mean_heads / rollout),
  c__heads__{token}   the head of every layer rauq_uncertainty picks (its argmax, restated from scores.py:189-194).

Run where the reference checkout exists (its location: REF in tools/make_goldens.py):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_rauq.py
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from make_goldens import OUT, REF  # noqa: E402

HEADS = ("original", "mean_heads", "rollout")
TOKENS = ("original", "mean_all_tokens")


def _load_reference():
    for name, path in (("runia_core", f"{REF}/runia_core"), ("runia_core.llm_uncertainty", f"{REF}/runia_core/llm_uncertainty")):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
    import runia_core.llm_uncertainty.attention_aggregation as agg
    import runia_core.llm_uncertainty.scores as scores

    return scores, agg


def reference_mocks():
    """unit_test_llm_uncertainty.py:379-391 and test_rauq_uncertainty_rollout (4 tokens, 4 layers, 4 heads, seq 8), and the
    5-token / 6-layer / 8-head shape of test_rauq_uncertainty_original; seeded per case as setUp does."""
    out = []
    for name, (n_tok, n_l, n_h, seq) in (("mock_rollout", (4, 4, 4, 8)), ("mock_original", (5, 6, 8, 10))):
        np.random.seed(42)
        torch.manual_seed(42)
        lp = torch.randn(1, n_tok)
        att = tuple(tuple(torch.softmax(torch.randn(1, n_h, 1, seq + t), dim=-1) for _ in range(n_l)) for t in range(n_tok))
        out.append((name, att, lp[0], seq, [0.2, 0.4, 0.7]))
    return out


def causal_maps(rng, n_l, n_h, inp, n_gen, dtype=torch.float32):
    """Softmax maps with HuggingFace's structure: a causal (in, in) prompt block (exact zeros above the diagonal), then
    one row of in + g keys per step."""
    steps = []
    for g in range(n_gen):
        per_layer = []
        for _ in range(n_l):
            if g == 0:
                x = torch.from_numpy(rng.standard_normal((1, n_h, inp, inp)).astype(np.float32) * 2)
                x = x.masked_fill(torch.triu(torch.ones(inp, inp, dtype=torch.bool), 1), float("-inf"))
            else:
                x = torch.from_numpy(rng.standard_normal((1, n_h, 1, inp + g)).astype(np.float32) * 2)
            per_layer.append(torch.softmax(x, dim=-1).to(dtype))
        steps.append(tuple(per_layer))
    return tuple(steps)


def causal_mocks():
    rng = np.random.default_rng(7)
    out = []
    att = causal_maps(rng, 5, 6, 9, 7)
    out.append(("causal_f32", att, torch.from_numpy(np.log(rng.uniform(0.05, 1.0, 7)).astype(np.float32)), 9, [0.2, 0.4, 0.7]))
    att = causal_maps(rng, 3, 2, 5, 2)
    out.append(("edge_ngen2", att, torch.from_numpy(np.log(rng.uniform(0.05, 1.0, 2)).astype(np.float32)), 5, [0.0, 0.5, 1.0]))
    att = causal_maps(rng, 2, 3, 4, 6)
    out.append(("edge_lp2d", att, torch.from_numpy(np.log(rng.uniform(0.05, 1.0, (1, 6))).astype(np.float32)), 4, [0.3]))
    return out


def tiny_llama(dtype, seed):
    """Greedy generation of a random-init eager LlamaForCausalLM on the CPU: attentions and transition log-probs."""
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=96, hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128, attn_implementation="eager")
    model = LlamaForCausalLM(cfg).to(dtype).eval()
    inp, n_gen = 11, 9
    ids = torch.randint(3, 96, (1, inp))
    with torch.no_grad():
        out = model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=n_gen, min_new_tokens=n_gen,
                             do_sample=False, output_attentions=True, output_scores=True, return_dict_in_generate=True,
                             pad_token_id=0)
        lp = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
    assert len(out.attentions) == n_gen and out.attentions[0][0].shape == (1, 4, inp, inp), out.attentions[0][0].shape
    return out.attentions, lp[0].float(), inp


def main():
    scores, agg = _load_reference()
    cases = reference_mocks() + causal_mocks()
    for name, dtype, seed in (("llama_bf16", torch.bfloat16, 11), ("llama_f16", torch.float16, 12)):
        att, lp, inp = tiny_llama(dtype, seed)
        cases.append((name, att, lp, inp, [0.2, 0.4, 0.7]))
    data = {"cases": np.array([c[0] for c in cases])}
    for name, att, lp, inp, alphas in cases:
        data[f"{name}__dtype"] = np.array(str(att[0][0].dtype).replace("torch.", ""))
        for g, step in enumerate(att):
            data[f"{name}__step{g}"] = torch.stack([t[0] for t in step]).float().numpy()
        lp_mode = lp  # the per-head modes get the log-probs as stored
        data[f"{name}__lp"] = lp_mode.numpy().astype(np.float32)
        data[f"{name}__lp2d"] = np.array(lp.dim() == 2)
        data[f"{name}__in"] = np.array(inp)
        data[f"{name}__alphas"] = np.array(alphas, dtype=np.float64)
        lp2 = lp.reshape(1, -1)
        for tok in TOKENS:
            data[f"{name}__original__{tok}"] = np.array(scores.rauq_uncertainty(lp_mode, att, tok, alphas, True))
            data[f"{name}__mean_heads__{tok}"] = np.array(scores.rauq_uncertainty_mean_heads(lp_mode, att, tok, alphas, True))
            data[f"{name}__rollout__{tok}"] = np.array(scores.rauq_uncertainty_rollout(lp2, att, tok, inp, alphas, True))
            w = (agg._get_recurent_attention if tok == "original" else agg._get_average_attention_all)(att)
            data[f"{name}__heads__{tok}"] = np.array([int(torch.argmax(w[l, :, 1:].mean(dim=1))) for l in range(w.shape[0])])
        print(name, {k.split("__", 1)[1]: v for k, v in data.items() if k.startswith(name + "__") and "step" not in k and v.size < 8})
    path = os.path.join(OUT, "ref_rauq.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(cases)} cases)")


if __name__ == "__main__":
    main()
