#!/usr/bin/env python3
"""Logit-score fixture: the reference's ``generation_entropy``, ``perplexity`` and ``normalized_entropy``
(runia_core/llm_uncertainty/scores.py:69-85, 121-152, utils.py:83-99, imported by path as in tools/make_goldens.py) and
HuggingFace's ``compute_transition_scores(normalize_logits=True)`` (the call compute_uncertainties makes,
scores.py:452-456, 495-499) on

- the seeded mocks of the reference's own tests (tests/unit_test_llm_uncertainty.py:121-370, SEED = 42): its
  generation_entropy logits, and its normalized_entropy / perplexity log-probabilities turned into V = 2 logits
  [lp, log(1 - e^lp)] with the token at 0 (the two torch.randn log-prob mocks are not log-probabilities and are left out);
- CPU ``generate()`` of a seeded random-init tiny ``LlamaForCausalLM`` (nothing downloaded): greedy, and do_sample with
  top_k and num_return_sequences = 5; eos_token_id ends some samples early, so their padded steps score -inf;
- synthetic cases: V = 1, 50, 32 001, 50 257, rows with many p < 1e-12, -inf-masked rows, rows of NaN / +inf / only -inf,
  bf16 and f16 scores, (B, 1, V) steps.

The reference runs on the f32 values of the scores (bf16 / f16 scores are widened first: the kernel computes in f32, the
reference's own bf16 softmax would round every probability to 8 bits).  Writes tests/golden/ref_logit_scores.npz (data
only, loads with allow_pickle=False).  Per case ``c``:
  c__steps    (T, B, V) f32 logits, or c__recipe = [seed, T, B, V] with c__scale: the logits are
              default_rng(seed).standard_normal((T, B, V), float32) * scale (large V: only the recipe is stored)
  c__dtype    float32 / float16 / bfloat16 (the scores are the f32 values cast to it), c__step3d: steps are (B, 1, V)
  c__sequences  (B, length) int64, the generated tokens are the last T columns
  c__log_probs  (B, T) HF compute_transition_scores(normalize_logits=True) (f32)
  c__token_entropy  (B, T) the reference's per-token entropy (generation_entropy of the one step, row b)
  c__generation_entropy, c__perplexity  (B,) the reference's generation_entropy of row b and perplexity(log_probs[b])
  c__normalized_entropy  the reference's normalized_entropy(log_probs) over all rows

Run where the reference checkout exists (its location: REF in tools/make_goldens.py):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_logits.py
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

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _load_reference():
    for name, path in (("runia_core", f"{REF}/runia_core"), ("runia_core.llm_uncertainty", f"{REF}/runia_core/llm_uncertainty")):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
    import runia_core.llm_uncertainty.scores as scores

    return scores


def hf_transition_scores(sequences, steps):
    """HuggingFace's compute_transition_scores(normalize_logits=True) without beams; it reads only config.vocab_size."""
    from transformers.generation.utils import GenerationMixin

    cfg = types.SimpleNamespace(vocab_size=int(steps[0].shape[-1]))
    cfg.get_text_config = lambda *a, **k: cfg
    owner = types.SimpleNamespace(config=cfg)
    return GenerationMixin.compute_transition_scores(owner, sequences, steps, normalize_logits=True)


def recipe_logits(seed, T, B, V, scale):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, B, V), dtype=np.float32) * np.float32(scale)


def reference_mocks():
    """(name, (T, B, V) f32 logits, tokens (B, T)) of unit_test_llm_uncertainty.py's generation_entropy and log-prob mocks."""
    out = []
    torch.manual_seed(42)
    np.random.seed(42)
    out.append(("mock_gen_basic", torch.stack([torch.randn(1, 100) for _ in range(5)]).numpy(), None))
    out.append(("mock_gen_uniform", np.zeros((3, 1, 50), np.float32), None))
    peaked = np.full((3, 1, 50), -10.0, np.float32)
    peaked[:, 0, 0] = 10.0
    out.append(("mock_gen_peaked", peaked, None))
    inf = -float("inf")
    lp_mocks = {
        "mock_ne_uniform": torch.log(torch.ones(3, 5) * 0.2),
        "mock_ne_inf": torch.tensor([[-0.5, -1.0, -0.3, inf, -0.8], [-0.2, -0.6, inf, -0.9, -1.2]]),
        "mock_ne_high_conf": torch.log(torch.tensor([[0.9, 0.05, 0.03, 0.01, 0.01], [0.85, 0.08, 0.04, 0.02, 0.01]])),
        "mock_ne_low_conf": torch.log(torch.full((2, 5), 0.2)),
        "mock_ppl_basic": torch.tensor([[-0.5, -0.8, -0.3, -0.6, -0.9]]),
        "mock_ppl_zero": torch.zeros(1, 10),
        "mock_ppl_consistency": torch.tensor([[-1.0, -2.0, -1.5, -0.5]]),
    }
    for name, lp in lp_mocks.items():
        lp = lp.double()
        rest = torch.log(-torch.expm1(lp))  # log(1 - e^lp): -inf for lp = 0, 0 for lp = -inf
        x = torch.stack([lp, rest], dim=-1).float().transpose(0, 1).contiguous().numpy()  # (T, B, 2)
        out.append((name, x, np.zeros(lp.shape, np.int64)))
    return out


def tiny_llama_generations():
    """Greedy (B = 1) and sampled (top_k = 20, 5 sequences) CPU generations of a random-init LlamaForCausalLM."""
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(31)
    cfg = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).eval()
    ids = torch.randint(3, 128, (1, 9))

    def gen(sample, eos, seed):
        torch.manual_seed(seed)
        kw = dict(do_sample=True, top_k=20, num_return_sequences=5) if sample else dict(do_sample=False)
        with torch.no_grad():
            out = model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=14, output_scores=True,
                                 return_dict_in_generate=True, pad_token_id=0, eos_token_id=eos, **kw)
        return out

    out = []
    greedy = gen(False, None, 0)
    out.append(("llama_greedy", greedy))
    # an eos id that a sample emits at its third step: that sample ends there and its later steps are padding (the pad id
    # is outside the top-k, so those steps score -inf); the same seed reproduces the draws up to the eos
    probe = gen(True, None, 5)
    eos = int(probe.sequences[1, ids.shape[1] + 2])
    sampled = gen(True, eos, 5)
    assert len(sampled.scores) > 3 and (sampled.sequences[:, ids.shape[1]:] == 0).any(), "no sample ended early"
    out.append(("llama_topk_eos", sampled))
    return out


def synthetic():
    """(name, logits (T, B, V) f32 or None, recipe or None, scale, dtype, step3d, tokens (B, T))."""
    rng = np.random.default_rng(2024)
    out = []
    out.append(("v1", np.array(rng.standard_normal((3, 2, 1)), np.float32), None, 0, "float32", False,
                np.zeros((2, 3), np.int64)))
    x = (rng.standard_normal((4, 3, 50)) * 2).astype(np.float32)
    out.append(("v50", x, None, 0, "float32", False, rng.integers(0, 50, (3, 4))))
    # top-5 masking: most logits -inf, some tokens drawn outside the top 5 score -inf
    m = (rng.standard_normal((4, 3, 50)) * 2).astype(np.float32)
    kth = np.sort(m, axis=-1)[..., -5:-4]
    m = np.where(m >= kth, m, -np.inf).astype(np.float32)
    tok = rng.integers(0, 50, (3, 4))
    tok[:, ::2] = m.argmax(-1).T[:, ::2]  # every other step takes the top token: every row keeps finite log-probs
    out.append(("v50_topk_masked", m, None, 0, "float32", False, tok))
    out.append(("v50_bf16", x, None, 0, "bfloat16", False, rng.integers(0, 50, (3, 4))))
    out.append(("v50_f16_3d", x, None, 0, "float16", True, rng.integers(0, 50, (3, 4))))
    bad = (rng.standard_normal((2, 4, 20))).astype(np.float32)
    bad[0, 1, 3] = np.nan
    bad[1, 2, 7] = np.inf
    bad[:, 3, :] = -np.inf
    out.append(("nan_rows", bad, None, 0, "float32", False, rng.integers(0, 20, (4, 2))))
    # large V: the recipe only.  Scale 12 leaves most probabilities far below 1e-12
    out.append(("v32001_tiny_p", None, (11, 3, 2, 32001), 12.0, "float32", False, rng.integers(0, 32001, (2, 3))))
    out.append(("v50257", None, (12, 2, 3, 50257), 3.0, "float32", True, rng.integers(0, 50257, (3, 2))))
    out.append(("v50257_bf16", None, (13, 2, 2, 50257), 3.0, "bfloat16", False, rng.integers(0, 50257, (2, 2))))
    return out


def score_case(ref, x32, dtype, step3d, sequences):
    """The reference's numbers on logits whose f32 values are x32 (T, B, V) cast to dtype."""
    T, B, V = x32.shape
    vals = torch.from_numpy(x32).to(DTYPES[dtype]).float()  # the values the kernel reads
    steps = tuple(vals[t][:, None, :] if step3d else vals[t] for t in range(T))
    lp = hf_transition_scores(sequences, steps)
    tok_ent = np.array([[ref.generation_entropy((steps[t][b:b + 1],)) for t in range(T)] for b in range(B)])
    gen = np.array([ref.generation_entropy(tuple(s[b:b + 1] for s in steps)) for b in range(B)])
    ppl = np.array([ref.perplexity(lp[b]) for b in range(B)])
    return dict(log_probs=lp.numpy().astype(np.float32), token_entropy=tok_ent, generation_entropy=gen, perplexity=ppl,
                normalized_entropy=np.array(ref.normalized_entropy(lp)))


def main():
    ref = _load_reference()
    data, names = {}, []

    def add(name, x32, recipe, scale, dtype, step3d, sequences):
        names.append(name)
        if recipe is None:
            data[f"{name}__steps"] = x32
        else:
            data[f"{name}__recipe"] = np.array(recipe, dtype=np.int64)
            data[f"{name}__scale"] = np.array(scale, dtype=np.float64)
        data[f"{name}__dtype"] = np.array(dtype)
        data[f"{name}__step3d"] = np.array(step3d)
        data[f"{name}__sequences"] = sequences.numpy().astype(np.int64)
        for k, v in score_case(ref, x32, dtype, step3d, sequences).items():
            data[f"{name}__{k}"] = v
        print(name, x32.shape, dtype, "normalized_entropy", float(data[f"{name}__normalized_entropy"]))

    for name, x, tok in reference_mocks():
        T, B, V = x.shape
        if tok is None:
            tok = np.random.default_rng(len(names)).integers(0, V, (B, T))
        add(name, x, None, 0, "float32", False, torch.from_numpy(tok))
    for name, out in tiny_llama_generations():
        x = torch.stack(out.scores).numpy()
        add(name, x, None, 0, "float32", False, out.sequences)
        # HF's own call on the generation's scores, as compute_uncertainties makes it
        data[f"{name}__hf_log_probs"] = hf_transition_scores(out.sequences, out.scores).numpy().astype(np.float32)
    for name, x, recipe, scale, dtype, step3d, tok in synthetic():
        if recipe is not None:
            x = recipe_logits(recipe[0], *recipe[1:], scale)
        add(name, x, recipe, scale, dtype, step3d, torch.from_numpy(np.asarray(tok, np.int64)))
    data["cases"] = np.array(names)
    path = os.path.join(OUT, "ref_logit_scores.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(names)} cases)")


if __name__ == "__main__":
    main()
