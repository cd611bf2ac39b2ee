#!/usr/bin/env python3
"""Batched RAUQ fixture: the reference's ``rauq_uncertainty``, ``rauq_uncertainty_mean_heads`` and
``rauq_uncertainty_rollout`` (runia_core/llm_uncertainty/scores.py:155-344, imported by path as in
tools/make_goldens_rauq.py) run on every row's own slices of a left-padded batch:

  step 0 [b:b+1, :, pad_b:, pad_b:], step 1 <= g < n_b [b:b+1, :, :, pad_b:], log-probs [b, :n_b] (1-D for the per-head
  modes, (1, n_b) for the rollout), input_length - pad_b.

A row whose one-row call raises (n_b < 2 for "original" token aggregation or the rollout) is stored as NaN.  Cases:

- llama_pad_f32 / llama_pad_bf16: a left-padded greedy batch of a seeded random-init eager ``LlamaForCausalLM`` on the CPU
  (nothing downloaded; its pad keys hold exact zeros);
- llama_sampled_eos: a left-padded top-k sampled batch with eos, so rows finish early (lengths up to the first eos);
- causal_mixed: causal f32 mocks with mixed padding and junk in the pad keys, one row with n_b = 1.

Writes tests/golden/ref_rauq_batch.npz (data only, loads with allow_pickle=False).  Per case ``c``:
  c__step{g}  (B, L, H, q, k) f32 - the full padded maps of step g (bf16 values are exact in f32), c__dtype the tag,
  c__mask     (B, in) int64 attention mask, c__lengths (B,) int64 n_b, c__lp (B, n_gen) f32, c__in, c__alphas,
  c__{head}__{token}  (B, n_alpha) f64 - the reference's scores with ablation=True.

Run where the reference checkout exists (its location: REF in tools/make_goldens.py):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_rauq_batch.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from make_goldens import OUT  # noqa: E402
from make_goldens_rauq import HEADS, TOKENS, _load_reference  # noqa: E402


def row_slices(att, lp, mask, lengths, b):
    """Row b's maps, 1-D log-probs and input length, as the contract cuts them."""
    pad = int((mask[b] == 0).sum())
    n = int(lengths[b])
    maps = tuple(tuple((t[b:b + 1, :, pad:, pad:] if g == 0 else t[b:b + 1, :, :, pad:]) for t in att[g]) for g in range(n))
    return maps, lp[b, :n], mask.shape[1] - pad


def reference_scores(scores, att, lp, mask, lengths, alphas):
    out = {}
    for head in HEADS:
        for tok in TOKENS:
            rows = []
            for b in range(lp.shape[0]):
                maps, lpb, inb = row_slices(att, lp, mask, lengths, b)
                if len(maps) < 2 and (tok == "original" or head == "rollout"):
                    rows.append([np.nan] * len(alphas))  # the one-row call raises
                elif head == "original":
                    rows.append(scores.rauq_uncertainty(lpb, maps, tok, alphas, True))
                elif head == "mean_heads":
                    rows.append(scores.rauq_uncertainty_mean_heads(lpb, maps, tok, alphas, True))
                else:
                    rows.append(scores.rauq_uncertainty_rollout(lpb.reshape(1, -1), maps, tok, inb, alphas, True))
            out[(head, tok)] = np.array([[float(v) for v in r] for r in rows], dtype=np.float64)
    return out


def tiny_llama_batch(dtype, seed, sample):
    """A left-padded batch of 4 prompts (pads 0, 3, 5, 1) generated on the CPU: maps, log-probs, mask, lengths."""
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(seed)
    eos = [5, 6, 7, 8, 9, 10]
    cfg = LlamaConfig(vocab_size=32, hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128, attn_implementation="eager", pad_token_id=0,
                      eos_token_id=eos if sample else None)
    model = LlamaForCausalLM(cfg).to(dtype).eval()
    inp, n_gen, pads = 10, 8, (0, 3, 5, 1)
    ids = torch.randint(11, 32, (len(pads), inp))
    mask = torch.ones_like(ids)
    for b, p in enumerate(pads):
        mask[b, :p] = 0
        ids[b, :p] = 0
    kw = dict(do_sample=True, top_k=8, eos_token_id=eos) if sample else dict(do_sample=False, min_new_tokens=n_gen)
    with torch.no_grad():
        out = model.generate(ids, attention_mask=mask, max_new_tokens=n_gen, output_attentions=True, output_scores=True,
                             return_dict_in_generate=True, pad_token_id=0, **kw)
        lp = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True).float()
    gen = out.sequences[:, inp:]
    n_steps = gen.shape[1]
    assert len(out.attentions) == n_steps and out.attentions[0][0].shape == (len(pads), 4, inp, inp)
    if sample:
        hit = torch.isin(gen, torch.tensor(eos))
        lengths = torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.full((len(pads),), n_steps))
        assert int(lengths.min()) < n_steps, lengths  # some row finishes early
    else:
        lengths = torch.full((len(pads),), n_steps)
    for b, p in enumerate(pads):  # the pad keys of the row's own queries are exact zeros
        assert all(float(t[b, :, (p if g == 0 else 0):, :p].abs().max()) == 0.0
                   for g, step in enumerate(out.attentions) for t in step if p)
    return out.attentions, lp, mask, lengths, inp  # -inf after a row's eos: never read


def causal_mixed(rng):
    """Causal f32 maps, B = 4 rows padded (0, 2, 4, 6) on in = 9, junk (not zero) in every pad key; lengths (7, 5, 1, 6)."""
    L, H, inp, n_gen, pads, lengths = 3, 4, 9, 7, (0, 2, 4, 6), (7, 5, 1, 6)
    B = len(pads)
    steps = []
    for g in range(n_gen):
        per = []
        for _ in range(L):
            q = inp if g == 0 else 1
            x = torch.from_numpy(rng.standard_normal((B, H, q, inp + g)).astype(np.float32) * 2)
            if g == 0:
                x = x.masked_fill(torch.triu(torch.ones(inp, inp, dtype=torch.bool), 1), float("-inf"))
            t = torch.from_numpy(rng.uniform(0.0, 1.0, (B, H, q, inp + g)).astype(np.float32))
            for b, p in enumerate(pads):
                if g == 0:
                    t[b, :, p:, p:] = torch.softmax(x[b, :, p:, p:], dim=-1)
                else:
                    t[b, :, :, p:] = torch.softmax(x[b, :, :, p:], dim=-1)
            per.append(t)
        steps.append(tuple(per))
    mask = torch.ones(B, inp, dtype=torch.int64)
    for b, p in enumerate(pads):
        mask[b, :p] = 0
    lp = torch.from_numpy(np.log(rng.uniform(0.05, 1.0, (B, n_gen))).astype(np.float32))
    return tuple(steps), lp, mask, torch.tensor(lengths), inp


def main():
    scores, _ = _load_reference()
    cases = []
    for name, dtype, seed, sample in (("llama_pad_f32", torch.float32, 31, False), ("llama_pad_bf16", torch.bfloat16, 32, False),
                                      ("llama_sampled_eos", torch.float32, 33, True)):
        att, lp, mask, lengths, inp = tiny_llama_batch(dtype, seed, sample)
        cases.append((name, att, lp, mask, lengths, inp, [0.2, 0.4, 0.7]))
    att, lp, mask, lengths, inp = causal_mixed(np.random.default_rng(17))
    cases.append(("causal_mixed", att, lp, mask, lengths, inp, [0.0, 0.3, 1.0]))
    data = {"cases": np.array([c[0] for c in cases])}
    for name, att, lp, mask, lengths, inp, alphas in cases:
        data[f"{name}__dtype"] = np.array(str(att[0][0].dtype).replace("torch.", ""))
        for g, step in enumerate(att):
            data[f"{name}__step{g}"] = torch.stack(step, dim=1).float().numpy()
        data[f"{name}__mask"] = mask.numpy().astype(np.int64)
        data[f"{name}__lengths"] = lengths.numpy().astype(np.int64)
        data[f"{name}__lp"] = lp.numpy().astype(np.float32)
        data[f"{name}__in"] = np.array(inp)
        data[f"{name}__alphas"] = np.array(alphas, dtype=np.float64)
        for (head, tok), v in reference_scores(scores, att, lp, mask, lengths, alphas).items():
            data[f"{name}__{head}__{tok}"] = v
        print(name, "lengths", lengths.tolist(), "pads", (mask == 0).sum(1).tolist(),
              {f"{h}/{t}": np.round(data[f"{name}__{h}__{t}"][:, 0], 4).tolist() for h in HEADS for t in TOKENS})
    path = os.path.join(OUT, "ref_rauq_batch.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(cases)} cases)")


if __name__ == "__main__":
    main()
