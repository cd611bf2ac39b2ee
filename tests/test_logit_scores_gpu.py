"""Logit scores on the device (csrc/logits.hip): reference fixture parity in f32, bf16 and f16, the input contract (host,
device, row-strided and (B, 1, V) steps give equal bits, inputs untouched), bitwise repeatability and row independence,
the Llama-3.1-8B shape against an f64 restatement and torch with the call's peak memory, and a real HuggingFace
generation (transition scores, and RAUQ fed the new log-probs)."""
import gc

import numpy as np
import pytest
import torch

from runia_core_amd.llm_uncertainty import RAUQ, generation_scores, token_entropies, transition_scores
from test_logit_scores_host import (SEQ_KEYS, assert_close, assert_log_probs, case_scores, case_tokens, case_values,
                                    fixture_cases, ref_tol, restate)

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _all(res):
    """Every output of a GenerationScores as host arrays (bitwise comparisons)."""
    return [_np(res.log_probs), _np(res.token_entropy), _np(res.generation_entropy), _np(res.perplexity),
            np.array(res.normalized_entropy)]


def _equal_bits(a, b, what=""):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert x.tobytes() == y.tobytes(), what


def _check(res, exp, V, tol_scale_ref, what):
    tol = (lambda t: ref_tol(V, t)) if tol_scale_ref else (lambda t: t)
    assert_log_probs(_np(res.log_probs), exp["log_probs"], what, tol(2e-6))
    assert_close(_np(res.token_entropy), exp["token_entropy"], tol(1e-6), False, f"{what} token entropy")
    got = dict(generation_entropy=_np(res.generation_entropy), perplexity=_np(res.perplexity),
               normalized_entropy=res.normalized_entropy)
    for k in SEQ_KEYS:
        assert_close(got[k], exp[k], tol(1e-6), True, f"{what} {k}")


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c["name"])
def test_logit_scores_fixture_parity(case):
    scores = case_scores(case, "cuda")
    seq = torch.from_numpy(case["sequences"]).cuda()
    res = generation_scores(seq, scores)
    T, B, V = case["logits"].shape
    assert res.log_probs.shape == (B, T) and res.log_probs.dtype == torch.float32 and res.log_probs.is_cuda
    assert res.token_entropy.shape == (B, T) and res.generation_entropy.shape == (B,) and res.perplexity.shape == (B,)
    assert isinstance(res.normalized_entropy, float)
    _check(res, case, V, True, case["name"])
    # the f64 restatement holds the kernels to the base tolerances at every V
    _check(res, restate(case_values(case), case_tokens(case)), V, False, f"{case['name']} vs f64")
    if "hf_log_probs" in case:
        assert_log_probs(_np(res.log_probs), case["hf_log_probs"], f"{case['name']} HF", ref_tol(V, 2e-6))
    # the single-output entry points give the same bits; normalize_logits=False is the plain gather
    assert _np(transition_scores(seq, scores, normalize_logits=True)).tobytes() == _np(res.log_probs).tobytes()
    assert _np(token_entropies(scores)).tobytes() == _np(res.token_entropy).tobytes()
    raw = _np(transition_scores(seq, scores))
    x = case_values(case).astype(np.float32)
    tok = case_tokens(case)
    exp_raw = np.take_along_axis(x, tok.T[..., None], -1)[..., 0].T
    assert raw.tobytes() == exp_raw.tobytes()


def _case(name):
    return next(c for c in fixture_cases() if c["name"] == name)


@pytest.mark.parametrize("name", ["v50257", "llama_topk_eos", "v50_bf16"])
def test_logit_scores_inputs_bitwise_and_untouched(name):
    case = _case(name)
    seq = torch.from_numpy(case["sequences"])
    dev = case_scores(case, "cuda")
    flat = tuple(s.reshape(s.shape[0], -1) for s in dev)
    host = case_scores(case, "cpu")
    # rows inside a wider buffer at an odd offset: row starts are not 16-byte aligned (the element-wise load path)
    strided = []
    for s in flat:
        store = torch.full((s.shape[0], s.shape[1] + 37), float("nan"), dtype=s.dtype, device="cuda")
        store[:, 5:5 + s.shape[1]] = s
        strided.append(store[:, 5:5 + s.shape[1]])
    strided = tuple(strided)
    three_d = tuple(s[:, None, :] for s in strided)
    # a vocabulary axis that is not unit-stride: made contiguous by the wrapper
    transposed = tuple(s.t().contiguous().t() for s in flat)
    snap = [s.clone() for s in strided]
    ref = _all(generation_scores(seq.cuda(), flat))
    for what, sc, sq in (("host", host, seq), ("device, host ids", flat, seq), ("strided", strided, seq.cuda()),
                         ("(B, 1, V) strided", three_d, seq.cuda()), ("vocab stride", transposed, seq.cuda())):
        res = generation_scores(sq, sc)
        if what == "host":
            assert not res.log_probs.is_cuda and not res.generation_entropy.is_cuda
        _equal_bits(ref, _all(res), what)
    torch.cuda.synchronize()
    for a, b in zip(snap, strided):
        assert torch.equal(a, b)
    _equal_bits(ref, _all(generation_scores(seq.cuda(), flat)), "second call")


def test_logit_scores_row_independent_of_the_batch():
    g = torch.Generator(device="cuda").manual_seed(3)
    T, B, V = 5, 10, 50257
    scores = tuple(torch.randn(B, V, generator=g, device="cuda") * 3 for _ in range(T))
    seq = torch.randint(0, V, (B, 7 + T), generator=g, device="cuda")
    full = generation_scores(seq, scores)
    for b in (0, 3, 9):
        one = generation_scores(seq[b:b + 1], tuple(s[b:b + 1] for s in scores))
        assert one.log_probs.cpu().numpy().tobytes() == full.log_probs[b:b + 1].cpu().numpy().tobytes()
        assert one.token_entropy.cpu().numpy().tobytes() == full.token_entropy[b:b + 1].cpu().numpy().tobytes()
        assert float(one.generation_entropy[0]) == float(full.generation_entropy[b])
        assert float(one.perplexity[0]) == float(full.perplexity[b])
    # single-step calls and the first T' steps give the same per-token bits
    head = generation_scores(seq[:, :-2], scores[:T - 2])
    assert _np(head.log_probs).tobytes() == _np(full.log_probs[:, :T - 2]).tobytes()
    assert _np(head.token_entropy).tobytes() == _np(full.token_entropy[:, :T - 2]).tobytes()


def test_logit_scores_llama_8b_shape_memory_and_accuracy():
    """T = 256 steps of (10, 128 256) f32 scores, 1.31 GB: the call's peak allocation beyond its inputs stays within the
    outputs + workspace + 1 MB.  HF's compute_transition_scores(normalize_logits=True) on the same scores allocates the
    stacked copy and the log_softmax output, 2 x 1.31 GB."""
    T, B, V = 256, 10, 128256
    g = torch.Generator(device="cuda").manual_seed(11)
    scores = tuple(torch.randn(B, V, generator=g, device="cuda") * 4 for _ in range(T))
    seq = torch.randint(0, V, (B, 32 + T), generator=g, device="cuda")
    try:
        from runia_core_amd import _hip

        ws = int(_hip.load_library().runia_logit_stats_workspace_bytes(T, B, V))
        out_bytes = 2 * B * T * 4 + (3 * B + 1) * 8
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = generation_scores(seq, scores)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        hf_bytes = 2 * T * B * V * 4
        assert peak <= out_bytes + ws + (1 << 20), (peak, out_bytes, ws, hf_bytes)
        print(f"peak extra {peak} B (outputs {out_bytes} + workspace {ws}); HF formulation >= {hf_bytes} B")
        # f64 restatement on the device, every row, and torch's own f32 log_softmax
        tok = seq[:, -T:]
        lp64 = torch.empty(B, T, dtype=torch.float64, device="cuda")
        h64 = torch.empty(B, T, dtype=torch.float64, device="cuda")
        lp_t = torch.empty(B, T, dtype=torch.float32, device="cuda")
        for t, s in enumerate(scores):
            x = s.double()
            lse = torch.logsumexp(x, -1)
            lp64[:, t] = x.gather(1, tok[:, t:t + 1])[:, 0] - lse
            p = torch.softmax(x, -1)
            h64[:, t] = -(p * p.clamp_min(1e-12).log()).sum(-1) / np.log(V)
            lp_t[:, t] = torch.log_softmax(s, -1).gather(1, tok[:, t:t + 1])[:, 0]
        assert_log_probs(_np(res.log_probs), _np(lp64), "8B vs f64", 2e-6)
        assert_log_probs(_np(res.log_probs), _np(lp_t), "8B vs torch", 1e-5)
        assert_close(_np(res.token_entropy), _np(h64), 1e-6, False, "8B entropy vs f64")
        assert_close(_np(res.generation_entropy), _np(h64.mean(1)), 1e-6, True, "8B generation entropy")
        assert_close(_np(res.perplexity), _np(-lp64.mean(1)), 1e-6, True, "8B perplexity")
        assert_close(res.normalized_entropy, float(-lp64.mean(1).mean()), 1e-6, True, "8B normalized entropy")
        # the chunked partials are the same for bf16 input of the same values
        bf = tuple(s.bfloat16() for s in scores[:8])
        rb = generation_scores(seq[:, :-(T - 8)], bf)
        xb = torch.stack([s.double() for s in bf])  # (8, B, V)
        lpb = (xb.gather(2, tok[:, :8].t()[..., None])[..., 0] - torch.logsumexp(xb, -1)).t()
        assert_log_probs(_np(rb.log_probs), _np(lpb), "8B bf16 vs f64", 2e-6)
    finally:
        del scores
        gc.collect()
        torch.cuda.empty_cache()


def test_logit_scores_real_hf_generation_and_rauq():
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(23)
    cfg = transformers.LlamaConfig(vocab_size=160, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256,
                                   attn_implementation="eager")
    model = transformers.LlamaForCausalLM(cfg).cuda().eval()
    ids = torch.randint(3, 160, (1, 12), device="cuda")
    with torch.no_grad():
        samp = model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=10, do_sample=True, top_k=30,
                              num_return_sequences=5, output_scores=True, return_dict_in_generate=True, pad_token_id=0)
        greedy = model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=10, min_new_tokens=10,
                                do_sample=False, output_attentions=True, output_scores=True, return_dict_in_generate=True,
                                pad_token_id=0)
    for out in (samp, greedy):
        assert out.scores[0].is_cuda
        hf = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
        ours = transition_scores(out.sequences, out.scores, normalize_logits=True)
        assert_log_probs(_np(ours), _np(hf.float()), "HF generation")
        raw = model.compute_transition_scores(out.sequences, out.scores)
        assert torch.equal(transition_scores(out.sequences, out.scores), raw.float())
    # RAUQ fed the new log-probs gives RAUQ's result on HF's
    hf = model.compute_transition_scores(greedy.sequences, greedy.scores, normalize_logits=True).float()
    lp = generation_scores(greedy.sequences, greedy.scores).log_probs
    alphas = [0.2, 0.4, 0.7]
    for head in ("original", "mean_heads", "rollout"):
        for tok in ("original", "mean_all_tokens"):
            a = RAUQ(hf if head == "rollout" else hf[0], greedy.attentions, 12, tok, head, alphas, True)
            b = RAUQ(lp if head == "rollout" else lp[0], greedy.attentions, 12, tok, head, alphas, True)
            rel = np.max(np.abs(np.array(a) - np.array(b)) / np.maximum(np.abs(np.array(a)), 1e-30))
            assert rel <= (1e-5 if head == "rollout" else 1e-6), (head, tok, a, b)
