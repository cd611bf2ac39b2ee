"""Batched RAUQ on the device (rauq_batch, csrc/rauq.hip): reference fixture parity, bitwise equality with the one-row
functions on every row's own slices (dtypes, host / device / strided maps, both rollout routes), row independence, a
real left-padded sampled generation, and the Llama-3.1-8B shape against an f64 restatement."""
import gc

import numpy as np
import pytest
import torch

from runia_core_amd.llm_uncertainty import RAUQ, generated_lengths, rauq_batch, transition_scores
from runia_core_amd.llm_uncertainty import rauq as rq
from test_rauq_batch_host import batch_fixture_cases, row_steps
from test_rauq_gpu import _restate_device, _strided
from test_rauq_host import HEADS, TOKENS, restate

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
MODES = [(h, t) for h in HEADS for t in TOKENS]


def _maps(case, device="cuda", dtype=None):
    dt = dtype or DTYPES[case["dtype"]]
    return tuple(tuple(torch.from_numpy(np.ascontiguousarray(s[:, l])).to(device=device, dtype=dt) for l in range(s.shape[1]))
                 for s in case["steps"])


def _pads(mask):
    return [int((torch.as_tensor(m) == 0).sum()) for m in mask]


def _one_row(att, lp, mask, lengths, inp, head, tok, alphas):
    """(B, n_alpha) f32 of the one-row RAUQ on every row's slices; NaN where it raises."""
    out = []
    for b, pad in enumerate(_pads(mask)):
        n = int(lengths[b])
        maps = tuple(tuple((t[b:b + 1, :, pad:, pad:] if g == 0 else t[b:b + 1, :, :, pad:]) for t in att[g]) for g in range(n))
        lpb = lp[b, :n]
        try:
            out.append(RAUQ(lpb.reshape(1, -1) if head == "rollout" else lpb, maps, inp - pad, tok, head, alphas, True))
        except (ValueError, IndexError):
            out.append([float("nan")] * len(alphas))
    return torch.tensor(out, dtype=torch.float32)


def _bits_equal(a, b):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _rel(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    ok = ~np.isnan(exp)
    assert np.array_equal(np.isnan(got), ~ok)
    return float(np.max(np.abs(got[ok] - exp[ok]) / np.maximum(np.abs(exp[ok]), 1e-30))) if ok.any() else 0.0


@pytest.mark.parametrize("case", batch_fixture_cases(), ids=lambda c: c["name"])
def test_rauq_batch_fixture_parity(case):
    att = _maps(case)
    lp, mask, lengths = torch.from_numpy(case["lp"]), torch.from_numpy(case["mask"]), torch.from_numpy(case["lengths"])
    for h, t in MODES:
        got = rauq_batch(lp, att, case["input_length"], t, h, case["alphas"], mask, lengths)
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == (len(lengths), len(case["alphas"]))
        tol = 1e-5 if h == "rollout" else 1e-6
        assert _rel(got.cpu().numpy(), case["scores"][(h, t)]) <= tol, (case["name"], h, t, got, case["scores"][(h, t)])


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_rauq_batch_bitwise_equals_one_row_calls(dtype):
    """Every mode, every fixture case, host / device / non-contiguous maps: the rows' bits are the one-row calls' on
    slices; the maps are left untouched."""
    for case in batch_fixture_cases():
        dev = _maps(case, dtype=DTYPES[dtype])
        host = _maps(case, device="cpu", dtype=DTYPES[dtype])
        strided = _strided(dev)
        snap = [t.clone() for s in strided for t in s]
        lp, mask, lengths = torch.from_numpy(case["lp"]), torch.from_numpy(case["mask"]), torch.from_numpy(case["lengths"])
        inp, alphas = case["input_length"], case["alphas"]
        for h, t in MODES:
            exp = _one_row(dev, lp, mask, lengths, inp, h, t, alphas)
            a = rauq_batch(lp, dev, inp, t, h, alphas, mask, lengths)
            b = rauq_batch(lp, host, inp, t, h, alphas, mask, lengths)
            c = rauq_batch(lp.cuda(), strided, inp, t, h, alphas, mask.cuda(), lengths.cuda())
            assert not b.is_cuda and a.is_cuda
            for got in (a, b, c):
                assert _bits_equal(got, exp), (case["name"], dtype, h, t, got, exp)
        torch.cuda.synchronize()
        for t0, t1 in zip(snap, (t for s in strided for t in s)):
            assert torch.equal(t0, t1)


def _padded_causal(L, H, inp, n_gen, pads, seed, dtype=torch.float32):
    """Causal softmax maps of B left-padded rows on the device; the pad keys are zeros."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    B = len(pads)
    key = torch.arange(inp + n_gen, device="cuda")
    padk = key[None, :] < torch.tensor(pads, device="cuda")[:, None]  # (B, k)
    causal = torch.triu(torch.ones(inp, inp, dtype=torch.bool, device="cuda"), 1)
    steps = []
    for s in range(n_gen):
        per = []
        for _ in range(L):
            if s == 0:
                x = torch.randn(B, H, inp, inp, generator=g, device="cuda") * 2
                x = x.masked_fill(causal[None, None] | padk[:, None, None, :inp], float("-inf"))
            else:
                x = torch.randn(B, H, 1, inp + s, generator=g, device="cuda") * 2
                x = x.masked_fill(padk[:, None, None, :inp + s], float("-inf"))
            per.append(torch.softmax(x, -1).nan_to_num(0.0).to(dtype))
            del x
        steps.append(tuple(per))
    return tuple(steps)


def _mask(pads, inp, device="cuda"):
    return (torch.arange(inp, device=device)[None, :] >= torch.tensor(pads, device=device)[:, None]).to(torch.int64)


def test_rauq_batch_rollout_routes_bitwise():
    """Causal rows take the one pass ("original") or the causal chain; a row with an entry above its prompt block's
    diagonal takes the general chain, next to rows that do not."""
    inp, n_gen, pads, alphas = 12, 9, [0, 3, 7, 1], [0.2, 0.4, 0.9]
    att = _padded_causal(4, 3, inp, n_gen, pads, 5)
    lp = torch.log(torch.rand(len(pads), n_gen, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.05)
    mask, lengths = _mask(pads, inp), torch.tensor([9, 6, 9, 2])
    bent = [list(s) for s in att]
    x = bent[0][2].clone()
    x[1, 1, 3 + 3, 3 + 7] = 0.25  # row 1, its own (3, 7)
    bent[0][2] = x
    bent = tuple(tuple(s) for s in bent)
    for maps, chained_rows in ((att, set()), (bent, {1})):
        for tok in TOKENS:
            for b, pad in enumerate(pads):  # the one-row route of every row
                n = int(lengths[b])
                sl = tuple(tuple((t[b:b + 1, :, pad:, pad:] if g == 0 else t[b:b + 1, :, :, pad:]) for t in maps[g])
                           for g in range(n))
                info = {}
                rq._rollout_scores(lp[b:b + 1, :n], sl, tok, inp - pad, alphas, info)
                assert info["upper_nonzero"] == (b in chained_rows)
                assert info["route"] == ("chain" if tok == "mean_all_tokens" or b in chained_rows else "one_pass")
            got = rauq_batch(lp, maps, inp, tok, "rollout", alphas, mask, lengths)
            exp = _one_row(maps, lp, mask, lengths, inp, "rollout", tok, alphas)
            assert _bits_equal(got, exp), (tok, got, exp)
            steps = [torch.stack(s, 1).double().cpu().numpy() for s in maps]
            for b, pad in enumerate(pads):
                n = int(lengths[b])
                r, _ = restate(row_steps(steps, pad, n, b), "float32", lp[b:b + 1, :n].numpy(), inp - pad, alphas, "rollout", tok)
                assert _rel(got[b].cpu().numpy(), r) <= 1e-5


def test_rauq_batch_rows_independent_and_repeatable():
    case = next(c for c in batch_fixture_cases() if c["name"] == "causal_mixed")
    att = _maps(case)
    lp, mask, lengths = torch.from_numpy(case["lp"]), torch.from_numpy(case["mask"]), torch.from_numpy(case["lengths"])
    inp, alphas = case["input_length"], case["alphas"]
    for perm in ([2, 0, 3, 1], [3, 1], [2]):
        idx = torch.tensor(perm)
        sub = tuple(tuple(t.index_select(0, idx.cuda()) for t in s) for s in att)
        for h, t in MODES:
            full = rauq_batch(lp, att, inp, t, h, alphas, mask, lengths)
            part = rauq_batch(lp[idx], sub, inp, t, h, alphas, mask[idx], lengths[idx])
            assert _bits_equal(part, full[idx.cuda()]), (perm, h, t)
            assert _bits_equal(full, rauq_batch(lp, att, inp, t, h, alphas, mask, lengths))


def test_rauq_batch_b1_without_mask_equals_rauq():
    case = next(c for c in batch_fixture_cases() if c["name"] == "llama_pad_bf16")
    att = tuple(tuple(t[:1] for t in s) for s in _maps(case))  # row 0: no padding
    lp = torch.from_numpy(case["lp"])[:1]
    for h, t in MODES:
        got = rauq_batch(lp, att, case["input_length"], t, h, case["alphas"])
        exp = RAUQ(lp if h == "rollout" else lp[0], att, case["input_length"], t, h, case["alphas"], True)
        assert _bits_equal(got[0], torch.tensor(exp, dtype=torch.float32)), (h, t)


def test_rauq_batch_real_padded_sampled_generation():
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(23)
    eos = [5, 6, 7, 8]
    cfg = transformers.LlamaConfig(vocab_size=48, hidden_size=64, intermediate_size=128, num_hidden_layers=3,
                                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256,
                                   attn_implementation="eager", pad_token_id=0)
    model = transformers.LlamaForCausalLM(cfg).cuda().eval()
    inp, pads = 16, [0, 4, 9, 2, 13]
    ids = torch.randint(11, 48, (len(pads), inp), device="cuda")
    mask = _mask(pads, inp)
    ids[mask == 0] = 0
    with torch.no_grad():
        out = model.generate(ids, attention_mask=mask, max_new_tokens=12, do_sample=True, top_k=8, eos_token_id=eos,
                             output_attentions=True, output_scores=True, return_dict_in_generate=True, pad_token_id=0)
    lp = transition_scores(out.sequences, out.scores, normalize_logits=True)
    lengths = generated_lengths(out.sequences, inp, eos)
    att = out.attentions
    assert att[0][0].shape == (len(pads), 4, inp, inp) and att[0][0].is_cuda and lengths.dtype == torch.int64
    alphas = [0.2, 0.4, 0.7]
    steps = [torch.stack(s, 1).double().cpu().numpy() for s in att]
    for h, t in MODES:
        got = rauq_batch(lp, att, inp, t, h, alphas, mask, lengths)
        assert _bits_equal(got, _one_row(att, lp, mask, lengths, inp, h, t, alphas)), (h, t)
        for b, pad in enumerate(pads):
            n = int(lengths[b])
            if n < 2 and (t == "original" or h == "rollout"):
                assert torch.isnan(got[b]).all()
                continue
            lpb = lp[b, :n].cpu().numpy()
            r, _ = restate(row_steps(steps, pad, n, b), "float32", lpb.reshape(1, -1) if h == "rollout" else lpb, inp - pad,
                           alphas, h, t)
            assert _rel(got[b].cpu().numpy(), r) <= (1e-5 if h == "rollout" else 1e-6), (h, t, b)


def test_rauq_batch_llama_8b_shape_bf16():
    """L = H = 32, bf16 causal maps, B = 4 rows, in = 512 with mixed padding, n_gen = 128 (~2.8 GB, freed at the end)."""
    L, H, inp, n_gen, alphas = 32, 32, 512, 128, [0.2, 0.4]
    pads, lengths = [0, 37, 200, 5], torch.tensor([128, 97, 128, 60])
    att = _padded_causal(L, H, inp, n_gen, pads, 8, dtype=torch.bfloat16)
    lp = torch.log(torch.rand(len(pads), n_gen, generator=torch.Generator().manual_seed(9)) * 0.9 + 0.05)
    mask = _mask(pads, inp)
    try:
        got = {(h, t): rauq_batch(lp, att, inp, t, h, alphas, mask, lengths).cpu() for h, t in MODES}
        for b, pad in enumerate(pads):
            n = int(lengths[b])
            sl = tuple(tuple((x[b:b + 1, :, pad:, pad:] if g == 0 else x[b:b + 1, :, :, pad:]) for x in att[g]) for g in range(n))
            exp = _restate_device(sl, lp[b:b + 1, :n], inp - pad, alphas)
            for h, t in MODES:
                assert _rel(got[(h, t)][b].numpy(), exp[(h, t)]) <= 1e-5, (b, h, t, got[(h, t)][b], exp[(h, t)])
    finally:
        del att
        gc.collect()
        torch.cuda.empty_cache()


# ---- the summation-order switch of gather_value at k = 512 (inputs: rauq_switch_cases.py) --------------------------------
import rauq_switch_cases as sw  # noqa: E402


@pytest.mark.parametrize("dtype", list(sw.DTYPES))
@pytest.mark.parametrize("tie", [False, True], ids=["margin", "tie"])
def test_rauq_batch_rows_on_both_sides_of_the_summation_switch(dtype, tie):
    """B = 3 left-padded rows whose k at step g is 513 + g, 510 + g and 507 + g: row 0 is always over 512 columns, row 1
    crosses 512 at its third step, row 2 (five steps) stays under it, so at each of row 2's steps a row under 512 sits next to one
    at or over it.  Every row's bits are the one-row call's on its slices, its scores meet the restatement
    of its own maps, and its chosen heads are the restatement's."""
    inp, pads = sw.BATCH["input_length"], list(sw.BATCH["pads"])
    lengths = torch.tensor(sw.BATCH["lengths"])
    steps = sw.batch_steps(dtype, 300, tie)
    att = sw.batch_tensors(steps, dtype, "cuda")
    lp = torch.from_numpy(sw.log_probs(sw.BATCH["n_gen"], 31, rows=len(pads)))
    mask = _mask(pads, inp)
    for h in HEADS:
        got = rauq_batch(lp, att, inp, "mean_all_tokens", h, sw.ALPHAS, mask, lengths)
        exp = _one_row(att, lp, mask, lengths, inp, h, "mean_all_tokens", sw.ALPHAS)
        assert _bits_equal(got, exp), (dtype, h, got, exp)
        for b, pad in enumerate(pads):
            n = int(lengths[b])
            lpb = lp[b, :n].numpy()
            r, heads = restate(row_steps(steps, pad, n, b), dtype, lpb.reshape(1, -1) if h == "rollout" else lpb, inp - pad,
                               sw.ALPHAS, h, "mean_all_tokens")
            print(f"batch row {b} {dtype} {h}: rel {_rel(got[b].cpu().numpy(), r):.2e}")
            assert _rel(got[b].cpu().numpy(), r) <= (1e-5 if h == "rollout" else 1e-6), (dtype, h, b)
            if h == "original":
                sl = tuple(tuple(t[b:b + 1, :, pad:, pad:] if g == 0 else t[b:b + 1, :, :, pad:] for t in att[g])
                           for g in range(n))
                _, got_heads = rq._gather_scores(lp[b, :n], sl, "mean_all_tokens", sw.ALPHAS, rq._HEAD_ARGMAX)
                np.testing.assert_array_equal(got_heads, heads, err_msg=f"heads of row {b}, {dtype}")
                if tie:
                    assert (np.asarray(got_heads) == sw.TIE_HEADS[0]).all()
