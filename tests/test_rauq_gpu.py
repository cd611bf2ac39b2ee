"""RAUQ on the device (csrc/rauq.hip): reference fixture parity, the input contract (host / device / strided maps, no
writes, bitwise repeatability), the two rollout routes, the Llama-3.1-8B shape against an f64 restatement, and the
structure of a real HuggingFace generation."""
import gc

import numpy as np
import pytest
import torch

from runia_core_amd.llm_uncertainty import RAUQ, rauq_uncertainty, rauq_uncertainty_mean_heads, rauq_uncertainty_rollout
from runia_core_amd.llm_uncertainty import rauq as rq
from test_rauq_host import HEADS, TOKENS, fixture_cases, restate

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _maps(case, device="cuda"):
    dt = DTYPES[case["dtype"]]
    return tuple(tuple(torch.from_numpy(s[l]).to(device=device, dtype=dt)[None] for l in range(s.shape[0]))
                 for s in (st.astype(np.float32) for st in case["steps"]))


def _call(head, tok, lp, att, inp, alphas):
    return RAUQ(lp, att, inp, tok, head, alphas, True)


def _rel(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    return float(np.max(np.abs(got - exp) / np.maximum(np.abs(exp), 1e-30)))


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c["name"])
def test_rauq_fixture_parity(case):
    att = _maps(case)
    lp = torch.from_numpy(case["lp"])
    lp2 = lp.reshape(1, -1)
    for h in HEADS:
        for t in TOKENS:
            got = _call(h, t, lp2 if h == "rollout" else lp, att, case["input_length"], case["alphas"])
            assert isinstance(got, list) and all(isinstance(v, float) for v in got)
            tol = 1e-5 if h == "rollout" else 1e-6
            assert _rel(got, case["scores"][(h, t)]) <= tol, (case["name"], h, t, got, case["scores"][(h, t)])
    for t in TOKENS:
        _, heads = rq._gather_scores(lp, att, t, case["alphas"], rq._HEAD_ARGMAX)
        np.testing.assert_array_equal(heads, case["heads"][t], err_msg=f"{case['name']} {t}")
    # ablation=False returns the first alpha's float, as the reference
    one = rauq_uncertainty(lp, att, "original", case["alphas"])
    assert isinstance(one, float) and one == _call("original", "original", lp, att, 0, case["alphas"])[0]


def _strided(att):
    """The same maps through non-contiguous views: (B, q, H, k) storage seen as (B, H, q, k), plus a column gap."""
    out = []
    for step in att:
        per = []
        for t in step:
            b, h, q, k = t.shape
            store = torch.full((b, q, h, k + 3), float("nan"), dtype=t.dtype, device=t.device)
            view = store[..., 1:k + 1].permute(0, 2, 1, 3)
            view.copy_(t)
            per.append(view)
        out.append(tuple(per))
    return tuple(out)


def test_rauq_host_device_strided_inputs_bitwise_and_untouched():
    case = next(c for c in fixture_cases() if c["name"] == "llama_bf16")
    dev = _maps(case)
    host = _maps(case, device="cpu")
    strided = _strided(dev)
    snap = [t.clone() for s in strided for t in s]
    lp = torch.from_numpy(case["lp"])
    lp2 = lp.reshape(1, -1)
    for h in HEADS:
        for t in TOKENS:
            l = lp2 if h == "rollout" else lp
            a = _call(h, t, l, dev, case["input_length"], case["alphas"])
            b = _call(h, t, l, host, case["input_length"], case["alphas"])
            c = _call(h, t, l.cuda(), strided, case["input_length"], case["alphas"])
            d = _call(h, t, l, strided, case["input_length"], case["alphas"])
            assert a == b == c == d, (h, t, a, b, c, d)
    torch.cuda.synchronize()
    for t0, t1 in zip(snap, (t for s in strided for t in s)):
        assert torch.equal(t0, t1)
        assert t1.is_cuda


def _causal(l_, h_, inp, n_gen, seed, dtype=torch.float32, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    mask = torch.triu(torch.ones(inp, inp, dtype=torch.bool, device=device), 1)
    steps = []
    for s in range(n_gen):
        per = []
        for _ in range(l_):
            if s == 0:
                x = torch.randn(1, h_, inp, inp, generator=g, device=device) * 2
                x = x.masked_fill(mask, float("-inf"))
            else:
                x = torch.randn(1, h_, 1, inp + s, generator=g, device=device) * 2
            per.append(torch.softmax(x, -1).to(dtype))
        steps.append(tuple(per))
    return tuple(steps)


def _np_steps(att):
    return [torch.stack([t[0] for t in step]).double().cpu().numpy() for step in att]


def test_rauq_rollout_routes():
    inp, n_gen, alphas = 12, 9, [0.2, 0.4, 0.9]
    att = _causal(4, 3, inp, n_gen, 5)
    lp = torch.log(torch.rand(1, n_gen, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.05)
    for tok in TOKENS:
        info = {}
        got = rq._rollout_scores(lp, att, tok, inp, alphas, info)
        assert info["route"] == ("one_pass" if tok == "original" else "chain") and not info["upper_nonzero"]
        exp, _ = restate(_np_steps(att), "float32", lp.numpy(), inp, alphas, "rollout", tok)
        assert _rel(got, exp) <= 1e-5, (tok, got, exp)
    # one entry above the prompt block's diagonal: the general chain, same restatement
    bent = [list(s) for s in att]
    x = bent[0][2].clone()
    x[0, 1, 3, 7] = 0.25
    bent[0][2] = x
    bent = tuple(tuple(s) for s in bent)
    for tok in TOKENS:
        info = {}
        got = rq._rollout_scores(lp, bent, tok, inp, alphas, info)
        assert info["route"] == "chain" and info["upper_nonzero"]
        assert info["chain_rows"] == (n_gen if tok == "original" else 1)
        exp, _ = restate(_np_steps(bent), "float32", lp.numpy(), inp, alphas, "rollout", tok)
        assert _rel(got, exp) <= 1e-5, (tok, got, exp)
    # the reference's broadcast mocks (one query row at step 0) take the chain
    case = next(c for c in fixture_cases() if c["name"] == "mock_rollout")
    info = {}
    rq._rollout_scores(torch.from_numpy(case["lp"]).reshape(1, -1), _maps(case), "original", case["input_length"], [0.4], info)
    assert info["route"] == "chain" and info["upper_nonzero"]


def _restate_device(att, lp, inp, alphas):
    """f64 restatement on the device for maps too large for the host one (test-only torch): the six combinations."""
    L = len(att[0])
    n_gen = len(att)
    T = inp + n_gen
    n = lp.shape[1]
    probs = lp.double().exp().reshape(-1).cuda()

    def rec(series):  # (L', N)
        out = []
        for a in alphas:
            conf = torch.empty_like(series)
            conf[:, 0] = probs[0]
            for i in range(1, series.shape[1]):
                conf[:, i] = a * probs[i] + (1 - a) * series[:, i] * conf[:, i - 1]
            out.append(float((-conf.log().mean(1)).max()))
        return out

    res = {}
    w_orig = torch.stack([torch.stack([att[g][l][0, :, 0, -2].double() for g in range(1, n_gen)], -1) for l in range(L)])
    rows = torch.stack([torch.stack([att[g][l][0, :, 0, :].double().mean(-1) for g in range(n_gen)], -1) for l in range(L)])
    w_mean = rows.float().to(att[0][0].dtype).double()  # the row mean rounded to the map dtype
    for tok, w in (("original", w_orig), ("mean_all_tokens", w_mean)):
        heads = w[:, :, 1:].mean(-1).argmax(1)
        res[("original", tok)] = rec(w[torch.arange(L), heads])
        res[("mean_heads", tok)] = rec(w.mean(1))
    r_orig = torch.eye(T, dtype=torch.float64, device="cuda")[T - n:]
    r_mean = torch.full((1, T), 1.0 / T, dtype=torch.float64, device="cuda")
    for l in range(L - 1, -1, -1):
        m = torch.zeros((T, T), dtype=torch.float64, device="cuda")
        m[:inp, :inp] = att[0][l][0].double().mean(0)
        for g in range(1, n_gen):
            m[inp + g, :inp + g] = att[g][l][0, :, 0, :].double().mean(0)
        m += torch.eye(T, dtype=torch.float64, device="cuda")
        a = m / m.sum(-1, keepdim=True)
        r_orig, r_mean = r_orig @ a, r_mean @ a
        del m, a
    res[("rollout", "original")] = rec(r_orig[torch.arange(n), T - n - 1 + torch.arange(n)][None])
    res[("rollout", "mean_all_tokens")] = rec(r_mean[:, T - n:])
    return res


def test_rauq_llama_8b_shape_bf16():
    """L = H = 32, in = 2048, n_gen = 256, bf16 causal maps (~9.7 GB of HBM, freed at the end)."""
    L, H, inp, n_gen, alphas = 32, 32, 2048, 256, [0.2, 0.4]
    att = _causal(L, H, inp, n_gen, 8, dtype=torch.bfloat16)
    lp = torch.log(torch.rand(1, n_gen, generator=torch.Generator().manual_seed(9)) * 0.9 + 0.05)
    try:
        exp = _restate_device(att, lp, inp, alphas)
        for h in HEADS:
            for t in TOKENS:
                info = {}
                if h == "rollout":
                    got = rq._rollout_scores(lp, att, t, inp, alphas, info)
                    assert info["route"] == ("one_pass" if t == "original" else "chain")
                else:
                    got = _call(h, t, lp[0], att, inp, alphas)
                assert _rel(got, exp[(h, t)]) <= 1e-5, (h, t, got, exp[(h, t)])
    finally:
        del att
        gc.collect()
        torch.cuda.empty_cache()


def test_rauq_real_hf_generation():
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(21)
    cfg = transformers.LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=3,
                                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256,
                                   attn_implementation="eager")
    model = transformers.LlamaForCausalLM(cfg).cuda().eval()
    inp, n_gen = 20, 12
    ids = torch.randint(3, 128, (1, inp), device="cuda")
    with torch.no_grad():
        out = model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=n_gen, min_new_tokens=n_gen,
                             do_sample=False, output_attentions=True, output_scores=True, return_dict_in_generate=True,
                             pad_token_id=0)
        lp = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True).float()
    att = out.attentions
    assert att[0][0].shape == (1, 4, inp, inp) and att[1][0].shape == (1, 4, 1, inp + 1) and att[0][0].is_cuda
    steps = _np_steps(att)
    alphas = [0.2, 0.4, 0.7]
    for h in HEADS:
        for t in TOKENS:
            info = {}
            if h == "rollout":
                got = rq._rollout_scores(lp, att, t, inp, alphas, info)
                assert info["route"] == ("one_pass" if t == "original" else "chain") and not info["upper_nonzero"]
            else:
                got = _call(h, t, lp[0], att, inp, alphas)
            exp, _ = restate(steps, "float32", lp.cpu().numpy(), inp, alphas, h, t)
            assert _rel(got, exp) <= (1e-5 if h == "rollout" else 1e-6), (h, t, got, exp)


# ---- the summation-order switch of gather_value at k = 512 (inputs: rauq_switch_cases.py) --------------------------------
import rauq_switch_cases as sw  # noqa: E402


def _switch_check(steps, dtype, inp, seed):
    """"mean_all_tokens" in the three head modes against the restatement, the chosen heads included."""
    n_gen = len(steps)
    att = sw.one_row_tensors(steps, dtype, "cuda")
    lp = torch.from_numpy(sw.log_probs(n_gen, seed))
    steps64 = [s.astype(np.float64) for s in steps]
    out = {}
    for h in HEADS:
        got = _call(h, "mean_all_tokens", lp if h == "rollout" else lp[0], att, inp, sw.ALPHAS)
        exp, heads = restate(steps64, dtype, lp.numpy() if h == "rollout" else lp[0].numpy(), inp, sw.ALPHAS, h,
                             "mean_all_tokens")
        print(f"k {inp}..{inp + n_gen - 1} {dtype} {h}: rel {_rel(got, exp):.2e}")
        assert _rel(got, exp) <= (1e-5 if h == "rollout" else 1e-6), (h, dtype, inp, got, exp)
        if h == "original":
            _, got_heads = rq._gather_scores(lp[0], att, "mean_all_tokens", sw.ALPHAS, rq._HEAD_ARGMAX)
            np.testing.assert_array_equal(got_heads, heads, err_msg=f"heads, k from {inp}, {dtype}")
            out["heads"] = np.asarray(got_heads)
        out[h] = got
    return out


@pytest.mark.parametrize("dtype", list(sw.DTYPES))
@pytest.mark.parametrize("k", sw.SWITCH_KS)
def test_rauq_row_means_at_the_summation_switch(k, dtype):
    """Prompt lengths that put the row means' k at 510, 511, 512 and 513: both sides of the switch from torch's cascade
    order to the wave sum.  The heads' gains keep the head choice off a near-tie (asserted in test_rauq_host.py)."""
    _switch_check(sw.one_row_steps(k, 3, dtype, 100 + k), dtype, k, k)


@pytest.mark.parametrize("dtype", list(sw.DTYPES))
@pytest.mark.parametrize("tie", [False, True], ids=["margin", "tie"])
def test_rauq_generation_crossing_the_summation_switch(dtype, tie):
    """Six steps from k = 509: the means of one series come from both summation orders.  With head 3 a copy of head 1
    and both largest, the first index wins, as the reference's argmax."""
    inp, n_gen = sw.GENERATION["input_length"], sw.GENERATION["n_gen"]
    out = _switch_check(sw.one_row_steps(inp, n_gen, dtype, 200, tie), dtype, inp, 7)
    if tie:
        assert (out["heads"] == sw.TIE_HEADS[0]).all()


def _gathered_means(ks):
    """w (L, H, len(ks)) f32 of runia_rauq_gather in "mean_all_tokens" on one step per k (rauq._gather_scores' own call)."""
    from runia_core_amd import _hip

    att = sw.mean_steps(ks, "cuda")
    lib = _hip.load_library()
    table, keep = rq._map_table(att, torch.device("cuda"), first_row_only=True)
    w = torch.full((sw.MEAN_L, sw.MEAN_H, len(ks)), float("nan"), dtype=torch.float32, device="cuda")
    _hip._check(lib.runia_rauq_gather(table.data_ptr(), rq._DTYPE_CODES[torch.float32], len(ks), sw.MEAN_L, sw.MEAN_H, 1,
                                      w.data_ptr(), _hip._stream()), "runia_rauq_gather")
    torch.cuda.synchronize()
    del keep
    return w.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_rauq_gathered_row_means_are_bitwise_torchs_below_512():
    """The kernel header's promise for rows of k < 512 columns, up to 510 and 511: the gathered f32 means are torch's own
    CPU mean(-1) of the same rows, bit for bit (and the oracle's restatement of that order).  These rows' bits differ
    under the wave order (test_rauq_host.py), so a switch one column early is seen."""
    from test_rauq_host import f32_mean_lastdim

    w = _gathered_means(sw.MEAN_KS_CASCADE)
    for i, k in enumerate(sw.MEAN_KS_CASCADE):
        a = sw.mean_rows(k)
        np.testing.assert_array_equal(_bits(w[:, :, i]), _bits(torch.from_numpy(a).mean(-1).numpy()[..., 0]), err_msg=f"torch, k = {k}")
        np.testing.assert_array_equal(_bits(w[:, :, i]), _bits(f32_mean_lastdim(a)[..., 0]), err_msg=f"oracle, k = {k}")


def test_rauq_gathered_row_means_are_bitwise_the_wave_sum_from_512():
    """From 512 columns on the documented order: lane j adds the elements j, j + 64, ... in index order, then the xor
    butterfly 32 .. 1.  These rows' bits differ under torch's cascade order, so a switch one column late is seen."""
    w = _gathered_means(sw.MEAN_KS_WAVE)
    for i, k in enumerate(sw.MEAN_KS_WAVE):
        np.testing.assert_array_equal(_bits(w[:, :, i]), _bits(sw.wave_order_mean(sw.mean_rows(k))[..., 0]), err_msg=f"k = {k}")
