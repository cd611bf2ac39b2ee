"""The logit-lens kernel (csrc/logit_lens.hip) against the f64 reference of logit_lens_cases, within its derived bounds.

Every test prints its largest |error| / bound.  Largest value seen on an MI355X: 0.178 (d = 1, bf16; 0.020 otherwise), and
0.003 of the tolerance for the final layer against generation_scores."""
import numpy as np
import pytest
import torch

import logit_lens_cases as cases
from runia_core_amd import _hip
from runia_core_amd.llm_uncertainty import compute_uncertainties_batch, generated_lengths, generation_scores
from runia_core_amd.llm_uncertainty.logit_lens import (LENS_GROUP_PLANES, LENS_MAX_SPLIT, LENS_VOCAB_STEP, LENS_VOCAB_TILE,
                                                        lens_split, logit_lens)

pytestmark = pytest.mark.gpu
STEP, GROUP = LENS_VOCAB_STEP, LENS_GROUP_PLANES
SPLIT_V = 2 * STEP * LENS_MAX_SPLIT  # two steps per chunk at the largest split


def score(x, w, tokens=None, final=-1):  # runia_lens_scores on device copies of x (planes, N, d), w (V, d) (a device w: in place)
    xd, wd = x.cuda().contiguous(), w if w.is_cuda else w.cuda()
    planes, n, d = xd.shape
    v = wd.shape[0]
    f = torch.empty((5, planes, n), dtype=torch.float32, device="cuda")
    top = torch.empty((planes, n), dtype=torch.int32, device="cuda")
    tok = None if tokens is None else tokens.cuda()
    ws = _hip.workspace(_hip.query("runia_lens_workspace_bytes", planes, n, v, d), xd.device)
    _hip.launch("runia_lens_scores", xd.data_ptr(), wd.data_ptr(), wd.stride(0) if v > 1 else d, _hip.ELEM_DTYPE_CODES[xd.dtype],
                planes, n, v, d, _hip._ptr(tok), final, f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(),
                top.data_ptr(), f[4].data_ptr(), ws.data_ptr(), ws.numel())
    out = {k: f[i].cpu().numpy() for i, k in enumerate(cases.FIELDS)}
    out["top_token"] = top.cpu().numpy()
    return out


def check(out, ref, what):
    worst = 0.0
    for k in cases.FIELDS:
        want, got = ref[k], out[k].astype(np.float64)
        assert (np.isnan(want) == np.isnan(got)).all(), (what, k)
        ok = ~np.isnan(want)
        if ok.any():
            worst = max(worst, float((np.abs(got - want)[ok] / ref["bound_" + k][ok]).max()))
    print(f"{what}: max |error| / bound = {worst:.3f}")
    assert worst <= 1.0, what
    assert ref["gap_ok"] and (out["top_token"] == ref["top_token"]).all(), what


def same_bits(a, b, rows=slice(None)):
    return all(np.array_equal(a[k][:, rows], b[k], equal_nan=True) for k in cases.FIELDS + ("top_token",))


MID = dict(planes=3, N=40, V=200, d=48)
EDGES = ([dict(MID, V=v) for v in (1, 31, 32, 33, STEP - 1, STEP + 1, 2 * STEP + 3)] +
         [dict(MID, d=d) for d in (1, 15, 16, 17, 33, 100)] + [dict(MID, N=n) for n in (1, 31, 32, 33, 70)] +
         [dict(MID, planes=p) for p in (1, 2, GROUP, GROUP + 1)])
CORNERS = [dict(planes=GROUP + 1, N=33, V=2 * STEP + 3, d=17), dict(planes=2, N=70, V=STEP + 1, d=100)]


@pytest.mark.parametrize("shape,dtype", [(s, "bf16") for s in EDGES + CORNERS] + [(s, t) for s in CORNERS for t in ("f16", "f32")])
def test_edge_shapes(shape, dtype):
    final = shape["planes"] - 1
    x, w, tok, ref = cases.make(7, dtype=dtype, final=final, **shape)
    out = score(x, w, tok, final)
    check(out, ref, f"{shape} {dtype}")
    if shape["V"] == 1:
        assert (out["entropy"] == 0).all() and (out["log_prob"] == 0).all()


def test_vocabulary_split_bounds_and_bits():  # S depends on V alone: rows alone, inside a larger call and twice: the same bits
    assert lens_split(SPLIT_V) == LENS_MAX_SPLIT > 1 and lens_split(3 * STEP) == 3
    x, w, tok, ref = cases.make(11, 2, 37, SPLIT_V, 16, final=1)
    big = score(x, w, tok, 1)
    check(big, ref, "split")
    assert same_bits(big, score(x, w, tok, 1))
    assert same_bits(big, score(x[:, :3].contiguous(), w, tok[:3], 1), slice(0, 3))


@pytest.mark.parametrize("lo,hi", [(5, 9), (5, STEP + 5), (5, 2 * STEP + 5)], ids=["one-tile", "two-steps", "two-chunks"])
def test_ties_take_the_lower_id(lo, hi):  # a duplicated, winning weight row (two steps per chunk at this V)
    assert lo // LENS_VOCAB_TILE == 0 and (hi // STEP) // 2 == (1 if hi >= 2 * STEP else 0)
    x, w, _, _ = cases.make(13, 2, 33, SPLIT_V, 16, tokens=False)
    w[lo] = w[hi] = w[lo] * 8  # (exact) the pair wins every row where its logit was above about 1.5
    wins = (x.double() @ w.double().T).argmax(-1) == lo
    assert wins.any()
    out = score(x, w)
    assert (out["top_token"][wins.numpy()] == lo).all()


def test_kl_against_the_final_plane():
    x, w, tok, _ = cases.make(17, GROUP + 1, 33, 3 * STEP + 7, 24)
    x[1] = x[GROUP]  # a plane equal to the final plane; the final plane lies in the second plane group of a call without one
    ref = cases.reference(x, w, tok, GROUP)
    out = score(x, w, tok, GROUP)
    check(out, ref, "kl")
    assert (np.abs(out["kl_final"][[1, GROUP]]) <= ref["bound_kl_final"][[1, GROUP]]).all()
    assert np.isnan(score(x, w, tok, -1)["kl_final"]).all()
    first = score(x, w, tok, 0)  # the final plane first: the other planes fill two groups behind it
    check(first, cases.reference(x, w, tok, 0), "kl, final plane 0")


def test_tokens_absent_and_in_the_last_tile():
    x, w, tok, _ = cases.make(19, 2, 34, STEP + 3, 20)
    tok[0], tok[1], tok[2] = -1, STEP + 2, STEP  # none | the last id of the partly filled tile | its first
    out = score(x, w, tok)
    check(out, cases.reference(x, w, tok), "tokens")
    assert np.isnan(out["log_prob"][:, 0]).all() and np.isnan(score(x, w)["log_prob"]).all()


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_bad_state_stays_in_its_row_and_its_kl_partners(value):
    x, w, tok, _ = cases.make(23, 3, 35, 2 * STEP + 3, 40)
    clean = score(x, w, tok, 2)
    x[0, 4, 7] = x[2, 9, 39] = value  # an ordinary row | a row of the final plane
    out = score(x, w, tok, 2)
    for k in cases.FIELDS:
        want = clean[k].copy()
        want[0, 4] = want[2, 9] = np.nan
        if k == "kl_final":
            want[:, 9] = np.nan
        assert np.array_equal(out[k], want, equal_nan=True), k
    assert (out["top_token"][[0, 2], [4, 9]] == -1).all() and (out["top_token"] != clean["top_token"]).sum() == 2


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_strided_weight_view_and_host_inputs(dtype):
    x, w, tok, _ = cases.make(29, 2, 33, STEP + 9, 40, dtype=dtype)
    wide = torch.zeros((w.shape[0], 61), dtype=w.dtype, device="cuda")
    view = wide[:, 3:43]  # starts off a 16-byte boundary, rows 61 elements apart
    view.copy_(w)
    assert view.data_ptr() % 16 and not view.is_contiguous()
    assert same_bits(score(x, view, tok, 1), score(x, w, tok, 1))
    hs = tuple(p[None] for p in x)  # forward form, one batch row: host inputs against device inputs
    kw = dict(sequences=torch.zeros((1, 34), dtype=torch.int64), windows=[[0, 33]])
    host, dev = logit_lens(hs, w, [0], **kw), logit_lens(tuple(h.cuda() for h in hs), w.cuda(), [0], **kw)
    assert host.lse.is_cuda and all(torch.equal(a.cpu(), b.cpu()) or (a.isnan() & b.isnan()).all() for a, b in zip(host, dev))


def test_forms_ragged_rows_and_empty_windows():  # generate() = forward form; ragged rows = their one-row calls; empty = NaN
    torch.manual_seed(5)
    B, P, G, d, V, L = 3, 5, 4, 24, 70, 3
    full = [torch.randn(B, P + G - 1, d, device="cuda").bfloat16() for _ in range(L)]
    w = (torch.randn(V, d, device="cuda") * 0.6).bfloat16()
    seq = torch.randint(0, V, (B, P + G), device="cuda")
    gen = tuple(tuple(t[:, :P] if g == 0 else t[:, P + g - 1:P + g] for t in full) for g in range(G))
    mask = torch.tensor([[1] * 5, [0, 0, 1, 1, 1], [0, 1, 1, 1, 1]])
    lengths = torch.tensor([4, 2, 3])
    kw = dict(sequences=seq, attention_mask=mask, lengths=lengths)
    a = logit_lens(gen, w, [0, 1], **kw)
    b = logit_lens(tuple(full), w, [0, 1], input_length=P, sequences=seq, lengths=lengths)
    same = lambda s, t: bool(((s == t) | (s.isnan() & t.isnan())).all())  # noqa: E731
    assert all(same(s, t) for s, t in zip(a, b))
    assert a.lse.shape == (B, 2, 4) and a.lse[1, :, 2:].isnan().all() and (a.top_token[1, :, 2:] == -1).all()
    for r in range(B):
        one = logit_lens(tuple(tuple(t[r:r + 1] for t in step) for step in gen), w, [0, 1], sequences=seq[r:r + 1],
                         attention_mask=mask[r:r + 1], lengths=lengths[r:r + 1])
        n = int(lengths[r])
        assert all(same(s[r:r + 1, :, :n] if s.dim() == 3 else s[r:r + 1], t) for s, t in zip(a, one)), r
    e = logit_lens(gen, w, [0], sequences=seq, windows=[[4, 2], [0, 0], [4, 1]], attention_mask=mask)
    assert e.mean_entropy[1].isnan().all() and e.mean_kl_final[1].isnan().all() and not e.mean_entropy[[0, 2]].isnan().any()


def test_real_model_requests_and_the_final_layer():
    from transformers import GenerationConfig

    from test_llm_pipeline_gpu import PROMPTS, IdTok, RecordingModel, tiny_llama

    class Model(RecordingModel):  # what the lens requests read of a model, passed through
        def __init__(self, model):
            super().__init__(model)
            self.config, self.base_model, self.get_output_embeddings = model.config, model.base_model, model.get_output_embeddings

    eos = [5, 6, 7]
    model = Model(tiny_llama(eos=eos, seed=29).float())
    cfg = GenerationConfig(max_new_tokens=8, pad_token_id=0, eos_token_id=eos)
    reqs = [{"method_name": "lens_entropy"}, {"method_name": "lens_log_prob", "layer": 9}, {"method_name": "lens_kl", "layer": 3}]
    _, scores = compute_uncertainties_batch(model, IdTok(), PROMPTS, reqs, cfg, 2)
    det = model.outs[0]
    in_len = int(det.sequences.shape[1] - len(det.scores))
    lengths = generated_lengths(det.sequences, in_len, eos).clamp_max(len(det.scores))
    kw = dict(sequences=det.sequences, norm=model.base_model.norm, attention_mask=det.sequences[:, :in_len] != 0, lengths=lengths)
    weight = model.get_output_embeddings().weight
    direct = logit_lens(det.hidden_states, weight, [15, 9, 3, 16], **kw)
    assert torch.equal(scores["lens_entropy"], direct.mean_entropy[:, 0].cpu())
    assert torch.equal(scores["lens_log_prob_9"], direct.mean_log_prob[:, 1].cpu())
    assert torch.equal(scores["lens_kl_3"], direct.mean_kl_final[:, 2].cpu())
    gs = generation_scores(det.sequences, det.scores).log_probs.double().cpu()
    worst = 0.0
    for b, n in enumerate(lengths.tolist()):
        x = torch.stack([det.hidden_states[0][16][b, in_len - 1]] + [det.hidden_states[g][16][b, 0] for g in range(1, n)])
        ref = cases.reference(x[None].cpu(), weight.detach().cpu(), det.sequences[b, in_len:in_len + n].cpu(), 0)
        got = direct.log_prob[b, 3, :n].double().cpu()
        tol = 2 * torch.from_numpy(ref["bound_log_prob"][0]) + 2.0 ** -20 * (1 + gs[b, :n].abs())
        worst = max(worst, float(((got - gs[b, :n]).abs() / tol).max()))
        assert (direct.kl_final[b, 3, :n].double().cpu().abs() <= torch.from_numpy(ref["bound_kl_final"][0])).all()
    print(f"final layer log_prob against generation_scores: max |error| / tolerance = {worst:.3f}")
    assert worst <= 1.0
