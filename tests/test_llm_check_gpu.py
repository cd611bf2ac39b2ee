"""LLM-Check hidden and attention scores on the device (csrc/llm_check.hip) against the NumPy references of
tests/llm_check_cases.py, at the tile (64), chunk (32), strip (16) and panel edges; bit equality across batch rows, layouts and
input forms.  The hidden-score bound is 16 * max(|f64 reference - longdouble|, 2^-50 |score|) around the longdouble value; every
test prints its largest |error| / bound.

Windows longer than the states are wide (d < T) go through the d x d form of the determinant, the others through the T x T form:
both are crossed here, and the layout, input-form and NaN tests run in each.  Measured on one MI355X: every case lies within
0.08 of its bound (largest: T = 63, d = 33 at 0.072)."""
import numpy as np
import pytest
import torch

import llm_check_cases as cases
from runia_core_amd.llm_uncertainty import attention_score, hidden_score, llm_check_scores

pytestmark = pytest.mark.gpu


def states(t, d, seed=0, batch=1):
    return np.random.default_rng([seed, t, d]).standard_normal((batch, t, d)).astype(np.float32)


def score(z, **kw):
    """hidden_score of (B, T, d) states as the one layer of a forward pass -> (B,) f64 on the host."""
    x = z if isinstance(z, torch.Tensor) else torch.from_numpy(z).cuda()
    return hidden_score((x,), (0,), **kw).cpu().numpy()[:, 0]


def check(got, z, what):
    ratio = cases.hidden_ratio(got, z)
    print(f"{what}: |error| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


EDGES = sorted({(t, 33) for t in (1, 2, 15, 16, 17, 63, 64, 65, 129, 193)} | {(65, d) for d in (1, 31, 32, 33, 100)} |
               {(1, 1), (64, 32), (129, 31), (193, 100), (193, 200)})  # (193, 200): four panels of the T x T form


@pytest.mark.parametrize("t,d", EDGES)
def test_hidden_score_at_tile_chunk_and_panel_edges(t, d):
    z = states(t, d)
    got = score(z)[0]
    check(got, z[0], f"T={t} d={d}")
    if d == 1:  # centring leaves zeros
        assert abs(got - np.log(cases.ALPHA)) <= 16 * 2.0 ** -50 * abs(np.log(cases.ALPHA))


def test_ragged_batch_matches_and_equals_the_one_row_calls():
    lens, pads, starts, total = (1, 16, 17, 64, 130), (3, 0, 7, 1, 2), (5, 2, 9, 30, 4), 140
    layers = [torch.from_numpy(states(total, 40, seed=s, batch=5)).cuda() for s in (1, 2)]
    mask = torch.tensor([[0] * p + [1] * (total - p) for p in pads])
    windows = [[s, n] for s, n in zip(starts, lens)]
    got = hidden_score(tuple(layers), (0, 1), attention_mask=mask, windows=windows)
    assert got.shape == (5, 2) and got.dtype == torch.float64 and got.is_cuda
    for b, (s, n) in enumerate(windows):
        one = hidden_score(tuple(x[b:b + 1] for x in layers), (0, 1), windows=[[s, n]])
        assert torch.equal(one[0], got[b]), b
        for l in range(2):
            check(float(got[b, l]), layers[l][b, s:s + n].cpu().numpy(), f"row {b} layer {l}")
    with pytest.raises(ValueError):
        hidden_score(tuple(layers), (0,), attention_mask=mask, windows=[[2, 4]] + windows[1:])  # into row 0's padding
    windows[2][1] = 0
    assert bool(hidden_score(tuple(layers), (0,), windows=windows).isnan()[:, 0].cpu().tolist() == [False, False, True, False, False])


# d > T: the T x T form every LLM shape takes (16-byte and element loads of StateSrc); d < T: the d x d form (FeatureSrc)
@pytest.mark.parametrize("d", [100, 50])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_dtypes_and_strided_views_give_the_bits_of_contiguous_copies(dtype, d):
    t = 70
    wide = torch.from_numpy(states(2 * t, 2 * d + 3, seed=3, batch=4)).to(dtype).cuda()
    view = wide[::2, ::2, 3:3 + d]  # batch- and row-strided, a slice of a wider d that starts off a 16-byte boundary
    assert not view.is_contiguous() and view.stride(2) == 1
    got = score(view)
    assert np.array_equal(got, score(view.contiguous()))
    assert np.array_equal(got, score(view.cpu()))  # host states: one upload
    for b in range(2):
        check(got[b], view[b].float().cpu().numpy(), f"{dtype} row {b}")


@pytest.mark.parametrize("d", [80, 24])  # the T x T form and the d x d form
def test_generate_form_equals_forward_form(d):
    prompt, steps, heads = 5, 70, 2
    n_pos = prompt + steps - 1
    rng = np.random.default_rng(4)
    x = torch.from_numpy(states(n_pos, d, seed=4, batch=2)).cuda()
    a = torch.from_numpy(cases.causal_maps(rng, 2, heads, n_pos)).cuda()
    gen_x = ((x[:, :prompt],),) + tuple((x[:, prompt + g - 1:prompt + g],) for g in range(1, steps))
    gen_a = ((a[:, :, :prompt, :prompt],),) + tuple((a[:, :, prompt + g - 1:prompt + g, :prompt + g],) for g in range(1, steps))
    lengths = [steps, 40]
    fwd = llm_check_scores((x,), (a,), (0,), per_head=True, input_length=prompt, lengths=[n - 1 for n in lengths])
    gen = llm_check_scores(gen_x, gen_a, (0,), per_head=True, lengths=lengths)
    assert torch.equal(fwd.hidden_score, gen.hidden_score) and torch.equal(fwd.attention_score, gen.attention_score)
    check(float(gen.hidden_score[0, 0]), x[0, prompt:].cpu().numpy(), "generate form")  # T = 69: the window crosses 64
    assert bool(hidden_score(gen_x, (0,), lengths=[1, 2]).isnan().cpu().tolist() == [[True], [False]])  # an empty window


def conditioning_cases():
    z = states(40, 48, seed=5)[0]
    rank3 = z[np.random.default_rng(5).integers(0, 3, 40)]  # repeated tokens: most eigenvalues equal alpha
    big = z.copy()
    big[:, 7] *= 1000.0
    return {"rank 3": rank3, "offset 1000": z + np.float32(1000.0), "one large feature": big}


@pytest.mark.parametrize("name", ["rank 3", "offset 1000", "one large feature"])
def test_hidden_score_conditioning(name):
    z = conditioning_cases()[name]
    check(score(z[None])[0], z, name)


@pytest.mark.parametrize("t", [1, 63, 64, 65, 300])
def test_attention_score_per_head_and_zero_diagonal(t):
    heads = 3
    a = cases.causal_maps(np.random.default_rng(t), 1, heads, t)
    per_head, total, abs_sum = cases.attention_ref(a[0])
    bound = 4 * t * heads * 2.0 ** -53 * abs_sum
    dev = torch.from_numpy(a).cuda()
    got_h = attention_score((dev,), (0,), per_head=True).cpu().numpy()[0, 0]
    got = float(attention_score((dev,), (0,))[0, 0])
    err = max(np.abs(got_h - per_head).max(), abs(got - total))
    print(f"T={t}: attention |error| / bound = {err / bound if bound else 0.0:.3f}")
    assert got_h.shape == (heads,) and err <= bound
    dev[0, 1, t // 2, t // 2] = 0.0
    got_h = attention_score((dev,), (0,), per_head=True).cpu().numpy()[0, 0]
    assert got_h[1] == -np.inf and np.isfinite(got_h[[0, 2]]).all()
    assert float(attention_score((dev,), (0,))[0, 0]) == -np.inf


@pytest.mark.parametrize("d", [90, 20])  # the T x T form and the d x d form
def test_nan_state_stays_in_its_row(d):
    x = torch.from_numpy(states(70, d, seed=6, batch=3)).cuda()
    clean = score(x[[0, 2]])
    x[1, 33, 4] = float("nan")
    got = score(x)
    assert np.isnan(got[1]) and np.array_equal(got[[0, 2]], clean)


def test_pipeline_requests_equal_the_direct_calls():
    from transformers import GenerationConfig

    from runia_core_amd.llm_uncertainty import compute_uncertainties_batch, generated_lengths
    from test_llm_pipeline_gpu import PROMPTS, IdTok, RecordingModel, tiny_llama

    eos = [5, 6, 7]
    model = RecordingModel(tiny_llama(eos=eos, seed=29))
    cfg = GenerationConfig(max_new_tokens=10, pad_token_id=0, eos_token_id=eos)
    reqs = [{"method_name": "hidden_score"}, {"method_name": "attention_score"}, {"method_name": "hidden_score", "layer": 3}]
    _, scores = compute_uncertainties_batch(model, IdTok(), PROMPTS, reqs, cfg, 4)
    (det,) = model.outs  # no sampled generation
    in_len = int(det.sequences.shape[1] - len(det.scores))
    tok = IdTok()
    tok.padding_side = "left"
    common = dict(attention_mask=tok(PROMPTS)["attention_mask"], lengths=generated_lengths(det.sequences, in_len, eos))
    assert set(scores) == {"hidden_score", "attention_score", "hidden_score_3"}
    want = {"hidden_score": hidden_score(det.hidden_states, (15,), **common),
            "hidden_score_3": hidden_score(det.hidden_states, (3,), **common),
            "attention_score": attention_score(det.attentions, (15,), **common)}
    for key, w in want.items():  # (a row that stops at its first token has an empty window: NaN in both)
        got, w = scores[key], w[:, 0].cpu()
        assert got.dtype == torch.float64 and bool(((got == w) | (got.isnan() & w.isnan())).all()), key
    assert bool(scores["hidden_score"].isfinite().any())
