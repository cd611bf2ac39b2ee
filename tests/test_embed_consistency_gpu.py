"""Embedding consistency on the device (csrc/cons_embed.hip) against the f64 restatement of tests/embed_consistency_cases.py:
every coverage entry within the derived bound, every similarity within twice it, at the row-block and column-tile (128), matrix
tile (32), stage (32 / 16 features) and load (8 / 4 features) edges; bit equality across input forms, batches and layouts.  Every
test prints its largest |error| / bound.  d = 513 / 520 (bf16) and 260 (f32) reach the second feature block of the mean kernel
and the second trip of the norm kernel's loop.

Measured on one MI355X: every f16 / bf16 case lies within 0.003 of its bound (the operands go to the matrix cores as hi + lo
pairs of the element type), the f32 cases within 0.051 (the small corner without centring).  With ONE rounding per operand the
same cases read up to 0.54, and the small f16 corner with centring 1.353 - the self-coverage of a one-token sample moves by up
to 2 x 2^-11 - which is why the kernel carries the pair."""
import numpy as np
import pytest
import torch

import embed_consistency_cases as cases
from runia_core_amd.llm_uncertainty import embedding_consistency_scores, embedding_similarity

pytestmark = pytest.mark.gpu


def run(x, windows, k, **kw):
    out = embedding_similarity((x,), k, 0, windows=windows, **kw)
    assert out.coverage.dtype == torch.float64 and out.n.tolist() == [n for _, n in windows]
    return {"coverage": out.coverage.cpu().numpy(), "similarity": out.similarity.cpu().numpy()}


def check(x, windows, k, dtype, what, center=True):
    got = run(x.cuda(), windows, k, center=center)
    ratio = cases.worst_ratio(got, cases.reference(x, windows, k, dtype, center))
    print(f"{what}: |error| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    return got


MID = dict(groups=2, k=3, n=40, d=48)
EDGES = ([dict(MID, n=n) for n in (1, 31, 32, 33, 65, 129)] + [dict(MID, d=d) for d in (1, 15, 16, 17, 33, 100, 513, 520)] +
         [dict(MID, k=k) for k in (2, 3, 5)] + [dict(MID, groups=g) for g in (1, 3)])


@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "G{groups}-K{k}-n{n}-d{d}".format(**s))
def test_ragged_groups_at_block_tile_and_stage_edges(shape):
    x, windows = cases.make(0, dtype="bf16", **shape)
    check(x, windows, shape["k"], "bf16", str(shape))


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", [dict(groups=1, k=2, n=3, d=5), dict(groups=3, k=5, n=129, d=100), dict(groups=1, k=2, n=5, d=260)],
                         ids=["small", "large", "wide"])  # wide: the f32 norm loop (256 features a trip) makes a second trip
def test_corners_in_every_dtype(shape, dtype, center):
    x, windows = cases.make(1, dtype=dtype, **shape)
    check(x, windows, shape["k"], dtype, f"{shape} {dtype} center={center}", center)


def test_generate_form_equals_forward_form():
    prompt, steps, k = 4, 140, 3
    x, _ = cases.make(2, 2, k, prompt + steps - 4, 40, ragged=False)  # (6, prompt + steps - 1, 40)
    lengths = [steps, 1, 130, 129, 2, 70]  # contents of lengths - 1: row 1 is empty, rows 0, 2 and 3 cross 128
    fwd = check(x, [[prompt, n - 1] for n in lengths], k, "bf16", "forward form")
    x = x.cuda()
    gen = ((x[:, :prompt],),) + tuple((x[:, prompt + g - 1:prompt + g],) for g in range(1, steps))
    got = embedding_similarity(gen, k, 0, lengths=lengths)
    assert got.n.tolist() == [n - 1 for n in lengths]
    assert np.array_equal(fwd["coverage"], got.coverage.cpu().numpy()) and np.array_equal(fwd["similarity"], got.similarity.cpu().numpy())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_group_alone_in_a_batch_and_through_a_strided_view_has_the_same_bits(dtype):
    k, d = 3, 52
    x, windows = cases.make(3, 3, k, 130, 2 * d + 3, dtype=dtype)
    wide = x.cuda()
    view = wide[:, :, 3:3 + d]  # row-strided, off a 16-byte boundary
    assert not view.is_contiguous()
    whole = run(view, windows, k)
    assert all(np.array_equal(whole[f], run(view.contiguous(), windows, k)[f]) for f in whole)
    host = embedding_similarity((view.cpu(),), k, 0, windows=windows)  # host states: one upload
    assert not host.coverage.is_cuda and np.array_equal(host.coverage.numpy(), whole["coverage"])
    short = [[s, min(n, 20)] for s, n in windows[k:2 * k]]  # another T_max, another batch
    alone = run(view[k:2 * k], short, k)
    inside = run(view, windows[:k] + short + windows[2 * k:], k)
    assert all(np.array_equal(alone[f][0], inside[f][1]) for f in alone)


def test_exact_cases():
    k, d = 3, 40
    x, windows = cases.make(4, 3, k, 33, d, ragged=False)
    x[1] = x[0]                                      # group 0: samples 0 and 1 identical, the same window
    windows[1] = windows[0]
    windows[3][1], windows[4][1], windows[5][1] = 0, 0, 7  # group 1: two empty samples and a full one
    got = check(x, windows, k, "bf16", "identical and empty samples")
    bound = cases.reference(x, windows, k, "bf16")["bound"]
    assert abs(got["similarity"][0, 0, 1] - 1.0) <= 2 * bound[0]
    assert got["similarity"][1].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]]
    x[0, windows[0][0] + 2] = 0.0                    # a zero token: cosine 0 with everything
    got = check(x, windows, k, "bf16", "zero token", center=False)
    x[7, windows[7][0]] = float("nan")               # group 2
    nan = check(x, windows, k, "bf16", "NaN state", center=False)
    assert np.isnan(nan["coverage"][2]).all() and np.isnan(nan["similarity"][2]).all()
    assert all(np.array_equal(nan[f][:2], got[f][:2]) for f in got)


def test_pipeline_requests_equal_the_direct_call():
    from transformers import GenerationConfig

    from runia_core_amd.llm_uncertainty import compute_uncertainties_batch, generated_lengths
    from test_llm_pipeline_gpu import PROMPTS, IdTok, RecordingModel, tiny_llama

    eos, k = [5, 6, 7], 4
    model = RecordingModel(tiny_llama(eos=eos, seed=29))
    cfg = GenerationConfig(max_new_tokens=10, pad_token_id=0, eos_token_id=eos)
    torch.manual_seed(4)
    reqs = [{"method_name": "deg", "similarity": "embedding"}, {"method_name": "num_sets", "similarity": "embedding"},
            {"method_name": "eigv", "similarity": "embedding", "layer": 3}, {"method_name": "deg"}]
    _, scores = compute_uncertainties_batch(model, IdTok(), PROMPTS, reqs, cfg, k)
    _, samp = model.outs
    in_len = int(samp.sequences.shape[1] - len(samp.scores))
    assert set(scores) == {"deg_embedding", "num_sets_embedding", "eigv_embedding_3", "deg"}
    lengths = generated_lengths(samp.sequences, in_len, eos)
    want = embedding_consistency_scores(samp.hidden_states, k, 15, lengths=lengths)
    want3 = embedding_consistency_scores(samp.hidden_states, k, 3, lengths=lengths)
    assert torch.equal(scores["deg_embedding"], want.u_deg.cpu()) and bool(want.u_deg.isfinite().all())
    assert torch.equal(scores["num_sets_embedding"], want.num_sets.cpu().to(torch.int64))
    assert torch.equal(scores["eigv_embedding_3"], want3.u_eigv.cpu())
