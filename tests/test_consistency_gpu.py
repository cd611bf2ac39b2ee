"""Sample-consistency kernels (csrc/consistency.hip) on the GPU against the NumPy statement of tests/consistency_cases.py.
The integer tables are compared for equality; the graph scores at SCORE_TOL = 1e-10 absolute, the project's figure for the same
Jacobi solver (the observed maximum is printed)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import consistency_cases as cc
import runia_core_amd.llm_uncertainty as L
from runia_core_amd import _hip

pytestmark = pytest.mark.gpu

FLOAT_FIELDS = ("eigenvalues", "u_deg", "u_eigv", "u_ecc", "lexical_similarity", "c_deg", "c_ecc")


def dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype)


def check_tables(got, want, what=""):
    ln, lcs, uq, it = want
    assert got.len.dtype == torch.int32 and got.lcs.dtype == torch.int32
    assert np.array_equal(got.len.cpu().numpy(), ln), what
    assert np.array_equal(got.lcs.cpu().numpy(), lcs), what
    if got.uniq is not None:
        assert np.array_equal(got.uniq.cpu().numpy(), uq), what
        assert np.array_equal(got.inter.cpu().numpy(), it), what


@functools.lru_cache(maxsize=None)
def mix_reference():
    ids, lengths = cc.length_mix_group()
    return ids, lengths, cc.pair_counts(ids, 8, lengths=lengths)


# ---- content lengths ------------------------------------------------------------------------------------------------------------
def test_lengths_0_to_129_mixed_in_one_group():
    ids, lengths, want = mix_reference()
    got = L.pairwise_counts(dev(ids), 8, lengths=dev(lengths))
    assert got.len.is_cuda and got.lcs.shape == (1, 8, 8) and got.uniq.shape == (8,)
    check_tables(got, want)


def test_max_t_against_max_t_minus_one():
    ids, lengths = cc.max_t_pair()
    want = cc.pair_counts(ids, 2, lengths=lengths, lcs=cc.lcs_scan)
    check_tables(L.pairwise_counts(dev(ids), 2, lengths=dev(lengths)), want)
    check_tables(L.pairwise_counts(dev(ids, torch.int32), 2, lengths=dev(lengths)), want)


# ---- content patterns -----------------------------------------------------------------------------------------------------------
def test_patterns_identical_disjoint_one_id_reverse_binary():
    groups = cc.pattern_groups()
    ids = np.concatenate(list(groups.values()))  # five K = 2 groups in one launch
    want = cc.pair_counts(ids, 2)
    got = L.pairwise_counts(dev(ids), 2)
    check_tables(got, want)
    lcs = got.lcs.cpu().numpy()
    names = list(groups)
    assert lcs[names.index("identical"), 0, 1] == 70 and lcs[names.index("disjoint"), 0, 1] == 0
    assert lcs[names.index("one_id"), 0, 1] == 70


# ---- ids, dtype and layout ------------------------------------------------------------------------------------------------------
def test_int64_ids_are_compared_on_all_64_bits():
    ids = cc.high_bit_pair()
    check_tables(L.pairwise_counts(dev(ids), 3), cc.pair_counts(ids, 3))
    low = ids.astype(np.int32)  # the low words alone are equal
    got = L.pairwise_counts(dev(low, torch.int32), 3)
    check_tables(got, cc.pair_counts(low, 3))
    assert got.lcs[0, 0, 1].item() == 6


def test_int32_and_int64_inputs_agree():
    ids, lengths, want = mix_reference()
    a = L.pairwise_counts(dev(ids, torch.int32), 8, lengths=dev(lengths, torch.int32))
    check_tables(a, want)


def test_strided_views_are_read_in_place():
    ids, lengths, want = mix_reference()
    wide = torch.full((8, 5 + 129), 3, dtype=torch.int64, device="cuda")
    wide[:, 5:] = dev(ids)
    view = wide[:, 5:]
    assert not view.is_contiguous()
    check_tables(L.pairwise_counts(view, 8, lengths=dev(lengths)), want, "column offset")
    check_tables(L.pairwise_counts(wide, 8, start=5, lengths=dev(lengths)), want, "start")
    inter = torch.full((8, 2 * 129), 5, dtype=torch.int64, device="cuda")
    inter[:, ::2] = dev(ids)
    check_tables(L.pairwise_counts(inter[:, ::2], 8, lengths=dev(lengths)), want, "every second column")
    rows = torch.zeros((16, 129), dtype=torch.int64, device="cuda")
    rows[::2] = dev(ids)
    check_tables(L.pairwise_counts(rows[::2], 8, lengths=dev(lengths)), want, "every second row")


# ---- eos and lengths ------------------------------------------------------------------------------------------------------------
def test_eos_at_zero_in_the_middle_two_ids_and_lengths():
    ids, eos = cc.eos_group()
    got = L.pairwise_counts(dev(ids), 4, eos_token_id=list(eos))
    check_tables(got, cc.pair_counts(ids, 4, eos=eos))
    assert got.len.tolist() == [0, 3, 3, 8]
    check_tables(L.pairwise_counts(dev(ids), 4, eos_token_id=1), cc.pair_counts(ids, 4, eos=(1,)), "one eos id")
    check_tables(L.pairwise_counts(dev(ids), 4), cc.pair_counts(ids, 4), "no eos id")
    lengths = np.array([4, 2, 8, 5], dtype=np.int64)
    check_tables(L.pairwise_counts(dev(ids), 4, eos_token_id=list(eos), lengths=dev(lengths)),
                 cc.pair_counts(ids, 4, eos=eos, lengths=lengths), "eos and lengths")
    w = L.pairwise_similarity(dev(ids), 4, eos_token_id=list(eos)).cpu().numpy()
    assert np.array_equal(w, cc.similarity(*cc.pair_counts(ids, 4, eos=eos), "rouge_l"))


# ---- group sizes and independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 64])
def test_group_sizes(k):
    ids, lengths = cc.random_groups(3, k, 24 if k == 64 else 70, seed=20 + k)
    lengths[k:2 * k] //= 3  # three groups of different lengths
    want = cc.pair_counts(ids, k, lengths=lengths, lcs=cc.lcs_scan)
    got = L.pairwise_counts(dev(ids), k, lengths=dev(lengths))
    check_tables(got, want)
    for kind in ("rouge_l", "jaccard"):
        w = L.pairwise_similarity(dev(ids), k, kind=kind, lengths=dev(lengths))
        assert w.dtype == torch.float64 and w.shape == (3, k, k)
        assert np.array_equal(w.cpu().numpy(), cc.similarity(*want, kind)), kind
        assert bool((w.diagonal(dim1=1, dim2=2) == 1.0).all()) and torch.equal(w, w.transpose(1, 2))


def test_a_group_gives_the_same_integers_first_and_last():
    ids, lengths = cc.random_groups(4, 5, 90, seed=31)
    first = L.pairwise_counts(dev(ids), 5, lengths=dev(lengths))
    order = np.r_[5:20, 0:5]  # group 0 moves to the end
    last = L.pairwise_counts(dev(ids[order]), 5, lengths=dev(lengths[order]))
    for a, b in zip(first, last):
        n = a.shape[0] // 4
        assert torch.equal(a[:n], b[-n:])


# ---- Jaccard --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["duplicates", "reordered", "uniq_64_65", "empty_row"])
def test_jaccard_tables(name):
    ids, lengths, k = cc.jaccard_groups()[name]
    want = cc.pair_counts(ids, k, lengths=lengths)
    got = L.pairwise_counts(dev(ids), k, lengths=None if lengths is None else dev(lengths))
    check_tables(got, want)
    only = L.pairwise_counts(dev(ids), k, lengths=None if lengths is None else dev(lengths), lcs=False)
    assert only.lcs is None and torch.equal(only.inter, got.inter) and torch.equal(only.uniq, got.uniq)
    w = L.pairwise_similarity(dev(ids), k, kind="jaccard", lengths=None if lengths is None else dev(lengths))
    assert np.array_equal(w.cpu().numpy(), cc.similarity(*want, "jaccard"))
    if name == "reordered":
        assert w[0, 0, 1].item() == 1.0
    if name == "empty_row":
        assert w[0, 0, 1].item() == 0.0 and w[0, 1, 1].item() == 1.0


def test_set_sizes_around_the_sorted_powers_of_two():
    """The row sort pads a content to a power of two: lengths at, one above and one below such a size, from the empty row to
    MAX_T, drawn from 38 ids so that duplicates abound, and one row of a single repeated id.  Set overlap only (lcs=False); the
    reference's LCS is switched off as well (its DP would take minutes at MAX_T)."""
    lengths = np.array([0, 1, 2, 3, 4, 5, 64, 65, cc.MAX_T - 1, cc.MAX_T, 100], dtype=np.int64)
    k = len(lengths)
    ids = np.random.default_rng(5).integers(2, 40, size=(k, cc.MAX_T)).astype(np.int64)
    ids[k - 1] = 7
    _, _, uq, it = cc.pair_counts(ids, k, lengths=lengths, lcs=lambda a, b: 0)
    assert uq[0] == 0 and uq[1] == 1 and uq[-1] == 1 and uq[8] == uq[9] == 38
    got = L.pairwise_counts(dev(ids), k, lengths=dev(lengths), lcs=False)
    assert got.lcs is None
    assert np.array_equal(got.uniq.cpu().numpy(), uq)
    assert np.array_equal(got.inter.cpu().numpy(), it)
    got32 = L.pairwise_counts(dev(ids, torch.int32), k, lengths=dev(lengths), lcs=False)
    assert torch.equal(got32.uniq, got.uniq) and torch.equal(got32.inter, got.inter)


def test_host_ids_go_up_and_the_tables_come_back():
    ids, lengths, want = mix_reference()
    got = L.pairwise_counts(torch.from_numpy(ids), 8, lengths=torch.from_numpy(lengths))
    assert not got.len.is_cuda and not got.inter.is_cuda
    check_tables(got, want)
    s = L.consistency_scores(torch.from_numpy(ids), 8, lengths=torch.from_numpy(lengths))
    assert not s.u_eigv.is_cuda and s.u_eigv.shape == (1,) and s.c_ecc.shape == (1, 8) and s.num_sets.dtype == torch.int32


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes():
    ids, lengths = cc.random_groups(6, 17, 100, seed=41)
    x, n = dev(ids), dev(lengths)
    a, b = L.pairwise_counts(x, 17, lengths=n), L.pairwise_counts(x, 17, lengths=n)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for kind in ("rouge_l", "jaccard"):
        p, q = (L.consistency_scores(x, 17, kind=kind, lengths=n) for _ in range(2))
        for name, u, v in zip(p._fields, p, q):
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (kind, name)


# ---- graph scores ---------------------------------------------------------------------------------------------------------------
def graph_error(got, g, want):
    """max |got - want| over the float outputs of group g (num_sets compared exactly)."""
    assert int(got.num_sets[g]) == want["num_sets"]
    err = 0.0
    for f in FLOAT_FIELDS:
        a = np.atleast_1d(getattr(got, f)[g].cpu().numpy())
        err = max(err, float(np.max(np.abs(a - np.atleast_1d(want[f])))))
    return err


@pytest.mark.parametrize("k", [2, 6, 17])
def test_hand_worked_matrices(k):
    worst = 0.0
    for name, (w, exp) in cc.hand_matrices(k).items():
        if name == "two_blocks" and k < 4:
            continue
        got = L.graph_scores(torch.from_numpy(w).cuda())
        assert got.eigenvalues.shape == (w.shape[0],) and got.u_eigv.dim() == 0 and got.num_sets.dtype == torch.int32
        batched = L.graph_scores(torch.from_numpy(w).cuda()[None])
        worst = max(worst, graph_error(batched, 0, cc.graph_scores(w)))
        for key, value in exp.items():
            a = getattr(got, key).cpu().numpy()
            assert np.max(np.abs(a - np.asarray(value))) <= cc.SCORE_TOL, (name, key)
    print(f"hand-worked K={k}: max |device - numpy| = {worst:.3e}")
    assert worst <= cc.SCORE_TOL


@pytest.mark.parametrize("k", cc.SPECTRAL_KS)
def test_random_rouge_groups_against_numpy(k):
    """ids -> tables -> similarity -> graph scores on the device, against the statement on its own similarity."""
    ids, lengths = cc.random_groups(1, k, 24, cc.SPECTRAL_SEEDS[k])
    w = cc.rouge_w(k, cc.SPECTRAL_SEEDS[k])
    cc.guard(w, set_threshold=cc.RANDOM_SET_THRESHOLD)
    got = L.consistency_scores(dev(ids), k, lengths=dev(lengths), set_threshold=cc.RANDOM_SET_THRESHOLD)
    assert np.array_equal(got.similarity[0].cpu().numpy(), w)
    err = graph_error(got, 0, cc.graph_scores(w, set_threshold=cc.RANDOM_SET_THRESHOLD))
    print(f"ROUGE-L group K={k}: max |device - numpy| = {err:.3e} (gap to the Ecc threshold {cc.spectral_gap(w):.2e})")
    assert err <= cc.SCORE_TOL
    for thr in (0.2, 0.37, 0.63):  # NumSet at other thresholds, each away from every w_ij
        if cc.set_gap(w, thr) >= cc.SET_GUARD:
            assert int(L.graph_scores(got.similarity, set_threshold=thr).num_sets[0]) == cc.num_sets(w, thr)


def test_nan_in_one_group_leaves_the_others_alone():
    ws = np.stack([cc.rouge_w(5, s) for s in (51, 52, 53)])
    bad = ws.copy()
    bad[1, 1, 3] = np.nan
    clean = L.graph_scores(torch.from_numpy(ws).cuda())
    got = L.graph_scores(torch.from_numpy(bad).cuda())
    for f in FLOAT_FIELDS:
        a, b = getattr(got, f), getattr(clean, f)
        assert bool(a[1].isnan().all()), f
        assert torch.equal(a[[0, 2]].view(torch.uint8), b[[0, 2]].view(torch.uint8)), f
    assert got.num_sets.tolist() == [int(clean.num_sets[0]), -1, int(clean.num_sets[2])]
    low = ws.copy()
    low[1, 3, 1] = np.nan  # below the diagonal: not read
    again = L.graph_scores(torch.from_numpy(low).cuda())
    assert torch.equal(again.u_ecc, clean.u_ecc) and torch.equal(again.num_sets, clean.num_sets)


def test_lower_triangle_and_diagonal_are_ignored():
    w = cc.rouge_w(7, 61)
    g = w.copy()
    g[np.tril_indices(7, -1)] = -1e300
    np.fill_diagonal(g, np.inf)
    a, b = L.graph_scores(torch.from_numpy(w).cuda()), L.graph_scores(torch.from_numpy(g).cuda())
    for f in FLOAT_FIELDS + ("num_sets",):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    c = L.graph_scores(torch.from_numpy(w).float().cuda())  # any floating dtype: widened to f64
    assert c.u_eigv.dtype == torch.float64 and abs(float(c.u_eigv) - float(a.u_eigv)) < 1e-5


# ---- through compute_uncertainties_batch ----------------------------------------------------------------------------------------
def test_pipeline_requests_share_one_count_call_and_one_graph_launch(monkeypatch):
    from transformers import GenerationConfig

    from test_llm_pipeline_gpu import PROMPTS, IdTok, RecordingModel, tiny_llama

    eos = [5, 6, 7]
    model = RecordingModel(tiny_llama(eos=eos, seed=29))
    cfg = GenerationConfig(max_new_tokens=10, pad_token_id=0, eos_token_id=eos)
    calls = {"pairs": 0, "graph": 0}
    pairs, graph = _hip.cons_pairs, _hip.cons_graph

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(_hip, "cons_pairs", counted("pairs", pairs))
    monkeypatch.setattr(_hip, "cons_graph", counted("graph", graph))
    reqs = [{"method_name": m} for m in ("lexical_similarity", "deg", "ecc", "eigv", "num_sets")]
    reqs.append({"method_name": "deg", "similarity": "jaccard"})
    torch.manual_seed(4)
    K, B = 4, len(PROMPTS)
    texts, scores = L.compute_uncertainties_batch(model, IdTok(), PROMPTS, reqs, cfg, K)
    assert calls == {"pairs": 1, "graph": 1}
    assert set(scores) == {"lexical_similarity", "deg", "ecc", "eigv", "num_sets", "deg_jaccard"} and len(texts) == B
    det, samp = model.outs
    in_len = int(det.sequences.shape[1] - len(det.scores))
    want = L.consistency_scores(samp.sequences[:, in_len:], K, eos_token_id=eos)
    jac = L.consistency_scores(samp.sequences[:, in_len:], K, kind="jaccard", eos_token_id=eos)
    for key, value in (("lexical_similarity", want.lexical_similarity), ("deg", want.u_deg), ("ecc", want.u_ecc),
                       ("eigv", want.u_eigv), ("deg_jaccard", jac.u_deg)):
        got = scores[key]
        assert got.dtype == torch.float64 and not got.is_cuda and got.shape == (B,)
        assert torch.equal(got, value.cpu()), key
    assert scores["num_sets"].dtype == torch.int64 and torch.equal(scores["num_sets"], want.num_sets.cpu().long())
    ref = cc.pair_counts(samp.sequences[:, in_len:].cpu().numpy(), K, eos=eos)
    assert np.array_equal(want.similarity.cpu().numpy(), cc.similarity(*ref, "rouge_l"))

    # the one-prompt function: Python numbers
    calls.update(pairs=0, graph=0)
    one = RecordingModel(model.model)
    torch.manual_seed(5)
    _, s1 = L.compute_uncertainties(one, IdTok(), PROMPTS[0], reqs, cfg, K)
    assert calls == {"pairs": 1, "graph": 1}
    n_in = int(one.outs[0].sequences.shape[1] - len(one.outs[0].scores))
    w1 = L.consistency_scores(one.outs[1].sequences[:, n_in:], K, eos_token_id=eos)
    assert isinstance(s1["num_sets"], int) and s1["num_sets"] == int(w1.num_sets[0])
    assert isinstance(s1["eigv"], float) and s1["eigv"] == float(w1.u_eigv[0]) and s1["deg"] == float(w1.u_deg[0])
    assert s1["ecc"] == float(w1.u_ecc[0]) and s1["lexical_similarity"] == float(w1.lexical_similarity[0])
    assert isinstance(s1["deg_jaccard"], float)
