"""Logit scores without a GPU: the C ABI's new entry points and their argument checks, the Python contract of
transition_scores / token_entropies / generation_scores (argument checks before any launch, no host fallback), and a
NumPy f64 restatement checked against every number of the reference fixture (tests/golden/ref_logit_scores.npz,
tools/make_goldens_logits.py).  The GPU tests (test_logit_scores_gpu.py) check the kernels against this restatement at
sizes the fixture cannot hold."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from runia_core_amd import _hip

LOGIT_SYMBOLS = ["runia_logit_stats", "runia_logit_stats_workspace_bytes"]
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SEQ_KEYS = ("generation_entropy", "perplexity", "normalized_entropy")


# ---- restatement (f64) ------------------------------------------------------------------------------------------------
def restate(x, tokens):
    """x (T, B, V) logits (any float dtype, read as f64), tokens (B, T) -> the reference's numbers in f64:
    log_probs = x[tok] - logsumexp(x) (-inf where x[tok] = -inf), token_entropy = -sum p log max(p, 1e-12) / log V,
    their per-row means, and normalized_entropy.  A row holding NaN or +inf, or only -inf, gives NaN."""
    x = np.asarray(x, dtype=np.float64)
    T, B, V = x.shape
    tok = np.asarray(tokens, dtype=np.int64).T  # (T, B)
    bad = np.isnan(x).any(-1) | np.isposinf(x).any(-1) | np.isneginf(x).all(-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.where(bad, 0.0, np.max(np.where(np.isnan(x), -np.inf, x), axis=-1))
        e = np.exp(x - m[..., None])
        s = e.sum(-1)
        p = e / s[..., None]
        h = -(p * np.log(np.maximum(p, 1e-12))).sum(-1) / np.log(V)
        xt = np.take_along_axis(x, tok[..., None], -1)[..., 0]
        # (x - m) - log s, as log_softmax: m + log s loses log s in f64 once |m| passes 2^53 (bf16 logits of 1e30)
        lp = np.where(np.isneginf(xt), -np.inf, (xt - m) - np.log(s))
    lp = np.where(bad, np.nan, lp).T
    h = np.where(bad, np.nan, h).T
    with np.errstate(invalid="ignore"):
        valid = ~np.isneginf(lp)
        row_means = np.where(valid, lp, 0.0).sum(1) / valid.sum(1)
    return dict(log_probs=lp, token_entropy=h, generation_entropy=h.mean(1), perplexity=-lp.mean(1),
                normalized_entropy=-row_means.sum() / B)


def recipe_logits(seed, T, B, V, scale):
    """The fixture's seed recipe for large V (tools/make_goldens_logits.py)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, B, V), dtype=np.float32) * np.float32(scale)


def case_scores(case, device="cpu"):
    """The case's scores as the tuple generate() returns: T steps of (B, V) or (B, 1, V) in the case's dtype."""
    x = torch.from_numpy(case["logits"]).to(device=device, dtype=DTYPES[case["dtype"]])
    return tuple(x[t][:, None, :] if case["step3d"] else x[t] for t in range(x.shape[0]))


def fixture_cases():
    with np.load(os.path.join(ROOT, "tests", "golden", "ref_logit_scores.npz"), allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    cases = []
    for name in data["cases"]:
        name = str(name)
        g = lambda k: data[f"{name}__{k}"]  # noqa: E731
        if f"{name}__steps" in data:
            x = g("steps")
        else:
            seed, T, B, V = (int(v) for v in g("recipe"))
            x = recipe_logits(seed, T, B, V, float(g("scale")))
        c = dict(name=name, logits=x, dtype=str(g("dtype")), step3d=bool(g("step3d")), sequences=g("sequences"),
                 log_probs=g("log_probs"), token_entropy=g("token_entropy"),
                 **{k: g(k) for k in SEQ_KEYS})
        if f"{name}__hf_log_probs" in data:
            c["hf_log_probs"] = g("hf_log_probs")
        cases.append(c)
    return cases


def case_values(case):
    """The f32 values the kernel reads (f32 logits cast to the case's dtype), (T, B, V) f64."""
    return torch.from_numpy(case["logits"]).to(DTYPES[case["dtype"]]).double().numpy()


def case_tokens(case):
    T = case["logits"].shape[0]
    return case["sequences"][:, -T:]


def ref_tol(V, tol):
    """A tolerance against the reference: as given, and 5x past V = 10 000, where the reference's own f32 arithmetic (HF's
    log_softmax and generation_entropy's sums, on the CPU) is off by up to 4e-6 of |lse| (0.5e-4 at V = 50 257) and 1.2e-6
    in the normalised entropy against the f64 restatement.  There the kernels are held to the given tolerance against the
    restatement instead (test_logit_scores_gpu.py)."""
    return tol if V <= 10_000 else 5 * tol


def assert_log_probs(got, exp, what="", tol=2e-6):
    """<= tol max(1, |ref|), with -inf and NaN at exactly the reference's places."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(exp), err_msg=f"{what}: -inf places")
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{what}: NaN places")
    f = np.isfinite(exp)
    err = np.abs(got[f] - exp[f]) / np.maximum(1.0, np.abs(exp[f]))
    assert err.size == 0 or err.max() <= tol, f"{what}: log-prob error {err.max():.3e}"


def assert_close(got, exp, tol, relative, what=""):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{what}: NaN places")
    np.testing.assert_array_equal(np.isinf(got), np.isinf(exp), err_msg=f"{what}: inf places")
    f = np.isfinite(exp)
    err = np.abs(got[f] - exp[f]) / (np.maximum(1.0, np.abs(exp[f])) if relative else 1.0)
    assert err.size == 0 or err.max() <= tol, f"{what}: error {err.max():.3e} > {tol}"


# ---- tests ------------------------------------------------------------------------------------------------------------
def test_logit_symbols_in_header_table_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(runia_logit_[a-z0-9_]+)\s*\(", text))
    assert sorted(declared) == LOGIT_SYMBOLS
    assert set(LOGIT_SYMBOLS) <= set(_hip.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True).stdout
    assert set(LOGIT_SYMBOLS) <= set(re.findall(r"\bT (runia_[a-z0-9_]+)", out))
    assert _hip.load_library().runia_abi_version() == 6


def test_logit_stats_argument_checks_before_any_launch():
    """Null pointers, bad sizes and dtypes return RUNIA_E_INVALID (-1); a short, missing or misaligned workspace
    RUNIA_E_WORKSPACE (-4).  Every call below returns before touching a device (none is needed)."""
    lib = _hip.load_library()
    fake = 1 << 20  # a non-null, aligned address that is never dereferenced
    # 16 bytes per (row, step, chunk of 4 096 logits); zero for sizes the kernels do not take
    assert lib.runia_logit_stats_workspace_bytes(256, 10, 128256) == 256 * 10 * 32 * 16
    assert lib.runia_logit_stats_workspace_bytes(3, 2, 1) == 3 * 2 * 16
    assert lib.runia_logit_stats_workspace_bytes(3, 2, 4097) == 3 * 2 * 2 * 16
    for bad in ((0, 2, 50), (3, 0, 50), (3, 2, 0), (-1, 2, 50), (3, 2, 1 << 40)):
        assert lib.runia_logit_stats_workspace_bytes(*bad) == 0, bad
    T, B, V = 4, 3, 50
    need = lib.runia_logit_stats_workspace_bytes(T, B, V)
    base = dict(table=fake, dtype=0, T=T, B=B, V=V, tok=fake, ts=T, norm=1, lse=None, lp=fake, ent=fake, seq=fake, ws=fake,
                wb=need, st=None)
    call = lambda **kw: lib.runia_logit_stats(*{**base, **kw}.values())  # noqa: E731
    assert call(table=None) == -1
    assert call(dtype=3) == -1 and call(dtype=-1) == -1
    assert call(T=0) == -1 and call(B=0) == -1 and call(V=0) == -1
    assert call(lp=None, ent=None, seq=None) == -1          # no output
    assert call(tok=None) == -1                               # log_prob needs the tokens
    assert call(ts=T - 1) == -1                               # token rows overlap
    assert call(lp=None) == -1 and call(ent=None) == -1       # the sequence scores need both
    assert call(wb=need - 1) == -4
    assert call(ws=None) == -4
    assert call(ws=fake + 8) == -4


def _mock(T=3, B=2, V=7, dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    scores = tuple(torch.randn(B, V, generator=g).to(dtype) for _ in range(T))
    seq = torch.randint(0, V, (B, 5 + T), generator=g)
    return seq, scores


def test_logit_python_contract_without_a_device(monkeypatch):
    import runia_core_amd.llm_uncertainty as pkg
    from runia_core_amd.llm_uncertainty import generation_scores, token_entropies, transition_scores

    assert {"GenerationScores", "generation_scores", "token_entropies", "transition_scores"} <= set(pkg.__all__)
    seq, scores = _mock()
    with pytest.raises(NotImplementedError):
        transition_scores(seq, scores, beam_indices=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="rows"):
        generation_scores(seq[:1], scores)
    with pytest.raises(ValueError, match="fewer than"):
        transition_scores(seq[:, :2], scores)
    bad = seq.clone()
    bad[1, -1] = 7
    with pytest.raises(ValueError, match=r"\[0, 7\)"):
        transition_scores(bad, scores, normalize_logits=True)
    bad[1, -1] = -1
    with pytest.raises(ValueError, match=r"\[0, 7\)"):
        generation_scores(bad, scores)
    bad = seq.clone()
    bad[0, 0] = 99  # a prompt column: not a generated token, not checked (HF gathers the last T columns only)
    for call in (lambda s: token_entropies(s), lambda s: generation_scores(seq, s)):
        with pytest.raises(ValueError):
            call(())
        with pytest.raises(ValueError):
            call(scores[:2] + (torch.randn(2, 8),))              # mixed shapes
        with pytest.raises(ValueError):
            call(scores[:2] + (scores[2].half(),))               # mixed dtypes
        with pytest.raises(ValueError):
            call(tuple(s[:, None, None, :] for s in scores))     # not (B, V) / (B, 1, V)
        with pytest.raises(TypeError):
            call(tuple(s.double() for s in scores))              # unsupported dtype
    # a valid call without a device raises: there is no host fallback
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for call in (lambda: transition_scores(bad, scores), lambda: transition_scores(seq, scores, normalize_logits=True),
                 lambda: token_entropies(tuple(s[:, None, :] for s in scores)), lambda: generation_scores(seq, scores),
                 lambda: generation_scores(seq, tuple(s.bfloat16() for s in scores))):
        with pytest.raises(_hip.RuniaHipError):
            call()


def test_reference_scores_stay_in_place():
    """The reference's host functions keep their names on .scores and gain no neighbour there."""
    import runia_core_amd.llm_uncertainty.scores as sc

    assert sc.__all__ == ["eigen_score", "normalized_entropy", "semantic_entropy", "perplexity", "generation_entropy"]
    for n in ("transition_scores", "token_entropies", "generation_scores", "GenerationScores"):
        assert not hasattr(sc, n)


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_every_fixture_number(case):
    got = restate(case_values(case), case_tokens(case))
    name = case["name"]
    V = case["logits"].shape[-1]
    assert_log_probs(got["log_probs"], case["log_probs"], name, ref_tol(V, 2e-6))
    assert_close(got["token_entropy"], case["token_entropy"], ref_tol(V, 1e-6), False, f"{name} token entropy")
    for k in SEQ_KEYS:
        assert_close(got[k], case[k], ref_tol(V, 1e-6), True, f"{name} {k}")
    if "hf_log_probs" in case:  # HF's call on the generation's own scores
        assert_log_probs(got["log_probs"], case["hf_log_probs"], f"{name} HF", ref_tol(V, 2e-6))


# ---- the edge-case generators of test_logit_scores_edges_gpu.py (logit_edge_cases.py), checked without a device ------
import logit_edge_cases as ec  # noqa: E402


def edge_cases():
    """Every case the GPU edge tests score, by name."""
    cases = [ec.v_sweep_case(V, d) for V in ec.V_SWEEP for d in ec.DTYPE_NAMES]
    cases += [ec.masked_case(V, d, m) for V in ec.MASK_VOCABS for d in ec.DTYPE_NAMES for m in (False, True)]
    cases += [ec.equal_rows_case(V, d) for V in ec.EQUAL_VOCABS for d in ec.DTYPE_NAMES]
    cases += [ec.maxima_case(d) for d in ec.DTYPE_NAMES]
    cases += [ec.peaked_case(lead, d) for lead in ec.PEAK_LEADS for d in ("float32", "bfloat16")]
    cases += [ec.extreme_case(d, mag) for d, mag in ec.EXTREMES]
    cases += [ec.batch_case(B, T) for B in ec.BATCH_SIZES for T in ec.BATCH_STEPS]
    return cases


def _torch_f64(case):
    """log_probs and token_entropy (B, T) of torch.log_softmax / torch.softmax in f64."""
    x = torch.from_numpy(case["x"]).double()
    tok = torch.from_numpy(case["tokens"]).t()[..., None]  # (T, B, 1)
    lp = torch.log_softmax(x, -1).gather(-1, tok)[..., 0].t()
    p = torch.softmax(x, -1)
    h = (-(p * p.clamp_min(1e-12).log()).sum(-1) / np.log(x.shape[-1])).t()
    return lp.numpy(), h.numpy()


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: c["name"])
def test_restatement_agrees_with_torch_f64_on_the_edge_cases(case):
    """restate() is the judge of the GPU edge tests: on every input they use it agrees with torch's own f64 log_softmax /
    softmax to 1e-12, with -inf and NaN at torch's places (no case here holds an all -inf row, the one place where
    restate's NaN convention is its own), and the case's values are exact in its dtype."""
    assert case["x"].dtype == np.float32 and case["tokens"].dtype == np.int64
    T, B, V = case["x"].shape
    assert case["tokens"].shape == (B, T) and case["tokens"].min() >= 0 and case["tokens"].max() < V
    np.testing.assert_array_equal(ec.representable(case["x"], case["dtype"]), case["x"])
    assert not np.isneginf(case["x"]).all(-1).any()
    got = restate(ec.values64(case), case["tokens"])
    lp, h = _torch_f64(case)
    assert_log_probs(got["log_probs"], lp, case["name"], 1e-12)
    assert_close(got["token_entropy"], h, 1e-12, False, f"{case['name']} token entropy")
    with np.errstate(invalid="ignore"):
        finite = ~np.isneginf(lp)
        means = np.where(finite, lp, 0.0).sum(1) / finite.sum(1)
    assert_close(got["generation_entropy"], h.mean(1), 1e-12, True, f"{case['name']} generation entropy")
    assert_close(got["perplexity"], -lp.mean(1), 1e-12, True, f"{case['name']} perplexity")
    assert_close(got["normalized_entropy"], -means.sum() / B, 1e-12, True, f"{case['name']} normalized entropy")


@pytest.mark.parametrize("V", ec.MASK_VOCABS)
@pytest.mark.parametrize("dtype", ec.DTYPE_NAMES)
@pytest.mark.parametrize("finfo_min", [False, True], ids=["inf", "min"])
def test_masked_cases_have_the_empty_chunks_and_lanes_they_are_named_for(V, dtype, finfo_min):
    case = ec.masked_case(V, dtype, finfo_min)
    nc = ec.n_chunks(V)
    assert nc == {128256: 32, 32001: 8}[V] and V % ec.K_CHUNK != 0 and ec.LANES * ec.PER_LANE == ec.K_CHUNK
    assert case["fill"] == (float(torch.finfo(DTYPES[dtype]).min) if finfo_min else -np.inf)
    assert [(r["placement"], r["k"]) for r in case["rows"]] == [(p, k) for p in ec.MASK_PLACEMENTS for k in ec.MASK_KEEP]
    seen = set()
    for b, row in enumerate(case["rows"]):
        k, placement, pos = row["k"], row["placement"], row["positions"]
        for t in range(case["x"].shape[0]):
            x = case["x"][t, b]
            np.testing.assert_array_equal(np.flatnonzero(x != case["fill"]), pos)
            assert np.isfinite(x[pos]).all() and np.abs(x[pos]).max() < 20
            chunks, lanes = ec.live_chunks_and_lanes(x, dtype, case["fill"])
            want_chunks, want_lanes = ec.mask_expected_live(V, k, placement)
            assert chunks == want_chunks, (placement, k)
            assert want_lanes is None or lanes == want_lanes, (placement, k)
            # the row's empty chunks and (chunk, lane) pairs: all but those few
            if placement in ("first_chunk", "last_chunk", "row_end"):
                assert nc - chunks == nc - 1
            if k == 1:
                assert nc * ec.LANES - lanes == nc * ec.LANES - 1
        live = {int(p) // ec.K_CHUNK for p in pos}
        if placement == "first_chunk":
            assert live == {0}
        elif placement in ("last_chunk", "row_end"):
            assert live == {nc - 1} and (placement == "last_chunk" or pos[-1] == V - 1)
        elif placement == "spread":
            assert live == (set(range(nc)) if k > nc else {nc // 2} if k == 1 else live) and len(live) == min(k, nc)
            if k == 2:
                assert live == {0, nc - 1}
        elif placement == "one_lane":
            assert {ec.lane_of(int(p), dtype)[1] for p in pos} == {3} and 0 not in live and nc - 1 not in live
        seen |= live
        # step 0 scores a survivor, step 1 a masked position
        assert case["tokens"][b, 0] in pos and case["tokens"][b, 1] not in pos
    assert {0, nc // 2, nc - 1} <= seen  # the finite chunk is first, in the middle and last
    b = case["all_tokens_masked_row"]
    ref = restate(ec.values64(case), case["tokens"])
    if finfo_min:
        assert np.isfinite(ref["log_probs"]).all() and np.isfinite(ref["token_entropy"]).all()
        assert np.isfinite(ref["normalized_entropy"])
    else:
        assert np.isneginf(ref["log_probs"][b]).all() and np.isnan(ref["normalized_entropy"])
        assert np.isneginf(ref["log_probs"][:b, 1]).all() and np.isfinite(ref["log_probs"][:b, 0]).all()
        assert np.isfinite(restate(ec.values64(case)[:, :b], case["tokens"][:b])["normalized_entropy"])


def test_repeated_maxima_sit_where_their_names_say():
    for dtype in ec.DTYPE_NAMES:
        case = ec.maxima_case(dtype)
        assert ec.n_chunks(ec.MAXIMA_V) == 4 and ec.MAXIMA_V % ec.K_CHUNK == 1
        for b, row in enumerate(case["rows"]):
            x, pos = case["x"][0, b], row["positions"]
            assert len(pos) == row["n"] == len(set(pos))
            np.testing.assert_array_equal(np.flatnonzero(x == x.max()), sorted(pos))
            where = [ec.lane_of(p, dtype) for p in pos]
            chunks, lanes = {c for c, _ in where}, {l for _, l in where}
            if row["placement"] == "same_lane":
                assert len(chunks) == 1 and len(lanes) == 1
            elif row["placement"] == "neighbour_lanes":
                assert len(chunks) == 1 and sorted(lanes) == list(range(min(lanes), min(lanes) + row["n"]))
                assert len({l // 64 for l in lanes}) == 1
            elif row["placement"] == "other_wave":
                assert len(chunks) == 1 and len({l // 64 for l in lanes}) == row["n"]
            elif row["placement"] == "other_chunk":
                assert len(chunks) == row["n"]
            else:
                assert pos[0] == ec.MAXIMA_V - 1 and len(chunks) == row["n"]
    for V in ec.EQUAL_VOCABS:
        case = ec.equal_rows_case(V, "bfloat16")
        assert (case["x"] == case["x"][..., :1]).all()
        ref = restate(ec.values64(case), case["tokens"])
        np.testing.assert_allclose(ref["log_probs"], -np.log(V), rtol=0, atol=1e-12)
        if V > 1:
            np.testing.assert_allclose(ref["token_entropy"], 1.0, rtol=0, atol=1e-12)
        else:
            assert np.isnan(ref["token_entropy"]).all()  # 0 / log 1


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("lead", ec.PEAK_LEADS)
def test_peaked_rows_are_peaked(lead, dtype):
    case = ec.peaked_case(lead, dtype)
    ref = restate(ec.values64(case), case["tokens"])
    # a lead of 10 over 50 256 Gaussian logits leaves them e^-10 * 50 256 * e^(1/2 - max) ~ 0.06 of the mass: peaked, but not
    # below 1e-3; from 30 on the entropy is below 1e-3 (1e-9 and smaller)
    bound = 1e-3 if lead >= 30 else 0.1
    assert (ref["token_entropy"] < bound).all() and (ref["token_entropy"] > 0).all()
    assert (ref["log_probs"][:, 0] > -bound).all() and (ref["log_probs"][:, 1] < -lead + bound).all()
    chunks = [w // ec.K_CHUNK for w in case["winners"]]
    assert chunks[0] == 0 and chunks[2] == ec.n_chunks(ec.PEAK_V) - 1 and 0 < chunks[1] < chunks[2]
    if lead == 120:
        assert ref["token_entropy"].max() < 1e-30 * 1e-10


def test_extreme_rows_are_finite_and_far_apart():
    for dtype, mag in ec.EXTREMES:
        case = ec.extreme_case(dtype, mag)
        assert np.isfinite(case["x"]).all() and case["x"].max() == case["mag"] and case["x"].min() == -case["mag"]
        assert abs(case["mag"] / mag - 1) < 2 ** -8
        ref = restate(ec.values64(case), case["tokens"])
        assert all(np.isfinite(np.asarray(v)).all() for v in ref.values())
        assert np.abs(ref["log_probs"]).max() < 10
        b, tok = case["overflow_token"]
        assert case["x"][0, b, tok] == -case["mag"]
    assert 2 * ec.extreme_case("bfloat16", 3e38)["mag"] > float(np.finfo(np.float32).max)


@pytest.mark.parametrize("which", ec.BAD_TOKEN_IDS)
@pytest.mark.parametrize("column", [0, 2], ids=["first", "last"])
def test_token_ids_out_of_range_raise_before_any_launch(which, column, monkeypatch):
    """finish_kernel loads row[token] unchecked: the wrapper's [0, V) check is the only guard.  No device exists here,
    so a missing check would surface as RuniaHipError, not as the ValueError asserted."""
    from runia_core_amd.llm_uncertainty import generation_scores, transition_scores
    from runia_core_amd.llm_uncertainty.logits import _token_ids

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    V, B, T = 7, 2, 3
    scores = tuple(torch.zeros(B, V) for _ in range(T))
    bad = torch.from_numpy(ec.bad_token_sequences(which, column, V, B, T))
    assert not (0 <= int(bad[1, 5 + column]) < V) and bad.shape == (B, 5 + T)
    with pytest.raises(ValueError, match=r"\[0, 7\)"):
        _token_ids(bad, B, T, V)
    for call in (lambda: generation_scores(bad, scores), lambda: transition_scores(bad, scores, normalize_logits=True),
                 lambda: transition_scores(bad, scores), lambda: generation_scores(bad.numpy(), scores)):
        with pytest.raises(ValueError, match=r"\[0, 7\)"):
            call()
    # the largest and smallest valid ids pass the check, and a bad id in a prompt column (not scored) is accepted
    ok = bad.clone()
    ok[1, 5 + column] = V - 1
    ok[0, 5] = 0
    assert torch.equal(_token_ids(ok, B, T, V), ok[:, 5:])
    ok[0, 4] = {"-1": -1, "V": V, "2**40": 2 ** 40}[which]
    assert torch.equal(_token_ids(ok, B, T, V), ok[:, 5:])
    with pytest.raises(_hip.RuniaHipError):  # past the checks: no device here
        generation_scores(ok, scores)
