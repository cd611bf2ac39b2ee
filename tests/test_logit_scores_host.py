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
        lse = m + np.log(s)
        p = e / s[..., None]
        h = -(p * np.log(np.maximum(p, 1e-12))).sum(-1) / np.log(V)
        xt = np.take_along_axis(x, tok[..., None], -1)[..., 0]
        lp = np.where(np.isneginf(xt), -np.inf, xt - lse)
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
