"""The logit-score kernels (csrc/logits.hip) at the places where they change code path: vocabulary sizes around the
4 096-logit chunk and the 16-byte load, rows whose lanes and chunks are mostly empty (top-k masks at real vocabularies,
with -inf and with the dtype's most negative finite value), repeated maxima, peaked rows, the ends of the f16 / bf16
range, and batches past the sequence kernel's 16 waves.  Every expected value is the f64 restatement of
test_logit_scores_host.py on the inputs of logit_edge_cases.py (both checked without a device there) or a closed form;
the tolerances are the project's own: 2e-6 max(1, |ref|) for log-probs, 1e-6 for the token entropy, 1e-6 relative for the
sequence scores."""
import numpy as np
import pytest
import torch

import logit_edge_cases as ec
from runia_core_amd.llm_uncertainty import generation_scores, token_entropies, transition_scores
from runia_core_amd.llm_uncertainty.logits import _token_ids
from test_logit_scores_host import SEQ_KEYS, assert_close, assert_log_probs, restate

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _all(res):
    return [_np(res.log_probs), _np(res.token_entropy), _np(res.generation_entropy), _np(res.perplexity),
            np.array(res.normalized_entropy)]


def _equal_bits(a, b, what):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert x.tobytes() == y.tobytes(), what


def _steps(case, rows=slice(None), misaligned=False):
    """The case's steps on the device in its dtype: (B, V) tensors, or views at element 5 of a wider NaN-filled buffer
    (row starts off the 16-byte grid: the element-wise load path)."""
    x = torch.from_numpy(case["x"][:, rows]).to(device="cuda", dtype=ec.DTYPES[case["dtype"]])
    if not misaligned:
        return tuple(x[t].clone() for t in range(x.shape[0]))  # own allocations: row 0 on the 16-byte grid
    out = []
    for t in range(x.shape[0]):
        store = torch.full((x.shape[1], x.shape[2] + 37), float("nan"), dtype=x.dtype, device="cuda")
        store[:, 5:5 + x.shape[2]] = x[t]
        out.append(store[:, 5:5 + x.shape[2]])
    return tuple(out)


def _check(res, exp, what):
    print(f"{what}: ", end="")
    for name, got, ref, tol, rel in (("log_probs", _np(res.log_probs), exp["log_probs"], 2e-6, True),
                                     ("token_entropy", _np(res.token_entropy), exp["token_entropy"], 1e-6, False),
                                     ("generation_entropy", _np(res.generation_entropy), exp["generation_entropy"], 1e-6, True),
                                     ("perplexity", _np(res.perplexity), exp["perplexity"], 1e-6, True),
                                     ("normalized_entropy", res.normalized_entropy, exp["normalized_entropy"], 1e-6, True)):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        f = np.isfinite(ref) & np.isfinite(got)
        err = np.abs(got[f] - ref[f]) / (np.maximum(1.0, np.abs(ref[f])) if rel else 1.0)
        print(f"{name} {err.max() if err.size else 0.0:.2e} (<= {tol:g})", end="; ")
    print()
    assert_log_probs(_np(res.log_probs), exp["log_probs"], what, 2e-6)
    assert_close(_np(res.token_entropy), exp["token_entropy"], 1e-6, False, f"{what} token entropy")
    got = dict(generation_entropy=_np(res.generation_entropy), perplexity=_np(res.perplexity),
               normalized_entropy=res.normalized_entropy)
    for k in SEQ_KEYS:
        assert_close(got[k], exp[k], 1e-6, True, f"{what} {k}")


def _score(case, rows=slice(None), misaligned=False):
    """generation_scores of the case (or of some of its rows), checked against the restatement; the single-output entry
    points give the same bits."""
    scores = _steps(case, rows, misaligned)
    tokens = case["tokens"][rows]
    T = len(scores)
    seq = torch.from_numpy(np.concatenate([np.zeros((tokens.shape[0], 3), dtype=np.int64), tokens], 1)).cuda()
    res = generation_scores(seq, scores)
    assert res.log_probs.shape == (tokens.shape[0], T) and res.log_probs.dtype == torch.float32
    _check(res, restate(case["x"][:, rows].astype(np.float64), tokens), case["name"] + (" misaligned" if misaligned else ""))
    assert _np(transition_scores(seq, scores, normalize_logits=True)).tobytes() == _np(res.log_probs).tobytes()
    assert _np(token_entropies(scores)).tobytes() == _np(res.token_entropy).tobytes()
    raw = _np(transition_scores(seq, scores))
    assert raw.tobytes() == np.take_along_axis(case["x"][:, rows], tokens.T[..., None], -1)[..., 0].T.tobytes()
    return res


@pytest.mark.parametrize("dtype", ec.DTYPE_NAMES)
@pytest.mark.parametrize("V", ec.V_SWEEP)
def test_logit_scores_vocabulary_sweep(V, dtype):
    """V at and next to the 16-byte vector width and the multiples of the chunk, rows on and off the 16-byte grid: both
    meet the restatement, and give the same bits (the element -> lane map depends on the element index only)."""
    case = ec.v_sweep_case(V, dtype)
    aligned = _score(case)
    assert all(s.data_ptr() % 16 == 0 for s in _steps(case))
    off = _steps(case, misaligned=True)
    assert all(s.data_ptr() % 16 != 0 for s in off)
    _equal_bits(_all(aligned), _all(_score(case, misaligned=True)), f"{case['name']}: aligned vs misaligned")


@pytest.mark.parametrize("finfo_min", [False, True], ids=["inf", "min"])
@pytest.mark.parametrize("dtype", ec.DTYPE_NAMES)
@pytest.mark.parametrize("V", ec.MASK_VOCABS)
def test_logit_scores_masked_rows(V, dtype, finfo_min):
    """k in {1, 2, 50} survivors of a top-k mask at a real vocabulary, placed in the first chunk, the last (partial) one,
    spread over the chunks, in one lane's elements and at the row's end: nearly every lane and most chunks are empty.
    Masked tokens get -inf exactly; the row whose tokens are all masked has NaN as its mean of finite log-probs, and so
    has normalized_entropy.  With finfo(dtype).min as the mask value every number is finite."""
    case = ec.masked_case(V, dtype, finfo_min)
    b = case["all_tokens_masked_row"]
    res = _score(case)
    lp = _np(res.log_probs)
    if finfo_min:
        assert np.isfinite(lp).all() and np.isfinite(_np(res.token_entropy)).all() and np.isfinite(res.normalized_entropy)
    else:
        assert np.isneginf(lp[:, 1]).all() and np.isfinite(lp[:b, 0]).all() and np.isneginf(lp[b]).all()
        assert np.isnan(res.normalized_entropy) and np.isposinf(_np(res.perplexity)).all()
    # without that row normalized_entropy is a number, and every row keeps its bits
    part = _score(case, rows=slice(0, b))
    assert np.isfinite(part.normalized_entropy)
    _equal_bits(_all(part)[:4], [a[:b] for a in _all(res)[:4]], f"{case['name']}: rows alone")
    _equal_bits(_all(res), _all(_score(case, misaligned=True)), f"{case['name']}: aligned vs misaligned")


@pytest.mark.parametrize("dtype", ec.DTYPE_NAMES)
@pytest.mark.parametrize("V", ec.EQUAL_VOCABS)
def test_logit_scores_all_equal_rows(V, dtype):
    """V equal logits: every element is a maximum.  Entropy 1 and log-prob -log V in closed form (V = 1: 0 / log 1, NaN
    at the restatement's places, and log-prob 0)."""
    case = ec.equal_rows_case(V, dtype)
    res = _score(case)
    assert_log_probs(_np(res.log_probs), np.full((3, 1), -np.log(V)), case["name"], 2e-6)
    if V > 1:
        assert_close(_np(res.token_entropy), np.ones((3, 1)), 1e-6, False, f"{case['name']} entropy")
    else:
        assert np.isnan(_np(res.token_entropy)).all()
    _equal_bits(_all(res), _all(_score(case, misaligned=True)), f"{case['name']}: aligned vs misaligned")


@pytest.mark.parametrize("dtype", ec.DTYPE_NAMES)
def test_logit_scores_repeated_maxima(dtype):
    """Two or three equal maxima in one lane's elements, in neighbouring lanes, in different waves, in different chunks,
    and with the row's last element (a chunk of one) among them: exactly one of them is the max's own term."""
    case = ec.maxima_case(dtype)
    res = _score(case)
    _equal_bits(_all(res), _all(_score(case, misaligned=True)), f"{case['name']}: aligned vs misaligned")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("lead", ec.PEAK_LEADS)
def test_logit_scores_peaked_rows(lead, dtype):
    """One logit ahead of 50 256 Gaussian ones by 10 .. 120, in the first chunk, a middle one and the last: entropies down
    to 1e-46 compared absolutely, the winner's log-prob (about -s') and another token's (about -lead) with the f64 values."""
    case = ec.peaked_case(lead, dtype)
    res = _score(case)
    ent = _np(res.token_entropy)
    assert (ent >= 0).all() and (ent < (1e-3 if lead >= 30 else 0.1)).all()
    assert (_np(res.log_probs)[:, 0] <= 0).all()


@pytest.mark.parametrize("dtype,mag", ec.EXTREMES, ids=lambda v: str(v))
def test_logit_scores_half_type_extremes(dtype, mag):
    """Rows holding +mag and -mag at the ends of the f16 and bf16 ranges: finite inputs, finite results equal to the
    restatement.  At 3e38 the gap m - x = 6e38 is past the f32 range."""
    case = ec.extreme_case(dtype, mag)
    res = _score(case)
    for a in _all(res):
        assert np.isfinite(a).all(), case["name"]
    _equal_bits(_all(res), _all(_score(case, misaligned=True)), f"{case['name']}: aligned vs misaligned")
    # a token at -mag in a row whose max is +mag: its log-prob -2 mag - log1p(s') in f64, rounded to the f32 output
    b, tok = case["overflow_token"]
    scores = _steps(case)
    seq = torch.from_numpy(case["tokens"].copy())
    seq[b, 0] = tok
    got = _np(transition_scores(seq.cuda(), scores, normalize_logits=True))[b, 0]
    exp = restate(case["x"].astype(np.float64), seq.numpy())["log_probs"][b, 0]
    with np.errstate(over="ignore"):
        exp32 = np.float64(np.float32(exp))
    assert np.isfinite(exp) and np.isneginf(exp32) == (2 * case["mag"] > float(np.finfo(np.float32).max))
    assert got == exp32 if np.isneginf(exp32) else abs(got - exp) <= 2e-6 * abs(exp), (got, exp)


@pytest.mark.parametrize("T", ec.BATCH_STEPS)
@pytest.mark.parametrize("B", ec.BATCH_SIZES)
def test_logit_scores_batches_past_sixteen_rows(B, T):
    """The sequence kernel gives each of its 16 waves one row per trip and each lane 64-strided steps: B in {16, 17, 33,
    100} and T around 64 against the restatement, and every row's bits against the same row scored alone."""
    case = ec.batch_case(B, T)
    res = _score(case)
    assert np.isfinite(res.normalized_entropy)
    full = _all(res)
    scores = _steps(case)
    seq = torch.from_numpy(case["tokens"]).cuda()
    for b in range(B):  # every row alone: the same bits
        one = _all(generation_scores(seq[b:b + 1], tuple(s[b:b + 1] for s in scores)))
        _equal_bits(one[:4], [a[b:b + 1] for a in full[:4]], f"{case['name']} row {b} alone")
    for b in sorted({0, 15, 16, B - 1} & set(range(B))):  # and against the restatement of the row alone
        _score(case, rows=slice(b, b + 1))


@pytest.mark.parametrize("device", ["cpu", "cuda"])
@pytest.mark.parametrize("which", ec.BAD_TOKEN_IDS)
@pytest.mark.parametrize("column", [0, 2], ids=["first", "last"])
def test_logit_scores_token_ids_out_of_range_raise(which, column, device):
    """The wrapper's [0, V) check, for host and device ids.  Its validation step is called first: were the check missing,
    this fails there, in Python, before the public entry points could launch a kernel with the bad id."""
    V, B, T = 7, 2, 3
    scores = tuple(torch.zeros(B, V, device="cuda") for _ in range(T))
    bad = torch.from_numpy(ec.bad_token_sequences(which, column, V, B, T)).to(device)
    with pytest.raises(ValueError, match=r"\[0, 7\)"):
        _token_ids(bad, B, T, V)
    for call in (lambda: generation_scores(bad, scores), lambda: transition_scores(bad, scores, normalize_logits=True),
                 lambda: transition_scores(bad, scores)):
        with pytest.raises(ValueError, match=r"\[0, 7\)"):
            call()
    # a bad id in a prompt column is not scored and not checked (HF gathers the last T columns only)
    ok = bad.clone()
    ok[1, 5 + column] = V - 1
    ok[0, 4] = bad[1, 5 + column]
    assert torch.equal(_token_ids(ok, B, T, V), ok[:, 5:])
    res = generation_scores(ok, scores)
    assert_log_probs(_np(res.log_probs), np.full((B, T), -np.log(V)), "valid ids", 2e-6)
