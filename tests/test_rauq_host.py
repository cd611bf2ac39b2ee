"""RAUQ without a GPU: the C ABI's new entry points and their argument checks, the Python contract of
runia_core_amd.llm_uncertainty's four RAUQ names, and a NumPy f64 restatement of the three modes checked against every
score of the reference fixture (tests/golden/ref_rauq.npz, tools/make_goldens_rauq.py).  The GPU tests
(test_rauq_gpu.py) check the kernels against this restatement at sizes the fixture cannot hold."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle.hotpath import torch_cpu_sum_lastdim
from runia_core_amd import _hip

RAUQ_SYMBOLS = ["runia_rauq_gather", "runia_rauq_rollout_att", "runia_rauq_rollout_rows", "runia_rauq_score",
                "runia_rauq_workspace_bytes"]
HEADS = ("original", "mean_heads", "rollout")
TOKENS = ("original", "mean_all_tokens")


# ---- restatement (f64) ------------------------------------------------------------------------------------------------
def round_to_dtype(x, dtype: str):
    """f64 values -> f32 -> the map dtype (round to nearest even) -> f64, as torch stores a bf16 / f16 mean."""
    x32 = np.asarray(x, dtype=np.float32)
    if dtype == "float16":
        return x32.astype(np.float16).astype(np.float64)
    if dtype == "bfloat16":
        u = x32.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32).astype(np.float64)
    return x32.astype(np.float64)


def f32_mean_lastdim(a):
    """torch's f32 mean over a contiguous last dimension: its summation order (oracle.hotpath, exact below 512 elements),
    then one f32 division.  Softmax rows all average to ~1/k, so which head "attends most" in the mean_all_tokens mode is
    decided in the last bits: the head choice is only reproducible with the reference's own f32 sums."""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (torch_cpu_sum_lastdim(a) / np.float32(a.shape[-1])).astype(np.float32)


def gather_values(steps, token_aggregation, dtype):
    """(L, H, N): attn[0, h, 0, -2] of steps 1.. or the row mean of query row 0 of every step (steps: (L, H, q, k))."""
    if token_aggregation == "original":
        return np.stack([s[:, :, 0, -2] for s in steps[1:]], axis=-1).astype(np.float64)
    return np.stack([round_to_dtype(f32_mean_lastdim(s[:, :, 0, :]), dtype) for s in steps], axis=-1)


def argmax_heads(w):
    """argmax_h mean_{i >= 1} w[l, h, i] (NaN is the maximum, first index wins - numpy's argmax does both)."""
    means = f32_mean_lastdim(w[:, :, 1:]) if w.shape[2] > 1 else np.full(w.shape[:2], np.nan)
    return np.argmax(means, axis=1)


def recurrence(series, probs, alphas):
    """series (L, N) -> max over layers of -mean log conf, per alpha."""
    L, N = series.shape
    out = []
    for a in alphas:
        conf = np.zeros((N, L))
        conf[0] = probs[0]
        for i in range(1, N):
            conf[i] = a * probs[i] + (1 - a) * series[:, i] * conf[i - 1]
        with np.errstate(divide="ignore"):
            out.append(float((-np.log(conf).mean(0)).max()))
    return out


def rollout_values(steps, input_length, n, token_aggregation):
    """joint.diagonal(-1)[-n:] or joint[:, -n:].mean(0) of the reconstructed maps, in f64."""
    L, H = steps[0].shape[:2]
    T = input_length + len(steps)
    full = np.zeros((L, H, T, T))
    full[:, :, :input_length, :input_length] = steps[0]  # broadcasts a single query row, as the reference's assignment
    for g, s in enumerate(steps[1:], start=1):
        full[:, :, input_length + g, : input_length + g] = s[:, :, 0, :]
    joint = np.eye(T)
    for l in range(L):
        a = full[l].mean(0) + np.eye(T)
        joint = (a / a.sum(-1, keepdims=True)) @ joint
    return joint.diagonal(-1)[-n:] if token_aggregation == "original" else joint[:, -n:].mean(0)


def restate(steps, dtype, lp, input_length, alphas, head_aggregation, token_aggregation):
    """Scores (list, one per alpha) and, for head_aggregation "original", the chosen heads."""
    probs = np.exp(np.asarray(lp, dtype=np.float64)).reshape(-1)
    if head_aggregation == "rollout":
        att = rollout_values(steps, input_length, probs.size, token_aggregation)
        return recurrence(att[None, :], probs, alphas), None
    w = gather_values(steps, token_aggregation, dtype)
    if head_aggregation == "mean_heads":
        return recurrence(w.mean(1), probs, alphas), None
    heads = argmax_heads(w)
    return recurrence(w[np.arange(w.shape[0]), heads], probs, alphas), heads


def fixture_cases():
    with np.load(os.path.join(ROOT, "tests", "golden", "ref_rauq.npz"), allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    cases = []
    for name in data["cases"]:
        name = str(name)
        n_steps = len([k for k in data if k.startswith(name + "__step")])
        cases.append(dict(name=name, steps=[data[f"{name}__step{g}"].astype(np.float64) for g in range(n_steps)],
                          dtype=str(data[f"{name}__dtype"]), lp=data[f"{name}__lp"], lp2d=bool(data[f"{name}__lp2d"]),
                          input_length=int(data[f"{name}__in"]), alphas=[float(a) for a in data[f"{name}__alphas"]],
                          scores={(h, t): data[f"{name}__{h}__{t}"] for h in HEADS for t in TOKENS},
                          heads={t: data[f"{name}__heads__{t}"] for t in TOKENS}))
    return cases


# ---- tests ------------------------------------------------------------------------------------------------------------
def test_rauq_symbols_in_header_table_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(runia_rauq_[a-z0-9_]+)\s*\(", text))
    assert sorted(declared) == RAUQ_SYMBOLS
    assert set(RAUQ_SYMBOLS) <= set(_hip.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True).stdout
    assert set(RAUQ_SYMBOLS) <= set(re.findall(r"\bT (runia_[a-z0-9_]+)", out))
    assert _hip.load_library().runia_abi_version() == 6


def test_rauq_argument_checks_before_any_launch():
    """Null pointers, bad sizes, dtypes and modes return RUNIA_E_INVALID (-1); a short, missing or misaligned workspace
    RUNIA_E_WORKSPACE (-4).  Every call below returns before touching a device (none is needed)."""
    lib = _hip.load_library()
    fake = 1 << 20  # a non-null, aligned address that is never dereferenced: every call fails its checks first
    # workspace sizes: zero for nonsense, growing with the chain rows
    assert lib.runia_rauq_workspace_bytes(0, 4, 8, 4, 1, 1) == 0
    assert lib.runia_rauq_workspace_bytes(4, 4, -1, 4, 1, 1) == 0
    w0 = lib.runia_rauq_workspace_bytes(4, 4, 8, 4, 0, 1)
    w1 = lib.runia_rauq_workspace_bytes(4, 4, 8, 4, 1, 1)
    wn = lib.runia_rauq_workspace_bytes(4, 4, 8, 4, 4, 1)
    assert 0 < w0 < w1 < wn
    # gather: null table / output, bad dtype, bad token aggregation, n_gen = 1 for "original" (no token), bad sizes
    assert lib.runia_rauq_gather(None, 0, 4, 2, 2, 0, fake, None) == -1
    assert lib.runia_rauq_gather(fake, 0, 4, 2, 2, 0, None, None) == -1
    assert lib.runia_rauq_gather(fake, 3, 4, 2, 2, 0, fake, None) == -1
    assert lib.runia_rauq_gather(fake, 0, 4, 2, 2, 2, fake, None) == -1
    assert lib.runia_rauq_gather(fake, 0, 1, 2, 2, 0, fake, None) == -1
    assert lib.runia_rauq_gather(fake, 0, 4, 0, 2, 0, fake, None) == -1
    assert lib.runia_rauq_gather(fake, 0, 4, 2, 0, 1, fake, None) == -1
    # score
    need = lib.runia_rauq_workspace_bytes(2, 5, 0, 0, 0, 3)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(att=fake, L=2, H=4, N=5, mode=0, lp=fake, al=fake, na=3, sc=fake, hd=fake,
                                                         ws=fake, wb=need, st=None).items()]  # noqa: E731
    assert lib.runia_rauq_score(*args(att=None)) == -1
    assert lib.runia_rauq_score(*args(lp=None)) == -1
    assert lib.runia_rauq_score(*args(al=None)) == -1
    assert lib.runia_rauq_score(*args(sc=None)) == -1
    assert lib.runia_rauq_score(*args(na=0)) == -1
    assert lib.runia_rauq_score(*args(N=0)) == -1
    assert lib.runia_rauq_score(*args(mode=3)) == -1
    assert lib.runia_rauq_score(*args(mode=2)) == -1  # one series: L = H = 1
    assert lib.runia_rauq_score(*args(wb=need - 1)) == -4
    assert lib.runia_rauq_score(*args(ws=None)) == -4
    assert lib.runia_rauq_score(*args(ws=fake + 4)) == -4
    # rollout row pass and attention
    flag = fake
    need = lib.runia_rauq_workspace_bytes(3, 4, 8, 0, 0, 1)
    assert lib.runia_rauq_rollout_rows(None, 0, 4, 3, 2, 8, flag, fake, need, None) == -1
    assert lib.runia_rauq_rollout_rows(fake, 0, 4, 3, 2, 8, None, fake, need, None) == -1
    assert lib.runia_rauq_rollout_rows(fake, 0, 1, 3, 2, 8, flag, fake, need, None) == -1  # n_gen = 1
    assert lib.runia_rauq_rollout_rows(fake, 0, 4, 3, 2, 0, flag, fake, need, None) == -1  # no prompt
    assert lib.runia_rauq_rollout_rows(fake, 0, 4, 3, 2, 8, flag, fake, need - 1, None) == -4
    need = lib.runia_rauq_workspace_bytes(3, 4, 8, 4, 1, 1)
    assert lib.runia_rauq_rollout_att(fake, 0, 4, 3, 2, 8, 0, 0, 4, None, fake, need, None) == -1
    assert lib.runia_rauq_rollout_att(fake, 0, 4, 3, 2, 8, 1, 0, 4, fake, fake, need, None) == -1  # one pass: "original" only
    assert lib.runia_rauq_rollout_att(fake, 0, 4, 3, 2, 8, 0, 3, 4, fake, fake, need, None) == -1  # route
    assert lib.runia_rauq_rollout_att(fake, 0, 4, 3, 2, 8, 0, 0, 12, fake, fake, need, None) == -1  # n > T - 1
    assert lib.runia_rauq_rollout_att(fake, 0, 4, 3, 2, 8, 1, 1, 13, fake, fake, need, None) == -1  # n > T
    assert lib.runia_rauq_rollout_att(fake, 0, 4, 3, 2, 8, 1, 1, 4, fake, fake, need - 1, None) == -4
    assert lib.runia_rauq_rollout_att(fake, 0, 4, 3, 2, 8, 0, 2, 4, fake, fake, need, None) == -4  # 4-row chain: more


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_every_fixture_score(case):
    for h in HEADS:
        for t in TOKENS:
            lp = case["lp"].reshape(1, -1) if h == "rollout" else case["lp"]
            got, heads = restate(case["steps"], case["dtype"], lp, case["input_length"], case["alphas"], h, t)
            exp = case["scores"][(h, t)]
            np.testing.assert_allclose(got, exp, rtol=1e-5, atol=0, err_msg=f"{case['name']} {h} {t}")
            if h == "original":
                np.testing.assert_array_equal(heads, case["heads"][t])


def _mock(n_tok=4, n_l=2, n_h=3, seq=6, batch=1):
    g = torch.Generator().manual_seed(0)
    att = tuple(tuple(torch.softmax(torch.randn(batch, n_h, 1, seq + t, generator=g), -1) for _ in range(n_l))
                for t in range(n_tok))
    return att, torch.randn(1, n_tok, generator=g)


def test_rauq_python_contract_without_a_device(monkeypatch):
    from runia_core_amd.llm_uncertainty import RAUQ, rauq_uncertainty, rauq_uncertainty_mean_heads, rauq_uncertainty_rollout
    import runia_core_amd.llm_uncertainty as pkg

    assert {"RAUQ", "rauq_uncertainty", "rauq_uncertainty_mean_heads", "rauq_uncertainty_rollout"} <= set(pkg.__all__)
    att, lp = _mock()
    # unknown aggregation names: KeyError, as the reference's dict lookups
    with pytest.raises(KeyError):
        rauq_uncertainty(lp[0], att, "bogus")
    with pytest.raises(KeyError):
        rauq_uncertainty_mean_heads(lp[0], att, "bogus")
    with pytest.raises(KeyError):
        rauq_uncertainty_rollout(lp, att, "bogus", 6)
    with pytest.raises(KeyError):
        RAUQ(lp, att, 6, "original", "bogus", [0.2], False)
    # rollout: batch > 1, one step, shapes that do not fit input_length, 1-D log-probs - all before any launch
    att2, _ = _mock(batch=2)
    with pytest.raises(ValueError, match="batch size 1"):
        rauq_uncertainty_rollout(lp, att2, "original", 6)
    with pytest.raises(ValueError, match="two generation steps"):
        rauq_uncertainty_rollout(lp[:, :1], att[:1], "original", 6)
    with pytest.raises(ValueError, match="does not fit"):
        rauq_uncertainty_rollout(lp, att, "original", 5)
    with pytest.raises(IndexError):
        rauq_uncertainty_rollout(lp[0], att, "original", 6)
    with pytest.raises(TypeError):
        rauq_uncertainty(lp[0], tuple(tuple(t.double() for t in s) for s in att), "original")
    # a valid call without a device raises: there is no host fallback
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for call in (lambda: rauq_uncertainty(lp[0], att, "original"),
                 lambda: rauq_uncertainty_mean_heads(lp[0], att, "mean_all_tokens"),
                 lambda: rauq_uncertainty_rollout(lp, att, "mean_all_tokens", 6),
                 lambda: RAUQ(lp, att, 6, "original", "rollout", [0.4], True)):
        with pytest.raises(_hip.RuniaHipError):
            call()


# ---- the inputs of the GPU tests at the summation-order switch (rauq_switch_cases.py) --------------------------------
import rauq_switch_cases as sw  # noqa: E402


def switch_rows():
    """(name, input_length, n_gen, seed, steps maker) of every one-row input the GPU switch tests score: the prompt
    lengths that put k at 510 .. 513, the generation crossing 512, and the batch's rows on their own."""
    rows = [(f"k{k}", k, 3, 100 + k) for k in sw.SWITCH_KS]
    rows.append(("generation", sw.GENERATION["input_length"], sw.GENERATION["n_gen"], 200))
    rows += [(f"batch_row{b}", sw.BATCH["input_length"] - pad, n, 300 + 10 * b)
             for b, (pad, n) in enumerate(zip(sw.BATCH["pads"], sw.BATCH["lengths"]))]
    return rows


@pytest.mark.parametrize("dtype", list(sw.DTYPES))
@pytest.mark.parametrize("tie", [False, True], ids=["margin", "tie"])
def test_switch_inputs_cross_512_with_a_clear_head_margin(dtype, tie):
    """The per-head mode picks a head by argmax over means that differ in their last bits for plain softmax rows.  On
    these inputs the oracle's two largest head means differ by at least 1e-3 relative in every layer, so the choice does
    not hang on a summation order; in the tie inputs heads 1 and 3 are bitwise equal and largest, the next is 1e-3 lower,
    and the reference's argmax takes head 1."""
    ks = set()
    for name, inp, n_gen, seed in switch_rows():
        steps = sw.one_row_steps(inp, n_gen, dtype, seed, tie)[:n_gen]
        assert [s.shape for s in steps] == [(sw.L, sw.H, inp, inp)] + [(sw.L, sw.H, 1, inp + g) for g in range(1, n_gen)]
        for s in steps:
            np.testing.assert_array_equal(sw._representable(s, dtype), s)
        assert not np.triu(steps[0], 1).any()  # causal
        ks |= {s.shape[-1] for s in steps}
        w = gather_values([s.astype(np.float64) for s in steps], "mean_all_tokens", dtype)
        means = f32_mean_lastdim(w[:, :, 1:]).astype(np.float64)
        heads = argmax_heads(w)
        for l in range(sw.L):
            order = np.argsort(-means[l], kind="stable")
            if tie:
                assert sorted(order[:2]) == list(sw.TIE_HEADS) and means[l, order[0]] == means[l, order[1]], (name, l)
                assert np.array_equal(w[l, sw.TIE_HEADS[0]], w[l, sw.TIE_HEADS[1]])
                assert heads[l] == sw.TIE_HEADS[0]
                order = order[1:]
            assert means[l, order[0]] - means[l, order[1]] >= 1e-3 * means[l, order[0]], (name, l, means[l])
    assert {509, 510, 511, 512, 513, 514} <= ks and sw.SWITCH == 512
    # the batch: at one step some row is under 512 columns and another at or over it
    inp, pads = sw.BATCH["input_length"], sw.BATCH["pads"]
    assert any(min(inp - p + g for p in pads) < 512 <= max(inp - p + g for p in pads) for g in range(sw.BATCH["n_gen"]))
    b_steps = sw.batch_steps(dtype, 300, tie)
    for b, pad in enumerate(pads):
        own = sw.one_row_steps(inp - pad, sw.BATCH["n_gen"], dtype, 300 + 10 * b, tie)
        for g, s in enumerate(b_steps):
            got = s[b, :, :, pad:, pad:] if g == 0 else s[b, :, :, :, pad:]
            np.testing.assert_array_equal(got, own[g])
            assert not s[b, ..., :pad].any()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_row_mean_orders_are_torchs_below_512_and_differ_from_the_wave_order():
    """The expected values of test_rauq_gathered_row_means_are_bitwise_* (test_rauq_gpu.py).  Below 512 columns torch's own
    CPU f32 mean(-1) of the rows equals the oracle's restatement of its cascade order bit for bit (the oracle was verified
    up to n = 69 only).  At every tested k, on both sides of 512, the cascade order and the wave order give different bits
    on some of the rows: a kernel that used the other order there, or switched one column early or late, is seen."""
    assert sw.SWITCH == 512 and max(sw.MEAN_KS_CASCADE) == 511 and min(sw.MEAN_KS_WAVE) == 512
    assert {510, 511} <= set(sw.MEAN_KS_CASCADE) and {512, 513} <= set(sw.MEAN_KS_WAVE)
    for k in sw.MEAN_KS_CASCADE + sw.MEAN_KS_WAVE:
        a = sw.mean_rows(k)
        assert a.shape == (sw.MEAN_L, sw.MEAN_H, 1, k) and a.dtype == np.float32 and (a > 0).all()
        cascade, wave = f32_mean_lastdim(a), sw.wave_order_mean(a)
        np.testing.assert_allclose(wave, a.astype(np.float64).mean(-1), rtol=1e-6)
        np.testing.assert_allclose(cascade, a.astype(np.float64).mean(-1), rtol=1e-6)
        assert (_bits(cascade) != _bits(wave)).sum() >= 8, k
        if k < sw.SWITCH:
            np.testing.assert_array_equal(_bits(torch.from_numpy(a).mean(-1).numpy()), _bits(cascade), err_msg=f"k = {k}")
    # the wave order by hand on a row whose sum depends on it: lanes 0 and 1 of two trips, then the butterfly
    row = np.zeros(128, dtype=np.float32)
    row[[0, 64, 1]] = [1.0, 2.0 ** -24, 2.0 ** -24]
    # lane 0: 1 + 2^-24 -> 1 (ties to even), then + lane 1's 2^-24 -> 1; index order would give 1 + 2^-23
    assert sw.wave_order_mean(row[None])[0] == np.float32(1.0) / np.float32(128)
    assert np.float32(np.float32(row[1] + row[64]) + row[0]) / np.float32(128) != np.float32(1.0) / np.float32(128)
