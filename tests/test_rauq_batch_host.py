"""Batched RAUQ without a GPU: the C ABI's runia_rauqb_* entry points and their argument checks, every check of
rauq_batch that fires before a launch, generated_lengths, and an f64 restatement of the per-row contract (each row's own
slices through test_rauq_host's restatement) checked against every score of the reference fixture
(tests/golden/ref_rauq_batch.npz, tools/make_goldens_rauq_batch.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from runia_core_amd import _hip
from test_rauq_host import HEADS, TOKENS, restate

RAUQB_SYMBOLS = ["runia_rauqb_gather", "runia_rauqb_rollout_att", "runia_rauqb_rollout_rows", "runia_rauqb_score",
                 "runia_rauqb_workspace_bytes"]


def batch_fixture_cases():
    with np.load(os.path.join(ROOT, "tests", "golden", "ref_rauq_batch.npz"), allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    cases = []
    for name in data["cases"]:
        name = str(name)
        n_steps = len([k for k in data if k.startswith(name + "__step")])
        cases.append(dict(name=name, steps=[data[f"{name}__step{g}"] for g in range(n_steps)], dtype=str(data[f"{name}__dtype"]),
                          mask=data[f"{name}__mask"], lengths=data[f"{name}__lengths"], lp=data[f"{name}__lp"],
                          input_length=int(data[f"{name}__in"]), alphas=[float(a) for a in data[f"{name}__alphas"]],
                          scores={(h, t): data[f"{name}__{h}__{t}"] for h in HEADS for t in TOKENS}))
    return cases


def row_steps(steps, pad, n, b):
    """Row b's slices of (B, L, H, q, k) steps as test_rauq_host's (L, H, q, k) steps."""
    return [(s[b, :, :, pad:, pad:] if g == 0 else s[b, :, :, :, pad:]).astype(np.float64) for g, s in enumerate(steps[:n])]


def restate_batch(case, head, tok):
    """(B, n_alpha) f64 restatement; NaN where the one-row call raises."""
    out = []
    for b in range(case["mask"].shape[0]):
        pad, n = int((case["mask"][b] == 0).sum()), int(case["lengths"][b])
        if n < 2 and (tok == "original" or head == "rollout"):
            out.append([np.nan] * len(case["alphas"]))
            continue
        lp = case["lp"][b, :n]
        got, _ = restate(row_steps(case["steps"], pad, n, b), case["dtype"], lp.reshape(1, -1) if head == "rollout" else lp,
                         case["input_length"] - pad, case["alphas"], head, tok)
        out.append(got)
    return np.array(out, dtype=np.float64)


# ---- tests ------------------------------------------------------------------------------------------------------------
def test_rauqb_symbols_in_header_table_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "runia_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(runia_rauqb_[a-z0-9_]+)\s*\(", text))
    assert sorted(declared) == RAUQB_SYMBOLS
    assert set(RAUQB_SYMBOLS) <= set(_hip.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.library_path()], capture_output=True, text=True).stdout
    assert set(RAUQB_SYMBOLS) <= set(re.findall(r"\bT (runia_[a-z0-9_]+)", out))
    assert _hip.load_library().runia_abi_version() == 6


def test_rauqb_argument_checks_before_any_launch():
    """RUNIA_E_INVALID (-1) for null pointers and bad sizes, RUNIA_E_WORKSPACE (-4) for a short, missing or misaligned
    workspace; every call returns before touching a device."""
    lib = _hip.load_library()
    fake = 1 << 20
    assert lib.runia_rauqb_workspace_bytes(0, 4, 4, 8, 1, 1) == 0
    assert lib.runia_rauqb_workspace_bytes(2, 0, 4, 8, 1, 1) == 0
    assert lib.runia_rauqb_workspace_bytes(2, 4, 4, -1, 1, 1) == 0
    w1 = lib.runia_rauqb_workspace_bytes(1, 4, 4, 8, 0, 1)
    w2 = lib.runia_rauqb_workspace_bytes(2, 4, 4, 8, 0, 1)
    w2k = lib.runia_rauqb_workspace_bytes(2, 4, 4, 8, 4, 1)
    assert 0 < w1 < w2 < w2k
    # gather: table, rows, output, dtype, token aggregation, batch, n_gen = 1 for "original"
    g = lambda **kw: lib.runia_rauqb_gather(*[kw.get(k, v) for k, v in dict(tab=fake, rows=fake, dt=0, B=2, n=4, L=2, H=2, tok=0,  # noqa: E731
                                                                              w=fake, st=None).items()])
    for bad in (dict(tab=None), dict(rows=None), dict(w=None), dict(dt=3), dict(tok=2), dict(B=0), dict(B=1 << 17),
                dict(n=1), dict(L=0), dict(H=0)):
        assert g(**bad) == -1, bad
    # score
    need = lib.runia_rauqb_workspace_bytes(3, 2, 5, 0, 0, 3)
    s = lambda **kw: lib.runia_rauqb_score(*[kw.get(k, v) for k, v in dict(att=fake, rows=fake, B=3, L=2, H=4, N=5, mode=0, tok=0,  # noqa: E731
                                                                             lp=fake, lps=5, al=fake, na=3, sc=fake, ws=fake,
                                                                             wb=need, st=None).items()])
    for bad in (dict(att=None), dict(rows=None), dict(lp=None), dict(al=None), dict(sc=None), dict(na=0), dict(N=0),
                dict(B=0), dict(mode=3), dict(mode=2), dict(tok=2), dict(lps=0)):
        assert s(**bad) == -1, bad
    assert s(wb=need - 1) == -4
    assert s(ws=None) == -4
    assert s(ws=fake + 4) == -4
    # rollout row pass
    need = lib.runia_rauqb_workspace_bytes(2, 3, 4, 8, 0, 1)
    r = lambda **kw: lib.runia_rauqb_rollout_rows(*[kw.get(k, v) for k, v in dict(tab=fake, rows=fake, dt=0, B=2, n=4, L=3, H=2,  # noqa: E731
                                                                                    inp=8, fl=fake, ws=fake, wb=need,
                                                                                    st=None).items()])
    for bad in (dict(tab=None), dict(rows=None), dict(fl=None), dict(n=1), dict(inp=0), dict(B=0), dict(dt=-1)):
        assert r(**bad) == -1, bad
    assert r(wb=need - 1) == -4
    assert r(ws=fake + 8) == -4
    # rollout attention: the host row table is checked, and the chain rows size the workspace
    host_rows = np.array([[0, 4], [3, 4]], dtype=np.int64)
    clear = np.zeros(2, dtype=np.int32)
    upper = np.array([0, 1], dtype=np.int32)
    need0 = lib.runia_rauqb_workspace_bytes(2, 3, 4, 8, 0, 1)
    needk = lib.runia_rauqb_workspace_bytes(2, 3, 4, 8, 4, 1)

    def a(**kw):
        args = dict(tab=fake, rows=fake, hr=host_rows.ctypes.data, fl=fake, hu=clear.ctypes.data, dt=0, B=2, n=4, L=3, H=2,
                    inp=8, tok=0, att=fake, ws=fake, wb=need0, st=None)
        args.update(kw)
        return lib.runia_rauqb_rollout_att(*args.values())

    for bad in (dict(tab=None), dict(rows=None), dict(hr=None), dict(fl=None), dict(hu=None), dict(att=None), dict(n=1),
                dict(inp=0), dict(tok=2), dict(B=0)):
        assert a(**bad) == -1, bad
    for rows in ([[8, 4], [0, 4]], [[-1, 4], [0, 4]], [[0, 0], [0, 4]], [[0, 5], [0, 4]]):
        bad_rows = np.array(rows, dtype=np.int64)
        assert a(hr=bad_rows.ctypes.data) == -1, rows
    assert a(wb=need0 - 1) == -4
    assert a(ws=fake + 4) == -4
    assert a(hu=upper.ctypes.data) == -4  # row 1 takes the 4-row chain: the larger workspace
    assert a(tok=1) == -4  # every row takes the 1-row chain
    assert needk > need0


def _mock(batch=3, n_l=2, n_h=3, inp=6, n_gen=4, q0=None):
    g = torch.Generator().manual_seed(0)
    att = tuple(tuple(torch.softmax(torch.randn(batch, n_h, (q0 or inp) if s == 0 else 1, inp + s, generator=g), -1)
                      for _ in range(n_l)) for s in range(n_gen))
    return att, torch.randn(batch, n_gen, generator=g)


def test_rauq_batch_checks_before_any_launch(monkeypatch):
    from runia_core_amd.llm_uncertainty import rauq_batch
    import runia_core_amd.llm_uncertainty as pkg

    assert {"rauq_batch", "generated_lengths"} <= set(pkg.__all__)
    att, lp = _mock()
    mask = torch.tensor([[1] * 6, [0, 0, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1]])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # nothing below may reach a launch
    with pytest.raises(KeyError):
        rauq_batch(lp, att, 6, "original", "bogus", [0.2])
    with pytest.raises(KeyError):
        rauq_batch(lp, att, 6, "bogus", "mean_heads", [0.2])
    bad_masks = (torch.tensor([[1] * 6, [1, 0, 1, 1, 1, 1], [1] * 6]),  # a zero after a one
                 torch.tensor([[1] * 6, [0] * 6, [1] * 6]),  # a row of zeros
                 torch.tensor([[1] * 6, [1] * 6]))  # wrong shape
    for m in bad_masks:
        with pytest.raises(ValueError, match="attention_mask"):
            rauq_batch(lp, att, 6, "original", "original", [0.2], attention_mask=m)
    for n in ([0, 4, 4], [1, 5, 4], [4, 4]):
        with pytest.raises(ValueError, match="lengths"):
            rauq_batch(lp, att, 6, "original", "original", [0.2], mask, n)
    for bad_lp in (lp[:2], lp[:, :3], lp[0]):
        with pytest.raises(ValueError, match="log_probs"):
            rauq_batch(bad_lp, att, 6, "original", "rollout", [0.2], mask)
    mixed = tuple(tuple(t if (g or l) else t[:2] for l, t in enumerate(step)) for g, step in enumerate(att))
    with pytest.raises(ValueError, match="batch size"):
        rauq_batch(lp, mixed, 6, "original", "mean_heads", [0.2])
    with pytest.raises(ValueError, match="does not fit"):
        rauq_batch(lp, att, 5, "original", "mean_heads", [0.2])
    one_row, lp1 = _mock(q0=1)
    with pytest.raises(ValueError, match="one query row"):
        rauq_batch(lp1, one_row, 6, "mean_all_tokens", "original", [0.2], mask)
    # valid calls without a device raise: there is no host fallback
    for call in (lambda: rauq_batch(lp, att, 6, "original", "original", [0.2], mask),
                 lambda: rauq_batch(lp[:, :3], att, 6, "mean_all_tokens", "rollout", [0.4], mask, torch.tensor([3, 2, 1])),
                 lambda: rauq_batch(lp1, one_row, 6, "original", "mean_heads", [0.3])):
        with pytest.raises(_hip.RuniaHipError):
            call()


def test_generated_lengths():
    from runia_core_amd.llm_uncertainty import generated_lengths

    seq = torch.tensor([[7, 7, 2, 5, 5, 5],   # eos first
                        [7, 7, 5, 3, 2, 0],   # eos in the middle
                        [7, 7, 5, 5, 5, 5],   # none
                        [7, 2, 4, 4, 4, 2]])  # eos at the prompt position 1 does not count; 2 last
    got = generated_lengths(seq, 2, 2)
    assert got.dtype == torch.int64 and got.tolist() == [1, 3, 4, 4]
    assert generated_lengths(seq, 2, [3, 4]).tolist() == [4, 2, 4, 1]
    assert generated_lengths(seq, 2, (9,)).tolist() == [4, 4, 4, 4]


@pytest.mark.parametrize("case", batch_fixture_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_every_batch_fixture_score(case):
    for h in HEADS:
        for t in TOKENS:
            got = restate_batch(case, h, t)
            exp = case["scores"][(h, t)]
            assert got.shape == exp.shape
            np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{case['name']} {h} {t}")
            ok = ~np.isnan(exp)
            np.testing.assert_allclose(got[ok], exp[ok], rtol=1e-5 if h == "rollout" else 1e-6, atol=0,
                                       err_msg=f"{case['name']} {h} {t}")
