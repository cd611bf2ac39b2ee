"""Inputs, the f64 reference and the derived error bounds of the logit-lens tests: states N(0, 1), weights N(0, 9 / d), both
rounded to the tested dtype (logits spread about 3).  The bounds are derived from the reference, not measured: with eps =
(d + 32) 2^-24 max_v sum_k |x_k| |W_vk| (an f32 sum of d exact products in any order) and r = 2^-20 (1 + max_v |z_v|),
    lse                      eps + r
    log_prob, top_log_prob   2 eps + r
    entropy                  2 a eps + r,        a = sum_v p_v |log p_v + H|   (the L1 norm of the entropy's gradient)
    kl_final                 2 (2 + b) eps' + r, b = sum_v q_v |log(q_v / p_v) - KL|, eps' the larger eps of the two rows.
"""
import numpy as np
import torch

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
FIELDS = ("lse", "entropy", "log_prob", "top_log_prob", "kl_final")


def reference(x: torch.Tensor, w: torch.Tensor, tokens=None, final=-1):
    """``{field: (planes, N) f64}``, ``top_token``, ``bound_<field>`` and ``gap_ok`` of host tensors x (planes, N, d), w (V, d)."""
    xs, ws = x.double().numpy(), w.double().numpy()
    d = xs.shape[-1]
    z = xs @ ws.T
    m = z.max(-1)
    lse = m + np.log(np.exp(z - m[..., None]).sum(-1))
    logp = z - lse[..., None]
    p = np.exp(logp)
    ent = -(p * logp).sum(-1)
    out = {"lse": lse, "entropy": ent, "top_log_prob": m - lse, "top_token": z.argmax(-1)}
    nan = np.full(lse.shape, np.nan)
    out["log_prob"] = nan.copy()
    if tokens is not None:
        t = np.asarray(tokens)
        ok = t >= 0
        out["log_prob"][:, ok] = logp[:, ok, t[ok]]
    eps = (d + 32) * 2.0 ** -24 * (np.abs(xs) @ np.abs(ws).T).max(-1)
    r = 2.0 ** -20 * (1 + np.abs(z).max(-1))
    out["bound_lse"] = eps + r
    out["bound_log_prob"] = out["bound_top_log_prob"] = 2 * eps + r
    out["bound_entropy"] = 2 * (p * np.abs(logp + ent[..., None])).sum(-1) * eps + r
    out["kl_final"], out["bound_kl_final"] = nan.copy(), nan.copy()
    if final >= 0:
        q, logq = p[final][None], logp[final][None]
        kl = (q * (logq - logp)).sum(-1)
        b = (q * np.abs(logq - logp - kl[..., None])).sum(-1)
        out["kl_final"], out["bound_kl_final"] = kl, 2 * (2 + b) * np.maximum(eps, eps[final][None]) + r
    top2 = np.sort(z, -1)[..., -2:] if z.shape[-1] > 1 else np.stack([z[..., 0] - 1, z[..., 0]], -1)
    out["gap_ok"] = bool((top2[..., 1] - top2[..., 0] > 4 * eps).all())
    return out


def make(seed, planes, N, V, d, dtype="bf16", tokens=True, final=-1):
    """``(x, w, tokens, ref)``: host tensors of ``dtype`` and their reference; the first seed from ``seed`` on whose rows all
    have a top-two logit gap above 4 eps (so the arg-max is decided within the kernel's error)."""
    for s in range(seed, seed + 20):
        rng = np.random.default_rng(s)
        x = torch.from_numpy(rng.standard_normal((planes, N, d))).to(DTYPES[dtype])
        w = torch.from_numpy(rng.standard_normal((V, d)) * 3 / np.sqrt(d)).to(DTYPES[dtype])
        tok = torch.from_numpy(rng.integers(0, V, N)) if tokens else None
        ref = reference(x, w, tok, final)
        if ref["gap_ok"]:
            return x, w, tok, ref
    raise AssertionError("no seed with a decided arg-max")
