"""References of the LLM-Check scores (include/runia_hip.h), NumPy only.

``hidden_ref`` / ``attention_ref`` are the definition in f64: centre every token over d, ``C C^T + alpha I``, ``slogdet``; the
log of the gathered diagonals.  ``hidden_ref_hi`` states the same in ``np.longdouble`` with a column-loop Cholesky (no LAPACK)
and only sets tolerances: the device value must lie within ``16 * max(|f64 - longdouble|, 2^-50 |score|)`` of it.
"""
import numpy as np

ALPHA = 1e-3


def hidden_ref(z, alpha=ALPHA):
    z = np.asarray(z, dtype=np.float64)
    c = z - z.mean(axis=1, keepdims=True)
    sign, logdet = np.linalg.slogdet(c @ c.T + alpha * np.eye(len(z)))
    assert sign == 1 and np.isfinite(logdet), "the reference itself must be positive definite"
    return logdet / len(z)


def hidden_ref_hi(z, alpha=ALPHA):
    z = np.asarray(z, dtype=np.float64).astype(np.longdouble)
    c = z - z.mean(axis=1, keepdims=True)
    a = c @ c.T + np.longdouble(alpha) * np.eye(len(z), dtype=np.longdouble)
    logs = np.longdouble(0)
    for j in range(len(z)):
        a[j:, j] -= a[j:, :j] @ a[j, :j]
        assert a[j, j] > 0
        a[j, j] = np.sqrt(a[j, j])
        a[j + 1:, j] /= a[j, j]
        logs += np.log(a[j, j])
    return 2 * logs / len(z)


def hidden_ratio(got, z, alpha=ALPHA):
    """|device - longdouble| over the bound; <= 1 passes."""
    hi = hidden_ref_hi(z, alpha)
    e_ref = abs(np.longdouble(hidden_ref(z, alpha)) - hi)
    return float(abs(np.longdouble(got) - hi) / (16 * max(e_ref, np.longdouble(2.0) ** -50 * abs(hi))))


def attention_ref(a, start=0, length=None):
    """(per_head [H], total) of one row's (H, T, T) map over the window."""
    a = np.asarray(a, dtype=np.float64)
    length = a.shape[-1] - start if length is None else length
    with np.errstate(divide="ignore"):
        logs = np.log(np.diagonal(a, axis1=-2, axis2=-1)[:, start:start + length])
    per_head = logs.sum(axis=1) / length
    return per_head, per_head.sum(), np.abs(logs).sum()


def causal_maps(rng, batch, heads, t):
    """(B, H, T, T) f32 causal attention: softmax over the keys up to the query."""
    logits = rng.standard_normal((batch, heads, t, t))
    logits[..., np.triu_indices(t, 1)[0], np.triu_indices(t, 1)[1]] = -np.inf
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
