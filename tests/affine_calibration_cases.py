"""Float64 restatement of ``runia_core_amd.evaluation.affine_calibration`` (vector / matrix / Dirichlet calibration): the input
map, the row sums of one evaluation, the per-row outputs and the regularised objective with its gradient.  NumPy only; the
reference has no calibration, so these definitions ARE the oracle.  Inputs come from ``calibration_cases``."""
import numpy as np

from calibration_cases import overconfident_case, seeded_case  # noqa: F401  (the tests take their inputs from here)

LOG_FLT_MIN = float(np.log(np.float64(np.finfo(np.float32).tiny)))  # -87.33654...
KINDS = ("vector", "matrix", "dirichlet")


def log_softmax(z):
    with np.errstate(all="ignore"):
        d = z - z.max(1, keepdims=True)
        return d - np.log(np.exp(d).sum(1, keepdims=True))


def inputs(kind, x):
    """u of the variant: the logits, or their floored log-softmax (a NaN stays)."""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(log_softmax(x), LOG_FLT_MIN) if kind == "dirichlet" else x


def split(kind, theta, c):
    nw = c if kind == "vector" else c * c
    return theta[:nw].reshape((c,) if kind == "vector" else (c, c)), theta[nw:]


def evaluate(kind, x, y, W, b, ignore_index=None):
    """One evaluation in float64 -> dict: n, nll (sum), grad (sum over rows of dW, then db, as one vector), z, and the per-row
    pred, conf, nll_rows, brier, logq of q = softmax(W u + b)."""
    u, y = inputs(kind, x), np.asarray(y)
    W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
    used = np.ones(len(y), bool) if ignore_index is None else y != ignore_index
    yy, r = np.where(used, y, 0), np.arange(len(y))
    z = (u * W if kind == "vector" else u @ W.T) + b
    lq = log_softmax(z)
    q = np.exp(lq)
    res = q.copy()
    res[r, yy] -= 1.0
    res, uu = res[used], u[used]
    dW = (res * uu).sum(0) if kind == "vector" else res.T @ uu
    return {"n": int(used.sum()), "nll": float(-lq[r, yy][used].sum()), "grad": np.concatenate([dW.ravel(), res.sum(0)]), "z": z,
            "pred": np.argmax(z, 1), "conf": q.max(1), "nll_rows": -lq[r, yy], "brier": (q * q).sum(1) - 2.0 * q[r, yy] + 1.0,
            "logq": lq}


def objective(kind, x, y, lam, mu):
    """theta -> (L, dL/dtheta) of the regularised objective in float64 (the input map is applied once)."""
    x = np.asarray(x, dtype=np.float64)
    c = x.shape[1]
    u = inputs(kind, x)

    def fun(theta):
        W, b = split(kind, theta, c)
        e = evaluate("vector" if kind == "vector" else "matrix", u, y, W, b)
        value, grad = e["nll"] / e["n"] + mu / c * b.dot(b), e["grad"] / e["n"]
        grad[W.size:] += 2.0 * mu / c * b
        if kind != "vector" and c > 1:
            off = W - np.diag(np.diag(W))
            value += lam / (c * (c - 1)) * (off * off).sum()
            grad[:W.size] += (2.0 * lam / (c * (c - 1)) * off).ravel()
        return float(value), grad

    return fun
