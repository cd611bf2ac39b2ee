"""Vector / matrix / Dirichlet calibration on the device (csrc/affine_calibration.hip, evaluation/affine_calibration.py) against
the float64 restatement of tests/affine_calibration_cases.py.  Bound of the sums and the per-row floats, as in
test_calibration_gpu.py: err(device, f64) <= 4 err(torch f32 on the CPU, f64) + 2e-6, the torch error measured here and
printed; the record's errors are relative to the largest magnitude of their block (nll sum, dW, db), the per-row ones by
``rel_err``.  ``pred`` is exact wherever the float64 maximum leads by more than f32 rounding of z (1e-5 max(1, |z|)); a row
inside that margin must still name a class that attains the maximum within it."""
import pickle

import numpy as np
import pytest
import torch

import affine_calibration_cases as cases
from calibration_cases import metrics_f64
from conftest import rel_err

pytestmark = pytest.mark.gpu

FULL_C = (1, 2, 3, 31, 32, 33, 100, 255, 256)
WIDE_C = (257, 1000, 4096)
SHAPES = [(k, c) for k in cases.KINDS for c in FULL_C] + [("vector", c) for c in WIDE_C]
IGNORE = -100


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def parameters(kind, c, seed):
    g = np.random.default_rng(seed)
    W = (np.ones(c) if kind == "vector" else np.eye(c)) + 0.3 * g.standard_normal((c,) if kind == "vector" else (c, c))
    return W.astype(np.float32), (0.3 * g.standard_normal(c)).astype(np.float32)


def device_case(kind, n, c, dtype, strided, seed):
    """-> device logits (a row-strided view if asked), device labels, the widened host logits, host labels"""
    x, y = cases.seeded_case(n, c, seed)
    if kind == "dirichlet" and c > 1:
        x[::3, seed % c] = -np.inf     # a class the model rules out: the floor
    if n >= 5:
        y[::5] = IGNORE
    xd = dev(x).to(dtype)
    if strided:
        wide = torch.zeros((n, c + 3), dtype=dtype, device="cuda")
        wide[:, :c] = xd
        xd = wide[:, :c]
    return xd, dev(y), host(xd.to(torch.float32)), y


def torch_f32(kind, x, y, W, b):
    """The evaluation as a plain torch float32 composition on the CPU (the keys of cases.evaluate that are compared)."""
    t, W, b = torch.from_numpy(np.asarray(x, dtype=np.float32)), torch.from_numpy(W), torch.from_numpy(b)
    used = torch.from_numpy(np.asarray(y) != IGNORE)
    yy, r = torch.from_numpy(np.where(np.asarray(y) != IGNORE, y, 0)), torch.arange(len(y))
    u = torch.clamp(torch.log_softmax(t, 1), min=cases.LOG_FLT_MIN) if kind == "dirichlet" else t
    lq = torch.log_softmax((u * W if kind == "vector" else u @ W.T) + b, 1)
    q = lq.exp()
    res = q.clone()
    res[r, yy] -= 1.0
    res, uu = res[used], u[used]
    dW = (res * uu).sum(0) if kind == "vector" else res.T @ uu
    out = {"nll": -lq[r, yy][used].sum(), "grad": torch.cat([dW.ravel(), res.sum(0)]), "conf": q.max(1).values,
           "nll_rows": -lq[r, yy], "brier": (q * q).sum(1) - 2 * q[r, yy] + 1, "logq": lq}
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def block_err(got, ref):
    scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    return float(np.max(np.abs(got - ref))) / (scale if scale > 0 else 1.0) if ref.size else 0.0


def check_eval(kind, xd, yd, x, y, W, b, what):
    from runia_core_amd import _hip as hip

    c, nw, used = x.shape[1], W.size, y != IGNORE
    got = hip.affine_calibration_eval(xd, yd, kind, dev(W), dev(b), IGNORE,
                                      want=("record", "pred", "conf", "nll", "brier", "logq"))
    want, ref32 = cases.evaluate(kind, x, y, W, b, IGNORE), torch_f32(kind, x, y, W, b)
    rec = host(got.record)
    assert rec.dtype == np.float64 and rec.shape == (2 + nw + c,) and rec[0] == want["n"]
    pairs = [("sum nll", block_err(rec[1:2], np.array([want["nll"]])), block_err(ref32["nll"].reshape(1), np.array([want["nll"]]))),
             ("dW", block_err(rec[2:2 + nw], want["grad"][:nw]), block_err(ref32["grad"][:nw], want["grad"][:nw])),
             ("db", block_err(rec[2 + nw:], want["grad"][nw:]), block_err(ref32["grad"][nw:], want["grad"][nw:]))]
    for k, field in (("conf", "conf"), ("nll_rows", "nll"), ("brier", "brier")):
        pairs.append((k, rel_err(host(getattr(got.rows, field))[used], want[k][used]), rel_err(ref32[k][used], want[k][used])))
        assert np.isnan(host(getattr(got.rows, field))[~used]).all()
    pairs.append(("logq", rel_err(host(got.logq), want["logq"]), rel_err(ref32["logq"], want["logq"])))
    for k, e_dev, e_torch in pairs:
        print(f"{what} {k}: device {e_dev:.2e} torch-f32 {e_torch:.2e}")
        assert e_dev <= 4 * e_torch + 2e-6, (k, e_dev, e_torch)
    pred, z = host(got.rows.pred), want["z"]
    top = z.max(1)
    margin = 1e-5 * np.maximum(1.0, np.abs(z).max(1))
    lead = top - np.partition(z, -2, 1)[:, -2] if c > 1 else np.full(len(y), np.inf)
    assert got.rows.pred.dtype == torch.int32 and np.array_equal(pred[lead > margin], want["pred"][lead > margin])
    assert (top - z[np.arange(len(y)), pred] <= margin).all()
    return got


@pytest.mark.parametrize("kind,c", SHAPES)
def test_objective_and_gradient_against_f64(kind, c):
    from runia_core_amd import _hip as hip

    W, b = parameters(kind, c, 7 * c)
    over = hip.query("runia_affcal_round_rows", c, hip.AFFCAL_KINDS[kind]) + 1   # a second tile for the first workgroup
    for n, dtype, strided in ((1, torch.float32, False), (33, torch.float16, True), (33, torch.bfloat16, False),
                              (over, torch.float32, True)):
        xd, yd, x, y = device_case(kind, n, c, dtype, strided, 1000 * c + n)
        check_eval(kind, xd, yd, x, y, W, b, f"{kind} n={n} c={c} {dtype}")


@pytest.mark.parametrize("kind,c", [("vector", 33), ("vector", 1000), ("matrix", 33), ("dirichlet", 100), ("dirichlet", 256)])
def test_same_bits_run_to_run_and_16_bit_as_widened_f32(kind, c):
    from runia_core_amd import _hip as hip

    W, b = parameters(kind, c, c)
    want = ("record", "pred", "conf", "nll", "brier", "logq")
    xd, yd, _, _ = device_case(kind, 700, c, torch.bfloat16, False, c)
    runs = [hip.affine_calibration_eval(t, yd, kind, dev(W), dev(b), IGNORE, want=want) for t in (xd, xd, xd.to(torch.float32))]
    for other in runs[1:]:
        assert torch.equal(other.record.view(torch.int64), runs[0].record.view(torch.int64))
        assert torch.equal(other.logq.view(torch.int32), runs[0].logq.view(torch.int32))
        assert all(host(p).tobytes() == host(q).tobytes() for p, q in zip(other.rows[:4], runs[0].rows[:4]))
    empty = hip.affine_calibration_eval(xd[:0], yd[:0], kind, dev(W), dev(b), IGNORE)
    assert not host(empty.record).any()


def torch_objective(kind, x, y, lam, mu):
    """The objective of the fit with its row sums formed by torch in float32 on the CPU."""
    from runia_core_amd.evaluation.affine_calibration import regulariser

    def fun(theta):
        W, b = cases.split(kind, theta, x.shape[1])
        e = torch_f32(kind, x, y, W.astype(np.float32), b.astype(np.float32))
        reg, dW, db = regulariser(kind, W, b, lam, mu)
        return e["nll"] / len(y) + reg, e["grad"] / len(y) + np.concatenate([dW.ravel(), db])
    return fun


@pytest.fixture(scope="module")
def fit_data():
    out = {}
    for n, c in ((2000, 10), (3000, 33)):
        x, y = cases.overconfident_case(n, c, 40 + c)
        out[c] = ((x + 2.0 * np.random.default_rng(c).standard_normal(c).astype(np.float32)).astype(np.float32), y)
    return out


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("c", [10, 33])
def test_fit_against_the_f64_optimum(fit_data, kind, c):
    from runia_core_amd.evaluation import calibration_metrics, fit_affine_calibration, fit_temperature
    from runia_core_amd.evaluation.affine_calibration import identity_parameters, lbfgs_minimize

    x, y = fit_data[c]
    lam = mu = 1e-3
    f64 = cases.objective(kind, x, y, lam, mu)
    start = identity_parameters(kind, c)
    best = lbfgs_minimize(f64, start, 5000, 1e-10)[1]
    cal = fit_affine_calibration(x, y, kind=kind, lam=lam, mu=mu)
    theta = np.concatenate([cal.W.ravel(), cal.b]).astype(np.float64)
    gap_dev = f64(theta)[0] - best
    gap_torch = f64(lbfgs_minimize(torch_objective(kind, x, y, lam, mu), start, 200, 1e-6)[0])[0] - best
    print(f"fit {kind} {x.shape}: L {cal.loss:.9f} f64 optimum {best:.9f} gap device {gap_dev:.2e} torch-f32 {gap_torch:.2e} "
          f"iterations {cal.n_iter}")
    assert gap_dev <= 4 * gap_torch + 1e-7
    at_t = start.copy()
    at_t[:start.size - c] /= fit_temperature(x, y)
    assert f64(theta)[0] < f64(start)[0] and f64(theta)[0] < f64(at_t)[0]
    assert abs(cal.loss - f64(theta)[0]) <= 2e-6 * max(1.0, abs(cal.loss))
    # metrics of the fitted map against the f64 z of its parameters
    got, want = cal.metrics(x, y, n_bins=15), metrics_f64(cases.evaluate(kind, x, y, cal.W, cal.b)["z"], y, 1.0, 15)
    assert got.n == want["n"] and got.accuracy == want["accuracy"]
    assert abs(got.nll - want["nll"]) <= 2e-6 * max(1, want["nll"]) and abs(got.brier - want["brier"]) <= 2e-6
    assert abs(got.ece - want["ece"]) <= 2e-6 + 4.0 / got.n and got.bins.count.sum() == got.n
    assert got.nll < calibration_metrics(x, y).nll
    back = pickle.loads(pickle.dumps(cal))
    assert back.kind == kind and np.array_equal(back.W, cal.W) and np.array_equal(back.b, cal.b) and back.loss == cal.loss
    assert [np.asarray(v).tobytes() for v in back.metrics(x, y)[:6]] == [np.asarray(v).tobytes() for v in got[:6]]
    p = cal.probabilities_device(x[:50])
    assert p.is_cuda and p.shape == (50, c) and torch.allclose(p.sum(1), torch.ones(50, device="cuda"), atol=1e-5)
    assert torch.equal(p, cal.log_probabilities_device(dev(x[:50])).exp())


@pytest.mark.parametrize("kind,c,w_shape,error", [("matrix", 257, None, "256"), ("dirichlet", 257, None, "256"),
                                                  ("vector", 4097, None, "4096"), ("matrix", 8, (8,), "shape"),
                                                  ("vector", 8, (8, 8), "shape"), ("diagonal", 8, None, "kind")])
def test_refusals_come_before_any_launch(kind, c, w_shape, error):
    from runia_core_amd import _hip as hip
    from runia_core_amd.evaluation import fit_affine_calibration

    x, y = torch.zeros((4, c), device="cuda"), torch.zeros((4,), dtype=torch.int64, device="cuda")
    W = torch.zeros(w_shape or ((c,) if kind == "vector" else (c, c)), device="cuda")
    with pytest.raises(ValueError, match=error):
        hip.affine_calibration_eval(x, y, kind, W, torch.zeros((c,), device="cuda"))
    if w_shape is None:
        with pytest.raises(ValueError, match=error):
            fit_affine_calibration(x, y, kind=kind)
