"""Vector / Dirichlet calibration: one objective evaluation and a whole fit of csrc/affine_calibration.hip against what a
user did before it.

  (a) new          ``_hip.affine_calibration_eval`` (record only) on the logits where they lie; ``ms_eval_new`` is the launch
                   sequence alone (device events, no read-back); ``ms_fit_new`` the public ``fit_affine_calibration`` (host
                   L-BFGS, one upload + evaluation + read-back per objective call), with its objective calls counted
  (b) composition  the same objective as torch on the device: ``log_softmax`` (dirichlet), a ``Linear`` (or ``w * x + b``),
                   ``log_softmax``, the NLL of the labels and autograd for the gradient; ``ms_eval_torch`` is one forward +
                   backward, ``ms_fit_torch`` the same L-BFGS loop (``lbfgs_minimize``) around it with a read-back per call

Sizes: 10 000 x 100 and 50 000 x 150 for dirichlet, 50 000 x 1000 for vector; f32 logits, lam = mu = 1e-3.  Every route is
timed with a device event pair after a warm-up, over ``--reps`` repetitions alternated inside one process; the input sets are
rotated and together exceed the 256 MB last-level cache.  Median and min are reported.  ``floor_ms`` = bytes of logits / 8 TB/s.

  python tools/ablate/run_affine_calibration.py [--reps N] [--out profiles/affine_calibration_ablate.jsonl]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.evaluation.affine_calibration import (fit_affine_calibration, identity_parameters, lbfgs_minimize,  # noqa: E402
                                                          regulariser)

HBM_BYTES_PER_S = 8.0e12
LLC_BYTES = 256 << 20
SHAPES = [("dirichlet", 10000, 100), ("dirichlet", 50000, 150), ("vector", 50000, 1000)]
LAM = MU = 1e-3


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def torch_eval(kind, x, y, W, b):
    """sum nll and its gradients by autograd, on the device"""
    W = W.detach().requires_grad_(True)
    b = b.detach().requires_grad_(True)
    u = torch.clamp(torch.log_softmax(x, 1), min=-87.33654475) if kind == "dirichlet" else x
    z = u * W + b if kind == "vector" else torch.nn.functional.linear(u, W, b)
    nll = torch.nn.functional.cross_entropy(z, y, reduction="sum")
    nll.backward()
    return nll.detach(), W.grad, b.grad


def torch_fit(kind, x, y, max_iter=200, tol=1e-6):
    n, c = x.shape
    calls = [0]

    def fun(theta):
        calls[0] += 1
        nw = c if kind == "vector" else c * c
        Wh, bh = theta[:nw].reshape((c,) if kind == "vector" else (c, c)), theta[nw:]
        nll, gW, gb = torch_eval(kind, x, y, torch.from_numpy(Wh.astype(np.float32)).cuda(), torch.from_numpy(bh.astype(np.float32)).cuda())
        grad = torch.cat([gW.ravel(), gb]).double().cpu().numpy() / n
        reg, dW, db = regulariser(kind, Wh, bh, LAM, MU)
        return float(nll) / n + reg, grad + np.concatenate([dW.ravel(), db])

    _, loss, it = lbfgs_minimize(fun, identity_parameters(kind, c), max_iter, tol)
    return loss, it, calls[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 3
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []
    for kind, n, c in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(7)
        one = n * c * 4
        n_sets = max(2, -(-LLC_BYTES // one) + 1)
        xs, ys = [], []
        for _ in range(n_sets):
            x = torch.randn((n, c), device="cuda", generator=gen) * 3.0 + torch.randn((c,), device="cuda", generator=gen)
            y = torch.where(torch.rand((n,), device="cuda", generator=gen) < 0.3,
                            torch.randint(0, c, (n,), device="cuda", generator=gen), x.argmax(1))
            xs.append(x)
            ys.append(y)
        W = (torch.ones(c, device="cuda") if kind == "vector" else torch.eye(c, device="cuda")) + 0.1 * torch.randn(
            (c,) if kind == "vector" else (c, c), device="cuda", generator=gen)
        b = 0.1 * torch.randn((c,), device="cuda", generator=gen)

        def new(k):
            return _hip.affine_calibration_eval(xs[k], ys[k], kind, W, b, want=("record",)).record

        def old(k):
            return torch_eval(kind, xs[k], ys[k], W, b)

        rec, ref = new(0).cpu().numpy(), old(0)
        ref_grad = torch.cat([ref[1].ravel(), ref[2]]).double().cpu().numpy()
        diff = float(np.max(np.abs(rec[2:] - ref_grad)) / np.max(np.abs(ref_grad)))
        for k in range(n_sets):
            new(k)
            old(k)
        t_new, t_old = [], []
        for r in range(a.reps):
            k = r % n_sets
            t_new.append(timed(lambda: new(k), start, stop))
            t_old.append(timed(lambda: old(k), start, stop))
        fit_new, fit_old = [], []
        for r in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cal = fit_affine_calibration(xs[0], ys[0], kind=kind, lam=LAM, mu=MU)
            t1 = time.perf_counter()
            loss_t, it_t, calls_t = torch_fit(kind, xs[0], ys[0])
            t2 = time.perf_counter()
            fit_new.append((t1 - t0) * 1e3)
            fit_old.append((t2 - t1) * 1e3)
        ms_new, ms_old = float(np.median(t_new)), float(np.median(t_old))
        floor = one / HBM_BYTES_PER_S * 1e3
        line = {"kind": kind, "shape": f"{n}x{c} f32", "ms_eval_new": round(ms_new, 4), "ms_eval_new_min": round(min(t_new), 4),
                "ms_eval_torch": round(ms_old, 4), "ms_eval_torch_min": round(min(t_old), 4),
                "torch_over_new_eval": round(ms_old / ms_new, 2), "floor_ms": round(floor, 4), "new_over_floor": round(ms_new / floor, 2),
                "ms_fit_new": round(float(np.median(fit_new)), 1), "fit_iterations_new": cal.n_iter, "fit_loss_new": cal.loss,
                "ms_fit_torch": round(float(np.median(fit_old)), 1), "fit_iterations_torch": it_t, "fit_calls_torch": calls_t,
                "fit_loss_torch": loss_t, "torch_over_new_fit": round(float(np.median(fit_old) / np.median(fit_new)), 2),
                "reps": a.reps, "input_sets": n_sets, "rel_diff_gradient_between_routes": diff,
                "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del xs, ys
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
