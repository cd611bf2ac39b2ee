"""MaxLogit / KL-Matching / fDBD / Relative Mahalanobis: ``postprocess_device`` of every postprocessor of
``inference/extended_postprocessors.py`` against the plain PyTorch composition of the same formula on the same device tensors.

  mls    ``logits.max(1)``
  klm    ``softmax`` -> ``matmul`` with ``log_q.T`` -> masked ``max`` -> minus ``sum p log p``; and a third route, the materialised
         form inside the package: ``softmax`` table, ``_hip.linear`` (N x K products written), ``max``
  fdbd   ``feats @ w.T + b`` -> ``argmax`` -> ``gather`` of the table rows -> sum / ((C - 1) ||feats - mu||)
  rmds   the two Mahalanobis terms as ``cdist``-free quadratic forms per class in f64 (N x 2048 features are not built here:
         D = 128, the classes of the shape capped at 64)

for N x C in {262 144 x 1000, 1 M x 10, 65 536 x 4096} (features: D = 128).  Every route is timed with a device event pair
around the whole route after a warm-up, ``--reps`` repetitions alternated in one process; median and min in ms.  One JSON
line per (case, method).  The routes' results are compared (max abs difference) before they are timed.

  python tools/ablate/run_logit_baselines.py [--reps N] [--out profiles/logit_baselines_ablate.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.inference import FDBD, KLMatching, MaxLogit, RelativeMahalanobis, fdbd_inverse_distances  # noqa: E402

SHAPES = [(262144, 1000), (1 << 20, 10), (65536, 4096)]
FEATURE_DIM = 128


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def neg_entropy_torch(logits):
    lp = torch.log_softmax(logits, 1)
    p = lp.exp()
    return torch.where(p > 0, p * lp, torch.zeros((), device=logits.device)).sum(1)


def klm_torch(logits, log_q, valid):
    cross = torch.softmax(logits, 1) @ log_q.T
    cross = cross.masked_fill(valid.unsqueeze(0) == 0, float("-inf"))
    return cross.max(1).values - neg_entropy_torch(logits)


def klm_materialised(logits, log_q, valid, stats):
    p = torch.exp(logits - stats.lse.unsqueeze(1))
    cross = _hip.linear(p, log_q, None).masked_fill(valid.unsqueeze(0) == 0, float("-inf"))
    return cross.max(1).values - stats.neg_entropy


def fdbd_torch(feats, w, b, mu, inv):
    logits = feats @ w.T + b
    top, pred = logits.max(1)
    terms = (top.unsqueeze(1) - logits).abs() * inv[pred]   # the gathered N x C rows of the table
    return terms.sum(1) / ((logits.shape[1] - 1) * torch.linalg.norm(feats - mu, dim=1))


def maha_torch(x, means, prec):
    x = x.double()
    best = None
    for mu in means:
        z = x - mu
        d = -((z @ prec) * z).sum(1)
        best = d if best is None else torch.maximum(best, d)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.require_gpu()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []
    for n, c in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(7)
        d = FEATURE_DIM
        feats = torch.randn((n, d), device="cuda", generator=gen)
        w = torch.randn((c, d), device="cuda", generator=gen) / d ** 0.5
        b = torch.randn((c,), device="cuda", generator=gen) * 0.1
        logits = _hip.linear(feats, w, b)
        log_q = torch.log_softmax(torch.randn((c, c), device="cuda", generator=gen) * 2.0, 1)
        valid = torch.ones((c,), dtype=torch.int32, device="cuda")
        valid[c // 2] = 0

        mls = MaxLogit(False)
        klm = KLMatching(False, c)
        klm.log_q, klm.valid = _hip.to_host(log_q), _hip.to_host(valid)
        fd = FDBD(False)
        fd.w, fd.b = _hip.to_host(w), _hip.to_host(b)
        fd.train_mean = _hip.to_host(feats[:4096].mean(0))
        fd.inv_dist = fdbd_inverse_distances(fd.w)
        inv, mu = torch.from_numpy(fd.inv_dist).cuda(), torch.from_numpy(fd.train_mean).cuda()
        k = min(c, 64)
        rm = RelativeMahalanobis(False, k)
        g = np.random.default_rng(3)
        rm.class_mean = g.standard_normal((k, d)).astype(np.float32)
        rm.background_mean = g.standard_normal((1, d)).astype(np.float32)
        m1, m2 = g.standard_normal((d, d)), g.standard_normal((d, d))
        rm.precision, rm.background_precision = m1 @ m1.T / d + np.eye(d), m2 @ m2.T / d + np.eye(d)
        cm, bm = torch.from_numpy(rm.class_mean).cuda().double(), torch.from_numpy(rm.background_mean).cuda().double()
        cp, bp = torch.from_numpy(rm.precision).cuda(), torch.from_numpy(rm.background_precision).cuda()

        routes = {
            "mls": {"hip": lambda: mls.postprocess_device(logits), "torch": lambda: logits.max(1).values},
            "klm": {"hip": lambda: klm.postprocess_device(logits), "torch": lambda: klm_torch(logits, log_q, valid),
                    "materialised": lambda: klm_materialised(logits, log_q, valid,
                                                             _hip.logit_row_stats(logits, False, True, True, False))},
            "fdbd": {"hip": lambda: fd.postprocess_device(feats), "torch": lambda: fdbd_torch(feats, w, b, mu, inv)},
            "rmds": {"hip": lambda: rm.postprocess_device(feats),
                     "torch": lambda: maha_torch(feats, cm, cp) - maha_torch(feats, bm, bp)},
        }
        for method, fns in routes.items():
            results = {name: fn().double() for name, fn in fns.items()}   # (also the warm-up of every route)
            torch.cuda.synchronize()
            diff = {name: float((r - results["hip"]).abs().max()) for name, r in results.items() if name != "hip"}
            del results
            times = {name: [] for name in fns}
            for _ in range(a.reps):
                for name, fn in fns.items():
                    times[name].append(timed(fn, start, stop))
            line = {"case": f"{n}x{c}", "method": method, "N": n, "C": c, "D": d, "reps": a.reps,
                    "max_abs_diff_vs_hip": diff, "device": torch.cuda.get_device_name(0)}
            for name, ts in times.items():
                line[f"{name}_ms_median"], line[f"{name}_ms_min"] = float(np.median(ts)), float(np.min(ts))
            if method == "rmds":
                line["classes"] = k
            print(json.dumps(line), flush=True)
            lines.append(line)
        del feats, logits, log_q, inv
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
