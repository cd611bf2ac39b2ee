"""PaCMAP fit_transform on the device (csrc/pacmap.hip via runia_core_amd.embedding) against a torch-ops restatement on the
same GPU (chunked cdist + topk kNN, index_add_ gradient, the same Adam) and, at N = 10 000, the NumPy restatement on the host.
One JSON line per size to profiles/pacmap_ablate.jsonl (and stdout).

  sizes: N = 10 000 / 50 000 / 200 000 rows at D = 64 and D = 2048 (ten Gaussian clusters), n_neighbors = 10, 450 iterations

Phase times (preprocess, kNN, pairs, optimiser) are wall times between device synchronisations; the per-kernel device times
come from a separate `rocprofv3 --kernel-trace --stats` run of this script.  The host restatement runs
--host-iters iterations and reports the per-iteration time times 450 (marked "extrapolated").

  python tools/ablate/run_pacmap.py [--sizes 10000,50000,200000] [--dims 64,2048] [--no-torch] [--host-iters 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from runia_core_amd import _hip  # noqa: E402
from runia_core_amd import embedding as emb  # noqa: E402

NB, ITERS = 10, 450


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def data(n, d, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    labels = torch.randint(0, 10, (n,), device="cuda", generator=g)
    centres = torch.randn((10, d), device="cuda", generator=g) * 3.0
    return (centres[labels] + torch.randn((n, d), device="cuda", generator=g)).contiguous(), labels


def hip_phases(x):
    """The estimator's fit, phase by phase (same calls as PaCMAP._fit_device)."""
    est = emb.PaCMAP(n_neighbors=NB, random_state=0)
    est._check_params()
    est.seed_ = 0
    n = x.shape[0]
    t0 = sync()
    xp, projected = est._fit_preprocess(x)
    t1 = sync()
    k = min(NB + 50, n - 1)
    idx, dist = _hip.pacmap_knn(xp, xp, k, exclude_self=True)
    t2 = sync()
    nb, mn, fp = _hip.pacmap_pairs(xp, xp, idx, dist, NB, est.n_MN, est.n_FP, 0, False)
    offsets, entries = emb.group_pairs(n, [(nb, 0), (mn, 1), (fp, 2)])
    t3 = sync()
    y = (0.01 * xp[:, :2]).contiguous()  # the optimiser's start (the PCA init of an unprojected fit is not timed here)
    y = emb.optimise(y, None, offsets, entries, ITERS, 1.0)
    t4 = sync()
    return {"preprocess_ms": (t1 - t0) * 1e3, "knn_ms": (t2 - t1) * 1e3, "pairs_ms": (t3 - t2) * 1e3,
            "optimiser_ms": (t4 - t3) * 1e3}, idx


def torch_restatement(xp, nb, mn, fp, chunk=2048):
    """kNN by cdist + topk (chunked rows), then 450 Adam steps with an index_add_ gradient: what a user writes in torch."""
    n = xp.shape[0]
    t0 = sync()
    k = min(NB + 50, n - 1)
    idx = torch.empty((n, k), dtype=torch.int64, device=xp.device)
    for s in range(0, n, chunk):
        d = torch.cdist(xp[s:s + chunk], xp)
        d[torch.arange(d.shape[0], device=d.device), torch.arange(s, s + d.shape[0], device=d.device)] = float("inf")
        idx[s:s + chunk] = torch.topk(d, k, largest=False).indices
    t1 = sync()
    pairs = [(nb.long(), 20.0, 10.0, 1.0), (mn.long(), 2e4, 1e4, 1.0), (fp.long(), -2.0, 1.0, 1.0)]
    y = 0.01 * xp[:, :2].clone()
    m = torch.zeros_like(y)
    v = torch.zeros_like(y)
    for t in range(ITERS):
        w = _hip.pacmap_phase_weights(t)
        g = torch.zeros_like(y)
        for (p, num, c, _), wk in zip(pairs, w):
            dy = y[p[:, 0]] - y[p[:, 1]]
            dd = 1.0 + (dy * dy).sum(1, keepdim=True)
            contrib = (wk * num / (c + dd) ** 2) * dy
            g.index_add_(0, p[:, 0], contrib)
            g.index_add_(0, p[:, 1], -contrib)
        lr_t = np.sqrt(1 - 0.999 ** (t + 1)) / (1 - 0.9 ** (t + 1))
        m += 0.1 * (g - m)
        v += 0.001 * (g * g - v)
        y = y - lr_t * m / (v.sqrt() + 1e-7)
    t2 = sync()
    return {"knn_ms": (t1 - t0) * 1e3, "optimiser_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}, idx


def numpy_restatement(xp, nb, mn, fp, iters):
    """Host kNN (blocked, argpartition) and `iters` Adam steps with bincount gradients."""
    x = xp.astype(np.float32)
    n = x.shape[0]
    k = min(NB + 50, n - 1)
    t0 = time.perf_counter()
    sq = (x * x).sum(1)
    for s in range(0, n, 1024):
        d = sq[s:s + 1024, None] + sq[None, :] - 2.0 * x[s:s + 1024] @ x.T
        d[np.arange(d.shape[0]), np.arange(s, s + d.shape[0])] = np.inf
        np.argpartition(d, k, axis=1)[:, :k]
    t1 = time.perf_counter()
    y = 0.01 * x[:, :2].astype(np.float64)
    m = np.zeros_like(y)
    v = np.zeros_like(y)
    pairs = [(nb, 20.0, 10.0), (mn, 2e4, 1e4), (fp, -2.0, 1.0)]
    for t in range(iters):
        w = _hip.pacmap_phase_weights(t)
        g = np.zeros_like(y)
        for (p, num, c), wk in zip(pairs, w):
            dy = y[p[:, 0]] - y[p[:, 1]]
            contrib = (wk * num / (c + 1.0 + (dy * dy).sum(1, keepdims=True)) ** 2) * dy
            for col in range(2):
                g[:, col] += np.bincount(p[:, 0], contrib[:, col], n) - np.bincount(p[:, 1], contrib[:, col], n)
        lr_t = np.sqrt(1 - 0.999 ** (t + 1)) / (1 - 0.9 ** (t + 1))
        m += 0.1 * (g - m)
        v += 0.001 * (g * g - v)
        y = y - lr_t * m / (np.sqrt(v) + 1e-7)
    t2 = time.perf_counter()
    return {"knn_ms": (t1 - t0) * 1e3, "optimiser_ms_extrapolated": (t2 - t1) / iters * ITERS * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000,200000")
    ap.add_argument("--dims", default="64,2048")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pacmap_ablate.jsonl"))
    args = ap.parse_args()
    _hip.require_gpu()
    warm, _ = data(2000, 64)
    emb.PaCMAP(n_neighbors=NB, random_state=0).fit_transform(warm)
    lines = []
    for d in (int(v) for v in args.dims.split(",")):
        for n in (int(v) for v in args.sizes.split(",")):
            x, _ = data(n, d)
            t0 = sync()
            emb.PaCMAP(n_neighbors=NB, random_state=0).fit_transform(x)
            wall_ms = (sync() - t0) * 1e3
            phases, idx = hip_phases(x)
            rec = {"op": "pacmap_fit_transform", "n": n, "d": d, "n_neighbors": NB, "iters": ITERS, "hip_wall_ms": round(wall_ms, 2),
                   **{f"hip_{k}": round(v, 3) for k, v in phases.items()}}
            est = emb.PaCMAP(n_neighbors=NB, random_state=0)
            est._check_params()
            est.seed_ = 0
            xp, _ = est._fit_preprocess(x)
            nb, mn, fp = _hip.pacmap_pairs(xp, xp, *_hip.pacmap_knn(xp, xp, min(NB + 50, n - 1), True), NB, est.n_MN,
                                           est.n_FP, 0, False)
            if not args.no_torch:
                tr, tidx = torch_restatement(xp, nb, mn, fp)
                rec.update({f"torch_{k}": round(v, 2) for k, v in tr.items()})
                rec["knn_lists_agree"] = float((torch.sort(tidx, 1).values == torch.sort(idx.long(), 1).values).all(1)
                                               .float().mean())
            if n <= 10000:
                hr = numpy_restatement(_hip.to_host(xp), _hip.to_host(nb), _hip.to_host(mn), _hip.to_host(fp), args.host_iters)
                rec.update({f"numpy_{k}": round(v, 1) for k, v in hr.items()})
            rec["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del x, xp, nb, mn, fp
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
