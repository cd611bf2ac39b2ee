"""Sample-consistency kernels (csrc/consistency.hip) against two baselines the harness carries itself, on ids drawn from a
32 000-word vocabulary under a Zipf law (so that matches occur), G prompts of K samples of T tokens:

- ``pairwise_counts`` (ROUGE-L tables alone, and with the Jaccard tables) and ``graph_scores``: host clock around the public
  call with a device synchronise, and device events around the call for the kernels alone;
- the same row recurrence as a torch composition on the device: all G K (K - 1) / 2 pairs side by side, per step one
  ``where`` and one ``cummax`` over a (pairs, T) tensor;
- a host NumPy run of the same recurrence (K = 10, T = 256 only);
- ``torch.linalg.eigh`` of the batched Laplacians, for the graph step.

The tables of the kernel and of the torch composition are compared for equality before anything is timed.

    python tools/ablate/run_consistency.py [--reps 5] [--json profiles/consistency_ablate.jsonl]   (the default)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.llm_uncertainty import graph_scores, pairwise_counts, pairwise_similarity  # noqa: E402

VOCAB = 32000
SHAPES = ((64, 10, 256), (64, 20, 1024))


def zipf_ids(g, k, t, seed):
    rng = np.random.default_rng(seed)
    return (2 + (rng.zipf(1.2, size=(g * k, t)) - 1) % (VOCAB - 2)).astype(np.int64)


def clock(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2]


def event_clock(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps + 1):
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e-3)
    return sorted(times[1:])[len(times[1:]) // 2]


def pair_index(k):
    i, j = np.triu_indices(k, 1)
    return i, j


def torch_lcs(ids, k):
    """(G, K, K) int32 LCS table by the kernel's recurrence, every pair a row of one (pairs, T) tensor."""
    n, t = ids.shape
    g = n // k
    i, j = pair_index(k)
    base = (torch.arange(g, device=ids.device) * k)[:, None]
    a = ids[(base + torch.as_tensor(i, device=ids.device)[None]).reshape(-1)].to(torch.int32)
    b = ids[(base + torch.as_tensor(j, device=ids.device)[None]).reshape(-1)].to(torch.int32)
    row = torch.zeros_like(b)
    zero = torch.zeros((b.shape[0], 1), dtype=torch.int32, device=ids.device)
    for s in range(t):
        left = torch.cat([zero, row[:, :-1]], dim=1)
        row = torch.cummax(torch.where(b == a[:, s:s + 1], left + 1, row), dim=1).values
    out = torch.zeros((g, k, k), dtype=torch.int32, device=ids.device)
    out[:, i, j] = row[:, -1].view(g, -1)
    out = out + out.transpose(1, 2)
    out.diagonal(dim1=1, dim2=2).fill_(t)
    return out


def numpy_lcs(ids, k):
    n, t = ids.shape
    g = n // k
    i, j = pair_index(k)
    base = (np.arange(g) * k)[:, None]
    a, b = ids[(base + i[None]).reshape(-1)], ids[(base + j[None]).reshape(-1)]
    row = np.zeros_like(b)
    for s in range(t):
        left = np.concatenate([np.zeros((b.shape[0], 1), dtype=b.dtype), row[:, :-1]], axis=1)
        row = np.maximum.accumulate(np.where(b == a[:, s:s + 1], left + 1, row), axis=1)
    return row[:, -1].reshape(g, -1)


def torch_graph(w):
    d = w.sum(dim=2)
    lap = torch.eye(w.shape[1], dtype=w.dtype, device=w.device) - w / torch.sqrt(d[:, :, None] * d[:, None, :])
    lam, vec = torch.linalg.eigh(lap)
    return lam, vec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                                                   "profiles", "consistency_ablate.jsonl"))
    a = ap.parse_args()
    _hip.require_gpu()
    lines = []
    for g, k, t in SHAPES:
        host = zipf_ids(g, k, t, seed=g + k + t)
        ids = torch.from_numpy(host).cuda()
        got = pairwise_counts(ids, k, jaccard=False)
        want = torch_lcs(ids, k)
        assert torch.equal(got.lcs, want), "the kernel and the torch composition disagree"
        pairs = g * k * (k - 1) // 2
        lcs_call = clock(lambda: pairwise_counts(ids, k, jaccard=False), a.reps)
        lcs_dev = event_clock(lambda: _hip.cons_pairs(ids, k, None, None, lcs=True, jaccard=False), a.reps)
        both_call = clock(lambda: pairwise_counts(ids, k), a.reps)
        both_dev = event_clock(lambda: _hip.cons_pairs(ids, k, None, None, lcs=True, jaccard=True), a.reps)
        torch_s = clock(lambda: torch_lcs(ids, k), max(1, min(a.reps, 3)))
        row = dict(what="pairwise_counts", G=g, K=k, T=t, vocab=VOCAB, pairs=pairs, dp_cells=pairs * t * t,
                   lcs_call_ms=lcs_call * 1e3, lcs_kernels_ms=lcs_dev * 1e3, lcs_jaccard_call_ms=both_call * 1e3,
                   lcs_jaccard_kernels_ms=both_dev * 1e3, torch_composition_ms=torch_s * 1e3,
                   torch_over_kernel=torch_s / lcs_call, dp_cells_per_s=pairs * t * t / lcs_dev,
                   mean_lcs=float(got.lcs.double().mean()))
        if (k, t) == (10, 256):
            t0 = time.perf_counter()
            ref = numpy_lcs(host, k)
            row["numpy_host_ms"] = (time.perf_counter() - t0) * 1e3
            row["numpy_over_kernel"] = row["numpy_host_ms"] / row["lcs_call_ms"]
            i, j = pair_index(k)
            assert np.array_equal(got.lcs.cpu().numpy()[:, i, j], ref)
        print(json.dumps(row), flush=True)
        lines.append(row)

        w = pairwise_similarity(ids, k)
        graph_call = clock(lambda: graph_scores(w), a.reps)
        graph_dev = event_clock(lambda: _hip.cons_graph(w, 0.9, 0.5), a.reps)
        eigh_s = clock(lambda: torch_graph(w), a.reps)
        lam = torch_graph(w)[0]
        err = float((graph_scores(w).eigenvalues - lam).abs().max())
        row = dict(what="graph_scores", G=g, K=k, call_ms=graph_call * 1e3, kernel_ms=graph_dev * 1e3,
                   torch_laplacian_eigh_ms=eigh_s * 1e3, torch_over_kernel=eigh_s / graph_call, max_abs_eigenvalue_diff=err)
        print(json.dumps(row), flush=True)
        lines.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
