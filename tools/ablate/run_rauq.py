"""RAUQ at Llama-3.1-8B shape (L = H = 32, bf16, causal maps generated on the device from a seed, n_gen = 256): call time
of the six (head_aggregation, token_aggregation) combinations after warm-up, by device events, and the algorithmic bytes
L H (in^2 + sum_g (in + g)) 2 over the call time as a fraction of the 8 TB/s HBM peak (the rollout routes read every
map; the per-head modes read only query row 0 of each step, so their fraction of the rollout byte count is not a
bandwidth figure and is printed for scale only).  With --host, the host cost the reference's formulation implies on the
same shape: reconstructing the (L, H, T, T) f32 array from the maps and multiplying L dense T x T matrices, with torch on
the host's CPU threads (skipped when the array does not fit in memory).

    python tools/ablate/run_rauq.py [--inputs 1024 2048] [--reps 5] [--host] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from runia_core_amd.llm_uncertainty import RAUQ  # noqa: E402

HBM_PEAK = 8.0e12
COMBOS = [(h, t) for h in ("original", "mean_heads", "rollout") for t in ("original", "mean_all_tokens")]


def causal_maps(L, H, inp, n_gen, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mask = torch.triu(torch.ones(inp, inp, dtype=torch.bool, device="cuda"), 1)
    steps = []
    for s in range(n_gen):
        per = []
        for _ in range(L):
            shape = (1, H, inp, inp) if s == 0 else (1, H, 1, inp + s)
            x = torch.randn(shape, generator=g, device="cuda") * 2
            if s == 0:
                x.masked_fill_(mask, float("-inf"))
            per.append(torch.softmax(x, -1).to(torch.bfloat16))
        steps.append(tuple(per))
    return tuple(steps)


def host_reference_cost(att, inp):
    """The reference's rollout formulation on the host: (L, H, T, T) f32 zeros, maps copied in, mean over heads + I, row
    normalisation, L - 1 dense products.  Seconds, or None when the array would not fit."""
    L, n_gen = len(att[0]), len(att)
    H = att[0][0].shape[1]
    T = inp + n_gen
    need = L * H * T * T * 4
    avail = os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_AVPHYS_PAGES")
    if need * 1.5 > avail:
        return None, need
    t0 = time.perf_counter()
    full = torch.zeros((L, H, T, T))
    for g, step in enumerate(att):
        for l, a in enumerate(step):
            if g == 0:
                full[l, :, :inp, :inp] = a[0].float().cpu()
            else:
                full[l, :, inp + g, : inp + g] = a[0, :, 0].float().cpu()
    eye = torch.eye(T)
    joint = None
    for l in range(L):
        a = full[l].mean(0) + eye
        a = a / a.sum(-1, keepdim=True)
        joint = a if joint is None else a @ joint
    return time.perf_counter() - t0, need


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--n-gen", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json", help="also write the result records to this file")
    args = ap.parse_args()
    L = H = 32
    results = []
    for inp in args.inputs:
        att = causal_maps(L, H, inp, args.n_gen, 1234 + inp)
        lp = torch.log(torch.rand(1, args.n_gen, generator=torch.Generator().manual_seed(5)) * 0.9 + 0.05)
        nbytes = L * H * (inp * inp + sum(inp + g for g in range(1, args.n_gen))) * 2
        for head, tok in COMBOS:
            x = lp if head == "rollout" else lp[0]
            call = lambda: RAUQ(x, att, inp, tok, head, [0.2, 0.4], True)  # noqa: E731
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.reps
            frac = nbytes / (ms * 1e-3) / HBM_PEAK
            r = dict(input_length=inp, n_gen=args.n_gen, head=head, token=tok, call_ms=round(ms, 3),
                     algorithmic_bytes=nbytes, hbm_fraction=round(frac, 3))
            results.append(r)
            print(json.dumps(r), flush=True)
        if args.host:
            s, need = host_reference_cost(att, inp)
            r = dict(input_length=inp, host_reference_rollout_s=None if s is None else round(s, 3), host_array_bytes=need,
                     host_threads=torch.get_num_threads())
            results.append(r)
            print(json.dumps(r), flush=True)
        del att
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
