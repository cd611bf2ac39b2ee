"""Batched RAUQ at Llama-3.1-8B shape (L = H = 32, bf16 causal maps of B left-padded rows generated on the device from a
seed, in = 512, n_gen = 128, pads spread over [0, 240), lengths over [n_gen / 2, n_gen]): end-to-end time of one
``rauq_batch`` call against B one-row ``RAUQ`` calls on sliced maps (the slicing included, as a caller pays it), for the
six (head_aggregation, token_aggregation) combinations, by device events after warm-up.  The rollout rows also report the
algorithmic bytes of the row pass, sum_b L H (in_b^2 + sum_{g < n_b} (in_b + g)) 2, over the batched call time as a
fraction of the 8 TB/s HBM peak (a kernel trace gives the row kernel's own time).

    python tools/ablate/run_rauq_batch.py [--batches 1 4 8] [--reps 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from runia_core_amd.llm_uncertainty import RAUQ, rauq_batch  # noqa: E402

HBM_PEAK = 8.0e12
COMBOS = [(h, t) for h in ("original", "mean_heads", "rollout") for t in ("original", "mean_all_tokens")]


def padded_causal_maps(L, H, inp, n_gen, pads, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    B = len(pads)
    padk = torch.arange(inp + n_gen, device="cuda")[None, :] < torch.tensor(pads, device="cuda")[:, None]
    causal = torch.triu(torch.ones(inp, inp, dtype=torch.bool, device="cuda"), 1)
    steps = []
    for s in range(n_gen):
        per = []
        for _ in range(L):
            if s == 0:
                x = torch.randn(B, H, inp, inp, generator=g, device="cuda") * 2
                x.masked_fill_(causal[None, None] | padk[:, None, None, :inp], float("-inf"))
            else:
                x = torch.randn(B, H, 1, inp + s, generator=g, device="cuda") * 2
                x.masked_fill_(padk[:, None, None, :inp + s], float("-inf"))
            per.append(torch.softmax(x, -1).nan_to_num_(0.0).to(torch.bfloat16))
            del x
        steps.append(tuple(per))
    return tuple(steps)


def one_row_calls(lp, att, inp, pads, lengths, tok, head, alphas):
    for b, pad in enumerate(pads):
        n = lengths[b]
        maps = tuple(tuple((t[b:b + 1, :, pad:, pad:] if g == 0 else t[b:b + 1, :, :, pad:]) for t in att[g]) for g in range(n))
        x = lp[b:b + 1, :n] if head == "rollout" else lp[b, :n]
        RAUQ(x, maps, inp - pad, tok, head, alphas, True)


def timed(call, reps):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--input", type=int, default=512)
    ap.add_argument("--n-gen", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", help="also write the result records to this file")
    args = ap.parse_args()
    L = H = 32
    inp, n_gen, alphas = args.input, args.n_gen, [0.2, 0.4]
    results = []
    for B in args.batches:
        pads = [(37 * b) % 240 if b else 0 for b in range(B)]
        lengths = [n_gen - (n_gen // 2 * b) // max(B - 1, 1) if B > 1 else n_gen for b in range(B)]
        att = padded_causal_maps(L, H, inp, n_gen, pads, 4321 + B)
        lp = torch.log(torch.rand(B, n_gen, generator=torch.Generator().manual_seed(5)) * 0.9 + 0.05)
        mask = (torch.arange(inp)[None, :] >= torch.tensor(pads)[:, None]).to(torch.int64)
        n_t = torch.tensor(lengths)
        nbytes = sum(L * H * ((inp - p) ** 2 + sum(inp - p + g for g in range(1, n))) * 2 for p, n in zip(pads, lengths))
        for head, tok in COMBOS:
            batched = timed(lambda: rauq_batch(lp, att, inp, tok, head, alphas, mask, n_t), args.reps)
            rows = timed(lambda: one_row_calls(lp, att, inp, pads, lengths, tok, head, alphas), args.reps)
            r = dict(B=B, input_length=inp, n_gen=n_gen, pads=pads, lengths=lengths, head=head, token=tok,
                     batch_ms=round(batched, 3), one_row_calls_ms=round(rows, 3), speedup=round(rows / batched, 2))
            if head == "rollout":
                r.update(algorithmic_bytes=nbytes, hbm_fraction_batch_call=round(nbytes / (batched * 1e-3) / HBM_PEAK, 3))
            results.append(r)
            print(json.dumps(r), flush=True)
        del att
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
