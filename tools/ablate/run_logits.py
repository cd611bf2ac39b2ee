"""Logit scores (csrc/logits.hip) at Llama-3.1-8B shapes (V = 128 256): device time of the kernels and host-clock time of
the whole generation_scores call, against the reference's formulation in the same process, alternated with it:
HF ``compute_transition_scores(normalize_logits=True)`` + ``generation_entropy`` + ``perplexity`` per row +
``normalized_entropy`` (runia_core_amd.llm_uncertainty.scores keeps the reference's host-style torch bodies), with torch
on the same GPU.

- kernel time: device events around the bare C call (three launches, preallocated table, workspace and outputs), over
  T x B x V x element-size algorithmic bytes = fraction of the 8 TB/s HBM peak;
- call time: host clock around generation_scores(...) and a device synchronise (argument checks, the token-range check's
  read-back, the descriptor table upload, the normalized_entropy read-back);
- each shape rotates through enough input sets to exceed the 256 MB Infinity Cache (the T = 32, B = 1 shape: 16 sets of
  16 MB, 262 MB, close to it: labelled).

    python tools/ablate/run_logits.py [--reps 20] [--quick] [--json out.json]
"""
import argparse
import json
import math
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.llm_uncertainty import generation_scores  # noqa: E402
from runia_core_amd.llm_uncertainty import scores as host_scores  # noqa: E402
from runia_core_amd.llm_uncertainty.rauq import _DTYPE_CODES  # noqa: E402

HBM_PEAK = 8.0e12
CACHE = 256 << 20
V = 128256
SHAPES = [(256, 10, torch.float32), (256, 10, torch.bfloat16), (256, 1, torch.float32), (32, 1, torch.float32)]


def hf_transition_scores(sequences, scores):
    """HF GenerationMixin.compute_transition_scores(normalize_logits=True); the method reads only config.vocab_size."""
    from transformers.generation.utils import GenerationMixin

    cfg = types.SimpleNamespace(vocab_size=int(scores[0].shape[-1]))
    cfg.get_text_config = lambda *a, **k: cfg
    return GenerationMixin.compute_transition_scores(types.SimpleNamespace(config=cfg), sequences, scores, normalize_logits=True)


def reference_formulation(seq, scores):
    lp = hf_transition_scores(seq, scores)
    ge = host_scores.generation_entropy(scores)
    ppl = [host_scores.perplexity(lp[b]) for b in range(lp.shape[0])]
    ne = host_scores.normalized_entropy(lp)
    return ge, ppl, ne


def input_sets(T, B, dtype, seed):
    nbytes = T * B * V * torch.finfo(dtype).bits // 8
    n = max(1, min(16, math.ceil(CACHE * 1.5 / nbytes))) if nbytes < CACHE else 1
    g = torch.Generator(device="cuda").manual_seed(seed)
    sets = []
    for _ in range(n):
        scores = tuple((torch.randn(B, V, generator=g, device="cuda") * 4).to(dtype) for _ in range(T))
        seq = torch.randint(0, V, (B, 64 + T), generator=g, device="cuda")
        sets.append((seq, scores))
    return sets, nbytes


def bare_call(lib, seq, scores):
    """The C call alone with everything preallocated: returns a closure launching the three kernels."""
    T, B = len(scores), scores[0].shape[0]
    table = torch.tensor([[s.data_ptr(), s.stride(0)] for s in scores], dtype=torch.int64).cuda()
    tok = seq[:, -T:]
    need = int(lib.runia_logit_stats_workspace_bytes(T, B, V))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    lp = torch.empty(B, T, device="cuda")
    ent = torch.empty(B, T, device="cuda")
    sq = torch.empty(3 * B + 1, dtype=torch.float64, device="cuda")
    code = _DTYPE_CODES[scores[0].dtype]

    def run():
        _hip._check(lib.runia_logit_stats(table.data_ptr(), code, T, B, V, tok.data_ptr(), tok.stride(0), 1, None, lp.data_ptr(),
                                          ent.data_ptr(), sq.data_ptr(), ws.data_ptr(), need, _hip._stream()), "runia_logit_stats")

    run.keep = (table, ws, lp, ent, sq)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the 1.31 GB shape only, 3 repetitions, no reference formulation")
    ap.add_argument("--json", help="also write the result records to this file")
    args = ap.parse_args()
    lib = _hip.load_library()
    _hip.require_gpu()
    shapes = SHAPES[:1] if args.quick else SHAPES
    reps = 3 if args.quick else args.reps
    results = []
    for T, B, dtype in shapes:
        sets, nbytes = input_sets(T, B, dtype, 100 + T + B)
        runs = [bare_call(lib, seq, sc) for seq, sc in sets]
        for r in runs:  # warm-up
            r()
        for seq, sc in sets[:1]:
            generation_scores(seq, sc)
        torch.cuda.synchronize()
        # kernel time: device events around the bare call, rotating the input sets
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for i, (e0, e1) in enumerate(evs):
            e0.record()
            runs[i % len(runs)]()
            e1.record()
        torch.cuda.synchronize()
        kern = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs)
        kern_us = kern[len(kern) // 2]
        # whole call, alternated with the reference formulation
        call, ref = [], []
        ref_reps = 0 if args.quick else max(3, reps // 4)
        if ref_reps:
            reference_formulation(*sets[0])  # warm-up
        torch.cuda.synchronize()
        for i in range(reps):
            seq, sc = sets[i % len(sets)]
            t0 = time.perf_counter()
            generation_scores(seq, sc)
            torch.cuda.synchronize()
            call.append((time.perf_counter() - t0) * 1e6)
            if i < ref_reps:
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                reference_formulation(seq, sc)
                torch.cuda.synchronize()
                ref.append((time.perf_counter() - t0) * 1e6)
                ref_peak = torch.cuda.max_memory_allocated() - base
        call.sort()
        call_us = call[len(call) // 2]
        r = dict(T=T, B=B, V=V, dtype=str(dtype).replace("torch.", ""), input_bytes=nbytes, input_sets=len(sets),
                 cache_resident=len(sets) * nbytes <= CACHE * 1.1, kernel_us=round(kern_us, 1),
                 kernel_hbm_fraction=round(nbytes / (kern_us * 1e-6) / HBM_PEAK, 3), call_us=round(call_us, 1),
                 host_share=round(max(0.0, 1 - kern_us / call_us), 3))
        if ref:
            ref.sort()
            r.update(reference_us=round(ref[len(ref) // 2], 1), reference_peak_extra_bytes=int(ref_peak),
                     speedup=round(ref[len(ref) // 2] / call_us, 1))
        results.append(r)
        print(json.dumps(r), flush=True)
        del sets, runs
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
