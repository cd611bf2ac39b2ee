"""Batched eigen_score (csrc/eigen_score.hip) against a loop of eigen_score, at Llama width (hidden 4096, bf16 hidden
states as generate() leaves them), for G prompts of k samples each:

- one ``eigen_scores`` call (one launch for all G groups) vs G ``eigen_score`` calls (per group: f32 copy, centred Gram
  launch, Jacobi sweeps with a read-back each, host sort, ``.item()``), host clock with a device synchronise;
- the kernel alone: device events around the bare C call, over the bytes it reads (G k hidden x 2) = fraction of the
  8 TB/s HBM peak;
- ``compute_uncertainties_batch`` end to end on a tiny 16-layer Llama on the GPU, split into the two generate() calls and
  the scoring.

    python tools/ablate/run_eigen_scores.py [--reps 10] [--json out.jsonl]
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from runia_core_amd import _hip  # noqa: E402
from runia_core_amd.llm_uncertainty import compute_uncertainties_batch, eigen_score, eigen_scores  # noqa: E402

HBM_PEAK = 8.0e12
HIDDEN = 4096


def clock(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best.append(time.perf_counter() - t0)
    best.sort()
    return best[len(best) // 2]


def kernel_time(e, G, k, reps):
    lib = _hip.load_library()
    out = torch.empty(G, dtype=torch.float64, device="cuda")
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps + 1):
        s.record()
        _hip._check(lib.runia_eigen_score_batch(e.data_ptr(), 2, G, k, HIDDEN, e.stride(0), 1e-3, out.data_ptr(),
                                                _hip._stream()), "runia_eigen_score_batch")
        t.record()
        t.synchronize()
        times.append(s.elapsed_time(t) * 1e-3)
    times = sorted(times[1:])
    return times[len(times) // 2]


def eigen_rows(reps, lines):
    for k in (5, 10, 32):
        for G in (1, 16, 256):
            g = torch.Generator(device="cuda").manual_seed(G * 100 + k)
            e = torch.randn(G * k, 1, HIDDEN, device="cuda", generator=g).bfloat16()
            hs = ((e,) * 16,)
            batched = clock(lambda: eigen_scores(hs, k), reps)
            groups = [((e[i * k:(i + 1) * k].transpose(0, 1),) * 16,) for i in range(G)]
            loop = clock(lambda: [eigen_score(h) for h in groups], max(1, min(reps, 3 if G > 16 else reps)))
            kt = kernel_time(e[:, 0, :], G, k, reps)
            got = eigen_scores(hs, k).cpu()
            err = max(abs(float(got[i]) - eigen_score(groups[i])) for i in range(min(G, 4)))
            nbytes = G * k * HIDDEN * 2
            row = dict(what="eigen_scores", G=G, k=k, hidden=HIDDEN, dtype="bf16", batched_call_ms=batched * 1e3,
                       loop_eigen_score_ms=loop * 1e3, speedup=loop / batched, kernel_us=kt * 1e6,
                       kernel_hbm_fraction=nbytes / kt / HBM_PEAK, bytes=nbytes, max_abs_diff_first4=err)
            print(json.dumps(row), flush=True)
            lines.append(row)


class TimedModel:
    def __init__(self, model):
        self.model, self.device, self.generation_config = model, model.device, model.generation_config
        self.gen_s = 0.0

    def generate(self, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = self.model.generate(**kw)
        torch.cuda.synchronize()
        self.gen_s += time.perf_counter() - t0
        return out


class IdTok:
    padding_side, pad_token, eos_token = "right", None, "<eos>"

    def __call__(self, text, return_tensors=None, padding=False):
        from transformers import BatchEncoding

        texts = [text] if isinstance(text, str) else list(text)
        ids = [[int(w) for w in t.split()] for t in texts]
        n = max(len(i) for i in ids)
        return BatchEncoding({"input_ids": torch.tensor([[0] * (n - len(i)) + i for i in ids]),
                              "attention_mask": torch.tensor([[0] * (n - len(i)) + [1] * len(i) for i in ids])})

    def batch_decode(self, seqs, skip_special_tokens=True):
        return [" ".join(str(int(t)) for t in row if int(t) > 1) for row in seqs]


def pipeline_rows(reps, lines):
    import transformers
    from transformers import GenerationConfig

    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=16,
                                   num_attention_heads=8, num_key_value_heads=4, max_position_embeddings=512,
                                   attn_implementation="eager", pad_token_id=0, eos_token_id=None, bos_token_id=None)
    model = TimedModel(transformers.LlamaForCausalLM(cfg).cuda().eval())
    reqs = ([{"method_name": m} for m in ("perplexity", "generation_entropy", "normalized_entropy", "eigen_score")] +
            [{"method_name": "RAUQ", "token_aggregation": "mean_all_tokens", "head_aggregation": h, "alphas": [0.3]}
             for h in ("original", "mean_heads", "rollout")])
    gen = GenerationConfig(max_new_tokens=32, pad_token_id=0)
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        prompts = [" ".join(str(int(v)) for v in torch.randint(3, 512, (int(n),), generator=g))
                   for n in torch.randint(16, 48, (B,), generator=g)]
        totals, gens = [], []
        for _ in range(reps + 1):
            model.gen_s = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            compute_uncertainties_batch(model, IdTok(), prompts, reqs, gen, 10)
            torch.cuda.synchronize()
            totals.append(time.perf_counter() - t0)
            gens.append(model.gen_s)
        totals, gens = totals[1:], gens[1:]
        i = sorted(range(reps), key=lambda j: totals[j])[reps // 2]
        row = dict(what="compute_uncertainties_batch", B=B, num_samples=10, max_new_tokens=32, layers=16, hidden=256,
                   total_ms=totals[i] * 1e3, generate_ms=gens[i] * 1e3, scoring_ms=(totals[i] - gens[i]) * 1e3)
        print(json.dumps(row), flush=True)
        lines.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    _hip.require_gpu()
    lines = []
    eigen_rows(a.reps, lines)
    if not a.no_pipeline:
        pipeline_rows(max(2, a.reps // 3), lines)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
