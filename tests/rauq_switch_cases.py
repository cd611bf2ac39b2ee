"""Seeded attention maps for the RAUQ tests at the summation-order switch of csrc/rauq.hip (gather_value: torch's cascade
order for rows of k < 512 columns, a wave sum from 512 on), shared by the CPU test of the head margins
(test_rauq_host.py) and the GPU tests (test_rauq_gpu.py, test_rauq_batch_gpu.py).

The maps are causal softmax rows, as a generation's attentions, each head's rows scaled by a gain.  Plain softmax rows all
average to 1/k, so the per-head mode's argmax over the heads' means would be decided in the last bits of the sums and a
test on them would pass or fail on a near-tie.  The gains of a layer's heads are 1, 0.97, 0.94, ... in a seeded order:
the two largest means then differ by about 3 %, well over the 1e-3 the host test asserts and over the bf16 spacing (2^-8)
of the stored means.  With tie=True head 3 is an exact copy of head 1 and both carry the largest gain: the reference's
argmax takes the first of them."""
import numpy as np
import torch

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SWITCH = 512
SWITCH_KS = (510, 511, 512, 513)
GENERATION = dict(input_length=509, n_gen=6)      # k = 509 .. 514: the steps cross the switch
BATCH = dict(input_length=513, n_gen=6, pads=(0, 3, 6), lengths=(6, 6, 5))  # k_b = 513 - pad_b + step
ALPHAS = [0.2, 0.4, 0.9]
L, H = 2, 4
TIE_HEADS = (1, 3)


def _representable(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DTYPES[dtype]).float().numpy()


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def gains(rng, tie):
    g = np.stack([1.0 - 0.03 * rng.permutation(H) for _ in range(L)])  # (L, H)
    if tie:
        for l in range(L):  # the largest gain moves to head 1, and head 3 takes it too
            top = int(np.argmax(g[l]))
            g[l, [TIE_HEADS[0], top]] = g[l, [top, TIE_HEADS[0]]]
            g[l, TIE_HEADS[1]] = g[l, TIE_HEADS[0]]
    return g


def one_row_steps(input_length, n_gen, dtype, seed, tie=False):
    """n_gen steps of (L, H, q, k) f32 values exact in `dtype`: step 0 the (in, in) causal prompt block, step g one query row
    of in + g columns."""
    rng = np.random.default_rng([seed, input_length, n_gen, int(tie)])
    gain = gains(rng, tie)[:, :, None, None]
    steps = []
    for g in range(n_gen):
        if g == 0:
            x = rng.standard_normal((L, H, input_length, input_length)) * 2
            x = np.where(np.triu(np.ones((input_length, input_length), dtype=bool), 1), -np.inf, x)
        else:
            x = rng.standard_normal((L, H, 1, input_length + g)) * 2
        a = _softmax(x) * gain
        if tie:
            a[:, TIE_HEADS[1]] = a[:, TIE_HEADS[0]]
        steps.append(_representable(a, dtype))
    return steps


def log_probs(n, seed, rows=None):
    rng = np.random.default_rng([seed, n, 77])
    return np.log(rng.random((rows or 1, n)) * 0.9 + 0.05).astype(np.float32)


def batch_steps(dtype, seed, tie=False):
    """BATCH's left-padded rows as n_gen steps of (B, L, H, q, k): row b's own maps (one_row_steps at its own prompt length)
    behind pad_b zero key columns (and zero query rows in step 0)."""
    inp, n_gen, pads = BATCH["input_length"], BATCH["n_gen"], BATCH["pads"]
    rows = [one_row_steps(inp - pad, n_gen, dtype, seed + 10 * b, tie) for b, pad in enumerate(pads)]
    steps = []
    for g in range(n_gen):
        q = inp if g == 0 else 1
        s = np.zeros((len(pads), L, H, q, inp + g if g else inp), dtype=np.float32)
        for b, pad in enumerate(pads):
            if g == 0:
                s[b, :, :, pad:, pad:] = rows[b][0]
            else:
                s[b, :, :, :, pad:] = rows[b][g]
        steps.append(s)
    return steps


def one_row_tensors(steps, dtype, device):
    """(L, H, q, k) steps -> generate()'s attentions: per step, per layer, (1, H, q, k)."""
    return tuple(tuple(torch.from_numpy(s[l]).to(device=device, dtype=DTYPES[dtype])[None] for l in range(s.shape[0]))
                 for s in steps)


def batch_tensors(steps, dtype, device):
    """(B, L, H, q, k) steps -> per step, per layer, (B, H, q, k)."""
    return tuple(tuple(torch.from_numpy(np.ascontiguousarray(s[:, l])).to(device=device, dtype=DTYPES[dtype])
                       for l in range(s.shape[1])) for s in steps)


# ---- the gathered row means themselves, bit for bit -------------------------------------------------------------------
MEAN_KS_CASCADE = (70, 127, 128, 255, 256, 300, 509, 510, 511)   # torch's cascade order (k < 512)
MEAN_KS_WAVE = (512, 513, 575, 576, 577, 1024)                   # the wave sum
MEAN_L, MEAN_H = 2, 32


def mean_rows(k, seed=900):
    """(MEAN_L, MEAN_H, 1, k) f32 attention rows (softmax rows times a gain in [0.5, 1]): 64 rows whose f32 sums depend on
    the summation order in their last bits."""
    rng = np.random.default_rng([seed, k])
    a = _softmax(rng.standard_normal((MEAN_L, MEAN_H, 1, k)) * 2) * rng.uniform(0.5, 1.0, (MEAN_L, MEAN_H, 1, 1))
    return a.astype(np.float32)


def wave_order_mean(a):
    """The f32 mean over the last axis in gather_value's order from 512 columns on: lane j of a 64-lane wave adds the
    elements j, j + 64, ... in index order, the lanes are summed by the xor butterfly 32, 16, .., 1, one f32 division."""
    a = np.asarray(a, dtype=np.float32)
    k = a.shape[-1]
    lanes = np.zeros(a.shape[:-1] + (64,), dtype=np.float32)
    for j0 in range(0, k, 64):
        part = a[..., j0:j0 + 64]
        lanes[..., :part.shape[-1]] = lanes[..., :part.shape[-1]] + part
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., np.arange(64) ^ o]
    return (lanes[..., 0] / np.float32(k)).astype(np.float32)


def mean_steps(ks, device):
    """One generation step per k, each layer's map (1, H, 1, k): what runia_rauq_gather reads in "mean_all_tokens"."""
    return tuple(tuple(torch.from_numpy(mean_rows(k)[l])[None].to(device) for l in range(MEAN_L)) for k in ks)
