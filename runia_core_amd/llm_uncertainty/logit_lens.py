"""Logit lens: what an intermediate layer would have predicted - white-box scores of ONE generation, no sampling.

A layer's hidden state is taken through the model's final norm and the unembedding matrix and read as a next-token
distribution.  Per (row, layer, position of the window):

- ``entropy``: how undecided the layer's distribution is (nats);
- ``log_prob``: the layer's log-probability of the token the model went on to emit;
- ``top_log_prob`` / ``top_token``: the layer's own best guess;
- ``kl_final``: ``KL(final layer || this layer)`` at the same position (the DoLa signal);
- ``lse``: the log-sum-exp of the layer's logits.

``hidden_states`` takes the two forms of ``llm_check.hidden_score`` (a forward pass's tuple over layers, or ``generate()``'s
tuple over steps of tuples over layers), f32 / f16 / bf16, on the host or on one GPU; ``weight`` is the ``(V, d)`` unembedding
in the same dtype on the same device (any row stride: tied embeddings and views are read where they lie).  The default window
of row b is the states that PRODUCED its generated tokens: ``[P - 1, P - 1 + n_b)`` in the generate form, ``[input_length -
1, input_length - 1 + lengths[b])`` in the forward form; the target of position p is ``sequences[b, p + 1]``.

The gather of the window rows and the norm are torch plumbing on ``planes x N x d`` values; the product against ``W`` and every
reduction over the vocabulary run in one pass of ``csrc/logit_lens.hip``, which never forms an ``N x V`` table.
An lm_head bias, logit soft-capping and logit scaling are out of scope.  Without a GPU a valid call raises ``RuniaHipError``:
there is no host fallback.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from .. import _hip
from .llm_check import _positions, _steps, _windows
from .rauq import _row_lengths

__all__ = ["LogitLensScores", "logit_lens", "LENS_VOCAB_TILE", "LENS_VOCAB_STEP", "LENS_MAX_SPLIT", "LENS_GROUP_PLANES",
           "LENS_MAX_VOCAB", "lens_split"]

# the tile constants of runia_lens_scores (include/runia_hip.h)
LENS_VOCAB_TILE = _hip._HEADER_MACROS["RUNIA_LENS_VOCAB_TILE"]      # vocabulary ids of one matrix tile
LENS_VOCAB_STEP = _hip._HEADER_MACROS["RUNIA_LENS_VOCAB_STEP"]      # vocabulary ids of one workgroup step
LENS_MAX_SPLIT = _hip._HEADER_MACROS["RUNIA_LENS_MAX_SPLIT"]        # the most chunks the vocabulary is cut into
LENS_GROUP_PLANES = _hip._HEADER_MACROS["RUNIA_LENS_GROUP_PLANES"]  # planes one workgroup scores together
LENS_MAX_VOCAB = _hip._HEADER_MACROS["RUNIA_LENS_MAX_VOCAB"]


def lens_split(vocab: int) -> int:
    """The number of chunks S the kernel cuts a vocabulary of ``vocab`` ids into: a function of ``vocab`` alone."""
    steps = -(-int(vocab) // LENS_VOCAB_STEP)
    per_chunk = -(-steps // LENS_MAX_SPLIT)
    return -(-steps // per_chunk)


class LogitLensScores(NamedTuple):
    """Device tensors.  The first five are ``(B, len(layers), T_max)`` f32, NaN outside a row's window; ``top_token`` is int32,
    -1 outside; the means are ``(B, len(layers))`` f64 over the row's window, NaN for an empty window."""

    lse: torch.Tensor
    entropy: torch.Tensor
    log_prob: torch.Tensor
    top_log_prob: torch.Tensor
    kl_final: torch.Tensor
    top_token: torch.Tensor
    mean_entropy: torch.Tensor
    mean_log_prob: torch.Tensor
    mean_kl_final: torch.Tensor


def _layer_count(hidden_states) -> int:
    if len(hidden_states) == 0:
        raise ValueError("hidden_states and layers must not be empty")
    first = hidden_states[0]
    return len(hidden_states) if isinstance(first, torch.Tensor) else len(first)


@_hip._device_guard()
def logit_lens(hidden_states, weight: torch.Tensor, layers: Sequence[int], *, sequences=None, norm=None,
               final_layer: Optional[int] = -1, input_length: Optional[int] = None, attention_mask=None, lengths=None,
               windows=None) -> LogitLensScores:
    """Score every position of every row's window at every layer of ``layers`` (indices into the layer tuple, HuggingFace's: 0
    is the embedding output).  ``norm``: the model's final norm module, applied to the gathered rows of every plane except the
    one taken from ``final_layer`` (the last hidden state, which HuggingFace returns already normalised); ``final_layer=None``
    gives no KL.  ``sequences``: the ``(B, >= P + n)`` token ids of the generation, for ``log_prob``.  A position's bits
    depend on its own states, the weight and its final partner alone."""
    n_layers = _layer_count(hidden_states)
    layers = [int(l) for l in layers]
    if any(not -n_layers <= l < n_layers for l in layers) or (final_layer is not None and
                                                               not -n_layers <= int(final_layer) < n_layers):
        raise ValueError(f"layers {layers} / final_layer {final_layer} do not index {n_layers} layers")
    wanted = [l % n_layers for l in layers]
    final = None if final_layer is None else int(final_layer) % n_layers
    plane_layers = list(dict.fromkeys(wanted + ([] if final is None else [final])))
    steps, forward = _steps(hidden_states, plane_layers, 3, "hidden_states")
    for g, step in enumerate(steps[1:], 1):
        if any(int(t.shape[1]) != 1 for t in step):
            raise ValueError(f"step {g} of a generate() output holds one position")
    first = steps[0][0]
    batch, d = int(first.shape[0]), int(first.shape[2])
    if not isinstance(weight, torch.Tensor) or weight.dim() != 2:
        raise ValueError("weight must be a (V, d) tensor")
    if weight.dtype != first.dtype:
        raise TypeError(f"hidden_states are {first.dtype}, weight is {weight.dtype}: both operands share one dtype")
    if weight.device != first.device:
        raise ValueError(f"hidden_states lie on {first.device}, weight on {weight.device}")
    vocab = int(weight.shape[0])
    if int(weight.shape[1]) != d or vocab < 1 or vocab > LENS_MAX_VOCAB:
        raise ValueError(f"weight {tuple(weight.shape)} does not fit states of width {d} (1 <= V <= {LENS_MAX_VOCAB})")
    prompt, n_pos = _positions(int(first.shape[1]), len(steps), forward, input_length)

    # the windows: the states that produced the generated tokens, or the caller's
    default = windows is None
    if default:
        n_gen = len(steps) if not forward else n_pos - prompt
        if prompt < 1 or n_gen < 1:
            raise ValueError(f"the default window starts at input_length - 1 and needs a generated token: input_length={prompt}, "
                             f"{n_pos} positions")
        # (a forward pass may hold the state of the last generated token's predecessor as its last position: one more)
        windows = [[prompt - 1, n] for n in ([n_gen] * batch if lengths is None else
                                             _row_lengths(lengths, batch, n_gen + (1 if forward else 0)))]
    rows_h, empty, _ = _windows(batch, prompt, n_pos, not forward, attention_mask, None, windows)
    spans = [(0, 0) if e else (int(s), int(t)) for (s, t), e in zip(rows_h.tolist(), empty)]
    tokens_h = None
    if sequences is not None:
        seq = torch.as_tensor(sequences).detach().cpu()
        if seq.dim() != 2 or int(seq.shape[0]) != batch or seq.is_floating_point() or seq.is_complex():
            raise ValueError(f"sequences must be ({batch}, length) integers, got {tuple(seq.shape)}")
        width = int(seq.shape[1])
        if default and any(s + t + 1 > width for s, t in spans if t):
            raise ValueError(f"sequences of length {width} are too short for the targets of the default window")
        seq = torch.cat([seq.to(torch.int64), torch.full((batch, 1), -1, dtype=torch.int64)], dim=1)
        tokens_h = torch.cat([seq[b, [min(p + 1, width) for p in range(s, s + t)]] for b, (s, t) in enumerate(spans)])
        if bool(((tokens_h < -1) | (tokens_h >= vocab)).any()):
            raise ValueError(f"sequences hold ids outside the {vocab} rows of weight")
    dev = _hip.require_gpu()

    n_rows, t_max, n_out = sum(t for _, t in spans), max(t for _, t in spans), len(wanted)
    nan32 = lambda: torch.full((batch, n_out, t_max), float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    fields = [nan32() for _ in range(5)]
    top = torch.full((batch, n_out, t_max), -1, dtype=torch.int32, device=dev)
    means = [torch.full((batch, n_out), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]
    if n_rows == 0:
        return LogitLensScores(*fields, top, *means)

    # the state table [planes, N, d]: every plane's window rows, the rows of the batch concatenated; norm where it applies
    src = first.device
    b_idx = torch.tensor([b for b, (_, t) in enumerate(spans) for _ in range(t)], dtype=torch.int64, device=src)
    p_idx = torch.tensor([p for s, t in spans for p in range(s, s + t)], dtype=torch.int64, device=src)
    planes = []
    for j, layer in enumerate(plane_layers):
        whole = steps[0][j] if len(steps) == 1 else torch.cat([step[j] for step in steps], dim=1)
        rows = whole[b_idx, p_idx]
        if norm is not None and layer != final:
            rows = norm(rows).detach().to(first.dtype)
        planes.append(rows)
    table = torch.stack(planes).contiguous().to(dev)  # (host inputs: the one copy up)
    weight_d = weight.detach() if weight.is_cuda else weight.detach().to(dev)
    if weight_d.stride(1) != 1 and d > 1:
        weight_d = weight_d.contiguous()
    tokens_d = None if tokens_h is None else tokens_h.to(dev)

    n_planes = len(plane_layers)
    out = torch.empty((5, n_planes, n_rows), dtype=torch.float32, device=dev)
    out_top = torch.empty((n_planes, n_rows), dtype=torch.int32, device=dev)
    ws = _hip.workspace(_hip.query("runia_lens_workspace_bytes", n_planes, n_rows, vocab, d), dev)
    _hip.launch("runia_lens_scores", table.data_ptr(), weight_d.data_ptr(), int(weight_d.stride(0)) if vocab > 1 else d,
                _hip.ELEM_DTYPE_CODES[first.dtype], n_planes, n_rows, vocab, d, _hip._ptr(tokens_d),
                -1 if final is None else plane_layers.index(final), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                out[3].data_ptr(), out_top.data_ptr(), out[4].data_ptr(), ws.data_ptr(), ws.numel())

    # back to (B, layers, T_max); the means row by row from a contiguous (layers, T_b) block: one order whatever the batch
    lp = torch.tensor([plane_layers.index(l) for l in wanted], dtype=torch.int64, device=dev)
    b_d, t_d = b_idx.to(dev), torch.tensor([t for _, n in spans for t in range(n)], dtype=torch.int64, device=dev)
    for k in range(5):
        fields[k][b_d, :, t_d] = out[k][lp].t()
    top[b_d, :, t_d] = out_top[lp].t()
    at = 0
    for b, (_, t) in enumerate(spans):
        if t:
            for mean, k in zip(means, (1, 2, 4)):
                mean[b] = out[k][lp, at:at + t].contiguous().double().sum(dim=1) / t
            at += t
    return LogitLensScores(*fields, top, *means)
