"""LLM-Check (Sriramanan et al., NeurIPS 2024): the white-box scores of ONE generation from one pass - no sampling.

- ``hidden_score``: the mean log-eigenvalue of the token-by-token covariance of a layer's hidden states over a token window,
  ``(1/T) log det(C C^T + alpha I_T)`` with every token centred over the hidden dimension (the published ``Z^T J Z``);
- ``attention_score``: the sum over heads of the mean log-diagonal of a layer's causal attention map over the window.

Values are returned raw, as published (no sign flip).  Two input forms, f32 / f16 / bf16, on the host or on one GPU:

- forward: ``model(..., output_hidden_states=True).hidden_states`` - a tuple over layers of ``(B, T, d)`` tensors (attentions:
  ``(B, H, T, T)``); the default window of row b is its response ``[input_length, input_length + lengths[b])``;
- ``generate()``: a tuple over steps of tuples over layers - step 0 ``(B, P, d)``, step g ``(B, 1, d)`` (attentions as for
  ``rauq_batch``); the default window is ``[P, P + lengths[b] - 1)``, the states ``generate()`` returned: the last token is
  never fed back.

``windows`` gives every row's ``(start, length)`` explicitly.  A window that reaches into a row's left padding
(``attention_mask``) raises; an empty window scores NaN.  Device tensors are read where they lie through a table of
descriptors, any batch / row strides; host tensors go up in one copy.  All arithmetic is in ``csrc/llm_check.hip`` (DESIGN
4.59): f64 means, the centred Gram matrix on the f64 matrix cores (of the tokens, or of the features where a window is longer
than the states are wide), a blocked Cholesky for the log-determinant - windows of up to 1024 tokens.  Without a GPU a valid
call raises ``RuniaHipError``: there is no host fallback.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _hip
from .rauq import _batch_table, _row_lengths, _row_pads, _upload_parts

__all__ = ["LLMCheckScores", "hidden_score", "attention_score", "llm_check_scores", "LLM_CHECK_MAX_TOKENS"]

LLM_CHECK_MAX_TOKENS = 1024  # the limit of runia_llmcheck_hidden


class LLMCheckScores(NamedTuple):
    """``(B, len(layers))`` f64 device tensors (``attention_score`` is ``(B, len(layers), H)`` with ``per_head=True``)."""

    hidden_score: torch.Tensor
    attention_score: torch.Tensor


def _steps(tensors, layers: Sequence[int], dims: int, what: str):
    """``(steps, forward)``: the chosen layers of every step as lists of tensors, after checking that they agree."""
    if len(tensors) == 0 or len(layers) == 0:
        raise ValueError(f"{what} and layers must not be empty")
    forward = isinstance(tensors[0], torch.Tensor)
    steps = [[tensors[l] for l in layers]] if forward else [[step[l] for l in layers] for step in tensors]
    first = steps[0][0]
    if first.dtype not in _hip.ELEM_DTYPE_CODES:
        raise TypeError(f"{what} must be float32, float16 or bfloat16, not {first.dtype}")
    same = 2 if dims == 3 else 1  # the dimension every step shares besides the batch: d, or the heads
    for g, step in enumerate(steps):
        for t in step:
            if not isinstance(t, torch.Tensor) or t.dim() != dims or t.shape != step[0].shape or min(t.shape) < 1 or \
                    t.shape[0] != first.shape[0] or t.shape[same] != first.shape[same]:
                raise ValueError(f"{what}: step {g} does not hold {dims}-d tensors that fit step 0's {tuple(first.shape)}")
            if t.dtype != first.dtype or t.device != first.device:
                raise ValueError(f"{what} must share one dtype and one device")
    return steps, forward


def _windows(batch: int, prompt: int, n_pos: int, generate: bool, attention_mask, lengths, windows
             ) -> Tuple[torch.Tensor, List[bool], List[int]]:
    """Host int64 ``(B, 2)`` ``{start, length}`` rows, which of them are empty, and every row's left padding."""
    pads = [0] * batch
    if attention_mask is not None:  # (a generate() mask covers the prompt; a forward pass's may be longer)
        pads = _row_pads(attention_mask, batch, prompt if generate else int(torch.as_tensor(attention_mask).shape[-1]))
    if windows is None:
        n = n_pos - prompt + (1 if generate else 0)  # generated tokens: one more than the states generate() returned
        ns = _row_lengths(lengths, batch, n) if n >= 1 else [0] * batch
        rows = [[prompt, v - 1 if generate else v] for v in ns]
    else:
        w = torch.as_tensor(windows).detach().cpu()
        if tuple(w.shape) != (batch, 2) or w.is_floating_point() or w.is_complex():
            raise ValueError(f"windows must be ({batch}, 2) integers, got {tuple(w.shape)}")
        rows = [[int(s), int(t)] for s, t in w.tolist()]
    for b, (s, t) in enumerate(rows):
        if s < 0 or t < 0 or s + t > n_pos:
            raise ValueError(f"row {b}: window [{s}, {s + t}) leaves the {n_pos} positions")
        if t > 0 and s < pads[b]:
            raise ValueError(f"row {b}: window [{s}, {s + t}) reaches into its left padding of {pads[b]}")
    empty = [t == 0 for _, t in rows]
    return torch.tensor([[0, 1] if e else r for r, e in zip(rows, empty)], dtype=torch.int64), empty, pads


def _finish(out: torch.Tensor, empty: List[bool]) -> torch.Tensor:
    if any(empty):
        out[torch.tensor(empty, device=out.device)] = float("nan")
    return out


def _positions(q0: int, n_steps: int, forward: bool, input_length) -> Tuple[int, int]:
    """``(prompt, n_pos)``: where the default window starts and how many positions the steps hold (step 0: ``q0``)."""
    if forward:
        prompt = 0 if input_length is None else int(input_length)
        if not 0 <= prompt <= q0:
            raise ValueError(f"input_length={input_length} does not fit {q0} positions")
        return prompt, q0
    if input_length is not None and int(input_length) != q0:
        raise ValueError(f"step 0 holds {q0} positions, input_length is {input_length}")
    return q0, q0 + n_steps - 1


@_hip._device_guard()
def hidden_score(hidden_states, layers: Sequence[int] = (15,), *, alpha: float = 1e-3, input_length: Optional[int] = None,
                 attention_mask=None, lengths=None, windows=None) -> torch.Tensor:
    """``(B, len(layers))`` f64, on the device: ``(1/T_b) log det(C C^T + alpha I)`` of every row's window at every layer
    of ``layers`` (indices into the layer tuple, HuggingFace's: 0 is the embedding output).  Row b's bits depend on
    row b alone.  NaN for an empty window and for a window with a NaN state."""
    steps, forward = _steps(hidden_states, layers, 3, "hidden_states")
    for g, step in enumerate(steps[1:], 1):
        if any(int(t.shape[1]) != 1 for t in step):
            raise ValueError(f"step {g} of a generate() output holds one position")
    batch, d, n_layers = int(steps[0][0].shape[0]), int(steps[0][0].shape[2]), len(steps[0])
    prompt, n_pos = _positions(int(steps[0][0].shape[1]), len(steps), forward, input_length)
    rows_h, empty, _ = _windows(batch, prompt, n_pos, not forward, attention_mask, lengths, windows)
    t_max = int(rows_h[:, 1].max())
    if t_max > LLM_CHECK_MAX_TOKENS:
        raise ValueError(f"a window of {t_max} tokens: at most {LLM_CHECK_MAX_TOKENS} are supported")
    dev = _hip.require_gpu()
    out = torch.full((batch, n_layers), float("nan"), dtype=torch.float64, device=dev)
    if all(empty):
        return out
    flat = [t for step in steps for t in step]
    if flat[0].is_cuda:
        keep = [t if t.stride(2) == 1 or d == 1 else t.contiguous() for t in flat]
        table = [[t.data_ptr(), t.stride(0), t.stride(1)] for t in keep]
    else:
        keep, addresses = _upload_parts(flat, dev)
        table = [[at, t.shape[1] * d, d] for at, t in zip(addresses, flat)]
    table_d = torch.tensor(table, dtype=torch.int64).to(dev)
    rows_d = rows_h.to(dev)
    ws = _hip.workspace(_hip.query("runia_llmcheck_workspace_bytes", batch * n_layers, t_max), dev)
    _hip.launch("runia_llmcheck_hidden", table_d.data_ptr(), rows_d.data_ptr(), rows_h.data_ptr(),
                _hip.ELEM_DTYPE_CODES[flat[0].dtype], batch, len(steps), n_layers, int(steps[0][0].shape[1]), d, float(alpha),
                out.data_ptr(), ws.data_ptr(), ws.numel())
    del keep
    return _finish(out, empty)


@_hip._device_guard()
def attention_score(attentions, layers: Sequence[int] = (15,), per_head: bool = False, *, input_length: Optional[int] = None,
                    attention_mask=None, lengths=None, windows=None) -> torch.Tensor:
    """``(B, len(layers))`` f64, on the device: ``sum_h (1/T_b) sum_t log A[b, h, t, t]`` over every row's window;
    ``per_head=True`` gives the ``(B, len(layers), H)`` terms.  A zero on the diagonal gives ``-inf``; NaN propagates."""
    steps, forward = _steps(attentions, layers, 4, "attentions")
    block = int(steps[0][0].shape[3])  # positions of step 0
    prompt, n_pos = _positions(block, len(steps), forward, input_length)
    for g, step in enumerate(steps):
        q, k = int(step[0].shape[2]), int(step[0].shape[3])
        if (g == 0 and q not in (1, k)) or (g > 0 and (q != 1 or k != block + g)):
            raise ValueError(f"step {g} map {tuple(step[0].shape)} does not fit a prompt block of {block} positions")
    batch, heads, n_layers = int(steps[0][0].shape[0]), int(steps[0][0].shape[1]), len(steps[0])
    rows_h, empty, pads = _windows(batch, prompt, n_pos, not forward, attention_mask, lengths, windows)
    if int(steps[0][0].shape[2]) < block and any(s < block and not e for (s, _), e in zip(rows_h.tolist(), empty)):
        raise ValueError("step 0 holds one query row: a window over prompt positions needs the whole prompt block")
    dev = _hip.require_gpu()
    out = torch.full((batch, n_layers, heads), float("nan"), dtype=torch.float64, device=dev)
    total = torch.full((batch, n_layers), float("nan"), dtype=torch.float64, device=dev)
    if not all(empty):
        table_d, keep = _batch_table(steps, dev, pads, first_row_only=False)
        rows_d = rows_h.to(dev)
        _hip.launch("runia_llmcheck_attention", table_d.data_ptr(), rows_d.data_ptr(), rows_h.data_ptr(),
                    _hip.ELEM_DTYPE_CODES[steps[0][0].dtype], batch, len(steps), n_layers, heads, block, out.data_ptr(),
                    total.data_ptr())
        del keep
    return _finish(out if per_head else total, empty)


def llm_check_scores(hidden_states, attentions, layers: Sequence[int] = (15,), *, attention_layers: Optional[Sequence[int]] = None,
                     alpha: float = 1e-3, per_head: bool = False, input_length: Optional[int] = None, attention_mask=None,
                     lengths=None, windows=None) -> LLMCheckScores:
    """Both scores of one generation over the same windows (``attention_layers`` defaults to ``layers``)."""
    common = dict(input_length=input_length, attention_mask=attention_mask, lengths=lengths, windows=windows)
    return LLMCheckScores(hidden_score(hidden_states, layers, alpha=alpha, **common),
                          attention_score(attentions, layers if attention_layers is None else attention_layers, per_head,
                                          **common))
