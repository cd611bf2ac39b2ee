"""Scores of LLM generations from their logits, on the device, in one pass (``csrc/logits.hip``).

``scores`` is HuggingFace ``generate(..., output_scores=True).scores``: a tuple of T steps, each ``(B, V)`` or
``(B, 1, V)``, f32, f16 or bf16, on the host or on one GPU.  The reference scores a generation with host-style torch:
``model.compute_transition_scores(sequences, scores, normalize_logits=True)`` stacks every step and runs a full
``log_softmax`` over the stack (two copies of all the logits, reference ``llm_uncertainty/scores.py:452-456, 495-499``),
``generation_entropy`` copies a softmax per step to the host for batch row 0 only (``scores.py:135-152``,
``utils.py:83-99``), and ``perplexity`` / ``normalized_entropy`` loop over the result.  Here the steps are read in place
through a device table of descriptors (pointer, row stride): nothing is stacked, and a step is made contiguous only when
its vocabulary axis is not unit-stride.  Host scores go to the device in one pinned copy and the results come back.

- ``transition_scores``: HF ``compute_transition_scores`` without beams, ``(B, T)`` f32;
- ``token_entropies``: the per-token terms of ``generation_entropy`` for every row, ``(B, T)`` f32;
- ``generation_scores``: both, and the sequence scores, from one pass (``GenerationScores``).

Without a GPU a valid call raises ``RuniaHipError``: there is no host fallback.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _hip

__all__ = ["GenerationScores", "generation_scores", "token_entropies", "transition_scores"]


class GenerationScores(NamedTuple):
    """Scores of every row of one ``generate()`` output (B rows, T steps).

    log_probs           (B, T) f32: HF's normalised transition scores (``-inf`` where the token's logit is ``-inf``)
    token_entropy       (B, T) f32: ``-sum p log p / log V`` per step
    generation_entropy  (B,) f64: mean of ``token_entropy`` over the steps (reference ``generation_entropy`` of row b)
    perplexity          (B,) f64: ``-mean(log_probs[b])`` (reference ``perplexity``)
    normalized_entropy  float: reference ``normalized_entropy(log_probs)`` over all B rows (``-inf`` entries are padding)
    """

    log_probs: torch.Tensor
    token_entropy: torch.Tensor
    generation_entropy: torch.Tensor
    perplexity: torch.Tensor
    normalized_entropy: float


def _steps(scores) -> Tuple[List[torch.Tensor], int, int, torch.dtype, Optional[torch.device]]:
    """The steps as (B, V) views, B, V, dtype and device (None: host), after checking that they agree."""
    if isinstance(scores, torch.Tensor) or len(scores) == 0:
        raise ValueError("scores must be a non-empty sequence of (B, V) or (B, 1, V) tensors, one per generation step")
    rows = []
    for t, s in enumerate(scores):
        if not isinstance(s, torch.Tensor):
            raise ValueError(f"step {t} is not a tensor")
        if s.dtype not in _hip.ELEM_DTYPE_CODES:
            raise TypeError(f"scores must be float32, float16 or bfloat16, not {s.dtype} (step {t})")
        if s.dim() == 3 and s.shape[1] == 1:
            s = s[:, 0, :]
        if s.dim() != 2 or s.shape[0] < 1 or s.shape[1] < 1:
            raise ValueError(f"step {t} has shape {tuple(scores[t].shape)}; expected (B, V) or (B, 1, V)")
        rows.append(s)
    first = rows[0]
    dev = first.device if first.is_cuda else None
    for t, s in enumerate(rows):
        if s.shape != first.shape:
            raise ValueError(f"step {t} is {tuple(s.shape)}, step 0 is {tuple(first.shape)}")
        if s.dtype != first.dtype or (s.device if s.is_cuda else None) != dev:
            raise ValueError("all steps must share one dtype and one device")
    return rows, int(first.shape[0]), int(first.shape[1]), first.dtype, dev


def _token_ids(sequences, B: int, T: int, V: int) -> torch.Tensor:
    """The generated tokens ``sequences[:, -T:]`` (as HF's ``cut_idx``), checked: B rows, at least T columns, ids in [0, V)."""
    seq = torch.as_tensor(sequences)
    if seq.dim() != 2:
        raise ValueError(f"sequences must be (B, length), got shape {tuple(seq.shape)}")
    if int(seq.shape[0]) != B:
        raise ValueError(f"sequences has {int(seq.shape[0])} rows, the scores have {B}")
    if int(seq.shape[1]) < T:
        raise ValueError(f"sequences has {int(seq.shape[1])} columns, fewer than the {T} generation steps")
    if seq.dtype.is_floating_point or seq.dtype.is_complex or seq.dtype == torch.bool:
        raise ValueError(f"sequences must hold integer token ids, not {seq.dtype}")
    tok = seq[:, seq.shape[1] - T:]
    lo, hi = (int(v) for v in torch.stack(torch.aminmax(tok)).tolist())  # one reduction, one read-back
    if lo < 0 or hi >= V:
        raise ValueError(f"token ids must lie in [0, {V}), got ids in [{lo}, {hi}]")
    return tok


def _table(rows: Sequence[torch.Tensor], dev: torch.device):
    """Device int64 table [T, 2] of {row 0 pointer, row stride} and the tensors it points into (kept alive by the caller)."""
    if rows[0].is_cuda:
        # read in place; only a step whose vocabulary axis is not unit-stride is made contiguous
        keep = [r if r.stride(1) == 1 else r.contiguous() for r in rows]
        desc = [[r.data_ptr(), r.stride(0)] for r in keep]
    else:
        # host steps: one pinned buffer (T, B, V), one upload
        T, (B, V) = len(rows), rows[0].shape
        try:
            host = torch.empty((T, B, V), dtype=rows[0].dtype, pin_memory=True)
        except RuntimeError:
            host = torch.empty((T, B, V), dtype=rows[0].dtype)
        for t, r in enumerate(rows):
            host[t].copy_(r)
        keep = host.to(dev, non_blocking=True)
        base, step = keep.data_ptr(), B * V * keep.element_size()
        desc = [[base + t * step, V] for t in range(T)]
    table = torch.tensor(desc, dtype=torch.int64).to(dev)
    return table, keep


@_hip._device_guard()
def _run(sequences, scores, normalize: bool, want_log_prob: bool, want_entropy: bool, want_seq: bool):
    rows, B, V, dtype, host_dev = _steps(scores)
    T = len(rows)
    tok = _token_ids(sequences, B, T, V) if want_log_prob else None
    dev = _hip.require_gpu()
    need = _hip.query("runia_logit_stats_workspace_bytes", T, B, V)
    if need == 0:
        raise ValueError(f"{T} steps of ({B}, {V}) logits exceed the kernel's size limits")
    table, keep = _table(rows, dev)
    if tok is not None:
        tok = tok.to(device=dev, dtype=torch.int64)
        if tok.stride(1) != 1:
            tok = tok.contiguous()
    ws = _hip.workspace(need, dev, 0)
    lp = torch.empty((B, T), dtype=torch.float32, device=dev) if want_log_prob else None
    ent = torch.empty((B, T), dtype=torch.float32, device=dev) if want_entropy else None
    seq = torch.empty(3 * B + 1, dtype=torch.float64, device=dev) if want_seq else None
    _hip.launch("runia_logit_stats", table.data_ptr(), _hip.ELEM_DTYPE_CODES[dtype], T, B, V, _hip._ptr(tok),
                tok.stride(0) if tok is not None else 0, int(bool(normalize)), None, _hip._ptr(lp), _hip._ptr(ent),
                _hip._ptr(seq), ws.data_ptr(), need)
    del keep
    if host_dev is None:
        lp = lp.cpu() if lp is not None else None
        ent = ent.cpu() if ent is not None else None
        seq = seq.cpu() if seq is not None else None
    return lp, ent, seq, B


def transition_scores(sequences: torch.Tensor, scores: Tuple[torch.Tensor, ...], beam_indices: Optional[torch.Tensor] = None,
                      normalize_logits: bool = False) -> torch.Tensor:
    """HF ``model.compute_transition_scores(sequences, scores, beam_indices, normalize_logits)`` without beams: the
    ``(B, T)`` f32 score of every generated token, ``log_softmax(x)[tok]`` when ``normalize_logits`` else ``x[tok]``.
    V is the scores' width (no model argument)."""
    if beam_indices is not None:
        raise NotImplementedError("transition_scores does not take beam_indices (beam search)")
    lp, _, _, _ = _run(sequences, scores, normalize_logits, True, False, False)
    return lp


def token_entropies(scores: Tuple[torch.Tensor, ...]) -> torch.Tensor:
    """``(B, T)`` f32 normalised entropy ``-sum p log p / log V`` of every step's softmax, for every row: the per-token terms
    the reference's ``generation_entropy`` averages for row 0."""
    _, ent, _, _ = _run(None, scores, True, False, True, False)
    return ent


def generation_scores(sequences: torch.Tensor, scores: Tuple[torch.Tensor, ...]) -> GenerationScores:
    """Log-probs, token entropies and the sequence scores of every row from one pass over the logits (see
    ``GenerationScores``).  ``log_probs`` can go straight into ``RAUQ``."""
    lp, ent, seq, B = _run(sequences, scores, True, True, True, True)
    return GenerationScores(lp, ent, seq[:B], seq[B:2 * B], float(seq[3 * B]))
