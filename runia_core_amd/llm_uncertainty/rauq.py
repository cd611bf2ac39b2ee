"""RAUQ: recurrent attention-based uncertainty of one LLM generation (Vazhentsev et al. 2025), with the reference's
signatures, defaults and return types (``runia_core/llm_uncertainty/scores.py:155-344``, helpers in
``attention_aggregation.py``).

``attentions`` is HuggingFace ``generate(..., output_attentions=True).attentions``: a tuple of ``n_gen`` steps, each a tuple
of L tensors ``(B, H, q, k)`` - step 0 the prompt block ``(B, H, in, in)`` (or one query row, which the rollout broadcasts
as the reference's tensor assignment does), step g >= 1 ``(B, H, 1, in + g)``.  f32, f16 or bf16, any strides, on the host
or on one GPU: device maps are read in place through a table of descriptors (never copied or written); host maps go to
the device in ONE copy of the rows the mode reads.  All arithmetic is in ``csrc/rauq.hip``:

- per-head (``rauq_uncertainty``) and head-mean (``rauq_uncertainty_mean_heads``) modes: one gather launch of the
  ``(L, H, N)`` token-aggregation values (batch 0), one score launch (head choice, ``exp`` of the log-probs, the
  recurrence, max over layers); ``n_alpha + L`` numbers are read back;
- rollout (``rauq_uncertainty_rollout``): a row pass over every layer's reconstructed ``T x T`` map (T = input_length +
  n_gen) gives the row sums and the diagonal / sub-diagonal of ``A^_l = rownorm(mean_h A_l + I)`` and tells whether the
  prompt block has a non-zero entry above its diagonal.  Causal maps: "original" needs only those bands (one pass over
  the maps, no matrix product); otherwise a 1-row ("mean_all_tokens") or n-row ("original") block is left-multiplied
  through the layers, O(k T^2 L) instead of the reference's O(T^3 L) host products, and ``joint`` is never formed.

The four names live on ``runia_core_amd.llm_uncertainty`` (the reference's package path, whose ``__init__`` star-imports
``scores``), not on ``.scores``.  Without a GPU a valid call raises ``RuniaHipError``: there is no host fallback.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import torch

from .. import _hip

__all__ = ["rauq_uncertainty", "rauq_uncertainty_mean_heads", "rauq_uncertainty_rollout", "RAUQ"]

_DTYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_TOKEN_AGGREGATION = {"original": 0, "mean_all_tokens": 1}
_HEAD_ARGMAX, _HEAD_MEAN, _SERIES = 0, 1, 2


class _UnknownTokenAggregation(KeyError, UnboundLocalError):
    """Unknown ``token_aggregation`` of the rollout: a KeyError like the other modes' dict lookups, and the
    UnboundLocalError the reference's if / elif chain ends in."""


def _map_shapes(attentions) -> Tuple[int, int, int, torch.dtype, Optional[torch.device]]:
    """(n_gen, L, H, dtype, device or None for host maps) after checking that all maps agree."""
    if len(attentions) == 0 or len(attentions[0]) == 0:
        raise ValueError("attentions must hold at least one step of at least one layer")
    n_gen, n_layers = len(attentions), len(attentions[0])
    first = attentions[0][0]
    heads, dtype, dev = int(first.shape[1]), first.dtype, (first.device if first.is_cuda else None)
    if dtype not in _DTYPE_CODES:
        raise TypeError(f"attention maps must be float32, float16 or bfloat16, not {dtype}")
    for g, step in enumerate(attentions):
        if len(step) != n_layers:
            raise ValueError(f"step {g} has {len(step)} layers, step 0 has {n_layers}")
        for t in step:
            if t.dim() != 4 or int(t.shape[1]) != heads or int(t.shape[0]) < 1 or int(t.shape[2]) < 1:
                raise ValueError(f"attention maps must be (B, {heads}, q, k) tensors, got {tuple(t.shape)} at step {g}")
            if t.dtype != dtype or (t.device if t.is_cuda else None) != dev:
                raise ValueError("all attention maps must share one dtype and one device")
    return n_gen, n_layers, heads, dtype, dev


def _map_table(attentions, dev: torch.device, first_row_only: bool):
    """Device int64 table [n_gen * L, 6] of map descriptors (batch 0) and the tensors it points into."""
    flat = [t for step in attentions for t in step]
    if flat[0].is_cuda:
        rows = [[t.data_ptr(), t.stride(1), t.stride(2), t.stride(3), t.shape[3], t.shape[2]] for t in flat]
        keep = flat
    else:
        # host maps: the rows the kernels read, packed into one buffer and uploaded in one copy
        parts = [t[0, :, :1, :] if first_row_only else t[0] for t in flat]
        total = sum(p.numel() for p in parts)
        try:
            host = torch.empty(total, dtype=flat[0].dtype, pin_memory=True)
        except RuntimeError:
            host = torch.empty(total, dtype=flat[0].dtype)
        rows, at = [], 0
        for p in parts:
            h, q, k = p.shape
            host[at:at + p.numel()].view(h, q, k).copy_(p)
            rows.append([at, q * k, k, 1, k, q])
            at += p.numel()
        dmaps = host.to(dev)
        base, size = dmaps.data_ptr(), dmaps.element_size()
        for r in rows:
            r[0] = base + r[0] * size
        keep = dmaps
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    return table, keep


def _probs_source(log_probs: torch.Tensor) -> torch.Tensor:
    """``log_probs.squeeze()`` as a flat f32 tensor (the reference's ``probs = log_probs.exp().squeeze()``)."""
    lp = torch.as_tensor(log_probs).squeeze()
    if lp.dim() > 1:
        raise ValueError(f"log_probs must be one sequence, got shape {tuple(log_probs.shape)}")
    return lp.reshape(-1)


def _score(att: torch.Tensor, n_layers: int, heads: int, n: int, head_mode: int, lp: torch.Tensor, alphas, ws: torch.Tensor):
    """One score launch; reads back ``n_alpha`` scores and (head_mode 0) the L chosen heads in one copy."""
    lib = _hip.load_library()
    dev = att.device
    lp_d = _hip.to_device(lp[:n], torch.float32)
    al = torch.tensor([float(a) for a in alphas], dtype=torch.float64).to(dev)
    out = torch.zeros(len(alphas) + n_layers, dtype=torch.int32, device=dev)
    _hip._check(lib.runia_rauq_score(att.data_ptr(), n_layers, heads, n, head_mode, lp_d.data_ptr(), al.data_ptr(), len(alphas),
                                     out.data_ptr(), out.data_ptr() + 4 * len(alphas), ws.data_ptr(), ws.numel(), _hip._stream()),
                "runia_rauq_score")
    host = out.cpu()
    scores = [float(v) for v in host[: len(alphas)].view(torch.float32).tolist()]
    return scores, host[len(alphas):].tolist()


@_hip._device_guard()
def _gather_scores(log_probs, attentions, token_aggregation: str, alphas, head_mode: int):
    """Scores of the per-head (head_mode 0) or head-mean (1) mode for every alpha, and the heads mode 0 picks."""
    tok = _TOKEN_AGGREGATION[token_aggregation]
    n_gen, n_layers, heads, dtype, _ = _map_shapes(attentions)
    n = n_gen if tok else n_gen - 1
    lp = _probs_source(log_probs)
    if n < 1 or lp.numel() < n:
        raise IndexError(f"{n} aggregated tokens need as many log-probabilities (got {lp.numel()})")
    for g in range(0 if tok else 1, n_gen):
        for t in attentions[g]:
            if int(t.shape[3]) < (1 if tok else 2):
                raise IndexError(f"step {g}: a row of {int(t.shape[3])} keys has no entry -{1 if tok else 2}")
    if len(alphas) == 0:
        return [], []
    lib = _hip.load_library()
    dev = _hip.require_gpu()
    table, keep = _map_table(attentions, dev, first_row_only=True)
    w = torch.empty((n_layers, heads, n), dtype=torch.float32, device=dev)
    _hip._check(lib.runia_rauq_gather(table.data_ptr(), _DTYPE_CODES[dtype], n_gen, n_layers, heads, tok, w.data_ptr(),
                                      _hip._stream()), "runia_rauq_gather")
    ws = torch.empty(int(lib.runia_rauq_workspace_bytes(n_layers, n, 0, 0, 0, len(alphas))), dtype=torch.uint8, device=dev)
    scores, chosen = _score(w, n_layers, heads, n, head_mode, lp, alphas, ws)
    del keep
    return scores, (chosen if head_mode == _HEAD_ARGMAX else None)


@_hip._device_guard()
def _rollout_scores(log_probs, attentions, token_aggregation: str, input_length: int, alphas, info: Optional[dict] = None):
    """Scores of the rollout mode for every alpha; ``info`` (optional dict) receives the route taken."""
    n_gen, n_layers, heads, dtype, _ = _map_shapes(attentions)
    in_len = int(input_length)
    if n_gen < 2:
        raise ValueError("rollout needs at least two generation steps")
    if in_len < 1:
        raise ValueError(f"input_length must be positive, got {input_length}")
    for g, step in enumerate(attentions):
        for t in step:
            b, _, q, k = (int(s) for s in t.shape)
            if b != 1:
                raise ValueError(f"rollout needs batch size 1, got {b}")
            ok = (k == in_len and q in (1, in_len)) if g == 0 else (k == in_len + g and q == 1)
            if not ok:
                raise ValueError(f"step {g} map {(b, heads, q, k)} does not fit input_length={in_len}")
    n = int(log_probs.shape[1])  # the reference's log_probs.shape[1]: 2-D log-probs (IndexError on 1-D, as there)
    if int(log_probs.shape[0]) != 1 or log_probs.dim() != 2:
        raise ValueError(f"rollout log_probs must be (1, n), got {tuple(log_probs.shape)}")
    if token_aggregation not in _TOKEN_AGGREGATION:
        raise _UnknownTokenAggregation(token_aggregation)
    tok = _TOKEN_AGGREGATION[token_aggregation]
    T = in_len + n_gen
    if n < 2 or n > (T if tok else T - 1):
        raise IndexError(f"rollout of T={T} positions cannot score {n} tokens")
    lp = log_probs.reshape(-1)
    if len(alphas) == 0:
        return []
    lib = _hip.load_library()
    dev = _hip.require_gpu()
    code = _DTYPE_CODES[dtype]
    table, keep = _map_table(attentions, dev, first_row_only=False)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def rows(chain_rows):
        ws = torch.empty(int(lib.runia_rauq_workspace_bytes(n_layers, n_gen, in_len, n, chain_rows, len(alphas))),
                         dtype=torch.uint8, device=dev)
        _hip._check(lib.runia_rauq_rollout_rows(table.data_ptr(), code, n_gen, n_layers, heads, in_len, flag.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _hip._stream()), "runia_rauq_rollout_rows")
        return ws

    ws = rows(1 if tok else 0)
    upper = bool(flag.item())
    if tok:
        route, k = (2 if upper else 1), 1
    elif upper:
        route, k = 2, n
        ws = rows(n)  # the n-row chain needs the larger workspace: the row pass runs again into it
    else:
        route, k = 0, 0
    att = torch.empty(n, dtype=torch.float32, device=dev)
    _hip._check(lib.runia_rauq_rollout_att(table.data_ptr(), code, n_gen, n_layers, heads, in_len, tok, route, n, att.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _hip._stream()), "runia_rauq_rollout_att")
    scores, _ = _score(att, 1, 1, n, _SERIES, lp, alphas, ws)
    if info is not None:
        info.update(route="one_pass" if route == 0 else "chain", upper_nonzero=upper, chain_rows=k, T=T)
    del keep
    return scores


def rauq_uncertainty(log_probs: torch.Tensor, attentions: Tuple[Tuple[torch.Tensor, ...], ...], token_aggregation: str,
                     alphas: List[float] = [0.2], ablation: bool = False) -> Union[float, List[float]]:
    """RAUQ with the head of every layer that attends most on average (tokens 1..), per alpha; max over layers."""
    scores, _ = _gather_scores(log_probs, attentions, token_aggregation, alphas, _HEAD_ARGMAX)
    return scores[0] if not ablation else scores


def rauq_uncertainty_mean_heads(log_probs: torch.Tensor, attentions: Tuple[Tuple[torch.Tensor, ...], ...],
                                token_aggregation: str, alphas: List[float] = [0.3],
                                ablation: bool = False) -> Union[float, List[float]]:
    """RAUQ with the attention averaged over the heads of every layer."""
    scores, _ = _gather_scores(log_probs, attentions, token_aggregation, alphas, _HEAD_MEAN)
    return scores[0] if not ablation else scores


def rauq_uncertainty_rollout(log_probs: torch.Tensor, attentions: Tuple[Tuple[torch.Tensor, ...], ...],
                             token_aggregation: str, input_length: int, alphas: List[float] = [0.4],
                             ablation: bool = False) -> Union[float, List[float]]:
    """RAUQ on the attention rollout (Abnar & Zuidema 2020) of the reconstructed maps; ``log_probs`` is ``(1, n)``."""
    scores = _rollout_scores(log_probs, attentions, token_aggregation, input_length, alphas)
    return scores if ablation else scores[0]


def RAUQ(log_probs, attentions, input_length, token_aggregation, head_aggregation, alphas, ablation):
    """Dispatch on ``head_aggregation``: "original", "mean_heads" or "rollout" (KeyError otherwise)."""
    modes = {
        "original": lambda: rauq_uncertainty(log_probs, attentions, token_aggregation, alphas, ablation),
        "mean_heads": lambda: rauq_uncertainty_mean_heads(log_probs, attentions, token_aggregation, alphas, ablation),
        "rollout": lambda: rauq_uncertainty_rollout(log_probs, attentions, token_aggregation, input_length, alphas, ablation),
    }
    return modes[head_aggregation]()
