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

``rauq_batch`` scores every row of a batched, left-padded generation in one walk over the maps: row b is scored as the
one-row functions score its own slices (its left padding stripped, its steps after ``lengths[b]`` cut), and the
kernels take all rows at once.  ``generated_lengths`` gives those lengths from a sampled generation's eos tokens.

The four one-row names and the two batched ones live on ``runia_core_amd.llm_uncertainty`` (the reference's package path, whose ``__init__`` star-imports
``scores``), not on ``.scores``.  Without a GPU a valid call raises ``RuniaHipError``: there is no host fallback.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import torch

from .. import _hip

__all__ = ["rauq_uncertainty", "rauq_uncertainty_mean_heads", "rauq_uncertainty_rollout", "RAUQ", "rauq_batch",
           "generated_lengths"]

_DTYPE_CODES = _hip.ELEM_DTYPE_CODES  # the name tests and tools read

_TOKEN_AGGREGATION = {"original": 0, "mean_all_tokens": 1}
_HEAD_ARGMAX, _HEAD_MEAN, _SERIES = 0, 1, 2
_HEAD_AGGREGATION = {"original": _HEAD_ARGMAX, "mean_heads": _HEAD_MEAN, "rollout": _SERIES}


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
    if dtype not in _hip.ELEM_DTYPE_CODES:
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


def _upload_parts(parts, dev: torch.device):
    """Host tensors packed into one (pinned, if it can be had) buffer and uploaded in ONE copy -> the device buffer and every
    part's address in it."""
    total = sum(p.numel() for p in parts)
    try:
        host = torch.empty(total, dtype=parts[0].dtype, pin_memory=True)
    except RuntimeError:
        host = torch.empty(total, dtype=parts[0].dtype)
    at = 0
    for p in parts:
        host[at:at + p.numel()].view(p.shape).copy_(p)
        at += p.numel()
    dmaps = host.to(dev)
    size, addresses, at = dmaps.element_size(), [], dmaps.data_ptr()
    for p in parts:
        addresses.append(at)
        at += p.numel() * size
    return dmaps, addresses


def _map_table(attentions, dev: torch.device, first_row_only: bool):
    """Device int64 table [n_gen * L, 6] of map descriptors (batch 0) and the tensors it points into."""
    flat = [t for step in attentions for t in step]
    if flat[0].is_cuda:
        rows = [[t.data_ptr(), t.stride(1), t.stride(2), t.stride(3), t.shape[3], t.shape[2]] for t in flat]
        keep = flat
    else:
        # host maps: the rows the kernels read, packed into one buffer and uploaded in one copy
        parts = [t[0, :, :1, :] if first_row_only else t[0] for t in flat]
        keep, addresses = _upload_parts(parts, dev)
        rows = [[at, q * k, k, 1, k, q] for at, (_, q, k) in zip(addresses, (p.shape for p in parts))]
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
    dev = att.device
    lp_d = _hip.to_device(lp[:n], torch.float32)
    al = torch.tensor([float(a) for a in alphas], dtype=torch.float64).to(dev)
    out = torch.zeros(len(alphas) + n_layers, dtype=torch.int32, device=dev)
    _hip.launch("runia_rauq_score", att.data_ptr(), n_layers, heads, n, head_mode, lp_d.data_ptr(), al.data_ptr(), len(alphas),
                out.data_ptr(), out.data_ptr() + 4 * len(alphas), ws.data_ptr(), ws.numel())
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
    dev = _hip.require_gpu()
    table, keep = _map_table(attentions, dev, first_row_only=True)
    w = torch.empty((n_layers, heads, n), dtype=torch.float32, device=dev)
    _hip.launch("runia_rauq_gather", table.data_ptr(), _hip.ELEM_DTYPE_CODES[dtype], n_gen, n_layers, heads, tok, w.data_ptr())
    ws = _hip.workspace(_hip.query("runia_rauq_workspace_bytes", n_layers, n, 0, 0, 0, len(alphas)), dev, 0)
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
    dev = _hip.require_gpu()
    code = _hip.ELEM_DTYPE_CODES[dtype]
    table, keep = _map_table(attentions, dev, first_row_only=False)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def rows(chain_rows):
        ws = _hip.workspace(_hip.query("runia_rauq_workspace_bytes", n_layers, n_gen, in_len, n, chain_rows, len(alphas)), dev, 0)
        _hip.launch("runia_rauq_rollout_rows", table.data_ptr(), code, n_gen, n_layers, heads, in_len, flag.data_ptr(),
                    ws.data_ptr(), ws.numel())
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
    _hip.launch("runia_rauq_rollout_att", table.data_ptr(), code, n_gen, n_layers, heads, in_len, tok, route, n, att.data_ptr(),
                ws.data_ptr(), ws.numel())
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


# ---- batched ---------------------------------------------------------------------------------------------------------------
def generated_lengths(sequences: torch.Tensor, input_length: int, eos_token_id: Union[int, List[int]]) -> torch.Tensor:
    """(B,) int64: per row, the generated tokens up to and including the first eos in ``sequences[:, input_length:]``, or
    all of them when the row has none (the ``lengths`` of ``rauq_batch`` for a sampled generation)."""
    gen = torch.as_tensor(sequences)[:, int(input_length):]
    ids = torch.as_tensor([eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id), device=gen.device)
    hit = torch.isin(gen, ids.to(gen.dtype))
    first = hit.to(torch.int8).argmax(dim=1).to(torch.int64) + 1
    full = torch.full_like(first, int(gen.shape[1]))
    return torch.where(hit.any(dim=1), first, full)


def _batch_table(attentions, dev: torch.device, pads: List[int], first_row_only: bool):
    """Device int64 table [n_gen * L, 7] of batched descriptors (batch 0 and the batch stride) and what it points into.
    Host maps go up in one copy of the rows the mode reads: query row 0 of every row's own view, or everything."""
    flat = [t for step in attentions for t in step]
    if flat[0].is_cuda:
        rows = [[t.data_ptr(), t.stride(0), t.stride(1), t.stride(2), t.stride(3), t.shape[3], t.shape[2]] for t in flat]
        return torch.tensor(rows, dtype=torch.int64).to(dev), flat
    parts = flat
    if first_row_only:
        # step 0: query row pad_b of row b, stored as one query row (which the kernels do not slice by rows again)
        parts = [torch.stack([t[b, :, p:p + 1, :] for b, p in enumerate(pads)]) if t.shape[2] > 1 else t
                 for t in attentions[0]] + [t[:, :, :1, :] for t in flat[len(attentions[0]):]]
    dmaps, addresses = _upload_parts(parts, dev)
    rows = [[at, h * q * k, q * k, k, 1, k, q] for at, (_, h, q, k) in zip(addresses, (p.shape for p in parts))]
    return torch.tensor(rows, dtype=torch.int64).to(dev), dmaps


def _row_pads(attention_mask, batch: int, in_len: int) -> List[int]:
    """Leading zeros of every mask row; ValueError unless the mask is left padding with a non-empty prompt per row."""
    if attention_mask is None:
        return [0] * batch
    m = torch.as_tensor(attention_mask).detach().cpu()
    if m.dim() != 2 or tuple(m.shape) != (batch, in_len):
        raise ValueError(f"attention_mask must be ({batch}, {in_len}), got {tuple(m.shape)}")
    on = m != 0
    if not bool(on.any(dim=1).all()):
        raise ValueError("attention_mask has a row of zeros: every row needs at least one prompt token")
    pads = on.to(torch.int8).argmax(dim=1)
    if not bool((on == (torch.arange(in_len)[None, :] >= pads[:, None])).all()):
        raise ValueError("attention_mask is not left padding: a zero follows a one")
    return [int(p) for p in pads]


def _row_lengths(lengths, batch: int, n_gen: int) -> List[int]:
    if lengths is None:
        return [n_gen] * batch
    n = torch.as_tensor(lengths).detach().cpu().reshape(-1)
    if n.numel() != batch or n.is_floating_point() or n.is_complex():
        raise ValueError(f"lengths must hold {batch} integers, got {tuple(torch.as_tensor(lengths).shape)}")
    out = [int(v) for v in n.tolist()]
    if any(v < 1 or v > n_gen for v in out):
        raise ValueError(f"lengths must lie in [1, {n_gen}], got {out}")
    return out


@_hip._device_guard()
def rauq_batch(log_probs: torch.Tensor, attentions: Tuple[Tuple[torch.Tensor, ...], ...], input_length: int,
               token_aggregation: str, head_aggregation: str, alphas: List[float], attention_mask=None,
               lengths=None) -> torch.Tensor:
    """RAUQ of every row of a batched, left-padded generation: ``(B, len(alphas))`` f32, on the maps' GPU (on the host for
    host maps).  Row b is bit for bit ``RAUQ(<its log-probs>, <its maps>, in_b, token_aggregation, head_aggregation,
    alphas, True)`` on its own slices: pad_b = the leading zeros of ``attention_mask[b]`` (0 without a mask), in_b =
    input_length - pad_b, n_b = ``lengths[b]`` (default: every step); step 0 ``[b:b+1, :, pad_b:, pad_b:]``, step 1 <= g <
    n_b ``[b:b+1, :, :, pad_b:]``, log-probs ``log_probs[b, :n_b]``.  A row whose one-row call raises (n_b < 2 for
    "original" token aggregation or the rollout) is NaN.  The maps are walked once for all rows."""
    head_mode = _HEAD_AGGREGATION[head_aggregation]
    tok = _TOKEN_AGGREGATION[token_aggregation]
    n_gen, n_layers, heads, dtype, map_dev = _map_shapes(attentions)
    in_len = int(input_length)
    batch = int(attentions[0][0].shape[0])
    if in_len < 1:
        raise ValueError(f"input_length must be positive, got {input_length}")
    for g, step in enumerate(attentions):
        for t in step:
            b, _, q, k = (int(v) for v in t.shape)
            if b != batch:
                raise ValueError(f"every map must have batch size {batch}, got {b} at step {g}")
            ok = (k == in_len and q in (1, in_len)) if g == 0 else (k == in_len + g and q == 1)
            if not ok:
                raise ValueError(f"step {g} map {tuple(t.shape)} does not fit input_length={in_len}")
    pads = _row_pads(attention_mask, batch, in_len)
    if int(attentions[0][0].shape[2]) == 1 and any(pads):
        raise ValueError("step 0 holds one query row: padded rows need the whole prompt block")
    ns = _row_lengths(lengths, batch, n_gen)
    lp = torch.as_tensor(log_probs)
    if lp.dim() != 2 or int(lp.shape[0]) != batch or int(lp.shape[1]) < max(ns):
        raise ValueError(f"log_probs must be ({batch}, >= {max(ns)}), got {tuple(lp.shape)}")
    dev = _hip.require_gpu()
    n_alpha = len(alphas)
    out_dev = map_dev if map_dev is not None else dev
    scores = torch.full((batch, n_alpha), float("nan"), dtype=torch.float32, device=dev)
    if n_alpha == 0:
        return scores if map_dev is not None else scores.cpu()
    code = _hip.ELEM_DTYPE_CODES[dtype]
    rows_h = torch.tensor([[p, n] for p, n in zip(pads, ns)], dtype=torch.int64)
    rows_d = rows_h.to(dev)
    lp_d = _hip.to_device(lp, torch.float32)
    al = torch.tensor([float(a) for a in alphas], dtype=torch.float64).to(dev)

    def score(att, n_l, n_h, width, mode, ws):
        _hip.launch("runia_rauqb_score", att.data_ptr(), rows_d.data_ptr(), batch, n_l, n_h, width, mode, tok, lp_d.data_ptr(),
                    lp_d.stride(0), al.data_ptr(), n_alpha, scores.data_ptr(), ws.data_ptr(), ws.numel())

    if head_mode != _SERIES:
        width = n_gen if tok else n_gen - 1
        if width >= 1:
            table, keep = _batch_table(attentions, dev, pads, first_row_only=True)
            w = torch.empty((batch, n_layers, heads, width), dtype=torch.float32, device=dev)
            _hip.launch("runia_rauqb_gather", table.data_ptr(), rows_d.data_ptr(), code, batch, n_gen, n_layers, heads, tok,
                        w.data_ptr())
            ws = _hip.workspace(_hip.query("runia_rauqb_workspace_bytes", batch, n_layers, width, 0, 0, n_alpha), dev, 0)
            score(w, n_layers, heads, width, head_mode, ws)
            del keep
    elif n_gen >= 2 and max(ns) >= 2:
        table, keep = _batch_table(attentions, dev, pads, first_row_only=False)
        flags = torch.zeros(batch, dtype=torch.int32, device=dev)

        def row_pass(chain_rows):
            ws = _hip.workspace(_hip.query("runia_rauqb_workspace_bytes", batch, n_layers, n_gen, in_len, chain_rows, 1), dev, 0)
            _hip.launch("runia_rauqb_rollout_rows", table.data_ptr(), rows_d.data_ptr(), code, batch, n_gen, n_layers, heads,
                        in_len, flags.data_ptr(), ws.data_ptr(), ws.numel())
            return ws

        ws = row_pass(1 if tok else 0)
        upper = flags.cpu()  # the B flags in one copy
        chained = [n for n, u in zip(ns, upper.tolist()) if n >= 2 and (tok or u)]
        k = 0 if not chained else (1 if tok else max(chained))
        if k > (1 if tok else 0):
            ws = row_pass(k)  # the n-row chains need the larger workspace: the row pass runs again into it
        att = torch.empty((batch, n_gen), dtype=torch.float32, device=dev)
        _hip.launch("runia_rauqb_rollout_att", table.data_ptr(), rows_d.data_ptr(), rows_h.data_ptr(), flags.data_ptr(),
                    upper.data_ptr(), code, batch, n_gen, n_layers, heads, in_len, tok, att.data_ptr(), ws.data_ptr(), ws.numel())
        score(att, 1, 1, n_gen, _SERIES, ws)
        del keep
    return scores if map_dev is not None else scores.cpu()
