"""Embedding-level sample consistency: the greedy token matching of BERTScore (Zhang et al. 2020; SelfCheckGPT-BERTScore,
Manakul et al. 2023) between the samples of a prompt, on the model's OWN hidden states - the sampled ``generate()`` call of
``compute_uncertainties`` already returned them, so the similarity costs no extra forward pass and no second model.

Rows are prompt-major, as in ``.consistency``: group g is rows ``g*K .. g*K+K-1``, ``2 <= K <= 64``.  The content of row r is
the states of one layer over its window ``(start_r, n_r)``; the window rules and both input forms are those of
``hidden_score`` (``generate()`` default ``[P, P + lengths[r] - 1)``), ``n_r = 0`` is allowed, ``n_r <= 1024``.

- centring (``center=True``): every token loses ``m_g``, the mean of all content tokens of its group - LLM states are strongly
  anisotropic, without it every cosine sits near 1; ``center=False`` uses the tokens as they are;
- ``x^ = x / |x|``; a zero token has cosine 0 with everything;
- ``coverage[g, i, j] = (1 / n_i) sum_{a in i} max_{b in j} <x^_a, y^_b>``: how well sample i is covered by sample j
  (directional); both contents empty gives 1, exactly one empty 0;
- ``similarity``: with ``R = max(cov[i, j], 0)``, ``P = max(cov[j, i], 0)``, ``w_ij = 2 P R / (P + R)`` (0 when ``P + R = 0``) and
  ``w_ii = 1`` - continuous everywhere, in [0, 1], symmetric, and with the empty-sample rules of the id similarities;
- a NaN (or infinite) state makes every entry of its group NaN and leaves the other groups alone.

Everything of size ``T x T`` stays in registers: ``csrc/cons_embed.hip`` reads the states where they lie through
the descriptor table of LLM-Check, multiplies on the matrix cores and keeps only row and column maxima.  Without a GPU a valid
call raises ``RuniaHipError``: there is no host fallback.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .. import _hip
from .consistency import ConsistencyScores, graph_scores
from .llm_check import _positions, _steps, _windows
from .rauq import _upload_parts

__all__ = ["EmbeddingSimilarity", "embedding_similarity", "embedding_consistency_scores", "EMBED_MAX_TOKENS"]

EMBED_MAX_TOKENS = _hip._HEADER_MACROS["RUNIA_CONS_EMBED_MAX_T"]


class EmbeddingSimilarity(NamedTuple):
    """``similarity`` and ``coverage``: ``(G, K, K)`` f64; ``n``: ``(G * K,)`` int32 content lengths.  On the device (on the
    host for host states)."""

    similarity: torch.Tensor
    coverage: torch.Tensor
    n: torch.Tensor


def _similarity_of(cov: torch.Tensor) -> torch.Tensor:
    """(G, K, K) f64 harmonic mean of the two clamped coverages of every pair; the diagonal is 1, NaN stays NaN."""
    r = cov.clamp_min(0.0)
    p = r.transpose(1, 2)
    total = p + r
    one = torch.ones((), dtype=torch.float64, device=cov.device)
    w = torch.where(total == 0, torch.zeros_like(total), 2.0 * p * r / torch.where(total == 0, one, total))
    eye = torch.eye(cov.shape[1], dtype=torch.bool, device=cov.device)
    return torch.where(eye & ~cov.isnan().flatten(1).any(dim=1)[:, None, None], one, w)


@_hip._device_guard()
def embedding_similarity(hidden_states, num_samples: int, layer: int = 15, *, center: bool = True, input_length=None,
                         attention_mask=None, lengths=None, windows=None) -> EmbeddingSimilarity:
    """Coverage and similarity of the samples of every group of ``num_samples`` consecutive rows of ``hidden_states`` at
    ``layer`` (an index into the layer tuple, HuggingFace's: 0 is the embedding output).  ``hidden_states`` is a forward pass's
    tuple over layers of ``(G * K, T, d)`` tensors or a ``generate()`` output's tuple over steps of such tuples; f32, f16 or
    bf16; on one GPU (any batch / row strides, read in place) or on the host (one upload, results come back).  ``input_length``,
    ``attention_mask``, ``lengths`` and ``windows`` as for ``hidden_score``.  One call of ``runia_cons_embed``."""
    steps, forward = _steps(hidden_states, (int(layer),), 3, "hidden_states")
    for g, step in enumerate(steps[1:], 1):
        if int(step[0].shape[1]) != 1:
            raise ValueError(f"step {g} of a generate() output holds one position")
    k = int(num_samples)
    if not 2 <= k <= _hip.CONS_MAX_K:
        raise ValueError(f"groups of num_samples = {num_samples}: the kernel takes 2 <= num_samples <= {_hip.CONS_MAX_K}")
    first = steps[0][0]
    batch, q0, d = (int(v) for v in first.shape)
    if batch % k:
        raise ValueError(f"{batch} rows do not form groups of num_samples = {k}")
    prompt, n_pos = _positions(q0, len(steps), forward, input_length)
    rows_h, empty, _ = _windows(batch, prompt, n_pos, not forward, attention_mask, lengths, windows)
    rows_h[torch.tensor(empty)] = 0  # (an empty content is a window of its own here, not a row to skip)
    t_max = int(rows_h[:, 1].max())
    if t_max > EMBED_MAX_TOKENS:
        raise ValueError(f"a window of {t_max} tokens: at most {EMBED_MAX_TOKENS} are supported")
    dev = _hip.require_gpu()
    flat = [step[0] for step in steps]
    on_host = not first.is_cuda
    if on_host:
        keep, addresses = _upload_parts(flat, dev)
        table = [[at, t.shape[1] * d, d] for at, t in zip(addresses, flat)]
    else:
        keep = [t if t.stride(2) == 1 or d == 1 else t.contiguous() for t in flat]
        table = [[t.data_ptr(), t.stride(0), t.stride(1)] for t in keep]
    table_d = torch.tensor(table, dtype=torch.int64).to(dev)
    rows_d = rows_h.to(dev)
    groups = batch // k
    cov = torch.empty((groups, k, k), dtype=torch.float64, device=dev)
    ws = _hip.workspace(_hip.query("runia_cons_embed_workspace_bytes", groups, k, t_max, d), dev)
    _hip.launch("runia_cons_embed", table_d.data_ptr(), rows_d.data_ptr(), rows_h.data_ptr(), _hip.ELEM_DTYPE_CODES[first.dtype],
                groups, k, len(steps), q0, d, int(bool(center)), cov.data_ptr(), ws.data_ptr(), ws.numel())
    del keep
    out = EmbeddingSimilarity(_similarity_of(cov), cov, rows_d[:, 1].to(torch.int32))
    return EmbeddingSimilarity(*(t.cpu() for t in out)) if on_host else out


def embedding_consistency_scores(hidden_states, num_samples: int, layer: int = 15, *, eigv_threshold: float = 0.9,
                                 set_threshold: float = 0.5, **kwargs) -> ConsistencyScores:
    """``graph_scores(embedding_similarity(hidden_states, num_samples, layer, **kwargs).similarity)``: NumSet / Deg / Ecc / EigV
    and the mean pairwise similarity over the embedding-level similarity of a batch of sampled generations."""
    w = embedding_similarity(hidden_states, num_samples, layer, **kwargs).similarity
    return graph_scores(w, eigv_threshold=eigv_threshold, set_threshold=set_threshold)
