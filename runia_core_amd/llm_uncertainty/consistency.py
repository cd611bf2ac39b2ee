"""Sample-consistency (black-box) uncertainty scores: they need only the sampled token ids of
``generate(num_return_sequences=num_samples)``, no logits and no hidden states.

- lexical similarity: the mean pairwise ROUGE-L of a prompt's samples (Fomicheva et al. 2020);
- NumSet, Deg, Ecc, EigV: the graph scores over a pairwise similarity matrix (Lin, Trivedi and Sun 2023, "Generating with
  Confidence"), here over ROUGE-L or Jaccard of the token ids - or over any similarity the caller brings, such as NLI
  entailment probabilities (``graph_scores``).

Rows are prompt-major: group g is rows ``g*K .. g*K+K-1``, ``2 <= K <= 64``.  The content of a row is its ids from column
``start`` on, cut before the first eos id (the eos is excluded: otherwise every pair shares one token for free) and at
``lengths[row]``; ``n_i`` is its length, 0 allowed.  ``lcs[i, j]`` is the LCS length of contents i and j, ``uniq[i]`` the number
of distinct ids, ``inter[i, j]`` the number of distinct ids in common.

    rouge_l   2 lcs / (n_i + n_j)                      (the ROUGE-L F-measure with beta = 1)
    jaccard   inter / (uniq_i + uniq_j - inter)        both: 1 when both contents are empty, 0 when exactly one is

Graph scores of a similarity W (upper triangle read, diagonal taken as 1): ``d_i = sum_j w_ij``, ``L = I - D^-1/2 W D^-1/2``
with eigenvalues ascending; ``lexical_similarity = mean_{i<j} w_ij``, ``u_deg = 1 - sum w / K^2``, ``c_deg = d / K``,
``u_eigv = sum max(0, 1 - lambda)``, ``c_ecc[i] = -s_i`` and ``u_ecc = sqrt(sum s_i^2)`` with ``s_i`` the norm of row i of the
eigenvectors of ``lambda < eigv_threshold`` centred over the rows, ``num_sets`` the connected components of
``{w_ij >= set_threshold}``.  A non-finite entry makes its group NaN / -1 and leaves the others alone.

Everything runs in two entry points of the library (``runia_cons_pairs``, ``runia_cons_graph``; csrc/consistency.hip); without
a GPU the calls raise ``RuniaHipError``: there is no host fallback.
"""
from __future__ import annotations

import re
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _hip

__all__ = ["PairCounts", "ConsistencyScores", "pairwise_counts", "pairwise_similarity", "graph_scores", "consistency_scores",
           "word_ids", "SIMILARITIES"]

SIMILARITIES = ("rouge_l", "jaccard")


class PairCounts(NamedTuple):
    """Integer tables of ``pairwise_counts`` (int32, where the ids lie): ``len`` and ``uniq`` are ``(G * K,)``, ``lcs`` and
    ``inter`` ``(G, K, K)``; a table that was not asked for is ``None``."""

    len: torch.Tensor
    lcs: Optional[torch.Tensor]
    uniq: Optional[torch.Tensor]
    inter: Optional[torch.Tensor]


class ConsistencyScores(NamedTuple):
    """What ``graph_scores`` returns, f64 where the similarity lies: ``(G,)`` scalars per group, ``(G, K)`` per sample
    (``num_sets`` int32); without the leading dimension for a ``(K, K)`` similarity."""

    eigenvalues: torch.Tensor
    u_deg: torch.Tensor
    u_eigv: torch.Tensor
    u_ecc: torch.Tensor
    lexical_similarity: torch.Tensor
    c_deg: torch.Tensor
    c_ecc: torch.Tensor
    num_sets: torch.Tensor
    similarity: torch.Tensor


def _eos_list(eos_token_id) -> List[int]:
    if eos_token_id is None:
        return []
    if isinstance(eos_token_id, bool):
        raise TypeError("eos_token_id must be an int or a sequence of ints")
    if isinstance(eos_token_id, int):
        return [eos_token_id]
    if isinstance(eos_token_id, torch.Tensor):
        eos_token_id = eos_token_id.tolist()
    out = [int(v) for v in eos_token_id]
    if len(out) > _hip.CONS_MAX_EOS:
        raise ValueError(f"{len(out)} eos ids: the kernel takes at most {_hip.CONS_MAX_EOS}")
    return out


def _checked_ids(sequences, num_samples, start, lengths):
    """Argument checks of the id functions -> (view of the content columns, K, lengths or None); nothing touches the device."""
    if not isinstance(sequences, torch.Tensor) or sequences.dim() != 2:
        raise ValueError("sequences must be a 2-D (G * num_samples, T) tensor of token ids")
    if sequences.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"token ids must be int32 or int64, not {sequences.dtype}")
    k = int(num_samples)
    if not 2 <= k <= _hip.CONS_MAX_K:
        raise ValueError(f"groups of num_samples = {num_samples}: the kernels take 2 <= num_samples <= {_hip.CONS_MAX_K}")
    n, width = (int(v) for v in sequences.shape)
    if n == 0 or n % k:
        raise ValueError(f"{n} rows do not form groups of num_samples = {k}")
    start = int(start)
    if not 0 <= start <= width:
        raise ValueError(f"start = {start} is outside the {width} columns")
    if width - start > _hip.CONS_MAX_T:
        raise ValueError(f"{width - start} content columns: the kernels take at most {_hip.CONS_MAX_T}")
    if lengths is not None:
        lengths = torch.as_tensor(lengths)
        if lengths.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise TypeError(f"lengths must be integers, not {lengths.dtype}")
        if tuple(lengths.shape) != (n,):
            raise ValueError(f"lengths must be ({n},), one per row, got {tuple(lengths.shape)}")
    return sequences.detach()[:, start:], k, lengths


def pairwise_counts(sequences: torch.Tensor, num_samples: int, *, start: int = 0, eos_token_id=None, lengths=None,
                    jaccard: bool = True, lcs: bool = True) -> PairCounts:
    """The integer tables of every group of ``num_samples`` consecutive rows of ``sequences`` ``(G * K, T)`` int32 / int64
    (``generate(...).sequences``: pass ``start=input_length`` or the view ``sequences[:, input_length:]``; any strides, read in
    place).  ``eos_token_id``: an int or up to 16 ints; ``lengths``: ``(G * K,)`` content lengths counted from ``start``.  At
    most 4 096 content columns.  ``jaccard=False`` / ``lcs=False`` leave out ``uniq`` and ``inter`` / ``lcs``.  One call of
    ``runia_cons_pairs``; a host tensor goes up in one copy and the tables come back to the host."""
    _hip.load_library()  # a missing library is reported before any argument
    ids, k, lengths = _checked_ids(sequences, num_samples, start, lengths)
    eos = _eos_list(eos_token_id)
    if not (lcs or jaccard):
        raise ValueError("ask for at least one of lcs and jaccard")
    dev = _hip.require_gpu()
    on_host = not ids.is_cuda
    if on_host:
        ids = ids.contiguous().to(dev)
    eos_t = torch.tensor(eos, dtype=torch.int64).to(ids.device) if eos else None
    len_t = None if lengths is None else lengths.to(device=ids.device, dtype=torch.int64).contiguous()
    out = _hip.cons_pairs(ids, k, eos_t, len_t, lcs=bool(lcs), jaccard=bool(jaccard))
    if on_host:
        out = tuple(None if t is None else t.cpu() for t in out)
    return PairCounts(*out)


def _similarity_of(counts: PairCounts, kind: str) -> torch.Tensor:
    """(G, K, K) f64 from the tables, on their device (K x K element-wise arithmetic; both-empty pairs and the diagonal are 1)."""
    if kind == "rouge_l":
        num = 2.0 * counts.lcs.double()
        size = counts.len.double().view(num.shape[0], num.shape[1])
        den = size[:, :, None] + size[:, None, :]
    else:
        num = counts.inter.double()
        size = counts.uniq.double().view(num.shape[0], num.shape[1])
        den = size[:, :, None] + size[:, None, :] - num
    one = torch.ones((), dtype=torch.float64, device=num.device)
    w = torch.where(den == 0, one, num / torch.where(den == 0, one, den))
    w.diagonal(dim1=1, dim2=2).fill_(1.0)
    return w


def _check_kind(kind):
    if kind not in SIMILARITIES:
        raise ValueError(f"kind must be one of {SIMILARITIES}, got {kind!r}")


def pairwise_similarity(sequences: torch.Tensor, num_samples: int, *, kind: str = "rouge_l", start: int = 0, eos_token_id=None,
                        lengths=None) -> torch.Tensor:
    """``(G, K, K)`` f64 similarity of the samples of every group (symmetric, diagonal exactly 1), where the ids lie:
    ``kind="rouge_l"`` or ``"jaccard"`` of the token ids (see the module docstring).  Arguments as ``pairwise_counts``."""
    _check_kind(kind)
    counts = pairwise_counts(sequences, num_samples, start=start, eos_token_id=eos_token_id, lengths=lengths,
                             jaccard=kind == "jaccard", lcs=kind == "rouge_l")
    return _similarity_of(counts, kind)


def graph_scores(similarity: torch.Tensor, *, eigv_threshold: float = 0.9, set_threshold: float = 0.5) -> ConsistencyScores:
    """NumSet / Deg / Ecc / EigV and the lexical similarity of ``similarity`` ``(G, K, K)`` or ``(K, K)``, any floating dtype,
    host or one GPU: one launch of ``runia_cons_graph`` for all groups.  Only the upper triangle is read and the diagonal is
    taken as 1; values are expected in [0, 1].  ``eigv_threshold`` (0.9, the authors' value) selects the eigenvectors of Ecc,
    ``set_threshold`` the edges of ``num_sets``.  Any similarity does: with NLI entailment probabilities this gives the
    paper's NLI variants."""
    _hip.load_library()
    if not isinstance(similarity, torch.Tensor) or similarity.dim() not in (2, 3) or similarity.shape[-1] != similarity.shape[-2]:
        raise ValueError("similarity must be a (G, K, K) or (K, K) tensor")
    if not similarity.dtype.is_floating_point:
        raise TypeError(f"similarity must be a floating-point tensor, not {similarity.dtype}")
    k = int(similarity.shape[-1])
    if not 2 <= k <= _hip.CONS_MAX_K:
        raise ValueError(f"K = {k} samples: the kernel takes 2 <= K <= {_hip.CONS_MAX_K}")
    if similarity.dim() == 3 and similarity.shape[0] == 0:
        raise ValueError("similarity holds no group")
    eigv_threshold, set_threshold = float(eigv_threshold), float(set_threshold)
    if eigv_threshold != eigv_threshold or set_threshold != set_threshold:
        raise ValueError("the thresholds must be numbers")
    dev = _hip.require_gpu()
    single, on_host = similarity.dim() == 2, not similarity.is_cuda
    w = similarity.detach()
    w = (w[None] if single else w).to(device=dev if on_host else w.device, dtype=torch.float64).contiguous()
    out = _hip.cons_graph(w, eigv_threshold, set_threshold) + (w,)
    if on_host:
        out = tuple(t.cpu() for t in out)
    if single:
        out = tuple(t[0] for t in out)
    return ConsistencyScores(*out)


def consistency_scores(sequences: torch.Tensor, num_samples: int, *, kind: str = "rouge_l", start: int = 0, eos_token_id=None,
                       lengths=None, eigv_threshold: float = 0.9, set_threshold: float = 0.5) -> ConsistencyScores:
    """``graph_scores(pairwise_similarity(sequences, num_samples, kind=...))``: every score of a batch of sampled generations
    from their ids, e.g. ``consistency_scores(out.sequences[:, n_in:], K, eos_token_id=eos)``, without leaving the device."""
    w = pairwise_similarity(sequences, num_samples, kind=kind, start=start, eos_token_id=eos_token_id, lengths=lengths)
    return graph_scores(w, eigv_threshold=eigv_threshold, set_threshold=set_threshold)


def scores_by_kind(sequences: torch.Tensor, num_samples: int, kinds: Sequence[str], *, start: int = 0, eos_token_id=None,
                   lengths=None, eigv_threshold: float = 0.9, set_threshold: float = 0.5):
    """``{kind: consistency_scores(..., kind=kind)}`` for several similarities from ONE ``runia_cons_pairs`` call and ONE
    ``runia_cons_graph`` launch (the similarities are stacked along the group dimension)."""
    kinds = list(dict.fromkeys(kinds))
    for kind in kinds:
        _check_kind(kind)
    counts = pairwise_counts(sequences, num_samples, start=start, eos_token_id=eos_token_id, lengths=lengths,
                             jaccard="jaccard" in kinds, lcs="rouge_l" in kinds)
    g = counts.len.shape[0] // int(num_samples)
    both = graph_scores(torch.cat([_similarity_of(counts, kind) for kind in kinds]), eigv_threshold=eigv_threshold,
                        set_threshold=set_threshold)
    return {kind: ConsistencyScores(*(t[i * g:(i + 1) * g] for t in both)) for i, kind in enumerate(kinds)}


_WORD = re.compile(r"[a-z0-9]+")


def word_ids(texts: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host helper for word-level ROUGE-L of decoded text: every text is lower-cased and split into its ``[a-z0-9]+`` runs, and
    the words are numbered in one vocabulary shared by the texts (from 1, in order of first appearance).  Returns the
    right-padded ``(N, T)`` int64 ids (padding 0, ``T`` the longest text, at least 1) and the ``(N,)`` int64 ``lengths``:
    ``pairwise_similarity(ids, K, lengths=lengths)`` is then ``rouge_score``'s ROUGE-L F-measure on its default tokens."""
    if isinstance(texts, str) or not all(isinstance(t, str) for t in texts):
        raise TypeError("texts must be a sequence of strings")
    vocab: dict = {}
    rows = [[vocab.setdefault(w, len(vocab) + 1) for w in _WORD.findall(t.lower())] for t in texts]
    width = max([len(r) for r in rows] + [1])
    ids = torch.zeros((len(rows), width), dtype=torch.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return ids, torch.tensor([len(r) for r in rows], dtype=torch.int64)
