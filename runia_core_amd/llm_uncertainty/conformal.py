"""Conformal next-token sets of an LLM generation (``csrc/conformal_wide.hip``): calibrate one threshold ``qhat`` on held-out
(logits, token) pairs - teacher-forced rows, or earlier generations - and attach to every step of a generation the set of tokens
that holds the true next token with probability at least ``1 - alpha``.  The definitions (LAC, APS, RAPS; ``u``; the quantile)
are those of ``evaluation/conformal.py``; what is new is the width: a vocabulary of 32 k to 256 k, where a row is never sorted
(the set of aps / raps is a prefix of the order, and the kernel finds the cut by a radix descent).  The set size is a
distribution-free per-token uncertainty; an APS set with ``u = 1`` is the calibrated nucleus (top-p) set.

``scores`` is ``generate(..., output_scores=True).scores``: T steps of ``(B, V)`` or ``(B, 1, V)``, float32 / float16 / bfloat16,
on the host or on one GPU, read in place through the descriptor table of ``llm_uncertainty/logits.py`` (nothing is stacked; host
steps go up in one pinned copy and the results come back on the host).  A plain ``[N, V]`` matrix is one step of N rows.
Without a GPU a valid call raises ``RuniaHipError``: there is no host fallback.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ..evaluation.calibration import _prepare
from ..evaluation.conformal import ConformalResult, _check_method, _label_scores, _row_numbers, conformal_quantile
from .logits import _steps, _table

__all__ = ["TokenConformal", "TokenSets"]


class TokenSets(NamedTuple):
    """``size`` (B, T) int32 and ``members`` (B, T, ceil(V / 32)) int32 (bit ``v % 32`` of word ``v // 32`` is token ``v``; None
    when not asked for), the threshold they were cut at and the vocabulary size.  On the device for device scores, on the host
    for host scores."""

    size: Tensor
    members: Optional[Tensor]
    qhat: float
    n_vocab: int

    def to_bool(self) -> Tensor:
        """The sets as a (B, T, V) bool tensor (plain torch: for inspection, not a hot path)."""
        if self.members is None:
            raise ValueError("these sets were predicted with return_members=False")
        shifts = torch.arange(32, dtype=torch.int32, device=self.members.device)
        bits = (self.members.unsqueeze(-1) >> shifts) & 1
        return bits.reshape(*self.members.shape[:2], -1)[..., :self.n_vocab].to(torch.bool)

    def tokens(self, b: int, t: int) -> np.ndarray:
        """The token ids of the set of row ``b`` at step ``t``, ascending (host int64)."""
        if self.members is None:
            raise ValueError("these sets were predicted with return_members=False")
        words = self.members[b, t].cpu().numpy().view(np.uint32)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.n_vocab]
        return np.flatnonzero(bits).astype(np.int64)

    def mean_log_size(self) -> Tensor:
        """(B,) float64: the mean over the steps of ``log(max(size, 1))`` - the per-generation score (0 when every set holds
        one token)."""
        return torch.log(self.size.clamp(min=1).to(torch.float64)).mean(dim=1)


def _as_steps(scores):
    """``scores`` -> what ``logits._steps`` takes: a [N, V] matrix (host array or tensor) is one step."""
    if isinstance(scores, np.ndarray):
        scores = torch.from_numpy(scores)
        if scores.dtype not in _hip.ELEM_DTYPE_CODES and scores.dtype.is_floating_point:
            scores = scores.to(torch.float32)
    if isinstance(scores, Tensor):
        if scores.dim() != 2:
            raise ValueError(f"a logits matrix must be [N, V], got shape {tuple(scores.shape)}")
        return (scores.detach(),)
    return scores


def _tokens(tokens, B: int, T: int, V: int, ignore_index: Optional[int]) -> Tensor:
    """The tokens of the T steps, (B, T) int64: ``tokens[:, -T:]`` of a (B, length) matrix as ``logits._token_ids`` cuts it, or a
    [B] vector for one step.  Ids lie in [0, V) or equal ``ignore_index`` (the pad id, which may itself lie in [0, V))."""
    if ignore_index is not None and not isinstance(ignore_index, (int, np.integer)):
        raise ValueError(f"ignore_index must be an integer or None, got {ignore_index!r}")
    tok = torch.as_tensor(tokens)
    if tok.dim() == 1 and T == 1:
        tok = tok.unsqueeze(1)
    if tok.dim() != 2:
        raise ValueError(f"tokens must be (B, length), got shape {tuple(tok.shape)}")
    if int(tok.shape[0]) != B:
        raise ValueError(f"tokens has {int(tok.shape[0])} rows, the scores have {B}")
    if int(tok.shape[1]) < T:
        raise ValueError(f"tokens has {int(tok.shape[1])} columns, fewer than the {T} steps")
    if tok.dtype.is_floating_point or tok.dtype.is_complex or tok.dtype == torch.bool:
        raise ValueError(f"tokens must hold integer token ids, not {tok.dtype}")
    tok = tok[:, tok.shape[1] - T:].to(torch.int64)
    off = (tok < 0) | (tok >= V)
    if ignore_index is not None:
        off &= tok != int(ignore_index)
    if bool(off.any()):
        raise ValueError(f"token ids must lie in [0, {V}) or equal ignore_index ({ignore_index!r})")
    return tok


def _flat_u(u, B: int, T: int):
    """A caller's ``u`` as one number per (b, t), flat in that order: (B, T) or [B * T]."""
    if u is None:
        return None
    if not isinstance(u, Tensor):
        u = np.asarray(u)
    if u.ndim == 2 and tuple(u.shape) == (B, T):
        u = u.reshape(B * T)
    return u


@_hip._device_guard()
def _wide_sets(scores, tokens, u, ignore_index, want_members, cfg: "TokenConformal"):
    rows, B, V, dtype, host_dev = _steps(_as_steps(scores))
    T = len(rows)
    if V > _hip.CONFORMAL_WIDE_MAX_CLASSES or B * T > _hip.CONFORMAL_WIDE_MAX_ROWS:
        raise ValueError(f"{T} steps of ({B}, {V}) logits exceed the kernel's size limits")
    tok = None if tokens is None else _tokens(tokens, B, T, V, ignore_index)
    u = _flat_u(u, B, T)
    dev = _hip.require_gpu()
    u = _row_numbers(u, B * T, cfg.method, cfg.randomized, cfg.seed + 1, dev)
    table, keep = _table(rows, dev)
    if tok is not None:
        tok = tok.to(dev).contiguous()
    sets = _hip.conformal_sets_wide(table, dtype, T, B, V, cfg.qhat_, cfg.method, 1.0 / cfg.temperature, u, cfg.lam, cfg.k_reg,
                                    tok, ignore_index, want_members)
    del keep  # (stream-ordered: the launch above reads it first)
    return sets, tok, B, T, V, host_dev is None


class TokenConformal:
    """Split conformal prediction over next tokens: ``calibrate`` finds ``qhat_`` on held-out (logits, token) pairs, ``predict``
    returns the set of every step of a generation in one launch, ``evaluate`` their coverage and sizes against the tokens.  The
    parameters, their checks and the ``u`` / seed rules are those of ``ConformalClassifier``; the state is host scalars only (it
    pickles)."""

    def __init__(self, method: str = "aps", alpha: float = 0.1, temperature: float = 1.0, randomized: bool = True,
                 lam: float = 0.0, k_reg: int = 0, seed: int = 0):
        _check_method(method, temperature, lam, k_reg)
        if not (0 < alpha < 1):
            raise ValueError(f"alpha must lie in (0, 1), got {alpha!r}")
        self.method = method
        self.alpha = float(alpha)
        self.temperature = float(temperature)
        self.randomized = bool(randomized)
        self.lam = float(lam)
        self.k_reg = int(k_reg)
        self.seed = int(seed)
        self.qhat_: Optional[float] = None
        self.n_calibration_: Optional[int] = None

    def calibrate(self, logits, tokens, ignore_index: Optional[int] = None, u=None) -> "TokenConformal":
        """``logits`` [N, V] with ``tokens`` [N] (teacher-forced rows), or T steps of (B, V) / (B, 1, V) with
        ``tokens = sequences`` (B, length), whose last T columns are scored; the pad id goes as ``ignore_index``.  The label
        scores come from the one-pass label kernel of ``evaluation/conformal.py`` (any width), one launch per step."""
        if isinstance(logits, (Tensor, np.ndarray)):
            x, y = _prepare(logits, tokens if isinstance(tokens, Tensor) else np.asarray(tokens), ignore_index)
            n = x.shape[0]
            uu = _row_numbers(u, n, self.method, self.randomized, self.seed, x.device)
            s = _label_scores(x, y, self.method, self.temperature, uu, self.lam, self.k_reg, ignore_index)
            keep = None if ignore_index is None else y != int(ignore_index)
        else:
            rows, B, V, _, _ = _steps(logits)
            T = len(rows)
            tok = _tokens(tokens, B, T, V, ignore_index)
            u = _flat_u(u, B, T)
            dev = _hip.require_gpu()
            uu = _row_numbers(u, B * T, self.method, self.randomized, self.seed, dev)
            tok = tok.to(dev)
            per_step = []
            for t, r in enumerate(rows):
                ut = None if uu is None else uu.view(B, T)[:, t].contiguous()
                per_step.append(_label_scores(r.to(dev), tok[:, t].contiguous(), self.method, self.temperature, ut, self.lam,
                                              self.k_reg, ignore_index))
            s = torch.stack(per_step, dim=1).reshape(-1)
            keep = None if ignore_index is None else tok.reshape(-1) != int(ignore_index)
        if keep is not None:
            s = s[keep]
        if s.numel() == 0:
            raise ValueError("calibrate: no scored token (tokens is empty or all ignore_index)")
        self.qhat_ = conformal_quantile(s, self.alpha)
        self.n_calibration_ = int(s.numel())
        return self

    def _checked(self):
        if self.qhat_ is None:
            raise ValueError("calibrate the predictor first")

    def predict(self, scores, u=None, return_members: bool = False) -> TokenSets:
        self._checked()
        sets, _, B, T, V, to_host = _wide_sets(scores, None, u, None, return_members, self)
        size = sets.size.view(B, T)
        members = None if sets.members is None else sets.members.view(B, T, -1)
        if to_host:
            size, members = size.cpu(), None if members is None else members.cpu()
        return TokenSets(size, members, self.qhat_, V)

    def evaluate(self, scores, tokens, u=None, ignore_index: Optional[int] = None) -> ConformalResult:
        """Coverage and sizes of the sets against the tokens (``tokens`` as in ``calibrate``); ``class_coverage`` and
        ``class_count`` are per token id, [V]."""
        self._checked()
        sets, tok, _, _, V, _ = _wide_sets(scores, tokens, u, ignore_index, False, self)
        rec = _hip.conformal_record(_hip.to_host(_hip.conformal_reduce(sets, tok.reshape(-1), V, ignore_index)), V)
        n = rec["n_used"]
        count, hit = rec["class_count"], rec["class_covered"]
        with np.errstate(invalid="ignore", divide="ignore"):
            class_coverage = np.where(count > 0, hit / count, np.nan)
        nan = float("nan")
        return ConformalResult(rec["n_covered"] / n if n else nan, rec["size_sum"] / n if n else nan, rec["hist"], class_coverage,
                               count, n, self.qhat_)
