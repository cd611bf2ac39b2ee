"""PaCMAP embedding on the device: the reference's ``fit_pacmap`` / ``apply_pacmap_transform`` / ``plot_samples_pacmap``
(``dimensionality_reduction.py:88-177``, on ``pacmap==0.7.0``, which is not on this platform).

The algorithm is the published one (Wang, Huang, Rudin, Shaposhnik, JMLR 22(201), 2021) with the choices listed in
INTEGRATION.md ("PaCMAP"): an exact kNN graph in place of Annoy, pair draws from a Philox4x32-10 stream keyed by
``random_state``, and a transform that optimises the new rows against the frozen fitted ones.  The kNN graph, the pair
sampling and every Adam iteration are kernels of ``csrc/pacmap.hip``; preprocessing reductions and the grouping of the
pairs by row (a stable device sort) are torch plumbing.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip

__all__ = ["PaCMAP", "fit_pacmap", "apply_pacmap_transform", "plot_samples_pacmap"]

_PCA_DIMS = 100  # rows wider than this are projected (apply_pca=True)
_EXTRA_CANDIDATES = 50  # kNN candidates beyond n_neighbors for the scaled-distance selection


def philox_words(rows: np.ndarray, c1: np.ndarray, c2: int, c3: int, seed: int) -> np.ndarray:
    """Philox4x32-10 output words ``(..., 4)`` uint32 of the counters ``(rows, c1, c2, c3)`` keyed by ``seed`` - the draws
    of ``csrc/pacmap.hip`` restated on the host (the "random" init is drawn here)."""
    rows, c1 = np.broadcast_arrays(np.asarray(rows, dtype=np.uint64), np.asarray(c1, dtype=np.uint64))
    mask = np.uint64(0xFFFFFFFF)
    c = [rows & mask, c1 & mask, np.full(rows.shape, c2, np.uint64), np.full(rows.shape, c3, np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & mask, p1 & mask, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & mask, p0 & mask]
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def random_init(n: int, n_components: int, seed: int) -> np.ndarray:
    """``1e-4 x`` standard normal draws: Box-Muller of words 0 and 1 of counter ``(row, (2 << 16) | component, 0, 0)``."""
    rows = np.arange(n, dtype=np.uint64)[:, None]
    comps = (np.uint64(2 << 16) | np.arange(n_components, dtype=np.uint64))[None, :]
    w = philox_words(rows, comps, 0, 0, seed).astype(np.float64)
    u1 = (np.floor(w[..., 0] / 256.0) + 1.0) * 2.0 ** -24  # (0, 1]
    u2 = np.floor(w[..., 1] / 256.0) * 2.0 ** -24
    return (1e-4 * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).astype(np.float32)


def _pack_entries(partner: torch.Tensor, kind: int) -> torch.Tensor:
    """int32 ``(kind << 30) | partner`` (bit pattern; kind 2 sets the sign bit)."""
    e = partner.to(torch.int64) + (kind << 30)
    return torch.where(e >= 2 ** 31, e - 2 ** 32, e).to(torch.int32)


def group_pairs(n: int, pairs) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pair lists ``[(pairs [P, 2] int32, kind), ...]`` of a fit -> ``(offsets [n + 1] int64, entries int32)``: every pair once
    under each endpoint, grouped by row with a stable sort (within a row: NB, MN, FP, in list order, first endpoints then
    second endpoints of each kind)."""
    dest, ent = [], []
    for p, kind in pairs:
        if p.numel() == 0:
            continue
        dest += [p[:, 0], p[:, 1]]
        ent += [_pack_entries(p[:, 1], kind), _pack_entries(p[:, 0], kind)]
    dest_t = torch.cat(dest).to(torch.int64)
    order = torch.sort(dest_t, stable=True).indices
    entries = torch.cat(ent)[order].contiguous()
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dest_t.device)
    offsets[1:] = torch.cumsum(torch.bincount(dest_t, minlength=n), 0)
    return offsets, entries


class PaCMAP:
    """Pairwise Controlled Manifold Approximation on the GPU, with pacmap 0.7's constructor and ``fit`` /
    ``fit_transform`` / ``transform``.  An ndarray in gives an f32 ndarray out; a CUDA tensor in gives a CUDA tensor out."""

    _device_attrs = ("_x_dev", "_y_dev", "_pairs_dev")

    def __init__(self, n_components: int = 2, n_neighbors: int = 10, MN_ratio: float = 0.5, FP_ratio: float = 2.0,
                 lr: float = 1.0, num_iters: int = 450, apply_pca: bool = True, random_state: Optional[int] = None,
                 distance: str = "euclidean"):
        self.n_components = int(n_components)
        self.n_neighbors = int(n_neighbors)
        self.MN_ratio = float(MN_ratio)
        self.FP_ratio = float(FP_ratio)
        self.n_MN = int(self.n_neighbors * self.MN_ratio)
        self.n_FP = int(self.n_neighbors * self.FP_ratio)
        self.lr = float(lr)
        self.num_iters = int(num_iters)
        self.apply_pca = bool(apply_pca)
        self.random_state = random_state
        self.distance = distance
        self.embedding_ = None
        self.seed_ = None
        self.n_rows_ = None
        self.preprocess_ = None  # ("pca", components [100, D] f64, mean [D] f64, variance) or ("scale", min, max, mean [D])
        self._pairs_host = {}
        self._x_dev = self._y_dev = self._pairs_dev = None

    # ---- argument checks (before any launch) ------------------------------------------------------------------------------
    def _check_params(self) -> None:
        if self.distance != "euclidean":
            raise NotImplementedError(f"distance={self.distance!r}: only 'euclidean' is implemented")
        if not 1 <= self.n_components <= _hip.PACMAP_MAX_COMPONENTS:
            raise ValueError(f"n_components={self.n_components}: 1 to {_hip.PACMAP_MAX_COMPONENTS} are supported")
        if not 1 <= self.n_neighbors <= _hip.PACMAP_MAX_K - _EXTRA_CANDIDATES:
            raise ValueError(f"n_neighbors={self.n_neighbors}: 1 to {_hip.PACMAP_MAX_K - _EXTRA_CANDIDATES} are supported")
        if not 0 <= self.n_MN <= _hip.PACMAP_MAX_MN:
            raise ValueError(f"n_neighbors * MN_ratio = {self.n_MN}: 0 to {_hip.PACMAP_MAX_MN} mid-near pairs per row")
        if not 0 <= self.n_FP <= _hip.PACMAP_MAX_FP:
            raise ValueError(f"n_neighbors * FP_ratio = {self.n_FP}: 0 to {_hip.PACMAP_MAX_FP} further pairs per row")
        if self.num_iters < 0:
            raise ValueError(f"num_iters={self.num_iters} must be >= 0")

    def _check_fit_shape(self, shape) -> None:
        if len(shape) != 2:
            raise ValueError(f"X must be 2-D, got shape {tuple(shape)}")
        n = shape[0]
        if n <= self.n_neighbors:
            raise ValueError(f"{n} rows: PaCMAP needs more rows than n_neighbors={self.n_neighbors}")
        if self.n_FP > n - 1 - self.n_neighbors:
            raise ValueError(f"{n} rows leave {n - 1 - self.n_neighbors} candidates for {self.n_FP} distinct further pairs "
                             "per row")
        if self.apply_pca and shape[1] > _PCA_DIMS and n < _PCA_DIMS:
            raise ValueError(f"{n} rows: the projection to {_PCA_DIMS} columns needs at least {_PCA_DIMS} rows")

    # ---- preprocessing --------------------------------------------------------------------------------------------------------
    def _fit_preprocess(self, x: torch.Tensor) -> Tuple[torch.Tensor, bool]:
        from .device_fit import pca_fit_device

        if self.apply_pca and x.shape[1] > _PCA_DIMS:
            pca = pca_fit_device(x, _PCA_DIMS, whiten=False)
            self.preprocess_ = ("pca", pca.components_, pca.mean_, pca.explained_variance_)
            return self._apply_preprocess(x), True
        xmin = float(x.min().item())
        x = x - xmin
        xmax = float(x.max().item())
        x = x / xmax
        mean = x.mean(dim=0)
        self.preprocess_ = ("scale", xmin, xmax, _hip.to_host(mean))
        return (x - mean).contiguous(), False

    def _apply_preprocess(self, x: torch.Tensor) -> torch.Tensor:
        from .dimensionality_reduction import DevicePCA

        kind = self.preprocess_[0]
        if kind == "pca":
            _, comps, mean, var = self.preprocess_
            if x.shape[1] != comps.shape[1]:
                raise ValueError(f"X has {x.shape[1]} columns, the fit had {comps.shape[1]}")
            return DevicePCA(comps, mean, var, False).transform_device(x).to(torch.float32).contiguous()
        _, xmin, xmax, mean = self.preprocess_
        if x.shape[1] != mean.shape[0]:
            raise ValueError(f"X has {x.shape[1]} columns, the fit had {mean.shape[0]}")
        return ((x - xmin) / xmax - torch.as_tensor(mean, device=x.device)).contiguous()

    # ---- fit ------------------------------------------------------------------------------------------------------------------
    def fit(self, X, init: str = "pca"):
        self.fit_transform(X, init=init)
        return self

    def fit_transform(self, X, init: str = "pca"):
        self._check_params()
        if init not in ("pca", "random"):
            raise ValueError(f"init={init!r}: 'pca' or 'random'")
        on_dev = isinstance(X, torch.Tensor) and X.is_cuda
        self._check_fit_shape(tuple(X.shape))
        seed = self.random_state if self.random_state is not None else int(np.random.randint(0, 2 ** 31 - 1))
        self.seed_ = int(seed)
        _hip.require_gpu()
        x = X.to(torch.float32).contiguous() if on_dev else _hip.to_device(np.asarray(X, dtype=np.float32), torch.float32)
        with torch.cuda.device(x.device):
            y = self._fit_device(x, init)
        self.embedding_ = y if on_dev else _hip.to_host(y)
        return self.embedding_

    def _fit_device(self, x: torch.Tensor, init: str) -> torch.Tensor:
        from .device_fit import pca_fit_device
        from .dimensionality_reduction import DevicePCA

        n = x.shape[0]
        xp, projected = self._fit_preprocess(x)
        self.n_rows_ = n
        self._x_dev = xp
        k = min(self.n_neighbors + _EXTRA_CANDIDATES, n - 1)
        idx, dist = _hip.pacmap_knn(xp, xp, k, exclude_self=True)
        nb, mn, fp = _hip.pacmap_pairs(xp, xp, idx, dist, self.n_neighbors, self.n_MN, self.n_FP, self.seed_, False)
        self._pairs_dev = (nb, mn, fp)
        self._pairs_host = {}
        c = self.n_components
        if init == "random":
            y = _hip.to_device(random_init(n, c, self.seed_), torch.float32)
        elif projected:
            y = (0.01 * xp[:, :c]).contiguous()
        else:
            pca = pca_fit_device(xp, c, whiten=False)
            scores = DevicePCA(pca.components_, pca.mean_, pca.explained_variance_, False).transform_device(xp)
            y = (0.01 * scores).to(torch.float32).contiguous()
        offsets, entries = group_pairs(n, [(nb, _hip.PACMAP_KIND_NB), (mn, _hip.PACMAP_KIND_MN), (fp, _hip.PACMAP_KIND_FP)])
        y = optimise(y, y_part=None, offsets=offsets, entries=entries, num_iters=self.num_iters, lr=self.lr)
        self._y_dev = y
        return y

    # ---- transform ------------------------------------------------------------------------------------------------------------
    def transform(self, X, basis=None):
        """Embed new rows against the fitted ones ("PaCMAP"): each new row takes NB pairs to its
        ``n_neighbors`` nearest fitted rows and ``n_FP`` FP pairs to other fitted rows, starts at the fitted position of its
        nearest one and runs the iteration schedule with the fitted rows frozen.  ``basis``: the fitted rows (same row
        count; needed after unpickling, when the preprocessed rows are no longer held)."""
        self._check_params()
        if self.embedding_ is None:
            raise ValueError("transform before fit")
        if len(X.shape) != 2:
            raise ValueError(f"X must be 2-D, got shape {tuple(X.shape)}")
        if basis is not None and basis.shape[0] != self.n_rows_:
            raise ValueError(f"basis has {basis.shape[0]} rows, the fit had {self.n_rows_}")
        if basis is None and self._x_dev is None:
            raise ValueError("this estimator holds no fitted rows (unpickled): pass basis=<the fitted rows>")
        if self.n_FP > self.n_rows_ - self.n_neighbors:
            raise ValueError(f"{self.n_rows_} fitted rows leave too few further pairs for {self.n_FP} per new row")
        on_dev = isinstance(X, torch.Tensor) and X.is_cuda
        _hip.require_gpu()
        x = X.to(torch.float32).contiguous() if on_dev else _hip.to_device(np.asarray(X, dtype=np.float32), torch.float32)
        with torch.cuda.device(x.device):
            y = self._transform_device(x, basis)
        return y if on_dev else _hip.to_host(y)

    def _transform_device(self, x: torch.Tensor, basis) -> torch.Tensor:
        dev = x.device
        xq = self._apply_preprocess(x)
        if basis is not None:
            b = basis.to(device=dev, dtype=torch.float32) if isinstance(basis, torch.Tensor) else \
                _hip.to_device(np.asarray(basis, dtype=np.float32), torch.float32)
            xb = self._apply_preprocess(b.contiguous())
        else:
            xb = self._x_dev.to(dev)
        yb = self._y_dev if self._y_dev is not None else \
            _hip.to_device(np.asarray(_hip.to_host(self.embedding_) if isinstance(self.embedding_, torch.Tensor)
                                      else self.embedding_, dtype=np.float32), torch.float32)
        yb = yb.to(dev).contiguous()
        r = x.shape[0]
        if r == 0:
            return torch.empty((0, self.n_components), dtype=torch.float32, device=dev)
        idx, dist = _hip.pacmap_knn(xq, xb, self.n_neighbors, exclude_self=False)
        nb, _, fp = _hip.pacmap_pairs(xq, xb, idx, dist, self.n_neighbors, 0, self.n_FP, self.seed_, True)
        per = self.n_neighbors + self.n_FP
        entries = torch.cat([_pack_entries(nb[:, 1], _hip.PACMAP_KIND_NB).reshape(r, -1),
                             _pack_entries(fp[:, 1], _hip.PACMAP_KIND_FP).reshape(r, -1)], dim=1).reshape(-1).contiguous()
        offsets = torch.arange(r + 1, dtype=torch.int64, device=dev) * per
        y0 = yb[idx[:, 0].long()].contiguous()
        return optimise(y0, y_part=yb, offsets=offsets, entries=entries, num_iters=self.num_iters, lr=self.lr)

    # ---- pairs, read back on first access -------------------------------------------------------------------------------------
    def _pairs(self, i: int, name: str):
        if name not in self._pairs_host:
            if self._pairs_dev is None:
                return None
            self._pairs_host[name] = _hip.to_host(self._pairs_dev[i])
        return self._pairs_host[name]

    @property
    def pair_neighbors(self):
        return self._pairs(0, "nb")

    @property
    def pair_MN(self):
        return self._pairs(1, "mn")

    @property
    def pair_FP(self):
        return self._pairs(2, "fp")

    def __getstate__(self):
        for i, name in enumerate(("nb", "mn", "fp")):
            self._pairs(i, name)
        state = dict(self.__dict__)
        for name in self._device_attrs:
            state[name] = None
        if isinstance(state.get("embedding_"), torch.Tensor):
            state["embedding_"] = _hip.to_host(state["embedding_"])
        return state


def optimise(y: torch.Tensor, y_part: Optional[torch.Tensor], offsets: torch.Tensor, entries: torch.Tensor, num_iters: int,
             lr: float, first_iter: int = 0) -> torch.Tensor:
    """``num_iters`` Adam iterations from ``first_iter`` (one ``runia_pacmap_step_f32`` launch each, ping-ponging two
    buffers); ``y_part`` None: the rows are their own partners (a fit), else the frozen partner rows (a transform)."""
    y = y.contiguous()
    buf = torch.empty_like(y)
    m = torch.zeros_like(y)
    v = torch.zeros_like(y)
    for t in range(first_iter, first_iter + num_iters):
        _hip.pacmap_step(y, y if y_part is None else y_part, buf, m, v, offsets, entries, t, lr)
        y, buf = buf, y
    return y


# ---- the reference's functions ---------------------------------------------------------------------------------------------
def fit_pacmap(samples_ind: np.ndarray, neighbors: int = 25, components: int = 2):
    """Fit PaCMAP (MN_ratio 0.5, FP_ratio 2, PCA init) -> ``(embedding of samples_ind, fitted estimator)``."""
    est = PaCMAP(n_components=components, n_neighbors=neighbors, MN_ratio=0.5, FP_ratio=2.0)
    return est.fit_transform(samples_ind, init="pca"), est


def apply_pacmap_transform(new_samples: np.ndarray, original_samples: np.ndarray, pm_instance: PaCMAP) -> np.ndarray:
    """Embed ``new_samples`` with a fitted estimator; ``original_samples`` are the rows it was fitted on."""
    return pm_instance.transform(X=new_samples, basis=original_samples)


def plot_samples_pacmap(samples_ind: np.ndarray, samples_ood: np.ndarray, neighbors: int = 25, components: int = 2,
                        title: str = "Plot Title", return_figure: bool = False):
    """Scatter of the InD rows (label 0) and OoD rows (label 1) embedded together by PaCMAP; returns the figure when
    ``return_figure``, else shows it."""
    import matplotlib.pyplot as plt

    rows = np.concatenate((samples_ind, samples_ood))
    labels = np.concatenate((np.zeros((len(samples_ind), 1)), np.ones((len(samples_ood), 1))))
    emb = PaCMAP(n_components=components, n_neighbors=neighbors, MN_ratio=0.5, FP_ratio=2.0).fit_transform(rows, init="pca")
    fig, ax = plt.subplots()
    points = ax.scatter(emb[:, 0], emb[:, 1], c=labels, cmap="brg", s=1.5)
    ax.set_title(title)
    ax.set_xlabel("PACMAP dimension 1")
    ax.set_ylabel("PACMAP dimension 2")
    ax.legend(handles=points.legend_elements()[0], labels=["In-Distribution", "Out-of-Distribution"])
    if return_figure:
        return fig
    plt.show()
