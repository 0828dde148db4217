"""Map a folder's windows in 2-D: principal components of the embeddings, fitted and projected on the device - and, from the
same projection, how far a window lies from everything the fit has seen.

    PCA                  ``partial_fit(rows)`` ... ``finish()``, ``fit(rows)``, ``transform(rows, residual=False)``
    fit_recordings       a folder of recordings (or an embedding store) -> PCAModel, streamed launch set by launch set
    project_recordings   a folder against a saved model -> MapResult, streamed
    map_recordings       fit and project a folder with one walk (its rows stay resident on the device) -> MapResult
    MapResult            ``coords``, ``residual``, ``to_csv``, ``outliers``, ``annotations``
    load                 the ``.npz`` ``PCAModel.save`` wrote -> PCAModel

A fit is three calls into ``include/buzzdetect_pca.h`` (csrc/pca.hip) per piece of at most 2^18 rows - squared norms (rows
with a NaN or an infinity are left out), column sums, and the 1024 x 1024 Gram matrix of the rows minus a fixed shift, on the
exact-f32 matrix instruction - and one read-back of the 4 MB matrix at the end, whose eigenvectors NumPy finds in float64.
A projection is one call: coordinates and the squared distance from the components' subspace.  The ``[W, 1024]`` rows stay
where they are.  Nothing is added atomically in floating point: the same rows in the same pieces give the same bits.

    from buzzdetect_amd import cluster, pca

    found = pca.map_recordings("audio_in", 2)
    found.to_csv("map.csv", clusters=cluster.cluster_recordings("audio_in", 24))     # ident,start,end,pc1,pc2,residual,cluster
    found.model.save("season.npz")

    new = pca.project_recordings("new_site", "season.npz")              # does the new site sound like the season?
    for ident, start, residual in new.outliers(20):
        print(ident, start, residual)
    new.annotations("review", 200, path="review.csv")                   # ident,start,end,label
"""
from __future__ import annotations

import csv
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .cluster import _result, _RowStore, _set_windows
from .dataset import FRAMELENGTH_S, _embed_parts, _open_engine, _torch
from .search import ANNOTATION_COLUMNS, _end, _walk, pack_queries

DIM = _lib.PCA_DIM
MAP_COLUMNS = ("ident", "start", "end")


# ---------------------------------------------------------------------------------------------------- host helpers
def _rows(e, name: str = "rows") -> np.ndarray:
    e = np.ascontiguousarray(e, np.float32)
    if e.ndim != 2 or e.shape[1] != DIM:
        raise ValueError(f"{name} must be [W, {DIM}], not {list(e.shape)}")
    return e


def _components(n_components) -> int:
    if not 1 <= int(n_components) <= _lib.PCA_MAX_COMPONENTS:
        raise ValueError(f"n_components must be in 1..{_lib.PCA_MAX_COMPONENTS}, not {n_components}")
    return int(n_components)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def _host_args(e, pick, n2, shift):
    e = _rows(e)
    pick = None if pick is None else np.ascontiguousarray(pick, np.int32)
    n2 = np.ascontiguousarray(n2, np.float32)
    if n2.shape != (e.shape[0],):
        raise ValueError("n2 must hold one squared norm per row of e")
    shift = None if shift is None else np.ascontiguousarray(shift, np.float32)
    if shift is not None and shift.shape != (DIM,):
        raise ValueError(f"shift must be [{DIM}]")
    return e, pick, n2, shift, (e.shape[0] if pick is None else pick.shape[0])


def sums_host(e, n2, shift=None, pick=None) -> np.ndarray:
    """``bd_pca_sums_host``: float32 [ceil(R / 256), 1024], the column sums of every slice in the device's order of operations."""
    e, pick, n2, shift, r = _host_args(e, pick, n2, shift)
    partial = np.zeros(((r + _lib.PCA_SUM_SLICE - 1) // _lib.PCA_SUM_SLICE, DIM), np.float32)
    _lib.check(_lib.load().bd_pca_sums_host(_ptr(e), max(e.shape[0], 1), _ptr(pick), r, _ptr(n2), _ptr(shift), _ptr(partial)))
    return partial


def gram_host(e, n2, shift=None, pick=None, into: Optional[np.ndarray] = None) -> np.ndarray:
    """``bd_pca_gram_host``: float32 [1024, 1024] in the device's order of operations; ``into``: a matrix to add to in place
    (``accumulate = 1``)."""
    e, pick, n2, shift, r = _host_args(e, pick, n2, shift)
    if into is not None and (into.dtype != np.float32 or into.shape != (DIM, DIM) or not into.flags.c_contiguous):
        raise ValueError(f"into must be a C-contiguous float32 [{DIM}, {DIM}] array")
    gram = np.zeros((DIM, DIM), np.float32) if into is None else into
    _lib.check(_lib.load().bd_pca_gram_host(_ptr(e), max(e.shape[0], 1), _ptr(pick), r, _ptr(n2), _ptr(shift),
                                            0 if into is None else 1, _ptr(gram)))
    return gram


def project_host(e, scores, mv, scale, mean, residual: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """``bd_pca_project_host``: (y float32 [W, d], resid float32 [W] or None) from the scores ``bd_search_scores`` stored."""
    e = _rows(e)
    scores = np.ascontiguousarray(scores, np.float32)
    mv, scale, mean = (np.ascontiguousarray(a, np.float32) for a in (mv, scale, mean))
    d = int(mv.shape[0])
    if scores.shape != (e.shape[0], d) or scale.shape != (d,) or mean.shape != (DIM,):
        raise ValueError("scores must be [W, d], mv and scale [d], mean [1024]")
    y = np.zeros((e.shape[0], d), np.float32)
    resid = np.zeros(e.shape[0], np.float32) if residual else None
    _lib.check(_lib.load().bd_pca_project_host(_ptr(e), e.shape[0], _ptr(scores), d, _ptr(mv), _ptr(scale), _ptr(mean), _ptr(y),
                                               _ptr(resid)))
    return y, resid


def sample_rows(w: int, fit_rows: Optional[int], seed: int = 0) -> Optional[np.ndarray]:
    """The rows ``PCA.fit(..., fit_rows, seed)`` fits: None for all of them, else ``fit_rows`` sorted ids drawn without
    repeats by ``numpy.random.default_rng(seed)``."""
    if fit_rows is None or int(fit_rows) >= int(w):
        return None
    if int(fit_rows) < 1:
        raise ValueError(f"fit_rows must be at least 1, not {fit_rows}")
    return np.sort(np.random.default_rng(int(seed)).choice(int(w), size=int(fit_rows), replace=False)).astype(np.int32)


def finish_host(gram, sums, n: int, shift, n_components: int):
    """The host's end of a fit, in float64: from the Gram matrix ``gram`` and the column sums ``sums`` of ``n`` rows minus
    ``shift``, C = (G - s s^T / n) / (n - 1), symmetrised, its ``n_components`` largest eigenpairs by ``numpy.linalg.eigh``,
    each component signed so that its entry of greatest magnitude (the first among equals) is positive.  Returns (components
    float64 [d, 1024], mean float64 [1024], explained_variance float64 [d], total_variance).  The formula is exact for every
    shift; one near the mean keeps it clear of the cancellation in G / n - m m^T."""
    d = _components(n_components)
    if int(n) < 2:
        raise ValueError(f"a covariance takes at least 2 rows, not {int(n)}")
    g, s = np.asarray(gram, np.float64), np.asarray(sums, np.float64)
    if g.shape != (DIM, DIM) or s.shape != (DIM,):
        raise ValueError(f"gram must be [{DIM}, {DIM}] and sums [{DIM}]")
    c = (g - np.outer(s, s) / float(n)) / float(int(n) - 1)
    c = 0.5 * (c + c.T)
    values, vectors = np.linalg.eigh(c)
    top = np.argsort(values, kind="stable")[::-1][:d]
    components = vectors[:, top].T.copy()
    for v in components:
        if v[int(np.argmax(np.abs(v)))] < 0:
            v *= -1.0
    mean = np.asarray(shift, np.float64) + s / float(n)
    return components, mean, values[top].copy(), float(np.trace(c))


# ---------------------------------------------------------------------------------------------------- the model
@dataclass
class PCAModel:
    """A fit as ``save`` writes it: what ``project_recordings`` and ``PCA.from_model`` take.  ``components`` float32 [d, 1024]
    (rows of unit length, strongest first), ``mean`` float32 [1024], ``explained_variance`` float64 [d] (the covariance's
    eigenvalues), ``total_variance`` (its trace), ``n_rows`` fitted, ``whiten``: whether coordinates are divided by the root
    of their variance."""
    components: np.ndarray
    mean: np.ndarray
    explained_variance: np.ndarray
    total_variance: float
    n_rows: int
    whiten: bool = False

    def __post_init__(self):
        self.components = _rows(self.components, "components")
        _components(self.components.shape[0])
        self.mean = np.ascontiguousarray(self.mean, np.float32)
        self.explained_variance = np.asarray(self.explained_variance, np.float64)
        self.total_variance, self.n_rows, self.whiten = float(self.total_variance), int(self.n_rows), bool(self.whiten)
        if self.mean.shape != (DIM,) or self.explained_variance.shape != (self.components.shape[0],):
            raise ValueError(f"mean must be [{DIM}] and explained_variance one value per component")

    @property
    def explained_variance_ratio(self) -> np.ndarray:
        return self.explained_variance / self.total_variance

    def constants(self) -> Tuple[np.ndarray, np.ndarray]:
        """(mv, scale) float32 [d] of ``bd_pca_project``: mv[j] = mean . v_j in float64, scale[j] = 1, or 1 / sqrt(variance j)
        when whitening (refused for a variance that is not positive)."""
        mv = (self.components.astype(np.float64) @ self.mean.astype(np.float64)).astype(np.float32)
        scale = np.ones(self.components.shape[0], np.float32)
        if self.whiten:
            if not np.all(self.explained_variance > 0):
                raise ValueError("whiten: a component's variance is not positive; fit fewer components")
            scale = (1.0 / np.sqrt(self.explained_variance)).astype(np.float32)
        return mv, scale

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            np.savez(f, components=self.components, mean=self.mean, explained_variance=self.explained_variance,
                     total_variance=np.float64(self.total_variance), n_rows=np.int64(self.n_rows), whiten=np.bool_(self.whiten))


def load(path: str) -> PCAModel:
    """The ``.npz`` of ``PCAModel.save``."""
    with np.load(path, allow_pickle=False) as z:
        return PCAModel(z["components"], z["mean"], z["explained_variance"], float(z["total_variance"]), int(z["n_rows"]),
                        bool(z["whiten"]))


class PCA:
    """Principal components of float32 [W, 1024] rows on the device.  ``partial_fit`` takes the rows piece by piece and
    ``finish`` ends the fit; ``fit`` is both.  After it: ``components`` float32 [d, 1024], ``mean`` float32 [1024],
    ``explained_variance`` and ``explained_variance_ratio`` float64 [d], ``total_variance``, ``n_rows`` (rows fitted) and
    ``n_skipped`` (rows left out because they hold a NaN or an infinity)."""

    def __init__(self, n_components: int = 2, whiten: bool = False, device=None):
        self.n_components, self.whiten = _components(n_components), bool(whiten)
        self._device_arg = device
        self.device = None
        self._lib = None
        self._model: Optional[PCAModel] = None
        self._consts = None
        self._reset()

    def _reset(self) -> None:
        self._shift = self._shift_dev = self._gram = self._workspace = None
        self._sums = np.zeros(DIM, np.float64)
        self.n_rows = self.n_skipped = 0
        self._started = False                                           # whether the Gram matrix holds a piece already

    @classmethod
    def from_model(cls, model: PCAModel, device=None) -> "PCA":
        """A saved fit, taken bit for bit, ready for ``transform``."""
        p = cls(model.components.shape[0], whiten=model.whiten, device=device)
        p._model, p.n_rows = model, model.n_rows
        return p

    def model(self) -> PCAModel:
        if self._model is None:
            raise RuntimeError("fit first")
        return self._model

    components = property(lambda self: self.model().components)
    mean = property(lambda self: self.model().mean)
    explained_variance = property(lambda self: self.model().explained_variance)
    explained_variance_ratio = property(lambda self: self.model().explained_variance_ratio)
    total_variance = property(lambda self: self.model().total_variance)

    # ------------------------------------------------------------------------------------------------ device plumbing
    def _empty(self, shape, dtype):
        """Every device buffer the kernels write comes from here (the tests put guard words around them)."""
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def _open(self, rows=None) -> None:
        torch = _torch()
        self._lib = _lib.load()
        if self.device is not None:
            return
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; the PCA has no CPU path")
        device = self._device_arg
        if device is None:
            device = rows.device if isinstance(rows, torch.Tensor) and rows.is_cuda else \
                torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)

    def _stream(self):
        return _torch().cuda.current_stream(self.device).cuda_stream

    def _check_rows(self, rows):
        torch = _torch()
        e = rows
        if not isinstance(e, torch.Tensor):
            e = torch.from_numpy(_rows(e)).to(self.device)
        if (e.dim() != 2 or e.shape[1] != DIM or e.dtype != torch.float32 or e.device != self.device or not e.is_contiguous()
                or e.data_ptr() % 16):
            raise ValueError(f"rows must be a contiguous, 16-byte aligned float32 [W, {DIM}] tensor on {self.device}")
        return e

    def _norms(self, e):
        torch = _torch()
        w = int(e.shape[0])
        n2 = self._empty((w,), torch.float32)
        with torch.cuda.device(self.device):
            for at in range(0, w, _lib.SEARCH_MAX_WINDOWS):
                n = min(_lib.SEARCH_MAX_WINDOWS, w - at)
                _lib.check(self._lib.bd_search_norms(e[at:at + n].data_ptr(), n, n2[at:at + n].data_ptr(), self._stream()))
        return n2

    def _column_sums(self, e, pick, r: int, n2, shift) -> np.ndarray:
        """float64 [1024]: the slices' partials of ``bd_pca_sums``, added on the host."""
        torch = _torch()
        partial = self._empty(((r + _lib.PCA_SUM_SLICE - 1) // _lib.PCA_SUM_SLICE, DIM), torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_pca_sums(e.data_ptr(), int(e.shape[0]), None if pick is None else pick.data_ptr(), r,
                                             n2.data_ptr(), None if shift is None else shift.data_ptr(), partial.data_ptr(),
                                             self._stream()))
        return partial.cpu().numpy().astype(np.float64).sum(axis=0)

    # ------------------------------------------------------------------------------------------------ fitting
    def _take(self, e, pick: Optional[np.ndarray]) -> None:
        """One ``partial_fit``: the rows of ``e`` (those of ``pick``, sorted ids, if given), in pieces of at most 2^18."""
        torch = _torch()
        r_all = int(e.shape[0]) if pick is None else int(pick.shape[0])
        if r_all == 0:
            return
        n2 = self._norms(e)
        pick_dev = None if pick is None else torch.from_numpy(np.ascontiguousarray(pick, np.int32)).to(self.device)
        taken = n2 if pick_dev is None else n2.index_select(0, pick_dev.long())
        present = int(torch.isfinite(taken).sum().item())
        pieces = [(at, min(_lib.PCA_MAX_ROWS, r_all - at)) for at in range(0, r_all, _lib.PCA_MAX_ROWS)]

        def piece(at, r):                                               # (rows, their pick, how many) as a call takes them
            if pick_dev is None:
                return e[at:at + r], None, r
            return e, pick_dev[at:at + r], r

        if self._shift is None:
            # the first call fixes the shift for the whole fit: the mean of its rows, as float32
            if present == 0:
                self.n_skipped += r_all
                return
            total = np.zeros(DIM, np.float64)
            for at, r in pieces:
                rows, pk, r = piece(at, r)
                total += self._column_sums(rows, pk, r, n2 if pk is not None else n2[at:at + r], None)
            self._shift = (total / present).astype(np.float32)
            self._shift_dev = torch.from_numpy(self._shift).to(self.device)
            self._gram = self._empty((DIM, DIM), torch.float32)
        for at, r in pieces:
            rows, pk, r = piece(at, r)
            n2_piece = n2 if pk is not None else n2[at:at + r]
            self._sums += self._column_sums(rows, pk, r, n2_piece, self._shift_dev)
            ws_bytes = _lib.check(self._lib.bd_pca_workspace_bytes(r))
            if self._workspace is None or self._workspace.numel() < ws_bytes:
                self._workspace = None                                  # (released before the larger one is asked for)
                self._workspace = self._empty((ws_bytes,), torch.uint8)
            with torch.cuda.device(self.device):
                _lib.check(self._lib.bd_pca_gram(rows.data_ptr(), int(rows.shape[0]), None if pk is None else pk.data_ptr(), r,
                                                 n2_piece.data_ptr(), self._shift_dev.data_ptr(), 1 if self._started else 0,
                                                 self._gram.data_ptr(), self._workspace.data_ptr(), ws_bytes, self._stream()))
            self._started = True
        self.n_rows += present
        self.n_skipped += r_all - present

    def partial_fit(self, rows) -> "PCA":
        """More rows of the fit: a device tensor or an array, float32 [W, 1024].  The first call that brings a usable row
        starts a new fit (and fixes the shift the Gram matrix is taken around)."""
        self._open(rows)
        if self._model is not None:                                     # a finished fit: this starts the next one
            self._model = self._consts = None
            self._reset()
        self._take(self._check_rows(rows), None)
        return self

    def finish(self) -> "PCA":
        """Ends the fit: one read-back of the Gram matrix, the eigenvectors in float64 on the host (``finish_host``)."""
        if self.n_rows < 2 or self._gram is None:
            raise ValueError(f"a covariance takes at least 2 rows, not {self.n_rows}")
        gram = self._gram.cpu().numpy()
        comps, mean, values, total = finish_host(gram, self._sums, self.n_rows, self._shift, self.n_components)
        self._model = PCAModel(comps.astype(np.float32), mean.astype(np.float32), values, total, self.n_rows, self.whiten)
        self._consts = None
        self._shift = self._shift_dev = self._gram = self._workspace = None
        return self

    def fit(self, rows, fit_rows: Optional[int] = None, seed: int = 0) -> "PCA":
        """Fits ``rows``; with ``fit_rows`` below their number, a seeded sample of that many (``sample_rows``), read where
        the rows lie."""
        self._open(rows)
        self._model = self._consts = None
        self._reset()
        e = self._check_rows(rows)
        self._take(e, sample_rows(int(e.shape[0]), fit_rows, seed))
        return self.finish()

    # ------------------------------------------------------------------------------------------------ projecting
    def transform(self, rows, residual: bool = False):
        """float32 [W, d] coordinates of ``rows`` on the components; with ``residual`` also float32 [W], each row's squared
        distance from the components' subspace through the mean.  A row with a NaN or an infinity gets NaN in both."""
        torch = _torch()
        model = self.model()
        self._open(rows)
        e = self._check_rows(rows)
        d = model.components.shape[0]
        if self._consts is None:
            mv, scale = model.constants()
            self._consts = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
                                 for a in (pack_queries(model.components), mv, scale, model.mean))
        packed, mv, scale, mean = self._consts
        w = int(e.shape[0])
        y = self._empty((w, d), torch.float32)
        resid = self._empty((w,), torch.float32) if residual else None
        with torch.cuda.device(self.device):
            for at in range(0, w, _lib.SEARCH_MAX_WINDOWS):
                n = min(_lib.SEARCH_MAX_WINDOWS, w - at)
                _lib.check(self._lib.bd_pca_project(e[at:at + n].data_ptr(), n, packed.data_ptr(), d, mv.data_ptr(),
                                                    scale.data_ptr(), mean.data_ptr(), y[at:at + n].data_ptr(),
                                                    None if resid is None else resid[at:at + n].data_ptr(), self._stream()))
        return (y.cpu().numpy(), resid.cpu().numpy()) if residual else y.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- results
@dataclass
class MapResult:
    """The windows of a folder on the map.  Window i lies in recording ``recordings[recording_of[i]]`` at ``starts[i]``
    (``analyze``'s start column for it), at ``coords[i]`` on the components of ``model``, ``residual[i]`` (a squared distance)
    away from their subspace."""
    coords: np.ndarray
    residual: np.ndarray
    recordings: List[str]
    recording_of: np.ndarray
    starts: np.ndarray
    model: Optional[PCAModel] = None
    messages: List[str] = field(default_factory=list)
    framelength_s: float = FRAMELENGTH_S
    clusters: Optional[object] = None

    def __post_init__(self):
        self.coords = np.asarray(self.coords, np.float32)
        self.residual = np.asarray(self.residual, np.float32)
        self.recording_of = np.asarray(self.recording_of, np.int64)
        self.starts = np.asarray(self.starts, np.float64)
        n = self.residual.shape[0]
        if self.coords.ndim != 2 or self.coords.shape[0] != n or not (self.recording_of.shape == self.starts.shape == (n,)):
            raise ValueError("coords must be [W, d]; residual, recording_of and starts must have one entry per window")

    def _window(self, i: int) -> Tuple[str, float]:
        return self.recordings[int(self.recording_of[i])], float(self.starts[i])

    def to_csv(self, path: str, clusters=None) -> None:
        """One row per window in the order of the walk: ``ident,start,end,pc1..pcd,residual`` (end = start + 0.96 s), and
        ``cluster`` behind them when ``clusters`` (or else ``self.clusters``) is the ``ClusterResult`` of the same walk."""
        n, d = self.coords.shape
        clusters = self.clusters if clusters is None else clusters
        if clusters is not None and np.asarray(clusters.labels).shape != (n,):
            raise ValueError(f"clusters holds {np.asarray(clusters.labels).shape[0]} windows, the map {n}: not the same walk")
        with open(path, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(list(MAP_COLUMNS) + [f"pc{j + 1}" for j in range(d)] + ["residual"] + (["cluster"] if clusters is not None else []))
            for i in range(n):
                ident, start = self._window(i)
                out.writerow([ident, repr(start), repr(_end(start, self.framelength_s))] + [repr(float(v)) for v in self.coords[i]]
                             + [repr(float(self.residual[i]))] + ([int(clusters.labels[i])] if clusters is not None else []))

    def _farthest(self, n: int) -> np.ndarray:
        r = self.residual.astype(np.float64)
        key = np.where(np.isnan(r), np.inf, -r)                         # greatest first, NaN last
        return np.lexsort((np.arange(r.shape[0]), key))[:max(int(n), 0)]

    def outliers(self, n: int = 20) -> List[Tuple[str, float, float]]:
        """The ``n`` windows of greatest residual as (ident, start, residual), greatest first; among equal residuals the
        window that comes first in the walk; windows without one (NaN) last."""
        return [(*self._window(i), float(self.residual[i])) for i in self._farthest(n)]

    def annotations(self, label: str, n: int = 20, path: Optional[str] = None) -> List[Tuple[str, float, float, str]]:
        """Those windows as annotation rows (ident, start, end, label), in the order of ``outliers``.  ``path``: also written
        there, in the format ``dataset.read_annotations`` reads."""
        rows = []
        for i in self._farthest(n):
            ident, start = self._window(i)
            rows.append((ident, start, _end(start, self.framelength_s), str(label)))
        if path is not None:
            with open(path, "w", newline="") as f:
                out = csv.writer(f)
                out.writerow(ANNOTATION_COLUMNS)
                for ident, start, end, lab in rows:
                    out.writerow([ident, repr(start), repr(end), lab])
        return rows


def _map_result(index, coords, residual, model, messages) -> MapResult:
    """Per-window recording and start exactly as ``cluster._result`` builds them (through it, with no clusters)."""
    w = int(np.asarray(residual).shape[0])
    places = _result(index, np.zeros(w, np.int32), np.zeros(w, np.float32), np.array([w]), None, "cosine", [])
    return MapResult(coords, residual, places.recordings, places.recording_of, places.starts, model, list(messages))


def _as_model(model) -> PCAModel:
    if isinstance(model, str):
        return load(model)
    if isinstance(model, PCA):
        return model.model()
    return model


def fit_recordings(dir_audio: str, n_components: int = 2, *, engine=None, framehop_prop: float = 1.0, chunklength: float = 200,
                   embeddername: str = "yamnet_k2", whiten: bool = False) -> PCAModel:
    """The principal components of the windows under ``dir_audio`` (a folder of recordings or an embedding store).  Every
    recording ``analyze`` would take is read, resampled and embedded as ``analyze(framehop_prop=..., chunklength=...)`` does
    it; each launch set's rows go to ``PCA.partial_fit`` and are dropped: no residency, no ``max_windows``."""
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        p = PCA(n_components, whiten=whiten, device=engine.device)
        seen = [0]

        def feed(parts, hop, step):
            emb, counts = _embed_parts(engine, parts, hop, step)
            p.partial_fit(emb)
            first, seen[0] = seen[0], seen[0] + int(emb.shape[0])
            return first, counts

        _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed)
        return p.finish().model()
    finally:
        if own:
            engine.close()


def project_recordings(dir_audio: str, model, *, engine=None, framehop_prop: float = 1.0, chunklength: float = 200,
                       embeddername: str = "yamnet_k2") -> MapResult:
    """The windows under ``dir_audio`` on a saved map (``model``: a ``PCAModel``, a fitted ``PCA`` or the path of a ``save``).
    Each launch set's rows are projected and dropped."""
    model = _as_model(model)
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        p = PCA.from_model(model, device=engine.device)
        coords, residual, seen = [], [], [0]

        def feed(parts, hop, step):
            emb, counts = _embed_parts(engine, parts, hop, step)
            y, r = p.transform(emb, residual=True)
            coords.append(y)
            residual.append(r)
            first, seen[0] = seen[0], seen[0] + int(emb.shape[0])
            return first, counts

        index = _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed)
        y = np.concatenate(coords) if coords else np.zeros((0, model.components.shape[0]), np.float32)
        r = np.concatenate(residual) if residual else np.zeros(0, np.float32)
        return _map_result(index, y, r, model, messages)
    finally:
        if own:
            engine.close()


def map_recordings(dir_audio: str, n_components: int = 2, *, fit_rows: Optional[int] = 262144, seed: int = 0,
                   max_windows: int = 1 << 22, clusters=None, engine=None, framehop_prop: float = 1.0, chunklength: float = 200,
                   embeddername: str = "yamnet_k2", whiten: bool = False) -> MapResult:
    """Fit and project the windows under ``dir_audio`` with one walk: the rows are gathered in a device buffer of 4 KB per
    window as ``cluster.cluster_recordings`` gathers them (more than ``max_windows`` windows are refused the same way),
    ``PCA(n_components).fit(rows, fit_rows, seed)`` fits a seeded sample of at most ``fit_rows`` of them where they lie, and
    ``transform`` places every one.  ``clusters``: the ``ClusterResult`` of the same walk (``cluster.cluster_recordings`` with
    the same folder and framing), kept on the result so that ``to_csv`` writes a label per window; one of another length is
    refused."""
    _components(n_components)
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        store = _RowStore(engine.device, max_windows)

        def feed(parts, hop, step):
            first = store.reserve(_set_windows(engine, parts, hop, step))
            emb, counts = _embed_parts(engine, parts, hop, step)
            store.put(first, emb)
            return first, counts

        index = _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed)
        p = PCA(n_components, whiten=whiten, device=engine.device).fit(store.rows(), fit_rows=fit_rows, seed=seed)
        y, r = p.transform(store.rows(), residual=True)
        found = _map_result(index, y, r, p.model(), messages)
        if clusters is not None:
            if np.asarray(clusters.labels).shape != (found.residual.shape[0],):
                raise ValueError(f"clusters holds {np.asarray(clusters.labels).shape[0]} windows, the folder "
                                 f"{found.residual.shape[0]}: not the same walk")
            found.clusters = clusters
        return found
    finally:
        if own:
            engine.close()
