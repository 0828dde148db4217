"""Spread a few labels over a folder: the k-nearest-neighbour graph of its windows and label propagation along it, on the
device - the step between ``search`` (which windows sound like these few) and ``train`` (hundreds of labels per class).

    neighbour_graph        a folder or an embedding store -> KnnGraph (``ids``, ``sims`` and the window index)
    KnnGraph               ``neighbours``, ``duplicates``, ``symmetrised``, ``save`` / ``load``
    Propagator             ``fit(graph, targets, alpha)``: the steps on device tensors, as ``KMeans`` is for ``cluster``
    propagate_recordings   a folder, annotations, classes -> PropagationResult
    PropagationResult      ``labels``, ``confidence``, ``margin``, ``reach``, ``scores``, ``to_csv``, ``annotations``
    holdout_accuracy       hide a share of the labels, propagate, compare: whether to trust the output

The lists come from ``include/buzzdetect_knn.h`` (csrc/knn.hip): an all-pairs product on the matrix cores with a selection per
row, no [W, W] matrix anywhere.  The steps and the read-out are ``include/buzzdetect_propagate.h`` (csrc/propagate.hip).  Every
result is reproducible bit for bit, and every kernel has a host restatement with the same bits (the ``*_host`` functions here).

    from buzzdetect_amd import dataset, propagate

    spread = propagate.propagate_recordings("audio_in", "reviewed.csv", ["ambient", "ins_buzz"])
    spread.to_csv("propagated.csv")                                     # ident,start,end,label,confidence,margin,reach
    spread.annotations(min_confidence=0.9, min_reach=0.5, path="more.csv")      # what dataset.read_annotations takes back
    ts = dataset.embed_annotated("audio_in", "more.csv", ["ambient", "ins_buzz"])
"""
from __future__ import annotations

import csv
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, framing
from .cluster import _RowStore, _set_windows
from .dataset import DIGITS_TIME, FRAMELENGTH_S, _as_annotations, _embed_parts, _label_at, _open_engine, _torch
from .search import ANNOTATION_COLUMNS, _end, _walk, norms_host

DIM = _lib.KNN_DIM
PROPAGATION_COLUMNS = ("ident", "start", "end", "label", "confidence", "margin", "reach")


# ---------------------------------------------------------------------------------------------------- host restatements
def _metric(metric: str) -> int:
    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.KNN_METRICS)}, not {metric!r}")
    return _lib.KNN_METRICS[metric]


def _rows(e, name: str = "rows") -> np.ndarray:
    e = np.ascontiguousarray(e, np.float32)
    if e.ndim != 2 or e.shape[1] != DIM:
        raise ValueError(f"{name} must be [W, {DIM}], not {list(e.shape)}")
    return e


def knn_update_host(keys: np.ndarray, queries, candidates, *, metric: str = "cosine", exclude_self: bool = False,
                    q_base_id: int = 0, c_base_id: int = 0) -> np.ndarray:
    """``bd_knn_update_host`` in place on ``keys`` (uint64 [Wq, k], C order); the squared norms are ``search.norms_host``."""
    if keys.dtype != np.uint64 or keys.ndim != 2 or not keys.flags.c_contiguous:
        raise ValueError("keys must be a C-contiguous uint64 [Wq, k] array")
    q, c = _rows(queries, "queries"), _rows(candidates, "candidates")
    if q.shape[0] != keys.shape[0]:
        raise ValueError(f"{keys.shape[0]} rows of keys for {q.shape[0]} queries")
    n2_q, n2_c = norms_host(q), norms_host(c)
    _lib.check(_lib.load().bd_knn_update_host(q.ctypes.data, q.shape[0], n2_q.ctypes.data, int(q_base_id), c.ctypes.data, c.shape[0],
                                              n2_c.ctypes.data, int(c_base_id), _metric(metric), int(bool(exclude_self)),
                                              keys.ctypes.data, keys.shape[1]))
    return keys


def decode_keys(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_knn_decode_host``: (ids int32, sims float32) in the shape of ``keys``; an empty slot reads (-1, 0.0)."""
    keys = np.ascontiguousarray(keys, np.uint64)
    ids, sims = np.zeros(keys.shape, np.int32), np.zeros(keys.shape, np.float32)
    _lib.check(_lib.load().bd_knn_decode_host(keys.ctypes.data, keys.size, ids.ctypes.data, sims.ctypes.data))
    return ids, sims


def weights_host(ids: np.ndarray, sims: np.ndarray, power: int) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_propagate_weights_host``: lists [N, k] -> (nbr int32 [N, k], w float32 [N, k])."""
    ids, sims = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(sims, np.float32)
    if ids.ndim != 2 or ids.shape != sims.shape:
        raise ValueError("ids and sims must be [N, k]")
    nbr, w = np.zeros(ids.shape, np.int32), np.zeros(ids.shape, np.float32)
    _lib.check(_lib.load().bd_propagate_weights_host(ids.ctypes.data, sims.ctypes.data, ids.shape[0], ids.shape[1], int(power),
                                                     nbr.ctypes.data, w.ctypes.data))
    return nbr, w


def step_host(row_start, nbr, w, f_in, y, alpha) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_propagate_step_host``: (F_out float32 [N, C], delta float32 [slices of 256 rows])."""
    row_start = np.ascontiguousarray(row_start, np.int64)
    nbr, w = np.ascontiguousarray(nbr, np.int32).reshape(-1), np.ascontiguousarray(w, np.float32).reshape(-1)
    f_in, y, alpha = np.ascontiguousarray(f_in, np.float32), np.ascontiguousarray(y, np.float32), np.ascontiguousarray(alpha, np.float32)
    n = row_start.shape[0] - 1
    if f_in.ndim != 2 or f_in.shape != y.shape or f_in.shape[0] != n or alpha.shape != (n,) or nbr.shape != w.shape:
        raise ValueError("row_start must be [N + 1], nbr and w [E], f_in and y [N, C], alpha [N]")
    f_out = np.zeros_like(f_in)
    delta = np.zeros((n + _lib.PROPAGATE_SLICE - 1) // _lib.PROPAGATE_SLICE, np.float32)
    _lib.check(_lib.load().bd_propagate_step_host(row_start.ctypes.data, nbr.ctypes.data, w.ctypes.data, n, nbr.shape[0],
                                                  f_in.ctypes.data, y.ctypes.data, alpha.ctypes.data, f_in.shape[1],
                                                  f_out.ctypes.data, delta.ctypes.data))
    return f_out, delta


def readout_host(f) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``bd_propagate_readout_host``: (reach float32, label int32, confidence float32, margin float32), each [N]."""
    f = np.ascontiguousarray(f, np.float32)
    if f.ndim != 2:
        raise ValueError("f must be [N, C]")
    n = f.shape[0]
    reach, label = np.zeros(n, np.float32), np.zeros(n, np.int32)
    confidence, margin = np.zeros(n, np.float32), np.zeros(n, np.float32)
    _lib.check(_lib.load().bd_propagate_readout_host(f.ctypes.data, n, f.shape[1], reach.ctypes.data, label.ctypes.data,
                                                     confidence.ctypes.data, margin.ctypes.data))
    return reach, label, confidence, margin


# ---------------------------------------------------------------------------------------------------- graphs on the host
@dataclass
class CsrGraph:
    """Edges in CSR form: row i's neighbours are ``nbr[row_start[i]:row_start[i + 1]]`` with similarities ``sims`` there."""
    row_start: np.ndarray
    nbr: np.ndarray
    sims: np.ndarray

    def __post_init__(self):
        self.row_start = np.ascontiguousarray(self.row_start, np.int64)
        self.nbr = np.ascontiguousarray(self.nbr, np.int32)
        self.sims = np.ascontiguousarray(self.sims, np.float32)
        if self.row_start.ndim != 1 or self.row_start.shape[0] < 1 or self.nbr.shape != self.sims.shape or self.nbr.ndim != 1:
            raise ValueError("row_start must be [N + 1], nbr and sims [E]")
        if self.row_start[0] != 0 or self.row_start[-1] != self.nbr.shape[0] or (np.diff(self.row_start) < 0).any():
            raise ValueError("row_start must ascend from 0 to the number of edges")

    @property
    def n_rows(self) -> int:
        return int(self.row_start.shape[0] - 1)

    def symmetrised(self) -> "CsrGraph":
        """The union of the edges and their reverses.  The two directions of an edge carry the same bits (the similarities are
        bit-symmetric), so a pair is kept once per direction; should they differ, the larger is kept.  Each row's edges are
        ordered by descending similarity, then ascending id.  Built on the host."""
        n = self.n_rows
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.row_start))
        dst = self.nbr.astype(np.int64)
        i, j, s = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([self.sims, self.sims])
        order = np.lexsort((-s.astype(np.float64), j, i))               # per (i, j) the larger similarity first
        i, j, s = i[order], j[order], s[order]
        first = np.ones(i.shape[0], bool)
        first[1:] = (i[1:] != i[:-1]) | (j[1:] != j[:-1])
        i, j, s = i[first], j[first], s[first]
        order = np.lexsort((j, -s.astype(np.float64), i))
        row_start = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(i, minlength=n), out=row_start[1:])
        return CsrGraph(row_start, j[order].astype(np.int32), s[order])


def lists_csr(ids: np.ndarray, sims: np.ndarray) -> CsrGraph:
    """Fixed-k lists [N, k] as CSR, empty slots (id -1) left out."""
    ids, sims = np.asarray(ids, np.int32), np.asarray(sims, np.float32)
    real = ids >= 0
    row_start = np.zeros(ids.shape[0] + 1, np.int64)
    np.cumsum(real.sum(axis=1), out=row_start[1:])
    return CsrGraph(row_start, ids[real], sims[real])


@dataclass
class KnnGraph:
    """The k nearest neighbours of every window.  Window i lies in recording ``recordings[recording_of[i]]`` at ``starts[i]``
    (``analyze``'s start column for it); ``ids[i]`` are its neighbours' window numbers, best first, ``sims[i]`` their
    similarities; an empty slot (fewer than k other windows) is id -1 with similarity 0."""
    ids: np.ndarray
    sims: np.ndarray
    recordings: List[str]
    recording_of: np.ndarray
    starts: np.ndarray
    metric: str = "cosine"
    messages: List[str] = field(default_factory=list)
    framelength_s: float = FRAMELENGTH_S

    def __post_init__(self):
        self.ids = np.ascontiguousarray(self.ids, np.int32)
        self.sims = np.ascontiguousarray(self.sims, np.float32)
        self.recording_of = np.asarray(self.recording_of, np.int64)
        self.starts = np.asarray(self.starts, np.float64)
        n = self.ids.shape[0]
        if self.ids.ndim != 2 or self.ids.shape != self.sims.shape or not (self.recording_of.shape == self.starts.shape == (n,)):
            raise ValueError("ids and sims must be [N, k], recording_of and starts [N]")

    @property
    def k(self) -> int:
        return int(self.ids.shape[1])

    def window(self, i: int) -> Tuple[str, float]:
        return self.recordings[int(self.recording_of[i])], float(self.starts[i])

    def row_of(self, ident: str, start: float) -> int:
        """The number of the window of ``ident`` that starts at ``start`` (``KeyError`` when there is none)."""
        if ident in self.recordings:
            r = self.recordings.index(ident)
            hit = np.flatnonzero((self.recording_of == r) & (np.abs(self.starts - float(start)) < 0.5 * 10.0 ** -DIGITS_TIME))
            if hit.size:
                return int(hit[0])
        raise KeyError(f"no window of {ident!r} starts at {start}")

    def neighbours(self, ident: str, start: float) -> List[Tuple[str, float, float]]:
        """The neighbours of one window as (ident, start, similarity), best first."""
        i = self.row_of(ident, start)
        return [(*self.window(j), float(s)) for j, s in zip(self.ids[i], self.sims[i]) if j >= 0]

    def duplicates(self, min_similarity: float = 0.999) -> List[Tuple[Tuple[str, float], Tuple[str, float], float]]:
        """Pairs of windows at least ``min_similarity`` alike, each pair once (the earlier window first), best first."""
        i, s = np.nonzero((self.ids >= 0) & (self.sims >= min_similarity))
        j = self.ids[i, s].astype(np.int64)
        a, b = np.minimum(i, j), np.maximum(i, j)
        pairs: Dict[Tuple[int, int], float] = {}
        for x, y, v in zip(a, b, self.sims[i, s]):
            pairs[(int(x), int(y))] = max(float(v), pairs.get((int(x), int(y)), -np.inf))
        ordered = sorted(pairs.items(), key=lambda item: (-item[1], item[0]))
        return [(self.window(x), self.window(y), v) for (x, y), v in ordered]

    def csr(self) -> CsrGraph:
        return lists_csr(self.ids, self.sims)

    def symmetrised(self) -> CsrGraph:
        """``CsrGraph.symmetrised`` of the lists: every edge with its reverse."""
        return self.csr().symmetrised()

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            np.savez(f, ids=self.ids, sims=self.sims, recordings=np.array(self.recordings, dtype=str),
                     recording_of=self.recording_of, starts=self.starts, metric=np.array(self.metric),
                     framelength_s=np.float64(self.framelength_s))

    @classmethod
    def load(cls, path: str) -> "KnnGraph":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["ids"], z["sims"], [str(r) for r in z["recordings"]], z["recording_of"], z["starts"], str(z["metric"]),
                       [], float(z["framelength_s"]))


# ---------------------------------------------------------------------------------------------------- device plumbing
class _Device:
    """What ``Neighbours`` and ``Propagator`` share: the library, the device, and where their buffers come from."""

    def __init__(self, device=None):
        self._device_arg = device
        self.device = None
        self._lib = None

    def _empty(self, shape, dtype):
        """Every device buffer the kernels write comes from here (the tests put guard words around them)."""
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def _open(self, like=None) -> None:
        torch = _torch()
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; the neighbour graph and propagation have no CPU path")
        device = self._device_arg
        if device is None:
            device = like.device if isinstance(like, torch.Tensor) and like.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)

    def _stream(self):
        return _torch().cuda.current_stream(self.device).cuda_stream

    def _tensor(self, array, dtype):
        torch = _torch()
        if isinstance(array, torch.Tensor):
            return array.to(device=self.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(array)).to(device=self.device, dtype=dtype).contiguous()


class Neighbours(_Device):
    """The k best candidates of every query row on the device.  ``update(queries, candidates)`` may be called any number of
    times with disjoint candidate id ranges; ``lists()`` reads the state back."""

    def __init__(self, k: int = 16, metric: str = "cosine", exclude_self: bool = True, device=None):
        super().__init__(device)
        if not 1 <= int(k) <= _lib.KNN_MAX_K:
            raise ValueError(f"k must be in 1..{_lib.KNN_MAX_K}, not {k}")
        self.k, self.metric, self._metric_id, self.exclude_self = int(k), metric, _metric(metric), bool(exclude_self)
        self.keys = None

    def _check_rows(self, e, name: str):
        torch = _torch()
        if not isinstance(e, torch.Tensor):
            e = torch.from_numpy(_rows(e, name)).to(self.device)
        if (e.dim() != 2 or e.shape[1] != DIM or e.dtype != torch.float32 or e.device != self.device or not e.is_contiguous()
                or e.data_ptr() % 16):
            raise ValueError(f"{name} must be a contiguous, 16-byte aligned float32 [W, {DIM}] tensor on {self.device}")
        return e

    def _norms(self, e):
        torch = _torch()
        w = int(e.shape[0])
        n2 = self._empty((w,), torch.float32)
        with torch.cuda.device(self.device):
            for at in range(0, w, _lib.SEARCH_MAX_WINDOWS):              # bd_search_norms takes 2^20 rows a call
                n = min(_lib.SEARCH_MAX_WINDOWS, w - at)
                _lib.check(self._lib.bd_search_norms(e[at:at + n].data_ptr(), n, n2[at:at + n].data_ptr(), self._stream()))
        return n2

    def update(self, queries, candidates=None, q_base_id: int = 0, c_base_id: int = 0) -> "Neighbours":
        """``candidates`` None: the queries against themselves (the graph of a folder)."""
        torch = _torch()
        if self.device is None:
            self._open(queries)
        q = self._check_rows(queries, "queries")
        c = q if candidates is None else self._check_rows(candidates, "candidates")
        wq, wc = int(q.shape[0]), int(c.shape[0])
        if self.keys is None:
            self.keys = self._empty((wq, self.k), torch.int64)
            self.keys.zero_()
        if self.keys.shape[0] != wq:
            raise ValueError(f"the state holds {self.keys.shape[0]} query rows, not {wq}")
        n2_q = self._norms(q)
        n2_c = n2_q if c is q else self._norms(c)
        step = _lib.KNN_MAX_ROWS
        with torch.cuda.device(self.device):
            for qa in range(0, wq, step):
                nq = min(step, wq - qa)
                for ca in range(0, wc, step):
                    nc = min(step, wc - ca)
                    nbytes = _lib.check(self._lib.bd_knn_workspace_bytes(nq, nc))
                    ws = self._empty((max(nbytes, 16),), torch.uint8)
                    _lib.check(self._lib.bd_knn_update(q[qa:qa + nq].data_ptr(), nq, n2_q[qa:qa + nq].data_ptr(), q_base_id + qa,
                                                       c[ca:ca + nc].data_ptr(), nc, n2_c[ca:ca + nc].data_ptr(), c_base_id + ca,
                                                       self._metric_id, int(self.exclude_self), self.keys[qa:qa + nq].data_ptr(),
                                                       self.k, ws.data_ptr(), nbytes, self._stream()))
        return self

    def lists(self) -> Tuple[np.ndarray, np.ndarray]:
        """(ids int32 [Wq, k], sims float32 [Wq, k]), best first; an empty slot is (-1, 0.0)."""
        if self.keys is None:
            raise RuntimeError("update first")
        return decode_keys(self.keys.cpu().numpy().view(np.uint64))


class Propagator(_Device):
    """Label propagation along a graph on the device.  ``fit(graph, targets, alpha)``: ``graph`` is a ``CsrGraph`` or lists
    ``(ids, sims)`` [N, k] (a directed graph); ``targets`` float32 [N, C] holds a labelled row's classes (one 1.0) and zeros
    elsewhere; ``alpha`` float32 [N] is 0 for a row clamped to its label, 1 for an unlabelled row, between for a soft clamp.
    An edge weighs max(similarity, 0) ** ``power``.  F starts as the targets; a step makes every row
    alpha x (the weighted mean of its neighbours) + (1 - alpha) x its target.  The steps end when no element moved by more
    than ``tol``, or at ``max_iter``.

    After ``fit``: ``scores`` float32 [N, C], ``reach`` (the sum over the classes: 0 for a window no label flowed to),
    ``labels`` int32 (-1 where reach is 0), ``confidence`` = top / reach, ``margin`` = (top - second) / reach, ``iterations``,
    ``delta_history``."""

    def __init__(self, power: int = 4, max_iter: int = 50, tol: float = 1e-4, device=None):
        super().__init__(device)
        if not 1 <= int(power) <= _lib.PROPAGATE_MAX_POWER:
            raise ValueError(f"power must be in 1..{_lib.PROPAGATE_MAX_POWER}, not {power}")
        if int(max_iter) < 1 or not float(tol) >= 0:
            raise ValueError("max_iter must be at least 1 and tol at least 0")
        self.power, self.max_iter, self.tol = int(power), int(max_iter), float(tol)
        self.scores = self.reach = self.labels = self.confidence = self.margin = None
        self.iterations = 0
        self.delta_history: List[float] = []

    def _graph(self, graph):
        """(row_start, nbr, w) on the device from a CsrGraph or from lists (ids, sims)."""
        torch = _torch()
        if isinstance(graph, CsrGraph):
            ids, sims, k = graph.nbr.reshape(-1, 1), graph.sims.reshape(-1, 1), 1
            row_start = graph.row_start
        else:
            ids, sims = (np.ascontiguousarray(a) for a in graph)
            if ids.ndim != 2 or ids.shape != sims.shape:
                raise ValueError("lists must be (ids [N, k], sims [N, k])")
            k = int(ids.shape[1])
            row_start = np.arange(ids.shape[0] + 1, dtype=np.int64) * k
        ids_dev, sims_dev = self._tensor(ids, torch.int32), self._tensor(sims, torch.float32)
        nbr, w = self._empty(tuple(ids.shape), torch.int32), self._empty(tuple(ids.shape), torch.float32)
        if ids.size:
            with torch.cuda.device(self.device):
                _lib.check(self._lib.bd_propagate_weights(ids_dev.data_ptr(), sims_dev.data_ptr(), int(ids.shape[0]), k, self.power,
                                                          nbr.data_ptr(), w.data_ptr(), self._stream()))
        return self._tensor(row_start, torch.int64), nbr, w

    def fit(self, graph, targets, alpha) -> "Propagator":
        torch = _torch()
        self._open(targets)
        y = self._tensor(targets, torch.float32)
        a = self._tensor(alpha, torch.float32)
        if y.dim() != 2 or not 1 <= y.shape[1] <= _lib.PROPAGATE_MAX_CLASSES or a.shape != (y.shape[0],):
            raise ValueError(f"targets must be [N, 1..{_lib.PROPAGATE_MAX_CLASSES}] and alpha [N]")
        n, c = int(y.shape[0]), int(y.shape[1])
        row_start, nbr, w = self._graph(graph)
        if row_start.shape[0] != n + 1:
            raise ValueError(f"the graph has {row_start.shape[0] - 1} rows, the targets {n}")
        edges = int(nbr.numel())
        slices = (n + _lib.PROPAGATE_SLICE - 1) // _lib.PROPAGATE_SLICE
        f = [self._empty((n, c), torch.float32), self._empty((n, c), torch.float32)]
        f[0].copy_(y)
        delta = self._empty((slices,), torch.float32)
        self.delta_history = []
        cur = 0
        with torch.cuda.device(self.device):
            for _ in range(self.max_iter if n else 0):
                _lib.check(self._lib.bd_propagate_step(row_start.data_ptr(), nbr.data_ptr(), w.data_ptr(), n, edges,
                                                       f[cur].data_ptr(), y.data_ptr(), a.data_ptr(), c, f[cur ^ 1].data_ptr(),
                                                       delta.data_ptr(), self._stream()))
                cur ^= 1
                self.delta_history.append(float(delta.max().item()))   # the step's one read-back
                if self.delta_history[-1] <= self.tol:
                    break
            reach, label = self._empty((n,), torch.float32), self._empty((n,), torch.int32)
            confidence, margin = self._empty((n,), torch.float32), self._empty((n,), torch.float32)
            if n:
                _lib.check(self._lib.bd_propagate_readout(f[cur].data_ptr(), n, c, reach.data_ptr(), label.data_ptr(),
                                                          confidence.data_ptr(), margin.data_ptr(), self._stream()))
        self.iterations = len(self.delta_history)
        self.scores = f[cur].cpu().numpy()
        self.reach, self.labels = reach.cpu().numpy(), label.cpu().numpy()
        self.confidence, self.margin = confidence.cpu().numpy(), margin.cpu().numpy()
        return self


def targets_of(labelled_rows, labels, n_rows: int, n_classes: int, clamp: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """(targets float32 [N, C], alpha float32 [N]) for rows ``labelled_rows`` of classes ``labels``: a labelled row's target is
    its class and its alpha is 1 - ``clamp``; every other row has no target and alpha 1."""
    if not 0.0 < float(clamp) <= 1.0:
        raise ValueError("clamp must be in (0, 1]")
    rows, labels = np.asarray(labelled_rows, np.int64), np.asarray(labels, np.int64)
    if rows.shape != labels.shape or rows.ndim != 1:
        raise ValueError("labelled_rows and labels must be [L]")
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows or labels.min() < 0 or labels.max() >= n_classes):
        raise ValueError("a labelled row or a label is out of range")
    y = np.zeros((int(n_rows), int(n_classes)), np.float32)
    alpha = np.ones(int(n_rows), np.float32)
    y[rows, labels] = 1.0
    alpha[rows] = np.float32(1.0) - np.float32(clamp)
    return y, alpha


def holdout_accuracy(graph, labelled_rows, labels, classes: Sequence[str], fraction: float = 0.2, seed: int = 0, repeats: int = 5,
                     clamp: float = 1.0, **propagator_options) -> Dict[str, object]:
    """Whether to trust the output: ``repeats`` times a seeded ``fraction`` of the labelled rows is hidden, the rest is
    propagated along ``graph`` (a ``CsrGraph`` or lists), and the hidden rows are compared.  Returns ``accuracy`` (of the
    hidden rows a label reached), ``coverage`` (the share a label reached), both overall and per class (``per_class``:
    name -> (accuracy, coverage, hidden rows)), summed over the repeats.  The same kernels as ``Propagator``."""
    rows, labels = np.asarray(labelled_rows, np.int64), np.asarray(labels, np.int64)
    if not 0.0 < float(fraction) < 1.0 or int(repeats) < 1:
        raise ValueError("fraction must be in (0, 1) and repeats at least 1")
    n = graph.n_rows if isinstance(graph, CsrGraph) else int(np.asarray(graph[0]).shape[0])
    c = len(classes)
    hidden_n, reached_n, right_n = np.zeros(c, np.int64), np.zeros(c, np.int64), np.zeros(c, np.int64)
    rng = np.random.default_rng(seed)
    for _ in range(int(repeats)):
        hide = np.zeros(rows.shape[0], bool)
        hide[rng.permutation(rows.shape[0])[:max(1, int(round(fraction * rows.shape[0])))]] = True
        y, alpha = targets_of(rows[~hide], labels[~hide], n, c, clamp)
        got = Propagator(**propagator_options).fit(graph, y, alpha).labels[rows[hide]]
        truth = labels[hide]
        hidden_n += np.bincount(truth, minlength=c)
        reached_n += np.bincount(truth[got >= 0], minlength=c)
        right_n += np.bincount(truth[got == truth], minlength=c)
    ratio = lambda a, b: float(a) / float(b) if b else float("nan")
    return {"accuracy": ratio(right_n.sum(), reached_n.sum()), "coverage": ratio(reached_n.sum(), hidden_n.sum()),
            "per_class": {str(name): (ratio(right_n[j], reached_n[j]), ratio(reached_n[j], hidden_n[j]), int(hidden_n[j]))
                          for j, name in enumerate(classes)}}


# ---------------------------------------------------------------------------------------------------- recordings
def _index_arrays(index) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``search._Index`` -> per window: its recording, its ``analyze`` start, and its exact start (what the labels go by)."""
    recording_of, starts, exact = [], [], []
    for r, (_, starts_s, counts) in enumerate(index.chunks):
        for start_s, n in zip(starts_s, counts):
            starts.append(np.asarray(framing.window_starts(n, start_s, index.framehop_s, DIGITS_TIME), np.float64).reshape(-1))
            exact.append(start_s + np.arange(int(n), dtype=np.float64) * index.framehop_s)
            recording_of.append(np.full(int(n), r, np.int64))
    cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype)
    return cat(recording_of, np.int64), cat(starts, np.float64), cat(exact, np.float64)


def _resident(source, engine, framehop_prop: float, chunklength: float, max_windows: int, messages: List[str]):
    """The windows of ``source`` (a folder or an embedding store) as device rows, as ``cluster_recordings`` holds them."""
    store = _RowStore(engine.device, max_windows)

    def feed(parts, hop, step):
        first = store.reserve(_set_windows(engine, parts, hop, step))
        emb, counts = _embed_parts(engine, parts, hop, step)
        store.put(first, emb)
        return first, counts

    index = _walk(source, engine, framehop_prop, chunklength, messages, feed)
    return store.rows(), index


def _graph_of(rows, index, k: int, metric: str, messages: List[str]) -> KnnGraph:
    ids, sims = Neighbours(k, metric=metric, device=rows.device).update(rows).lists() if rows.shape[0] else \
        (np.zeros((0, k), np.int32), np.zeros((0, k), np.float32))
    recording_of, starts, _ = _index_arrays(index)
    return KnnGraph(ids, sims, list(index.idents), recording_of, starts, metric, list(messages))


def neighbour_graph(source, k: int = 16, *, metric: str = "cosine", engine=None, framehop_prop: float = 1.0,
                    chunklength: float = 200, embeddername: str = "yamnet_k2", max_windows: int = 1 << 22) -> KnnGraph:
    """The ``k`` nearest other windows of every window under ``source`` (a folder of recordings or an embedding store).  Every
    recording ``analyze`` would take is read and embedded as ``analyze(framehop_prop=..., chunklength=...)`` does it; the
    rows stay resident on the device (4 KB a window, at most ``max_windows``), and one sweep builds all lists."""
    _metric(metric)
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        rows, index = _resident(source, engine, framehop_prop, chunklength, max_windows, messages)
        return _graph_of(rows, index, k, metric, messages)
    finally:
        if own:
            engine.close()


@dataclass
class PropagationResult:
    """The windows of a folder with their propagated labels.  Window i lies in ``recordings[recording_of[i]]`` at ``starts[i]``;
    ``labels[i]`` is its class (-1 where no label flowed to it), ``reach[i]`` how much label mass arrived (0 .. 1),
    ``confidence[i]`` the top class's share of it, ``margin[i]`` the top's lead over the second; ``scores`` [N, C];
    ``annotated[i]``: the window carried a label going in."""
    labels: np.ndarray
    confidence: np.ndarray
    margin: np.ndarray
    reach: np.ndarray
    scores: np.ndarray
    iterations: int
    classes: List[str]
    annotated: np.ndarray
    recordings: List[str]
    recording_of: np.ndarray
    starts: np.ndarray
    graph: Optional[KnnGraph] = None
    messages: List[str] = field(default_factory=list)
    framelength_s: float = FRAMELENGTH_S

    def _window(self, i: int) -> Tuple[str, float]:
        return self.recordings[int(self.recording_of[i])], float(self.starts[i])

    def _name(self, i: int) -> str:
        return self.classes[int(self.labels[i])] if self.labels[i] >= 0 else ""

    def to_csv(self, path: str) -> None:
        """One row per window in the order of the walk: ``ident,start,end,label,confidence,margin,reach`` (an empty label where
        none arrived)."""
        with open(path, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(PROPAGATION_COLUMNS)
            for i in range(self.labels.shape[0]):
                ident, start = self._window(i)
                out.writerow([ident, repr(start), repr(_end(start, self.framelength_s)), self._name(i),
                              repr(float(self.confidence[i])), repr(float(self.margin[i])), repr(float(self.reach[i]))])

    def annotations(self, min_confidence: float = 0.9, min_reach: float = 0.5,
                    path: Optional[str] = None) -> List[Tuple[str, float, float, str]]:
        """The windows whose propagated label is trusted, as annotation rows (ident, start, end, label) in the order of the
        walk: ``confidence >= min_confidence`` and ``reach >= min_reach``.  The windows that were annotated going in are left
        out.  The two defaults are placeholders, not tuned on field data: check them with ``holdout_accuracy`` on your own
        labels.  ``path``: also written there, in the format ``dataset.read_annotations`` reads."""
        rows = []
        for i in np.flatnonzero((self.labels >= 0) & ~self.annotated & (self.confidence >= min_confidence) & (self.reach >= min_reach)):
            ident, start = self._window(i)
            rows.append((ident, start, _end(start, self.framelength_s), self._name(i)))
        if path is not None:
            with open(path, "w", newline="") as f:
                out = csv.writer(f)
                out.writerow(ANNOTATION_COLUMNS)
                for ident, start, end, label in rows:
                    out.writerow([ident, repr(start), repr(end), label])
        return rows


def label_rows(index, annotations, classes: Sequence[str], min_overlap: float = 0.5,
               background: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(labelled rows int64 [L], their classes int64 [L]) of the walk's windows, labelled as ``dataset.embed_annotated`` labels
    them; a window that is ambiguous, carries several classes or none is left unlabelled."""
    notes = _as_annotations(annotations)
    recording_of, _, exact = _index_arrays(index)
    label = np.full(exact.shape[0], -1, np.int64)
    for r, ident in enumerate(index.idents):
        mine = np.flatnonzero(recording_of == r)
        targets, keep, _ = _label_at(exact[mine], notes.get(ident, ()), classes, min_overlap, background)
        one = keep & (targets.sum(axis=1) == 1)
        label[mine[one]] = targets[one].argmax(axis=1)
    rows = np.flatnonzero(label >= 0)
    return rows, label[rows]


def propagate_recordings(source, annotations, classes: Sequence[str], *, k: int = 16, power: int = 4, symmetric: bool = True,
                         clamp: float = 1.0, max_iter: int = 50, tol: float = 1e-4, min_overlap: float = 0.5,
                         background: Optional[str] = None, graph: Optional[KnnGraph] = None, metric: str = "cosine", engine=None,
                         framehop_prop: float = 1.0, chunklength: float = 200, embeddername: str = "yamnet_k2",
                         max_windows: int = 1 << 22) -> PropagationResult:
    """The labels of ``annotations`` spread over every window under ``source`` (a folder or an embedding store).  The windows
    are labelled as ``dataset.embed_annotated`` labels them (ambiguous ones stay unlabelled), the ``k``-nearest-neighbour graph
    is built (or taken: ``graph``, a ``KnnGraph`` of the same walk), made symmetric unless ``symmetric=False`` (on a directed
    graph a label only flows against the lists' direction and reaches fewer windows), and ``Propagator(power, max_iter, tol)``
    runs on it; labelled rows get ``alpha = 1 - clamp``."""
    classes = list(classes)
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        if graph is None:
            rows, index = _resident(source, engine, framehop_prop, chunklength, max_windows, messages)
            graph = _graph_of(rows, index, k, metric, messages)
            del rows
        else:
            index = _walk(source, engine, framehop_prop, chunklength, messages,
                          _Counter(engine).feed)
        recording_of, starts, _ = _index_arrays(index)
        if graph.ids.shape[0] != starts.shape[0]:
            raise ValueError(f"the graph holds {graph.ids.shape[0]} windows, the walk {starts.shape[0]}")
        labelled, labels = label_rows(index, annotations, classes, min_overlap, background)
        y, alpha = targets_of(labelled, labels, starts.shape[0], len(classes), clamp)
        p = Propagator(power=power, max_iter=max_iter, tol=tol, device=engine.device)
        p.fit(graph.symmetrised() if symmetric else (graph.ids, graph.sims), y, alpha)
        annotated = np.zeros(starts.shape[0], bool)
        annotated[labelled] = True
        return PropagationResult(p.labels, p.confidence, p.margin, p.reach, p.scores, p.iterations, classes, annotated,
                                 list(index.idents), recording_of, starts, graph, messages)
    finally:
        if own:
            engine.close()


class _Counter:
    """A walk that only counts windows (the graph is given): nothing is embedded."""

    def __init__(self, engine):
        self.engine, self.seen = engine, 0

    def feed(self, parts, hop, step):
        from .dataset import _part_windows
        counts = [_part_windows(self.engine, p, hop, step) for p in parts]
        first, self.seen = self.seen, self.seen + sum(counts)
        return first, counts
