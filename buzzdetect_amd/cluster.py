"""Group a folder's windows by sound: k-means over the embeddings, on the device - the step before there is a first example to
``search`` with.

    KMeans               ``fit(embeddings)``, ``assign(embeddings)``: Lloyd's iterations where the rows lie
    cluster_recordings   a folder of recordings -> ClusterResult (the folder's rows stay resident on the device)
    assign_recordings    a folder against saved centres -> ClusterResult (streamed, launch set by launch set)
    ClusterResult        ``labels``, ``distances``, ``counts``, ``to_csv``, ``representatives``, ``annotations``, ``save``
    load                 the centres ``ClusterResult.save`` wrote -> ClusterModel

An iteration is four calls into ``include/buzzdetect_cluster.h`` (csrc/cluster.hip): assign (no [W, K] matrix is written),
statistics, a stable counting sort of the rows by label, chunked sums in a fixed order, and a finishing pass that leaves the next
centroids row-major, packed for the next assign and with their squared norms, all on the device.  One read-back per iteration
carries the statistics' slice partials; the ``[W, 1024]`` rows and the centroids stay where they are.  Nothing is added
atomically in floating point: the same data and the same seed give the same bits.

    from buzzdetect_amd import cluster, dataset, train

    found = cluster.cluster_recordings("audio_in", 24)
    for c, rows in enumerate(found.representatives(10)):                # listen to the windows nearest each centre
        print(c, found.counts[c], rows[:3])
    found.to_csv("clusters.csv")
    found.annotations({3: "ins_buzz", 7: "ambient"}, max_distance=0.2, path="first.csv")    # ident,start,end,label
    found.save("centres.npz")                                           # cluster.assign_recordings(later_folder, "centres.npz")
    ts = dataset.embed_annotated("audio_in", "first.csv", ["ambient", "ins_buzz"], background="ambient")
"""
from __future__ import annotations

import csv
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib, framing
from .dataset import DIGITS_TIME, FRAMELENGTH_S, _embed_parts, _open_engine, _part_windows, _torch
from .search import ANNOTATION_COLUMNS, _end, _walk, norms_host, pack_queries

CLUSTER_COLUMNS = ("ident", "start", "end", "cluster", "distance")
DIM = _lib.CLUSTER_DIM


# ---------------------------------------------------------------------------------------------------- host helpers
def _metric(metric: str) -> int:
    if metric not in _lib.CLUSTER_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.CLUSTER_METRICS)}, not {metric!r}")
    return _lib.CLUSTER_METRICS[metric]


def _rows(e, name: str = "rows") -> np.ndarray:
    e = np.ascontiguousarray(e, np.float32)
    if e.ndim != 2 or e.shape[1] != DIM:
        raise ValueError(f"{name} must be [W, {DIM}], not {list(e.shape)}")
    return e


def order_host(labels: np.ndarray, n_clusters: int) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_cluster_order_host``: (order int32 [W], offsets int32 [K + 1]) - the row ids sorted by (label, row id)."""
    labels = np.ascontiguousarray(labels, np.int32)
    order, offsets = np.zeros(labels.shape[0], np.int32), np.zeros(int(n_clusters) + 1, np.int32)
    _lib.check(_lib.load().bd_cluster_order_host(labels.ctypes.data, labels.shape[0], int(n_clusters), order.ctypes.data,
                                                 offsets.ctypes.data))
    return order, offsets


def centroids_host(e: np.ndarray, n2: Optional[np.ndarray], order: np.ndarray, offsets: np.ndarray, metric: str,
                   prev: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``bd_cluster_centroids_host``: (centroids float32 [K, 1024], packed, c2 float32 [K]) in the device's order of operations.
    ``n2``: the rows' squared norms (``search.norms_host``), read for ``cosine``."""
    e, prev = _rows(e), _rows(prev, "prev")
    k = prev.shape[0]
    order, offsets = np.ascontiguousarray(order, np.int32), np.ascontiguousarray(offsets, np.int32)
    if offsets.shape != (k + 1,) or order.shape != (e.shape[0],):
        raise ValueError("order must be [W] and offsets [K + 1]")
    n2 = None if n2 is None else np.ascontiguousarray(n2, np.float32)
    lib = _lib.load()
    cent = np.zeros((k, DIM), np.float32)
    packed = np.zeros(_lib.check(lib.bd_search_packed_floats(k)), np.float32)
    c2 = np.zeros(k, np.float32)
    _lib.check(lib.bd_cluster_centroids_host(e.ctypes.data, e.shape[0], None if n2 is None else n2.ctypes.data, order.ctypes.data,
                                             offsets.ctypes.data, k, _metric(metric), prev.ctypes.data, cent.ctypes.data,
                                             packed.ctypes.data, c2.ctypes.data))
    return cent, packed, c2


def stats_host(dist: np.ndarray, labels: np.ndarray, prev_labels: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_cluster_stats_host``: (partial float32 [S], changed int32 [S]) over slices of 256 rows."""
    dist = np.ascontiguousarray(dist, np.float32)
    labels, prev_labels = np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(prev_labels, np.int32)
    if not dist.shape == labels.shape == prev_labels.shape or dist.ndim != 1:
        raise ValueError("dist, labels and prev_labels must be [W]")
    slices = (dist.shape[0] + _lib.CLUSTER_STAT_SLICE - 1) // _lib.CLUSTER_STAT_SLICE
    partial, changed = np.zeros(slices, np.float32), np.zeros(slices, np.int32)
    _lib.check(_lib.load().bd_cluster_stats_host(dist.ctypes.data, labels.ctypes.data, prev_labels.ctypes.data, dist.shape[0],
                                                 partial.ctypes.data, changed.ctypes.data))
    return partial, changed


def normalise_centroids(rows, metric: str) -> np.ndarray:
    """float32 [K, 1024] as assign takes them: for ``cosine`` every row brought to unit length in float64 (a zero row stays
    zero), then cast - what ``search.normalise_queries`` does to queries."""
    _metric(metric)
    c = np.asarray(rows, np.float64)
    if c.ndim != 2 or c.shape[1] != DIM or not 1 <= c.shape[0] <= _lib.CLUSTER_MAX_CLUSTERS:
        raise ValueError(f"centroids must be [1..{_lib.CLUSTER_MAX_CLUSTERS}, {DIM}], not {list(c.shape)}")
    if metric == "cosine":
        length = np.sqrt((c * c).sum(axis=1, keepdims=True))
        c = np.divide(c, length, out=np.zeros_like(c), where=length > 0)
    return np.ascontiguousarray(c.astype(np.float32))


def kmeanspp_draw(rng: np.random.Generator, distances) -> int:
    """The next k-means++ centre among rows at ``distances`` from their nearest centre so far: row i with probability
    distances[i] / sum, by one ``rng.random()`` against the float64 cumulative sum (a distance that is negative, infinite or
    NaN weighs nothing); when no row weighs anything, one ``rng.integers`` over all rows."""
    d = np.asarray(distances, np.float64)
    d = np.where(np.isfinite(d) & (d > 0), d, 0.0)
    cum = np.cumsum(d)
    if not cum[-1] > 0:
        return int(rng.integers(d.size))
    return int(min(np.searchsorted(cum, rng.random() * cum[-1], side="right"), d.size - 1))


# ---------------------------------------------------------------------------------------------------- the model
@dataclass
class ClusterModel:
    """Centres as ``save`` writes them: what ``assign_recordings`` and ``KMeans.from_model`` take."""
    centroids: np.ndarray
    metric: str
    counts: np.ndarray

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            np.savez(f, centroids=np.asarray(self.centroids, np.float32), metric=np.array(self.metric),
                     counts=np.asarray(self.counts, np.int64))


def load(path: str) -> ClusterModel:
    """The ``.npz`` of ``ClusterResult.save`` (``ClusterModel.save``)."""
    with np.load(path, allow_pickle=False) as z:
        model = ClusterModel(_rows(z["centroids"], "centroids"), str(z["metric"]), np.asarray(z["counts"], np.int64))
    _metric(model.metric)
    if model.counts.shape != (model.centroids.shape[0],):
        raise ValueError(f"{path}: {model.counts.shape[0]} counts for {model.centroids.shape[0]} centroids")
    return model


class _Centres:
    """One centroid set on the device: the rows, their packed form and their squared norms."""

    def __init__(self, owner: "KMeans", k: int):
        torch = _torch()
        self.rows = owner._empty((k, DIM), torch.float32)
        self.packed = owner._empty((_lib.check(owner._lib.bd_search_packed_floats(k)),), torch.float32)
        self.c2 = owner._empty((k,), torch.float32)

    def upload(self, rows: np.ndarray) -> "_Centres":
        torch = _torch()
        self.rows.copy_(torch.from_numpy(rows))
        self.packed.copy_(torch.from_numpy(pack_queries(rows)))
        self.c2.copy_(torch.from_numpy(norms_host(rows)))
        return self


class KMeans:
    """Lloyd's k-means over float32 [W, 1024] rows on the device.  ``metric``: ``"cosine"`` (spherical k-means: rows and centres
    at unit length, distance 1 - cosine; groups the way ``search`` ranks) or ``"euclidean"`` (squared distance).  ``init``:
    ``"k-means++"`` on a seeded subsample of at most ``init_rows`` rows, or an array [K, 1024] of first centres.  An iteration
    assigns, then stops if no label changed, if the inertia fell by at most ``tol`` of its value, or at ``max_iter``; else it
    moves the centres.  So ``labels`` and ``distances`` always belong to ``centroids``.  A cluster that loses all its rows keeps
    its centre and reports ``counts == 0``.  ``n_init`` fits (seeds ``seed, seed + 1, ...``) keep the one of lowest inertia.

    After ``fit``: ``centroids`` [K, 1024], ``labels`` int32 [W], ``distances`` float32 [W], ``counts`` int64 [K],
    ``inertia_history`` (one float per iteration), ``n_iter``."""

    def __init__(self, n_clusters: int, metric: str = "cosine", max_iter: int = 50, tol: float = 0.0, seed: int = 0,
                 init="k-means++", n_init: int = 1, init_rows: int = 65536, device=None):
        if not 1 <= int(n_clusters) <= _lib.CLUSTER_MAX_CLUSTERS:
            raise ValueError(f"n_clusters must be in 1..{_lib.CLUSTER_MAX_CLUSTERS}, not {n_clusters}")
        self._metric_id = _metric(metric)
        if int(max_iter) < 1 or int(n_init) < 1 or int(init_rows) < 1 or not float(tol) >= 0:
            raise ValueError("max_iter, n_init and init_rows must be at least 1 and tol at least 0")
        if isinstance(init, str):
            if init != "k-means++":
                raise ValueError(f"init must be \"k-means++\" or an array [{n_clusters}, {DIM}], not {init!r}")
        else:
            init = normalise_centroids(init, metric)
            if init.shape[0] != int(n_clusters):
                raise ValueError(f"init holds {init.shape[0]} rows for {n_clusters} clusters")
        self.n_clusters, self.metric, self.max_iter, self.tol = int(n_clusters), metric, int(max_iter), float(tol)
        self.seed, self.init, self.n_init, self.init_rows = int(seed), init, int(n_init), int(init_rows)
        self._device_arg = device
        self.device = None
        self._lib = None
        self._centres: Optional[_Centres] = None
        self.centroids = self.labels = self.distances = self.counts = None
        self.inertia_history: List[float] = []
        self.n_iter = 0

    @classmethod
    def from_model(cls, model: ClusterModel, device=None) -> "KMeans":
        """Saved centres, taken bit for bit (not brought to unit length again), ready for ``assign``."""
        km = cls(model.centroids.shape[0], metric=model.metric, device=device)
        km.centroids = _rows(model.centroids, "centroids")
        km.counts = np.asarray(model.counts, np.int64)
        return km

    def model(self) -> ClusterModel:
        if self.centroids is None:
            raise RuntimeError("fit first")
        return ClusterModel(self.centroids, self.metric, self.counts)

    # ------------------------------------------------------------------------------------------------ device plumbing
    def _empty(self, shape, dtype):
        """Every device buffer the kernels write comes from here (the tests put guard words around them)."""
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def _open(self, embeddings=None) -> None:
        torch = _torch()
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; clustering has no CPU path")
        device = self._device_arg
        if device is None:
            device = embeddings.device if isinstance(embeddings, torch.Tensor) and embeddings.is_cuda else \
                torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)

    def _stream(self):
        return _torch().cuda.current_stream(self.device)

    def _check_rows(self, embeddings):
        torch = _torch()
        e = embeddings
        if not isinstance(e, torch.Tensor):
            e = torch.from_numpy(_rows(e, "embeddings")).to(self.device)
        if (e.dim() != 2 or e.shape[1] != DIM or e.dtype != torch.float32 or e.device != self.device or not e.is_contiguous()
                or e.data_ptr() % 16):
            raise ValueError(f"embeddings must be a contiguous, 16-byte aligned float32 [W, {DIM}] tensor on {self.device}")
        if e.shape[0] > _lib.CLUSTER_MAX_ROWS:
            raise ValueError(f"a call takes at most {_lib.CLUSTER_MAX_ROWS} rows, not {e.shape[0]}")
        return e

    def _norms(self, e):
        torch = _torch()
        w = int(e.shape[0])
        n2 = self._empty((w,), torch.float32)
        with torch.cuda.device(self.device):
            for at in range(0, w, _lib.SEARCH_MAX_WINDOWS):              # bd_search_norms takes 2^20 rows a call
                n = min(_lib.SEARCH_MAX_WINDOWS, w - at)
                _lib.check(self._lib.bd_search_norms(e[at:at + n].data_ptr(), n, n2[at:at + n].data_ptr(),
                                                     self._stream().cuda_stream))
        return n2

    def _assign(self, e, n2, centres: _Centres, k: int, labels, dist) -> None:
        torch = _torch()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_cluster_assign(e.data_ptr(), int(e.shape[0]), n2.data_ptr(), centres.packed.data_ptr(),
                                                   centres.c2.data_ptr(), k, self._metric_id, labels.data_ptr(), dist.data_ptr(),
                                                   self._stream().cuda_stream))

    # ------------------------------------------------------------------------------------------------ initialisation
    def _plus_plus(self, e, n2, rng: np.random.Generator) -> np.ndarray:
        """k-means++ over a subsample: K - 1 one-centre assign passes, the running minimum kept on the device, each draw made
        on the host from its float64 cumulative sum.  Returns the K chosen rows (float32, as they lie in ``e``)."""
        torch = _torch()
        w = int(e.shape[0])
        m = min(w, self.init_rows)
        if m < w:
            pick = torch.from_numpy(np.sort(rng.choice(w, size=m, replace=False))).to(self.device)
            e, n2 = e.index_select(0, pick).contiguous(), n2.index_select(0, pick).contiguous()
        chosen = [int(rng.integers(m))]
        one = _Centres(self, 1)
        labels, dist = self._empty((m,), torch.int32), self._empty((m,), torch.float32)
        nearest = None
        for _ in range(1, self.n_clusters):
            one.upload(normalise_centroids(e[chosen[-1]:chosen[-1] + 1].cpu().numpy(), self.metric))
            self._assign(e, n2, one, 1, labels, dist)
            nearest = dist.clone() if nearest is None else torch.minimum(nearest, dist)
            chosen.append(kmeanspp_draw(rng, nearest.cpu().numpy()))
        return e.index_select(0, torch.tensor(chosen, dtype=torch.int64, device=self.device)).cpu().numpy()

    # ------------------------------------------------------------------------------------------------ fitting
    def _fit_once(self, e, n2, first: np.ndarray):
        torch = _torch()
        w, k = int(e.shape[0]), self.n_clusters
        slices = (w + _lib.CLUSTER_STAT_SLICE - 1) // _lib.CLUSTER_STAT_SLICE
        sets = [_Centres(self, k).upload(first), _Centres(self, k)]
        labels = [self._empty((w,), torch.int32), self._empty((w,), torch.int32)]
        labels[1].fill_(-1)                                             # no row has a label yet: every one changes
        dist = self._empty((w,), torch.float32)
        stats = self._empty((2, slices), torch.int32)                   # row 0: float32 partials, row 1: counts
        order, offsets = self._empty((w,), torch.int32), self._empty((k + 1,), torch.int32)
        ws_bytes = _lib.check(self._lib.bd_cluster_workspace_bytes(w, k))
        workspace = self._empty((ws_bytes,), torch.uint8)
        history: List[float] = []
        cur = 0
        stream = self._stream().cuda_stream
        for it in range(self.max_iter):
            new, old = labels[it & 1], labels[(it & 1) ^ 1]
            self._assign(e, n2, sets[cur], k, new, dist)
            with torch.cuda.device(self.device):
                _lib.check(self._lib.bd_cluster_stats(dist.data_ptr(), new.data_ptr(), old.data_ptr(), w, stats[0].data_ptr(),
                                                      stats[1].data_ptr(), stream))
            host = stats.cpu().numpy()                                  # the iteration's one read-back
            inertia = float(host[0].view(np.float32).astype(np.float64).sum())
            changed = int(host[1].astype(np.int64).sum())
            history.append(inertia)
            settled = len(history) > 1 and history[-2] - inertia <= self.tol * history[-2]
            if changed == 0 or settled or it == self.max_iter - 1:
                break
            with torch.cuda.device(self.device):
                _lib.check(self._lib.bd_cluster_order(new.data_ptr(), w, k, order.data_ptr(), offsets.data_ptr(),
                                                      workspace.data_ptr(), ws_bytes, stream))
                nxt = sets[cur ^ 1]
                _lib.check(self._lib.bd_cluster_centroids(e.data_ptr(), w, n2.data_ptr(), order.data_ptr(), offsets.data_ptr(), k,
                                                          self._metric_id, sets[cur].rows.data_ptr(), nxt.rows.data_ptr(),
                                                          nxt.packed.data_ptr(), nxt.c2.data_ptr(), workspace.data_ptr(),
                                                          ws_bytes, stream))
            cur ^= 1
        return sets[cur], labels[(len(history) - 1) & 1], dist, history

    def fit(self, embeddings) -> "KMeans":
        """``embeddings``: a device tensor or an array, float32 [W, 1024] with W >= n_clusters."""
        self._open(embeddings)
        e = self._check_rows(embeddings)
        w = int(e.shape[0])
        if w < self.n_clusters:
            raise ValueError(f"{w} rows cannot make {self.n_clusters} clusters")
        n2 = self._norms(e)
        best = None
        for run in range(self.n_init if isinstance(self.init, str) else 1):
            if isinstance(self.init, str):
                first = normalise_centroids(self._plus_plus(e, n2, np.random.default_rng(self.seed + run)), self.metric)
            else:
                first = self.init                                       # (brought to unit length once, in __init__)
            centres, labels, dist, history = self._fit_once(e, n2, first)
            if best is None or history[-1] < best[3][-1]:
                best = (centres, labels, dist, history)
        self._centres, labels, dist, history = best
        self.centroids = self._centres.rows.cpu().numpy()
        self.labels, self.distances = labels.cpu().numpy(), dist.cpu().numpy()
        self.counts = np.bincount(self.labels, minlength=self.n_clusters).astype(np.int64)
        self.inertia_history, self.n_iter = list(history), len(history)
        return self

    def assign(self, embeddings) -> Tuple[np.ndarray, np.ndarray]:
        """(labels int32 [W], distances float32 [W]) of new rows against the fitted centres."""
        torch = _torch()
        if self.centroids is None:
            raise RuntimeError("fit first (or build from saved centres with KMeans.from_model)")
        if self.device is None:
            self._open(embeddings)
        if self._centres is None:
            self._centres = _Centres(self, self.n_clusters).upload(self.centroids)
        e = self._check_rows(embeddings)
        w = int(e.shape[0])
        labels, dist = self._empty((w,), torch.int32), self._empty((w,), torch.float32)
        if w:
            self._assign(e, self._norms(e), self._centres, self.n_clusters, labels, dist)
        return labels.cpu().numpy(), dist.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- results
@dataclass
class ClusterResult:
    """The windows of a folder with their clusters.  Window i lies in recording ``recordings[recording_of[i]]`` at ``starts[i]``
    (``analyze``'s start column for it), in cluster ``labels[i]`` at ``distances[i]`` from its centre.  ``counts[c]``: windows in
    cluster c."""
    labels: np.ndarray
    distances: np.ndarray
    counts: np.ndarray
    recordings: List[str]
    recording_of: np.ndarray
    starts: np.ndarray
    centroids: Optional[np.ndarray] = None
    metric: str = "cosine"
    messages: List[str] = field(default_factory=list)
    framelength_s: float = FRAMELENGTH_S

    def __post_init__(self):
        self.labels = np.asarray(self.labels, np.int32)
        self.distances = np.asarray(self.distances, np.float32)
        self.counts = np.asarray(self.counts, np.int64)
        self.recording_of = np.asarray(self.recording_of, np.int64)
        self.starts = np.asarray(self.starts, np.float64)
        n = self.labels.shape[0]
        if not (self.distances.shape == self.recording_of.shape == self.starts.shape == (n,)):
            raise ValueError("labels, distances, recording_of and starts must have one entry per window")

    def _window(self, i: int) -> Tuple[str, float]:
        return self.recordings[int(self.recording_of[i])], float(self.starts[i])

    def to_csv(self, path: str) -> None:
        """One row per window in the order of the walk: ``ident,start,end,cluster,distance`` (end = start + 0.96 s)."""
        with open(path, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(CLUSTER_COLUMNS)
            for i in range(self.labels.shape[0]):
                ident, start = self._window(i)
                out.writerow([ident, repr(start), repr(_end(start, self.framelength_s)), int(self.labels[i]),
                              repr(float(self.distances[i]))])

    def representatives(self, n: int = 10) -> List[List[Tuple[str, float, float]]]:
        """Per cluster the ``n`` windows nearest its centre as (ident, start, distance), nearest first; among equal distances
        the window that comes first in the walk."""
        ids = np.arange(self.labels.shape[0])
        out = []
        for c in range(self.counts.shape[0]):
            mine = ids[self.labels == c]
            best = mine[np.lexsort((mine, self.distances[mine].astype(np.float64)))][:max(int(n), 0)]
            out.append([(*self._window(i), float(self.distances[i])) for i in best])
        return out

    def annotations(self, labels: Dict[int, str], max_distance: Optional[float] = None,
                    path: Optional[str] = None) -> List[Tuple[str, float, float, str]]:
        """The windows of the reviewed clusters as annotation rows (ident, start, end, label), in the order of the walk.
        ``labels``: cluster -> label, for the clusters to keep.  ``max_distance``: only windows at most that far from their
        centre.  ``path``: also written there, in the format ``dataset.read_annotations`` reads."""
        names = {int(c): str(l) for c, l in labels.items()}
        bad = [c for c in names if not 0 <= c < self.counts.shape[0]]
        if bad:
            raise ValueError(f"clusters {bad} are not among 0..{self.counts.shape[0] - 1}")
        rows = []
        for i in range(self.labels.shape[0]):
            c = int(self.labels[i])
            if c in names and (max_distance is None or self.distances[i] <= max_distance):
                ident, start = self._window(i)
                rows.append((ident, start, _end(start, self.framelength_s), names[c]))
        if path is not None:
            with open(path, "w", newline="") as f:
                out = csv.writer(f)
                out.writerow(ANNOTATION_COLUMNS)
                for ident, start, end, label in rows:
                    out.writerow([ident, repr(start), repr(end), label])
        return rows

    def model(self) -> ClusterModel:
        if self.centroids is None:
            raise RuntimeError("this result carries no centroids")
        return ClusterModel(self.centroids, self.metric, self.counts)

    def save(self, path: str) -> None:
        """One ``.npz``: centroids, metric, counts (``cluster.load`` reads it, ``assign_recordings`` takes it)."""
        self.model().save(path)


def _result(index, labels, distances, counts, centroids, metric: str, messages) -> ClusterResult:
    """``search._Index`` -> per-window recording and start (``_Index.lookup`` for every id, by whole chunks)."""
    recording_of, starts = [], []
    for r, (_, starts_s, chunk_counts) in enumerate(index.chunks):
        for start_s, n in zip(starts_s, chunk_counts):
            starts.append(np.asarray(framing.window_starts(n, start_s, index.framehop_s, DIGITS_TIME), np.float64).reshape(-1))
            recording_of.append(np.full(int(n), r, np.int64))
    cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype)
    return ClusterResult(labels, distances, counts, list(index.idents), cat(recording_of, np.int64), cat(starts, np.float64),
                         centroids, metric, list(messages))


class _RowStore:
    """The folder's rows on the device, 4 KB a window: grows by doubling up to ``max_windows`` and refuses before it would
    allocate past that."""

    def __init__(self, device, max_windows: int):
        self.device, self.max_windows = device, int(max_windows)
        self.buf = None
        self.n = 0

    def reserve(self, n: int) -> int:
        torch = _torch()
        if self.n + n > self.max_windows:
            raise ValueError(f"the folder holds more than max_windows = {self.max_windows} windows ({self.n + n} counted so far): "
                             f"cluster a part of it, raise max_windows if the device has 4 KB for each, or fit on a sample and "
                             f"label the rest with assign_recordings")
        cap = 0 if self.buf is None else int(self.buf.shape[0])
        if self.n + n > cap:
            grown = torch.empty((min(max(2 * cap, self.n + n, 4096), self.max_windows), DIM), dtype=torch.float32,
                                device=self.device)
            if self.n:
                grown[:self.n].copy_(self.buf[:self.n])
            self.buf = grown
        first, self.n = self.n, self.n + n
        return first

    def put(self, first: int, rows) -> None:
        self.buf[first:first + int(rows.shape[0])].copy_(rows)

    def rows(self):
        torch = _torch()
        if self.buf is None:
            return torch.empty((0, DIM), dtype=torch.float32, device=self.device)
        return self.buf[:self.n]


def _set_windows(engine, parts, hop: int, step: int) -> int:
    return sum(_part_windows(engine, p, hop, step) for p in parts)


def cluster_recordings(dir_audio: str, n_clusters: int, *, metric: str = "cosine", engine=None, framehop_prop: float = 1.0,
                       chunklength: float = 200, embeddername: str = "yamnet_k2", max_windows: int = 1 << 22,
                       **kmeans_options) -> ClusterResult:
    """``n_clusters`` groups of the windows under ``dir_audio``.  Every recording ``analyze`` would take is read, resampled and
    embedded as ``analyze(framehop_prop=..., chunklength=...)`` does it, one launch set alive at a time; the rows are gathered
    in a device buffer of 4 KB per window, ``KMeans(n_clusters, metric=metric, **kmeans_options)`` fits them there.  A folder
    of more than ``max_windows`` windows is refused (``ValueError``) before anything past the limit is allocated."""
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
        km = KMeans(n_clusters, metric=metric, device=engine.device, **kmeans_options).fit(store.rows())
        return _result(index, km.labels, km.distances, km.counts, km.centroids, metric, messages)
    finally:
        if own:
            engine.close()


def assign_recordings(dir_audio: str, model, *, engine=None, framehop_prop: float = 1.0, chunklength: float = 200,
                      embeddername: str = "yamnet_k2") -> ClusterResult:
    """The windows under ``dir_audio`` labelled with saved centres (``model``: a ``ClusterModel``, a fitted ``KMeans`` or the
    path of a ``save``).  Each launch set's rows are assigned and dropped: no residency, no ``max_windows``.  ``counts`` are
    this folder's."""
    if isinstance(model, str):
        model = load(model)
    if isinstance(model, KMeans):
        model = model.model()
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        km = KMeans.from_model(model, device=engine.device)
        labels, distances, seen = [], [], [0]

        def feed(parts, hop, step):
            emb, counts = _embed_parts(engine, parts, hop, step)
            l, d = km.assign(emb)
            labels.append(l)
            distances.append(d)
            first, seen[0] = seen[0], seen[0] + int(emb.shape[0])
            return first, counts

        index = _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed)
        l = np.concatenate(labels) if labels else np.zeros(0, np.int32)
        d = np.concatenate(distances) if distances else np.zeros(0, np.float32)
        counts = np.bincount(l, minlength=model.centroids.shape[0]).astype(np.int64)
        return _result(index, l, d, counts, model.centroids, model.metric, messages)
    finally:
        if own:
            engine.close()
