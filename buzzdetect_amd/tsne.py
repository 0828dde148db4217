"""A neighbour-preserving 2-D map of a folder: exact t-SNE from the k-nearest-neighbour lists, on the device - the picture
``pca.map_recordings`` cannot give once a folder holds more than a handful of sound types.

    layout_recordings      a folder or an embedding store -> LayoutResult (``coords``, ``kl``, the graph, the window index)
    layout_graph           a saved ``KnnGraph`` without rows -> LayoutResult
    TSNE                   ``fit(graph, init)``: calibration and layout on device tensors, as ``Propagator`` is for propagation
    Schedule               perplexity, exaggeration, momentum, learning rate, iterations
    joint_probabilities    conditional probabilities of the lists -> the symmetric P in CSR form
    LayoutResult           ``to_csv``, ``preservation``, ``save`` / ``load``

The lists come from ``include/buzzdetect_knn.h``; calibration, forces and update are ``include/buzzdetect_tsne.h``
(csrc/tsne.hip).  The repulsion is the full sum over all pairs: no tree, no grid, no sampling.  Attraction, repulsion and update
are reproducible bit for bit and have host restatements with the same bits (the ``*_host`` functions here, and ``fit_host`` for
the whole loop); the affinities and the divergence use exp and log and agree with their restatements closely, not in every bit.

    from buzzdetect_amd import tsne

    found = tsne.layout_recordings("audio_in")                          # a folder or an embedding store
    found.to_csv("layout.csv")                                          # ident,start,end,x,y
    print(found.kl, found.preservation())
"""
from __future__ import annotations

import csv
from dataclasses import dataclass, field
from typing import List, Optional, Tuple, Union

import numpy as np

from . import _lib
from .dataset import FRAMELENGTH_S, _open_engine, _torch
from .propagate import KnnGraph, _Device, _graph_of, _resident
from .search import _end

LAYOUT_COLUMNS = ("ident", "start", "end", "x", "y")


# ---------------------------------------------------------------------------------------------------- host restatements
def _lists(ids, sims) -> Tuple[np.ndarray, np.ndarray]:
    ids, sims = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(sims, np.float32)
    if ids.ndim != 2 or ids.shape != sims.shape:
        raise ValueError("ids and sims must be [N, k]")
    return ids, sims


def _points(y, name: str = "y") -> np.ndarray:
    y = np.ascontiguousarray(y, np.float32)
    if y.ndim != 2 or y.shape[1] != 2:
        raise ValueError(f"{name} must be [N, 2], not {list(y.shape)}")
    return y


def affinities_host(ids, sims, perplexity: float) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_tsne_affinities_host``: lists [N, k] -> (p float32 [N, k], beta float32 [N])."""
    ids, sims = _lists(ids, sims)
    p, beta = np.zeros(ids.shape, np.float32), np.zeros(ids.shape[0], np.float32)
    _lib.check(_lib.load().bd_tsne_affinities_host(ids.ctypes.data, sims.ctypes.data, ids.shape[0], ids.shape[1], float(perplexity),
                                                   p.ctypes.data, beta.ctypes.data))
    return p, beta


@dataclass
class JointGraph:
    """The symmetric P in CSR form: row i's neighbours are ``nbr[row_start[i]:row_start[i + 1]]`` (ascending) with ``P`` there."""
    row_start: np.ndarray
    nbr: np.ndarray
    P: np.ndarray

    def __post_init__(self):
        self.row_start = np.ascontiguousarray(self.row_start, np.int64)
        self.nbr = np.ascontiguousarray(self.nbr, np.int32).reshape(-1)
        self.P = np.ascontiguousarray(self.P, np.float32).reshape(-1)
        if self.row_start.ndim != 1 or self.row_start.shape[0] < 1 or self.nbr.shape != self.P.shape:
            raise ValueError("row_start must be [N + 1], nbr and P [E]")

    @property
    def n_rows(self) -> int:
        return int(self.row_start.shape[0] - 1)

    @property
    def n_edges(self) -> int:
        return int(self.nbr.shape[0])


def _graph_args(graph: JointGraph, y: np.ndarray):
    if graph.n_rows != y.shape[0]:
        raise ValueError(f"the graph has {graph.n_rows} rows, y {y.shape[0]}")
    return graph.row_start.ctypes.data, graph.nbr.ctypes.data, graph.P.ctypes.data, graph.n_rows, graph.n_edges, y.ctypes.data


def attract_host(graph: JointGraph, y) -> np.ndarray:
    """``bd_tsne_attract_host``: attr float32 [N, 2]."""
    y = _points(y)
    attr = np.zeros_like(y)
    _lib.check(_lib.load().bd_tsne_attract_host(*_graph_args(graph, y), attr.ctypes.data))
    return attr


def repulse_host(y) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_tsne_repulse_host``: (rep float32 [N, 2], z float32 [N])."""
    y = _points(y)
    rep, z = np.zeros_like(y), np.zeros(y.shape[0], np.float32)
    _lib.check(_lib.load().bd_tsne_repulse_host(y.ctypes.data, y.shape[0], rep.ctypes.data, z.ctypes.data))
    return rep, z


def update_host(y, v, gain, attr, rep, z, exaggeration: float, momentum: float, rate: float,
                min_gain: float = 0.01) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.float32]:
    """``bd_tsne_update_host`` on copies: (y, v, gain, Z)."""
    y, v, gain = _points(y).copy(), _points(v, "v").copy(), _points(gain, "gain").copy()
    attr, rep, z = _points(attr, "attr"), _points(rep, "rep"), np.ascontiguousarray(z, np.float32)
    n = y.shape[0]
    if not (v.shape == gain.shape == attr.shape == rep.shape == (n, 2)) or z.shape != (n,):
        raise ValueError("y, v, gain, attr and rep must be [N, 2] and z [N]")
    total = np.zeros(1, np.float32)
    _lib.check(_lib.load().bd_tsne_update_host(y.ctypes.data, v.ctypes.data, gain.ctypes.data, attr.ctypes.data, rep.ctypes.data,
                                               z.ctypes.data, n, float(exaggeration), float(momentum), float(rate), float(min_gain),
                                               total.ctypes.data))
    return y, v, gain, total[0]


def kl_host(graph: JointGraph, y, z) -> np.float32:
    """``bd_tsne_kl_host``: the divergence of the map ``y`` from ``graph``'s P, with ``z`` as ``repulse_host(y)`` gives it."""
    y, z = _points(y), np.ascontiguousarray(z, np.float32)
    if z.shape != (y.shape[0],):
        raise ValueError("z must be [N]")
    kl = np.zeros(1, np.float32)
    _lib.check(_lib.load().bd_tsne_kl_host(*_graph_args(graph, y), z.ctypes.data, kl.ctypes.data))
    return kl[0]


def joint_probabilities(ids, p) -> JointGraph:
    """The union of every edge of the lists and its reverse: ``P_ij = (p_j|i + p_i|j) / (2 N)``, formed in float64 and rounded
    once, so that both directions carry the same bits.  Each row is ordered by ascending neighbour.  A pair whose P is 0 is
    left out.  Built on the host."""
    ids, p = _lists(ids, p)
    n = ids.shape[0]
    real = (ids >= 0) & (ids < n) & (ids != np.arange(n, dtype=np.int32)[:, None])
    src = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], ids.shape)[real]
    dst = ids[real].astype(np.int64)
    val = p[real].astype(np.float64)
    i, j, s = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([val, val])
    order = np.lexsort((j, i))
    i, j, s = i[order], j[order], s[order]
    first = np.ones(i.shape[0], bool)
    first[1:] = (i[1:] != i[:-1]) | (j[1:] != j[:-1])
    group = np.cumsum(first) - 1
    total = np.bincount(group, weights=s, minlength=int(first.sum()))    # at most two terms a pair: the order cannot matter
    i, j = i[first], j[first]
    big = (total / (2.0 * n)).astype(np.float32)
    keep = big > 0
    i, j, big = i[keep], j[keep], big[keep]
    row_start = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=row_start[1:])
    return JointGraph(row_start, j.astype(np.int32), big)


# ---------------------------------------------------------------------------------------------------- schedule
@dataclass
class Schedule:
    """How the map is laid out.  ``n_iter`` is the total number of iterations, the first ``exaggeration_iter`` of them with P
    multiplied by ``early_exaggeration`` and the first momentum.  ``learning_rate`` "auto" is
    ``max(N / early_exaggeration / 4, 50)``."""
    perplexity: float = 16.0
    early_exaggeration: float = 12.0
    exaggeration_iter: int = 250
    n_iter: int = 750
    momentum: Tuple[float, float] = (0.5, 0.8)
    learning_rate: Union[str, float] = "auto"
    min_gain: float = 0.01

    def __post_init__(self):
        if not (np.isfinite(self.perplexity) and self.perplexity >= 1):
            raise ValueError(f"perplexity must be finite and at least 1, not {self.perplexity}")
        if not (np.isfinite(self.early_exaggeration) and self.early_exaggeration >= 1):
            raise ValueError(f"early_exaggeration must be finite and at least 1, not {self.early_exaggeration}")
        if int(self.n_iter) < 0 or not 0 <= int(self.exaggeration_iter) <= int(self.n_iter):
            raise ValueError("n_iter is the total: it must be at least exaggeration_iter, and neither may be negative")
        self.momentum = tuple(float(m) for m in self.momentum)
        if len(self.momentum) != 2 or not all(0 <= m < 1 for m in self.momentum):
            raise ValueError("momentum must be two values in [0, 1)")
        if self.learning_rate != "auto" and not (np.isfinite(float(self.learning_rate)) and float(self.learning_rate) > 0):
            raise ValueError(f'learning_rate must be "auto" or positive, not {self.learning_rate!r}')
        if not 0 < float(self.min_gain) <= 1:
            raise ValueError("min_gain must be in (0, 1]")

    def check_k(self, k: int) -> None:
        if not 3 * self.perplexity <= k:
            raise ValueError(f"perplexity {self.perplexity} needs lists of at least k = {int(np.ceil(3 * self.perplexity))} "
                             f"neighbours (3 x perplexity), not {k}")
        if k > _lib.TSNE_MAX_K:
            raise ValueError(f"k must be at most {_lib.TSNE_MAX_K}, not {k}")

    def rate(self, n_rows: int) -> float:
        return max(n_rows / float(self.early_exaggeration) / 4.0, 50.0) if self.learning_rate == "auto" else float(self.learning_rate)

    def at(self, iteration: int) -> Tuple[float, float]:
        """(exaggeration, momentum) of iteration 0 .. n_iter - 1."""
        early = iteration < int(self.exaggeration_iter)
        return (float(self.early_exaggeration) if early else 1.0), self.momentum[0 if early else 1]


def fit_host(graph: JointGraph, init, schedule: Optional[Schedule] = None,
             report_every: Optional[int] = None) -> Tuple[np.ndarray, np.float32, List[Tuple[int, float]]]:
    """The whole loop on the host restatements, from P: (coords, kl, kl_history) with the bits ``TSNE.fit`` has for attraction,
    repulsion and update (and so for the coordinates, given the same P)."""
    schedule = schedule or Schedule()
    lib = _lib.load()
    y = _points(init, "init").copy()
    n = y.shape[0]
    v, gain = np.zeros_like(y), np.ones_like(y)
    attr, rep, z = np.zeros_like(y), np.zeros_like(y), np.zeros(n, np.float32)
    kl, history = np.zeros(1, np.float32), []
    rate = schedule.rate(n)
    args = _graph_args(graph, y)

    def divergence():
        _lib.check(lib.bd_tsne_repulse_host(y.ctypes.data, n, rep.ctypes.data, z.ctypes.data))
        _lib.check(lib.bd_tsne_kl_host(*args, z.ctypes.data, kl.ctypes.data))
        return kl[0]

    for it in range(int(schedule.n_iter) if n else 0):
        exaggeration, momentum = schedule.at(it)
        _lib.check(lib.bd_tsne_attract_host(*args, attr.ctypes.data))
        _lib.check(lib.bd_tsne_repulse_host(y.ctypes.data, n, rep.ctypes.data, z.ctypes.data))
        _lib.check(lib.bd_tsne_update_host(y.ctypes.data, v.ctypes.data, gain.ctypes.data, attr.ctypes.data, rep.ctypes.data,
                                           z.ctypes.data, n, exaggeration, momentum, rate, float(schedule.min_gain), None))
        if report_every and (it + 1) % int(report_every) == 0:
            history.append((it + 1, float(divergence())))
    return y, (divergence() if n else np.float32(np.nan)), history


# ---------------------------------------------------------------------------------------------------- rows left out
def leave_out(ids, sims, init) -> Tuple[np.ndarray, np.ndarray, np.ndarray, List[str]]:
    """Which rows take part: (keep bool [N], ids of the kept rows renumbered, their sims, messages).  A row whose start is not
    finite is left out, and with it every list entry that names it; then a row with no usable neighbour that is in nobody's
    list.  An entry is usable if its id is a kept row and its similarity is finite."""
    ids, sims = _lists(ids, sims)
    init = _points(init, "init")
    n = ids.shape[0]
    if init.shape[0] != n:
        raise ValueError(f"the lists have {n} rows, init {init.shape[0]}")
    messages: List[str] = []
    finite = np.isfinite(init).all(axis=1)
    inside = (ids >= 0) & (ids < n)
    usable = inside & np.isfinite(sims) & finite[np.where(inside, ids, 0)] & finite[:, None]
    listed = np.zeros(n, bool)
    listed[ids[usable]] = True
    lonely = finite & ~usable.any(axis=1) & ~listed
    keep = finite & ~lonely
    if (~finite).any():
        messages.append(f"{int((~finite).sum())} windows have no finite start position and are left off the map")
    if lonely.any():
        messages.append(f"{int(lonely.sum())} windows have no usable neighbour, are in nobody's list and are left off the map")
    new_id = np.full(n, -1, np.int32)
    new_id[keep] = np.arange(int(keep.sum()), dtype=np.int32)
    target = np.where(inside, ids, 0)
    kept_ids = np.where(inside & keep[target], new_id[target], -1)      # (an entry without a finite similarity stays: it is not used)
    return keep, np.ascontiguousarray(kept_ids[keep], np.int32), np.ascontiguousarray(sims[keep]), messages


# ---------------------------------------------------------------------------------------------------- device
class TSNE(_Device):
    """Exact t-SNE on the device.  ``fit(graph, init)``: ``graph`` is a ``KnnGraph`` or lists ``(ids, sims)`` [N, k] with cosine
    similarities; ``init`` float32 [N, 2] is where the windows start.  The lists are calibrated to ``schedule.perplexity``
    (``bd_tsne_affinities``), made symmetric on the host (``joint_probabilities``), and ``schedule.n_iter`` iterations of
    attraction, all-pairs repulsion and update are enqueued with no read-back between them.

    After ``fit``: ``coords`` float32 [N, 2] (NaN for a row left out, see ``leave_out``), ``kl_``, ``kl_history`` (one
    (iteration, kl) per ``report_every`` iterations), ``beta_`` [N], ``joint_`` (the P of the rows that took part), ``keep_``,
    ``messages``."""

    def __init__(self, schedule: Optional[Schedule] = None, device=None):
        super().__init__(device)
        self.schedule = schedule or Schedule()
        self.coords = self.beta_ = self.joint_ = self.keep_ = None
        self.kl_ = float("nan")
        self.kl_history: List[Tuple[int, float]] = []
        self.messages: List[str] = []

    def _workspace(self, nbytes: int):
        return self._empty((max(int(nbytes), 16),), _torch().uint8)

    def affinities(self, ids, sims) -> Tuple[np.ndarray, np.ndarray]:
        """``bd_tsne_affinities`` on lists [N, k]: (p float32 [N, k], beta float32 [N])."""
        torch = _torch()
        ids, sims = _lists(ids, sims)
        if self.device is None:
            self._open()
        n, k = ids.shape
        p, beta = self._empty((n, k), torch.float32), self._empty((n,), torch.float32)
        ids_dev, sims_dev = self._tensor(ids, torch.int32), self._tensor(sims, torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_tsne_affinities(ids_dev.data_ptr(), sims_dev.data_ptr(), n, k, float(self.schedule.perplexity),
                                                    p.data_ptr(), beta.data_ptr(), self._stream()))
        return p.cpu().numpy(), beta.cpu().numpy()

    def fit(self, graph, init, report_every: Optional[int] = None) -> np.ndarray:
        """Lays the windows out and returns ``coords``; ``kl_`` and the other results are set."""
        torch = _torch()
        ids, sims = (graph.ids, graph.sims) if isinstance(graph, KnnGraph) else graph
        ids, sims = _lists(ids, sims)
        self.schedule.check_k(ids.shape[1])
        init = _points(init, "init")
        keep, ids_c, sims_c, self.messages = leave_out(ids, sims, init)
        self._open()
        n_all, n = ids.shape[0], int(keep.sum())
        self.keep_ = keep
        self.coords = np.full((n_all, 2), np.nan, np.float32)
        self.beta_ = np.zeros(n_all, np.float32)
        self.kl_, self.kl_history = float("nan"), []
        self.joint_ = JointGraph(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
        if n == 0:
            return self.coords
        p, beta = self.affinities(ids_c, sims_c)
        self.beta_[keep] = beta
        joint = self.joint_ = joint_probabilities(ids_c, p)
        edges = joint.n_edges
        s = self.schedule
        rate = s.rate(n)
        row_start = self._tensor(joint.row_start, torch.int64)
        nbr, big = self._tensor(joint.nbr, torch.int32), self._tensor(joint.P, torch.float32)
        y, v, gain = (self._empty((n, 2), torch.float32) for _ in range(3))
        y.copy_(torch.from_numpy(init[keep]))
        v.zero_()
        gain.fill_(1.0)
        attr, rep, z = self._empty((n, 2), torch.float32), self._empty((n, 2), torch.float32), self._empty((n,), torch.float32)
        total, kl = self._empty((1,), torch.float32), self._empty((1,), torch.float32)
        nbytes = _lib.check(self._lib.bd_tsne_workspace_bytes(n))
        ws = self._workspace(nbytes)
        lib, stream = self._lib, self._stream()

        def repulse():
            _lib.check(lib.bd_tsne_repulse(y.data_ptr(), n, rep.data_ptr(), z.data_ptr(), ws.data_ptr(), nbytes, stream))

        def divergence() -> float:
            repulse()
            _lib.check(lib.bd_tsne_kl(row_start.data_ptr(), nbr.data_ptr(), big.data_ptr(), n, edges, y.data_ptr(), z.data_ptr(),
                                      kl.data_ptr(), ws.data_ptr(), nbytes, stream))
            return float(kl.item())                       # read back only when asked

        with torch.cuda.device(self.device):
            for it in range(int(s.n_iter)):
                exaggeration, momentum = s.at(it)
                _lib.check(lib.bd_tsne_attract(row_start.data_ptr(), nbr.data_ptr(), big.data_ptr(), n, edges, y.data_ptr(),
                                               attr.data_ptr(), stream))
                repulse()
                _lib.check(lib.bd_tsne_update(y.data_ptr(), v.data_ptr(), gain.data_ptr(), attr.data_ptr(), rep.data_ptr(),
                                              z.data_ptr(), n, exaggeration, momentum, rate, float(s.min_gain), total.data_ptr(),
                                              ws.data_ptr(), nbytes, stream))
                if report_every and (it + 1) % int(report_every) == 0:
                    self.kl_history.append((it + 1, divergence()))
            if int(s.n_iter) == 0:                        # attr and total are outputs like the others: every word is written
                attr.zero_()
                total.zero_()
            self.kl_ = divergence()
        self.coords[keep] = y.cpu().numpy()
        return self.coords


# ---------------------------------------------------------------------------------------------------- results
@dataclass
class _Labels:
    """What ``LayoutResult.load`` keeps of the clusters: a label per window."""
    labels: np.ndarray


@dataclass
class LayoutResult:
    """The windows of a folder on the map.  Window i lies in recording ``recordings[recording_of[i]]`` at ``starts[i]``
    (``analyze``'s start column for it), at ``coords[i]`` (NaN for a window left off the map, named in ``messages``); ``kl`` is
    the divergence of the map from the calibrated lists, ``graph`` the lists themselves."""
    coords: np.ndarray
    kl: float
    graph: Optional[KnnGraph]
    recordings: List[str]
    recording_of: np.ndarray
    starts: np.ndarray
    messages: List[str] = field(default_factory=list)
    clusters: Optional[object] = None
    framelength_s: float = FRAMELENGTH_S

    def __post_init__(self):
        self.coords = np.asarray(self.coords, np.float32)
        self.recording_of = np.asarray(self.recording_of, np.int64)
        self.starts = np.asarray(self.starts, np.float64)
        n = self.coords.shape[0]
        if self.coords.ndim != 2 or self.coords.shape[1] != 2 or not (self.recording_of.shape == self.starts.shape == (n,)):
            raise ValueError("coords must be [W, 2]; recording_of and starts must have one entry per window")

    def _window(self, i: int) -> Tuple[str, float]:
        return self.recordings[int(self.recording_of[i])], float(self.starts[i])

    def to_csv(self, path: str, clusters=None) -> None:
        """One row per window in the order of the walk: ``ident,start,end,x,y`` (end = start + 0.96 s), and ``cluster`` behind
        them when ``clusters`` (or else ``self.clusters``) is the ``ClusterResult`` of the same walk."""
        n = self.coords.shape[0]
        clusters = self.clusters if clusters is None else clusters
        if clusters is not None and np.asarray(clusters.labels).shape != (n,):
            raise ValueError(f"clusters holds {np.asarray(clusters.labels).shape[0]} windows, the map {n}: not the same walk")
        with open(path, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(list(LAYOUT_COLUMNS) + (["cluster"] if clusters is not None else []))
            for i in range(n):
                ident, start = self._window(i)
                out.writerow([ident, repr(start), repr(_end(start, self.framelength_s))] + [repr(float(c)) for c in self.coords[i]]
                             + ([int(clusters.labels[i])] if clusters is not None else []))

    def preservation(self, k: int = 10, sample: int = 2048, seed: int = 0) -> float:
        """The mean share of a window's ``k`` best list entries among its ``k`` nearest neighbours on the map, over a seeded
        sample of at most ``sample`` windows that are on the map; brute force in NumPy."""
        if self.graph is None:
            raise ValueError("the result holds no graph")
        on = np.flatnonzero(np.isfinite(self.coords).all(axis=1))
        if on.size < 2:
            return float("nan")
        pick = on if on.size <= int(sample) else np.sort(np.random.default_rng(seed).permutation(on)[:int(sample)])
        y = self.coords.astype(np.float64)
        d = ((y[pick][:, None, :] - y[on][None, :, :]) ** 2).sum(axis=2)
        d[on[None, :] == pick[:, None]] = np.inf
        k_map = min(int(k), on.size - 1)
        near = on[np.argsort(d, axis=1, kind="stable")[:, :k_map]]
        shares = []
        for row, i in enumerate(pick):
            best = self.graph.ids[i, :int(k)]
            best = best[best >= 0]
            if best.size:
                shares.append(np.isin(best, near[row]).sum() / best.size)
        return float(np.mean(shares)) if shares else float("nan")

    def save(self, path: str) -> None:
        g = self.graph
        with open(path, "wb") as f:
            np.savez(f, coords=self.coords, kl=np.float64(self.kl), recordings=np.array(self.recordings, dtype=str),
                     recording_of=self.recording_of, starts=self.starts, messages=np.array(self.messages, dtype=str),
                     framelength_s=np.float64(self.framelength_s), has_graph=np.array(g is not None),
                     ids=g.ids if g is not None else np.zeros((0, 0), np.int32),
                     sims=g.sims if g is not None else np.zeros((0, 0), np.float32),
                     metric=np.array(g.metric if g is not None else "cosine"), has_clusters=np.array(self.clusters is not None),
                     cluster_labels=np.asarray(self.clusters.labels if self.clusters is not None else np.zeros(0, np.int32)))

    @classmethod
    def load(cls, path: str) -> "LayoutResult":
        with np.load(path, allow_pickle=False) as z:
            recordings = [str(r) for r in z["recordings"]]
            graph = KnnGraph(z["ids"], z["sims"], recordings, z["recording_of"], z["starts"], str(z["metric"]), [],
                             float(z["framelength_s"])) if bool(z["has_graph"]) else None
            clusters = _Labels(np.asarray(z["cluster_labels"])) if bool(z["has_clusters"]) else None
            return cls(z["coords"], float(z["kl"]), graph, recordings, z["recording_of"], z["starts"], [str(m) for m in z["messages"]],
                       clusters, float(z["framelength_s"]))


def _check_clusters(clusters, n: int) -> None:
    if clusters is not None and np.asarray(clusters.labels).shape != (n,):
        raise ValueError(f"clusters holds {np.asarray(clusters.labels).shape[0]} windows, the folder {n}: not the same walk")


def scaled_start(coords) -> np.ndarray:
    """Coordinates scaled in float64 so that the first one's standard deviation is 1e-4, as float32; rows that are not finite
    stay out of the deviation.  Where there is no deviation to scale by the coordinates are returned as they are."""
    y = np.asarray(coords, np.float64)
    ok = np.isfinite(y).all(axis=1)
    std = y[ok, 0].std() if ok.any() else 0.0
    return (y / std * 1e-4).astype(np.float32) if np.isfinite(std) and std > 0 else y.astype(np.float32)


def layout_graph(graph: KnnGraph, init=None, seed: int = 0, schedule: Optional[Schedule] = None, device=None,
                 report_every: Optional[int] = None) -> LayoutResult:
    """The map of a saved ``KnnGraph`` (cosine) without its rows.  ``init`` None: seeded normal x 1e-4."""
    if graph.metric != "cosine":
        raise ValueError(f"the map takes cosine lists, not {graph.metric!r}")
    n = graph.ids.shape[0]
    if init is None:
        init = (np.random.default_rng(seed).normal(size=(n, 2)) * 1e-4).astype(np.float32)
    t = TSNE(schedule, device=device)
    t.fit(graph, init, report_every=report_every)
    return LayoutResult(t.coords, t.kl_, graph, list(graph.recordings), graph.recording_of, graph.starts,
                        list(graph.messages) + t.messages, None, graph.framelength_s)


def layout_recordings(source, *, k: int = 48, schedule: Optional[Schedule] = None, seed: int = 0, max_windows: int = 1 << 18,
                      clusters=None, engine=None, framehop_prop: float = 1.0, chunklength: float = 200,
                      embeddername: str = "yamnet_k2") -> LayoutResult:
    """The neighbour-preserving map of every window under ``source`` (a folder of recordings or an embedding store).  The
    windows are walked once and stay resident on the device as ``pca.map_recordings`` and ``propagate.neighbour_graph`` hold
    them (more than ``max_windows`` windows are refused the same way); the lists are ``Neighbours(k, "cosine")``; the start is
    their PCA plane (``pca.PCA(2)`` as ``pca.map_recordings`` fits it, ``seed`` drawing its sample where the folder holds more
    than 262144 windows) scaled to a standard deviation of 1e-4; ``TSNE(schedule)`` lays them out.  ``clusters``: the ``ClusterResult`` of the same walk, kept on the
    result so that ``to_csv`` writes a label per window; one of another length is refused."""
    from . import pca
    schedule = schedule or Schedule()
    schedule.check_k(int(k))
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        rows, index = _resident(source, engine, framehop_prop, chunklength, max_windows, messages)
        n = int(rows.shape[0])
        _check_clusters(clusters, n)
        graph = _graph_of(rows, index, int(k), "cosine", messages)
        if n >= 2:
            p = pca.PCA(2, device=engine.device).fit(rows, fit_rows=262144, seed=seed)
            init = scaled_start(p.transform(rows))
        else:
            init = np.zeros((n, 2), np.float32)
        del rows
        t = TSNE(schedule, device=engine.device)
        t.fit(graph, init)
        return LayoutResult(t.coords, t.kl_, graph, list(graph.recordings), graph.recording_of, graph.starts, messages + t.messages,
                            clusters)
    finally:
        if own:
            engine.close()
