"""Search recordings by example: the windows of a folder that sound most like a few given ones, or that a model scores
highest for a class - the step before there is an ``annotations.csv``.

    Searcher                  queries on the device, ``update(embeddings)`` per pass, ``result()``: the k best per query
    search_recordings         a folder of recordings against queries -> SearchResult
    top_windows               a folder of recordings through a model -> the k highest (or lowest) windows per class
    queries_from_annotations  the embeddings of the windows that carry a label, each or as their mean
    SearchResult              ``hits``, ``to_csv``, ``annotations`` (rows ``dataset.read_annotations`` reads)

The scores and the running top-k are computed where the embeddings lie (``include/buzzdetect_search.h``, csrc/simsearch.hip): no
``[W, 1024]`` rows go back to the host, only ``[Q, k]`` keys at the end.  The recordings are found, read, resampled and embedded
by ``dataset``'s helpers, that is as ``analyze`` does it, in the straight loop of ``dataset.embed_annotated`` (not ``Pipeline``'s
threads); a hit's ``start`` is the value ``analyze`` writes in that window's row.

    from buzzdetect_amd import dataset, search, train

    queries = search.queries_from_annotations("audio_in", "few.csv", "ins_buzz")          # a handful of marked buzzes
    found = search.search_recordings("audio_in", queries, k=200)
    found.to_csv("hits.csv")                                                               # review; delete the wrong rows
    found.annotations("ins_buzz", path="more.csv")                                         # ident,start,end,label
    more = dataset.embed_annotated("audio_in", "more.csv", ["ambient", "ins_buzz"], background="ambient")
"""
from __future__ import annotations

import bisect
import csv
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, framing
from .dataset import (DIGITS_TIME, FRAMELENGTH_S, _as_annotations, _embed_parts, _launch_sets, _open_engine, _part_windows,
                      _sources, _stored, _torch, embed_annotated)

HIT_COLUMNS = ("query", "rank", "ident", "start", "end", "score")
ANNOTATION_COLUMNS = ("ident", "start", "end", "label")


# ---------------------------------------------------------------------------------------------------- host helpers
def pack_queries(queries: np.ndarray) -> np.ndarray:
    """``bd_search_pack_queries``: float32 [Q, 1024] -> the matrix instruction's fragment order (host only)."""
    lib = _lib.load()
    q = np.ascontiguousarray(queries, np.float32)
    if q.ndim != 2 or q.shape[1] != _lib.SEARCH_DIM:
        raise ValueError(f"queries must be [Q, {_lib.SEARCH_DIM}], not {list(q.shape)}")
    packed = np.zeros(_lib.check(lib.bd_search_packed_floats(q.shape[0])), np.float32)
    _lib.check(lib.bd_search_pack_queries(q.ctypes.data, q.shape[0], packed.ctypes.data))
    return packed


def norms_host(e: np.ndarray) -> np.ndarray:
    """``bd_search_norms_host``: the squared norm of every row, in the device's order of operations."""
    e = np.ascontiguousarray(e, np.float32)
    if e.ndim != 2 or e.shape[1] != _lib.SEARCH_DIM:
        raise ValueError(f"rows must be [W, {_lib.SEARCH_DIM}], not {list(e.shape)}")
    n2 = np.zeros(e.shape[0], np.float32)
    _lib.check(_lib.load().bd_search_norms_host(e.ctypes.data, e.shape[0], n2.ctypes.data))
    return n2


def update_host(keys: np.ndarray, scores: np.ndarray, base_id: int) -> np.ndarray:
    """``bd_search_update_host`` in place on ``keys`` (uint64 [Q, k], C order) with ``scores`` (float32 [W, Q], any strides)."""
    if keys.dtype != np.uint64 or keys.ndim != 2 or not keys.flags.c_contiguous:
        raise ValueError("keys must be a C-contiguous uint64 [Q, k] array")
    if scores.dtype != np.float32 or scores.ndim != 2 or scores.shape[1] != keys.shape[0]:
        raise ValueError("scores must be float32 [W, Q]")
    rs, cs = (s // 4 for s in scores.strides) if scores.size else (keys.shape[0], 1)
    _lib.check(_lib.load().bd_search_update_host(scores.ctypes.data, scores.shape[0], keys.shape[0], rs, cs, int(base_id),
                                                 keys.ctypes.data, keys.shape[1]))
    return keys


def decode_keys(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
    """``bd_search_decode_host``: (scores float32, ids uint32, number of real keys) in the shape of ``keys``; an empty slot
    reads (-inf, 0xFFFFFFFF)."""
    keys = np.ascontiguousarray(keys, np.uint64)
    scores, ids = np.zeros(keys.shape, np.float32), np.zeros(keys.shape, np.uint32)
    real = _lib.check(_lib.load().bd_search_decode_host(keys.ctypes.data, keys.size, scores.ctypes.data, ids.ctypes.data))
    return scores, ids, real


def decode_result(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """A state (uint64 [Q, k]) as (scores float32 [Q, k'], ids int64 [Q, k']), best first, empty slots left out: every query
    has seen the same rows, so every row of the state holds the same number k' of real keys, in front."""
    keys = np.ascontiguousarray(keys, np.uint64)
    scores, ids, _ = decode_keys(keys)
    filled = (keys != 0).sum(axis=1)
    if filled.size and (filled != filled[0]).any():
        raise ValueError("the queries of one state hold different numbers of hits")
    n = int(filled[0]) if filled.size else 0
    return scores[:, :n].copy(), ids[:, :n].astype(np.int64)


def normalise_queries(queries, metric: str) -> np.ndarray:
    """float32 [Q, 1024] as the scorer takes them: for ``cosine`` every row brought to unit length in float64 (a zero row
    stays zero), then cast."""
    if metric not in _lib.SEARCH_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.SEARCH_METRICS)}, not {metric!r}")
    if type(queries).__module__.split(".")[0] == "torch":
        queries = queries.detach().cpu().numpy()
    q = np.asarray(queries, np.float64)
    if q.ndim == 1:
        q = q[None, :]
    if q.ndim != 2 or q.shape[1] != _lib.SEARCH_DIM or not 1 <= q.shape[0] <= _lib.SEARCH_MAX_QUERIES:
        raise ValueError(f"queries must be [1..{_lib.SEARCH_MAX_QUERIES}, {_lib.SEARCH_DIM}], not {list(q.shape)}")
    if metric == "cosine":
        length = np.sqrt((q * q).sum(axis=1, keepdims=True))
        q = np.divide(q, length, out=np.zeros_like(q), where=length > 0)
    return np.ascontiguousarray(q.astype(np.float32))


# ---------------------------------------------------------------------------------------------------- the searcher
class Searcher:
    """The k best windows per query over any number of passes.  ``queries``: [Q, 1024] (NumPy or tensor), normalised
    (``normalise_queries``), packed and uploaded once; ``queries=None`` with ``n_queries=Q`` gives a selector for
    ``update_scores`` alone.  Ids count the rows fed so far, from 0.  Everything runs on the current stream of ``device``."""

    def __init__(self, queries=None, k: int = 100, metric: str = "cosine", device=None, n_queries: Optional[int] = None):
        torch = _torch()
        self._lib = _lib.load()
        if not 1 <= int(k) <= _lib.SEARCH_MAX_K:
            raise ValueError(f"k must be in 1..{_lib.SEARCH_MAX_K}, not {k}")
        if metric not in _lib.SEARCH_METRICS:
            raise ValueError(f"metric must be one of {sorted(_lib.SEARCH_METRICS)}, not {metric!r}")
        self.k, self.metric = int(k), metric
        self.queries = None if queries is None else normalise_queries(queries, metric)
        if self.queries is None and n_queries is None:
            raise ValueError("give queries, or n_queries for a selector of ready-made scores")
        self.n_queries = int(n_queries) if self.queries is None else self.queries.shape[0]
        if not 1 <= self.n_queries <= _lib.SEARCH_MAX_QUERIES:
            raise ValueError(f"the number of queries must be in 1..{_lib.SEARCH_MAX_QUERIES}, not {self.n_queries}")
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; the searcher has no CPU path")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        self._packed = None if self.queries is None else torch.from_numpy(pack_queries(self.queries)).to(self.device)
        self._keys = self._empty((self.n_queries, self.k), torch.int64).zero_()                         # (uint64 bit patterns)
        self.seen = 0

    def _empty(self, shape, dtype):
        """Every device buffer the kernels write comes from here (the tests put guard words around them)."""
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def close(self) -> None:
        self._packed = self._keys = None

    def _stream(self):
        return _torch().cuda.current_stream(self.device)

    def _check_rows(self, embeddings):
        torch = _torch()
        e = embeddings
        if (not isinstance(e, torch.Tensor) or e.dim() != 2 or e.shape[1] != _lib.SEARCH_DIM or e.dtype != torch.float32
                or e.device != self.device or not e.is_contiguous() or e.data_ptr() % 16):
            raise ValueError(f"embeddings must be a contiguous, 16-byte aligned float32 [W, {_lib.SEARCH_DIM}] tensor on {self.device}")
        if self._packed is None:
            raise RuntimeError("this Searcher was made without queries: it takes update_scores only")
        return e

    def _score(self, e, out, row_stride: int, col_stride: int) -> None:
        torch = _torch()
        w = int(e.shape[0])
        stream = self._stream()
        with torch.cuda.device(self.device):
            n2 = None
            if self.metric == "cosine":
                n2 = self._empty((w,), torch.float32)
                _lib.check(self._lib.bd_search_norms(e.data_ptr(), w, n2.data_ptr(), stream.cuda_stream))
            _lib.check(self._lib.bd_search_scores(e.data_ptr(), w, self._packed.data_ptr(), self.n_queries,
                                                  _lib.SEARCH_METRICS[self.metric], n2.data_ptr() if n2 is not None else None,
                                                  out.data_ptr(), row_stride, col_stride, stream.cuda_stream))
        for t in (e, out) + ((n2,) if n2 is not None else ()):
            t.record_stream(stream)

    def scores(self, embeddings):
        """The device float32 [W, Q] scores of these rows; the state is not touched."""
        torch = _torch()
        e = self._check_rows(embeddings)
        out = self._empty((int(e.shape[0]), self.n_queries), torch.float32)
        if e.shape[0]:
            self._score(e, out, self.n_queries, 1)
        return out

    def _select(self, scores, w: int, row_stride: int, col_stride: int) -> int:
        torch = _torch()
        first = self.seen
        stream = self._stream()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_search_update(scores.data_ptr(), w, self.n_queries, row_stride, col_stride, first,
                                                  self._keys.data_ptr(), self.k, stream.cuda_stream))
        scores.record_stream(stream)
        self.seen += w
        return first

    def update(self, embeddings) -> int:
        """Norms, scores and selection over a device [W, 1024] tensor; the ids of its rows are ``seen .. seen + W - 1``.
        Returns the first of them."""
        torch = _torch()
        e = self._check_rows(embeddings)
        w = int(e.shape[0])
        if w > _lib.SEARCH_MAX_WINDOWS:
            raise ValueError(f"a pass takes at most {_lib.SEARCH_MAX_WINDOWS} rows, not {w}")
        if w == 0:
            return self.seen
        qmajor = self._empty((self.n_queries, w), torch.float32)                               # the selector reads along w
        self._score(e, qmajor, 1, w)
        return self._select(qmajor, w, 1, w)

    def update_scores(self, scores) -> int:
        """Selection alone over a device float32 [W, Q] tensor of any strides (logits, say).  Returns the first id."""
        torch = _torch()
        s = scores
        if (not isinstance(s, torch.Tensor) or s.dim() != 2 or s.shape[1] != self.n_queries or s.dtype != torch.float32
                or s.device != self.device):
            raise ValueError(f"scores must be a float32 [W, {self.n_queries}] tensor on {self.device}")
        w = int(s.shape[0])
        if w == 0:
            return self.seen
        if s.stride(0) == 0 or s.stride(1) == 0:
            s = s.contiguous()
        return self._select(s, w, int(s.stride(0)), int(s.stride(1)))

    def keys(self) -> np.ndarray:
        """The state as it is: uint64 [Q, k], best first, 0 where a slot is empty (waits for the stream)."""
        return self._keys.cpu().numpy().view(np.uint64)

    def result(self) -> Tuple[np.ndarray, np.ndarray]:
        """(scores float32 [Q, k'], ids int64 [Q, k']), best first, k' = min(k, rows seen)."""
        scores, ids = decode_result(self.keys())
        assert scores.shape[1] == min(self.k, self.seen)
        return scores, ids


# ---------------------------------------------------------------------------------------------------- results
@dataclass
class SearchResult:
    """``hits[q]``: (ident, start, score) of query q's windows, best first; ``start`` is ``analyze``'s start column for the
    window.  ``names[q]``: what the query is called in ``to_csv`` (its index, or the class for ``top_windows``)."""
    hits: List[List[Tuple[str, float, float]]]
    messages: List[str] = field(default_factory=list)
    names: Optional[List[str]] = None
    framelength_s: float = FRAMELENGTH_S

    def _name(self, q: int) -> str:
        return str(q) if self.names is None else str(self.names[q])

    def to_csv(self, path: str) -> None:
        """One row per hit: ``query,rank,ident,start,end,score`` (rank from 0, end = start + 0.96 s)."""
        with open(path, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(HIT_COLUMNS)
            for q, rows in enumerate(self.hits):
                for rank, (ident, start, score) in enumerate(rows):
                    out.writerow([self._name(q), rank, ident, repr(float(start)), repr(_end(start, self.framelength_s)),
                                  repr(float(score))])

    def annotations(self, labels, length: float = FRAMELENGTH_S, path: Optional[str] = None) -> List[Tuple[str, float, float, str]]:
        """The hits as annotation rows (ident, start, end = start + ``length``, label), in the order of ``hits``; a window
        several queries found under one label is listed once.  ``labels``: one label for every query, or one per query.
        ``path``: also written there, in the format ``dataset.read_annotations`` reads."""
        if isinstance(labels, str):
            labels = [labels] * len(self.hits)
        labels = [str(l) for l in labels]
        if len(labels) != len(self.hits):
            raise ValueError(f"{len(labels)} labels for {len(self.hits)} queries")
        if not length > 0:
            raise ValueError("length must be positive")
        rows, seen = [], set()
        for label, found in zip(labels, self.hits):
            for ident, start, _ in found:
                row = (ident, float(start), _end(start, length), label)
                if row not in seen:
                    seen.add(row)
                    rows.append(row)
        if path is not None:
            with open(path, "w", newline="") as f:
                out = csv.writer(f)
                out.writerow(ANNOTATION_COLUMNS)
                for ident, start, end, label in rows:
                    out.writerow([ident, repr(start), repr(end), label])
        return rows


def _end(start: float, length: float) -> float:
    return round(float(start) + float(length), 6)


class _Index:
    """Window id -> (ident, start): per recording the id of its first window, its chunks' left edges and window counts."""

    def __init__(self, framehop_s: float):
        self.framehop_s = framehop_s
        self.first: List[int] = []
        self.idents: List[str] = []
        self.chunks: List[Tuple[np.ndarray, List[float], List[int]]] = []

    def add(self, ident: str, first_id: int, starts_s: Sequence[float], counts: Sequence[int]) -> None:
        self.first.append(int(first_id))
        self.idents.append(ident)
        self.chunks.append((np.cumsum([0] + list(counts)), list(starts_s), list(counts)))

    def lookup(self, wid: int) -> Tuple[str, float]:
        r = bisect.bisect_right(self.first, int(wid)) - 1
        edges, starts_s, counts = self.chunks[r]
        local = int(wid) - self.first[r]
        c = int(np.searchsorted(edges, local, side="right")) - 1
        start = framing.window_starts(counts[c], starts_s[c], self.framehop_s, DIGITS_TIME)[local - int(edges[c])]
        return self.idents[r], float(start)

    def result(self, scores: np.ndarray, ids: np.ndarray, messages, names=None, sign: float = 1.0) -> SearchResult:
        hits = [[(*self.lookup(i), float(sign * s)) for s, i in zip(srow, irow)] for srow, irow in zip(scores, ids)]
        return SearchResult(hits, list(messages), names)


def _walk(dir_audio: str, engine, framehop_prop: float, chunklength: float, messages: List[str], feed, recording_done=None,
          recording_starts=None, annotations=None, only_annotated: bool = False) -> _Index:
    """embed_annotated's loop: every recording analyze would take, launch set by launch set.  ``feed(parts, hop, step)`` runs
    one set, hands its rows to a Searcher and returns (first id, windows per part); the rows are dropped before the next.
    ``recording_done(ident, chunk starts, windows per chunk)``, if given, is called after a recording's last set,
    ``recording_starts(ident, chunk starts)`` before its first.  ``annotations`` / ``only_annotated``: as embed_annotated
    takes them (recordings the annotations do not mention are left out; annotated ones that do not exist are reported).
    ``dir_audio`` may be an embedding store (``dataset._sources``): the parts are then handles on stored rows."""
    from .engine import hop_samples, patch_step
    framehop_s = FRAMELENGTH_S * framehop_prop
    hop, step = hop_samples(framehop_s), patch_step(framehop_s)
    chunklength = framing.round_chunklength(chunklength, FRAMELENGTH_S, DIGITS_TIME)
    index = _Index(framehop_s)
    for ident, chunks in _sources(dir_audio, engine, framehop_prop, chunklength, {} if annotations is None else annotations,
                                  only_annotated, messages):
        if recording_starts is not None:
            recording_starts(ident, [c.start_s for c in chunks])
        parts = [c.pcm for c in chunks]
        windows = [_part_windows(engine, p, hop, step) for p in parts]
        first_id, all_counts = None, []
        for a, b in _launch_sets(parts, windows):
            first, counts = feed(parts[a:b], hop, step)
            first_id = first if first_id is None else first_id
            all_counts += list(counts)
        index.add(ident, first_id, [c.start_s for c in chunks], all_counts)
        if recording_done is not None:
            recording_done(ident, [c.start_s for c in chunks], all_counts)
    return index


def search_recordings(dir_audio: str, queries, *, k: int = 100, metric: str = "cosine", engine=None, framehop_prop: float = 1.0,
                      chunklength: float = 200, embeddername: str = "yamnet_k2") -> SearchResult:
    """The ``k`` windows under ``dir_audio`` most similar to each row of ``queries`` ([Q, 1024] embeddings).  Every recording
    ``analyze`` would take is read, resampled and embedded as ``analyze(framehop_prop=..., chunklength=...)`` does it; each
    launch set's embeddings go to ``Searcher.update`` and are dropped, so one set's rows are alive at a time.  ``engine``: a
    ``HipEngine`` to use; else one is built for ``embeddername`` and closed."""
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        searcher = Searcher(queries, k=k, metric=metric, device=engine.device)

        def feed(parts, hop, step):
            emb, counts = _embed_parts(engine, parts, hop, step)
            return searcher.update(emb), counts

        index = _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed)
        scores, ids = searcher.result()
        searcher.close()
        return index.result(scores, ids, messages)
    finally:
        if own:
            engine.close()


def _logit_parts(engine, parts, hop: int, step: int):
    """``dataset._embed_parts`` for logits: one launch set, final (a set whose activations left the f16 range is repeated
    with exact-f32 products).  Parts of an embedding store: their stored rows through ``engine.score_rows``, the heads alone."""
    if _stored(parts):
        rows, counts = _embed_parts(engine, parts, hop, step)
        return engine.score_rows(rows), counts
    from .engine import LaunchVerdict
    f16 = engine._mode != "f32"
    verdict = LaunchVerdict(engine._stream()) if f16 else None
    _, logits, counts = engine.launch(parts, hop, step, want_embeddings=False, want_logits=True, verdict=verdict)
    if verdict is not None and verdict.wait():
        _, logits, counts = engine.launch(parts, hop, step, want_embeddings=False, want_logits=True, mode="f32")
        engine.overflow_reruns += 1
    return logits, counts


def top_windows(dir_audio: str, modelname: Optional[str] = "model_general_v3", *, classes: Optional[Sequence[str]] = None,
                k: int = 100, largest: bool = True, engine=None, framehop_prop: float = 1.0, chunklength: float = 200,
                embeddername: str = "yamnet_k2", models_dir: Optional[str] = None) -> SearchResult:
    """The ``k`` windows under ``dir_audio`` that model ``modelname`` scores highest (``largest=False``: lowest) for each of
    ``classes`` (default: all of the model's), by the model's output columns as ``analyze`` would write them before rounding.
    ``hits[c]`` belongs to ``classes[c]``.  ``engine``: a ``HipEngine`` that carries the model (``modelname`` is then not
    read)."""
    from .engine import HipEngine
    messages: List[str] = []
    own = engine is None
    if own:
        engine = HipEngine(embeddername=embeddername, modelname=modelname, models_dir=models_dir)
    try:
        if not engine.n_classes:
            raise ValueError("top_windows needs an engine with a classifier")
        names = list(engine.classes) if classes is None else [str(c) for c in classes]
        missing = [c for c in names if c not in engine.classes]
        if missing or not names:
            raise ValueError(f"classes {missing} are not among the model's {list(engine.classes)}" if missing else "no classes")
        torch = _torch()
        columns = torch.tensor([engine.classes.index(c) for c in names], dtype=torch.int64, device=engine.device)
        searcher = Searcher(None, k=k, device=engine.device, n_queries=len(names))

        def feed(parts, hop, step):
            logits, counts = _logit_parts(engine, parts, hop, step)
            picked = logits.index_select(1, columns)
            return searcher.update_scores(picked if largest else -picked), counts

        index = _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed)
        scores, ids = searcher.result()
        searcher.close()
        return index.result(scores, ids, messages, names, 1.0 if largest else -1.0)
    finally:
        if own:
            engine.close()


def queries_from_annotations(dir_audio: str, annotations, label: str, *, reduce: str = "each", engine=None,
                             embeddername: str = "yamnet_k2", **embed_kwargs) -> np.ndarray:
    """float32 [n, 1024]: the embeddings of the windows ``annotations`` label ``label`` (``dataset.embed_annotated`` over the
    annotated recordings, with its rules for which windows carry a label), as they are (``reduce="each"``) or as their float64
    mean cast to float32, one prototype (``"mean"``).  ``ValueError`` when no window carries the label."""
    if reduce not in ("each", "mean"):
        raise ValueError(f"reduce must be \"each\" or \"mean\", not {reduce!r}")
    notes = _as_annotations(annotations)
    classes = sorted({l for rows in notes.values() for _, _, l in rows})
    if label not in classes:
        raise ValueError(f"label {label!r} is not among the annotations' {classes}")
    ts = embed_annotated(dir_audio, notes, classes, engine=engine, embeddername=embeddername, only_annotated=True, **embed_kwargs)
    rows = np.flatnonzero(ts.targets[:, classes.index(label)] > 0)
    if rows.size == 0:
        raise ValueError(f"no window carries the label {label!r}")
    torch = _torch()
    emb = ts.embeddings.index_select(0, torch.from_numpy(rows).to(ts.embeddings.device)).cpu().numpy()
    if reduce == "mean":
        return emb.astype(np.float64).mean(axis=0, keepdims=True).astype(np.float32)
    return emb
