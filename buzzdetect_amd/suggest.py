"""Suggest the windows to annotate next: the ones a committee of models is least sure of, or disagrees most about, and among
those a batch that is not forty neighbouring windows of the same three buzzes - active learning, the step after the first fit.

    acquire_host / acquire_device   entropy, margin and BALD of every window from the members' logits
    pick_host / pick_device         k of n candidates, greedily: gain x cosine distance to everything picked so far
    Suggester                       ``update(rows)`` per launch set keeps the ``pool`` most uncertain windows AND their embeddings
                                    on the device; ``finish(k)`` picks the diverse batch
    suggest_recordings              a folder of recordings (or an embedding store) through a set of models -> Suggestion
    Suggestion                      ``hits``, ``pool``, ``to_csv``, ``annotations`` (rows ``dataset.read_annotations`` reads)

The scores, the running pool and the pick are computed where the logits and embeddings lie (``include/buzzdetect_suggest.h``,
csrc/suggest.hip; the pool is the selector of ``include/buzzdetect_search.h``); the recordings are walked ONCE, as ``search`` walks
them, and per launch set only the pool's 8 KB of keys come back to the host.

    from buzzdetect_amd import suggest

    found = suggest.suggest_recordings("audio_in", "folds_ensemble", k=100, strategy="bald", exclude="annotations.csv")
    found.to_csv("review.csv")                                     # rank,ident,start,end,score,novelty: listen, decide
    found.annotations(labels, path="more.csv")                     # one label per hit, None = skipped
"""
from __future__ import annotations

import csv
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, search, weights
from .dataset import EDGE_S, FRAMELENGTH_S, _as_annotations, _embed_parts, _torch

STRATEGIES = tuple(_lib.SUGGEST_STRATEGIES)                      # "entropy", "margin", "bald": the rows of an acquisition
HIT_COLUMNS = ("rank", "ident", "start", "end", "score", "novelty")


def _link_id(link) -> int:
    if link not in ("softmax", "sigmoid"):
        raise ValueError(f"link must be \"softmax\" or \"sigmoid\", not {link!r}")
    return _lib.LINKS[link]


def _members_array(member_first) -> np.ndarray:
    first = np.ascontiguousarray(member_first, np.int32)
    if first.ndim != 1:
        raise ValueError("member_first must be a list of column offsets")
    return first


# ---------------------------------------------------------------------------------------------------- the two entry points
def acquire_host(wide: np.ndarray, member_first, width: int, link: str = "softmax", target: Optional[int] = None) -> np.ndarray:
    """``bd_suggest_acquire_host``: float32 [3, W] (``STRATEGIES`` order) from ``wide`` float32 [W, ld], the members' columns
    side by side; member m's ``width`` logits start at column ``member_first[m]``.  ``target``: a column of the members, for
    the question "this class or not"; None: the whole distribution."""
    wide = np.ascontiguousarray(wide, np.float32)
    if wide.ndim != 2:
        raise ValueError(f"wide must be [W, ld], not {list(wide.shape)}")
    first = _members_array(member_first)
    w = wide.shape[0]
    out = np.zeros((len(STRATEGIES), w), np.float32)
    _lib.check(_lib.load().bd_suggest_acquire_host(wide.ctypes.data, w, wide.shape[1], first.ctypes.data, first.size, int(width),
                                                   _link_id(link), -1 if target is None else int(target), out.ctypes.data, w))
    return out


def _empty(shape, dtype, device):
    """Every device buffer a kernel of this module writes comes from here (the tests put guard words around them)."""
    return _torch().empty(shape, dtype=dtype, device=device)


def acquire_device(wide, member_first, width: int, link: str = "softmax", target: Optional[int] = None, out=None):
    """``bd_suggest_acquire`` on the current stream: ``wide`` a device float32 [W, ld] tensor with contiguous rows (what
    ``engine.predict`` / ``engine.score_rows`` of ``HipEngine(heads=...)`` give) -> device float32 [3, W].  ``out``: optional
    caller-owned [3, S >= W] rows to write the first W columns of."""
    torch = _torch()
    if not isinstance(wide, torch.Tensor) or wide.dim() != 2 or wide.dtype != torch.float32 or not wide.is_cuda or wide.stride(1) != 1 \
            or (wide.shape[0] > 1 and wide.stride(0) < wide.shape[1]):
        raise ValueError("wide must be a device float32 [W, ld] tensor with contiguous rows")
    first = _members_array(member_first)
    w = int(wide.shape[0])
    ld = int(wide.stride(0)) if w > 1 else int(wide.shape[1])
    if out is None:
        out = _empty((len(STRATEGIES), w), torch.float32, wide.device)
    elif (not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape[0] != len(STRATEGIES) or out.dtype != torch.float32
          or out.device != wide.device or out.stride(1) != 1):
        raise ValueError(f"out must be a float32 [{len(STRATEGIES)}, S] tensor on {wide.device}")
    stride = int(out.stride(0)) if out.shape[1] else w
    stream = torch.cuda.current_stream(wide.device)
    with torch.cuda.device(wide.device):
        _lib.check(_lib.load().bd_suggest_acquire(wide.data_ptr() if w else None, w, ld, first.ctypes.data, first.size, int(width),
                                                  _link_id(link), -1 if target is None else int(target),
                                                  out.data_ptr() if w else None, stride, stream.cuda_stream))
    wide.record_stream(stream)
    out.record_stream(stream)
    return out


def pick_host(sim: np.ndarray, gain: np.ndarray, d0: Optional[np.ndarray], k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``bd_suggest_pick_host``: (picked int32 [k], value float32 [k], dist float32 [k]) from ``sim`` float32 [n, ld >= n]
    (``sim[j, i]``: how similar candidate i is to candidate j), ``gain`` [n] and ``d0`` [n] or None (1 everywhere)."""
    sim = np.ascontiguousarray(sim, np.float32)
    gain = np.ascontiguousarray(gain, np.float32)
    if sim.ndim != 2 or gain.ndim != 1 or sim.shape[0] != gain.size:
        raise ValueError(f"sim must be [n, ld] and gain [n], not {list(sim.shape)} and {list(gain.shape)}")
    if d0 is not None:
        d0 = np.ascontiguousarray(d0, np.float32)
        if d0.shape != gain.shape:
            raise ValueError(f"d0 must be [{gain.size}] like gain, not {list(d0.shape)}")
    k = int(k)
    picked, value, dist = np.zeros(max(k, 0), np.int32), np.zeros(max(k, 0), np.float32), np.zeros(max(k, 0), np.float32)
    _lib.check(_lib.load().bd_suggest_pick_host(sim.ctypes.data, sim.shape[1], gain.ctypes.data, None if d0 is None else d0.ctypes.data,
                                                gain.size, k, picked.ctypes.data, value.ctypes.data, dist.ctypes.data))
    return picked, value, dist


def pick_device(sim, gain, d0, k: int, empty=None):
    """``bd_suggest_pick`` on the current stream: device tensors as ``pick_host`` takes arrays -> device (picked int32 [k],
    value float32 [k], dist float32 [k]).  ``empty(shape, dtype, device)``: the allocator of the three (default ``_empty``)."""
    torch = _torch()
    for name, t, dim in (("sim", sim, 2), ("gain", gain, 1)) + ((("d0", d0, 1),) if d0 is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dim() != dim or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous device float32 tensor of {dim} dimension(s)")
    n, k = int(gain.shape[0]), int(k)
    if sim.shape[0] != n or (d0 is not None and d0.shape[0] != n) or sim.device != gain.device:
        raise ValueError(f"sim must be [n, ld], gain and d0 [n]; got {list(sim.shape)}, {list(gain.shape)}")
    empty = _empty if empty is None else empty
    picked = empty((max(k, 0),), torch.int32, gain.device)
    value, dist = empty((max(k, 0),), torch.float32, gain.device), empty((max(k, 0),), torch.float32, gain.device)
    stream = torch.cuda.current_stream(gain.device)
    with torch.cuda.device(gain.device):
        _lib.check(_lib.load().bd_suggest_pick(sim.data_ptr(), int(sim.shape[1]), gain.data_ptr(), None if d0 is None else d0.data_ptr(),
                                               n, k, picked.data_ptr(), value.data_ptr(), dist.data_ptr(), stream.cuda_stream))
    for t in (sim, gain, picked, value, dist) + ((d0,) if d0 is not None else ()):
        t.record_stream(stream)
    return picked, value, dist


# ---------------------------------------------------------------------------------------------------- the members
def _committee(members: dict, link: str, target, strategy: str):
    """What a set of plain heads must be to vote (``ValueError`` names the member): shared classes, linear last layers, a
    width the kernel takes.  Returns (classes, target column or None)."""
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be one of {list(STRATEGIES)}, not {strategy!r}")
    _link_id(link)
    if not members:
        raise ValueError("no models given")
    first_name, first = next(iter(members.items()))
    for name, head in members.items():
        if isinstance(head, weights.EnsembleWeights):
            raise ValueError(f"member {name!r} is an ensemble: open it into its members (weights.expand_head_set)")
        if list(head.classes) != list(first.classes):
            raise ValueError(f"member {name!r} has classes {list(head.classes)}, member {first_name!r} {list(first.classes)}: "
                             "a committee votes on one set of classes")
        if head.layers[-1][2] != "linear":
            raise ValueError(f"member {name!r} ends in {head.layers[-1][2]!r}: the acquisition applies the {link} itself and takes "
                             "members whose last layer is linear")
    classes = list(first.classes)
    if len(members) > _lib.SUGGEST_MAX_MEMBERS or not 1 <= len(classes) <= _lib.SUGGEST_MAX_WIDTH:
        raise ValueError(f"{len(members)} members of {len(classes)} classes: at most {_lib.SUGGEST_MAX_MEMBERS} of 1.."
                         f"{_lib.SUGGEST_MAX_WIDTH} are taken")
    if strategy == "bald" and len(members) == 1:
        raise ValueError('strategy "bald" measures how the members disagree and is identically 0 for one model: use "entropy" or '
                         '"margin", or give several models (the folds of a cross-validation, an ensemble)')
    column = None
    if target is not None:
        if isinstance(target, str):
            if target not in classes:
                raise ValueError(f"target {target!r} is not among the classes {classes}")
            column = classes.index(target)
        else:
            column = int(target)
            if not 0 <= column < len(classes):
                raise ValueError(f"target {target} is outside the columns 0..{len(classes) - 1}")
    if link == "sigmoid" and column is None:
        raise ValueError('link "sigmoid" scores one class at a time: name a target')
    if link == "softmax" and len(classes) < 2:
        raise ValueError('link "softmax" needs at least 2 classes')
    return classes, column


class Suggester:
    """The ``pool`` most uncertain windows of any number of passes, with their embeddings, then a diverse batch of them.
    ``engine``: a ``HipEngine(heads={name: HeadWeights})`` - a set of plain heads, no ensemble attached - whose members share
    classes and end linear.  ``strategy``: "entropy", "margin" or "bald"; ``target``: a class (name or column) for the binary
    question, None for the whole distribution; ``link``: how the members' logits become probabilities.  Ids count the rows fed
    so far, from 0.  After ``finish`` the stages are kept for inspection: ``pool_ids`` / ``pool_scores`` (best first),
    ``pool_rows`` (device [n, 1024]), ``sim`` (device [n, n]) and ``d0`` (device [n] or None)."""

    def __init__(self, engine, *, strategy: str = "bald", target=None, pool: int = _lib.SUGGEST_MAX_POOL, link: str = "softmax"):
        torch = _torch()
        if getattr(engine, "members", None) is None or getattr(engine, "head", None) is not None:
            raise ValueError("a Suggester takes an engine with a set of heads (HipEngine(heads=...) or modelname=[...])")
        self.classes, self.target = _committee(engine.members, link, target, strategy)
        if not 1 <= int(pool) <= _lib.SUGGEST_MAX_POOL:
            raise ValueError(f"pool must be in 1..{_lib.SUGGEST_MAX_POOL}, not {pool}")
        self.engine, self.strategy, self.link, self.pool = engine, strategy, link, int(pool)
        self.device = engine.device
        self.member_first = np.array([cols.start for cols in engine.member_columns.values()], np.int32)
        self._row = _lib.SUGGEST_STRATEGIES[strategy]
        self._searcher = search.Searcher(None, k=self.pool, device=self.device, n_queries=1)
        self._rows = self._empty((self.pool, _lib.SEARCH_DIM), torch.float32)
        self._slot = {}                                           # window id -> its row of _rows
        self._free = list(range(self.pool - 1, -1, -1))
        self.pool_ids = self.pool_scores = self.pool_rows = self.sim = self.d0 = None

    def _empty(self, shape, dtype):
        return _empty(shape, dtype, self.device)

    def _alloc(self, shape, dtype, device):
        return self._empty(shape, dtype)

    @property
    def seen(self) -> int:
        return self._searcher.seen

    def close(self) -> None:
        self._searcher.close()
        self._rows = self.pool_rows = self.sim = self.d0 = None

    def acquire(self, rows):
        """The device float32 [3, W] acquisition scores of these embeddings (``engine.score_rows``, then
        ``bd_suggest_acquire``); the state is not touched."""
        torch = _torch()
        logits = self.engine.score_rows(rows)
        out = self._empty((len(STRATEGIES), int(rows.shape[0])), torch.float32)
        return acquire_device(logits, self.member_first, len(self.classes), self.link, self.target, out=out)

    def update(self, rows, exclude=None) -> int:
        """One launch set's embeddings (device float32 [W, 1024]): scored, ranked into the pool, and the rows that entered it
        copied beside it.  ``exclude``: a bool [W] mask (array or tensor) of windows that are no candidates.  Returns the id
        of the first row."""
        torch = _torch()
        w = int(rows.shape[0])
        if w == 0:
            return self.seen
        score = self.acquire(rows)[self._row]
        if exclude is not None:
            mask = torch.as_tensor(np.asarray(exclude, bool) if not isinstance(exclude, torch.Tensor) else exclude).to(self.device)
            if tuple(mask.shape) != (w,) or mask.dtype != torch.bool:
                raise ValueError(f"exclude must be a bool [{w}] mask")
            score = torch.where(mask, torch.full_like(score, float("-inf")), score)
        first = self._searcher.update_scores(score.view(w, 1))
        _, ids, _ = search.decode_keys(self._searcher.keys())    # 8 KB per pass; empty slots read 0xFFFFFFFF
        now = {int(i) for i in ids.ravel() if i != 0xFFFFFFFF}
        for wid in [i for i in self._slot if i not in now]:
            self._free.append(self._slot.pop(wid))
        entered = sorted(i for i in now if i not in self._slot)   # all of this pass: first <= id < first + W
        if entered:
            slots = [self._free.pop() for _ in entered]
            self._slot.update(zip(entered, slots))
            src = torch.tensor([i - first for i in entered], dtype=torch.int64, device=self.device)
            self._rows.index_copy_(0, torch.tensor(slots, dtype=torch.int64, device=self.device), rows.index_select(0, src))
        return first

    def finish(self, k: int, diversity: bool = True, avoid=None):
        """(ids int64 [k'], scores float32 [k'], novelty float32 [k']) of the batch, in pick order; k' = min(k, candidates).
        The pool in rank order, candidates at -inf dropped; their cosine similarities by ``bd_search_scores``; ``avoid``
        ([A, 1024] embeddings that are labelled already): every candidate's cosine distance to the nearest of them
        (``bd_cluster_assign`` in groups of 1024, negative roundings raised to 0) starts the distances; ``bd_suggest_pick``.
        ``diversity=False``: the first k of the pool, their novelty the starting distance."""
        torch = _torch()
        if int(k) < 1:
            raise ValueError(f"k must be at least 1, not {k}")
        lib = _lib.load()
        scores, ids = self._searcher.result()
        keep = scores[0] > -np.inf
        self.pool_scores, self.pool_ids = scores[0][keep].copy(), ids[0][keep].copy()
        n = int(self.pool_ids.size)
        self.pool_rows = self.sim = self.d0 = None
        if n == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32)
        k = min(int(k), n)
        order = torch.tensor([self._slot[int(i)] for i in self.pool_ids], dtype=torch.int64, device=self.device)
        rows = self.pool_rows = self._rows.index_select(0, order)
        stream = torch.cuda.current_stream(self.device)
        if avoid is not None:
            labelled = avoid.detach().cpu().numpy() if isinstance(avoid, torch.Tensor) else np.asarray(avoid, np.float32)
            labelled = np.ascontiguousarray(labelled, np.float32).reshape(-1, _lib.SEARCH_DIM)
            n2 = self._empty((n,), torch.float32)
            with torch.cuda.device(self.device):
                _lib.check(lib.bd_search_norms(rows.data_ptr(), n, n2.data_ptr(), stream.cuda_stream))
            for at in range(0, labelled.shape[0], _lib.CLUSTER_MAX_CLUSTERS):
                group = search.normalise_queries(labelled[at:at + _lib.CLUSTER_MAX_CLUSTERS], "cosine")
                packed = torch.from_numpy(search.pack_queries(group)).to(self.device)
                nearest, dist = self._empty((n,), torch.int32), self._empty((n,), torch.float32)
                with torch.cuda.device(self.device):
                    _lib.check(lib.bd_cluster_assign(rows.data_ptr(), n, n2.data_ptr(), packed.data_ptr(), None, group.shape[0],
                                                     _lib.CLUSTER_METRICS["cosine"], nearest.data_ptr(), dist.data_ptr(),
                                                     stream.cuda_stream))
                packed.record_stream(stream)
                self.d0 = dist if self.d0 is None else torch.minimum(self.d0, dist)
            if self.d0 is not None:
                self.d0 = self.d0.clamp_min(0.0).contiguous()
        if not diversity:
            novelty = np.ones(k, np.float32) if self.d0 is None else self.d0[:k].cpu().numpy()
            return self.pool_ids[:k].copy(), self.pool_scores[:k].copy(), novelty
        among = search.Searcher(rows.cpu().numpy(), k=1, metric="cosine", device=self.device)
        self.sim = self._empty((n, n), torch.float32)
        among._score(rows, self.sim, 1, n)                       # sim[j, i]: candidate i against unit candidate j
        among.close()
        gain = torch.from_numpy(self.pool_scores).to(self.device)
        picked, value, dist = pick_device(self.sim, gain, self.d0, k, empty=self._alloc)
        picked = picked.cpu().numpy()
        return self.pool_ids[picked], value.cpu().numpy(), dist.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- results
@dataclass
class Suggestion:
    """``hits``: (ident, start, score, novelty) in pick order - ``start`` is ``analyze``'s start column for the window, ``score``
    the acquisition discounted by ``novelty``, the window's cosine distance to everything picked before it (and to ``avoid``).
    ``pool``: (ident, start, score) of every candidate, most uncertain first, with the plain acquisition score."""
    hits: List[Tuple[str, float, float, float]]
    pool: List[Tuple[str, float, float]] = field(default_factory=list)
    messages: List[str] = field(default_factory=list)
    strategy: str = "bald"
    framelength_s: float = FRAMELENGTH_S

    def to_csv(self, path: str) -> None:
        """One row per hit: ``rank,ident,start,end,score,novelty`` (rank from 0, end = start + 0.96 s)."""
        with open(path, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(HIT_COLUMNS)
            for rank, (ident, start, score, novelty) in enumerate(self.hits):
                out.writerow([rank, ident, repr(float(start)), repr(search._end(start, self.framelength_s)), repr(float(score)),
                              repr(float(novelty))])

    def annotations(self, labels: Sequence[Optional[str]], path: Optional[str] = None,
                    length: float = FRAMELENGTH_S) -> List[Tuple[str, float, float, str]]:
        """The reviewer's verdicts as annotation rows (ident, start, end = start + ``length``, label): ``labels`` holds one
        label per hit, in order; None leaves the hit out.  ``path``: also written there, in the format
        ``dataset.read_annotations`` reads."""
        labels = list(labels)
        if len(labels) != len(self.hits):
            raise ValueError(f"{len(labels)} labels for {len(self.hits)} hits")
        if not length > 0:
            raise ValueError("length must be positive")
        rows = [(ident, float(start), search._end(start, length), str(label))
                for (ident, start, _, _), label in zip(self.hits, labels) if label is not None]
        if path is not None:
            with open(path, "w", newline="") as f:
                out = csv.writer(f)
                out.writerow(search.ANNOTATION_COLUMNS)
                for ident, start, end, label in rows:
                    out.writerow([ident, repr(start), repr(end), label])
        return rows


def _load_committee(models, models_dir: Optional[str], link: Optional[str]):
    """``models`` (a name, a list of names, an ensemble's name) as ({member name: HeadWeights}, link)."""
    names = [models] if isinstance(models, str) else list(models)
    loaded = weights.load_head_set(names, models_dir)
    if link is None:
        own = [h.link for h in loaded.values() if isinstance(h, weights.EnsembleWeights) and h.link is not None]
        link = own[0] if own else "softmax"
    return weights.expand_head_set(loaded), link


def _overlaps(starts: np.ndarray, intervals) -> np.ndarray:
    """Which windows [start, start + 0.96 s) meet one of the (start, end, label) intervals."""
    hit = np.zeros(starts.shape, bool)
    for a, b, _ in intervals:
        hit |= (starts < b - EDGE_S) & (starts + FRAMELENGTH_S > a + EDGE_S)
    return hit


def suggest_recordings(dir_audio, models=None, *, k: int = 100, strategy: str = "bald", target=None, pool: Optional[int] = None,
                       diversity: bool = True, exclude=None, avoid=None, link: Optional[str] = None, engine=None,
                       framehop_prop: float = 1.0, chunklength: float = 200, embeddername: str = "yamnet_k2",
                       models_dir: Optional[str] = None) -> Suggestion:
    """The ``k`` windows under ``dir_audio`` (recordings, or an embedding store of them) that are worth a reviewer's time.
    ``models``: a model's name, a list of names, or an ensemble's name - opened into its members, which run as one set of heads
    behind one embedder pass.  Every window is scored by ``strategy`` ("entropy": how flat the committee's mean distribution
    is; "margin": how close its two best classes are; "bald": how much the members disagree), for ``target`` (a class: the
    question "this or not") or the whole distribution.  The ``pool`` (default ``min(1024, 8 k)``) highest are kept with their
    embeddings, and the batch is picked from them greedily: each pick has the highest score x cosine distance to everything
    picked before it, so forty neighbouring windows of one ambiguous buzz yield one hit (``diversity=False``: the plain top
    k).  ``exclude``: annotations (a path, or what ``dataset.read_annotations`` returns) - a window that overlaps an annotated
    interval of its recording is no candidate.  ``avoid``: [A, 1024] embeddings that are labelled already
    (``TrainingSet.embeddings``) - windows close to them are discounted from the start.  ``link``: "softmax" or "sigmoid";
    default the ensemble's own, else "softmax".  ``engine``: a ``HipEngine(heads=...)`` that already carries the members
    (``models`` is then not read)."""
    from .engine import HipEngine
    if not 1 <= int(k) <= _lib.SUGGEST_MAX_POOL:
        raise ValueError(f"k must be in 1..{_lib.SUGGEST_MAX_POOL}, not {k}")
    k = int(k)
    pool = min(_lib.SUGGEST_MAX_POOL, 8 * k) if pool is None else int(pool)
    if not k <= pool <= _lib.SUGGEST_MAX_POOL:
        raise ValueError(f"pool must be in k..{_lib.SUGGEST_MAX_POOL} = {k}..{_lib.SUGGEST_MAX_POOL}, not {pool}")
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be one of {list(STRATEGIES)}, not {strategy!r}")
    if link is not None:
        _link_id(link)
    if not framehop_prop > 0:
        raise ValueError("framehop_prop must be positive")
    notes = {} if exclude is None else _as_annotations(exclude)
    if engine is None:
        if models is None:
            raise ValueError("give models (a name, a list of names, or an ensemble's name) or an engine that carries them")
        members, link = _load_committee(models, models_dir, link)
        _committee(members, link, target, strategy)               # host only: refused before any device work
    elif getattr(engine, "members", None) is None:
        raise ValueError("engine must carry a set of heads (HipEngine(heads=...)); or leave it out and name the models")
    else:
        link = "softmax" if link is None else link
        _committee(engine.members, link, target, strategy)
    messages: List[str] = []
    own = engine is None
    if own:
        engine = HipEngine(embeddername=embeddername, modelname=None, heads=members)
    try:
        suggester = Suggester(engine, strategy=strategy, target=target, pool=pool, link=link)
        framehop_s = FRAMELENGTH_S * framehop_prop
        at = {"ident": None, "starts": [], "next": 0}

        def recording_starts(ident, starts_s):
            at.update(ident=ident, starts=list(starts_s), next=0)

        def feed(parts, hop, step):
            emb, counts = _embed_parts(engine, parts, hop, step)
            mask = None
            if notes.get(at["ident"]):
                starts_s = at["starts"][at["next"]:at["next"] + len(parts)]
                exact = np.concatenate([s + np.arange(n, dtype=np.float64) * framehop_s for s, n in zip(starts_s, counts)])
                mask = _overlaps(exact, notes[at["ident"]])
            at["next"] += len(parts)
            return suggester.update(emb, exclude=mask), counts

        index = search._walk(dir_audio, engine, framehop_prop, chunklength, messages, feed, recording_starts=recording_starts)
        ids, scores, novelty = suggester.finish(k, diversity=diversity, avoid=avoid)
        hits = [(*index.lookup(i), float(s), float(d)) for i, s, d in zip(ids, scores, novelty)]
        candidates = [(*index.lookup(i), float(s)) for i, s in zip(suggester.pool_ids, suggester.pool_scores)]
        suggester.close()
        return Suggestion(hits, candidates, messages, strategy)
    finally:
        if own:
            engine.close()
