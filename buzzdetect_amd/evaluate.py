"""Evaluate models on annotated recordings: the reference's ``test_model`` step, starting from audio, with the threshold sweep
taken where the logits lie (include/buzzdetect_eval.h, csrc/evalsweep.hip).

    Sweep                 the integer state of C score columns on the device; ``update(scores, labels)``, ``counts()``, ``curves()``
    sweep_host            the library's host restatement of the definition, no device needed
    Curve                 one column's rows: ``table()`` (the text of ``tests/metrics.csv``), ``threshold_for_precision``,
                          ``average_precision``, ``auc``, ``best_f1``
    evaluate_logits       logits and targets that already exist (out-of-fold logits, a stored ``TrainingSet``) -> Evaluation
    evaluate_recordings   a folder of recordings, annotations and one or several models -> Evaluation
    Evaluation            ``curves``, ``events``, ``summary()``, ``to_csv``, ``write_metrics``

``train.metrics_table`` has one row per distinct logit rounded to two decimals and counts a window as detected when its logit
>= the threshold.  Both depend on a logit through two integers, ``kr = rint(z * 100)`` and ``kf = max{k : k / 100 <= z}``, so
three histograms per column - negatives by ``kf``, positives by ``kf``, all labelled rows by ``kr`` - hold everything the table
needs, and they are all that leaves the device.  Everything a ``Curve`` reports is a metric of that 0.01-grid table, computed in
float64 from integer counts; none is a metric of the raw ranks of the logits.

    from buzzdetect_amd import evaluate, calls

    found = evaluate.evaluate_recordings("held_out_audio", "held_out.csv", ["model_a", "model_b"], models_dir="models",
                                         rules={"ins_buzz": calls.Rule(-1.2, -2.0, merge_gap_s=2.0)})
    print(found.summary())
    found.write_metrics("models")                    # <models>/<model>/tests/metrics.csv: what analyze(precision=...) reads
"""
from __future__ import annotations

import csv
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, calls, framing
from .dataset import DIGITS_TIME, FRAMELENGTH_S, _as_annotations, _label_at, _merged, _torch
from .search import _logit_parts, _walk
from .train import METRICS_HEADER, _num

BINS, K_MIN, PLANES, TAILS = _lib.EVAL_BINS, _lib.EVAL_K_MIN, _lib.EVAL_PLANES, _lib.EVAL_TAILS
NEGATIVES, POSITIVES, ROWS = range(PLANES)                       # the planes of ``hist``
SKIPPED, NON_FINITE, BELOW, ABOVE = range(TAILS)                 # the words of ``tail``
TAIL_NAMES = ("skipped", "non-finite", "below -81.92", "above 81.91")
MAX_ROWS = (1 << 32) - 1                                          # rows per column of one state: its counters are uint32
SKIP = 2                                                          # the label of a row that counts for nothing
EVENT_TICKS = int(round(100 * FRAMELENGTH_S))                    # a kept event ends this many ticks after its last window's start
SUMMARY_COLUMNS = ("model", "class", "n_pos", "n_neg", "average_precision", "auc", "best_f1_threshold", "best_f1", "events",
                   "hits", "pieces", "found", "event_precision", "event_recall", "window_tp", "window_fp", "window_fn")


# ---------------------------------------------------------------------------------------------------- arguments
def _check_label_of(label_of, n_labels: int) -> np.ndarray:
    n_labels = int(n_labels)
    if not 1 <= n_labels <= _lib.EVAL_MAX_LABELS:
        raise ValueError(f"n_labels = {n_labels}, allowed are 1..{_lib.EVAL_MAX_LABELS}")
    out = np.ascontiguousarray(label_of, np.int32)
    if out.ndim != 1 or not 1 <= out.shape[0] <= _lib.EVAL_MAX_COLUMNS:
        raise ValueError(f"label_of must name the label column of 1..{_lib.EVAL_MAX_COLUMNS} score columns")
    bad = np.flatnonzero((out < -1) | (out >= n_labels))
    if bad.size:
        raise ValueError(f"label_of[{int(bad[0])}] = {int(out[bad[0]])}, allowed are -1..{n_labels - 1}")
    return out


def _check_labels(labels, w: int, n_labels: int) -> np.ndarray:
    labels = np.asarray(labels)
    if labels.dtype != np.uint8 or labels.shape != (w, n_labels):
        raise ValueError(f"labels must be uint8 [{w}, {n_labels}], not {labels.dtype} {list(labels.shape)}")
    return np.ascontiguousarray(labels)


# ---------------------------------------------------------------------------------------------------- curves
@dataclass
class Curve:
    """The rows of one score column's metrics table.  ``thresholds``: k / 100.0 for every k some labelled logit rounds to,
    descending; ``tp`` / ``fp``: the positives / negatives with logit >= the threshold, int64; ``n_pos`` / ``n_neg``: the
    labelled rows.  All metrics below are metrics of this 0.01-grid table - a row's counts are those of ``logit >= threshold``
    at a threshold that rounding may have moved past the logits that created the row - not of the raw ranks of the logits, and
    all are float64 arithmetic on the integer counts."""
    thresholds: np.ndarray
    tp: np.ndarray
    fp: np.ndarray
    n_pos: int
    n_neg: int
    name: str = ""
    n_skipped: int = 0                                                # rows whose label was neither 0 nor 1

    @classmethod
    def from_counts(cls, hist: np.ndarray, tail: Optional[np.ndarray] = None, name: str = "") -> "Curve":
        """``hist``: one column's uint32 [3, BINS]; ``tail``: its uint32 [4].  A column with non-finite or out-of-range rows
        has no table (``train.metrics_table`` refuses non-finite logits alike): ``ValueError`` with the column and the count."""
        hist = np.asarray(hist)
        if hist.shape != (PLANES, BINS):
            raise ValueError(f"hist must be [{PLANES}, {BINS}], not {list(hist.shape)}")
        if tail is not None:
            for word in (NON_FINITE, BELOW, ABOVE):
                if int(tail[word]):
                    raise ValueError(f"column {name!r}: {int(tail[word])} labelled rows with a logit {TAIL_NAMES[word]}: no table")
        neg, pos = hist[NEGATIVES].astype(np.int64), hist[POSITIVES].astype(np.int64)
        tp_from = np.cumsum(pos[::-1])[::-1]                          # positives with kf >= k
        fp_from = np.cumsum(neg[::-1])[::-1]
        rows = np.flatnonzero(hist[ROWS])[::-1]
        return cls((rows + K_MIN) / 100.0, tp_from[rows], fp_from[rows], int(pos.sum()), int(neg.sum()), name,
                   0 if tail is None else int(tail[SKIPPED]))

    def table(self) -> str:
        """The text ``train.metrics_table`` writes for the same logits and labels: the same header, the same formatting, an
        empty cell where a denominator is zero (the zero row is always ``0``, never ``-0``)."""
        rows = [METRICS_HEADER]
        for t, tp, fp in zip(self.thresholds.tolist(), self.tp.tolist(), self.fp.tolist()):
            detected = tp + fp
            rows.append(",".join((_num(t), _num(tp / detected) if detected else "", _num(tp / self.n_pos) if self.n_pos else "",
                                  _num(fp / self.n_neg) if self.n_neg else "")))
        return "\n".join(rows) + "\n"

    def threshold_for_precision(self, precision_requested: float, tolerance: float = 0.01) -> float:
        """``results.threshold_for_precision`` on this table: the mean threshold of the rows whose precision, as the table
        prints it (15 significant digits), lies within ``tolerance / 2`` of the request; NaN when there is none."""
        detected = self.tp + self.fp
        has = detected > 0
        p = np.array([float(_num(tp / d)) for tp, d in zip(self.tp[has].tolist(), detected[has].tolist())], np.float64)
        t = self.thresholds[has]
        sel = np.abs(p - precision_requested) <= tolerance / 2
        return float(t[sel].mean()) if sel.any() else float("nan")

    def average_precision(self) -> float:
        """sum_i (R_i - R_{i-1}) P_i down the table's rows, R_{-1} = 0; NaN without positives.  Of the 0.01-grid table."""
        if not self.n_pos:
            return float("nan")
        detected = (self.tp + self.fp).astype(np.float64)
        has = detected > 0
        recall = self.tp[has] / np.float64(self.n_pos)
        precision = self.tp[has] / detected[has]
        return float(np.sum(np.diff(recall, prepend=0.0) * precision))

    def auc(self) -> float:
        """The trapezoid under (fpr, tpr) from (0, 0) through the table's rows; NaN without positives or without negatives.
        Of the 0.01-grid table: the curve ends at the lowest row, which need not be (1, 1)."""
        if not self.n_pos or not self.n_neg:
            return float("nan")
        fpr = np.concatenate([[0.0], self.fp / np.float64(self.n_neg)])
        tpr = np.concatenate([[0.0], self.tp / np.float64(self.n_pos)])
        return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))

    def best_f1(self) -> Tuple[float, float]:
        """(threshold, F1) of the row with the greatest F1 = 2 TP / (2 TP + FP + FN); a tie goes to the higher threshold;
        (NaN, NaN) without a row that has positives or detections.  Of the 0.01-grid table."""
        bottom = (self.tp + self.fp + self.n_pos).astype(np.float64)
        has = bottom > 0
        if not has.any():
            return float("nan"), float("nan")
        f1 = 2.0 * self.tp[has] / bottom[has]
        at = int(np.argmax(f1))                                        # (the first of the greatest: thresholds descend)
        return float(self.thresholds[has][at]), float(f1[at])


# ---------------------------------------------------------------------------------------------------- the sweep
def sweep_host(scores: np.ndarray, labels, label_of, n_labels: int, state=None) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_eval_accumulate_host``: (hist uint32 [C, 3, BINS], tail uint32 [C, 4]) of float32 ``scores`` [W, C] (any strides)
    and uint8 ``labels`` [W, L].  ``state``: a (hist, tail) pair to add to, else zeros."""
    if not isinstance(scores, np.ndarray) or scores.dtype != np.float32 or scores.ndim != 2:
        raise ValueError("scores must be float32 [W, C]")
    w, c = scores.shape
    label_of = _check_label_of(label_of, n_labels)
    if label_of.shape[0] != c:
        raise ValueError(f"label_of names {label_of.shape[0]} columns, scores has {c}")
    if w > _lib.EVAL_MAX_WINDOWS:
        raise ValueError(f"scores has {w} rows, a call takes at most {_lib.EVAL_MAX_WINDOWS}")
    labels = _check_labels(labels, w, int(n_labels))
    rs, cs = calls._strides(scores, c)
    if rs == 0 or cs == 0:
        scores = np.ascontiguousarray(scores)
        rs, cs = c, 1
    if state is None:
        state = np.zeros((c, PLANES, BINS), np.uint32), np.zeros((c, TAILS), np.uint32)
    hist, tail = state
    if hist.dtype != np.uint32 or hist.shape != (c, PLANES, BINS) or tail.dtype != np.uint32 or tail.shape != (c, TAILS) \
            or not hist.flags.c_contiguous or not tail.flags.c_contiguous:
        raise ValueError(f"state must be contiguous uint32 [{c}, {PLANES}, {BINS}] and [{c}, {TAILS}]")
    _lib.check(_lib.load().bd_eval_accumulate_host(scores.ctypes.data, w, c, rs, cs, labels.ctypes.data, int(n_labels),
                                                   label_of.ctypes.data, hist.ctypes.data, tail.ctypes.data))
    return hist, tail


def curves_of(hist: np.ndarray, tail: np.ndarray, label_of, names: Optional[Sequence[str]] = None) -> List[Optional[Curve]]:
    """One ``Curve`` per column of a state, None for a column with ``label_of == -1``."""
    names = [str(i) for i in range(hist.shape[0])] if names is None else [str(n) for n in names]
    return [None if label_of[i] < 0 else Curve.from_counts(hist[i], tail[i], names[i]) for i in range(hist.shape[0])]


class Sweep:
    """The state of C score columns on the device.  ``label_of``: per score column the label column it is scored against, -1
    for a column that is not evaluated; ``n_labels``: the label columns.  Everything runs on the current stream of ``device``."""

    def __init__(self, label_of, n_labels: int, device=None):
        self.label_of = _check_label_of(label_of, n_labels)
        self.n_labels = int(n_labels)
        self.columns = int(self.label_of.shape[0])
        torch = _torch()
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; use sweep_host without one")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        self.rows = 0
        self._label_of = torch.from_numpy(self.label_of).to(self.device)
        self._hist = self._empty((self.columns, PLANES, BINS), torch.int32).zero_()      # (uint32 words: read back as such)
        self._tail = self._empty((self.columns, TAILS), torch.int32).zero_()
        assert 4 * (self._hist.numel() + self._tail.numel()) == self._lib.bd_eval_state_bytes(self.columns)

    def _empty(self, shape, dtype):
        """Every device buffer the kernel writes comes from here (the tests put guard words around them)."""
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def close(self) -> None:
        self._hist = self._tail = self._label_of = None

    def update(self, scores, labels) -> None:
        """Adds W rows.  ``scores``: a float32 [W, C] tensor on the device, any non-zero strides ([W][C] logits, a column-major
        matrix, a slice of a wider one); ``labels``: uint8 [W, L], NumPy or a tensor: 0 negative, 1 positive, anything else
        skip."""
        torch = _torch()
        if self._hist is None:
            raise ValueError("this Sweep is closed")
        s = scores
        if not isinstance(s, torch.Tensor) or s.dim() != 2 or s.shape[1] != self.columns or s.dtype != torch.float32 \
                or s.device != self.device:
            raise ValueError(f"scores must be a float32 [W, {self.columns}] tensor on {self.device}")
        w, c = int(s.shape[0]), self.columns
        if w > _lib.EVAL_MAX_WINDOWS:
            raise ValueError(f"scores has {w} rows, an update takes at most {_lib.EVAL_MAX_WINDOWS}")
        if self.rows + w > MAX_ROWS:
            raise ValueError(f"{self.rows} + {w} rows are more than the {MAX_ROWS} a state counts")
        if isinstance(labels, torch.Tensor):
            if labels.dtype != torch.uint8 or tuple(labels.shape) != (w, self.n_labels):
                raise ValueError(f"labels must be uint8 [{w}, {self.n_labels}], not {labels.dtype} {list(labels.shape)}")
            lab = labels.to(self.device).contiguous()
        else:
            lab = torch.from_numpy(_check_labels(labels, w, self.n_labels)).to(self.device)
        # (the stride of a dimension of one element is never used: any non-zero value serves)
        rs, cs = int(s.stride(0)) if w > 1 else c, int(s.stride(1)) if c > 1 else 1
        if rs == 0 or cs == 0:
            s, rs, cs = s.contiguous(), c, 1
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_eval_accumulate(s.data_ptr(), w, c, rs, cs, lab.data_ptr(), self.n_labels,
                                                    self._label_of.data_ptr(), self._hist.data_ptr(), self._tail.data_ptr(),
                                                    stream.cuda_stream))
        for used in (s, lab):
            used.record_stream(stream)
        self.rows += w

    def counts(self) -> Tuple[np.ndarray, np.ndarray]:
        """(hist uint32 [C, 3, BINS], tail uint32 [C, 4]) on the host."""
        if self._hist is None:
            raise ValueError("this Sweep is closed")
        return self._hist.cpu().numpy().view(np.uint32), self._tail.cpu().numpy().view(np.uint32)

    def curves(self, names: Optional[Sequence[str]] = None) -> List[Optional[Curve]]:
        """One ``Curve`` per column (None where ``label_of`` is -1); ``ValueError`` for a column with non-finite or
        out-of-range rows."""
        hist, tail = self.counts()
        return curves_of(hist, tail, self.label_of, names)


# ---------------------------------------------------------------------------------------------------- events against annotations
@dataclass
class EventScore:
    """Kept events of one (model, class) against that class's annotated pieces: ``hits`` of the ``events`` overlap a piece,
    ``found`` of the ``pieces`` are overlapped by an event; ``tp`` / ``fp`` / ``fn``: labelled windows with mark >= 2 that are
    positive / negative, and positive windows without such a mark."""
    events: int = 0
    hits: int = 0
    pieces: int = 0
    found: int = 0
    tp: int = 0
    fp: int = 0
    fn: int = 0

    @property
    def precision(self) -> float:
        return self.hits / self.events if self.events else float("nan")

    @property
    def recall(self) -> float:
        return self.found / self.pieces if self.pieces else float("nan")


def pieces_ticks(intervals) -> np.ndarray:
    """(start, end) seconds -> int64 [P, 2]: the union of [round(100 start), round(100 end)) as disjoint pieces, ascending
    (touching ones become one piece, one that rounds to nothing is left out)."""
    spans = [(int(round(100.0 * float(a))), int(round(100.0 * float(b)))) for a, b in intervals]
    merged = _merged((a, b) for a, b in spans if b > a)
    return np.array(merged, np.int64).reshape(-1, 2)


def match_events(spans: np.ndarray, pieces: np.ndarray, min_event_overlap: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """(hit bool [E], found bool [P]): event e = [spans[e, 0], spans[e, 1]) is a hit iff it shares at least
    ``min_event_overlap`` ticks with some piece; a piece is found iff some event shares as many with it.  Integer ticks."""
    if int(min_event_overlap) < 1:
        raise ValueError(f"min_event_overlap = {min_event_overlap} must be at least 1 tick")
    spans = np.asarray(spans, np.int64).reshape(-1, 2)
    pieces = np.asarray(pieces, np.int64).reshape(-1, 2)
    shared = np.minimum(spans[:, None, 1], pieces[None, :, 1]) - np.maximum(spans[:, None, 0], pieces[None, :, 0])
    ok = shared >= int(min_event_overlap)
    return ok.any(axis=1), ok.any(axis=0)


def event_spans(events: np.ndarray, t: np.ndarray) -> np.ndarray:
    """int64 [E, 2]: [t[first], t[last] + 96) of the KEPT rows of a column's events (``calls.Calls.events[c]``)."""
    kept = events[events[:, calls.KEPT] != 0]
    t = np.asarray(t, np.int64)
    return np.stack([t[kept[:, calls.FIRST]], t[kept[:, calls.LAST]] + EVENT_TICKS], axis=1).reshape(-1, 2)


def score_events(events: np.ndarray, marks: np.ndarray, t: np.ndarray, intervals, labels: np.ndarray,
                 min_event_overlap: int = 1) -> EventScore:
    """One column of one recording: its events and marks (``calls``), the ticks of its windows, the (start, end) seconds of
    the class's annotations and the windows' labels (0, 1, anything else skipped)."""
    pieces = pieces_ticks(intervals)
    spans = event_spans(events, t)
    hit, found = match_events(spans, pieces, min_event_overlap)
    called = np.asarray(marks) >= 2
    return EventScore(int(spans.shape[0]), int(hit.sum()), int(pieces.shape[0]), int(found.sum()),
                      int((called & (labels == 1)).sum()), int((called & (labels == 0)).sum()), int((~called & (labels == 1)).sum()))


def _add_scores(a: EventScore, b: EventScore) -> EventScore:
    return EventScore(*(getattr(a, k) + getattr(b, k) for k in ("events", "hits", "pieces", "found", "tp", "fp", "fn")))


# ---------------------------------------------------------------------------------------------------- results
@dataclass
class Evaluation:
    """``curves[(model, class)]``: the ``Curve``; ``events[(model, class)]``: the ``EventScore`` (with ``rules``);
    ``messages``: what was skipped, and why."""
    curves: Dict[Tuple[str, str], Curve]
    events: Dict[Tuple[str, str], EventScore] = field(default_factory=dict)
    messages: List[str] = field(default_factory=list)

    def summary(self) -> List[dict]:
        """One row per curve, in ``SUMMARY_COLUMNS``; the event columns are None without ``rules`` for the class."""
        rows = []
        for (model, name), curve in self.curves.items():
            at, f1 = curve.best_f1()
            ev = self.events.get((model, name))
            rows.append(dict(zip(SUMMARY_COLUMNS, (
                model, name, curve.n_pos, curve.n_neg, curve.average_precision(), curve.auc(), at, f1,
                *((None,) * 9 if ev is None else (ev.events, ev.hits, ev.pieces, ev.found, ev.precision, ev.recall, ev.tp, ev.fp,
                                                  ev.fn))))))
        return rows

    def to_csv(self, dir_out: str) -> None:
        """``metrics_<model>_<class>.csv`` per curve (``Curve.table()``) and ``summary.csv`` under ``dir_out``."""
        os.makedirs(dir_out, exist_ok=True)
        for (model, name), curve in self.curves.items():
            with open(os.path.join(dir_out, f"metrics_{model}_{name}.csv".replace(os.sep, "_")), "w") as f:
                f.write(curve.table())
        with open(os.path.join(dir_out, "summary.csv"), "w", newline="") as f:
            out = csv.writer(f, lineterminator="\n")
            out.writerow(SUMMARY_COLUMNS)
            for row in self.summary():
                out.writerow(["" if v is None or (isinstance(v, float) and math.isnan(v)) else
                              (_num(v) if isinstance(v, float) else v) for v in row.values()])

    def write_metrics(self, models_dir: str, class_name: str = "ins_buzz", overwrite: bool = False) -> List[str]:
        """``class_name``'s table of every model as ``<models_dir>/<model>/tests/metrics.csv`` - where ``analyze(precision=...)``
        and ``call_recordings(precision=...)`` look.  A file that exists is refused without ``overwrite=True``, before anything
        is written."""
        mine = [(model, curve) for (model, name), curve in self.curves.items() if name == class_name]
        if not mine:
            raise ValueError(f"class_name {class_name!r} is not among the evaluated classes {sorted({n for _, n in self.curves})}")
        paths = [os.path.join(models_dir, model, "tests", "metrics.csv") for model, _ in mine]
        there = [p for p in paths if os.path.exists(p)]
        if there and not overwrite:
            raise FileExistsError(f"{there[0]} exists; pass overwrite=True to replace it")
        for path, (_, curve) in zip(paths, mine):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                f.write(curve.table())
        return paths


# ---------------------------------------------------------------------------------------------------- logits that exist
def evaluate_logits(logits, targets, classes: Sequence[str], *, keep=None, names: Optional[Sequence[str]] = None) -> Evaluation:
    """Logits that already exist - a cross-validation's out-of-fold logits, a model over a stored ``TrainingSet`` - against
    their targets.  ``logits``: float32 [N, M * C], the C = len(classes) columns of M models side by side ([N, C] for one); a
    tensor on the device goes through ``Sweep``, a NumPy array through ``sweep_host`` (no device needed).  ``targets``: int [N]
    labels or [N, C] multi-label zeros and ones.  ``keep``: bool [N], rows that count (default: all).  ``names``: the M models
    (default ``model`` for one, else ``0`` ..)."""
    classes = [str(c) for c in classes]
    c = len(classes)
    if not c or len(set(classes)) != c:
        raise ValueError("classes must be at least one name, none twice")
    resident = not isinstance(logits, np.ndarray)
    shape = tuple(int(v) for v in logits.shape)
    if len(shape) != 2 or shape[1] == 0 or shape[1] % c:
        raise ValueError(f"logits must be [N, M * {c}] for the {c} classes, not {list(shape)}")
    n, m = shape[0], shape[1] // c
    if shape[1] > _lib.EVAL_MAX_COLUMNS or c > _lib.EVAL_MAX_LABELS:
        raise ValueError(f"logits has {shape[1]} columns, at most {_lib.EVAL_MAX_COLUMNS} are swept at once")
    names = (["model"] if m == 1 else [str(i) for i in range(m)]) if names is None else [str(v) for v in names]
    if len(names) != m or len(set(names)) != m:
        raise ValueError(f"names must name the {m} models of logits, none twice")
    t = np.asarray(targets)
    if t.shape == (n,) and (t.dtype.kind in "iu"):
        if n and (t.min() < 0 or t.max() >= c):
            raise ValueError(f"targets must be labels in 0..{c - 1}")
        labels = (t[:, None] == np.arange(c)[None, :]).astype(np.uint8)
    elif t.shape == (n, c):
        if not np.isin(t, (0, 1)).all():
            raise ValueError("multi-label targets must be zeros and ones")
        labels = (t != 0).astype(np.uint8)
    else:
        raise ValueError(f"targets must be int labels [{n}] or multi-label [{n}, {c}], not {t.dtype} {list(t.shape)}")
    if keep is not None:
        keep = np.asarray(keep)
        if keep.dtype != bool or keep.shape != (n,):
            raise ValueError(f"keep must be bool [{n}]")
        labels[~keep] = SKIP
    label_of = np.tile(np.arange(c, dtype=np.int32), m)
    columns = [f"{model}/{name}" for model in names for name in classes]
    step = _lib.EVAL_MAX_WINDOWS
    if not resident:
        x = logits if logits.dtype == np.float32 else logits.astype(np.float32)
        state = None
        for at in range(0, max(n, 1), step):
            state = sweep_host(x[at:at + step], labels[at:at + step], label_of, c, state)
        found = curves_of(*state, label_of, columns)
    else:
        sweep = Sweep(label_of, c, device=logits.device)
        for at in range(0, max(n, 1), step):
            sweep.update(logits[at:at + step], labels[at:at + step])
        found = sweep.curves(columns)
        sweep.close()
    return Evaluation({(model, name): found[i * c + j] for i, model in enumerate(names) for j, name in enumerate(classes)})


# ---------------------------------------------------------------------------------------------------- recordings
def _models_of(engine, modelname) -> Dict[str, Tuple[int, List[str]]]:
    """{model: (its first column, its classes)} of an engine with one model or a set of heads."""
    if engine.members is not None:
        return {name: (int(engine.member_columns[name].start), [str(c) for c in head.classes]) for name, head in engine.members.items()}
    return {modelname if isinstance(modelname, str) else "model": (0, [str(c) for c in engine.classes])}


def evaluate_recordings(dir_audio: str, annotations, modelname="model_general_v3", *, classes: Optional[Sequence[str]] = None,
                        background: Optional[str] = None, min_overlap: float = 0.5, only_annotated: bool = True,
                        rules: Optional[Dict[str, "calls.Rule"]] = None, framehop_prop: float = 1.0, chunklength: float = 200,
                        engine=None, embeddername: str = "yamnet_k2", models_dir: Optional[str] = None,
                        min_event_overlap: int = 1) -> Evaluation:
    """Every recording under ``dir_audio`` that ``analyze`` would take, read, resampled and scored as ``call_recordings`` does
    it, against ``annotations`` (a path for ``dataset.read_annotations`` or what it returns).  ``modelname``: one name, or a
    list - a set of heads behind one pass; ``engine``: a ``HipEngine`` that carries the model or the set.

    A window's start is the ``start`` ``analyze`` writes for it, and its labels are ``dataset.label_windows``' for that start:
    1 for a class whose annotated piece it overlaps enough, 0 for the other classes, every class skipped where the window
    meets a piece and gets no class (ambiguous); a window that meets nothing is a negative of every class but ``background``,
    whose positive it is.  ``classes``: the classes to evaluate (default: the first model's classes that occur as annotation
    labels); every model must carry them; annotation rows with another label are ignored and said so.  With
    ``only_annotated`` a recording that the annotations do not mention is not scored at all; without, it is all negative.

    Each launch set's columns go to ``Sweep.update`` and are dropped: no [W, C] matrix returns to the host.

    ``rules``: {class: ``calls.Rule``}.  The recording's columns of those classes are then also called as ``call_recordings``
    calls them, and on the host, in integer ticks, the kept events - [t[first], t[last] + 96) - are matched against the
    class's annotated intervals, merged into pieces [round(100 start), round(100 end)): an event is a hit iff it overlaps
    some piece by at least ``min_event_overlap`` ticks, a piece is found iff some kept event overlaps it likewise."""
    from .engine import HipEngine
    notes = _as_annotations(annotations)
    if not 0.0 < min_overlap <= 1.0:
        raise ValueError("min_overlap must be in (0, 1]")
    if int(min_event_overlap) < 1:
        raise ValueError(f"min_event_overlap = {min_event_overlap} must be at least 1 tick")
    if isinstance(modelname, (list, tuple)) and engine is None and (not modelname or len(set(modelname)) != len(modelname)):
        raise ValueError("modelname must list at least one model, none twice")
    rules = {} if rules is None else dict(rules)
    if not all(isinstance(r, calls.Rule) for r in rules.values()):
        raise ValueError("rules must map classes to calls.Rule")
    framehop_s = FRAMELENGTH_S * framehop_prop
    adjacent = calls.adjacent_ticks(framehop_s)
    annotated = {label for rows in notes.values() for _, _, label in rows}
    messages: List[str] = []
    own = engine is None
    if own:
        engine = HipEngine(embeddername=embeddername, modelname=modelname, models_dir=models_dir)
    try:
        if not engine.n_classes:
            raise ValueError("evaluate_recordings needs an engine with a classifier")
        models = _models_of(engine, modelname)
        first_classes = next(iter(models.values()))[1]
        names = [c for c in first_classes if c in annotated] if classes is None else [str(c) for c in classes]
        if not names or len(set(names)) != len(names):
            raise ValueError("classes: no class to evaluate (none of the model's classes is an annotation label)" if not names
                             else "classes names a class twice")
        for model, (_, own_classes) in models.items():
            absent = [c for c in names if c not in own_classes]
            if absent:
                raise ValueError(f"classes {absent} are not among the classes of {model!r}: {own_classes}")
        if background is not None and background not in names:
            raise ValueError(f"background {background!r} is not one of the classes {names}")
        unknown = sorted(set(rules) - set(names))
        if unknown:
            raise ValueError(f"rules for {unknown}, which are not among the classes {names}")
        ignored = sorted(annotated - set(names))
        if ignored:
            messages.append(f"annotation labels that are not evaluated, ignored: {', '.join(ignored)}")
        notes = {ident: [row for row in rows if row[2] in names] for ident, rows in notes.items()}
        keys = [(model, name) for model in models for name in names]
        picked = [first + own_classes.index(name) for first, own_classes in models.values() for name in names]
        if len(picked) > _lib.EVAL_MAX_COLUMNS:
            raise ValueError(f"{len(models)} models x {len(names)} classes are more than {_lib.EVAL_MAX_COLUMNS} columns")
        ruled = [i for i, (_, name) in enumerate(keys) if name in rules]
        if len(ruled) > _lib.CALLS_MAX_COLUMNS:
            raise ValueError(f"rules for {len(ruled)} columns, at most {_lib.CALLS_MAX_COLUMNS} are called at once")
        torch = _torch()
        columns = torch.tensor(picked, dtype=torch.int64, device=engine.device)
        sweep = Sweep(np.tile(np.arange(len(names), dtype=np.int32), len(models)), len(names), device=engine.device)
        caller = calls.Caller([rules[keys[i][1]] for i in ruled], device=engine.device) if ruled else None
        ruled_dev = torch.tensor(ruled, dtype=torch.int64, device=engine.device)
        scores_of = {keys[i]: EventScore() for i in ruled}
        now = {"ident": None, "starts": [], "chunk": 0}
        held: List[object] = []
        held_labels: List[np.ndarray] = []
        fed = [0]

        def recording_starts(ident, chunk_starts):
            now.update(ident=ident, starts=list(chunk_starts), chunk=0)

        def feed(parts, hop, step):
            logits, counts = _logit_parts(engine, parts, hop, step)
            edges = now["starts"][now["chunk"]:now["chunk"] + len(counts)]
            now["chunk"] += len(counts)
            starts = np.concatenate([framing.window_starts(n, s, framehop_s, DIGITS_TIME) for s, n in zip(edges, counts)]
                                    + [np.zeros(0)])
            targets, keep, _ = _label_at(starts, notes.get(now["ident"], ()), names, min_overlap, background)
            labels = targets.astype(np.uint8)
            labels[~keep] = SKIP
            scores = logits.index_select(1, columns)
            sweep.update(scores, labels)
            if caller is not None:
                held.append(scores.index_select(1, ruled_dev))
                held_labels.append(labels)
            first = fed[0]
            fed[0] += int(sum(counts))
            return first, counts

        def recording_done(ident, chunk_starts, counts):
            if caller is None:
                return
            scores = torch.cat(held) if held else torch.zeros((0, len(ruled)), dtype=torch.float32, device=engine.device)
            labels = np.concatenate(held_labels) if held_labels else np.zeros((0, len(names)), np.uint8)
            held.clear()
            held_labels.clear()
            starts = np.concatenate([framing.window_starts(n, s, framehop_s, DIGITS_TIME) for s, n in zip(chunk_starts, counts)]
                                    + [np.zeros(0)])
            if starts.shape[0] > _lib.CALLS_MAX_WINDOWS:
                messages.append(f"more than {_lib.CALLS_MAX_WINDOWS} windows, events not scored: {ident}")
                return
            t = calls.ticks(starts)
            got = caller.call(scores, t, adjacent)
            for at, i in enumerate(ruled):
                name = keys[i][1]
                spans = [(a, b) for a, b, label in notes.get(ident, ()) if label == name]
                one = score_events(got.events[at], got.marks[at], t, spans, labels[:, names.index(name)], min_event_overlap)
                scores_of[keys[i]] = _add_scores(scores_of[keys[i]], one)

        _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed, recording_done, recording_starts, notes,
              only_annotated)
        found = sweep.curves([f"{model}/{name}" for model, name in keys])
        sweep.close()
        if caller is not None:
            caller.close()
        return Evaluation(dict(zip(keys, found)), scores_of, messages)
    finally:
        if own:
            engine.close()
