"""Call detections: a model's score columns become events and per-bin rates - "from sounds to stats", the step after
``analyze``'s 90 000 rows of ``activation_*`` per recording-day.

    Rule                high / low thresholds (hysteresis), the gap an event bridges, the shortest event kept
    Caller              rules on the device, ``call(scores, ticks, adjacent, seg)``: marks, events and bins of one sequence
    call_recordings     a folder of recordings through a model -> CallResult (events and per-minute bins per class)
    call_results        the same rules by the host routines over a result tree ``analyze`` already wrote (no device)
    CallResult          ``events``, ``bins``, ``to_csv``, ``annotations`` (rows ``dataset.read_annotations`` reads)
    events_host / bins_host   the library's host restatements of the definitions

The definitions are those of ``include/buzzdetect_calls.h``: a window is ON from a score above ``high`` until one not above
``low`` (or a hole in the recording); ON windows at most ``link`` ticks apart form an event; an event shorter than
``min_extent`` ticks is dropped.  A tick is a hundredth of a second.  The calling runs where the logits lie (csrc/calls.hip): a
recording's windows are scored as ``search.top_windows`` scores them, their logits stay on the device, and only marks, the
events' rows and the bins come back.

    from buzzdetect_amd import calls

    found = calls.call_recordings("audio_in", thresholds={"ins_buzz": -1.2}, low={"ins_buzz": -2.0},
                                  merge_gap_s=2.0, min_duration_s=1.5, bin_s=60.0)
    found.to_csv("called")                              # <ident>_buzzevents.csv, <ident>_buzzbins.csv
    found.annotations(path="pseudo_labels.csv")         # ident,start,end,label

    again = calls.call_results("models/model_general_v3/output", {"ins_buzz": calls.Rule(-1.2, -2.0, merge_gap_s=2.0)})
"""
from __future__ import annotations

import csv
import json
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib, framing
from .dataset import DIGITS_TIME, FRAMELENGTH_S, _torch
from .search import ANNOTATION_COLUMNS, _end, _logit_parts, _walk

EVENT_COLUMNS = ("class", "start", "end", "windows", "detected", "peak", "peak_start")
SUFFIX_EVENTS = "_buzzevents.csv"
SUFFIX_BINS = "_buzzbins.csv"
RULE = np.dtype([("high", "<f4"), ("low", "<f4"), ("link", "<i4"), ("min_extent", "<i4")])      # bd_calls_rule
FIRST, LAST, N_ON, PEAK, KEPT = range(_lib.CALLS_EVENT_FIELDS)
assert RULE.itemsize == 16


# ---------------------------------------------------------------------------------------------------- rules and ticks
@dataclass(frozen=True)
class Rule:
    """``high``: a score above it switches a window ON; ``low`` (default ``high``): a score not above it switches OFF, one
    between the two keeps the state.  ``merge_gap_s``: ON windows whose starts lie up to a hop plus this many seconds apart
    belong to one event.  ``min_duration_s``: an event lasts from its first window's start to its last window's start + 0.96 s;
    a shorter one is dropped."""
    high: float
    low: Optional[float] = None
    merge_gap_s: float = 0.0
    min_duration_s: float = 0.0

    def __post_init__(self):
        low = self.high if self.low is None else self.low
        if math.isnan(float(self.high)) or math.isnan(float(low)) or float(low) > float(self.high):
            raise ValueError(f"a rule needs high >= low and neither a NaN, not high = {self.high}, low = {low}")
        if not self.merge_gap_s >= 0 or not math.isfinite(self.merge_gap_s):
            raise ValueError(f"merge_gap_s must be finite and not negative, not {self.merge_gap_s}")
        if not math.isfinite(self.min_duration_s):
            raise ValueError(f"min_duration_s must be finite, not {self.min_duration_s}")

    def packed(self, adjacent: int) -> Tuple[float, float, int, int]:
        """(high, low, link, min_extent) in ticks for windows ``adjacent`` ticks apart."""
        low = self.high if self.low is None else self.low
        return (float(self.high), float(low), int(adjacent) + int(round(100 * self.merge_gap_s)),
                max(0, int(round(100 * (self.min_duration_s - FRAMELENGTH_S)))))


def pack_rules(rules, adjacent: int) -> np.ndarray:
    """``bd_calls_rule[C]``: every rule a ``Rule`` or a ready (high, low, link, min_extent) in ticks; checked as the library does."""
    rows = [r.packed(adjacent) if isinstance(r, Rule) else tuple(r) for r in rules]
    if not 1 <= len(rows) <= _lib.CALLS_MAX_COLUMNS:
        raise ValueError(f"there must be 1..{_lib.CALLS_MAX_COLUMNS} rules, not {len(rows)}")
    out = np.array(rows, dtype=RULE)
    bad = np.isnan(out["high"]) | np.isnan(out["low"]) | (out["high"] < out["low"]) | (out["link"] < adjacent) | (out["min_extent"] < 0)
    if adjacent < 1 or bad.any():
        raise ValueError(f"adjacent = {adjacent} must be at least 1" if adjacent < 1 else
                         f"rule {int(np.flatnonzero(bad)[0])} needs high >= low, link >= adjacent = {adjacent} and min_extent >= 0: "
                         f"{rows[int(np.flatnonzero(bad)[0])]}")
    return out


def ticks(starts) -> np.ndarray:
    """Window starts in seconds (``framing.window_starts(..., digits_time=2)``: analyze's start column) as int32 ticks."""
    return np.rint(100.0 * np.asarray(starts, np.float64)).astype(np.int32)


def adjacent_ticks(framehop_s: float) -> int:
    """The largest step between neighbouring windows at this hop, in ticks: starts are rounded to 0.01 s, so a hop that is no
    whole number of ticks steps by its floor and its ceiling."""
    if not framehop_s >= 0.01:
        raise ValueError(f"a framehop of {framehop_s} s is below a tick, 0.01 s")
    return int(math.ceil(round(100.0 * framehop_s, 6)))


def _check_ticks(t: np.ndarray) -> np.ndarray:
    t = np.ascontiguousarray(t, np.int32)
    if t.ndim != 1 or t.shape[0] > _lib.CALLS_MAX_WINDOWS:
        raise ValueError(f"ticks must be one int32 per window, at most {_lib.CALLS_MAX_WINDOWS}")
    if t.shape[0] > 1 and (np.diff(t.astype(np.int64)) <= 0).any():
        raise ValueError("ticks must be strictly increasing")
    return t


def _strides(x, c: int) -> Tuple[int, int]:
    return tuple(s // 4 for s in x.strides) if x.size else (c, 1)


# ---------------------------------------------------------------------------------------------------- host routines
def events_host(scores: np.ndarray, t, adjacent: int, rules) -> Tuple[np.ndarray, List[np.ndarray]]:
    """``bd_calls_events_host``: (marks uint8 [C, W], per column its events int32 [n, 5]: first, last, n_on, peak, kept) of
    float32 ``scores`` [W, C] (any strides)."""
    if scores.dtype != np.float32 or scores.ndim != 2:
        raise ValueError("scores must be float32 [W, C]")
    w, c = scores.shape
    t = _check_ticks(t)
    if t.shape[0] != w:
        raise ValueError(f"{t.shape[0]} ticks for {w} windows")
    packed = pack_rules(rules, adjacent)
    if packed.shape[0] != c:
        raise ValueError(f"{packed.shape[0]} rules for {c} columns")
    rs, cs = _strides(scores, c)
    if rs == 0 or cs == 0:
        scores = np.ascontiguousarray(scores)
        rs, cs = c, 1
    marks = np.zeros((c, w), np.uint8)
    events = np.zeros((c, w, _lib.CALLS_EVENT_FIELDS), np.int32)
    n = np.zeros(c, np.int32)
    _lib.check(_lib.load().bd_calls_events_host(scores.ctypes.data, w, c, rs, cs, t.ctypes.data, int(adjacent), packed.ctypes.data,
                                                marks.ctypes.data, events.ctypes.data, n.ctypes.data))
    return marks, [events[i, :n[i]].copy() for i in range(c)]


def bins_host(scores: np.ndarray, marks: np.ndarray, seg) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_calls_bins_host``: (counts int32 [C, B, 2]: detected, events; values float32 [C, B, 2]: sum, max) of the bins
    ``seg[b] .. seg[b + 1] - 1``."""
    if scores.dtype != np.float32 or scores.ndim != 2:
        raise ValueError("scores must be float32 [W, C]")
    w, c = scores.shape
    marks = np.ascontiguousarray(marks, np.uint8)
    if marks.shape != (c, w):
        raise ValueError(f"marks must be uint8 [{c}, {w}], not {list(marks.shape)}")
    seg = np.ascontiguousarray(seg, np.int32)
    if seg.ndim != 1 or seg.shape[0] < 1:
        raise ValueError("seg must hold B + 1 offsets")
    b = seg.shape[0] - 1
    rs, cs = _strides(scores, c)
    if rs == 0 or cs == 0:
        scores = np.ascontiguousarray(scores)
        rs, cs = c, 1
    counts = np.zeros((c, b, 2), np.int32)
    values = np.zeros((c, b, 2), np.float32)
    _lib.check(_lib.load().bd_calls_bins_host(scores.ctypes.data, w, c, rs, cs, marks.ctypes.data, seg.ctypes.data, b,
                                              counts.ctypes.data, values.ctypes.data))
    return counts, values


def _check_seg(seg, w: int) -> np.ndarray:
    seg = np.ascontiguousarray(seg, np.int32)
    if seg.ndim != 1 or not 1 <= seg.shape[0] <= _lib.CALLS_MAX_BINS + 1:
        raise ValueError(f"seg must hold B + 1 offsets, B at most {_lib.CALLS_MAX_BINS}")
    if seg[0] < 0 or seg[-1] > w or (np.diff(seg.astype(np.int64)) < 0).any():
        raise ValueError(f"seg must not decrease and lie within 0..{w}")
    return seg


# ---------------------------------------------------------------------------------------------------- the caller
class Calls(NamedTuple):
    """One sequence called.  ``events[c]``: int32 [n, 5] (first, last, n_on, peak, kept), dropped events included;
    ``peaks[c]``: the float32 score at every event's peak; ``counts`` / ``values``: [C, B, 2], None without ``seg``."""
    marks: np.ndarray
    events: List[np.ndarray]
    peaks: List[np.ndarray]
    counts: Optional[np.ndarray]
    values: Optional[np.ndarray]


class Caller:
    """The rules of C columns and the device side of calling.  ``rules``: one per column, each a ``Rule`` or a ready
    (high, low, link, min_extent) in ticks.  Everything runs on the current stream of ``device``."""

    def __init__(self, rules, device=None):
        torch = _torch()
        self._lib = _lib.load()
        self.rules = list(rules)
        self.columns = len(self.rules)
        if not 1 <= self.columns <= _lib.CALLS_MAX_COLUMNS:
            raise ValueError(f"there must be 1..{_lib.CALLS_MAX_COLUMNS} rules, not {self.columns}")
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; use events_host / bins_host without one")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        self._packed: Dict[int, object] = {}                 # adjacent -> bd_calls_rule[C] on the device

    def _empty(self, shape, dtype):
        """Every device buffer the kernels write comes from here (the tests put guard words around them)."""
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def close(self) -> None:
        self._packed = {}

    def _rules_dev(self, adjacent: int):
        if adjacent not in self._packed:
            host = pack_rules(self.rules, adjacent)
            self._packed[adjacent] = _torch().from_numpy(host.view(np.int32).reshape(-1, 4).copy()).to(self.device)
        return self._packed[adjacent]

    def call(self, scores, ticks, adjacent: int, seg=None) -> Calls:
        """``scores``: float32 [W, C], a tensor on the device (any non-zero strides) or NumPy; ``ticks``: int32 [W], strictly
        increasing; ``seg``: B + 1 window offsets of the bins, or None for no bins.  One scan, one finishing pass and one bins
        pass; marks, the events' rows and the bins are read back."""
        torch = _torch()
        adjacent = int(adjacent)
        if not isinstance(scores, torch.Tensor):
            scores = torch.from_numpy(np.ascontiguousarray(scores, np.float32)).to(self.device)
        s = scores
        if s.dim() != 2 or s.shape[1] != self.columns or s.dtype != torch.float32 or s.device != self.device:
            raise ValueError(f"scores must be a float32 [W, {self.columns}] tensor on {self.device}")
        w, c = int(s.shape[0]), self.columns
        # (the stride of a dimension of one element is never used: any non-zero value serves)
        rs, cs = int(s.stride(0)) if w > 1 else c, int(s.stride(1)) if c > 1 else 1
        if rs == 0 or cs == 0:
            s, rs, cs = s.contiguous(), c, 1
        t_host = _check_ticks(ticks)
        if t_host.shape[0] != w:
            raise ValueError(f"{t_host.shape[0]} ticks for {w} windows")
        seg_host = None if seg is None else _check_seg(seg, w)
        rules = self._rules_dev(adjacent)
        t = torch.from_numpy(t_host).to(self.device)
        marks = self._empty((c, w), torch.uint8)
        events = self._empty((c, w, _lib.CALLS_EVENT_FIELDS), torch.int32)
        n_events = self._empty((c,), torch.int32)
        stream = torch.cuda.current_stream(self.device)
        counts = values = None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_calls_events(s.data_ptr(), w, c, rs, cs, t.data_ptr(), adjacent, rules.data_ptr(),
                                                 marks.data_ptr(), events.data_ptr(), n_events.data_ptr(), stream.cuda_stream))
            if seg_host is not None:
                b = seg_host.shape[0] - 1
                seg_dev = torch.from_numpy(seg_host).to(self.device)
                counts = self._empty((c, b, 2), torch.int32)
                values = self._empty((c, b, 2), torch.float32)
                _lib.check(self._lib.bd_calls_bins(s.data_ptr(), w, c, rs, cs, marks.data_ptr(), seg_dev.data_ptr(), b,
                                                   counts.data_ptr(), values.data_ptr(), stream.cuda_stream))
                seg_dev.record_stream(stream)
        for used in (s, t, rules):
            used.record_stream(stream)
        n = n_events.cpu().numpy()
        most = int(n.max()) if c else 0
        rows = events[:, :most].cpu().numpy()
        found = [rows[i, :n[i]].copy() for i in range(c)]
        peaks = []
        if most:
            at = events[:, :most, PEAK].to(torch.int64).clamp_(0, max(w - 1, 0))                  # (rows past n[i] are not read below)
            picked = torch.stack([s[at[i], i] for i in range(c)]).cpu().numpy()
            peaks = [picked[i, :n[i]].copy() for i in range(c)]
        else:
            peaks = [np.zeros(0, np.float32) for _ in range(c)]
        return Calls(marks.cpu().numpy(), found, peaks, None if counts is None else counts.cpu().numpy(),
                     None if values is None else values.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- results
@dataclass
class RecordingBins:
    """The bins of one recording that hold windows: ``bin_start`` seconds, ``windows`` per bin, ``counts`` int32 [C, B, 2]
    (detected windows, events), ``values`` float32 [C, B, 2] (sum, max)."""
    bin_start: np.ndarray
    windows: np.ndarray
    counts: np.ndarray
    values: np.ndarray


@dataclass
class CallResult:
    """``events[c]``: the kept events of ``classes[c]`` as (ident, start, end, windows, detected, peak, peak_start) in the order
    of the walk - start of the first window, end of the last (its start + 0.96 s), windows from first to last, those among them
    that were ON, the greatest ON score and its window's start.  ``bins[ident]``: that recording's ``RecordingBins``."""
    classes: List[str]
    events: List[List[Tuple[str, float, float, int, int, float, float]]]
    bins: Dict[str, RecordingBins] = field(default_factory=dict)
    messages: List[str] = field(default_factory=list)
    bin_s: float = 60.0
    digits_results: int = 2
    framelength_s: float = FRAMELENGTH_S

    def _rounded(self, v) -> str:
        return str(np.round(np.float32(v), self.digits_results))          # as results.activation_table rounds its float32 values

    def to_csv(self, dir_out: str) -> None:
        """Per recording ``<ident>_buzzevents.csv`` (``class,start,end,windows,detected,peak,peak_start``) and
        ``<ident>_buzzbins.csv`` (``bin_start,windows`` and per class ``detected_<c>,events_<c>,mean_<c>,max_<c>``) under
        ``dir_out``, in the layout of ``analyze``'s tree."""
        for ident, bins in self.bins.items():
            base = os.path.join(dir_out, ident)
            os.makedirs(os.path.dirname(base) or ".", exist_ok=True)
            with open(base + SUFFIX_EVENTS, "w", newline="") as f:
                out = csv.writer(f, lineterminator="\n")
                out.writerow(EVENT_COLUMNS)
                for name, rows in zip(self.classes, self.events):
                    for who, start, end, windows, detected, peak, peak_start in rows:
                        if who == ident:
                            out.writerow([name, repr(float(start)), repr(float(end)), int(windows), int(detected), self._rounded(peak),
                                          repr(float(peak_start))])
            with open(base + SUFFIX_BINS, "w", newline="") as f:
                out = csv.writer(f, lineterminator="\n")
                out.writerow(["bin_start", "windows"]
                             + [f"{k}_{name}" for name in self.classes for k in ("detected", "events", "mean", "max")])
                for b in range(bins.bin_start.shape[0]):
                    row = [repr(float(bins.bin_start[b])), int(bins.windows[b])]
                    for c in range(len(self.classes)):
                        mean = round(float(np.float64(bins.values[c, b, 0]) / np.float64(bins.windows[b])), 4)
                        row += [int(bins.counts[c, b, 0]), int(bins.counts[c, b, 1]), repr(mean), self._rounded(bins.values[c, b, 1])]
                    out.writerow(row)

    def annotations(self, labels: Optional[Dict[str, str]] = None, path: Optional[str] = None) -> List[Tuple[str, float, float, str]]:
        """The kept events as annotation rows (ident, start, end, label), class by class; the label is the class name, or
        ``labels[class]``.  ``path``: also written there, in the format ``dataset.read_annotations`` reads."""
        labels = {} if labels is None else {str(k): str(v) for k, v in labels.items()}
        unknown = sorted(set(labels) - set(self.classes))
        if unknown:
            raise ValueError(f"labels for {unknown}, which are not among the classes {self.classes}")
        rows = [(ident, float(start), float(end), labels.get(name, name))
                for name, found in zip(self.classes, self.events) for ident, start, end, *_ in found]
        if path is not None:
            with open(path, "w", newline="") as f:
                out = csv.writer(f)
                out.writerow(ANNOTATION_COLUMNS)
                for ident, start, end, label in rows:
                    out.writerow([ident, repr(start), repr(end), label])
        return rows


def bin_ticks(bin_s: float) -> int:
    n = int(round(100.0 * bin_s))
    if not (bin_s > 0 and n >= 1 and abs(100.0 * bin_s - n) < 1e-6):
        raise ValueError(f"bin_s must be a positive multiple of 0.01 s, not {bin_s}")
    return n


def bin_segments(t: np.ndarray, per_bin: int) -> Tuple[np.ndarray, np.ndarray]:
    """(the bins floor(tick / per_bin) that hold windows, seg int32 [B + 1]: their window offsets)."""
    of = np.asarray(t, np.int64) // per_bin
    ids = np.unique(of)
    seg = np.concatenate([np.searchsorted(of, ids, side="left"), [of.shape[0]]]).astype(np.int32)
    return ids, seg


def _add(result: CallResult, ident: str, starts: np.ndarray, events, peaks, ids: np.ndarray, seg: np.ndarray, per_bin: int,
         counts: np.ndarray, values: np.ndarray) -> None:
    for c, (rows, scores) in enumerate(zip(events, peaks)):
        for row, peak in zip(rows, scores):
            if row[KEPT]:
                result.events[c].append((ident, float(starts[row[FIRST]]), _end(starts[row[LAST]], result.framelength_s),
                                         int(row[LAST] - row[FIRST] + 1), int(row[N_ON]), float(peak), float(starts[row[PEAK]])))
    result.bins[ident] = RecordingBins(ids.astype(np.float64) * per_bin / 100.0, np.diff(seg).astype(np.int64), counts, values)


# ---------------------------------------------------------------------------------------------------- folders
def call_recordings(dir_audio: str, modelname: Optional[str] = "model_general_v3", *, classes: Sequence[str] = ("ins_buzz",),
                    thresholds: Optional[Dict[str, float]] = None, precision: Optional[float] = None, low=None,
                    merge_gap_s: float = 0.0, min_duration_s: float = 0.0, bin_s: float = 60.0, engine=None,
                    framehop_prop: float = 1.0, chunklength: float = 200, embeddername: str = "yamnet_k2",
                    models_dir: Optional[str] = None) -> CallResult:
    """Events and bins of ``classes`` for every recording under ``dir_audio`` that ``analyze`` would take, read, resampled and
    scored as ``search.top_windows`` does it.  ``thresholds``: {class: high}; or ``precision``, looked up in the model's
    metrics for ``ins_buzz`` as ``analyze`` does.  ``low``: one value for all classes or {class: low} (default: ``high``).
    The logits of one recording are gathered on the device and called at once; a window's tick is the ``start`` ``analyze``
    writes for it.  Bins are ``floor(start / bin_s)``; those without windows are left out.  ``engine``: a ``HipEngine`` that
    carries the model or a set of heads (the columns are then named as ``engine.classes`` names them)."""
    from .engine import HipEngine
    from . import results
    per_bin = bin_ticks(bin_s)
    framehop_s = FRAMELENGTH_S * framehop_prop
    adjacent = adjacent_ticks(framehop_s)
    names = [str(c) for c in classes]
    highs = {} if thresholds is None else {str(k): float(v) for k, v in thresholds.items()}
    if precision is not None and "ins_buzz" not in highs:
        highs["ins_buzz"] = results.threshold_for_precision(modelname, precision)
    missing = [c for c in names if c not in highs]
    if missing or not names:
        raise ValueError(f"no threshold for {missing}: give thresholds={{class: high}} (or precision, for ins_buzz)" if missing
                         else "no classes")
    lows = low if isinstance(low, dict) else {c: low for c in names}
    rules = [Rule(highs[c], lows.get(c), merge_gap_s, min_duration_s) for c in names]
    messages: List[str] = []
    own = engine is None
    if own:
        engine = HipEngine(embeddername=embeddername, modelname=modelname, models_dir=models_dir)
    try:
        if not engine.n_classes:
            raise ValueError("call_recordings needs an engine with a classifier")
        absent = [c for c in names if c not in engine.classes]
        if absent:
            raise ValueError(f"classes {absent} are not among the model's {list(engine.classes)}")
        torch = _torch()
        columns = torch.tensor([engine.classes.index(c) for c in names], dtype=torch.int64, device=engine.device)
        caller = Caller(rules, device=engine.device)
        result = CallResult(names, [[] for _ in names], bin_s=per_bin / 100.0)
        held: List[object] = []
        fed = [0]

        def feed(parts, hop, step):
            logits, counts = _logit_parts(engine, parts, hop, step)
            held.append(logits.index_select(1, columns))
            first = fed[0]
            fed[0] += int(sum(counts))
            return first, counts

        def recording_done(ident, chunk_starts, counts):
            scores = torch.cat(held) if held else torch.zeros((0, len(names)), dtype=torch.float32, device=engine.device)
            held.clear()
            starts = np.concatenate([framing.window_starts(n, s, framehop_s, DIGITS_TIME) for s, n in zip(chunk_starts, counts)]
                                    + [np.zeros(0)])
            if starts.shape[0] > _lib.CALLS_MAX_WINDOWS:
                messages.append(f"more than {_lib.CALLS_MAX_WINDOWS} windows, skipped: {ident}")
                return
            t = ticks(starts)
            ids, seg = bin_segments(t, per_bin)
            got = caller.call(scores, t, adjacent, seg)
            _add(result, ident, starts, got.events, got.peaks, ids, seg, per_bin, got.counts, got.values)

        _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed, recording_done)
        caller.close()
        result.messages = messages
        return result
    finally:
        if own:
            engine.close()


def call_results(dir_results: str, rules_by_class: Dict[str, Rule], *, bin_s: float = 60.0) -> CallResult:
    """The same rules by the host routines over the ``*_buzzdetect.csv`` activation files of a result tree ``analyze`` wrote; no
    device is needed.  Every file needs the ``start`` column and ``activation_<class>`` for every class of ``rules_by_class``;
    the framehop comes from the tree's manifest.  The values of such a file are the ROUNDED ones (two decimals by default):
    a window whose score lies within that rounding of a threshold can fall on the other side here than in
    ``call_recordings``, which sees the scores before rounding."""
    import pandas as pd
    from .results import MANIFEST_NAME, PREFIX_ACTIVATION, SUFFIX_COMPLETE
    per_bin = bin_ticks(bin_s)
    names = [str(c) for c in rules_by_class]
    rules = [rules_by_class[c] for c in rules_by_class]
    if not names or not all(isinstance(r, Rule) for r in rules):
        raise ValueError("rules_by_class must map at least one class to a Rule")
    manifest = os.path.join(dir_results, MANIFEST_NAME)
    if not os.path.exists(manifest):
        raise FileNotFoundError(f"{manifest} not found: the framehop of the tree is not known")
    with open(manifest) as f:
        framehop_s = FRAMELENGTH_S * float(json.load(f)["framehop_prop"])
    adjacent = adjacent_ticks(framehop_s)
    result = CallResult(names, [[] for _ in names], bin_s=per_bin / 100.0)
    paths = sorted(os.path.join(root, name) for root, _, files in os.walk(dir_results) for name in files
                   if name.endswith(SUFFIX_COMPLETE))
    for path in paths:
        ident = os.path.relpath(path, dir_results)[:-len(SUFFIX_COMPLETE)].replace(os.sep, "/")
        table = pd.read_csv(path)
        wanted = ["start"] + [PREFIX_ACTIVATION + c for c in names]
        absent = [c for c in wanted if c not in table.columns]
        if absent:
            raise ValueError(f"{path}: no column {', '.join(absent)}")
        starts = table["start"].to_numpy(np.float64)
        if starts.shape[0] > _lib.CALLS_MAX_WINDOWS:
            result.messages.append(f"more than {_lib.CALLS_MAX_WINDOWS} windows, skipped: {ident}")
            continue
        t = ticks(starts)
        if t.shape[0] > 1 and (np.diff(t.astype(np.int64)) <= 0).any():
            raise ValueError(f"{path}: the start column is not strictly increasing")
        scores = np.ascontiguousarray(table[wanted[1:]].to_numpy(np.float32))
        marks, events = events_host(scores, t, adjacent, rules)
        ids, seg = bin_segments(t, per_bin)
        counts, values = bins_host(scores, marks, seg)
        peaks = [scores[rows[:, PEAK], c] for c, rows in enumerate(events)]
        _add(result, ident, starts, events, peaks, ids, seg, per_bin, counts, values)
    return result
