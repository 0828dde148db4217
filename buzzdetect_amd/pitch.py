"""Wingbeat frequency of called buzzes: whose buzz was it?  Bumblebees, honey bees, hoverflies and mosquitoes beat their wings
in different bands between about 100 and 800 Hz, and the fundamental of a buzz is the cheapest physical answer.

    PitchTracker          ``track(samples, sel, step_samples)``: f0, clarity and voiced frames of selected windows of a chunk
    track_host            the library's host restatement of the definition, the same bits
    event_wingbeats       the windows of called events -> f0, its range, clarity and voiced windows per event (host)
    wingbeat_recordings   a folder of recordings through a model -> WingbeatResult: ``calls.call_recordings``'s events, each
                          with the wingbeat fundamental of its windows
    WingbeatResult        ``events``, ``to_csv``, ``table``

The definition is that of ``include/buzzdetect_pitch.h``: per frame of 1024 samples a normalised autocorrelation over the lags
of ``fmin .. fmax``, the greatest value of the first run above ``pick_ratio`` times the maximum behind the lag-0 lobe, refined
by a parabola; per window the lower median of its voiced frames.  It runs where the engine holds the samples
(csrc/pitch.hip), and only for the windows that can belong to an event - those a class scores above its ``low`` - because a
window costs about 6 M fused multiply-adds.

    from buzzdetect_amd import pitch

    found = pitch.wingbeat_recordings("audio_in", thresholds={"ins_buzz": -1.2}, low={"ins_buzz": -2.0}, merge_gap_s=2.0)
    found.to_csv("called")                              # <ident>_wingbeat.csv
    found.table()["f0"]                                 # Hz per event, NaN where no window of it is voiced
"""
from __future__ import annotations

import csv
import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, calls, framing
from .dataset import DIGITS_TIME, FRAMELENGTH_S, _store_of, _torch
from .search import _end, _logit_parts, _walk

RATE_HZ = 16000.0
STFT_HOP = 160                                  # samples of a spectrogram frame: a window starts at patch_step * 160 * k
WINGBEAT_COLUMNS = ("class", "start", "end", "windows", "detected", "peak", "f0", "f0_min", "f0_max", "clarity", "voiced_windows")
SUFFIX_WINGBEAT = "_wingbeat.csv"
TABLE = np.dtype([("ident", "O"), ("class", "O"), ("start", "<f8"), ("end", "<f8"), ("windows", "<i8"), ("detected", "<i8"),
                  ("peak", "<f4"), ("f0", "<f4"), ("f0_min", "<f4"), ("f0_max", "<f4"), ("clarity", "<f4"), ("voiced_windows", "<i8")])


def lag_range(fmin: float, fmax: float, rate_hz: float = RATE_HZ) -> Tuple[int, int]:
    """(lag_lo, lag_hi) = (ceil(rate / fmax), floor(rate / fmin)), refused unless 1 <= lag_lo <= lag_hi <= 511."""
    if not (fmin > 0 and fmax >= fmin and math.isfinite(fmax)):
        raise ValueError(f"fmin and fmax must be positive with fmin <= fmax, not fmin = {fmin}, fmax = {fmax}")
    lo, hi = int(math.ceil(rate_hz / fmax)), int(math.floor(rate_hz / fmin))
    if not 1 <= lo <= hi <= _lib.PITCH_MAX_LAG:
        raise ValueError(f"fmin = {fmin}, fmax = {fmax} at {rate_hz} Hz are the lags {lo}..{hi}; allowed are 1 <= lag_lo <= "
                         f"lag_hi <= {_lib.PITCH_MAX_LAG}")
    return lo, hi


def params(lag_lo: int, lag_hi: int, pick_ratio: float = 0.8, clarity_min: float = 0.5, min_voiced: int = 8,
           rate_hz: float = RATE_HZ) -> "_lib.bd_pitch_params":
    """``bd_pitch_params`` as given; the library checks them."""
    return _lib.bd_pitch_params(int(lag_lo), int(lag_hi), float(pick_ratio), float(clarity_min), int(min_voiced), float(rate_hz))


def _check_sel(sel) -> np.ndarray:
    sel = np.ascontiguousarray(sel, np.int32)
    if sel.ndim != 1 or sel.shape[0] > _lib.PITCH_MAX_SELECTED:
        raise ValueError(f"sel must be one int32 per selected window, at most {_lib.PITCH_MAX_SELECTED}")
    return sel


def track_host(samples, sel, step_samples: int, p=None, want_frames: bool = False):
    """``bd_pitch_windows_host``: (f0 float32 [S], clarity float32 [S], voiced int32 [S][, frames float32 [S, 29, 2]]) of the
    windows ``sel`` of the float32 chunk ``samples``; window k starts at sample ``k * step_samples``.  ``p``: ``params(...)``
    (default: the lags of 80..1000 Hz)."""
    x = np.ascontiguousarray(samples, np.float32)
    if x.ndim != 1:
        raise ValueError("samples must be one-dimensional")
    sel = _check_sel(sel)
    p = params(*lag_range(80.0, 1000.0)) if p is None else p
    s = sel.shape[0]
    values = np.zeros((s, 2), np.float32)
    voiced = np.zeros(s, np.int32)
    frames = np.zeros((s, _lib.PITCH_FRAMES, 2), np.float32) if want_frames else None
    _lib.check(_lib.load().bd_pitch_windows_host(x.ctypes.data if x.size else None, x.shape[0], sel.ctypes.data if s else None, s,
                                                 int(step_samples), C.addressof(p), values.ctypes.data if s else None,
                                                 voiced.ctypes.data if s else None, frames.ctypes.data if want_frames and s else None))
    out = (values[:, 0].copy(), values[:, 1].copy(), voiced)
    return out + (frames,) if want_frames else out


class PitchTracker:
    """The parameters of a tracker and the device side of tracking.  ``fmin`` / ``fmax``: the band of fundamentals in Hz (the
    lags ``ceil(16000 / fmax) .. floor(16000 / fmin)``); ``pick_ratio``, ``clarity_min``, ``min_voiced``: as
    ``include/buzzdetect_pitch.h`` defines them.  Everything runs on the current stream of ``device``."""

    def __init__(self, fmin: float = 80.0, fmax: float = 1000.0, pick_ratio: float = 0.8, clarity_min: float = 0.5,
                 min_voiced: int = 8, device=None):
        torch = _torch()
        self._lib = _lib.load()
        self.lag_lo, self.lag_hi = lag_range(fmin, fmax)
        if not (0 < pick_ratio <= 1) or not (0 < clarity_min <= 1):
            raise ValueError(f"pick_ratio and clarity_min must lie in (0, 1], not pick_ratio = {pick_ratio}, clarity_min = {clarity_min}")
        if not 1 <= int(min_voiced) <= _lib.PITCH_FRAMES:
            raise ValueError(f"min_voiced must be in 1..{_lib.PITCH_FRAMES}, not {min_voiced}")
        self.params = params(self.lag_lo, self.lag_hi, pick_ratio, clarity_min, min_voiced)
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; use track_host without one")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)

    def _empty(self, shape, dtype):
        """Every device buffer the kernel writes comes from here (the tests put guard words around them)."""
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def track_host(self, samples, sel, step_samples: int, want_frames: bool = False):
        """The same through ``bd_pitch_windows_host`` on host arrays: the same bits."""
        if type(samples).__module__.split(".")[0] == "torch":
            samples = samples.detach().cpu().numpy()
        if type(sel).__module__.split(".")[0] == "torch":
            sel = sel.detach().cpu().numpy()
        return track_host(samples, sel, step_samples, self.params, want_frames)

    def launch(self, samples_dev, sel, step_samples: int, want_frames: bool = False):
        """``track`` without the read-back: one launch on the current stream, nothing waited for.  Returns the device tensors
        (values float32 [S, 2]: f0, clarity; voiced int32 [S]; frames float32 [S, 29, 2] or None)."""
        torch = _torch()
        x = samples_dev
        if (not isinstance(x, torch.Tensor) or x.dim() != 1 or x.dtype != torch.float32 or x.device != self.device
                or not x.is_contiguous() or x.data_ptr() % 4):
            raise ValueError(f"samples must be a one-dimensional contiguous float32 tensor on {self.device}")
        if isinstance(sel, torch.Tensor):
            if sel.dim() != 1 or sel.dtype != torch.int32 or sel.device != self.device or sel.shape[0] > _lib.PITCH_MAX_SELECTED:
                raise ValueError(f"sel must be an int32 [S] tensor on {self.device}, S at most {_lib.PITCH_MAX_SELECTED}")
            sel_dev = sel.contiguous()
        else:
            sel_dev = torch.from_numpy(_check_sel(sel)).to(self.device)
        s = int(sel_dev.shape[0])
        values = self._empty((s, 2), torch.float32)
        voiced = self._empty((s,), torch.int32)
        frames = self._empty((s, _lib.PITCH_FRAMES, 2), torch.float32) if want_frames else None
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_pitch_windows(x.data_ptr() if x.numel() else None, int(x.numel()),
                                                  sel_dev.data_ptr() if s else None, s, int(step_samples), C.addressof(self.params),
                                                  values.data_ptr() if s else None, voiced.data_ptr() if s else None,
                                                  frames.data_ptr() if want_frames and s else None, stream.cuda_stream))
        for used in (x, sel_dev):
            used.record_stream(stream)
        return values, voiced, frames

    def track(self, samples_dev, sel, step_samples: int, want_frames: bool = False):
        """``samples_dev``: a contiguous float32 chunk on the device; ``sel``: int32 window indices (NumPy, or a tensor on the
        device); window k starts at sample ``k * step_samples``.  One launch; returns NumPy (f0 [S], clarity [S], voiced [S]
        [, frames [S, 29, 2]])."""
        values, voiced, frames = self.launch(samples_dev, sel, step_samples, want_frames)
        got = values.cpu().numpy()
        out = (got[:, 0].copy(), got[:, 1].copy(), voiced.cpu().numpy())
        return out + (frames.cpu().numpy(),) if want_frames else out


# ---------------------------------------------------------------------------------------------------- events
def lower_median(values: np.ndarray) -> int:
    """The index of the lower median of ``values`` (no NaN among them): ordered by value, then by index."""
    order = np.lexsort((np.arange(values.shape[0]), values))
    return int(order[(values.shape[0] - 1) // 2])


def event_wingbeats(rows: np.ndarray, marks: np.ndarray, f0: np.ndarray, clarity: np.ndarray) -> List[Tuple[float, float, float, float, int]]:
    """Per event of one column its (f0, f0_min, f0_max, clarity, voiced_windows).  ``rows``: int32 [n, 5] (first, last, n_on,
    peak, kept) as ``calls`` lists them; ``marks``: uint8 [W], that column's marks (not 0: the window is ON); ``f0`` /
    ``clarity``: float32 [W] of the recording's windows, f0 a NaN where a window is unvoiced or was not tracked.  An event's f0
    is the lower median of the f0 of its ON, voiced windows (by value, then window), its clarity that window's; f0_min and
    f0_max span those windows; without a voiced window the three are NaN and the clarity 0."""
    out = []
    for first, last, *_ in np.asarray(rows).reshape(-1, _lib.CALLS_EVENT_FIELDS):
        span = np.arange(int(first), int(last) + 1)
        at = span[(marks[span] != 0) & ~np.isnan(f0[span])]
        if at.size == 0:
            out.append((float("nan"), float("nan"), float("nan"), 0.0, 0))
            continue
        mid = at[lower_median(f0[at])]
        out.append((float(f0[mid]), float(f0[at].min()), float(f0[at].max()), float(clarity[mid]), int(at.size)))
    return out


@dataclass
class WingbeatResult:
    """``events[c]``: the kept events of ``classes[c]`` in the order of the walk, each ``calls.CallResult``'s (ident, start, end,
    windows, detected, peak, peak_start) followed by (f0, f0_min, f0_max, clarity, voiced_windows).  ``idents``: every recording
    that was walked."""
    classes: List[str]
    events: List[List[tuple]]
    idents: List[str] = field(default_factory=list)
    messages: List[str] = field(default_factory=list)
    digits_results: int = 2

    def calls(self) -> List[List[tuple]]:
        """The events as ``calls.call_recordings`` lists them."""
        return [[e[:7] for e in found] for found in self.events]

    def table(self) -> np.ndarray:
        """All events as one array with the fields ``ident`` and ``WINGBEAT_COLUMNS``: class by class, in the order of the walk."""
        rows = [(e[0], name, e[1], e[2], e[3], e[4], e[5], e[7], e[8], e[9], e[10], e[11])
                for name, found in zip(self.classes, self.events) for e in found]
        return np.array(rows, dtype=TABLE)

    def to_csv(self, dir_out: str) -> None:
        """Per recording ``<ident>_wingbeat.csv`` (``WINGBEAT_COLUMNS``) under ``dir_out``, in the layout of ``analyze``'s tree;
        a recording without events gets the header alone."""
        for ident in self.idents:
            base = os.path.join(dir_out, ident)
            os.makedirs(os.path.dirname(base) or ".", exist_ok=True)
            with open(base + SUFFIX_WINGBEAT, "w", newline="") as f:
                out = csv.writer(f, lineterminator="\n")
                out.writerow(WINGBEAT_COLUMNS)
                for name, found in zip(self.classes, self.events):
                    for e in found:
                        if e[0] == ident:
                            out.writerow([name, repr(float(e[1])), repr(float(e[2])), int(e[3]), int(e[4]),
                                          str(np.round(np.float32(e[5]), self.digits_results))]
                                         + [repr(float(np.float32(v))) for v in e[7:11]] + [int(e[11])])


# ---------------------------------------------------------------------------------------------------- folders
def wingbeat_recordings(dir_audio: str, modelname: Optional[str] = "model_general_v3", *, classes: Sequence[str] = ("ins_buzz",),
                        thresholds: Optional[Dict[str, float]] = None, precision: Optional[float] = None, low=None,
                        merge_gap_s: float = 0.0, min_duration_s: float = 0.0, fmin: float = 80.0, fmax: float = 1000.0,
                        pick_ratio: float = 0.8, clarity_min: float = 0.5, min_voiced: int = 8, engine=None,
                        framehop_prop: float = 1.0, chunklength: float = 200, embeddername: str = "yamnet_k2",
                        models_dir: Optional[str] = None) -> WingbeatResult:
    """The events ``calls.call_recordings`` finds under ``dir_audio`` with the same arguments, each with its wingbeat
    fundamental.  While a launch set's chunks are still on the device, the windows of every chunk that some class scores above
    its ``low`` - an ON window can be nothing else - are tracked (``PitchTracker``), and only those; after a recording's last
    set its events are called as ``call_recordings`` calls them and get the f0 of their ON, voiced windows
    (``event_wingbeats``).  An embedding store holds no audio and is refused."""
    from .engine import HipEngine
    from . import results
    if _store_of(dir_audio) is not None:
        raise ValueError("wingbeat_recordings needs the recordings themselves: an embedding store holds no audio")
    framehop_s = FRAMELENGTH_S * framehop_prop
    adjacent = calls.adjacent_ticks(framehop_s)
    names = [str(c) for c in classes]
    highs = {} if thresholds is None else {str(k): float(v) for k, v in thresholds.items()}
    if precision is not None and "ins_buzz" not in highs:
        highs["ins_buzz"] = results.threshold_for_precision(modelname, precision)
    missing = [c for c in names if c not in highs]
    if missing or not names:
        raise ValueError(f"no threshold for {missing}: give thresholds={{class: high}} (or precision, for ins_buzz)" if missing
                         else "no classes")
    lows = low if isinstance(low, dict) else {c: low for c in names}
    rules = [calls.Rule(highs[c], lows.get(c), merge_gap_s, min_duration_s) for c in names]
    lag_range(fmin, fmax)                                   # (refused before an engine is built)
    messages: List[str] = []
    own = engine is None
    if own:
        engine = HipEngine(embeddername=embeddername, modelname=modelname, models_dir=models_dir)
    try:
        if not engine.n_classes:
            raise ValueError("wingbeat_recordings needs an engine with a classifier")
        absent = [c for c in names if c not in engine.classes]
        if absent:
            raise ValueError(f"classes {absent} are not among the model's {list(engine.classes)}")
        torch = _torch()
        columns = torch.tensor([engine.classes.index(c) for c in names], dtype=torch.int64, device=engine.device)
        floor = torch.tensor([r.packed(adjacent)[1] for r in rules], dtype=torch.float32, device=engine.device)
        caller = calls.Caller(rules, device=engine.device)
        tracker = PitchTracker(fmin, fmax, pick_ratio, clarity_min, min_voiced, device=engine.device)
        result = WingbeatResult(names, [[] for _ in names])
        held: List[object] = []
        tracked: List[Tuple[np.ndarray, np.ndarray]] = []      # per launch set of the recording: (f0, clarity) of all its windows
        fed = [0]

        def feed(parts, hop, step):
            logits, counts = _logit_parts(engine, parts, hop, step)
            scores = logits.index_select(1, columns)
            held.append(scores)
            counts = [int(n) for n in counts]
            edges = np.concatenate([[0], np.cumsum(counts)])
            # the set's candidates in one read-back (how many each part has decides the launches), every part's launch behind
            # it without waiting, and one read-back of all the results
            where_dev = torch.nonzero((scores > floor).any(dim=1)).flatten()
            where = where_dev.cpu().numpy()
            cuts = np.searchsorted(where, edges)
            pending = [tracker.launch(part, (where_dev[a:b] - int(lo)).to(torch.int32), step * STFT_HOP)[0]
                       for part, lo, a, b in zip(parts, edges[:-1], cuts[:-1], cuts[1:]) if b > a]
            f0 = np.full(int(edges[-1]), np.nan, np.float32)
            clarity = np.zeros(int(edges[-1]), np.float32)
            if pending:
                values = torch.cat(pending).cpu().numpy()
                f0[where], clarity[where] = values[:, 0], values[:, 1]
            tracked.append((f0, clarity))
            first = fed[0]
            fed[0] += int(sum(counts))
            return first, counts

        def recording_done(ident, chunk_starts, counts):
            scores = torch.cat(held) if held else torch.zeros((0, len(names)), dtype=torch.float32, device=engine.device)
            held.clear()
            f0 = np.concatenate([t[0] for t in tracked] + [np.zeros(0, np.float32)])
            clarity = np.concatenate([t[1] for t in tracked] + [np.zeros(0, np.float32)])
            tracked.clear()
            starts = np.concatenate([framing.window_starts(n, s, framehop_s, DIGITS_TIME) for s, n in zip(chunk_starts, counts)]
                                    + [np.zeros(0)])
            if starts.shape[0] > _lib.CALLS_MAX_WINDOWS:
                messages.append(f"more than {_lib.CALLS_MAX_WINDOWS} windows, skipped: {ident}")
                return
            result.idents.append(ident)
            got = caller.call(scores, calls.ticks(starts), adjacent)
            for c, (rows, peaks) in enumerate(zip(got.events, got.peaks)):
                for row, peak, beat in zip(rows, peaks, event_wingbeats(rows, got.marks[c], f0, clarity)):
                    if row[calls.KEPT]:
                        result.events[c].append((ident, float(starts[row[calls.FIRST]]), _end(starts[row[calls.LAST]], FRAMELENGTH_S),
                                                 int(row[calls.LAST] - row[calls.FIRST] + 1), int(row[calls.N_ON]), float(peak),
                                                 float(starts[row[calls.PEAK]])) + beat)

        _walk(dir_audio, engine, framehop_prop, chunklength, messages, feed, recording_done)
        caller.close()
        result.messages = messages
        return result
    finally:
        if own:
            engine.close()
