"""Recording health per bin: could anything have been heard?  ``calls`` reports "0 buzzes" for a minute in which the microphone
was dead, the recorder wrote digital silence, the gain clipped or wind buried the band the buzz lives in; a rate per bin needs an
effort column beside it.  The numbers are taken from the samples where the chunks already lie, on the device.

    HealthMeter           ``levels(raw, rate, first_frame)``: peak, level, DC, clipped and stuck runs of a chunk of native
                          samples per bin and channel; ``spectrum(pcm16k, start_s)``: band powers of the 16 kHz mono chunk per
                          bin; ``levels_host`` / ``spectrum_host``: the library's host restatements, the same bits
    health_recordings     a folder of recordings -> HealthResult, read in ``analyze``'s chunks; no classifier is needed
    HealthResult          ``table``, ``to_csv`` (``<ident>_health.csv``, ``<ident>_ltsa.csv``), ``flags``

The definitions are those of ``include/buzzdetect_health.h``.  Bins are the bins of ``<ident>_buzzbins.csv``: sample ``i`` of a
recording at ``rate`` lies in bin ``(100 i) // (rate * calls.bin_ticks(bin_s))``, in exact integer arithmetic.  The per-bin band
levels, stacked over a day, are the long-term spectral average (``<ident>_ltsa.csv``).  Levels are in dB re a full-scale square
wave (power 1.0): a full-scale sine reads -3.01 dB.

    from buzzdetect_amd import health

    found = health.health_recordings("audio_in", bin_s=60.0)
    found.to_csv("called")                              # <ident>_health.csv, <ident>_ltsa.csv
    found.flags(band_rules={"wind": ((0, 125), (250, 2000), 20.0)})["rec1"]     # [(bin_start, usable, reasons), ..]
"""
from __future__ import annotations

import csv
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, calls, framing
from .dataset import DIGITS_TIME, FRAMELENGTH_S, _read_chunks, _recordings, _store_of, _torch

RATE_16K = 16000
BIN_HZ = RATE_16K / _lib.HEALTH_FRAME            # 15.625 Hz
DEFAULT_BANDS = (0, 62.5, 125, 250, 500, 1000, 2000, 4000, 8000)
SPECTRUM_SEGMENT = 16                            # frames of a spectrum segment as the meter cuts them (frame_segments)
RECORD = np.dtype([("n", "<i4"), ("nonfinite", "<i4"), ("peak", "<f4"), ("sum", "<f4"), ("sumsq", "<f4"), ("n_full", "<i4"),
                   ("clipped", "<i4"), ("clip_runs", "<i4"), ("flat", "<i4"), ("flat_runs", "<i4")])       # bd_health_record
COUNTS = ("n", "nonfinite", "n_full", "clipped", "clip_runs", "flat", "flat_runs")
SUFFIX_HEALTH = "_health.csv"
SUFFIX_LTSA = "_ltsa.csv"
HEALTH_COLUMNS = ("bin_start", "channel", "seconds", "peak_dbfs", "rms_dbfs", "dc", "full", "clipped", "clip_runs", "flat",
                  "flat_runs", "nonfinite")
assert RECORD.itemsize == C.sizeof(_lib.bd_health_record) == 40


def band_bins(bands: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """(the band edges in Hz, rounded to multiples of 15.625 Hz; bedges int32 [B + 1], the FFT bins they are).  Refused unless
    strictly ascending within 0..8000 after rounding, with 1..64 bands.  An edge at 8000 Hz becomes bin 513, so that a band that
    ends there holds the Nyquist bin and a cover of 0..8000 holds all the power."""
    hz = np.asarray(list(bands), np.float64)
    if hz.ndim != 1 or not 2 <= hz.shape[0] <= _lib.HEALTH_MAX_BANDS + 1 or not np.isfinite(hz).all():
        raise ValueError(f"bands must be 2..{_lib.HEALTH_MAX_BANDS + 1} finite edges in Hz, not {bands}")
    k = np.round(hz / BIN_HZ).astype(np.int64)
    if k[0] < 0 or k[-1] > _lib.HEALTH_FRAME // 2 or (np.diff(k) <= 0).any():
        raise ValueError(f"bands must be strictly ascending within 0..8000 Hz in steps of {BIN_HZ} Hz, not {bands}")
    bedges = np.where(k == _lib.HEALTH_FRAME // 2, _lib.HEALTH_BINS, k).astype(np.int32)
    return k * BIN_HZ, bedges


def level_params(clip_hi: float, clip_lo: float, clip_run: int, flat_run: int) -> "_lib.bd_health_level_params":
    """``bd_health_level_params`` as given; the library checks them."""
    return _lib.bd_health_level_params(float(clip_hi), float(clip_lo), int(clip_run), int(flat_run))


def cut_segments(first: int, n: int, rate: int, bin_ticks: int, max_len: int) -> Tuple[np.ndarray, np.ndarray]:
    """Items ``first .. first + n - 1`` of a recording at ``rate`` items per second, cut where the bin changes and every
    ``max_len`` items inside a bin: (edges int64 [S + 1] counted from ``first``, the bin of each segment int64 [S]).  Item ``i``
    lies in bin ``(100 i) // (rate * bin_ticks)``; Python integers, so nothing rounds."""
    first, n, per = int(first), int(n), int(rate) * int(bin_ticks)
    if first < 0 or n < 0 or per < 1 or max_len < 1:
        raise ValueError(f"first = {first}, n = {n}, rate = {rate}, bin_ticks = {bin_ticks} do not describe a stretch of a recording")
    edges, bins = [np.zeros(1, np.int64)], []
    if n:
        for b in range((100 * first) // per, (100 * (first + n - 1)) // per + 1):
            lo = max(first, -((-b * per) // 100)) - first             # the bin's first item: ceil(b * per / 100)
            hi = min(first + n, -((-(b + 1) * per) // 100)) - first
            if hi <= lo:
                continue
            cuts = np.arange(lo, hi, max_len, dtype=np.int64)
            edges.append(np.concatenate([cuts[1:], [hi]]).astype(np.int64))
            bins.append(np.full(cuts.shape[0], b, np.int64))
    return np.concatenate(edges), np.concatenate(bins + [np.zeros(0, np.int64)])


def frame_segments(first16: int, n16: int, bin_ticks: int, max_len: int = SPECTRUM_SEGMENT) -> Tuple[np.ndarray, np.ndarray]:
    """The whole frames of a 16 kHz chunk that starts at sample ``first16`` of its recording, each in the bin of its first
    sample, cut where the bin changes and every ``max_len`` frames: (fedges int64 [T + 1], the bin of each segment int64 [T]).
    The library takes up to 64 frames a segment; a segment is one workgroup that takes four frames at a time, so 16 gives a
    200 s chunk 393 workgroups for the device's 256 compute units where 64 gives it 100, and the bins are added up in float64
    on the host either way."""
    if not 1 <= int(max_len) <= _lib.HEALTH_SEGMENT_FRAMES:
        raise ValueError(f"max_len must be in 1..{_lib.HEALTH_SEGMENT_FRAMES}, not {max_len}")
    frames = (int(n16) - _lib.HEALTH_FRAME) // _lib.HEALTH_HOP + 1 if n16 >= _lib.HEALTH_FRAME else 0
    of = (100 * (int(first16) + _lib.HEALTH_HOP * np.arange(frames, dtype=np.int64))) // (RATE_16K * int(bin_ticks))
    starts = np.flatnonzero(np.concatenate([[True], of[1:] != of[:-1]])) if frames else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [frames]]).astype(np.int64)
    edges, bins = [np.zeros(1, np.int64)], []
    for lo, hi in zip(starts, ends):
        cuts = np.arange(lo, hi, int(max_len), dtype=np.int64)
        edges.append(np.concatenate([cuts[1:], [hi]]).astype(np.int64))
        bins.append(np.full(cuts.shape[0], of[lo], np.int64))
    return np.concatenate(edges), np.concatenate(bins + [np.zeros(0, np.int64)])


def _check_cover(edges: np.ndarray, total: int, max_len: int, what: str) -> np.ndarray:
    edges = np.ascontiguousarray(edges, np.int64)
    if edges.ndim != 1 or edges.shape[0] < 1:
        raise ValueError(f"{what} must be int64 [S + 1]")
    _lib.check(_lib.load().bd_health_check_cover(edges.ctypes.data, edges.shape[0] - 1, int(total), int(max_len), what.encode()))
    return edges


def _dtype_code(dtype) -> int:
    name = str(dtype).replace("torch.", "")
    if name not in ("int16", "float32"):
        raise ValueError(f"raw samples must be int16 or float32, not {dtype}")
    return _lib.HEALTH_S16 if name == "int16" else _lib.HEALTH_F32


def levels_records_host(x: np.ndarray, edges, p) -> np.ndarray:
    """``bd_health_levels_host``: the records (``RECORD`` [S, channels]) of the segments ``edges`` of ``x`` [n, channels]."""
    x = np.ascontiguousarray(x)
    if x.ndim == 1:
        x = x[:, None]
    code = _dtype_code(x.dtype)
    edges = np.ascontiguousarray(edges, np.int64)
    s = edges.shape[0] - 1
    records = np.zeros((s, x.shape[1]), RECORD)
    _lib.check(_lib.load().bd_health_levels_host(x.ctypes.data if x.size else None, code, x.shape[0], x.shape[1], edges.ctypes.data, s,
                                                 C.addressof(p), records.ctypes.data if s else None))
    return records


def spectrum_host(x16k: np.ndarray, fedges, bedges, tables: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_health_spectrum_host``: (power float32 [T, B], bad_frames int32 [T])."""
    x = np.ascontiguousarray(x16k, np.float32)
    fedges, bedges = np.ascontiguousarray(fedges, np.int64), np.ascontiguousarray(bedges, np.int32)
    t, b = fedges.shape[0] - 1, bedges.shape[0] - 1
    power, bad = np.zeros((t, max(b, 0)), np.float32), np.zeros(t, np.int32)
    _lib.check(_lib.load().bd_health_spectrum_host(x.ctypes.data if x.size else None, x.shape[0], fedges.ctypes.data, t, bedges.ctypes.data, b,
                                                   tables.ctypes.data, power.ctypes.data if t else None, bad.ctypes.data if t else None))
    return power, bad


def tables() -> np.ndarray:
    """``bd_health_tables``: the window and the twiddles, float32 [2048]."""
    out = np.zeros(_lib.HEALTH_TABLE_FLOATS, np.float32)
    _lib.check(_lib.load().bd_health_tables(out.ctypes.data))
    return out


@dataclass
class LevelBins:
    """The levels of a stretch of a recording merged into bins: ``bins`` int64 [nb] ascending; ``counts[name]`` int64 [nb, ch] for
    ``COUNTS``; ``peak``, ``sum``, ``sumsq`` float64 [nb, ch]."""
    bins: np.ndarray
    counts: Dict[str, np.ndarray]
    peak: np.ndarray
    sum: np.ndarray
    sumsq: np.ndarray


@dataclass
class SpectrumBins:
    """``bins`` int64 [nb]; ``frames`` / ``bad_frames`` int64 [nb] (good and bad); ``power`` float64 [nb, B], summed over good frames."""
    bins: np.ndarray
    frames: np.ndarray
    bad_frames: np.ndarray
    power: np.ndarray


def merge_levels(parts: Sequence[LevelBins]) -> LevelBins:
    """Several stretches of one recording as one: records of the same bin are added in the order given, in float64."""
    ch = parts[0].peak.shape[1] if parts else 1
    ids = np.unique(np.concatenate([p.bins for p in parts] + [np.zeros(0, np.int64)]))
    out = LevelBins(ids, {k: np.zeros((ids.shape[0], ch), np.int64) for k in COUNTS}, np.zeros((ids.shape[0], ch)),
                    np.zeros((ids.shape[0], ch)), np.zeros((ids.shape[0], ch)))
    for p in parts:
        at = np.searchsorted(ids, p.bins)
        for k in COUNTS:
            np.add.at(out.counts[k], at, p.counts[k])
        np.maximum.at(out.peak, at, p.peak)
        np.add.at(out.sum, at, p.sum)
        np.add.at(out.sumsq, at, p.sumsq)
    return out


def merge_spectrum(parts: Sequence[SpectrumBins], n_bands: int) -> SpectrumBins:
    ids = np.unique(np.concatenate([p.bins for p in parts] + [np.zeros(0, np.int64)]))
    out = SpectrumBins(ids, np.zeros(ids.shape[0], np.int64), np.zeros(ids.shape[0], np.int64), np.zeros((ids.shape[0], n_bands)))
    for p in parts:
        at = np.searchsorted(ids, p.bins)
        np.add.at(out.frames, at, p.frames)
        np.add.at(out.bad_frames, at, p.bad_frames)
        np.add.at(out.power, at, p.power)
    return out


def _level_bins(records: np.ndarray, seg_bins: np.ndarray) -> LevelBins:
    """Records [S, ch] into bins, in segment order, in float64."""
    return merge_levels([LevelBins(seg_bins, {k: records[k].astype(np.int64) for k in COUNTS}, records["peak"].astype(np.float64),
                                   records["sum"].astype(np.float64), records["sumsq"].astype(np.float64))])


def _spectrum_bins(power: np.ndarray, bad: np.ndarray, fedges: np.ndarray, seg_bins: np.ndarray) -> SpectrumBins:
    n = np.diff(fedges).astype(np.int64)
    one = SpectrumBins(seg_bins, n - bad.astype(np.int64), bad.astype(np.int64), power.astype(np.float64))
    return merge_spectrum([one], power.shape[1])


class HealthMeter:
    """The parameters of a meter and both sides of metering.  ``bin_s``: a positive multiple of 0.01 s (``calls.bin_ticks``).
    ``clip_level``: a sample at or beyond +-clip_level is at full scale (default: 32767/32768 and -1.0 for 16-bit sources, +-0.9999
    for float sources); ``clip_run``: consecutive such samples that count as clipped; ``flat_s``: the seconds of identical
    samples that count as stuck (at least 2 samples).  ``bands``: edges in Hz, rounded to multiples of 15.625 Hz
    (``band_bins``).  The host forms need no device; the device forms run on the current stream of ``device``."""

    def __init__(self, bin_s: float = 60.0, clip_level: Optional[float] = None, clip_run: int = 3, flat_s: float = 0.02,
                 bands: Sequence[float] = DEFAULT_BANDS, device=None):
        self._lib = _lib.load()
        self.bin_ticks = calls.bin_ticks(bin_s)
        self.bin_s = self.bin_ticks / 100.0
        if clip_level is not None and not 0 < float(clip_level) < float("inf"):
            raise ValueError(f"clip_level must be positive and finite, not {clip_level}")
        if not 1 <= int(clip_run) <= _lib.HEALTH_MAX_RUN:
            raise ValueError(f"clip_run must be in 1..{_lib.HEALTH_MAX_RUN}, not {clip_run}")
        if not 0 < float(flat_s) < float("inf"):
            raise ValueError(f"flat_s must be positive and finite, not {flat_s}")
        self.clip_level, self.clip_run, self.flat_s = clip_level, int(clip_run), float(flat_s)
        self.band_hz, self.bedges = band_bins(bands)
        self.tables = tables()
        self._device = device
        self._tables_dev = None

    @property
    def n_bands(self) -> int:
        return self.bedges.shape[0] - 1

    @property
    def device(self):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; use levels_host / spectrum_host without one")
        d = self._device
        if d is None:
            d = torch.device("cuda", torch.cuda.current_device())
        self._device = torch.device(d) if not isinstance(d, int) else torch.device("cuda", d)
        return self._device

    def _empty(self, shape, dtype):
        """Every device buffer the kernels write comes from here (the tests put guard words around them)."""
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def params(self, is_s16: bool, rate: int) -> "_lib.bd_health_level_params":
        """The level parameters for a source of this sample type and rate."""
        if self.clip_level is not None:
            hi, lo = self.clip_level, -self.clip_level
        else:
            hi, lo = (32767.0 / 32768.0, -1.0) if is_s16 else (0.9999, -0.9999)
        flat_run = min(max(2, int(round(self.flat_s * int(rate)))), _lib.HEALTH_MAX_RUN)
        return level_params(hi, lo, self.clip_run, flat_run)

    # ------------------------------------------------------------------------------------------------ levels
    def level_segments(self, n_frames: int, rate: int, first_frame: int) -> Tuple[np.ndarray, np.ndarray]:
        return cut_segments(first_frame, n_frames, rate, self.bin_ticks, _lib.HEALTH_SEGMENT)

    def levels_host(self, raw, rate: int, first_frame: int = 0) -> LevelBins:
        """``levels`` through ``bd_health_levels_host`` on host arrays: the same bits."""
        if type(raw).__module__.split(".")[0] == "torch":
            raw = raw.detach().cpu().numpy()
        x = np.ascontiguousarray(raw)
        x = x[:, None] if x.ndim == 1 else x
        edges, seg_bins = self.level_segments(x.shape[0], rate, first_frame)
        return _level_bins(levels_records_host(x, edges, self.params(x.dtype == np.int16, rate)), seg_bins)

    def launch_levels(self, raw_dev, edges, p):
        """Three launches on the current stream, nothing waited for: the records as an int32 tensor [S, channels, 10]."""
        torch = _torch()
        x = raw_dev
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.device != self.device or not x.is_contiguous():
            raise ValueError(f"raw must be a contiguous [frames, channels] int16 or float32 tensor on {self.device}")
        code = _dtype_code(x.dtype)
        n, ch = int(x.shape[0]), int(x.shape[1])
        edges = _check_cover(edges, n, _lib.HEALTH_SEGMENT, "edges")
        s = edges.shape[0] - 1
        records = self._empty((s, ch, RECORD.itemsize // 4), torch.int32)
        if s == 0:
            return records
        need = _lib.check(self._lib.bd_health_levels_workspace_bytes(s, ch))
        workspace = self._empty((need // 4,), torch.int32)
        edges_dev = torch.from_numpy(edges).to(self.device)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_health_levels(x.data_ptr(), code, n, ch, edges_dev.data_ptr(), s, C.addressof(p), records.data_ptr(),
                                                  workspace.data_ptr(), need, stream.cuda_stream))
        for used in (x, edges_dev):
            used.record_stream(stream)
        return records

    def levels(self, raw_dev, rate: int, first_frame: int = 0) -> LevelBins:
        """``raw_dev``: a chunk as ``HipEngine.read_audio(raw=True)`` returns it, whose first frame is frame ``first_frame`` of
        its recording at ``rate``.  One read-back."""
        edges, seg_bins = self.level_segments(int(raw_dev.shape[0]), rate, first_frame)
        records = self.launch_levels(raw_dev, edges, self.params(str(raw_dev.dtype).endswith("int16"), rate))
        return _level_bins(records.cpu().numpy().view(RECORD)[..., 0], seg_bins)

    # ------------------------------------------------------------------------------------------------ spectrum
    def spectrum_host(self, pcm16k, start_s: float = 0.0) -> SpectrumBins:
        """``spectrum`` through ``bd_health_spectrum_host`` on a host array: the same bits."""
        if type(pcm16k).__module__.split(".")[0] == "torch":
            pcm16k = pcm16k.detach().cpu().numpy()
        x = np.ascontiguousarray(pcm16k, np.float32)
        fedges, seg_bins = frame_segments(int(round(float(start_s) * RATE_16K)), x.shape[0], self.bin_ticks)
        power, bad = spectrum_host(x, fedges, self.bedges, self.tables)
        return _spectrum_bins(power, bad, fedges, seg_bins)

    def launch_spectrum(self, pcm_dev, fedges):
        """One launch on the current stream, nothing waited for: (power float32 [T, B], bad_frames int32 [T]) on the device."""
        torch = _torch()
        x = pcm_dev
        if (not isinstance(x, torch.Tensor) or x.dim() != 1 or x.dtype != torch.float32 or x.device != self.device
                or not x.is_contiguous() or x.data_ptr() % 4):
            raise ValueError(f"pcm16k must be a one-dimensional contiguous float32 tensor on {self.device}")
        n = int(x.numel())
        frames = (n - _lib.HEALTH_FRAME) // _lib.HEALTH_HOP + 1 if n >= _lib.HEALTH_FRAME else 0
        fedges = _check_cover(fedges, frames, _lib.HEALTH_SEGMENT_FRAMES, "fedges")
        t = fedges.shape[0] - 1
        power = self._empty((t, self.n_bands), torch.float32)
        bad = self._empty((t,), torch.int32)
        if t == 0:
            return power, bad
        if self._tables_dev is None:
            self._tables_dev = torch.from_numpy(self.tables).to(self.device)
        fedges_dev = torch.from_numpy(fedges).to(self.device)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_health_spectrum(x.data_ptr(), n, fedges_dev.data_ptr(), t, self.bedges.ctypes.data, self.n_bands,
                                                    self._tables_dev.data_ptr(), power.data_ptr(), bad.data_ptr(), stream.cuda_stream))
        for used in (x, fedges_dev, self._tables_dev):
            used.record_stream(stream)
        return power, bad

    def spectrum(self, pcm_dev, start_s: float = 0.0) -> SpectrumBins:
        """``pcm_dev``: the 16 kHz mono chunk the embedder gets, whose first sample lies ``start_s`` into its recording.  One
        read-back (power and bad_frames travel as one tensor)."""
        torch = _torch()
        fedges, seg_bins = frame_segments(int(round(float(start_s) * RATE_16K)), int(pcm_dev.numel()), self.bin_ticks)
        power, bad = self.launch_spectrum(pcm_dev, fedges)
        both = torch.cat([power.view(torch.int32), bad[:, None]], dim=1).cpu().numpy()
        return _spectrum_bins(np.ascontiguousarray(both[:, :-1]).view(np.float32), both[:, -1], fedges, seg_bins)


# ---------------------------------------------------------------------------------------------------- results
def _db(power: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(power)


@dataclass
class RecordingHealth:
    """One recording, per bin that holds samples.  ``bin_start`` seconds [nb]; ``seconds`` [nb]: the audio in the bin; per
    channel [nb, ch]: ``peak_dbfs``, ``rms_dbfs`` (-inf for digital silence), ``dc``, ``samples``, ``full``, ``clipped``,
    ``clip_runs``, ``flat``, ``flat_runs``, ``nonfinite``; of the 16 kHz mono mix: ``frames`` (good) and ``bad_frames`` [nb] and
    ``band_power`` [nb, B], the mean power of a good frame per band (NaN without one; ``band_db`` in dB)."""
    rate: int
    bin_start: np.ndarray
    seconds: np.ndarray
    peak_dbfs: np.ndarray
    rms_dbfs: np.ndarray
    dc: np.ndarray
    samples: np.ndarray
    full: np.ndarray
    clipped: np.ndarray
    clip_runs: np.ndarray
    flat: np.ndarray
    flat_runs: np.ndarray
    nonfinite: np.ndarray
    frames: np.ndarray
    bad_frames: np.ndarray
    band_power: np.ndarray

    @property
    def band_db(self) -> np.ndarray:
        return _db(self.band_power)


def recording_health(levels: LevelBins, spectrum: SpectrumBins, rate: int, bin_ticks: int) -> RecordingHealth:
    """The merged bins of one recording as a ``RecordingHealth``; its bins are those that hold samples."""
    ids = levels.bins
    n = levels.counts["n"].astype(np.float64)
    nb, bands = ids.shape[0], spectrum.power.shape[1]
    frames, bad, power = np.zeros(nb, np.int64), np.zeros(nb, np.int64), np.full((nb, bands), np.nan)
    at = np.searchsorted(ids, spectrum.bins)
    ok = (at < nb) & (ids[np.minimum(at, max(nb - 1, 0))] == spectrum.bins) if nb else np.zeros(spectrum.bins.shape[0], bool)
    frames[at[ok]], bad[at[ok]] = spectrum.frames[ok], spectrum.bad_frames[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        power[at[ok]] = spectrum.power[ok] / spectrum.frames[ok, None]
        rms, peak, dc = _db(levels.sumsq / n), 2.0 * _db(levels.peak), levels.sum / n
    c = levels.counts
    return RecordingHealth(int(rate), ids.astype(np.float64) * bin_ticks / 100.0, n[:, 0] / float(rate), peak, rms, dc, c["n"], c["n_full"],
                           c["clipped"], c["clip_runs"], c["flat"], c["flat_runs"], c["nonfinite"], frames, bad, power)


def _band_name(lo: float, hi: float) -> str:
    return f"band_{lo:g}_{hi:g}"


@dataclass
class HealthResult:
    """``recordings[ident]``: that recording's ``RecordingHealth``; ``band_hz``: the band edges in Hz."""
    band_hz: np.ndarray
    recordings: Dict[str, RecordingHealth] = field(default_factory=dict)
    messages: List[str] = field(default_factory=list)
    bin_s: float = 60.0

    def band_names(self) -> List[str]:
        return [_band_name(a, b) for a, b in zip(self.band_hz[:-1], self.band_hz[1:])]

    def table(self) -> np.ndarray:
        """One row per (recording, bin, channel): ``ident`` and ``HEALTH_COLUMNS``, then ``frames``, ``bad_frames`` and a column
        of dB per band of the mono mix (the same on every channel's row)."""
        names = self.band_names()
        dtype = np.dtype([("ident", "O"), ("bin_start", "<f8"), ("channel", "<i8"), ("seconds", "<f8"), ("peak_dbfs", "<f8"),
                          ("rms_dbfs", "<f8"), ("dc", "<f8"), ("full", "<i8"), ("clipped", "<i8"), ("clip_runs", "<i8"), ("flat", "<i8"),
                          ("flat_runs", "<i8"), ("nonfinite", "<i8"), ("frames", "<i8"), ("bad_frames", "<i8")] + [(k, "<f8") for k in names])
        rows = []
        for ident, r in self.recordings.items():
            db = r.band_db
            for b in range(r.bin_start.shape[0]):
                for c in range(r.peak_dbfs.shape[1]):
                    rows.append((ident, r.bin_start[b], c, r.seconds[b], r.peak_dbfs[b, c], r.rms_dbfs[b, c], r.dc[b, c], r.full[b, c],
                                 r.clipped[b, c], r.clip_runs[b, c], r.flat[b, c], r.flat_runs[b, c], r.nonfinite[b, c], r.frames[b],
                                 r.bad_frames[b]) + tuple(db[b]))
        return np.array(rows, dtype=dtype)

    def to_csv(self, dir_out: str) -> None:
        """Per recording ``<ident>_health.csv`` (``HEALTH_COLUMNS``, one row per bin and channel, levels with two decimals) and
        ``<ident>_ltsa.csv`` (``bin_start,frames,bad_frames`` and a column of dB per band, one row per bin) under ``dir_out``, in
        the layout of ``analyze``'s tree."""
        for ident, r in self.recordings.items():
            base = os.path.join(dir_out, ident)
            os.makedirs(os.path.dirname(base) or ".", exist_ok=True)
            with open(base + SUFFIX_HEALTH, "w", newline="") as f:
                out = csv.writer(f, lineterminator="\n")
                out.writerow(HEALTH_COLUMNS)
                for b in range(r.bin_start.shape[0]):
                    for c in range(r.peak_dbfs.shape[1]):
                        out.writerow([repr(float(r.bin_start[b])), c, repr(round(float(r.seconds[b]), 6)), f"{r.peak_dbfs[b, c]:.2f}",
                                      f"{r.rms_dbfs[b, c]:.2f}", f"{r.dc[b, c]:.6f}", int(r.full[b, c]), int(r.clipped[b, c]),
                                      int(r.clip_runs[b, c]), int(r.flat[b, c]), int(r.flat_runs[b, c]), int(r.nonfinite[b, c])])
            with open(base + SUFFIX_LTSA, "w", newline="") as f:
                out = csv.writer(f, lineterminator="\n")
                out.writerow(["bin_start", "frames", "bad_frames"] + self.band_names())
                db = r.band_db
                for b in range(r.bin_start.shape[0]):
                    out.writerow([repr(float(r.bin_start[b])), int(r.frames[b]), int(r.bad_frames[b])] + [f"{v:.2f}" for v in db[b]])

    def _band_span(self, lo: float, hi: float) -> slice:
        a, b = np.flatnonzero(self.band_hz == float(lo)), np.flatnonzero(self.band_hz == float(hi))
        if not a.size or not b.size or b[0] <= a[0]:
            raise ValueError(f"a band rule's range {lo}..{hi} Hz must run between two of the meter's band edges {self.band_hz.tolist()}")
        return slice(int(a[0]), int(b[0]))

    def flags(self, clip_fraction: float = 1e-3, flat_fraction: float = 0.5, silent_dbfs: float = -80.0,
              band_rules: Optional[Dict[str, tuple]] = None) -> Dict[str, List[Tuple[float, bool, Tuple[str, ...]]]]:
        """Per recording and bin (bin_start, usable, reasons).  Reasons: ``clipped`` - on some channel more than ``clip_fraction``
        of the samples lie in clipped runs; ``flat`` - on some channel more than ``flat_fraction`` lie in stuck runs; ``silent`` -
        every channel's RMS is below ``silent_dbfs``; ``nonfinite`` - a sample was no number; and per entry
        ``name: ((a_lo, a_hi), (b_lo, b_hi), db)`` of ``band_rules`` (ranges between the meter's band edges) ``name`` where the
        power in A exceeds that in B by more than ``db`` dB, e.g. ``{"wind": ((0, 125), (250, 2000), 20.0)}``.  No band rule
        is on by default.  The three numeric defaults (0.001, 0.5, -80 dB) are placeholders that were NOT tuned on field data:
        set them from recordings of your own recorders.  A bin is usable when it has no reason."""
        rules = {str(k): (self._band_span(*v[0]), self._band_span(*v[1]), float(v[2])) for k, v in (band_rules or {}).items()}
        out = {}
        for ident, r in self.recordings.items():
            n = np.maximum(r.samples, 1).astype(np.float64)
            rows = []
            for b in range(r.bin_start.shape[0]):
                why = []
                if (r.clipped[b] / n[b] > clip_fraction).any():
                    why.append("clipped")
                if (r.flat[b] / n[b] > flat_fraction).any():
                    why.append("flat")
                if (r.rms_dbfs[b] < silent_dbfs).all():
                    why.append("silent")
                if r.nonfinite[b].any() or r.bad_frames[b]:
                    why.append("nonfinite")
                for name, (sa, sb, db) in rules.items():
                    with np.errstate(divide="ignore", invalid="ignore"):
                        over = _db(r.band_power[b, sa].sum() / r.band_power[b, sb].sum())
                    if over > db:
                        why.append(name)
                rows.append((float(r.bin_start[b]), not why, tuple(why)))
            out[ident] = rows
        return out


# ---------------------------------------------------------------------------------------------------- folders
def health_recordings(dir_audio: str, *, bin_s: float = 60.0, clip_level: Optional[float] = None, clip_run: int = 3, flat_s: float = 0.02,
                      bands: Sequence[float] = DEFAULT_BANDS, engine=None, chunklength: float = 200,
                      embeddername: str = "yamnet_k2") -> HealthResult:
    """The health of every recording under ``dir_audio`` that ``analyze`` would take, read in ``analyze``'s chunks
    (``dataset._read_chunks``): every chunk's native samples go through ``HealthMeter.levels`` while they lie on the device, its
    16 kHz mono form - what the embedder gets - through ``HealthMeter.spectrum``; one read-back per chunk and kernel.  Runs are
    not carried from chunk to chunk: one that crosses a chunk end counts as two.  No classifier is needed.  An embedding
    store holds no audio and is refused."""
    from .dataset import _open_engine
    if _store_of(dir_audio) is not None:
        raise ValueError("health_recordings needs the recordings themselves: an embedding store holds no audio")
    chunklength = framing.round_chunklength(chunklength, FRAMELENGTH_S, DIGITS_TIME)
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        meter = HealthMeter(bin_s, clip_level, clip_run, flat_s, bands, device=engine.device)
        result = HealthResult(meter.band_hz, bin_s=meter.bin_s)
        for path, ident in _recordings(dir_audio, {}, False, messages):
            level_parts: List[LevelBins] = []
            rates: List[int] = []

            def on_raw(raw, rate, first_frame):
                rates.append(int(rate))
                level_parts.append(meter.levels(raw.contiguous(), rate, first_frame))

            chunks = _read_chunks(engine, path, ident, 0, chunklength, messages, on_raw=on_raw)
            if not chunks:
                continue
            spectra = [meter.spectrum(c.pcm, c.start_s) for c in chunks]
            result.recordings[ident] = recording_health(merge_levels(level_parts), merge_spectrum(spectra, meter.n_bands), rates[0],
                                                        meter.bin_ticks)
        result.messages = messages
        return result
    finally:
        if own:
            engine.close()
