"""Training sets from annotated recordings: the first link of ``embed -> fit_head -> save_model -> analyze``.

    read_annotations   a CSV of ``ident,start,end,label`` -> {ident: [(start, end, label), ...]}
    label_windows      intervals -> per-window targets and a keep mask (pure NumPy)
    embed_annotated    a folder of recordings + annotations -> TrainingSet (embeddings on the device, targets, groups)
    augment            annotated events overlaid on background stretches at chosen SNRs (``bd_mix``, csrc/mixaug.hip) and embedded
    concat, save, load

The recordings are found, opened, chunked, brought to 16 kHz mono and embedded as ``analyze`` does it (``analyze.search_audio``,
``flacio.open_track``, ``framing``'s chunk arithmetic, ``engine.resample``, one ``engine.launch`` per set of chunks), so row k of a
recording's embeddings is the window whose ``start`` ``analyze`` writes in row k of its result file.  ``groups`` names the
recording of every row: windows of one recording are near-duplicates and belong into one fold
(``train.cross_validate_head(groups=...)``), and a mixture stays with the recording its event came from.

    from buzzdetect_amd import dataset, train
    from buzzdetect_amd.analyze import analyze

    classes = ["ambient", "ins_buzz"]
    notes = dataset.read_annotations("annotations.csv")
    real = dataset.embed_annotated("audio_in", notes, classes, background="ambient")
    mixed = dataset.augment("audio_in", notes, classes, background="ambient", snr_db=(0, 5, 10, 20), per_event=4)
    both = dataset.concat(real, mixed)
    fit = train.fit_head(both.embeddings, both.labels(), classes, class_weight="balanced")
    train.save_model("models/model_field", fit)
    analyze("model_field", dir_audio="audio_in", dir_out="out")
"""
from __future__ import annotations

import csv
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, framing

FRAMELENGTH_S = 0.96
WINDOW_SAMPLES = 15360            # a 0.96 s window at 16 kHz: the hop of the mixtures (framehop_prop 1)
DIGITS_TIME = 2
EDGE_S = 1e-9                     # overlaps below a nanosecond are none: 3 * 0.96 and the literal 2.88 differ in the last bit
MIX_CLIPS_PER_CALL = 64           # one bd_mix call feeds one engine.launch (bd_predict_chunks takes 64 chunks)
COLUMNS = ("ident", "start", "end", "label")

Annotations = Dict[str, List[Tuple[float, float, str]]]

# bd_mix_clip (include/buzzdetect_mix.h) as a NumPy record: 40 bytes, the C layout
MIX_CLIP = np.dtype([("ev_off", "<i8"), ("nz_off", "<i8"), ("out_off", "<i8"), ("n", "<i4"), ("ev_gain", "<f4"), ("ratio", "<f4")],
                    align=True)
assert MIX_CLIP.itemsize == C.sizeof(_lib.bd_mix_clip)

# one row per mixture (draw_plan): which event clip, which stretch of background, where in the audio, at what SNR and gain
PLAN = np.dtype([("event", "<i4"), ("stretch", "<i4"), ("group", "<i4"), ("ev_off", "<i8"), ("nz_off", "<i8"), ("n", "<i4"),
                 ("snr_db", "<f8"), ("gain_db", "<f8"), ("dropped", "?")])


@dataclass
class TrainingSet:
    """``embeddings``: device float32 [N, 1024]; ``targets``: float32 [N, C]; ``groups``: int32 [N], the index into ``idents``;
    ``starts``: float64 [N], the ``start`` ``analyze`` writes for the row's window; ``plan``: the mixtures of ``augment``
    (``PLAN`` records), else None; ``messages``: what was skipped or dropped, and why."""
    embeddings: object
    targets: np.ndarray
    groups: np.ndarray
    idents: List[str]
    starts: np.ndarray
    classes: List[str]
    plan: Optional[np.ndarray] = None
    messages: List[str] = field(default_factory=list)

    def __len__(self) -> int:
        return int(self.targets.shape[0])

    def labels(self) -> np.ndarray:
        """int32 [N]: the one class of every row, for ``loss="categorical"`` (and ``class_weight``).  ``ValueError`` when a row
        has no class or several (no ``background`` named, or intervals of two classes in one window): such sets are for
        ``loss="binary"`` on ``targets``."""
        if len(self) and not (self.targets.sum(axis=1) == 1).all():
            raise ValueError("rows with no class or several: use targets with loss=\"binary\"")
        return self.targets.argmax(axis=1).astype(np.int32) if len(self) else np.zeros(0, np.int32)


# ---------------------------------------------------------------------------------------------------- annotations
def read_annotations(path: str) -> Annotations:
    """A CSV with the columns ``ident,start,end,label`` (any order, a header line first) as {ident: [(start, end, label)]}.
    ``ident`` is a recording's path below the audio folder without its extension (``analyze.build_ident``); ``start`` and
    ``end`` are seconds from the start of the recording.  Another set of columns, a number that does not parse, a negative
    start or ``end <= start`` raise ``ValueError`` naming the line."""
    out: Annotations = {}
    with open(path, newline="") as f:
        reader = csv.reader(f)
        header = next(reader, None)
        names = [h.strip() for h in header] if header is not None else []
        if sorted(names) != sorted(COLUMNS):
            raise ValueError(f"{path}: line 1: the columns must be {','.join(COLUMNS)}, found {','.join(names) or 'nothing'}")
        at = {name: names.index(name) for name in COLUMNS}
        for row in reader:
            line = reader.line_num
            if not row or all(not cell.strip() for cell in row):
                continue
            if len(row) != len(COLUMNS):
                raise ValueError(f"{path}: line {line}: {len(row)} fields, expected {len(COLUMNS)}")
            ident, label = row[at["ident"]].strip(), row[at["label"]].strip()
            try:
                start, end = float(row[at["start"]]), float(row[at["end"]])
            except ValueError:
                raise ValueError(f"{path}: line {line}: start and end must be numbers") from None
            if not ident or not label:
                raise ValueError(f"{path}: line {line}: empty ident or label")
            if not (np.isfinite(start) and np.isfinite(end)) or start < 0:
                raise ValueError(f"{path}: line {line}: start and end must be finite and start >= 0")
            if end <= start:
                raise ValueError(f"{path}: line {line}: end {end} is not after start {start}")
            out.setdefault(ident, []).append((start, end, label))
    return out


def _merged(intervals: Iterable[Tuple[float, float]]) -> List[Tuple[float, float]]:
    """The union of the intervals as disjoint pieces in ascending order (touching intervals become one piece)."""
    out: List[List[float]] = []
    for a, b in sorted(intervals):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def _label_at(win_start: np.ndarray, intervals, classes: Sequence[str], min_overlap: float, background: Optional[str]):
    """``label_windows`` for windows that start at the given seconds; also returns which windows meet an interval."""
    classes = list(classes)
    if background is not None and background not in classes:
        raise ValueError(f"background {background!r} is not one of the classes")
    if not 0.0 < min_overlap <= 1.0:
        raise ValueError("min_overlap must be in (0, 1]")
    win_start = np.asarray(win_start, dtype=np.float64)
    n = win_start.size
    win_end = win_start + FRAMELENGTH_S
    targets = np.zeros((n, len(classes)), np.float32)
    touched = np.zeros(n, bool)
    by_class: Dict[str, list] = {}
    for a, b, label in intervals:
        if label not in classes:
            raise ValueError(f"label {label!r} is not one of the classes {classes}")
        if not b > a:
            raise ValueError(f"interval ({a}, {b}) of {label!r} is empty")
        by_class.setdefault(label, []).append((float(a), float(b)))
    for label, spans in by_class.items():
        c = classes.index(label)
        for a, b in _merged(spans):
            overlap = np.minimum(win_end, b) - np.maximum(win_start, a)
            met = overlap > EDGE_S
            touched |= met
            need = min_overlap * min(FRAMELENGTH_S, b - a)
            targets[met & (overlap >= need - EDGE_S), c] = 1.0
    labelled = targets.any(axis=1)
    keep = labelled | ~touched
    if background is not None:
        targets[~touched, classes.index(background)] = 1.0
    return targets, keep, touched


def label_windows(n_windows: int, framehop_s: float, intervals, classes: Sequence[str], *, min_overlap: float = 0.5,
                  background: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(targets float32 [n, C], keep bool [n]) for windows k = 0 .. n-1 covering [k hop, k hop + 0.96) seconds.

    ``intervals``: (start, end, label) in seconds, labels from ``classes``.  The intervals of one class are merged into
    disjoint pieces first.  Class c is set in a window when the window's overlap with one of c's pieces is at least
    ``min_overlap`` x min(0.96, the piece's length).  A window that meets some piece but gets no class is ambiguous:
    ``keep`` is False and its row is all zero.  A window that meets no piece gets the ``background`` class when one is
    named, else keeps an all-zero row (the ``multilabel`` loss's "nothing here"); both are kept.

    Boundaries.  Windows are half-open and an overlap below one nanosecond counts as none, so an interval that ends exactly
    on a window's left edge does not meet that window (it is background there), and one that starts exactly on a window's
    right edge does not meet it either.  An interval shorter than a window that lies wholly inside one overlaps it by its own
    length, which is min(0.96, length): the class is set for every ``min_overlap``.  Where such a short interval straddles two
    windows, each half is measured against ``min_overlap`` x its length: with 0.5 an even split sets both windows."""
    starts = np.arange(int(n_windows), dtype=np.float64) * float(framehop_s)
    targets, keep, _ = _label_at(starts, intervals, classes, min_overlap, background)
    return targets, keep


# ---------------------------------------------------------------------------------------------------- reading as analyze reads
@dataclass
class _Chunk:
    group: int
    start_s: float                 # the chunk's left edge, as analyze passes it to the result rows
    pcm: object                    # device float32 [n16]: the chunk at 16 kHz mono


def _as_annotations(annotations) -> Annotations:
    if isinstance(annotations, (str, os.PathLike)):
        return read_annotations(os.fspath(annotations))
    return {k: [(float(a), float(b), str(l)) for a, b, l in v] for k, v in dict(annotations).items()}


def _recordings(dir_audio: str, annotations: Annotations, only_annotated: bool, messages: List[str]):
    """(path, ident) of every recording ``analyze`` would take, by its rules (extensions, conflicting names, minimum size)."""
    from .analyze import build_ident, search_audio
    from .pipeline import FILE_SIZE_MINIMUM
    paths = search_audio(dir_audio)
    idents = [build_ident(p, dir_audio) for p in paths]
    out = []
    for p, i in zip(paths, idents):
        if idents.count(i) > 1:
            messages.append(f"conflicting names, skipped: {i}")
        elif os.path.getsize(p) < FILE_SIZE_MINIMUM:
            messages.append(f"below minimum analyzeable size, skipped: {i}")
        elif only_annotated and i not in annotations:
            continue
        else:
            out.append((p, i))
    for i in sorted(set(annotations) - set(idents)):
        messages.append(f"annotated, but no such recording: {i}")
    return out


def _read_chunks(engine, path: str, ident: str, group: int, chunklength: float, messages: List[str], on_raw=None) -> List[_Chunk]:
    """One recording as the feeder and the analyzers bring it to the CNN: analyze's chunks, each at 16 kHz mono on the device.
    ``on_raw(raw, rate, first_frame)``, if given, sees every chunk's native samples on the device before they are resampled."""
    from .flacio import open_track
    from .wavio import WavFormatError
    try:
        track = open_track(path)
    except (WavFormatError, OSError) as exc:
        messages.append(f"unreadable, skipped: {ident} ({exc})")
        return []
    try:
        rate = track.samplerate
        if rate != 16000 and _lib.load().bd_anyrate_supported(int(rate), 16000, int(engine.resample_quality)) != 1:
            messages.append(f"sample rate {rate} Hz not supported, skipped: {ident}")
            return []
        out = []
        for chunk in framing.gaps_to_chunklist([(0, track.duration)], chunklength):
            a, b = framing.chunk_sample_range(chunk, rate)
            want = min(b, track.frames_declared) - a
            if want <= 0:
                continue
            raw = engine.read_audio(track, a, want, raw=True)
            got = int(raw.shape[0])
            if got == 0:
                break
            if on_raw is not None:
                on_raw(raw, rate, a)
            if raw.dtype != _torch().float32 or rate != 16000 or track.channels > 1:
                pcm = engine.resample(raw, rate, 16000)          # also int16 -> float32 and the channel mean
            else:
                pcm = raw[:, 0].contiguous()
            out.append(_Chunk(group, float(chunk[0]), pcm))
            if got < want:
                messages.append(f"unreadable audio, stopped at {round((a + got) / rate, 1)}s: {ident}")
                break
        return out
    finally:
        track.close()


def _torch():
    import torch
    return torch


def _store_of(dir_audio):
    """The embedding store ``dir_audio`` is (a ``store.Store``, or a folder that holds one), else None: audio."""
    from . import store
    return store.as_store(dir_audio)


def _sources(dir_audio, engine, framehop_prop: float, chunklength: float, annotations: Annotations, only_annotated: bool,
             messages: List[str]):
    """(ident, chunks) of every recording the tools walk, in order: from audio (``_recordings``, ``_read_chunks``; ``chunklength``
    already rounded), or from an embedding store, whose chunks' ``pcm`` are handles on stored rows (``store.StoredPart``) and
    whose parameters must be the caller's."""
    st = _store_of(dir_audio)
    if st is not None:
        yield from st.walk(engine, framehop_prop, chunklength, annotations, only_annotated, messages)
        return
    group = 0
    for path, ident in _recordings(dir_audio, annotations, only_annotated, messages):
        chunks = _read_chunks(engine, path, ident, group, chunklength, messages)
        if chunks:
            group += 1
            yield ident, chunks


def _stored(parts) -> bool:
    return bool(parts) and hasattr(parts[0], "stored_rows")


def _part_windows(engine, part, hop: int, step: int) -> int:
    """Windows of one part: a chunk of audio at 16 kHz, or a handle on stored rows."""
    if hasattr(part, "stored_rows"):
        return int(part.windows)
    return int(engine.num_windows(int(part.numel()), hop, step))


def _embed_parts(engine, parts, hop: int, step: int):
    """One launch set's embeddings, final: the set's range verdict is waited for, and a flagged set is computed again with
    exact-f32 products, as ``engine.embed`` does for its one chunk.  Returns (rows, windows per part).  Parts of an embedding
    store are read and decoded instead (``store.stored_rows``): no embedder launch."""
    if _stored(parts):
        from .store import stored_rows
        return stored_rows(engine, parts)
    from .engine import LaunchVerdict
    f16 = engine._mode != "f32"
    verdict = LaunchVerdict(engine._stream()) if f16 else None
    emb, _, counts = engine.launch(parts, hop, step, want_embeddings=True, want_logits=False, verdict=verdict)
    if verdict is not None and verdict.wait():
        emb, _, counts = engine.launch(parts, hop, step, want_embeddings=True, want_logits=False, mode="f32")
        engine.overflow_reruns += 1
    return emb, counts


def _launch_sets(parts, windows, max_windows: int = 4096):
    """Consecutive parts gathered into launch sets of at most 64 chunks and about ``max_windows`` windows."""
    at = 0
    while at < len(parts):
        end, total = at, 0
        while end < len(parts) and end - at < 64 and (end == at or total + windows[end] <= max_windows):
            total += windows[end]
            end += 1
        yield at, end
        at = end


def _open_engine(engine, embeddername: str):
    if engine is not None:
        return engine, False
    from .engine import HipEngine
    return HipEngine(embeddername=embeddername, modelname=None), True


def embed_annotated(dir_audio: str, annotations, classes: Sequence[str], *, engine=None, framehop_prop: float = 1.0,
                    chunklength: float = 200, min_overlap: float = 0.5, background: Optional[str] = None,
                    embeddername: str = "yamnet_k2", only_annotated: bool = False) -> TrainingSet:
    """Every recording under ``dir_audio`` that ``analyze`` would analyse, embedded window by window and labelled from
    ``annotations`` (a path for ``read_annotations`` or what it returns).  Same chunks, same resampling, same windows as
    ``analyze(framehop_prop=..., chunklength=...)``: ``starts`` is that run's ``start`` column.  A recording without
    annotation rows is all background (``only_annotated=True`` leaves such recordings out).  Ambiguous windows
    (``label_windows``) are left out.  ``engine``: a ``HipEngine`` to use; else one is built for ``embeddername`` and closed.
    ``dir_audio`` may be an embedding store (``store.embed_recordings``: its folder, or a ``store.Store``) made with the same
    ``framehop_prop`` and ``chunklength``: the rows are then read, not computed, and the set is the same."""
    from .engine import hop_samples, patch_step
    torch = _torch()
    classes = list(classes)
    notes = _as_annotations(annotations)
    framehop_s = FRAMELENGTH_S * framehop_prop
    hop, step = hop_samples(framehop_s), patch_step(framehop_s)
    chunklength = framing.round_chunklength(chunklength, FRAMELENGTH_S, DIGITS_TIME)
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        idents, emb_rows, tgt_rows, grp_rows, start_rows = [], [], [], [], []
        for ident, chunks in _sources(dir_audio, engine, framehop_prop, chunklength, notes, only_annotated, messages):
            idents.append(ident)
            parts = [c.pcm for c in chunks]
            windows = [_part_windows(engine, p, hop, step) for p in parts]
            for a, b in _launch_sets(parts, windows):
                emb, counts = _embed_parts(engine, parts[a:b], hop, step)
                at = 0
                for c, n in zip(chunks[a:b], counts):
                    exact = c.start_s + np.arange(n, dtype=np.float64) * framehop_s
                    targets, keep, _ = _label_at(exact, notes.get(ident, ()), classes, min_overlap, background)
                    rows = torch.from_numpy(np.nonzero(keep)[0]).to(emb.device)
                    emb_rows.append(emb[at:at + n].index_select(0, rows))
                    tgt_rows.append(targets[keep])
                    grp_rows.append(np.full(int(keep.sum()), c.group, np.int32))
                    start_rows.append(framing.window_starts(n, c.start_s, framehop_s, DIGITS_TIME)[keep])
                    at += n
        return _assemble(engine, emb_rows, tgt_rows, grp_rows, start_rows, idents, classes, None, messages)
    finally:
        if own:
            engine.close()


def _assemble(engine, emb_rows, tgt_rows, grp_rows, start_rows, idents, classes, plan, messages) -> TrainingSet:
    torch = _torch()
    if emb_rows:
        emb = torch.cat(emb_rows).contiguous()
    else:
        emb = torch.empty((0, _lib.EMBEDDING_SIZE), dtype=torch.float32, device=engine.device)
    targets = np.concatenate(tgt_rows) if tgt_rows else np.zeros((0, len(classes)), np.float32)
    groups = np.concatenate(grp_rows) if grp_rows else np.zeros(0, np.int32)
    starts = np.concatenate(start_rows) if start_rows else np.zeros(0, np.float64)
    return TrainingSet(emb, targets.astype(np.float32), groups.astype(np.int32), list(idents), starts.astype(np.float64),
                       list(classes), plan, messages)


# ---------------------------------------------------------------------------------------------------- the mixer
def mix_descriptors(ev_off, nz_off, n, snr_db, gain_db) -> np.ndarray:
    """``MIX_CLIP`` records for one ``bd_mix`` call, outputs packed back to back: ``ratio = 10^(-snr_db / 20)`` and
    ``ev_gain = 10^(gain_db / 20)`` in double, then float32."""
    n = np.asarray(n, dtype=np.int64)
    clips = np.zeros(n.size, MIX_CLIP)
    clips["ev_off"], clips["nz_off"], clips["n"] = ev_off, nz_off, n
    clips["out_off"] = np.cumsum(n) - n
    clips["ratio"] = (10.0 ** (-np.asarray(snr_db, dtype=np.float64) / 20.0)).astype(np.float32)
    clips["ev_gain"] = (10.0 ** (np.asarray(gain_db, dtype=np.float64) / 20.0)).astype(np.float32)
    return clips


def _clip_pointer(clips: np.ndarray):
    if clips.dtype != MIX_CLIP or not clips.flags.c_contiguous:
        raise ValueError("clips must be a contiguous array of dataset.MIX_CLIP records")
    return C.cast(clips.ctypes.data, C.POINTER(_lib.bd_mix_clip)) if clips.size else None


def mix_host(ev: np.ndarray, nz: np.ndarray, clips: np.ndarray, out: Optional[np.ndarray] = None):
    """``bd_mix_host``: (out float32, power float32 [n, 2] of (Pe, Pn), flags uint32 [n]) on host arrays."""
    lib = _lib.load()
    ev, nz = np.ascontiguousarray(ev, np.float32), np.ascontiguousarray(nz, np.float32)
    if out is None:
        out = np.zeros(int((clips["out_off"] + clips["n"]).max()) if clips.size else 0, np.float32)
    power, flags = np.zeros((clips.size, 2), np.float32), np.zeros(clips.size, np.uint32)
    _lib.check(lib.bd_mix_host(ev.ctypes.data, ev.size, nz.ctypes.data, nz.size, _clip_pointer(clips), clips.size, out.ctypes.data,
                               out.size, power.ctypes.data, flags.ctypes.data))
    return out, power, flags


def mix_device(ev, nz, clips: np.ndarray, out=None, workspace=None):
    """``bd_mix`` on the current stream: ``ev`` and ``nz`` are one-dimensional float32 device tensors (they may be the same),
    ``out`` a float32 device tensor that holds every clip's output range (default: just large enough).  Returns
    (out, power float32 [n, 2], flags int32 [n]) on the device; nothing is waited for."""
    torch = _torch()
    lib = _lib.load()
    for t in (ev, nz) + ((out,) if out is not None else ()):
        if t.dim() != 1 or t.dtype != torch.float32 or not t.is_contiguous() or t.device != ev.device or not t.is_cuda:
            raise ValueError("mix_device takes one-dimensional contiguous float32 tensors on one device")
    if out is None:
        out = torch.empty(int((clips["out_off"] + clips["n"]).max()) if clips.size else 0, dtype=torch.float32, device=ev.device)
    power = torch.zeros((clips.size, 2), dtype=torch.float32, device=ev.device)
    flags = torch.zeros(clips.size, dtype=torch.int32, device=ev.device)
    need = _lib.check(lib.bd_mix_workspace_bytes(_clip_pointer(clips), clips.size))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=ev.device)
    with torch.cuda.device(ev.device):
        stream = torch.cuda.current_stream(ev.device)
        _lib.check(lib.bd_mix(ev.data_ptr(), ev.numel(), nz.data_ptr(), nz.numel(), _clip_pointer(clips), clips.size,
                              out.data_ptr(), out.numel(), power.data_ptr(), flags.data_ptr(), workspace.data_ptr(),
                              workspace.numel(), stream.cuda_stream))
    for t in (ev, nz, out, workspace):
        t.record_stream(stream)
    return out, power, flags


# ---------------------------------------------------------------------------------------------------- augment
@dataclass
class EventClip:
    """A run of labelled windows of one chunk: ``offset`` samples into the audio buffer, ``windows`` whole windows long."""
    group: int
    offset: int
    windows: int
    targets: np.ndarray            # float32 [windows, C]
    starts: np.ndarray             # float64 [windows]: analyze's start column for these windows


@dataclass
class Stretch:
    """A maximal run of windows of one chunk that meet no annotation."""
    group: int
    offset: int
    windows: int
    start_s: float


def find_clips(chunks, annotations_of_group, classes: Sequence[str], *, background: str, min_overlap: float = 0.5,
               max_clip_s: float = 9.6) -> Tuple[List[EventClip], List[Stretch]]:
    """Event clips and background stretches of recordings laid out in one audio buffer.  ``chunks``: (group, chunk start in
    seconds, samples at 16 kHz, offset of the chunk in the buffer), one per chunk; ``annotations_of_group``: group -> intervals.
    Only whole windows count (a chunk's ragged last window is neither event nor background).  An event clip is a maximal run
    of consecutive windows that carry a class other than ``background``, cut into pieces of at most ``max_clip_s``; ambiguous
    windows end a run and belong to nothing.  Needs no device."""
    classes = list(classes)
    if background not in classes:
        raise ValueError(f"background {background!r} is not one of the classes")
    max_w = int(np.floor(max_clip_s / FRAMELENGTH_S + 1e-9))
    if max_w < 1:
        raise ValueError("max_clip_s must be at least one window (0.96 s)")
    bg = classes.index(background)
    events: List[EventClip] = []
    stretches: List[Stretch] = []
    for group, start_s, n16, offset in chunks:
        whole = int(n16) // WINDOW_SAMPLES
        if whole == 0:
            continue
        exact = start_s + np.arange(whole, dtype=np.float64) * FRAMELENGTH_S
        targets, keep, touched = _label_at(exact, annotations_of_group.get(group, ()), classes, min_overlap, background)
        shown = framing.window_starts(whole, start_s, FRAMELENGTH_S, DIGITS_TIME)
        is_event = keep & (np.delete(targets, bg, axis=1).any(axis=1))
        is_quiet = ~touched
        for mask, is_ev in ((is_event, True), (is_quiet, False)):
            edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
            for a, b in zip(edges[::2], edges[1::2]):
                if not is_ev:
                    stretches.append(Stretch(group, int(offset) + int(a) * WINDOW_SAMPLES, int(b - a), float(exact[a])))
                    continue
                for k in range(int(a), int(b), max_w):
                    e = min(k + max_w, int(b))
                    events.append(EventClip(group, int(offset) + k * WINDOW_SAMPLES, e - k, targets[k:e].copy(), shown[k:e].copy()))
    return events, stretches


def draw_plan(events: Sequence[EventClip], stretches: Sequence[Stretch], *, snr_db=(0, 5, 10, 20), per_event: int = 4,
              gain_db=(0.0,), seed: int = 0, idents: Optional[Sequence[str]] = None) -> np.ndarray:
    """``per_event`` mixtures per event clip, drawn from ``np.random.default_rng(seed)`` in a fixed order (per clip and
    repetition: the stretch among those at least as long as the clip, the offset into it in samples, the SNR, the gain).
    Returns ``PLAN`` records; the same arguments give the same plan.  ``ValueError`` names the clip no stretch is long
    enough for.  Needs no device."""
    snr_db, gain_db = [float(v) for v in snr_db], [float(v) for v in gain_db]
    if not snr_db or not gain_db or per_event < 1:
        raise ValueError("snr_db and gain_db need a value each and per_event must be at least 1")
    rng = np.random.default_rng(seed)
    plan = np.zeros(len(events) * per_event, PLAN)
    for e, ev in enumerate(events):
        fits = [s for s, st in enumerate(stretches) if st.windows >= ev.windows]
        if not fits:
            name = idents[ev.group] if idents is not None else f"recording {ev.group}"
            raise ValueError(f"no background stretch of {ev.windows} windows ({ev.windows * FRAMELENGTH_S:.2f} s) for the clip at "
                             f"{ev.starts[0]:.2f} s of {name}; lower max_clip_s or add background audio")
        n = ev.windows * WINDOW_SAMPLES
        for r in range(per_event):
            s = fits[int(rng.integers(len(fits)))]
            room = stretches[s].windows * WINDOW_SAMPLES - n
            shift = int(rng.integers(room + 1))
            row = plan[e * per_event + r]
            row["event"], row["stretch"], row["group"] = e, s, ev.group
            row["ev_off"], row["nz_off"], row["n"] = ev.offset, stretches[s].offset + shift, n
            row["snr_db"] = snr_db[int(rng.integers(len(snr_db)))]
            row["gain_db"] = gain_db[int(rng.integers(len(gain_db)))]
    return plan


def augment(dir_audio: str, annotations, classes: Sequence[str], *, snr_db=(0, 5, 10, 20), per_event: int = 4, gain_db=(0.0,),
            background: str, max_clip_s: float = 9.6, seed: int = 0, engine=None, chunklength: float = 200,
            min_overlap: float = 0.5, embeddername: str = "yamnet_k2", only_annotated: bool = False) -> TrainingSet:
    """Mixtures of the annotated events with background from the same folder, embedded.

    The recordings are read as ``embed_annotated`` reads them (hop 0.96 s) and kept on the device.  ``find_clips`` cuts event
    clips of whole windows (at most ``max_clip_s``) and background stretches, ``draw_plan`` draws ``per_event`` mixtures per
    clip from ``seed``, ``bd_mix`` mixes up to 64 of them per call at the drawn SNR (``snr_db``; ``inf`` is the event alone)
    and gain, and the 64 mixtures are the 64 parts of one ``engine.launch``: each keeps its own end-of-chunk padding, so its
    rows are those of ``engine.embed(mixture)``.  Targets and ``starts`` are the event clip's windows'; ``groups`` is the
    event's recording.  A mixture whose background came out silent (``bd_mix``'s flag) is dropped, marked in ``plan`` and
    counted in ``messages``.  The same folder, annotations and seed give the same bits.  Mixing needs the audio: an embedding
    store in place of ``dir_audio`` is refused (``ValueError``)."""
    from .engine import hop_samples, patch_step
    if _store_of(dir_audio) is not None:
        raise ValueError("augment mixes audio and needs the recordings themselves: an embedding store holds none")
    torch = _torch()
    classes = list(classes)
    notes = _as_annotations(annotations)
    hop, step = hop_samples(FRAMELENGTH_S), patch_step(FRAMELENGTH_S)
    chunklength = framing.round_chunklength(chunklength, FRAMELENGTH_S, DIGITS_TIME)
    messages: List[str] = []
    engine, own = _open_engine(engine, embeddername)
    try:
        idents, layout, pieces, at = [], [], [], 0
        for path, ident in _recordings(dir_audio, notes, only_annotated, messages):
            chunks = _read_chunks(engine, path, ident, len(idents), chunklength, messages)
            if not chunks:
                continue
            idents.append(ident)
            for c in chunks:
                layout.append((c.group, c.start_s, int(c.pcm.numel()), at))
                pieces.append(c.pcm)
                at += int(c.pcm.numel())
        by_group = {g: notes.get(i, ()) for g, i in enumerate(idents)}
        events, stretches = find_clips(layout, by_group, classes, background=background, min_overlap=min_overlap,
                                       max_clip_s=max_clip_s)
        plan = draw_plan(events, stretches, snr_db=snr_db, per_event=per_event, gain_db=gain_db, seed=seed, idents=idents)
        audio = torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.float32, device=engine.device)
        emb_rows, tgt_rows, grp_rows, start_rows = [], [], [], []
        workspace = None
        for a in range(0, plan.size, MIX_CLIPS_PER_CALL):
            rows = plan[a:a + MIX_CLIPS_PER_CALL]
            clips = mix_descriptors(rows["ev_off"], rows["nz_off"], rows["n"], rows["snr_db"], rows["gain_db"])
            need = _lib.check(_lib.load().bd_mix_workspace_bytes(_clip_pointer(clips), clips.size))
            if workspace is None or workspace.numel() < need:
                workspace = torch.empty(need, dtype=torch.uint8, device=engine.device)
            mixed, _, flags = mix_device(audio, audio, clips, workspace=workspace)
            parts = [mixed[int(c["out_off"]): int(c["out_off"]) + int(c["n"])] for c in clips]
            emb, counts = _embed_parts(engine, parts, hop, step)
            silent = (flags.cpu().numpy() & _lib.MIX_FLAG_SILENT_BACKGROUND) != 0
            row_at = 0
            for k, n in enumerate(counts):
                ev = events[int(rows["event"][k])]
                assert n == ev.windows
                if silent[k]:
                    plan["dropped"][a + k] = True
                else:
                    emb_rows.append(emb[row_at:row_at + n])
                    tgt_rows.append(ev.targets)
                    grp_rows.append(np.full(n, ev.group, np.int32))
                    start_rows.append(ev.starts)
                row_at += n
        dropped = int(plan["dropped"].sum())
        if dropped:
            messages.append(f"silent background, dropped: {dropped} of {plan.size} mixtures")
        return _assemble(engine, emb_rows, tgt_rows, grp_rows, start_rows, idents, classes, plan, messages)
    finally:
        if own:
            engine.close()


# ---------------------------------------------------------------------------------------------------- sets
def concat(*sets: TrainingSet) -> TrainingSet:
    """The rows of the sets in order.  The classes must agree; recordings of the same ident become one group, so a mixture
    stays in the fold of the recording it came from.  ``plan`` is not carried over."""
    torch = _torch()
    if not sets:
        raise ValueError("concat needs at least one set")
    classes = list(sets[0].classes)
    idents: List[str] = []
    groups = []
    for s in sets:
        if list(s.classes) != classes:
            raise ValueError(f"the sets' classes differ: {classes} and {list(s.classes)}")
        for i in s.idents:
            if i not in idents:
                idents.append(i)
        remap = np.array([idents.index(i) for i in s.idents], np.int32) if s.idents else np.zeros(0, np.int32)
        groups.append(remap[s.groups] if len(s) else np.zeros(0, np.int32))
    device = next((s.embeddings.device for s in sets if _is_tensor(s.embeddings)), None)
    emb = [s.embeddings if _is_tensor(s.embeddings) else torch.from_numpy(np.asarray(s.embeddings, np.float32)) for s in sets]
    emb = torch.cat([e.to(device) if device is not None else e for e in emb]).contiguous()
    return TrainingSet(emb, np.concatenate([s.targets for s in sets]).astype(np.float32),
                       np.concatenate(groups).astype(np.int32), idents,
                       np.concatenate([s.starts for s in sets]).astype(np.float64), classes, None,
                       [m for s in sets for m in s.messages])


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _strings(values) -> np.ndarray:
    values = list(values)
    return np.array(values, dtype=np.str_) if values else np.zeros(0, dtype="<U1")


def save(path: str, ts: TrainingSet) -> None:
    """One ``.npz`` (written to exactly ``path``) of plain arrays: nothing in it is a pickled object."""
    emb = ts.embeddings.detach().cpu().numpy() if _is_tensor(ts.embeddings) else np.asarray(ts.embeddings, np.float32)
    arrays = dict(embeddings=emb, targets=ts.targets, groups=ts.groups, starts=ts.starts, idents=_strings(ts.idents),
                  classes=_strings(ts.classes), messages=_strings(ts.messages))
    if ts.plan is not None:
        arrays["plan"] = np.asarray(ts.plan, PLAN)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def load(path: str, device=None) -> TrainingSet:
    """``save``'s set.  ``device``: a torch device for the embeddings (None: the current HIP device when there is one, else
    the host)."""
    torch = _torch()
    with np.load(path, allow_pickle=False) as z:
        emb = torch.from_numpy(np.ascontiguousarray(z["embeddings"], np.float32))
        if device is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if device is not None:
            emb = emb.to(device)
        return TrainingSet(emb, z["targets"].astype(np.float32), z["groups"].astype(np.int32), [str(i) for i in z["idents"]],
                           z["starts"].astype(np.float64), [str(c) for c in z["classes"]],
                           z["plan"].astype(PLAN) if "plan" in z.files else None, [str(m) for m in z["messages"]])
