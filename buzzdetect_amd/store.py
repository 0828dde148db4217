"""Embed recordings once: an on-disk store of window embeddings that every tool reads in place of the audio.

    embed_recordings   a folder of recordings -> one ``<ident>.bdemb`` per recording under ``dir_store`` (resumes)
    Store              a store's recordings and parameters; ``verify()`` on the host; the rows of a recording on the device
    score_store        a store through one model or several -> the result trees ``analyze`` writes, no CNN pass
    encode_host / decode_host / encode_device / decode_device      the record codec (include/buzzdetect_rows.h)

``search_recordings``, ``top_windows``, ``cluster_recordings``, ``assign_recordings``, ``call_recordings``,
``evaluate_recordings``, ``embed_annotated`` and ``queries_from_annotations`` take a store's folder (or a ``Store``) where they
take ``dir_audio``: their loop (``dataset._sources``) then hands out handles on stored rows, ``dataset._embed_parts`` returns
them decoded and ``search._logit_parts`` runs ``engine.score_rows`` on them.  A window's embedding is 4 KB (2 KB and 1 KB under
the lossy codecs); the same window is 31 - 92 KB of 16-bit audio, and reading it back costs no pass through the embedder.

    from buzzdetect_amd import store, search
    store.embed_recordings("audio_in", "emb", framehop_prop=1.0, chunklength=200)         # once per season
    store.score_store("emb", ["model_a", "model_b"], "out")                                # = analyze([...], dir_out="out")
    found = search.top_windows("emb", "model_a", k=200)

The file.  Little endian throughout:

    0      8 bytes  magic "BDEMBED" 0x01
    8      uint32   format version (1)
    12     uint32   n: bytes of the JSON header
    16     n bytes  the header (UTF-8 JSON, below), then zeros up to the next multiple of 4096
    R      windows x record bytes: the records (include/buzzdetect_rows.h: 4096, 2064 or 1040 bytes each)
    T      ceil(windows / 256) x (uint64 S1, uint64 S2): the checksums of the slices of 256 records
    T+..   uint64 total length of the file, 8 bytes "BDEMBEND"

The trailer repeats the length the header implies, so a file cut anywhere is recognised without reading a record.  A file is
written as ``<name>.part`` and renamed when whole; a ``.part`` is never read.  Header fields: ``ident``, ``embeddername``,
``weights_sha256`` (the embedder weights as loaded), ``mode`` (arithmetic of the 1x1 convolutions), ``resample_quality``,
``framehop_prop``, ``chunklength`` (rounded), ``codec``, ``windows``, ``source`` (path below the audio folder, size, mtime_ns,
rate, channels, duration), ``chunks`` ([start_s, windows] per chunk: what the tools' walk reports for the recording) and
``messages`` (what reading the recording said, e.g. "unreadable audio, stopped at ...").  ``store.json`` beside the files
marks the folder as a store and keeps what the embedding run said about recordings it did not store.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, framing
from .dataset import (DIGITS_TIME, FRAMELENGTH_S, _Chunk, _embed_parts, _launch_sets, _open_engine, _part_windows, _read_chunks,
                      _recordings, _torch)

MAGIC = b"BDEMBED\x01"
END_MAGIC = b"BDEMBEND"
FORMAT_VERSION = 1
SUFFIX = ".bdemb"
MANIFEST = "store.json"
ALIGN = 4096
PREFIX = struct.Struct("<8sII")
TRAILER = struct.Struct("<Q8s")
SLICE = _lib.ROWS_SLICE
DIM = _lib.EMBEDDING_SIZE
PARAMETERS = ("embeddername", "weights_sha256", "mode", "resample_quality", "framehop_prop", "chunklength", "codec")
MAX_HEADER = 1 << 26
STAGE_BYTES = 8 << 20


class StoreError(RuntimeError):
    """A store file that is cut, damaged or not one; the message names the file (and the slice, for a checksum)."""


# ---------------------------------------------------------------------------------------------------- the codec
def record_bytes(codec: str) -> int:
    return _lib.check(_lib.load().bd_rows_record_bytes(_codec(codec)))


def _codec(codec: str) -> int:
    if codec not in _lib.ROWS_CODECS:
        raise ValueError(f"codec must be one of {sorted(_lib.ROWS_CODECS)}, not {codec!r}")
    return _lib.ROWS_CODECS[codec]


def slices_of(windows: int) -> int:
    return (int(windows) + SLICE - 1) // SLICE


def encode_host(rows: np.ndarray, codec: str) -> Tuple[np.ndarray, np.ndarray, int]:
    """``bd_rows_encode_host``: float32 [W, 1024] -> (records uint8 [W, record bytes], sums uint64 [slices, 2], rows that are
    not representable)."""
    rows = np.ascontiguousarray(rows, np.float32)
    if rows.ndim != 2 or rows.shape[1] != DIM:
        raise ValueError(f"rows must be [W, {DIM}], not {list(rows.shape)}")
    w = rows.shape[0]
    records = np.zeros((w, record_bytes(codec)), np.uint8)
    sums, flags = np.zeros((slices_of(w), 2), np.uint64), np.zeros(1, np.uint32)
    _lib.check(_lib.load().bd_rows_encode_host(rows.ctypes.data, w, _codec(codec), records.ctypes.data, sums.ctypes.data,
                                               flags.ctypes.data))
    return records, sums, int(flags[0])


def decode_host(records: np.ndarray, codec: str) -> Tuple[np.ndarray, np.ndarray]:
    """``bd_rows_decode_host``: records uint8 [W, record bytes] -> (rows float32 [W, 1024], sums of the bytes read)."""
    records = np.ascontiguousarray(records, np.uint8)
    if records.ndim != 2 or records.shape[1] != record_bytes(codec):
        raise ValueError(f"records must be [W, {record_bytes(codec)}], not {list(records.shape)}")
    w = records.shape[0]
    rows, sums = np.zeros((w, DIM), np.float32), np.zeros((slices_of(w), 2), np.uint64)
    _lib.check(_lib.load().bd_rows_decode_host(records.ctypes.data, w, _codec(codec), rows.ctypes.data, sums.ctypes.data))
    return rows, sums


def _device_empty(shape, dtype, device):
    """Every device buffer the codec's kernels write comes from here (the tests put guard words around them)."""
    return _torch().empty(shape, dtype=dtype, device=device)


def _check_device(t, shape_tail, dtype, what: str):
    torch = _torch()
    if (not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != shape_tail or t.dtype != dtype or not t.is_cuda
            or not t.is_contiguous() or t.data_ptr() % 16):
        raise ValueError(f"{what} must be a contiguous, 16-byte aligned {dtype} [W, {shape_tail}] device tensor")


def encode_device(rows, codec: str):
    """``bd_rows_encode`` on the current stream of the rows' device: float32 [W, 1024] -> (records uint8 [W, record bytes], sums
    int64 [slices, 2] (uint64 bit patterns), flags int32 [1]), all on the device; nothing is waited for."""
    torch = _torch()
    _check_device(rows, DIM, torch.float32, "rows")
    w, rb = int(rows.shape[0]), record_bytes(codec)
    records = _device_empty((w, rb), torch.uint8, rows.device)
    sums = _device_empty((slices_of(w), 2), torch.int64, rows.device)
    flags = _device_empty((1,), torch.int32, rows.device)
    with torch.cuda.device(rows.device):
        stream = torch.cuda.current_stream(rows.device)
        _lib.check(_lib.load().bd_rows_encode(rows.data_ptr() if w else None, w, _codec(codec), records.data_ptr() if w else None,
                                              sums.data_ptr() if w else None, flags.data_ptr(), stream.cuda_stream))
    rows.record_stream(stream)
    return records, sums, flags


def decode_device(records, codec: str):
    """``bd_rows_decode`` on the current stream: records uint8 [W, record bytes] -> (rows float32 [W, 1024], sums int64
    [slices, 2] of the bytes read), on the device; nothing is waited for."""
    torch = _torch()
    _check_device(records, record_bytes(codec), torch.uint8, "records")
    w = int(records.shape[0])
    rows = _device_empty((w, DIM), torch.float32, records.device)
    sums = _device_empty((slices_of(w), 2), torch.int64, records.device)
    with torch.cuda.device(records.device):
        stream = torch.cuda.current_stream(records.device)
        _lib.check(_lib.load().bd_rows_decode(records.data_ptr() if w else None, w, _codec(codec), rows.data_ptr() if w else None,
                                              sums.data_ptr() if w else None, stream.cuda_stream))
    records.record_stream(stream)
    return rows, sums


# ---------------------------------------------------------------------------------------------------- the file
@dataclass
class Layout:
    records: int                  # offset of the first record
    table: int                    # offset of the checksum table
    total: int                    # length of the file
    record_bytes: int
    windows: int


def _layout(header_len: int, windows: int, codec: str) -> Layout:
    rb = record_bytes(codec)
    records = (PREFIX.size + header_len + ALIGN - 1) // ALIGN * ALIGN
    table = records + windows * rb
    return Layout(records, table, table + slices_of(windows) * 16 + TRAILER.size, rb, windows)


def make_header(*, ident: str, embeddername: str, weights_sha256: str, mode: str, resample_quality: int, framehop_prop: float,
                chunklength: float, codec: str, source: dict, chunks: Sequence[Tuple[float, int]],
                messages: Sequence[str] = ()) -> dict:
    _codec(codec)
    chunks = [[float(s), int(n)] for s, n in chunks]
    return {"format": FORMAT_VERSION, "ident": str(ident), "embeddername": str(embeddername), "weights_sha256": str(weights_sha256),
            "mode": str(mode), "resample_quality": int(resample_quality), "framehop_prop": float(framehop_prop),
            "chunklength": float(framing.round_chunklength(chunklength, FRAMELENGTH_S, DIGITS_TIME)), "codec": codec,
            "windows": sum(n for _, n in chunks), "source": dict(source), "chunks": chunks, "messages": [str(m) for m in messages]}


class _FileWriter:
    """One store file on its way: ``<path>.part`` until ``close`` has written the table and the trailer."""

    def __init__(self, path: str, header: dict):
        self.path, self.header = path, header
        text = json.dumps(header, sort_keys=True).encode()
        self.layout = _layout(len(text), int(header["windows"]), header["codec"])
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        self._f = open(path + ".part", "wb")            # (a stale .part of an interrupted run is overwritten)
        self._f.write(PREFIX.pack(MAGIC, FORMAT_VERSION, len(text)) + text)
        self._f.write(b"\0" * (self.layout.records - PREFIX.size - len(text)))
        self._sums: List[np.ndarray] = []
        self.written = 0

    def append(self, records: np.ndarray, sums: np.ndarray) -> None:
        """Whole slices (only the last call of a file may end inside one), with their sums in file order."""
        if self.written % SLICE:
            raise ValueError("records were appended behind a partial slice")
        self._f.write(np.ascontiguousarray(records, np.uint8).tobytes())
        self._sums.append(np.ascontiguousarray(sums).view(np.uint64).reshape(-1, 2))
        self.written += int(records.shape[0])

    def close(self) -> None:
        if self.written != self.layout.windows:
            self.abort()
            raise StoreError(f"{self.path}: {self.written} rows written, the header says {self.layout.windows}")
        table = np.concatenate(self._sums) if self._sums else np.zeros((0, 2), np.uint64)
        assert table.shape[0] == slices_of(self.written)
        self._f.write(table.astype("<u8").tobytes() + TRAILER.pack(self.layout.total, END_MAGIC))
        self._f.flush()
        os.fsync(self._f.fileno())
        assert self._f.tell() == self.layout.total
        self._f.close()
        os.replace(self.path + ".part", self.path)

    def abort(self) -> None:
        self._f.close()
        if os.path.exists(self.path + ".part"):
            os.remove(self.path + ".part")


def write_rows_host(path: str, rows: np.ndarray, header: dict) -> None:
    """One store file from host rows through the host codec (no device): ``header`` from ``make_header``, whose chunks' windows
    add up to the rows.  ``StoreError`` when a row is not representable; nothing is left behind then."""
    rows = np.ascontiguousarray(rows, np.float32)
    records, sums, bad = encode_host(rows, header["codec"])
    if bad:
        raise StoreError(f"{path}: {bad} rows are not representable (non-finite, or negative under codec b); not stored")
    w = _FileWriter(path, header)
    try:
        w.append(records, sums)
    except BaseException:
        w.abort()
        raise
    w.close()


class RecordingFile:
    """One ``<ident>.bdemb``: the header and the layout, checked against the file's length and trailer on opening (a cut file
    raises ``StoreError``); the records are read on demand."""

    def __init__(self, path: str):
        self.path = path
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(PREFIX.size)
            if len(head) < PREFIX.size or size < PREFIX.size + TRAILER.size:
                raise StoreError(f"{path}: truncated ({size} bytes: shorter than any store file)")
            magic, version, n = PREFIX.unpack(head)
            if magic != MAGIC:
                raise StoreError(f"{path}: not an embedding store file (magic {magic!r})")
            if version != FORMAT_VERSION:
                raise StoreError(f"{path}: format version {version}, this reader takes {FORMAT_VERSION}")
            if n > MAX_HEADER or PREFIX.size + n + TRAILER.size > size:
                raise StoreError(f"{path}: truncated (the header alone is {n} bytes, the file {size})")
            try:
                self.header = json.loads(f.read(n).decode())
                self.layout = _layout(n, int(self.header["windows"]), self.header["codec"])
                if sum(int(c[1]) for c in self.header["chunks"]) != self.layout.windows:
                    raise ValueError("the chunk table does not add up to the windows")
                missing = [k for k in PARAMETERS + ("ident", "source", "messages") if k not in self.header]
                if missing:
                    raise ValueError(f"no {missing[0]}")
            except (ValueError, KeyError, TypeError, UnicodeDecodeError) as exc:
                raise StoreError(f"{path}: unreadable header ({exc})") from None
            if self.layout.total != size:
                raise StoreError(f"{path}: truncated or padded ({size} bytes, the header implies {self.layout.total})")
            f.seek(size - TRAILER.size)
            total, end = TRAILER.unpack(f.read(TRAILER.size))
            if end != END_MAGIC or total != size:
                raise StoreError(f"{path}: no trailer for {size} bytes (truncated, or written over)")
        self.ident = self.header["ident"]
        self.windows = self.layout.windows
        self.codec = self.header["codec"]

    @property
    def parameters(self) -> dict:
        return {k: self.header[k] for k in PARAMETERS}

    def table(self) -> np.ndarray:
        """The file's checksum table: uint64 [slices, 2]."""
        with open(self.path, "rb") as f:
            f.seek(self.layout.table)
            return np.frombuffer(f.read(slices_of(self.windows) * 16), "<u8").reshape(-1, 2).astype(np.uint64)

    def records(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Records [first, first + count) as uint8 [count, record bytes], read on the host."""
        count = self.windows - first if count is None else count
        if first < 0 or count < 0 or first + count > self.windows:
            raise ValueError(f"records {first}..{first + count} of {self.windows}")
        rb = self.layout.record_bytes
        with open(self.path, "rb") as f:
            f.seek(self.layout.records + first * rb)
            data = f.read(count * rb)
        if len(data) != count * rb:
            raise StoreError(f"{self.path}: short read of records {first}..{first + count}")
        return np.frombuffer(data, np.uint8).reshape(count, rb)

    def rows_host(self) -> np.ndarray:
        """Every row decoded on the host, checksums compared (``StoreError`` names the slice)."""
        rows, sums = decode_host(self.records(), self.codec)
        _compare(self.path, 0, sums, self.table())
        return rows

    def verify(self) -> int:
        """The records against the checksum table, slice by slice, on the host.  Returns the number of records."""
        want = self.table()
        for s in range(0, slices_of(self.windows), 64):                       # 64 slices (64 MB of f32 records) at a time
            first = s * SLICE
            _, sums = decode_host(self.records(first, min(64 * SLICE, self.windows - first)), self.codec)
            _compare(self.path, s, sums, want[s:s + sums.shape[0]])
        return self.windows


def _compare(path: str, first_slice: int, got: np.ndarray, want: np.ndarray) -> None:
    got, want = np.asarray(got).view(np.uint64).reshape(-1, 2), np.asarray(want).view(np.uint64).reshape(-1, 2)
    if got.shape != want.shape:
        raise StoreError(f"{path}: {got.shape[0]} slices read, the table holds {want.shape[0]} from slice {first_slice}")
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        k = int(bad[0])
        raise StoreError(f"{path}: slice {first_slice + k} (records {(first_slice + k) * SLICE}..): checksum "
                         f"({int(got[k, 0]):#x}, {int(got[k, 1]):#x}) of the bytes read, the file's table says "
                         f"({int(want[k, 0]):#x}, {int(want[k, 1]):#x})")


# ---------------------------------------------------------------------------------------------------- the store
def is_store(path) -> bool:
    return isinstance(path, (str, os.PathLike)) and os.path.isfile(os.path.join(os.fspath(path), MANIFEST))


def as_store(dir_audio) -> Optional["Store"]:
    """``dir_audio`` as a ``Store`` when it is one (or a folder with a ``store.json``), else None: a folder of audio."""
    if isinstance(dir_audio, Store):
        return dir_audio
    return Store(os.fspath(dir_audio)) if is_store(dir_audio) else None


class StoredPart:
    """A chunk's rows in a store file: what the tools' walk hands out in place of a chunk of audio."""
    stored_rows = True

    def __init__(self, recording: "_OpenRecording", first: int, windows: int):
        self.recording, self.first, self.windows = recording, int(first), int(windows)


class _OpenRecording:
    """A store file while a tool walks it: read through the store's stager, decoded on the device, the sums of every slice read
    kept on the device until ``finish`` compares them with the file's table."""

    def __init__(self, store: "Store", rec: RecordingFile, engine):
        self.store, self.rec, self.engine = store, rec, engine
        self.fd = os.open(rec.path, os.O_RDONLY)
        self._seen: List[Tuple[int, object]] = []

    def rows(self, r0: int, r1: int):
        """Rows [r0, r1) on the engine's device, float32 [r1 - r0, 1024]: the whole slices around them are read and decoded."""
        torch = _torch()
        device = self.engine.device
        if r1 <= r0:
            return torch.empty((0, DIM), dtype=torch.float32, device=device)
        a0, a1 = r0 // SLICE * SLICE, min((r1 + SLICE - 1) // SLICE * SLICE, self.rec.windows)
        rb = self.rec.layout.record_bytes
        records = _device_empty((a1 - a0, rb), torch.uint8, device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            got = _lib.check(_lib.load().bd_stager_read(self.store._stager(device), self.fd, self.rec.layout.records + a0 * rb,
                                                        (a1 - a0) * rb, records.data_ptr(), stream.cuda_stream))
        if got != (a1 - a0) * rb:
            raise StoreError(f"{self.rec.path}: short read of records {a0}..{a1}")
        rows, sums = decode_device(records, self.rec.codec)
        self._seen.append((a0 // SLICE, sums))
        return rows[r0 - a0:r1 - a0]

    def finish(self) -> None:
        """Compares what was read with the file's table (waits for the device) and closes the file."""
        try:
            want = self.rec.table() if self._seen else None
            for first, sums in self._seen:
                got = sums.cpu().numpy()
                _compare(self.rec.path, first, got, want[first:first + got.shape[0]])
        finally:
            self.close()

    def close(self) -> None:
        if self.fd >= 0:
            os.close(self.fd)
            self.fd = -1
        self._seen = []


def stored_rows(engine, parts):
    """``dataset._embed_parts`` for parts of a store: consecutive chunks of one recording -> (rows, windows per part)."""
    rec = parts[0].recording
    at = parts[0].first
    for p in parts:
        if p.recording is not rec or p.first != at:
            raise ValueError("a launch set of stored rows takes consecutive chunks of one recording")
        at += p.windows
    if rec.engine is not engine:
        raise ValueError("these stored rows were opened for another engine")
    return rec.rows(parts[0].first, at), [p.windows for p in parts]


def _scan(dir_store: str) -> Tuple[List[RecordingFile], List[Tuple[str, StoreError]]]:
    """Every ``*.bdemb`` below ``dir_store``: the files that open, and (path, error) of those that do not."""
    found, damaged = [], []
    for path in sorted(os.path.join(root, f) for root, _, files in os.walk(dir_store) for f in files if f.endswith(SUFFIX)):
        try:
            found.append(RecordingFile(path))
        except StoreError as exc:
            damaged.append((path, exc))
    return found, damaged


class Store:
    """The recordings of ``dir_store`` (every ``*.bdemb`` below it; ``.part`` files are not read), in the order the audio folder
    was walked, and the parameters they were embedded with.  Opening reads the headers only and refuses a cut file and files
    that disagree about a parameter (``StoreError``)."""

    def __init__(self, dir_store: str):
        self.dir = os.fspath(dir_store)
        if not os.path.isdir(self.dir):
            raise FileNotFoundError(f"no such embedding store: {self.dir}")
        found, damaged = _scan(self.dir)
        if damaged:
            raise damaged[0][1]
        self.recordings: List[RecordingFile] = sorted(found, key=lambda r: r.header["source"]["path"])
        self.parameters: Optional[dict] = self.recordings[0].parameters if self.recordings else None
        for r in self.recordings:
            for k in PARAMETERS:
                if r.header[k] != self.parameters[k]:
                    raise StoreError(f"{r.path}: {k} = {r.header[k]!r}, but {self.recordings[0].path} has {self.parameters[k]!r}: "
                                     f"one store holds one set of parameters")
        self.skipped: List[str] = []                       # what the embedding run said about the folder (dataset._recordings)
        self.dropped: List[Tuple[str, str, List[str]]] = []    # (source path, ident, messages) of recordings with nothing to store
        self.seen: List[str] = [r.ident for r in self.recordings]
        manifest = os.path.join(self.dir, MANIFEST)
        if os.path.isfile(manifest):
            with open(manifest) as f:
                m = json.load(f)
            self.skipped = [str(s) for s in m.get("skipped", [])]
            self.dropped = [(str(p), str(i), [str(x) for x in ms]) for p, i, ms in m.get("dropped", [])]
            self.seen = [str(i) for i in m.get("seen", self.seen)]
        self._stagers: Dict[int, C.c_void_p] = {}

    def __len__(self) -> int:
        return len(self.recordings)

    @property
    def idents(self) -> List[str]:
        return [r.ident for r in self.recordings]

    @property
    def windows(self) -> int:
        return sum(r.windows for r in self.recordings)

    def verify(self) -> int:
        """Every file's records against its checksum table, on the host; ``StoreError`` names the file and the slice.  Returns
        the number of records checked."""
        return sum(r.verify() for r in self.recordings)

    def check(self, engine=None, framehop_prop: Optional[float] = None, chunklength: Optional[float] = None) -> None:
        """``ValueError`` when the caller's ``framehop_prop`` / ``chunklength`` (both values are named) or the engine's embedder
        weights are not the store's."""
        if self.parameters is None:
            return
        p = self.parameters
        if framehop_prop is not None or chunklength is not None:
            hop = p["framehop_prop"] if framehop_prop is None else float(framehop_prop)
            length = p["chunklength"] if chunklength is None else float(framing.round_chunklength(chunklength, FRAMELENGTH_S, DIGITS_TIME))
            if hop != p["framehop_prop"] or length != p["chunklength"]:
                raise ValueError(f"the store {self.dir} was embedded with framehop_prop={p['framehop_prop']}, chunklength="
                                 f"{p['chunklength']}; asked for framehop_prop={hop}, chunklength={length}")
        if engine is not None:
            check_weights(self.dir, p, getattr(engine, "embeddername", None), engine.weights_sha256)

    def _stager(self, device):
        torch = _torch()
        index = torch.device(device).index
        if index not in self._stagers:
            handle = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(_lib.load().bd_stager_create(C.byref(handle), index, STAGE_BYTES, 2))
            self._stagers[index] = handle
        return self._stagers[index]

    def close(self) -> None:
        """Gives the page-locked staging buffers back (waits for the devices that used them)."""
        for index, handle in list(self._stagers.items()):
            _torch().cuda.synchronize(index)
            _lib.load().bd_stager_destroy(handle)
        self._stagers = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def walk(self, engine, framehop_prop: float, chunklength: float, annotations, only_annotated: bool, messages: List[str]):
        """``dataset._sources`` for a store: (ident, chunks) per recording, the chunks' ``pcm`` handles on its rows; the messages
        of the audio route in its order.  After a recording's chunks have been consumed its checksums are compared."""
        self.check(engine, framehop_prop, chunklength)
        messages += self.skipped
        for i in sorted(set(annotations) - set(self.seen)):
            messages.append(f"annotated, but no such recording: {i}")
        todo = [(r.header["source"]["path"], r.ident, r) for r in self.recordings] + [(p, i, ms) for p, i, ms in self.dropped]
        group = 0
        for _, ident, what in sorted(todo, key=lambda t: t[0]):
            if only_annotated and ident not in annotations:
                continue
            if not isinstance(what, RecordingFile):
                messages += what
                continue
            messages += what.header["messages"]
            rec = _OpenRecording(self, what, engine)
            try:
                chunks, at = [], 0
                for start_s, n in what.header["chunks"]:
                    chunks.append(_Chunk(group, float(start_s), StoredPart(rec, at, n)))
                    at += n
                group += 1
                yield ident, chunks
                rec.finish()
            finally:
                rec.close()

    def rows(self, engine, ident: str):
        """One recording's rows on the engine's device, float32 [windows, 1024], checksums compared."""
        rec = next((r for r in self.recordings if r.ident == ident), None)
        if rec is None:
            raise KeyError(ident)
        self.check(engine)
        opened = _OpenRecording(self, rec, engine)
        try:
            rows = opened.rows(0, rec.windows)
            opened.finish()
            return rows
        finally:
            opened.close()


def check_weights(where: str, parameters: dict, embeddername: Optional[str], weights_sha256: str) -> None:
    if embeddername is not None and embeddername != parameters["embeddername"]:
        raise ValueError(f"the store {where} was embedded with {parameters['embeddername']!r}, the engine runs {embeddername!r}")
    if weights_sha256 != parameters["weights_sha256"]:
        raise ValueError(f"the store {where} was embedded with other embedder weights (sha256 {parameters['weights_sha256'][:12]}..., "
                         f"the engine's is {weights_sha256[:12]}...)")


def write_manifest(dir_store: str, skipped: Sequence[str] = (), dropped=(), seen: Optional[Sequence[str]] = None) -> None:
    """``store.json``: marks the folder as a store; keeps the embedding run's messages about recordings it did not store."""
    os.makedirs(dir_store, exist_ok=True)
    body = {"format": FORMAT_VERSION, "skipped": list(skipped), "dropped": [[p, i, list(ms)] for p, i, ms in dropped]}
    if seen is not None:
        body["seen"] = list(seen)
    tmp = os.path.join(dir_store, MANIFEST + ".part")
    with open(tmp, "w") as f:
        json.dump(body, f, indent=2)
    os.replace(tmp, os.path.join(dir_store, MANIFEST))


# ---------------------------------------------------------------------------------------------------- writing a store
@dataclass
class EmbedReport:
    """``written`` / ``kept``: idents embedded by this run / found whole and current; ``windows``: rows written by this run."""
    written: List[str] = field(default_factory=list)
    kept: List[str] = field(default_factory=list)
    windows: int = 0
    messages: List[str] = field(default_factory=list)


def _source_of(path: str, dir_audio: str) -> dict:
    from .flacio import open_track
    st = os.stat(path)
    track = open_track(path)
    try:
        return {"path": os.path.relpath(path, dir_audio).replace(os.sep, "/"), "size": int(st.st_size), "mtime_ns": int(st.st_mtime_ns),
                "rate": int(track.samplerate), "channels": int(track.channels), "duration": float(track.duration)}
    finally:
        track.close()


def embed_recordings(dir_audio: str, dir_store: str, *, codec: str = "f32", framehop_prop: float = 1.0, chunklength: float = 200,
                     engine=None, embeddername: str = "yamnet_k2") -> EmbedReport:
    """Every recording under ``dir_audio`` that ``analyze`` would take, embedded as ``dataset.embed_annotated`` embeds it (the
    same chunks, resampling and windows; a launch set whose activations left the f16 range is repeated in exact f32, so the
    rows are final), encoded on the device (``codec``: ``"f32"``, ``"h"`` or ``"b"``) and written to
    ``<dir_store>/<ident>.bdemb``.  The straight loop, recording by recording; a recording's file is renamed into place when
    it is whole.  Resumes: a whole file whose source has the same size and modification time is kept; a store made with other
    parameters is refused (``ValueError``) before anything is embedded.  A recording with a row that is not representable
    (non-finite, or negative under ``"b"``) is not stored: ``StoreError``."""
    from .analyze import build_ident, search_audio
    from .engine import hop_samples, patch_step
    torch = _torch()
    _codec(codec)
    framehop_s = FRAMELENGTH_S * framehop_prop
    hop, step = hop_samples(framehop_s), patch_step(framehop_s)
    chunklength = framing.round_chunklength(chunklength, FRAMELENGTH_S, DIGITS_TIME)
    if is_store(dir_audio):
        raise ValueError(f"{dir_audio} is an embedding store, not a folder of recordings")
    report = EmbedReport()
    engine, own = _open_engine(engine, embeddername)
    try:
        mine = {"embeddername": getattr(engine, "embeddername", embeddername), "weights_sha256": engine.weights_sha256,
                "mode": engine._mode, "resample_quality": int(engine.resample_quality), "framehop_prop": float(framehop_prop),
                "chunklength": float(chunklength), "codec": codec}
        whole, _ = _scan(dir_store) if os.path.isdir(dir_store) else ([], [])      # (a damaged file is written again)
        for r in whole:
            differ = [k for k in PARAMETERS if r.header[k] != mine[k]]
            if differ:
                raise ValueError(f"the store {dir_store} holds recordings embedded with " +
                                 ", ".join(f"{k}={r.header[k]!r}" for k in differ) + "; this run asks for " +
                                 ", ".join(f"{k}={mine[k]!r}" for k in differ))
        have = {r.ident: r for r in whole}
        skipped: List[str] = []
        todo = _recordings(dir_audio, {}, False, skipped)
        seen = [build_ident(p, dir_audio) for p in search_audio(dir_audio)]
        dropped: List[Tuple[str, str, List[str]]] = []
        write_manifest(dir_store, skipped, dropped, seen)
        report.messages += skipped
        for path, ident in todo:
            target = os.path.join(dir_store, ident + SUFFIX)
            st = os.stat(path)
            old = have.get(ident)
            if old is not None and (old.header["source"].get("size"), old.header["source"].get("mtime_ns")) == (st.st_size, st.st_mtime_ns):
                report.kept.append(ident)
                report.messages += old.header["messages"]
                continue
            said: List[str] = []
            chunks = _read_chunks(engine, path, ident, 0, chunklength, said)
            report.messages += said
            if not chunks:
                dropped.append((os.path.relpath(path, dir_audio).replace(os.sep, "/"), ident, said))
                continue
            parts = [c.pcm for c in chunks]
            windows = [_part_windows(engine, p, hop, step) for p in parts]
            header = make_header(ident=ident, chunks=[(c.start_s, n) for c, n in zip(chunks, windows)], messages=said,
                                 source=_source_of(path, dir_audio), **mine)
            writer = _FileWriter(target, header)
            try:
                pending, bad = None, []
                for a, b in _launch_sets(parts, windows):
                    emb, counts = _embed_parts(engine, parts[a:b], hop, step)
                    if list(counts) != windows[a:b]:
                        raise StoreError(f"{ident}: the pass gave {list(counts)} windows, the chunk table says {windows[a:b]}")
                    rows = emb if pending is None else torch.cat([pending, emb])
                    whole = int(rows.shape[0]) // SLICE * SLICE           # whole slices go out; the rest waits for the next set
                    if whole:
                        bad.append(_encode_into(writer, rows[:whole], codec))
                    pending = rows[whole:] if whole < rows.shape[0] else None
                if pending is not None:
                    bad.append(_encode_into(writer, pending.contiguous(), codec))
                flagged = sum(int(f.cpu()[0]) for f in bad)
                if flagged:
                    raise StoreError(f"{ident}: {flagged} of {sum(windows)} embeddings are not representable under codec {codec!r} "
                                     f"(non-finite, or negative under \"b\"); the recording is not stored")
            except BaseException:
                writer.abort()
                raise
            writer.close()
            report.written.append(ident)
            report.windows += sum(windows)
        write_manifest(dir_store, skipped, dropped, seen)
        return report
    finally:
        if own:
            engine.close()


def _encode_into(writer: _FileWriter, rows, codec: str):
    """One encode call's records and sums to the file; returns the call's flags word, still on the device."""
    records, sums, flags = encode_device(rows, codec)
    writer.append(records.cpu().numpy(), sums.cpu().numpy())
    return flags


# ---------------------------------------------------------------------------------------------------- scoring a store
def score_store(dir_store, modelname="model_general_v3", dir_out: Optional[str] = None, classes_out="all",
                precision: Optional[float] = None, *, engine=None, dir_models: Optional[str] = None):
    """``analyze(modelname, classes_out, precision, dir_out=...)`` from a store in place of the audio: the same result trees,
    byte for byte (``<ident>_buzzdetect.csv`` and the manifest; for a list of models one tree per model, ``<dir_out>/<name>``
    or ``models/<name>/output``), written by the writer's own formatting (``pipeline.Member.csv``, ``results.ResultFile``,
    ``Pipeline._finalize_file``) and locked by the same manifests.  Framehop and chunks are the store's.  Every launch set of
    stored rows goes through ``engine.score_rows``: the heads alone, no embedder launch.  A recording whose result files
    exist is left alone; a partial file of an interrupted run is written again from the start.  ``engine``: a ``HipEngine``
    that carries the model (or the set, in this order).  Returns ``analyze``'s ``Report``."""
    from . import results, weights
    from .analyze import member_dirs, set_members
    from .engine import HipEngine
    from .pipeline import Member, MemberFile, Pipeline, Report
    store = as_store(dir_store)
    if store is None:
        raise ValueError(f"{dir_store} is not an embedding store (no {MANIFEST})")
    several = isinstance(modelname, (list, tuple))
    names = list(modelname) if several else [modelname]
    if engine is not None:
        carried = list(engine.members) if getattr(engine, "members", None) else None
        if several and carried != names:
            raise ValueError(f"engine= must carry the models {names} as a set of heads, in this order; this one carries {carried}")
        if not several and carried is not None:
            raise ValueError(f"engine= carries a set of heads ({carried}); name the same models as a list")
    if several:
        heads = dict(engine.members) if engine is not None else weights.load_head_set(names, dir_models)
        members = set_members(heads, classes_out, precision)
        dirs = member_dirs(names, dir_out)
    else:
        head = getattr(engine, "head", None) if engine is not None else None
        if head is None:
            head = weights.load_head(modelname, dir_models)
        keep = list(head.classes) if classes_out == "all" else classes_out
        threshold = None if precision is None else results.threshold_for_precision(modelname, precision, metrics_path=head.metrics_path)
        members = [Member(modelname, slice(0, len(head.classes)), list(head.classes), keep, head.digits_results, threshold)]
        dirs = {modelname: dir_out or os.path.join("models", modelname, "output")}
    report = Report(files_total=len(store))
    if store.parameters is None:
        return report
    framehop_prop = store.parameters["framehop_prop"]
    framehop_s = FRAMELENGTH_S * framehop_prop
    if float(framehop_prop).is_integer():                  # the manifest's text for analyze's default: 1, not 1.0 (they compare equal)
        framehop_prop = int(framehop_prop)
    for m in members:
        ok, msg = results.check_or_write_manifest(dirs[m.name], results.build_manifest(m.name, framehop_prop, precision, m.classes_out))
        if not ok:
            raise RuntimeError(msg)
    own = engine is None
    if own:
        kind = dict(heads=heads) if several else dict(head=head)
        engine = HipEngine(embeddername=store.parameters["embeddername"], **kind)
    try:
        if not engine.n_classes:
            raise ValueError("score_store needs an engine with a classifier")
        done = {r.ident for r in store.recordings
                if all(results.ResultFile(os.path.join(dirs[m.name], r.ident)).complete for m in members)}
        report.files_skipped = len(done)
        messages: List[str] = []
        for ident, chunks in store.walk(engine, framehop_prop, store.parameters["chunklength"], {}, False, messages):
            if ident in done:
                continue
            files = [MemberFile(k, results.ResultFile(os.path.join(dirs[m.name], ident))) for k, m in enumerate(members)]
            for mf in files:
                if os.path.exists(mf.rf.path_partial):
                    os.remove(mf.rf.path_partial)
            parts = [c.pcm for c in chunks]
            for a, b in _launch_sets(parts, [p.windows for p in parts]):
                rows, counts = stored_rows(engine, parts[a:b])
                logits = engine.score_rows(rows).cpu().numpy()
                at = 0
                for c, n in zip(chunks[a:b], counts):
                    for mf in files:
                        head_line, body = members[mf.member].csv(logits[at:at + n], framehop_s, DIGITS_TIME, c.start_s)
                        mf.rf.append_text(head_line, body)
                        mf.header = head_line
                        mf.bodies.append((c.start_s, body))
                    at += n
                    report.chunks += 1
                    report.windows += n
            wrote = [Pipeline._finalize_file(mf.rf, mf) for mf in files]
            report.files_done += 1 if any(wrote) else 0
        report.messages += messages
        return report
    finally:
        if own:
            engine.close()
