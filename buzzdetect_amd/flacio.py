"""FLAC files by positioned reads: the streamer's view of a FLAC recording (the counterpart of wavio.WavTrack).

The file is parsed once (an optional ID3v2 tag, ``fLaC``, STREAMINFO, SEEKTABLE; other metadata blocks are skipped),
and its readable length comes from ONE read of its tail: the end of the last complete frame.  A chunk's compressed
bytes are found by ``byte_range`` - seek table, then interpolation search by small reads whose frame headers are
parsed by ``bd_flac_parse_frame_header`` - and decoded on the device (``bd_flac_decode``, include/buzzdetect_flac.h).
Nothing here passes over the whole file.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .devdecode import DeviceDecoder
from .wavio import WavFormatError, WavTrack

SEARCH_WINDOW = 64 << 10          # bytes read per probe of the locator


class FlacFormatError(WavFormatError):
    pass


def open_track(path: str):
    """WavTrack, FlacTrack or pcmio.PcmTrack, chosen by the file's magic bytes: fLaC (an ID3v2 tag before it allowed),
    FORM / .snd / the Wave64 riff GUID, RIFF / RF64 with a codec format tag (pcmio.CODEC_TAGS); any other RIFF is WavTrack's."""
    from . import pcmio
    with open(path, "rb") as f:
        head = f.read(16)
    if head[:4] == b"fLaC" or head[:3] == b"ID3":
        return FlacTrack(path)
    if pcmio.claims(path, head):
        return pcmio.PcmTrack(path)
    return WavTrack(path)


class FlacDecoder(DeviceDecoder):
    """One thread's device-side FLAC decoder state (bd_flac_decode)."""
    status_type, workspace_fn, decode_fn = _lib.bd_flac_status, "bd_flac_workspace_bytes", "bd_flac_decode"


class FlacTrack:
    decoder = FlacDecoder             # the device decoder of this track's ranges

    def __init__(self, path: str):
        self.path = path
        self._lib = _lib.load()
        self._fd = os.open(path, os.O_RDONLY)
        try:
            self._parse()
        except BaseException:
            self.close()
            raise

    # ------------------------------------------------------------------ metadata
    def _pread(self, off: int, n: int) -> bytes:
        return os.pread(self._fd, max(0, n), off) if n > 0 else b""

    def _parse(self) -> None:
        self.size = os.fstat(self._fd).st_size
        at = 0
        head = self._pread(0, 10)
        if head[:3] == b"ID3" and len(head) == 10:
            size = (head[6] << 21) | (head[7] << 14) | (head[8] << 7) | head[9]
            at = 10 + size + (10 if head[5] & 0x10 else 0)
        if self._pread(at, 4) != b"fLaC":
            raise FlacFormatError(f"{self.path}: not a FLAC stream")
        at += 4
        info, seek = None, []
        while True:
            bh = self._pread(at, 4)
            if len(bh) < 4:
                raise FlacFormatError(f"{self.path}: metadata ends early")
            last, kind, length = bh[0] >> 7, bh[0] & 0x7F, int.from_bytes(bh[1:4], "big")
            if kind == 0:
                info = self._pread(at + 4, length)
            elif kind == 3:
                data = self._pread(at + 4, length)
                for k in range(len(data) // 18):
                    s, o, _ = struct.unpack(">QQH", data[18 * k: 18 * k + 18])
                    if s != 0xFFFFFFFFFFFFFFFF:
                        seek.append((s, o))
            at += 4 + length
            if last:
                break
        if info is None or len(info) < 34:
            raise FlacFormatError(f"{self.path}: no STREAMINFO")
        min_bs, max_bs = struct.unpack(">HH", info[:4])
        self.max_framesize = int.from_bytes(info[7:10], "big")
        v = int.from_bytes(info[10:18], "big")
        self.samplerate = v >> 44
        self.channels = ((v >> 41) & 7) + 1
        self.bits_per_sample = ((v >> 36) & 31) + 1
        total = v & ((1 << 36) - 1)
        if self.bits_per_sample > 24 or self.bits_per_sample < 4:
            raise FlacFormatError(f"{self.path}: {self.bits_per_sample}-bit FLAC is not supported (4-24 bits)")
        if self.samplerate < 1 or max_bs < 16 or min_bs < 1:
            raise FlacFormatError(f"{self.path}: bad STREAMINFO")
        self.si = _lib.bd_flac_streaminfo(min_bs, max_bs, self.samplerate, self.channels, self.bits_per_sample, 0, total)
        self.first_frame = at
        self._seek = sorted(seek)
        self._bound = max_bs * self.channels * ((self.bits_per_sample + 1 + 7) // 8) + 1024   # largest possible frame
        readable, self.end_offset = self._tail()
        # `frames` is what can be read; `frames_declared` what STREAMINFO promises (0: unknown -> what can be read)
        self.frames = min(readable, total) if total else readable
        self.frames_declared = total if total else readable

    def _headers(self, off: int, data: bytes) -> List[Tuple[int, "_lib.bd_flac_frame_header"]]:
        """Valid frame headers in `data` (file offset `off`), in order."""
        a = np.frombuffer(data, np.uint8)
        if a.size < 2:
            return []
        hits = np.nonzero((a[:-1] == 0xFF) & ((a[1:] & 0xFE) == 0xF8))[0]
        out = []
        base = C.cast(C.c_char_p(data), C.c_void_p).value
        for k in hits.tolist():
            h = _lib.bd_flac_frame_header()
            if self._lib.bd_flac_parse_frame_header(base + k, len(data) - k, C.byref(self.si), C.byref(h)) > 0:
                out.append((off + k, h))
        return out

    def _tail(self) -> Tuple[int, int]:
        """(samples readable, end offset of the last complete frame) from a read of the file's tail."""
        span = max(SEARCH_WINDOW, 3 * max(self.max_framesize, 1) + 1024)
        while True:
            start = max(self.first_frame, self.size - span)
            data = self._pread(start, self.size - start)
            buf = np.frombuffer(data, np.uint8)
            st = _lib.bd_flac_status()
            for off, h in self._headers(start, data):
                rel = off - start
                view = buf[rel:]
                _lib.check(self._lib.bd_flac_decode_host(view.ctypes.data if view.size else None, view.size, C.byref(self.si),
                                                         0, 0, None, C.byref(st)))
                if st.frames > 0:
                    return int(st.end_sample), off + int(st.stop_offset)
            if start == self.first_frame:
                return 0, self.first_frame
            span *= 4

    # ------------------------------------------------------------------ locating frames
    def _frame_at_or_after(self, off: int, lo_s: int, hi_s: int):
        """The first header at or after `off` whose first sample lies in [lo_s, hi_s]."""
        while off < self.end_offset:
            data = self._pread(off, min(SEARCH_WINDOW, self.end_offset - off + 16))
            for o, h in self._headers(off, data):
                if o < self.end_offset and lo_s <= h.first_sample <= hi_s:
                    return o, h
            off += max(1, len(data) - 32)
        return None

    def _next_frame(self, off: int, h):
        """The frame after the one at `off` (the first header behind it whose number follows on), or None at the end."""
        if h.first_sample + h.blocksize >= self.frames or off >= self.end_offset:
            return None
        data = self._pread(off + h.header_bytes, min(self._bound + 32, self.end_offset - off - h.header_bytes + 16))
        for o, g in self._headers(off + h.header_bytes, data):
            if g.variable == h.variable and (g.number == h.number + (h.blocksize if h.variable else 1)):
                return o, g
        return None

    def locate(self, sample: int):
        """(file offset, header) of the frame that holds `sample` (0 <= sample < frames)."""
        lo = (self.first_frame, 0)
        for s, o in self._seek:
            if s <= sample and self.first_frame + o < self.end_offset:
                lo = (self.first_frame + o, s)
        hi = (self.end_offset, self.frames)
        step = 0
        while hi[0] - lo[0] > SEARCH_WINDOW:
            span = hi[1] - lo[1]
            if step % 2 == 0 and span > 0:          # interpolation, then bisection, in turn: progress either way
                mid = lo[0] + int((hi[0] - lo[0]) * (sample - lo[1]) / span)
            else:
                mid = (lo[0] + hi[0]) // 2
            mid = min(max(mid, lo[0] + 1), hi[0] - 1)
            step += 1
            found = self._frame_at_or_after(mid, lo[1] + 1, hi[1])
            if found is None or found[0] >= hi[0]:
                hi = (mid, hi[1])
            elif found[1].first_sample <= sample:
                lo = (found[0], int(found[1].first_sample))
            else:
                hi = (found[0], int(found[1].first_sample))
        data = self._pread(lo[0], 16)
        h = _lib.bd_flac_frame_header()
        if len(data) < 6 or self._lib.bd_flac_parse_frame_header(data, len(data), C.byref(self.si), C.byref(h)) <= 0:
            raise FlacFormatError(f"{self.path}: no frame header at byte {lo[0]}")
        cur = (lo[0], h)
        while cur[1].first_sample + cur[1].blocksize <= sample:
            nxt = self._next_frame(*cur)
            if nxt is None:
                break
            cur = nxt
        return cur

    def byte_range(self, first: int, n: int) -> Tuple[int, int]:
        """File offsets [a, b): a is where the frame holding `first` starts, b where the frame holding first + n - 1 ends."""
        first = min(max(int(first), 0), self.frames)
        last = min(first + max(int(n), 1), self.frames) - 1
        if last < first:
            return self.end_offset, self.end_offset
        a, _ = self.locate(first)
        b, hb = self.locate(last)
        nxt = self._next_frame(b, hb)
        return a, (nxt[0] if nxt is not None else self.end_offset)

    # ------------------------------------------------------------------ the WavTrack surface the pipeline uses
    @property
    def duration(self) -> float:
        return self.frames_declared / self.samplerate

    @property
    def duration_readable(self) -> float:
        return self.frames / self.samplerate

    @property
    def is_s16(self) -> bool:
        return self.bits_per_sample == 16

    @property
    def fd(self) -> int:
        return self._fd

    @property
    def out_bytes_per_frame(self) -> int:
        """Bytes of one decoded frame: int16 for 16-bit streams, float32 otherwise."""
        return self.channels * (2 if self.is_s16 else 4)

    @property
    def header(self) -> "_lib.bd_flac_streaminfo":
        """What the decode calls take as the stream's description."""
        return self.si

    def pieces(self, first: int, n: int) -> List[Tuple[int, int]]:
        """A FLAC range is staged and decoded as one piece (pcmio.PcmTrack.pieces)."""
        return [(first, n)]

    def decode_host_into(self, first: int, n: int, out_ptr: Optional[int]) -> "_lib.bd_flac_status":
        """Samples [first, first + n) decoded on the host to `out_ptr` (int16 or float32, interleaved); the status."""
        a, b = self.byte_range(first, n)
        data = np.frombuffer(self._pread(a, b - a), np.uint8)
        st = _lib.bd_flac_status()
        _lib.check(self._lib.bd_flac_decode_host(data.ctypes.data if data.size else None, data.size, C.byref(self.si), first, n,
                                                 out_ptr, C.byref(st)))
        return st

    def decode_host(self, first: int, n: int) -> Tuple[np.ndarray, "_lib.bd_flac_status"]:
        """Samples [first, first + n) decoded on the host: ([got, channels] int16 or float32, status)."""
        out = np.zeros((max(n, 0), self.channels), np.int16 if self.is_s16 else np.float32)
        st = self.decode_host_into(first, n, out.ctypes.data if out.size else None)
        return out[: st.samples], st

    def __del__(self):
        self.close()

    def close(self) -> None:
        fd, self._fd = getattr(self, "_fd", None), None
        if fd is not None:
            os.close(fd)

