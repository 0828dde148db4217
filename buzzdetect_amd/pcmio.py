"""AIFF / AIFF-C, Sun AU, Sony Wave64 and the codec tags of RIFF/RF64 WAVE by positioned reads: the streamer's view of a
recording in one of libsndfile's table-free formats (the counterpart of wavio.WavTrack and flacio.FlacTrack).

The container is parsed once on the host; its sample encoding becomes a ``bd_pcm_format`` (include/buzzdetect_pcm.h):
linear integers of 8-32 bits and IEEE floats in either byte order, G.711 mu-law / A-law, IMA/DVI ADPCM (tag 0x11) and
Microsoft ADPCM (tag 2).  A chunk's bytes (``byte_range``: whole blocks, no search) go to the device as they lie in the
file and are decoded there (``bd_pcm_decode``) into the layout a WAV chunk has: int16 for 16-bit linear, G.711 and ADPCM,
float32 otherwise.

    container   magic                 encodings
    AIFF        FORM....AIFF          big-endian signed 8-32 bit
    AIFF-C      FORM....AIFC          NONE / twos, sowt (little-endian 16 bit), fl32, fl64, ulaw, alaw
    AU          .snd                  1 mu-law, 2-5 linear 8-32 bit, 6 float, 7 double, 27 A-law (big-endian)
    Wave64      the riff GUID         every WAVE fmt tag below, PCM and float included
    RIFF/RF64   RIFF / RF64 + WAVE    tags 6 (A-law), 7 (mu-law), 0x11 (IMA ADPCM), 2 (MS ADPCM); PCM and float stay WavTrack's

The declared length (AIFF numSampleFrames, AU data size, a ``fact`` chunk, the data chunk's size) is ``frames_declared``;
what the file's bytes hold is ``frames``: a file cut short gets the reference's bad-read handling (wavio.WavTrack's rule,
placeholder sizes included).
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from fractions import Fraction
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .devdecode import DeviceDecoder
from .wavio import FORMAT_EXTENSIBLE, FORMAT_FLOAT, FORMAT_PCM, WavFormatError

FORMAT_MS_ADPCM, FORMAT_ALAW, FORMAT_ULAW, FORMAT_IMA_ADPCM = 2, 6, 7, 0x11
CODEC_TAGS = (FORMAT_MS_ADPCM, FORMAT_ALAW, FORMAT_ULAW, FORMAT_IMA_ADPCM)     # the WAVE tags this module reads

_W64_TAIL = b"\xf3\xac\xd3\x11\x8c\xd1\x00\xc0\x4f\x8e\xdb\x8a"
W64_RIFF = b"riff\x2e\x91\xcf\x11\xa5\xd6\x28\xdb\x04\xc1\x00\x00"
W64_WAVE = b"wave" + _W64_TAIL
W64_FMT = b"fmt " + _W64_TAIL
W64_FACT = b"fact" + _W64_TAIL
W64_DATA = b"data" + _W64_TAIL

AIFC_TYPES = {   # compression type -> (codec, bytes per sample or None: from sampleSize, big-endian)
    b"NONE": (_lib.PCM_LINEAR, None, 1), b"twos": (_lib.PCM_LINEAR, None, 1), b"sowt": (_lib.PCM_LINEAR, None, 0),
    b"fl32": (_lib.PCM_FLOAT, 4, 1), b"FL32": (_lib.PCM_FLOAT, 4, 1), b"fl64": (_lib.PCM_FLOAT, 8, 1),
    b"FL64": (_lib.PCM_FLOAT, 8, 1), b"ulaw": (_lib.PCM_ULAW, 1, 1), b"ULAW": (_lib.PCM_ULAW, 1, 1),
    b"alaw": (_lib.PCM_ALAW, 1, 1), b"ALAW": (_lib.PCM_ALAW, 1, 1),
}
AU_ENCODINGS = {1: (_lib.PCM_ULAW, 1), 2: (_lib.PCM_LINEAR, 1), 3: (_lib.PCM_LINEAR, 2), 4: (_lib.PCM_LINEAR, 3),
                5: (_lib.PCM_LINEAR, 4), 6: (_lib.PCM_FLOAT, 4), 7: (_lib.PCM_FLOAT, 8), 27: (_lib.PCM_ALAW, 1)}
PLACEHOLDER = 0x7FFFF000          # data sizes from here on say nothing about the length (wavio.WavTrack)
PIECE_BYTES = 256 << 20           # a range is staged and decoded in pieces of whole blocks of at most this many bytes
                                  # (bd_pcm_decode takes ranges below 2 GiB; 600 s of 8-channel 96 kHz float64 is 3.7 GB)


class PcmFormatError(WavFormatError):
    pass


def make_format(codec: int, channels: int, width: int = 1, big_endian: bool = False, signed: bool = True,
                block_align: Optional[int] = None, samples_per_block: int = 1, coefs=()) -> "_lib.bd_pcm_format":
    """A bd_pcm_format; `width` is bytes per stored sample (ignored by ADPCM, which is 4 bits)."""
    f = _lib.bd_pcm_format()
    f.codec, f.channels = codec, channels
    adpcm = codec in (_lib.PCM_IMA_ADPCM, _lib.PCM_MS_ADPCM)
    f.bits = 4 if adpcm else 8 * width
    f.big_endian, f.is_signed = int(bool(big_endian)), int(bool(signed))
    f.block_align = block_align if block_align is not None else channels * width
    f.samples_per_block = samples_per_block
    f.n_coefs = len(coefs) // 2
    for i, c in enumerate(coefs[: 2 * _lib.PCM_MAX_COEFS]):
        f.coefs[i] = c
    return f


def out_is_s16(f) -> bool:
    return (f.codec == _lib.PCM_LINEAR and f.bits == 16) or f.codec in (_lib.PCM_ULAW, _lib.PCM_ALAW, _lib.PCM_IMA_ADPCM,
                                                                       _lib.PCM_MS_ADPCM)


def block_frames(f, rem: int) -> int:
    """Frames whose codes lie entirely inside the first `rem` bytes of a block (pcmcodec.hip's block_frames)."""
    ch = f.channels
    if f.codec == _lib.PCM_IMA_ADPCM:
        if rem < 4 * ch:
            return 0
        body = rem - 4 * ch
        r = body % (4 * ch) - 4 * (ch - 1)
        k = 1 + 8 * (body // (4 * ch)) + (min(8, 2 * r) if r > 0 else 0)
    elif f.codec == _lib.PCM_MS_ADPCM:
        if rem < 7 * ch:
            return 0
        k = 2 + 2 * (rem - 7 * ch) // ch
    else:
        k = 1 if rem >= f.block_align else 0
    return min(k, f.samples_per_block)


def frames_in(f, nbytes: int) -> int:
    """Frames `nbytes` of sample data hold (a final block cut short counts what it holds)."""
    nbytes = max(0, int(nbytes))
    return (nbytes // f.block_align) * f.samples_per_block + block_frames(f, nbytes % f.block_align)


def wave_format(fmt: bytes, where: str, codecs_only: bool) -> Tuple["_lib.bd_pcm_format", int]:
    """A WAVE fmt chunk body -> (bd_pcm_format, sample rate).  `codecs_only`: PCM and float are refused (RIFF: WavTrack's)."""
    if len(fmt) < 16:
        raise PcmFormatError(f"{where}: fmt chunk too short")
    tag, ch, rate, _, block, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == FORMAT_EXTENSIBLE and len(fmt) >= 26:
        tag = struct.unpack("<H", fmt[24:26])[0]
    if ch < 1 or ch > 8 or rate < 1:
        raise PcmFormatError(f"{where}: {ch} channels at {rate} Hz not supported")
    ext = fmt[18: 18 + struct.unpack("<H", fmt[16:18])[0]] if len(fmt) >= 18 else b""
    if tag in (FORMAT_PCM, FORMAT_FLOAT) and not codecs_only:
        width = bits // 8
        ok = width in (1, 2, 3, 4) if tag == FORMAT_PCM else width in (4, 8)
        if not ok or block != width * ch:
            raise PcmFormatError(f"{where}: unsupported sample layout ({bits} bits, block align {block})")
        codec = _lib.PCM_LINEAR if tag == FORMAT_PCM else _lib.PCM_FLOAT
        return make_format(codec, ch, width, signed=not (tag == FORMAT_PCM and width == 1)), rate
    if tag in (FORMAT_ULAW, FORMAT_ALAW):
        if block != ch:
            raise PcmFormatError(f"{where}: G.711 with block align {block}")
        return make_format(_lib.PCM_ULAW if tag == FORMAT_ULAW else _lib.PCM_ALAW, ch, 1), rate
    if tag in (FORMAT_IMA_ADPCM, FORMAT_MS_ADPCM) and bits != 4:
        raise PcmFormatError(f"{where}: {bits}-bit ADPCM is not supported (4 bits per code)")
    if tag == FORMAT_IMA_ADPCM:
        if len(ext) < 2:
            raise PcmFormatError(f"{where}: IMA ADPCM fmt without samples per block")
        spb = struct.unpack("<H", ext[:2])[0]
        f = make_format(_lib.PCM_IMA_ADPCM, ch, block_align=block, samples_per_block=spb)
    elif tag == FORMAT_MS_ADPCM:
        if len(ext) < 4:
            raise PcmFormatError(f"{where}: MS ADPCM fmt without its coefficient table")
        spb, ncoef = struct.unpack("<HH", ext[:4])
        if ncoef < 1 or ncoef > _lib.PCM_MAX_COEFS or len(ext) < 4 + 4 * ncoef:
            raise PcmFormatError(f"{where}: MS ADPCM with {ncoef} coefficient pairs")
        f = make_format(_lib.PCM_MS_ADPCM, ch, block_align=block, samples_per_block=spb,
                        coefs=struct.unpack(f"<{2 * ncoef}h", ext[4: 4 + 4 * ncoef]))
    else:
        raise PcmFormatError(f"{where}: unsupported WAVE format tag {tag:#x}")
    hdr = (4 if tag == FORMAT_IMA_ADPCM else 7) * ch
    cap = block_frames(make_format(f.codec, ch, block_align=block, samples_per_block=1 << 30), block)
    if block < hdr or spb < (1 if tag == FORMAT_IMA_ADPCM else 2) or spb > cap:
        raise PcmFormatError(f"{where}: {spb} samples do not fit an ADPCM block of {block} bytes")
    return f, rate


def wave_codec_tag(path: str) -> Optional[int]:
    """The format tag of a RIFF/RF64 WAVE file's fmt chunk (extensible resolved), None when there is none."""
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] not in (b"RIFF", b"RF64") or head[8:12] != b"WAVE":
            return None
        size = fh.seek(0, 2)
        at = 12
        while at + 8 <= size:
            fh.seek(at)
            cid, clen = struct.unpack("<4sI", fh.read(8))
            if cid == b"fmt ":
                fmt = fh.read(min(clen, 26))
                if len(fmt) < 2:
                    return None
                tag = struct.unpack("<H", fmt[:2])[0]
                if tag == FORMAT_EXTENSIBLE and len(fmt) >= 26:
                    tag = struct.unpack("<H", fmt[24:26])[0]
                return tag
            if cid == b"data":
                return None
            at += 8 + clen + (clen & 1)
    return None


def claims(path: str, head: bytes) -> bool:
    """True when PcmTrack (not WavTrack) opens this file: the magic of AIFF, AU or Wave64, or WAVE with a codec tag."""
    if head[:4] in (b"FORM", b".snd") or head[:16] == W64_RIFF:
        return True
    return head[:4] in (b"RIFF", b"RF64") and wave_codec_tag(path) in CODEC_TAGS


def _extended_rate(b: bytes) -> Fraction:
    """The 80-bit IEEE extended float of AIFF's COMM chunk, exactly."""
    se, mant = struct.unpack(">HQ", b[:10])
    if se & 0x7FFF == 0 and mant == 0:
        return Fraction(0)
    v = Fraction(mant) * Fraction(2) ** ((se & 0x7FFF) - 16383 - 63)
    return -v if se & 0x8000 else v


class PcmDecoder(DeviceDecoder):
    """One thread's device-side decoder state for pcmio's formats (bd_pcm_decode); its workspace is kept zeroed."""
    status_type, workspace_fn, decode_fn, ws_zeroed = _lib.bd_pcm_status, "bd_pcm_workspace_bytes", "bd_pcm_decode", 256


class PcmTrack:
    decoder = PcmDecoder              # the device decoder of this track's ranges

    def __init__(self, path: str):
        self.path = path
        self._fd = os.open(path, os.O_RDONLY)
        try:
            self.size = os.fstat(self._fd).st_size
            head = os.pread(self._fd, 16, 0)
            if head[:4] == b"FORM":
                self._parse_aiff()
            elif head[:4] == b".snd":
                self._parse_au()
            elif head[:16] == W64_RIFF:
                self._parse_w64()
            elif head[:4] in (b"RIFF", b"RF64"):
                self._parse_wave()
            else:
                raise PcmFormatError(f"{path}: not an AIFF, AU, Wave64 or WAVE file")
        except BaseException:
            self.close()
            raise

    # ------------------------------------------------------------------ containers
    def _pread(self, off: int, n: int) -> bytes:
        return os.pread(self._fd, n, off) if n > 0 else b""

    def _finish(self, f, rate: int, data_off: int, data_declared: Optional[int], frames_declared: Optional[int] = None) -> None:
        """Readable and declared lengths from the data's place, its declared size in bytes (None: to the end of the file)
        and a declared frame count (AIFF numSampleFrames, a fact chunk) where the container has one."""
        self.fmt, self.samplerate, self.channels = f, int(rate), int(f.channels)
        end = self.size - data_off
        avail = max(0, end if data_declared is None else min(data_declared, end))
        self.frames = frames_in(f, avail)
        if frames_declared is not None:
            self.frames = min(self.frames, int(frames_declared))
            self.frames_declared = max(self.frames, int(frames_declared))
        elif data_declared is None:
            self.frames_declared = self.frames
        else:
            self.frames_declared = max(self.frames, frames_in(f, data_declared))
        self.data_off, self.data_bytes = data_off, avail

    def _parse_aiff(self) -> None:
        head = self._pread(0, 12)
        if len(head) < 12 or head[8:12] not in (b"AIFF", b"AIFC"):
            raise PcmFormatError(f"{self.path}: not an AIFF file")
        aifc = head[8:12] == b"AIFC"
        comm = ssnd = None
        at = 12
        while at + 8 <= self.size:
            cid, clen = struct.unpack(">4sI", self._pread(at, 8))
            if cid == b"COMM":
                comm = self._pread(at + 8, min(clen, 256))
            elif cid == b"SSND":
                ssnd = (at + 8, clen)
            at += 8 + clen + (clen & 1)                # chunks of odd length are padded to even
        if comm is None or len(comm) < 18 or ssnd is None:
            raise PcmFormatError(f"{self.path}: missing COMM or SSND chunk")
        ch, nframes, bits = struct.unpack(">hIh", comm[:8])
        rate = _extended_rate(comm[8:18])
        if rate.denominator != 1 or rate < 1:
            raise PcmFormatError(f"{self.path}: sample rate {float(rate)} Hz is not a whole number")
        ctype = comm[18:22] if aifc else b"NONE"
        if ctype not in AIFC_TYPES:
            raise PcmFormatError(f"{self.path}: AIFF-C compression {ctype!r} is not supported")
        if ch < 1 or ch > 8:
            raise PcmFormatError(f"{self.path}: {ch} channels not supported")
        codec, width, be = AIFC_TYPES[ctype]
        if width is None:
            width = (bits + 7) // 8
            if width not in (1, 2, 3, 4) or (not be and width != 2):
                raise PcmFormatError(f"{self.path}: {bits}-bit {ctype.decode(errors='replace')} samples not supported")
        f = make_format(codec, ch, width, big_endian=bool(be))
        if len(self._pread(ssnd[0], 8)) < 8:
            raise PcmFormatError(f"{self.path}: SSND chunk ends early")
        offset = struct.unpack(">I", self._pread(ssnd[0], 4))[0]
        data_off = ssnd[0] + 8 + offset
        self.container = "aifc" if aifc else "aiff"
        self._finish(f, int(rate), data_off, max(0, ssnd[1] - 8 - offset), frames_declared=nframes)

    def _parse_au(self) -> None:
        head = self._pread(0, 24)
        if len(head) < 24:
            raise PcmFormatError(f"{self.path}: AU header ends early")
        off, size, enc, rate, ch = struct.unpack(">IIIII", head[4:24])
        if enc not in AU_ENCODINGS:
            raise PcmFormatError(f"{self.path}: AU encoding {enc} is not supported")
        if ch < 1 or ch > 8 or rate < 1 or off < 24:
            raise PcmFormatError(f"{self.path}: {ch} channels at {rate} Hz not supported")
        codec, width = AU_ENCODINGS[enc]
        f = make_format(codec, ch, width, big_endian=True)
        self.container = "au"
        # 0xFFFFFFFF: "unknown", the data runs to the end of the file
        self._finish(f, rate, off, None if size == 0xFFFFFFFF else size)

    def _parse_w64(self) -> None:
        if self._pread(24, 16) != W64_WAVE:
            raise PcmFormatError(f"{self.path}: not a Wave64 WAVE file")
        fmt = data = fact = None
        at = 40
        while at + 24 <= self.size:
            guid, clen = struct.unpack("<16sQ", self._pread(at, 24))
            if clen < 24:
                break
            if guid == W64_FMT:
                fmt = self._pread(at + 24, min(clen - 24, 1024))
            elif guid == W64_FACT:
                fact = self._pread(at + 24, 8)
            elif guid == W64_DATA:
                data = (at + 24, clen - 24)
                break
            at += (clen + 7) // 8 * 8                      # chunks are aligned to 8 bytes
        if fmt is None or data is None:
            raise PcmFormatError(f"{self.path}: missing fmt or data chunk")
        f, rate = wave_format(fmt, self.path, codecs_only=False)
        declared = struct.unpack("<Q", fact)[0] if fact is not None and len(fact) == 8 and f.samples_per_block > 1 else None
        self.container = "w64"
        self._finish(f, rate, data[0], data[1], frames_declared=declared)

    def _parse_wave(self) -> None:
        fmt = data = fact = None
        at = 12
        while at + 8 <= self.size:
            cid, clen = struct.unpack("<4sI", self._pread(at, 8))
            if cid == b"fmt ":
                fmt = self._pread(at + 8, min(clen, 1024))
            elif cid == b"fact":
                fact = self._pread(at + 8, 4)
            elif cid == b"data":
                data = (at + 8, clen)
                break
            at += 8 + clen + (clen & 1)
        if fmt is None or data is None:
            raise PcmFormatError(f"{self.path}: missing fmt or data chunk")
        f, rate = wave_format(fmt, self.path, codecs_only=True)
        # fact holds the sample count of a compressed stream (blocks are padded): the declared length when it is there
        declared = struct.unpack("<I", fact)[0] if fact is not None and len(fact) == 4 and f.samples_per_block > 1 else None
        self.container = "wave"
        self._finish(f, rate, data[0], None if data[1] >= PLACEHOLDER else data[1], frames_declared=declared)

    # ------------------------------------------------------------------ the surface the pipeline uses
    @property
    def duration(self) -> float:
        return self.frames_declared / self.samplerate

    @property
    def duration_readable(self) -> float:
        return self.frames / self.samplerate

    @property
    def is_s16(self) -> bool:
        return out_is_s16(self.fmt)

    @property
    def raw_s16(self) -> bool:
        """The file holds little-endian 16-bit samples: its bytes are the slot's (no decode)."""
        f = self.fmt
        return f.codec == _lib.PCM_LINEAR and f.bits == 16 and not f.big_endian

    @property
    def fd(self) -> int:
        return self._fd

    @property
    def out_bytes_per_frame(self) -> int:
        return self.channels * (2 if self.is_s16 else 4)

    def byte_range(self, first: int, n: int) -> Tuple[int, int]:
        """File offsets [a, b): a is where the block holding `first` starts, b where the block holding first + n - 1 ends
        (or the data the file holds)."""
        f = self.fmt
        first = min(max(int(first), 0), self.frames)
        last = min(first + max(int(n), 1), self.frames)
        a = (first // f.samples_per_block) * f.block_align
        b = -(-last // f.samples_per_block) * f.block_align
        b = min(b, self.data_bytes)
        return self.data_off + a, self.data_off + max(a, b)

    def pieces(self, first: int, n: int) -> List[Tuple[int, int]]:
        """[first, first + n) as consecutive (first, n) pieces whose byte ranges hold whole blocks and at most PIECE_BYTES
        (one block when a block is larger)."""
        f = self.fmt
        per = max(1, PIECE_BYTES // f.block_align) * f.samples_per_block        # frames of a piece that starts on a block
        out, at, end = [], int(first), int(first) + int(n)
        while at < end:
            stop = min(end, (at // f.samples_per_block) * f.samples_per_block + per)
            out.append((at, stop - at))
            at = stop
        return out

    @property
    def header(self) -> "_lib.bd_pcm_format":
        """What the decode calls take as the stream's description."""
        return self.fmt

    def decode_host_into(self, first: int, n: int, out_ptr: Optional[int]) -> "_lib.bd_pcm_status":
        """Frames [first, first + n) decoded on the host to `out_ptr` (int16 or float32, interleaved); the status."""
        a, b = self.byte_range(first, n)
        data = np.frombuffer(self._pread(a, b - a), np.uint8)
        st = _lib.bd_pcm_status()
        _lib.check(_lib.load().bd_pcm_decode_host(data.ctypes.data if data.size else None, data.size, C.byref(self.fmt), first,
                                                  max(n, 0), out_ptr, C.byref(st)))
        return st

    def decode_host(self, first: int, n: int) -> Tuple[np.ndarray, "_lib.bd_pcm_status"]:
        """Frames [first, first + n) decoded on the host: ([got, channels] int16 or float32, status)."""
        out = np.zeros((max(n, 0), self.channels), np.int16 if self.is_s16 else np.float32)
        st = self.decode_host_into(first, n, out.ctypes.data if out.size else None)
        return out[: st.samples], st

    def __del__(self):
        self.close()

    def close(self) -> None:
        fd, self._fd = getattr(self, "_fd", None), None
        if fd is not None:
            os.close(fd)

