"""FLAC stream writer for test fixtures: NumPy only, written from the format (RFC 9639).

Not an encoder for use: it spends no effort on compression.  It emits every feature the decoder must handle, on
demand: subframe types (CONSTANT, VERBATIM, FIXED 0-4, LPC 1-32 with chosen precision / shift), wasted bits, Rice /
Rice2 / escaped partitions (escape width 0 included) at partition orders 0-8, the four channel assignments, fixed and
variable blocking, every block-size and sample-rate header encoding, and SEEKTABLE / VORBIS_COMMENT / PADDING blocks
and an ID3v2 tag in front.

    data = encode(pcm, rate, bps, blocksize=4096, subframe=("lpc", 8), ...)      # pcm: int [n, channels]
"""
from __future__ import annotations

import struct
from typing import Optional, Sequence

import numpy as np

_G16 = 0x18005


def crc8(data: bytes) -> int:
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


def _crc16_table() -> np.ndarray:
    t = np.zeros(256, np.uint32)
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
        t[i] = c
    return t


_T16 = _crc16_table()
_XPOW = [1]                       # x^(8k) mod G, k = 0, 1, ...


def _mulmod(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Products of 16-bit polynomials modulo the CRC-16 polynomial, elementwise."""
    a = a.astype(np.uint64)
    b = b.astype(np.uint64)
    r = np.zeros(np.broadcast(a, b).shape, np.uint64)
    for j in range(16):
        r ^= ((b >> np.uint64(j)) & np.uint64(1)) * (a << np.uint64(j))
    for j in range(30, 15, -1):
        r ^= ((r >> np.uint64(j)) & np.uint64(1)) * np.uint64(_G16 << (j - 16))
    return r.astype(np.uint32)


def _xpow(k: int) -> np.ndarray:
    while len(_XPOW) <= k:
        v = _XPOW[-1] << 8
        for j in range(23, 15, -1):
            if v >> j & 1:
                v ^= _G16 << (j - 16)
        _XPOW.append(v)
    return np.asarray(_XPOW[: k + 1], np.uint32)


def crc16(data: bytes) -> int:
    """CRC-16 (poly 0x8005, init 0): the XOR over the bytes of table[b] * x^(8 * bytes after it), all at once."""
    b = np.frombuffer(bytes(data), np.uint8)
    if b.size == 0:
        return 0
    pw = _xpow(b.size - 1)[::-1]
    return int(np.bitwise_xor.reduce(_mulmod(_T16[b], pw)))


def crc16_concat(crc_a: int, crc_b: int, len_b: int) -> int:
    """CRC-16 of a || b from the CRCs of both parts."""
    return int(_mulmod(np.uint32(crc_a), _xpow(len_b)[len_b])) ^ crc_b


# ------------------------------------------------------------------ bit packing
class Fields:
    """(value, width) pairs, MSB first; packed at once."""

    def __init__(self):
        self.v: list = []
        self.w: list = []

    def add(self, value: int, width: int) -> None:
        if width:
            self.v.append(np.asarray([value & ((1 << width) - 1)], np.uint64))
            self.w.append(np.asarray([width], np.int64))

    def add_signed(self, values, width: int) -> None:
        values = np.asarray(values, np.int64).reshape(-1)
        if width == 0 or values.size == 0:
            return
        self.v.append((values & ((1 << width) - 1)).astype(np.uint64))
        self.w.append(np.full(values.size, width, np.int64))

    def add_array(self, values: np.ndarray, widths: np.ndarray) -> None:
        self.v.append(values.astype(np.uint64))
        self.w.append(widths.astype(np.int64))

    def pack(self) -> bytes:
        """Bytes, zero-padded to a byte boundary.  Every width is <= 57."""
        if not self.v:
            return b""
        v = np.concatenate(self.v)
        w = np.concatenate(self.w)
        keep = w > 0
        v, w = v[keep], w[keep]
        assert w.max() <= 57
        end = np.cumsum(w)
        pos = end - w
        total = int(end[-1])
        nbytes = (total + 7) // 8
        shifted = v << (64 - (pos & 7) - w).astype(np.uint64)
        first = pos >> 3
        out = np.zeros(nbytes + 8, np.float64)
        for lane in range(8):
            byte = ((shifted >> np.uint64(56 - 8 * lane)) & np.uint64(0xFF)).astype(np.float64)
            out += np.bincount(first + lane, weights=byte, minlength=nbytes + 8)[: nbytes + 8]
        return out[:nbytes].astype(np.uint8).tobytes()


def _utf8(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    for n in range(2, 8):
        if v < 1 << (5 * n + 1):
            break
    out = []
    for _ in range(n - 1):
        out.append(0x80 | (v & 0x3F))
        v >>= 6
    lead = (0xFF << (8 - n)) & 0xFF if n < 7 else 0xFE
    return bytes([lead | v] + out[::-1])


# ------------------------------------------------------------------ residuals and subframes
def _residual(f: Fields, res: np.ndarray, bs: int, order: int, method: str, porder: Optional[int]) -> None:
    """Residual section: method "rice", "rice2", "escape" (raw width from the data) or "escape0" (width 0: all zero)."""
    if porder is None:
        porder = 0
        while porder < 8 and bs % (2 << porder) == 0 and (bs >> (porder + 1)) >= order and (bs >> (porder + 1)) >= 64:
            porder += 1
    while porder > 0 and (bs % (1 << porder) or (bs >> porder) < order):     # (a shorter last block)
        porder -= 1
    rice2 = method == "rice2"
    f.add(1 if rice2 else 0, 2)
    f.add(porder, 4)
    pbits, esc = (5, 31) if rice2 else (4, 15)
    per = bs >> porder
    at = 0
    for p in range(1 << porder):
        r = res[at: at + (per - order if p == 0 else per)]
        at += r.size
        if method in ("escape", "escape0"):
            width = 0 if not np.any(r) else int(max(int(r.max()), int(-r.min()) - 1)).bit_length() + 1
            assert method == "escape" or width == 0
            f.add(esc, pbits)
            f.add(width, 5)
            f.add_signed(r, width)
            continue
        u = ((r << 1) ^ (r >> 63)).astype(np.uint64)           # zigzag
        mean = float(u.mean()) if u.size else 0.0
        k = max(0, min(int(np.log2(mean + 1)), esc - 1))
        q = u >> np.uint64(k)
        f.add(k, pbits)
        if u.size == 0:
            continue
        long = q + np.uint64(1 + k) > np.uint64(57)
        if np.any(long):                                        # (rare) a zero run split into pieces
            for uu in u:
                qq = int(uu) >> k
                while qq + 1 + k > 57:
                    f.add(0, 56)
                    qq -= 56
                f.add((1 << k) | (int(uu) & ((1 << k) - 1)), qq + 1 + k)
        else:
            f.add_array((np.uint64(1) << np.uint64(k)) | (u & np.uint64((1 << k) - 1)), (q + np.uint64(1 + k)).astype(np.int64))


FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def _predict(x: np.ndarray, coefs: Sequence[int], shift: int) -> np.ndarray:
    order = len(coefs)
    acc = np.zeros(x.size - order, np.int64)
    for j, c in enumerate(coefs):
        acc += int(c) * x[order - 1 - j: x.size - 1 - j]
    return x[order:] - (acc >> shift)


def _lpc_coefs(x: np.ndarray, order: int, precision: int, shift: Optional[int]):
    xf = x.astype(np.float64)
    n = xf.size
    if n > order:
        a = np.stack([xf[order - 1 - j: n - 1 - j] for j in range(order)], 1)
        c, *_ = np.linalg.lstsq(a, xf[order:], rcond=None)
    else:
        c = np.zeros(order)
    lim = (1 << (precision - 1)) - 1
    if shift is None:
        m = float(np.abs(c).max()) if order else 0.0
        shift = precision - 1 - (max(0, int(np.ceil(np.log2(m + 1e-9)))) if m > 0 else 0) - 1
        shift = max(0, min(15, shift))
    q = np.clip(np.round(c * (1 << shift)), -lim - 1, lim).astype(np.int64)
    return [int(v) for v in q], shift


def subframe(f: Fields, x: np.ndarray, sbps: int, kind, method: str = "rice", porder: Optional[int] = None,
             wasted: bool = False) -> None:
    """One subframe.  kind: "constant", "verbatim", ("fixed", order), ("lpc", order[, precision[, shift]])."""
    x = np.asarray(x, np.int64)
    bs = x.size
    w = 0
    if wasted and np.any(x):
        nz = x[x != 0]
        while w < sbps - 1 and np.all((nz >> w) & 1 == 0):
            w += 1
    xs = x >> w
    eb = sbps - w
    name = kind if isinstance(kind, str) else kind[0]
    if name == "constant":
        assert np.all(x == x[0])
        t = 0
    elif name == "verbatim":
        t = 1
    elif name == "fixed":
        t = 0b001000 | kind[1]
    else:
        t = 0b100000 | (kind[1] - 1)
    f.add((t << 1) | (1 if w else 0), 8)                        # zero pad bit, type, wasted-bits flag
    if w:
        f.add(1, w)                                            # unary w - 1: w - 1 zeros and a one
    if name == "constant":
        f.add_signed([xs[0]], eb)
    elif name == "verbatim":
        f.add_signed(xs, eb)
    elif name == "fixed":
        order = kind[1]
        f.add_signed(xs[:order], eb)
        _residual(f, _predict(xs, FIXED[order], 0), bs, order, method, porder)
    else:
        order = kind[1]
        precision = kind[2] if len(kind) > 2 else 15
        coefs, shift = _lpc_coefs(xs, order, precision, kind[3] if len(kind) > 3 else None)
        f.add_signed(xs[:order], eb)
        f.add(precision - 1, 4)
        f.add(shift, 5)
        f.add_signed(coefs, precision)
        _residual(f, _predict(xs, coefs, shift), bs, order, method, porder)


# ------------------------------------------------------------------ frames
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
BPS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}
MODES = {"independent": None, "left_side": 8, "side_right": 9, "mid_side": 10}


def frame_header(number: int, bs: int, rate: int, assign: int, bps: int, variable: bool, bs_tail: Optional[int] = None,
                 rate_code: Optional[str] = None, bps_in_header: bool = True) -> bytes:
    """bs_tail 8 / 16: the block size as an 8- / 16-bit tail even when a code exists.  rate_code: None (table code when one
    exists, else the smallest tail), "streaminfo", "khz", "hz", "tens"."""
    tail = b""
    if bs_tail is None and bs == 192:
        c = 1
    elif bs_tail is None and bs in (576, 1152, 2304, 4608):
        c = 2 + [576, 1152, 2304, 4608].index(bs)
    elif bs_tail is None and bs in [256 << k for k in range(8)]:
        c = 8 + [256 << k for k in range(8)].index(bs)
    elif (bs_tail or 8) == 8 and bs <= 256:
        c, tail = 6, bytes([bs - 1])
    else:
        c, tail = 7, struct.pack(">H", bs - 1)
    if rate_code is None:
        rate_code = "table" if rate in RATE_CODES else ("khz" if rate % 1000 == 0 and rate // 1000 < 256 else
                                                        "hz" if rate < 65536 else "tens")
    rtail = b""
    if rate_code == "streaminfo":
        rc = 0
    elif rate_code == "table":
        rc = RATE_CODES[rate]
    elif rate_code == "khz":
        rc, rtail = 12, bytes([rate // 1000])
    elif rate_code == "hz":
        rc, rtail = 13, struct.pack(">H", rate)
    else:
        rc, rtail = 14, struct.pack(">H", rate // 10)
    bc = BPS_CODES.get(bps, 0) if bps_in_header else 0
    h = struct.pack(">H", 0xFFF8 | int(variable)) + bytes([(c << 4) | rc, (assign << 4) | (bc << 1)]) + _utf8(number) + tail + rtail
    return h + bytes([crc8(h)])


def frame_body(pcm: np.ndarray, bps: int, mode: str, kinds, method: str, porder: Optional[int], wasted: bool):
    """Subframes of one block ([bs, channels] int): (body bytes, its CRC-16, channel assignment)."""
    ch = pcm.shape[1]
    assign = MODES[mode]
    x = pcm.astype(np.int64)
    if assign is None:
        assign = ch - 1
        chans, bpss = [x[:, c] for c in range(ch)], [bps] * ch
    else:
        assert ch == 2
        left, right = x[:, 0], x[:, 1]
        side = left - right
        if assign == 8:
            chans, bpss = [left, side], [bps, bps + 1]
        elif assign == 9:
            chans, bpss = [side, right], [bps + 1, bps]
        else:
            chans, bpss = [(left + right) >> 1, side], [bps, bps + 1]
    f = Fields()
    for c, (s, b) in enumerate(zip(chans, bpss)):
        kind = kinds(c) if callable(kinds) else kinds
        if kind == "constant" and not np.all(s == s[0]):
            kind = "verbatim"
        subframe(f, s, b, kind, method, porder, wasted)
    body = f.pack()
    return body, crc16(body), assign


def streaminfo_block(min_bs, max_bs, min_fs, max_fs, rate, ch, bps, total, last) -> bytes:
    v = (rate << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | total
    data = struct.pack(">HH", min_bs, max_bs) + min_fs.to_bytes(3, "big") + max_fs.to_bytes(3, "big") + v.to_bytes(8, "big") + bytes(16)
    return bytes([0x80 * last | 0]) + len(data).to_bytes(3, "big") + data


def encode(pcm, rate: int, bps: int, blocksize=4096, variable: bool = False, mode: str = "independent",
           subframe_kind=("lpc", 8), method: str = "rice", porder: Optional[int] = None, wasted: bool = False,
           bs_tail: Optional[int] = None, rate_code: Optional[str] = None, bps_in_header: bool = True,
           seektable: Optional[int] = None, vorbis: bool = False, padding: int = 0, id3: bool = False,
           total_unknown: bool = False, return_offsets: bool = False):
    """``pcm``: int [n, channels] (or [n]) of ``bps``-bit samples.  ``blocksize``: an int, or (variable blocking) a
    sequence of block sizes used in turn.  ``subframe_kind``: a kind for every subframe, or a callable
    (frame index, channel) -> kind.  ``seektable``: a seek point every that many samples.  With ``return_offsets`` the
    result is (bytes, [(first sample, frame byte offset, frame end)])."""
    x = np.asarray(pcm)
    if x.ndim == 1:
        x = x[:, None]
    n, ch = x.shape
    sizes = [blocksize] if np.isscalar(blocksize) else list(blocksize)
    frames, at, k = [], 0, 0
    cache = {}
    while at < n:
        bs = min(sizes[k % len(sizes)], n - at)
        kinds = (lambda c, k=k: subframe_kind(k, c)) if callable(subframe_kind) else subframe_kind
        block = x[at: at + bs].astype(np.int64)
        key = None if callable(subframe_kind) else block.tobytes()
        if key is not None and key in cache:
            body, bcrc, assign = cache[key]
        else:
            body, bcrc, assign = frame_body(block, bps, mode, kinds, method, porder, wasted)
            if key is not None and len(cache) < 4096:
                cache[key] = (body, bcrc, assign)
        number = at if variable else k
        head = frame_header(number, bs, rate, assign, bps, variable, bs_tail, rate_code, bps_in_header)
        crc = crc16_concat(crc16(head), bcrc, len(body))
        frames.append((at, head + body + struct.pack(">H", crc)))
        at += bs
        k += 1
    fixed_bs = sizes[0]
    min_bs = min(sizes) if variable else fixed_bs
    max_bs = max(sizes) if variable else fixed_bs
    fsz = [len(fr) for _, fr in frames]
    blocks = []
    if seektable:
        pts, off = [], 0
        next_pt = 0
        for (s, fr) in frames:
            if s >= next_pt:
                pts.append(struct.pack(">QQH", s, off, 0))
                next_pt = (s // seektable + 1) * seektable
            off += len(fr)
        blocks.append((3, b"".join(pts)))
    if vorbis:
        vendor = b"flacgen"
        blocks.append((4, struct.pack("<I", len(vendor)) + vendor + struct.pack("<I", 1) + struct.pack("<I", 9) + b"TITLE=bee"))
    if padding:
        blocks.append((1, bytes(padding)))
    out = bytearray()
    if id3:
        tag = bytes(20)
        size = len(tag)
        out += b"ID3\x04\x00\x00" + bytes([(size >> 21) & 0x7F, (size >> 14) & 0x7F, (size >> 7) & 0x7F, size & 0x7F]) + tag
    out += b"fLaC"
    out += streaminfo_block(min_bs, max_bs, min(fsz) if fsz else 0, max(fsz) if fsz else 0, rate, ch, bps,
                            0 if total_unknown else n, not blocks)
    for i, (t, data) in enumerate(blocks):
        out += bytes([0x80 * (i == len(blocks) - 1) | t]) + len(data).to_bytes(3, "big") + data
    offsets = []
    for s, fr in frames:
        offsets.append((s, len(out), len(out) + len(fr)))
        out += fr
    return (bytes(out), offsets) if return_offsets else bytes(out)


def wav_bytes(pcm, rate: int, bps: int) -> bytes:
    """The same samples as a PCM WAV (8-bit unsigned, 16 / 24-bit signed little-endian)."""
    x = np.asarray(pcm, np.int64)
    if x.ndim == 1:
        x = x[:, None]
    ch = x.shape[1]
    if bps == 8:
        data = (x + 128).astype(np.uint8).tobytes()
    elif bps == 16:
        data = x.astype("<i2").tobytes()
    elif bps == 24:
        u = (x & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]
        data = u.tobytes()
    else:
        raise ValueError("wav_bytes: 8, 16 or 24 bits")
    width = (bps + 7) // 8
    fmt = struct.pack("<HHIIHH", 1, ch, rate, rate * ch * width, ch * width, width * 8)
    return b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + \
        b"data" + struct.pack("<I", len(data)) + data


def test_signal(n: int, channels: int, bps: int, seed: int = 0) -> np.ndarray:
    """Band-limited noise plus tones at about half scale: predictable enough that LPC residuals stay small."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    out = np.empty((n, channels), np.int64)
    amp = (1 << (bps - 1)) - 1
    for c in range(channels):
        noise = np.convolve(rng.standard_normal(n + 16), np.hanning(16) / 8, "same")[:n]
        s = 0.3 * np.sin(2 * np.pi * t * (0.01 + 0.003 * c)) + 0.1 * noise + 0.05 * np.sin(2 * np.pi * t * 0.13)
        out[:, c] = np.clip(np.round(s * amp), -amp - 1, amp)
    return out
