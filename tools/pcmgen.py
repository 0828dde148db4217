"""Fixture writer for pcmio's formats, NumPy and the standard library only: AIFF / AIFF-C (every compression type pcmio
reads), Sun AU, Wave64, RF64, and RIFF WAVE with mu-law, A-law, IMA ADPCM and MS ADPCM; plus the encoders behind them.

Encoders are vectorised over blocks and channels (one step per frame of a block), so hours of audio take seconds.  Any
valid ADPCM bitstream serves the tests (decoding is deterministic); these follow the usual encoder loops.
"""
from __future__ import annotations

import struct
from fractions import Fraction
from typing import Optional, Sequence, Tuple

import numpy as np

from tools.flacgen import test_signal  # noqa: F401  (re-exported: the signal the tests encode)

W64_TAIL = b"\xf3\xac\xd3\x11\x8c\xd1\x00\xc0\x4f\x8e\xdb\x8a"
W64_RIFF = b"riff\x2e\x91\xcf\x11\xa5\xd6\x28\xdb\x04\xc1\x00\x00"
MS_COEFS = (256, 0, 512, -256, 0, 0, 192, 64, 240, 0, 460, -208, 392, -232)    # the 7 pairs encoders usually write
IMA_STEPS = np.array([
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
    130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
    1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132,
    7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], np.int64)
IMA_INDEX = np.array([-1, -1, -1, -1, 2, 4, 6, 8] * 2, np.int64)
MS_ADAPT = np.array([230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230], np.int64)


def _2d(x) -> np.ndarray:
    x = np.asarray(x)
    return x[:, None] if x.ndim == 1 else x


# ---------------------------------------------------------------- sample encodings
def linear(pcm, width: int, big_endian: bool = False, signed: bool = True) -> bytes:
    """Integers (already in range for `width` bytes) -> interleaved stored samples."""
    x = _2d(pcm).astype(np.int64).reshape(-1)
    if not signed:
        x = x + (1 << (8 * width - 1))
    u = (x & ((1 << (8 * width)) - 1)).astype("<u8").view(np.uint8).reshape(-1, 8)[:, :width]
    return (u[:, ::-1] if big_endian else u).tobytes()


def floats(x, width: int, big_endian: bool = False) -> bytes:
    return _2d(x).astype((">" if big_endian else "<") + ("f4" if width == 4 else "f8")).tobytes()


def ulaw_table() -> np.ndarray:
    """The 256 mu-law codes expanded (G.711)."""
    u = ~np.arange(256) & 0xFF
    t = ((u & 0x0F) << 3) + 0x84
    t = t << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int64)


def alaw_table() -> np.ndarray:
    a = np.arange(256) ^ 0x55
    i = (a & 0x0F) << 4
    seg = (a & 0x70) >> 4
    t = np.where(seg == 0, i + 8, np.where(seg == 1, i + 0x108, (i + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(a & 0x80, t, -t).astype(np.int64)


def g711(pcm, law: str) -> bytes:
    """int16 samples -> the code whose expansion is nearest (ties: the lower value)."""
    table = ulaw_table() if law == "ulaw" else alaw_table()
    order = np.argsort(table, kind="stable")
    vals = table[order]
    x = _2d(pcm).astype(np.int64).reshape(-1)
    k = np.clip(np.searchsorted(vals, x), 1, 255)
    k = np.where(np.abs(vals[k - 1] - x) <= np.abs(vals[k] - x), k - 1, k)
    return order[k].astype(np.uint8).tobytes()


def ima_spb(block_align: int, ch: int) -> int:
    return (block_align - 4 * ch) * 2 // ch + 1


def ima_encode(pcm, block_align: int, index0: int = 0) -> Tuple[bytes, int]:
    """int16 [n, ch] -> (IMA ADPCM blocks in the WAVE layout, samples per block).  Every block's header holds its first
    sample and step index `index0`; the last block is padded with zero codes."""
    x = _2d(pcm).astype(np.int64)
    n, ch = x.shape
    spb = ima_spb(block_align, ch)
    nblk = -(-n // spb)
    xs = np.zeros((nblk * spb, ch), np.int64)
    xs[:n] = x
    xs = xs.reshape(nblk, spb, ch)
    pred = xs[:, 0, :].copy()
    index = np.full((nblk, ch), index0, np.int64)
    codes = np.zeros((nblk, spb - 1, ch), np.int64)
    for k in range(1, spb):
        step = IMA_STEPS[index]
        diff = xs[:, k, :] - pred
        sign = np.where(diff < 0, 8, 0)
        diff = np.abs(diff)
        code = np.zeros_like(diff)
        vp = step >> 3
        m = diff >= step
        code |= np.where(m, 4, 0); diff = np.where(m, diff - step, diff); vp = vp + np.where(m, step, 0)
        s1 = step >> 1
        m = diff >= s1
        code |= np.where(m, 2, 0); diff = np.where(m, diff - s1, diff); vp = vp + np.where(m, s1, 0)
        s2 = step >> 2
        m = diff >= s2
        code |= np.where(m, 1, 0); vp = vp + np.where(m, s2, 0)
        pred = np.clip(np.where(sign, pred - vp, pred + vp), -32768, 32767)
        code |= sign
        index = np.clip(index + IMA_INDEX[code], 0, 88)
        codes[:, k - 1, :] = code
    out = np.zeros((nblk, block_align), np.uint8)
    h = out[:, : 4 * ch].reshape(nblk, ch, 4)
    p0 = xs[:, 0, :].astype("<i2").view(np.uint8).reshape(nblk, ch, 2)
    h[:, :, 0:2] = p0
    h[:, :, 2] = index0
    # codes: groups of 8 frames, one 4-byte word per channel per group, low nibble first
    groups = (spb - 1) // 8
    c = codes[:, : groups * 8, :].reshape(nblk, groups, 8, ch).transpose(0, 1, 3, 2)      # [blk, group, ch, 8]
    byte = (c[..., 0::2] | (c[..., 1::2] << 4)).astype(np.uint8)                             # [blk, group, ch, 4]
    out[:, 4 * ch: 4 * ch + groups * ch * 4] = byte.reshape(nblk, -1)
    return out.tobytes(), spb


def ms_spb(block_align: int, ch: int) -> int:
    return (block_align - 7 * ch) * 2 // ch + 2


def ms_encode(pcm, block_align: int, coefs: Sequence[int] = MS_COEFS) -> Tuple[bytes, int]:
    """int16 [n, ch] -> (MS ADPCM blocks, samples per block).  Block b uses predictor b % len(coefs) // 2 in every channel;
    the last block is padded with zero samples."""
    x = _2d(pcm).astype(np.int64)
    n, ch = x.shape
    spb = ms_spb(block_align, ch)
    nblk = -(-n // spb)
    xs = np.zeros((nblk * spb, ch), np.int64)
    xs[:n] = x
    xs = xs.reshape(nblk, spb, ch)
    cf = np.asarray(coefs, np.int64).reshape(-1, 2)
    p = np.repeat((np.arange(nblk) % len(cf))[:, None], ch, 1)
    c1, c2 = cf[p, 0], cf[p, 1]
    s2, s1 = xs[:, 0, :].copy(), xs[:, 1, :].copy()
    delta0 = np.maximum(16, np.abs(xs[:, 2, :] - xs[:, 1, :]) // 4) if spb > 2 else np.full((nblk, ch), 16)
    delta0 = np.minimum(delta0, 32767)
    delta = delta0.copy()
    nibs = np.zeros((nblk, spb - 2, ch), np.int64)
    for k in range(2, spb):
        predict = (s1 * c1 + s2 * c2) >> 8
        code = np.clip(np.round((xs[:, k, :] - predict) / delta), -8, 7).astype(np.int64)
        v = np.clip(predict + code * delta, -32768, 32767)
        s2, s1 = s1, v
        nib = code & 15
        delta = np.maximum(16, (MS_ADAPT[nib] * delta) >> 8)
        nibs[:, k - 2, :] = nib
    out = np.zeros((nblk, block_align), np.uint8)
    out[:, :ch] = p
    out[:, ch: 3 * ch] = delta0.astype("<i2").view(np.uint8).reshape(nblk, 2 * ch)
    out[:, 3 * ch: 5 * ch] = xs[:, 1, :].astype("<i2").view(np.uint8).reshape(nblk, 2 * ch)
    out[:, 5 * ch: 7 * ch] = xs[:, 0, :].astype("<i2").view(np.uint8).reshape(nblk, 2 * ch)
    flat = nibs.reshape(nblk, -1)                                                           # interleaved by channel
    if flat.shape[1] % 2:
        flat = np.concatenate([flat, np.zeros((nblk, 1), np.int64)], 1)
    body = ((flat[:, 0::2] << 4) | flat[:, 1::2]).astype(np.uint8)
    out[:, 7 * ch: 7 * ch + body.shape[1]] = body
    return out.tobytes(), spb


def random_adpcm(kind: str, nblk: int, block_align: int, ch: int, seed: int = 0, n_coefs: int = 7) -> bytes:
    """nblk blocks of random codes with valid headers (every code sequence is a valid ADPCM stream): for long ranges."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (nblk, block_align), dtype=np.uint8)
    if kind == "ima":
        h = out[:, : 4 * ch].reshape(nblk, ch, 4)
        h[:, :, 2] = rng.integers(0, 89, (nblk, ch))
        h[:, :, 3] = 0
    else:
        out[:, :ch] = rng.integers(0, n_coefs, (nblk, ch))
        d = rng.integers(16, 2048, (nblk, ch)).astype("<i2").view(np.uint8).reshape(nblk, 2 * ch)
        out[:, ch: 3 * ch] = d
    return out.tobytes()


# ---------------------------------------------------------------- containers
def extended(rate) -> bytes:
    """A positive rate as the 80-bit IEEE extended float of AIFF's COMM chunk (rounded to 64 mantissa bits)."""
    r = Fraction(rate)
    e = r.numerator.bit_length() - r.denominator.bit_length()
    while Fraction(2) ** e > r:
        e -= 1
    while Fraction(2) ** (e + 1) <= r:
        e += 1
    mant = round(r * Fraction(2) ** (63 - e))
    return struct.pack(">HQ", 16383 + e, mant)


def aiff(data: bytes, rate, ch: int, frames: int, bits: int, compression: Optional[bytes] = None, ssnd_offset: int = 0,
         odd_chunk: bool = False, declared: Optional[int] = None) -> bytes:
    """AIFF (compression None) or AIFF-C holding `data` as SSND, `ssnd_offset` zero bytes before it; `odd_chunk` puts a
    chunk of odd length (and its pad byte) between COMM and SSND; `declared` overrides numSampleFrames."""
    nf = frames if declared is None else declared
    comm = struct.pack(">hIh", ch, nf, bits) + extended(rate)
    form = b"AIFF"
    chunks = b""
    if compression is not None:
        form = b"AIFC"
        chunks += b"FVER" + struct.pack(">I", 4) + struct.pack(">I", 0xA2805140)
        name = b"\x03abc"
        comm += compression + name
    chunks += b"COMM" + struct.pack(">I", len(comm)) + comm + (b"\0" if len(comm) & 1 else b"")
    if odd_chunk:
        chunks += b"ANNO" + struct.pack(">I", 5) + b"hello" + b"\0"
    ssnd = struct.pack(">II", ssnd_offset, 0) + b"\0" * ssnd_offset + data
    chunks += b"SSND" + struct.pack(">I", len(ssnd)) + ssnd + (b"\0" if len(ssnd) & 1 else b"")
    return b"FORM" + struct.pack(">I", 4 + len(chunks)) + form + chunks


def au(data: bytes, rate: int, ch: int, encoding: int, unknown_size: bool = False, annotation: bytes = b"\0" * 8) -> bytes:
    off = 24 + len(annotation)
    size = 0xFFFFFFFF if unknown_size else len(data)
    return b".snd" + struct.pack(">IIIII", off, size, encoding, rate, ch) + annotation + data


def fmt_body(tag: int, ch: int, rate: int, bits: int, block_align: int, ext: Optional[bytes] = None) -> bytes:
    body = struct.pack("<HHIIHH", tag, ch, rate, rate * block_align, block_align, bits)
    if ext is not None:
        body += struct.pack("<H", len(ext)) + ext
    return body


def fmt_ima(ch: int, rate: int, block_align: int, spb: int) -> bytes:
    return fmt_body(0x11, ch, rate, 4, block_align, struct.pack("<H", spb))


def fmt_ms(ch: int, rate: int, block_align: int, spb: int, coefs: Sequence[int] = MS_COEFS) -> bytes:
    return fmt_body(2, ch, rate, 4, block_align, struct.pack("<HH", spb, len(coefs) // 2) + struct.pack(f"<{len(coefs)}h", *coefs))


def wave(fmt: bytes, data: bytes, fact: Optional[int] = None, rf64: bool = False, data_size: Optional[int] = None) -> bytes:
    """RIFF (or RF64, sizes 0xFFFFFFFF and a ds64 chunk) WAVE; `data_size` overrides the data chunk's size field."""
    body = b"fmt " + struct.pack("<I", len(fmt)) + fmt + (b"\0" if len(fmt) & 1 else b"")
    if fact is not None:
        body += b"fact" + struct.pack("<II", 4, fact)
    size = len(data) if data_size is None else data_size
    if rf64:
        ds64 = struct.pack("<QQQI", 4 + 36 + len(body) + 8 + len(data), len(data), fact or 0, 0)
        body = b"ds64" + struct.pack("<I", len(ds64)) + ds64 + body
        size = 0xFFFFFFFF
    body += b"data" + struct.pack("<I", size) + data
    return (b"RF64" + struct.pack("<I", 0xFFFFFFFF) if rf64 else b"RIFF" + struct.pack("<I", 4 + len(body))) + b"WAVE" + body


def w64(fmt: bytes, data: bytes, fact: Optional[int] = None) -> bytes:
    def chunk(name: bytes, body: bytes) -> bytes:
        raw = name + W64_TAIL + struct.pack("<Q", 24 + len(body)) + body
        return raw + b"\0" * (-len(raw) % 8)
    body = chunk(b"fmt ", fmt)
    if fact is not None:
        body += chunk(b"fact", struct.pack("<Q", fact))
    body += chunk(b"data", data)
    return W64_RIFF + struct.pack("<Q", 40 + len(body)) + b"wave" + W64_TAIL + body


def wav16(pcm, rate: int) -> bytes:
    """int16 samples as a 16-bit PCM WAV."""
    x = _2d(pcm)
    return wave(fmt_body(1, x.shape[1], rate, 16, 2 * x.shape[1]), x.astype("<i2").tobytes())


def wav_f32(x, rate: int) -> bytes:
    """float32 samples as an IEEE float WAV."""
    x = _2d(x)
    return wave(fmt_body(3, x.shape[1], rate, 32, 4 * x.shape[1]), x.astype("<f4").tobytes())
