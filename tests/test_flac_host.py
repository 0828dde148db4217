"""FLAC on the host: checksums, the host decoder (the same parse / decode code the device runs) against source PCM over
the format's feature matrix, the locator of flacio.FlacTrack, truncated files, refused bit depths.  No device needed."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from buzzdetect_amd import _lib
from tools import flacgen as G


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def host_decode(lib, data: bytes, si, first: int, n: int):
    buf = np.frombuffer(data, np.uint8)
    out = np.zeros((n, si.channels), np.int16 if si.bits_per_sample == 16 else np.float32)
    st = _lib.bd_flac_status()
    _lib.check(lib.bd_flac_decode_host(buf.ctypes.data if buf.size else None, buf.size, C.byref(si), first, n,
                                       out.ctypes.data if out.size else None, C.byref(st)))
    return out, st


def expected(pcm: np.ndarray, bps: int) -> np.ndarray:
    return pcm.astype(np.int16) if bps == 16 else (pcm.astype(np.float64) / (1 << (bps - 1))).astype(np.float32)


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_crc_known_answers(lib):
    assert lib.bd_flac_crc8(b"123456789", 9) == 0xF4
    assert lib.bd_flac_crc16(b"123456789", 9) == 0xFEE8
    assert G.crc8(b"123456789") == 0xF4 and G.crc16(b"123456789") == 0xFEE8


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value: int, width: int):
        self.bits += [(value >> (width - 1 - k)) & 1 for k in range(width)]

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def bytes(self) -> bytes:
        self.align()
        return bytes(int("".join(map(str, self.bits[i:i + 8])), 2) for i in range(0, len(self.bits), 8))


def test_hand_assembled_stream(lib, tmp_path):
    """One frame written field by field: mono 16-bit, 16 samples (8-bit block-size tail), FIXED order 2, Rice parameter 2,
    partition order 1.  x[0] = 100, x[1] = 103, residuals r = 1, -1, 0, 2, ... -> x[i] = 2 x[i-1] - x[i-2] + r[i]."""
    res = [1, -1, 0, 2, -2, 3, 0, 0, 1, -1, 0, 0, 1, 1]
    x = [100, 103]
    for r in res:
        x.append(2 * x[-1] - x[-2] + r)
    w = BitWriter()
    w.put(0xFFF8, 16)                  # sync, reserved 0, fixed blocking
    w.put(6, 4)                        # block size: 8-bit tail
    w.put(5, 4)                        # 16 kHz
    w.put(0, 4)                        # one channel
    w.put(4, 3)                        # 16 bits
    w.put(0, 1)
    w.put(0, 8)                        # frame number 0
    w.put(15, 8)                       # block size - 1
    head = w.bytes()
    w.put(G.crc8(head), 8)
    w.put(0, 1)                        # subframe: pad, FIXED order 2 (0b001010), no wasted bits
    w.put(0b001010, 6)
    w.put(0, 1)
    w.put(100, 16)                     # warm-up
    w.put(103, 16)
    w.put(0, 2)                        # Rice, 4-bit parameters
    w.put(1, 4)                        # partition order 1: 8 - 2 and 8 residuals
    for p, part in enumerate((res[:6], res[6:])):
        w.put(2, 4)
        for r in part:
            u = 2 * r if r >= 0 else -2 * r - 1
            w.put(0, u >> 2)
            w.put(1, 1)
            w.put(u & 3, 2)
    frame = w.bytes()
    frame += struct.pack(">H", G.crc16(frame))
    si = _lib.bd_flac_streaminfo(16, 16, 16000, 1, 16, 0, 16)
    out, st = host_decode(lib, frame, si, 0, 16)
    assert (st.reason, st.samples, st.frames, st.stop_offset) == (0, 16, 1, len(frame))
    assert out[:, 0].tolist() == x


MATRIX = [
    # bps, channels, block sizes, variable, mode, subframe kind, method, partition order, wasted, header options
    (16, 1, 4096, False, "independent", ("lpc", 8), "rice", None, False, {}),
    (16, 2, 4608, False, "mid_side", ("lpc", 12, 15), "rice2", 3, False, {}),
    (16, 2, 1152, False, "left_side", ("fixed", 2), "rice", 0, False, {"bs_tail": 16}),
    (16, 2, 576, False, "side_right", ("fixed", 3), "escape", 2, False, {}),
    (8, 1, 192, False, "independent", ("fixed", 1), "rice", 1, False, {"rate_code": "khz"}),
    (12, 3, 256, False, "independent", ("lpc", 4, 10, 6), "rice", 6, False, {"rate_code": "hz"}),
    (20, 6, 2048, False, "independent", ("lpc", 32, 15), "rice2", 2, False, {"rate_code": "tens"}),
    (24, 2, [4096, 1000, 65535, 16, 333], True, "mid_side", ("lpc", 16, 14), "rice", 0, False, {}),
    (24, 1, 8192, False, "independent", ("fixed", 4), "rice2", 8, True, {"bps_in_header": False, "rate_code": "streaminfo"}),
    (16, 1, 4096, False, "independent", ("fixed", 0), "rice", 4, True, {}),
    (16, 2, 300, True, "independent", "verbatim", "rice", None, True, {"bs_tail": 16}),
    (12, 1, 1024, False, "independent", ("lpc", 1, 8, 3), "rice", 5, False, {}),
    (16, 1, 4096, False, "independent", ("lpc", 2, 5, 0), "rice", 0, False, {}),
]


@pytest.mark.parametrize("case", range(len(MATRIX)))
def test_host_decoder_round_trip(lib, case):
    bps, ch, bs, variable, mode, kind, method, po, wasted, opts = MATRIX[case]
    n = 70_000 if np.isscalar(bs) else 80_000
    pcm = G.test_signal(n, ch, bps, seed=case)
    if wasted:
        pcm = (pcm >> 3) << 3
    data, offs = G.encode(pcm, 44100 if "tens" in str(opts) else 48000, bps, blocksize=bs, variable=variable, mode=mode,
                          subframe_kind=kind, method=method, porder=po, wasted=wasted, return_offsets=True, **opts)
    sizes = [bs] if np.isscalar(bs) else bs
    si = _lib.bd_flac_streaminfo(min(sizes), max(sizes), 44100 if "tens" in str(opts) else 48000, ch, bps, 0, n)
    body = data[offs[0][1]:]
    out, st = host_decode(lib, body, si, 0, n)
    assert (st.reason, st.samples, st.frames) == (0, n, len(offs))
    np.testing.assert_array_equal(out, expected(pcm, bps))
    # a window that starts and ends inside frames, from a range that starts on the frame holding its first sample
    rng = np.random.default_rng(case)
    for _ in range(3):
        a = int(rng.integers(0, n - 1))
        m = int(rng.integers(1, n - a + 1))
        k = max(i for i, (s, _, _) in enumerate(offs) if s <= a)
        e = max(i for i, (s, _, _) in enumerate(offs) if s <= a + m - 1)
        seg = data[offs[k][1]: offs[e][2]]
        out, st = host_decode(lib, seg, si, a, m)
        assert st.samples == m and st.reason == 0 and st.first_sample == offs[k][0]
        np.testing.assert_array_equal(out, expected(pcm[a:a + m], bps))


def test_constant_and_escape_width_zero(lib):
    pcm = np.zeros((8192, 2), np.int64)
    pcm[:4096] = 1234
    pcm[4096:, 1] = np.arange(4096)                 # a ramp: FIXED order 2 leaves all-zero residuals
    kinds = lambda k, c: "constant" if k == 0 else ("fixed", 2)
    data, offs = G.encode(pcm, 16000, 16, blocksize=4096, subframe_kind=kinds, method="escape0", return_offsets=True)
    si = _lib.bd_flac_streaminfo(4096, 4096, 16000, 2, 16, 0, 8192)
    out, st = host_decode(lib, data[offs[0][1]:], si, 0, 8192)
    assert st.samples == 8192
    np.testing.assert_array_equal(out, pcm.astype(np.int16))


@pytest.mark.parametrize("seek,variable,unknown", [(None, False, False), (48000, False, False), (None, True, False),
                                                   (30000, True, True), (None, False, True)])
def test_byte_range_covers_exactly_the_needed_frames(tmp_path, seek, variable, unknown):
    from buzzdetect_amd.flacio import FlacTrack
    n = 600_000
    pcm = G.test_signal(n, 1, 16, seed=7)
    bs = [4096, 1024, 2500] if variable else 4096
    data, offs = G.encode(pcm, 48000, 16, blocksize=bs, variable=variable, subframe_kind=("fixed", 2), seektable=seek,
                          vorbis=True, padding=100, id3=bool(seek), total_unknown=unknown, return_offsets=True)
    t = FlacTrack(write(tmp_path, "x.flac", data))
    assert t.frames == n and t.frames_declared == n and t.samplerate == 48000 and t.is_s16
    starts = [s for s, _, _ in offs]
    rng = np.random.default_rng(1)
    for a, m in [(0, 1), (0, n), (n - 1, 1)] + [(int(x), int(y)) for x, y in zip(rng.integers(0, n - 1, 12), rng.integers(1, 200_000, 12))]:
        m = min(m, n - a)
        k = int(np.searchsorted(starts, a, "right")) - 1
        e = int(np.searchsorted(starts, a + m - 1, "right")) - 1
        assert t.byte_range(a, m) == (offs[k][1], offs[e][2]), (a, m)
    out, st = t.decode_host(123_456, 100_000)
    np.testing.assert_array_equal(out, pcm[123_456:223_456].astype(np.int16))
    t.close()


def test_truncated_file_reads_to_its_last_complete_frame(tmp_path):
    from buzzdetect_amd.flacio import FlacTrack
    n = 200_000
    pcm = G.test_signal(n, 2, 16, seed=2)
    data, offs = G.encode(pcm, 16000, 16, blocksize=4096, mode="mid_side", return_offsets=True)
    cut = (offs[20][1] + offs[20][2]) // 2                 # inside frame 20
    t = FlacTrack(write(tmp_path, "cut.flac", data[:cut]))
    assert t.frames == offs[20][0] and t.frames_declared == n and t.end_offset == offs[20][1]
    out, st = t.decode_host(offs[18][0] + 7, 4096 * 3)
    assert st.samples == offs[20][0] - offs[18][0] - 7
    np.testing.assert_array_equal(out, pcm[offs[18][0] + 7: offs[20][0]].astype(np.int16))
    t.close()


def test_32_bit_streams_are_refused(tmp_path, lib):
    from buzzdetect_amd.flacio import FlacFormatError, FlacTrack
    pcm = G.test_signal(10_000, 1, 16, seed=0)
    data = bytearray(G.encode(pcm, 16000, 16, blocksize=4096))
    v = int.from_bytes(data[18:26], "big")
    v = (v & ~(31 << 36)) | (31 << 36)                       # STREAMINFO: 32 bits per sample
    data[18:26] = v.to_bytes(8, "big")
    with pytest.raises(FlacFormatError, match="32-bit"):
        FlacTrack(write(tmp_path, "wide.flac", bytes(data)))
    si = _lib.bd_flac_streaminfo(4096, 4096, 16000, 1, 32, 0, 0)
    st = _lib.bd_flac_status()
    assert lib.bd_flac_decode_host(None, 0, C.byref(si), 0, 0, None, C.byref(st)) == -1
    assert lib.bd_flac_workspace_bytes(C.byref(si), 100, 100) == -1


def test_planner_skips_32_bit_flac_with_a_warning_and_finds_flac_files(tmp_path, caplog):
    import logging
    from buzzdetect_amd import analyze as A
    from buzzdetect_amd import pipeline as P, results as R
    pcm = G.test_signal(20_000, 1, 16, seed=0)
    data = bytearray(G.encode(pcm, 16000, 16, blocksize=4096))
    data[18:26] = (int.from_bytes(data[18:26], "big") | (31 << 36)).to_bytes(8, "big")
    (tmp_path / "a").mkdir()
    (tmp_path / "a" / "w.FLAC").write_bytes(bytes(data))
    assert A.search_audio(str(tmp_path)) == [str(tmp_path / "a" / "w.FLAC")]
    pipe = P.Pipeline(make_engine=None, classes=["a"], framehop_s=0.96, hop=15360, step=96, chunklength=10, framelength_s=0.96,
                      digits_time=2, digits_results=2, classes_out="all", threshold=None, readers=1, analyzers=1, pin_memory=False)
    job = P.FileJob(str(tmp_path / "a" / "w.FLAC"), "a/w", "a/w.FLAC", R.ResultFile(str(tmp_path / "out" / "a" / "w")))
    with caplog.at_level(logging.DEBUG, logger="buzzdetect"):
        pipe._plan_file(job)
    assert pipe.report.files_skipped == 1 and pipe.q_units.empty()
    assert any(r.levelno == logging.WARNING and "32-bit" in r.getMessage() for r in caplog.records)


def test_host_reader_stage_gives_the_wav_chunks(tmp_path):
    """The planner and reader on a FLAC give the ChunkTasks (and the bytes) a WAV of the same samples gives."""
    from buzzdetect_amd import pipeline as P, results as R
    pcm = G.test_signal(16000 * 30, 1, 16, seed=4)
    (tmp_path / "a.flac").write_bytes(G.encode(pcm, 16000, 16, blocksize=4096))
    (tmp_path / "b.wav").write_bytes(G.wav_bytes(pcm, 16000, 16))
    got = {}
    for name in ("a.flac", "b.wav"):
        pipe = P.Pipeline(make_engine=None, classes=["a"], framehop_s=0.96, hop=15360, step=96, chunklength=7.1, framelength_s=0.96,
                          digits_time=2, digits_results=2, classes_out="all", threshold=None, readers=1, analyzers=1,
                          pin_memory=False, stream_buffer_depth=64)
        job = P.FileJob(str(tmp_path / name), name[:1], name, R.ResultFile(str(tmp_path / "out" / name[:1])))
        pipe._plan_file(job)
        while not pipe.q_units.empty():
            pipe._read_unit(pipe.q_units.get())
        tasks = []
        while not pipe.q_analyze.empty():
            t = pipe.q_analyze.get()
            tasks.append((t.chunk, t.frames, t.nbytes, t.s16, bytes(pipe.pool.buffer(t.slot).numpy()[: t.nbytes])))
        got[name] = tasks
    assert got["a.flac"] == got["b.wav"] and len(got["b.wav"]) == 5
