"""FLAC on the device: bd_flac_decode == the host decoder == source PCM bit for bit, false syncs, CRC-16 failures, and
analyze() on FLAC writing the bytes it writes for a WAV of the same samples."""
import ctypes as C
import logging

import numpy as np
import pytest

from buzzdetect_amd import _lib
from tools import flacgen as G

pytestmark = pytest.mark.gpu


def device_decode(data: bytes, si, first: int, n: int):
    """Range bytes -> (decoded [n, ch] numpy, status) through bd_flac_decode on the current stream."""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    comp = torch.zeros((len(data) + 3) // 4 * 4 + 8, dtype=torch.uint8, device=dev)
    if data:
        comp[: len(data)].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    ws = torch.empty(_lib.check(lib.bd_flac_workspace_bytes(C.byref(si), len(data), n)), dtype=torch.uint8, device=dev)
    out = torch.zeros((max(n, 1), si.channels), dtype=torch.int16 if si.bits_per_sample == 16 else torch.float32, device=dev)
    status = torch.zeros(C.sizeof(_lib.bd_flac_status), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    _lib.check(lib.bd_flac_decode(comp.data_ptr(), len(data), C.byref(si), first, n, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                  status.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    st = _lib.bd_flac_status.from_buffer_copy(status.cpu().numpy().tobytes())
    return out[:n].cpu().numpy(), st


def host_decode(data: bytes, si, first: int, n: int):
    buf = np.frombuffer(data, np.uint8)
    out = np.zeros((n, si.channels), np.int16 if si.bits_per_sample == 16 else np.float32)
    st = _lib.bd_flac_status()
    _lib.check(_lib.load().bd_flac_decode_host(buf.ctypes.data if buf.size else None, buf.size, C.byref(si), first, n,
                                               out.ctypes.data if out.size else None, C.byref(st)))
    return out, st


def fields(st):
    return (st.samples, st.stop_offset, st.first_sample, st.end_sample, st.reason, st.frames)


def expected(pcm, bps):
    return pcm.astype(np.int16) if bps == 16 else (pcm.astype(np.float64) / (1 << (bps - 1))).astype(np.float32)


MATRIX = [
    (16, 1, 4096, False, "independent", ("lpc", 8), "rice", None, False),
    (16, 2, 4608, False, "mid_side", ("lpc", 12, 15), "rice2", 3, False),
    (16, 2, 1152, False, "left_side", ("fixed", 2), "rice", 0, False),
    (16, 2, 576, False, "side_right", ("fixed", 3), "escape", 2, False),
    (8, 1, 192, False, "independent", ("fixed", 1), "rice", 1, False),
    (12, 3, 256, False, "independent", ("lpc", 4, 10, 6), "rice", 6, False),
    (20, 6, 2048, False, "independent", ("lpc", 32, 15), "rice2", 2, False),
    (24, 2, [4096, 1000, 65535, 16, 333], True, "mid_side", ("lpc", 16, 14), "rice", 0, False),
    (24, 1, 8192, False, "independent", ("fixed", 4), "rice2", 8, True),
    (16, 2, 300, True, "independent", "verbatim", "rice", None, True),
]


@pytest.mark.parametrize("case", range(len(MATRIX)))
def test_device_equals_host_equals_source(case):
    bps, ch, bs, variable, mode, kind, method, po, wasted = MATRIX[case]
    n = 90_000
    pcm = G.test_signal(n, ch, bps, seed=case)
    if wasted:
        pcm = (pcm >> 2) << 2
    data, offs = G.encode(pcm, 48000, bps, blocksize=bs, variable=variable, mode=mode, subframe_kind=kind, method=method,
                          porder=po, wasted=wasted, return_offsets=True)
    sizes = [bs] if np.isscalar(bs) else bs
    si = _lib.bd_flac_streaminfo(min(sizes), max(sizes), 48000, ch, bps, 0, n)
    rng = np.random.default_rng(case)
    windows = [(0, n), (n - 1, 1), (n - 5000, 5000)] + [(int(a), int(rng.integers(1, n - a + 1))) for a in rng.integers(1, n - 1, 4)]
    for a, m in windows:
        k = max(i for i, (s, _, _) in enumerate(offs) if s <= a)
        e = max(i for i, (s, _, _) in enumerate(offs) if s <= a + m - 1)
        seg = data[offs[k][1]: offs[e][2]]
        d, sd = device_decode(seg, si, a, m)
        h, sh = host_decode(seg, si, a, m)
        assert fields(sd) == fields(sh) and sd.samples == m and sd.reason == 0, (a, m, fields(sd), fields(sh))
        np.testing.assert_array_equal(d, h)
        np.testing.assert_array_equal(d, expected(pcm[a:a + m], bps))


def test_one_hour_48k_mono_in_600_s_ranges(tmp_path):
    from buzzdetect_amd.flacio import FlacTrack
    period = 4096 * 704                                     # ~60 s: frames repeat (the writer reuses their bodies)
    base = G.test_signal(period, 1, 16, seed=11).astype(np.int16)
    n = 48000 * 3600
    pcm = np.tile(base, (n // period + 1, 1))[:n]
    path = tmp_path / "hour.flac"
    path.write_bytes(G.encode(pcm, 48000, 16, blocksize=4096, subframe_kind=("lpc", 8), seektable=48000 * 10))
    t = FlacTrack(str(path))
    assert t.frames == n
    step = 48000 * 600
    raw = path.read_bytes()
    for a in range(0, n, step):
        m = min(step, n - a)
        off, end = t.byte_range(a, m)
        seg = raw[off:end]
        d, st = device_decode(seg, t.si, a, m)
        assert st.samples == m and st.reason == 0
        np.testing.assert_array_equal(d[:, 0], pcm[a:a + m, 0].astype(np.int16))
    t.close()


def test_false_sync_inside_a_verbatim_subframe():
    """A verbatim subframe whose samples spell a frame header with a good CRC-8 (frame number 0): a candidate of the scan
    that lies inside a real frame, never reached by the chain."""
    n = 4096 * 6
    pcm = G.test_signal(n, 1, 16, seed=5)
    fake = G.frame_header(0, 4096, 48000, 0, 16, False)
    fake = fake + b"\x00" * (len(fake) % 2)
    words = np.frombuffer(fake, ">i2").astype(np.int64)
    pcm[4096 * 2 + 100: 4096 * 2 + 100 + words.size, 0] = words
    kinds = lambda k, c: "verbatim" if k == 2 else ("lpc", 8)
    data, offs = G.encode(pcm, 48000, 16, blocksize=4096, subframe_kind=kinds, return_offsets=True)
    body = data[offs[0][1]:]
    assert body.count(fake[:-1]) >= 1
    si = _lib.bd_flac_streaminfo(4096, 4096, 48000, 1, 16, 0, n)
    d, sd = device_decode(body, si, 0, n)
    h, sh = host_decode(body, si, 0, n)
    assert fields(sd) == fields(sh) and sd.samples == n and sd.frames == 6
    np.testing.assert_array_equal(d[:, 0], pcm[:, 0].astype(np.int16))


def test_corrupted_crc16_stops_the_decode_there():
    n = 4096 * 8
    pcm = G.test_signal(n, 2, 16, seed=6)
    data, offs = G.encode(pcm, 48000, 16, blocksize=4096, mode="mid_side", return_offsets=True)
    body = bytearray(data[offs[0][1]:])
    bad = offs[5][2] - offs[0][1] - 1                       # the last CRC byte of frame 5
    body[bad] ^= 0x5A
    si = _lib.bd_flac_streaminfo(4096, 4096, 48000, 2, 16, 0, n)
    d, sd = device_decode(bytes(body), si, 100, n - 100)
    h, sh = host_decode(bytes(body), si, 100, n - 100)
    assert fields(sd) == fields(sh)
    assert sd.reason == 1 and sd.stop_offset == offs[5][1] - offs[0][1] and sd.frames == 5 and sd.samples == 4096 * 5 - 100
    np.testing.assert_array_equal(d[: sd.samples], pcm[100: 4096 * 5].astype(np.int16))


def test_read_flac_is_soundfile_float32(engine, tmp_path):
    pcm = G.test_signal(100_000, 2, 24, seed=8)
    (tmp_path / "x.flac").write_bytes(G.encode(pcm, 44100, 24, blocksize=4608, mode="left_side"))
    got = engine.read_flac(str(tmp_path / "x.flac"), start=1234, frames=50_000).cpu().numpy()
    np.testing.assert_array_equal(got, (pcm[1234:51234] / 2.0 ** 23).astype(np.float32))
    pcm16 = G.test_signal(30_000, 1, 16, seed=9)
    (tmp_path / "y.flac").write_bytes(G.encode(pcm16, 16000, 16))
    got = engine.read_flac(str(tmp_path / "y.flac")).cpu().numpy()
    np.testing.assert_array_equal(got, (pcm16 / 32768.0).astype(np.float32))


FORMATS = [(16000, 1, 16, 4096, 7.3), (48000, 2, 16, 4608, 5.1), (44100, 1, 24, 4096, 6.7), (48000, 6, 16, 4096, 5.1),
           (44100, 3, 24, 4096, 6.7)]


@pytest.mark.parametrize("fmt", range(len(FORMATS)))
def test_analyze_flac_writes_the_bytes_of_the_wav(engine, tmp_path, fmt):
    from buzzdetect_amd.analyze import analyze
    rate, ch, bps, bs, chunk = FORMATS[fmt]
    pcm = G.test_signal(rate * 23 + 77, ch, bps, seed=fmt)
    for name in ("flac", "wav"):
        (tmp_path / name).mkdir()
    (tmp_path / "flac" / "a.flac").write_bytes(G.encode(pcm, rate, bps, blocksize=bs, mode="mid_side" if ch == 2 else "independent"))
    (tmp_path / "wav" / "a.wav").write_bytes(G.wav_bytes(pcm, rate, bps))
    reps = {}
    for name in ("flac", "wav"):
        reps[name] = analyze("model_general_v3", chunklength=chunk, dir_audio=str(tmp_path / name), dir_out=str(tmp_path / ("o" + name)),
                             engine=engine)
    a = (tmp_path / "oflac" / "a_buzzdetect.csv").read_bytes()
    b = (tmp_path / "owav" / "a_buzzdetect.csv").read_bytes()
    assert a == b and a.count(b"\n") > 10
    assert reps["flac"].chunks == reps["wav"].chunks and reps["flac"].busy.get("decode", 0) > 0


def test_resume_and_two_analyzers_on_flac(engine, tmp_path):
    import threading
    from buzzdetect_amd.analyze import analyze
    audio = tmp_path / "audio"
    audio.mkdir()
    pcm = G.test_signal(48000 * 40, 2, 16, seed=3)
    (audio / "r.flac").write_bytes(G.encode(pcm, 48000, 16, blocksize=4096, mode="mid_side"))
    (audio / "s.flac").write_bytes(G.encode(pcm[: 48000 * 17], 48000, 16, blocksize=1152, mode="left_side"))
    whole = analyze("model_general_v3", chunklength=4.8, dir_audio=str(audio), dir_out=str(tmp_path / "whole"), engine=engine)
    assert whole.files_done == 2
    stop = threading.Event()
    from buzzdetect_amd import pipeline as P
    orig = P.Pipeline._read_unit
    count = [0]

    def read_then_stop(self, unit):
        count[0] += 1
        if count[0] == 4:
            stop.set()
        return orig(self, unit)
    P.Pipeline._read_unit = read_then_stop
    try:
        part = analyze("model_general_v3", chunklength=4.8, dir_audio=str(audio), dir_out=str(tmp_path / "resumed"), engine=engine,
                       event_stopanalysis=stop)
    finally:
        P.Pipeline._read_unit = orig
    assert part.end_reason == "interrupted"
    analyze("model_general_v3", chunklength=4.8, dir_audio=str(audio), dir_out=str(tmp_path / "resumed"), engine=engine)
    two = analyze("model_general_v3", chunklength=4.8, dir_audio=str(audio), dir_out=str(tmp_path / "two"), analyzers_gpu=2,
                  n_streamers=4)
    assert two.files_done == 2
    for rel in ("r", "s"):
        a = (tmp_path / "whole" / f"{rel}_buzzdetect.csv").read_bytes()
        assert a == (tmp_path / "resumed" / f"{rel}_buzzdetect.csv").read_bytes()
        assert a == (tmp_path / "two" / f"{rel}_buzzdetect.csv").read_bytes()


def test_flac_cut_short_matches_the_wav_cut_at_the_same_sample(engine, tmp_path, caplog):
    from buzzdetect_amd.analyze import analyze
    pcm = G.test_signal(16000 * 100, 1, 16, seed=3)
    data, offs = G.encode(pcm, 16000, 16, blocksize=4096, return_offsets=True)
    k = next(i for i, (s, _, _) in enumerate(offs) if s >= 16000 * 60)
    cut_sample = offs[k][0]
    for name in ("f", "w"):
        (tmp_path / name).mkdir()
    (tmp_path / "f" / "dead.flac").write_bytes(data[: offs[k][1] + 40])      # cut inside frame k
    wav = G.wav_bytes(pcm, 16000, 16)
    (tmp_path / "w" / "dead.wav").write_bytes(wav[: 44 + cut_sample * 2])
    msgs = {}
    for name in ("f", "w"):
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="buzzdetect"):
            analyze("model_general_v3", framehop_prop=1, chunklength=19.2, dir_audio=str(tmp_path / name),
                    dir_out=str(tmp_path / ("o" + name)), engine=engine)
        msgs[name] = [(r.levelno, r.getMessage().replace(".flac", ".x").replace(".wav", ".x")) for r in caplog.records
                      if "Unreadable audio" in r.getMessage()]
    assert msgs["f"] == msgs["w"] and len(msgs["f"]) == 1 and msgs["f"][0][0] == logging.WARNING
    assert (tmp_path / "of" / "dead_buzzdetect.csv").read_bytes() == (tmp_path / "ow" / "dead_buzzdetect.csv").read_bytes()
