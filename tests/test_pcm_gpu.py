"""pcmio's formats on the device: bd_pcm_decode == bd_pcm_decode_host bit for bit (status included) for every codec and
layout over the ranges a chunk can take, on a range that fills the chip, and analyze() on each new format writing the bytes
it writes for a WAV of the same decoded samples."""
import ctypes as C
import logging

import numpy as np
import pytest

from buzzdetect_amd import _lib, pcmio
from tools import pcmgen as G

pytestmark = pytest.mark.gpu


def device_decode(data: bytes, fmt, first: int, n: int, fill: int = 0):
    """Range bytes -> (decoded [n, ch] numpy, status) through bd_pcm_decode on the current stream."""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    comp = torch.zeros((len(data) + 3) // 4 * 4 + 8, dtype=torch.uint8, device=dev)
    if data:
        comp[: len(data)].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    ws = torch.empty(max(_lib.check(lib.bd_pcm_workspace_bytes(C.byref(fmt), len(data), n)), 1), dtype=torch.uint8, device=dev)
    s16 = pcmio.out_is_s16(fmt)
    out = torch.full((max(n, 1), fmt.channels), fill, dtype=torch.int16 if s16 else torch.float32, device=dev)
    status = torch.zeros(C.sizeof(_lib.bd_pcm_status), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    _lib.check(lib.bd_pcm_decode(comp.data_ptr(), len(data), C.byref(fmt), first, n, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                 status.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    st = _lib.bd_pcm_status.from_buffer_copy(status.cpu().numpy().tobytes())
    return out[:n].cpu().numpy(), st


def host_decode(data: bytes, fmt, first: int, n: int, fill: int = 0):
    buf = np.frombuffer(data, np.uint8)
    out = np.full((n, fmt.channels), fill, np.int16 if pcmio.out_is_s16(fmt) else np.float32)
    st = _lib.bd_pcm_status()
    _lib.check(_lib.load().bd_pcm_decode_host(buf.ctypes.data if buf.size else None, buf.size, C.byref(fmt), first, n,
                                              out.ctypes.data if out.size else None, C.byref(st)))
    return out, st


def fields(st):
    return (st.samples, st.end_sample, st.bad_block, st.reason)


def stream_of(kind: str, ch: int, n: int, seed: int):
    """(format, bytes) of n frames of `kind`."""
    pcm = G.test_signal(n, ch, 16, seed=seed)
    if kind == "ima":
        data, spb = G.ima_encode(pcm, 256 * ch)
        return pcmio.make_format(_lib.PCM_IMA_ADPCM, ch, block_align=256 * ch, samples_per_block=spb), data
    if kind == "ms":
        data, spb = G.ms_encode(pcm, 128 * ch + 100)
        return pcmio.make_format(_lib.PCM_MS_ADPCM, ch, block_align=128 * ch + 100, samples_per_block=spb, coefs=G.MS_COEFS), data
    if kind in ("ulaw", "alaw"):
        return pcmio.make_format(_lib.PCM_ULAW if kind == "ulaw" else _lib.PCM_ALAW, ch, 1), G.g711(pcm, kind)
    if kind.startswith("f"):
        width, big = (4 if kind.startswith("f32") else 8), kind.endswith("be")
        x = pcm / 32768.0 + np.random.default_rng(seed).standard_normal(pcm.shape) * 1e-6
        return pcmio.make_format(_lib.PCM_FLOAT, ch, width, big_endian=big), G.floats(x, width, big)
    # linear: s8 u8 be16 le16 be24 le24 u24 be32 le32
    width = {"8": 1, "16": 2, "24": 3, "32": 4}[kind.lstrip("sulbe")]
    big, signed = kind.startswith("be"), not kind.startswith("u")
    x = pcm >> (16 - 8 * width) if width == 1 else pcm << (8 * width - 16)
    x = x + np.random.default_rng(seed).integers(0, 1 << max(8 * width - 16, 0), x.shape)
    return pcmio.make_format(_lib.PCM_LINEAR, ch, width, big_endian=big, signed=signed), G.linear(x, width, big, signed)


KINDS = ["ima", "ms", "ulaw", "alaw", "s8", "u8", "be16", "le16", "be24", "le24", "u24", "be32", "le32", "f32be", "f32le",
         "f64be", "f64le"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ch", [1, 2, 6])
def test_device_equals_host(kind, ch):
    n = 40_000 + 7 * ch
    fmt, data = stream_of(kind, ch, n, seed=ch)
    spb, ba = fmt.samples_per_block, fmt.block_align
    total = len(data) // ba * spb
    rng = np.random.default_rng(ch)
    windows = [(0, total), (spb // 2 + 3, 1), (total - 1, 1), (spb + 5, 3 * spb + 1), (total - spb - 9, spb + 9)] + \
              [(int(a), int(rng.integers(1, total - a + 1))) for a in rng.integers(1, total - 1, 3)]
    for a, m in windows:
        seg = data[a // spb * ba: -(-(a + m) // spb) * ba]
        d, sd = device_decode(seg, fmt, a, m, fill=77)
        h, sh = host_decode(seg, fmt, a, m, fill=77)
        assert fields(sd) == fields(sh) and sd.samples == m and sd.reason == 0, (a, m, fields(sd), fields(sh))
        assert d.tobytes() == h.tobytes(), (a, m)
    # a range cut inside a block, and (ADPCM) an invalid header two blocks in
    seg = data[ba: 4 * ba + ba // 2 + 1]
    d, sd = device_decode(seg, fmt, spb + 1, 4 * spb, fill=77)
    h, sh = host_decode(seg, fmt, spb + 1, 4 * spb, fill=77)
    assert fields(sd) == fields(sh) and d.tobytes() == h.tobytes()
    if spb > 1:
        assert sd.reason == 2 and 0 < sd.samples < 4 * spb
        bad = bytearray(data[: 6 * ba])
        bad[3 * ba + (2 if kind == "ima" else 0)] = 200
        d, sd = device_decode(bytes(bad), fmt, 5, 6 * spb - 5, fill=77)
        h, sh = host_decode(bytes(bad), fmt, 5, 6 * spb - 5, fill=77)
        assert fields(sd) == fields(sh) == (3 * spb - 5, 3 * spb, 3, 1) and d.tobytes() == h.tobytes()


@pytest.mark.parametrize("kind", ["ima", "ms", "ulaw", "be16", "be24", "f32be"])
def test_600_s_of_48k_stereo_fills_the_chip(kind):
    """One chunk of 600 s at 48 kHz stereo (28.8 M frames): every block / group of the range at once."""
    n = 48000 * 600
    if kind in ("ima", "ms"):
        ba = 2048
        spb = G.ima_spb(ba, 2) if kind == "ima" else G.ms_spb(ba, 2)
        nblk = -(-n // spb)
        data = G.random_adpcm(kind, nblk, ba, 2, seed=1)
        fmt = pcmio.make_format(_lib.PCM_IMA_ADPCM if kind == "ima" else _lib.PCM_MS_ADPCM, 2, block_align=ba,
                                samples_per_block=spb, coefs=G.MS_COEFS if kind == "ms" else ())
    else:
        width = {"ulaw": 1, "be16": 2, "be24": 3, "f32be": 4}[kind]
        data = np.random.default_rng(2).integers(0, 256, n * 2 * width, dtype=np.uint8).tobytes()
        codec = {"ulaw": _lib.PCM_ULAW, "f32be": _lib.PCM_FLOAT}.get(kind, _lib.PCM_LINEAR)
        fmt = pcmio.make_format(codec, 2, width, big_endian=True)
        if kind == "f32be":                                  # no NaN payloads: finite floats of every exponent
            x = np.frombuffer(data, ">u4").copy() & np.uint32(0xBFFFFFFF)
            data = x.astype(">u4").tobytes()
    first = 12345
    m = n - first
    seg = data[first // fmt.samples_per_block * fmt.block_align:]
    d, sd = device_decode(seg, fmt, first, m)
    h, sh = host_decode(seg, fmt, first, m)
    assert fields(sd) == fields(sh) and sd.samples == m
    assert d.tobytes() == h.tobytes()


def test_read_pcm_is_soundfile_float32(engine, tmp_path):
    pcm = G.test_signal(50_000, 2, 16, seed=8)
    ima, spb = G.ima_encode(pcm, 1024)
    (tmp_path / "i.wav").write_bytes(G.wave(G.fmt_ima(2, 44100, 1024, spb), ima, fact=50_000))
    t = pcmio.PcmTrack(str(tmp_path / "i.wav"))
    host, _ = t.decode_host(0, t.frames)
    t.close()
    got = engine.read_pcm(str(tmp_path / "i.wav"), start=1234, frames=30_000).cpu().numpy()
    np.testing.assert_array_equal(got, (host[1234:31234] / 32768.0).astype(np.float32))
    x24 = G.test_signal(20_000, 1, 24, seed=9)
    (tmp_path / "a.aiff").write_bytes(G.aiff(G.linear(x24, 3, True), 16000, 1, 20_000, 24))
    got = engine.read_pcm(str(tmp_path / "a.aiff")).cpu().numpy()
    np.testing.assert_array_equal(got, (x24 / 2.0 ** 23).astype(np.float32))


def _formats(pcm, rate):
    """name -> file bytes of the same signal in every new container / encoding."""
    ch = pcm.shape[1]
    n = pcm.shape[0]
    ima, ispb = G.ima_encode(pcm, 512 * ch)
    ms, mspb = G.ms_encode(pcm, 512 * ch)
    return {
        "a.aiff": G.aiff(G.linear(pcm, 2, True), rate, ch, n, 16),
        "b.aiff": G.aiff(G.linear(pcm, 2, False), rate, ch, n, 16, compression=b"sowt", ssnd_offset=4),
        "c.aiff": G.aiff(G.floats(pcm / 32768.0, 4, True), rate, ch, n, 32, compression=b"fl32"),
        "d.aiff": G.aiff(G.g711(pcm, "alaw"), rate, ch, n, 16, compression=b"alaw"),
        "e.au": G.au(G.g711(pcm, "ulaw"), rate, ch, 1),
        "f.au": G.au(G.linear(pcm << 8, 3, True), rate, ch, 4, unknown_size=True),
        "g.w64": G.w64(G.fmt_body(1, ch, rate, 16, 2 * ch), G.linear(pcm, 2)),
        "h.w64": G.w64(G.fmt_ms(ch, rate, 512 * ch, mspb), ms, fact=n),
        "i.wav": G.wave(G.fmt_ima(ch, rate, 512 * ch, ispb), ima, fact=n),
        "j.wav": G.wave(G.fmt_ms(ch, rate, 512 * ch, mspb), ms, fact=n),
        "k.wav": G.wave(G.fmt_body(7, ch, rate, 8, ch), G.g711(pcm, "ulaw")),
        "l.rf64": G.wave(G.fmt_body(6, ch, rate, 8, ch), G.g711(pcm, "alaw"), rf64=True),
    }


def _as_wav(path, rate):
    t = pcmio.PcmTrack(path)
    x, _ = t.decode_host(0, t.frames)
    t.close()
    return G.wav16(x, rate) if x.dtype == np.int16 else G.wav_f32(x, rate)


ANALYZE = [(16000, 1, 1.0, None, 7.3), (16000, 1, 0.5, 0.95, 5.1), (48000, 2, 1.0, None, 6.7), (48000, 6, 1.0, None, 6.7),
           (16000, 3, 1.0, None, 7.3)]


@pytest.mark.parametrize("case", range(len(ANALYZE)))
def test_analyze_writes_the_bytes_of_the_wav(engine, tmp_path, case):
    from buzzdetect_amd.analyze import analyze
    rate, ch, hop, precision, chunk = ANALYZE[case]
    pcm = G.test_signal(rate * 23 + 77, ch, 16, seed=case)
    files = _formats(pcm, rate)
    if rate == 48000:                                        # the resample path: one container of each decode kind
        files = {k: files[k] for k in ("a.aiff", "c.aiff", "i.wav", "k.wav")}
    src, ref = tmp_path / "src", tmp_path / "ref"
    src.mkdir()
    ref.mkdir()
    for name, data in files.items():
        (src / name).write_bytes(data)
        (ref / (name.split(".")[0] + ".wav")).write_bytes(_as_wav(str(src / name), rate))
    kw = dict(chunklength=chunk, framehop_prop=hop, engine=engine)
    if precision is not None:                              # detections instead of activations
        kw.update(precision=precision)
    ra = analyze("model_general_v3", dir_audio=str(src), dir_out=str(tmp_path / "osrc"), **kw)
    rb = analyze("model_general_v3", dir_audio=str(ref), dir_out=str(tmp_path / "oref"), **kw)
    assert ra.files_done == rb.files_done == len(files) and ra.chunks == rb.chunks
    for name in files:
        stem = name.split(".")[0]
        a = (tmp_path / "osrc" / f"{stem}_buzzdetect.csv").read_bytes()
        b = (tmp_path / "oref" / f"{stem}_buzzdetect.csv").read_bytes()
        assert a == b and a.count(b"\n") > (1 if precision else 10), name
    assert ra.busy.get("decode", 0) > 0


@pytest.mark.parametrize("kind", ["ima", "ms", "aiff"])
def test_cut_short_mid_block_matches_the_wav_cut_at_the_same_frame(engine, tmp_path, caplog, kind):
    from buzzdetect_amd.analyze import analyze
    pcm = G.test_signal(16000 * 100, 1, 16, seed=3)
    if kind == "ima":
        data, spb = G.ima_encode(pcm, 1024)
        full = G.wave(G.fmt_ima(1, 16000, 1024, spb), data, fact=pcm.shape[0])
    elif kind == "ms":
        data, spb = G.ms_encode(pcm, 1024)
        full = G.wave(G.fmt_ms(1, 16000, 1024, spb), data, fact=pcm.shape[0])
    else:
        full = G.aiff(G.linear(pcm, 2, True), 16000, 1, pcm.shape[0], 16)
    for name in ("p", "w"):
        (tmp_path / name).mkdir()
    src = tmp_path / "p" / ("dead.aiff" if kind == "aiff" else "dead.wav")
    src.write_bytes(full[: int(len(full) * 0.6) + 333])          # inside a block
    t = pcmio.PcmTrack(str(src))
    dec, _ = t.decode_host(0, t.frames)
    declared = t.frames_declared
    t.close()
    wav = G.wav16(np.concatenate([dec, np.zeros((declared - dec.shape[0], 1), np.int16)]), 16000)
    (tmp_path / "w" / "dead.wav").write_bytes(wav[: 44 + 2 * dec.shape[0]])
    msgs = {}
    for name in ("p", "w"):
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="buzzdetect"):
            analyze("model_general_v3", framehop_prop=1, chunklength=19.2, dir_audio=str(tmp_path / name),
                    dir_out=str(tmp_path / ("o" + name)), engine=engine)
        msgs[name] = [(r.levelno, r.getMessage().replace(".aiff", ".x").replace(".wav", ".x")) for r in caplog.records
                      if "Unreadable audio" in r.getMessage()]
    assert msgs["p"] == msgs["w"] and len(msgs["p"]) == 1 and msgs["p"][0][0] == logging.WARNING
    assert (tmp_path / "op" / "dead_buzzdetect.csv").read_bytes() == (tmp_path / "ow" / "dead_buzzdetect.csv").read_bytes()


def test_ranges_in_pieces_decode_as_one(engine, tmp_path, monkeypatch):
    """Ranges past pcmio.PIECE_BYTES go through bd_pcm_decode in pieces of whole blocks: read_pcm and analyze() give what one
    piece gives."""
    from buzzdetect_amd.analyze import analyze
    pcm = G.test_signal(16000 * 40, 2, 16, seed=21)
    ms, spb = G.ms_encode(pcm, 1024)
    src = tmp_path / "src"
    src.mkdir()
    (src / "m.wav").write_bytes(G.wave(G.fmt_ms(2, 16000, 1024, spb), ms, fact=pcm.shape[0]))
    (src / "f.au").write_bytes(G.au(G.floats(pcm / 32768.0, 8, True), 16000, 2, 7))
    whole = {n: engine.read_pcm(str(src / n), start=777).cpu().numpy() for n in ("m.wav", "f.au")}
    analyze("model_general_v3", chunklength=9.6, dir_audio=str(src), dir_out=str(tmp_path / "one"), engine=engine)
    monkeypatch.setattr(pcmio, "PIECE_BYTES", 5 * 1024 + 17)
    for n in ("m.wav", "f.au"):
        got = engine.read_pcm(str(src / n), start=777).cpu().numpy()
        assert got.shape[0] == pcm.shape[0] - 777 and got.tobytes() == whole[n].tobytes(), n
    rep = analyze("model_general_v3", chunklength=9.6, dir_audio=str(src), dir_out=str(tmp_path / "pieces"), engine=engine)
    assert rep.files_done == 2
    for stem in ("m", "f"):
        a = (tmp_path / "one" / f"{stem}_buzzdetect.csv").read_bytes()
        assert a == (tmp_path / "pieces" / f"{stem}_buzzdetect.csv").read_bytes() and a.count(b"\n") > 10
