"""pcmio's formats on the host: container parsing (AIFF / AIFF-C, AU, Wave64, RF64, coded WAVE), the host decoder (the same
routines the device runs) against independent oracles - audioop's G.711 and IMA ADPCM, a NumPy restatement of MS ADPCM,
WavTrack.convert for the sample layouts, the aifc / sunau modules for their files - ranges, invalid block headers, routing
by magic, discovery and the host-only reader stage.  No device needed."""
import ctypes as C
import logging
import os
import struct
import warnings

import numpy as np
import pytest

from buzzdetect_amd import _lib, pcmio
from buzzdetect_amd.wavio import WavTrack
from tools import pcmgen as G

with warnings.catch_warnings():
    warnings.simplefilter("ignore", DeprecationWarning)
    import aifc
    import audioop
    import sunau


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def host_decode(lib, fmt, data: bytes, first: int, n: int, fill: int = 0):
    buf = np.frombuffer(data, np.uint8)
    s16 = pcmio.out_is_s16(fmt)
    out = np.full((n, fmt.channels), fill, np.int16 if s16 else np.float32)
    st = _lib.bd_pcm_status()
    _lib.check(lib.bd_pcm_decode_host(buf.ctypes.data if buf.size else None, buf.size, C.byref(fmt), first, n,
                                      out.ctypes.data if out.size else None, C.byref(st)))
    return out, st


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def wav_convert(tmp_path, pcm, width: int, is_float: bool = False) -> np.ndarray:
    """The float32 samples WavTrack.convert gives for the same samples written as WAV."""
    x = G._2d(pcm)
    ch = x.shape[1]
    if is_float:
        data, tag = G.floats(x, width), 3
    else:
        data, tag = G.linear(x, width, signed=width != 1) if width != 1 else G.linear(x, 1, signed=False), 1
    path = write(tmp_path, "ref.wav", G.wave(G.fmt_body(tag, ch, 8000, 8 * width, width * ch), data))
    t = WavTrack(path)
    raw = np.zeros(t.frames * t.bytes_per_frame, np.uint8)
    t.read_raw_into(0, t.frames, raw)
    out = t.convert(raw)
    t.close()
    return out


# ---------------------------------------------------------------- G.711
def test_g711_all_256_codes_match_audioop(lib):
    codes = bytes(range(256))
    for codec, oracle in ((_lib.PCM_ULAW, audioop.ulaw2lin), (_lib.PCM_ALAW, audioop.alaw2lin)):
        f = pcmio.make_format(codec, 1, 1)
        got, st = host_decode(lib, f, codes, 0, 256)
        want = np.frombuffer(oracle(codes, 2), "<i2")
        np.testing.assert_array_equal(got[:, 0], want)
        assert st.samples == 256 and st.reason == 0
    assert host_decode(lib, pcmio.make_format(_lib.PCM_ULAW, 1, 1), b"\x00", 0, 1)[0][0, 0] == -32124
    np.testing.assert_array_equal(G.ulaw_table(), np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2"))
    np.testing.assert_array_equal(G.alaw_table(), np.frombuffer(audioop.alaw2lin(codes, 2), "<i2"))


def test_g711_encoder_round_trips_its_table():
    for law, table in (("ulaw", G.ulaw_table()), ("alaw", G.alaw_table())):
        codes = np.frombuffer(G.g711(table, law), np.uint8)
        np.testing.assert_array_equal(table[codes], table)


# ---------------------------------------------------------------- IMA ADPCM
def ima_oracle(data: bytes, ch: int, block_align: int, spb: int, nblk: int) -> np.ndarray:
    """audioop.adpcm2lin fed each block's header state, the block's codes reordered to its high-nibble-first packing."""
    raw = np.frombuffer(data, np.uint8).reshape(nblk, block_align)
    out = np.zeros((nblk, spb, ch), np.int64)
    groups = (spb - 1) // 8
    for b in range(nblk):
        for c in range(ch):
            pred = int(np.frombuffer(raw[b, 4 * c: 4 * c + 2].tobytes(), "<i2")[0])
            index = int(raw[b, 4 * c + 2])
            words = raw[b, 4 * ch:].reshape(groups, ch, 4)[:, c, :].reshape(-1)
            nib = np.empty(words.size * 2, np.int64)
            nib[0::2], nib[1::2] = words & 15, words >> 4                       # WAVE order: low nibble first
            packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()  # audioop: high nibble first
            dec, _ = audioop.adpcm2lin(packed, 2, (pred, index))
            out[b, 0, c] = pred
            out[b, 1:, c] = np.frombuffer(dec, "<i2")[: spb - 1]
    return out.reshape(nblk * spb, ch)


def test_ima_step_table_is_audioops():
    """The 89 steps: audioop's decode of code 7 from index i at predictor 0 adds step_i * 7/8 (shift form) -> step_i."""
    for i, step in enumerate(G.IMA_STEPS.tolist()):
        dec, _ = audioop.adpcm2lin(b"\x70", 2, (0, i))
        want = (step >> 3) + step + (step >> 1) + (step >> 2)
        assert np.frombuffer(dec, "<i2")[0] == min(want, 32767), i


@pytest.mark.parametrize("ch,block_align,index0", [(1, 256, 0), (1, 1024, 30), (2, 512, 10), (2, 2048, 60), (6, 24 * 16, 5)])
def test_ima_matches_audioop(lib, ch, block_align, index0):
    pcm = G.test_signal(7000, ch, 16, seed=ch)
    data, spb = G.ima_encode(pcm, block_align, index0)
    nblk = len(data) // block_align
    f = pcmio.make_format(_lib.PCM_IMA_ADPCM, ch, block_align=block_align, samples_per_block=spb)
    got, st = host_decode(lib, f, data, 0, nblk * spb)
    np.testing.assert_array_equal(got, ima_oracle(data, ch, block_align, spb, nblk))
    assert st.samples == nblk * spb and st.reason == 0 and st.bad_block == -1
    # the encoder is a real one: the decode follows the signal
    assert np.abs(got[:7000].astype(np.int64) - pcm).mean() < 0.1 * np.abs(pcm).mean()
    # random codes with random valid headers too
    data = G.random_adpcm("ima", 5, block_align, ch, seed=3)
    got, st = host_decode(lib, f, data, 0, 5 * spb)
    np.testing.assert_array_equal(got, ima_oracle(data, ch, block_align, spb, 5))


# ---------------------------------------------------------------- MS ADPCM
def ms_oracle(data: bytes, ch: int, block_align: int, spb: int, nblk: int, coefs) -> np.ndarray:
    """A restatement of the MS ADPCM decoder: header (predictor, delta, sample1, sample2), sample2 then sample1 out,
    codes high nibble first, predict = (s1 c1 + s2 c2) >> 8, delta = max(16, adapt[code] delta >> 8)."""
    raw = np.frombuffer(data, np.uint8).reshape(nblk, block_align)
    cf = np.asarray(coefs, np.int64).reshape(-1, 2)
    out = np.zeros((nblk, spb, ch), np.int64)
    for b in range(nblk):
        hdr = raw[b]
        p = hdr[:ch].astype(np.int64)
        delta = np.frombuffer(hdr[ch: 3 * ch].tobytes(), "<i2").astype(np.int64)
        s1 = np.frombuffer(hdr[3 * ch: 5 * ch].tobytes(), "<i2").astype(np.int64)
        s2 = np.frombuffer(hdr[5 * ch: 7 * ch].tobytes(), "<i2").astype(np.int64)
        out[b, 0], out[b, 1] = s2, s1
        body = hdr[7 * ch:]
        nib = np.empty(body.size * 2, np.int64)
        nib[0::2], nib[1::2] = body >> 4, body & 15
        for k in range(2, spb):
            code = nib[(k - 2) * ch: (k - 1) * ch]
            predict = (s1 * cf[p, 0] + s2 * cf[p, 1]) >> 8
            v = np.clip(predict + np.where(code >= 8, code - 16, code) * delta, -32768, 32767)
            s2, s1 = s1, v
            delta = np.clip((G.MS_ADAPT[code] * delta) >> 8, 16, 2 ** 31 - 1)
            out[b, k] = v
    return out.reshape(nblk * spb, ch)


@pytest.mark.parametrize("ch,block_align,coefs", [(1, 256, G.MS_COEFS), (2, 512, G.MS_COEFS), (1, 1024, G.MS_COEFS),
                                                 (2, 300, (256, 0, 300, -100, 100, 50))])
def test_ms_adpcm_matches_the_restatement(lib, ch, block_align, coefs):
    pcm = G.test_signal(5000, ch, 16, seed=ch + 10)
    data, spb = G.ms_encode(pcm, block_align, coefs)
    nblk = len(data) // block_align
    f = pcmio.make_format(_lib.PCM_MS_ADPCM, ch, block_align=block_align, samples_per_block=spb, coefs=coefs)
    got, st = host_decode(lib, f, data, 0, nblk * spb)
    np.testing.assert_array_equal(got, ms_oracle(data, ch, block_align, spb, nblk, coefs))
    assert st.samples == nblk * spb and st.reason == 0
    assert np.abs(got[:5000].astype(np.int64) - pcm).mean() < 400
    data = G.random_adpcm("ms", 4, block_align, ch, seed=5, n_coefs=len(coefs) // 2)
    got, st = host_decode(lib, f, data, 0, 4 * spb)
    np.testing.assert_array_equal(got, ms_oracle(data, ch, block_align, spb, 4, coefs))


# ---------------------------------------------------------------- sample layouts
@pytest.mark.parametrize("width,signed,big", [(1, True, True), (1, False, False), (2, True, True), (3, True, True),
                                              (3, True, False), (3, False, True), (4, True, True), (4, True, False),
                                              (4, False, False)])
def test_layouts_match_wavtrack_convert(lib, tmp_path, width, signed, big):
    rng = np.random.default_rng(width)
    lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1))
    pcm = rng.integers(lo, hi, (3001, 2))
    pcm[:4] = [[lo, hi - 1], [0, -1], [1, lo + 1], [hi - 2, 2]]
    f = pcmio.make_format(_lib.PCM_LINEAR, 2, width, big_endian=big, signed=signed)
    got, st = host_decode(lib, f, G.linear(pcm, width, big, signed), 0, 3001)
    assert st.samples == 3001
    if width == 2:
        np.testing.assert_array_equal(got, pcm.astype(np.int16))
    else:
        want = wav_convert(tmp_path, pcm if width != 1 else pcm, width)
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("width,big", [(4, True), (4, False), (8, True), (8, False)])
def test_float_layouts_match_wavtrack_convert(lib, tmp_path, width, big):
    rng = np.random.default_rng(width)
    x = rng.standard_normal((2000, 3)) * 0.3
    x[0] = [1e-40, -0.0, 1.0 + 2 ** -30]
    f = pcmio.make_format(_lib.PCM_FLOAT, 3, width, big_endian=big)
    got, _ = host_decode(lib, f, G.floats(x, width, big), 0, 2000)
    assert got.tobytes() == wav_convert(tmp_path, x, width, is_float=True).tobytes()


# ---------------------------------------------------------------- containers
def test_aiff_and_aifc_parse_and_decode(tmp_path):
    pcm = G.test_signal(4000, 2, 16, seed=1)
    cases = [
        ("a.aiff", G.aiff(G.linear(pcm, 2, True), 44100, 2, 4000, 16), 2, False),
        ("b.aiff", G.aiff(G.linear(pcm, 2, True), 44100, 2, 4000, 16, compression=b"NONE", ssnd_offset=6, odd_chunk=True), 2, False),
        ("c.aiff", G.aiff(G.linear(pcm, 2, False), 44100, 2, 4000, 16, compression=b"sowt"), 2, False),
        ("d.aiff", G.aiff(G.g711(pcm, "ulaw"), 44100, 2, 4000, 16, compression=b"ulaw"), 1, False),
        ("e.aiff", G.aiff(G.g711(pcm, "alaw"), 44100, 2, 4000, 16, compression=b"ALAW"), 1, False),
        ("f.aiff", G.aiff(G.floats(pcm / 32768.0, 4, True), 44100, 2, 4000, 32, compression=b"fl32"), 4, True),
        ("g.aiff", G.aiff(G.floats(pcm / 32768.0, 8, True), 44100, 2, 4000, 64, compression=b"FL64"), 8, True),
    ]
    for name, data, width, is_float in cases:
        t = pcmio.PcmTrack(write(tmp_path, name, data))
        assert (t.samplerate, t.channels, t.frames, t.frames_declared) == (44100, 2, 4000, 4000), name
        got, st = t.decode_host(0, 4000)
        if name[0] in "abc":
            np.testing.assert_array_equal(got, pcm.astype(np.int16))
        elif is_float:
            np.testing.assert_array_equal(got, (pcm / 32768.0).astype(np.float32))
        else:
            table = G.ulaw_table() if name == "d.aiff" else G.alaw_table()
            codes = np.frombuffer(G.g711(pcm, "ulaw" if name == "d.aiff" else "alaw"), np.uint8)
            np.testing.assert_array_equal(got.reshape(-1), table[codes])
        t.close()


def test_aiff_cut_short_and_declared_lengths(tmp_path):
    pcm = G.test_signal(4000, 1, 24, seed=2)
    data = G.aiff(G.linear(pcm, 3, True), 48000, 1, 4000, 24)
    t = pcmio.PcmTrack(write(tmp_path, "cut.aiff", data[: len(data) - 3 * 1000 - 1]))
    assert (t.frames, t.frames_declared) == (2999, 4000)
    t.close()
    # numSampleFrames smaller than the SSND data: the declared count is what is read
    t = pcmio.PcmTrack(write(tmp_path, "short.aiff", G.aiff(G.linear(pcm, 3, True), 48000, 1, 4000, 24, declared=3000)))
    assert (t.frames, t.frames_declared) == (3000, 3000)
    t.close()


def test_aiff_rate_must_be_a_whole_number(tmp_path):
    data = G.aiff(G.linear(np.zeros(100, np.int64), 2, True), 44100.5, 1, 100, 16)
    with pytest.raises(pcmio.PcmFormatError, match="whole number"):
        pcmio.PcmTrack(write(tmp_path, "frac.aiff", data))
    assert pcmio._extended_rate(G.extended(44100)) == 44100 and pcmio._extended_rate(G.extended(8000)) == 8000


def test_files_written_by_aifc_read_back(tmp_path):
    rng = np.random.default_rng(0)
    for width, ch in ((1, 1), (2, 2), (3, 1), (4, 2)):
        frames = rng.integers(0, 256, 700 * width * ch, dtype=np.uint8).tobytes()
        for name in ("x.aiff", "x.aifc"):
            p = str(tmp_path / name)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)
                w = aifc.open(p, "wb")
                if name.endswith("aiff"):
                    w.aiff()
                w.setnchannels(ch)
                w.setsampwidth(width)
                w.setframerate(22050)
                w.writeframes(frames)
                w.close()
                r = aifc.open(p, "rb")
                back = r.readframes(r.getnframes())
                r.close()
            t = pcmio.PcmTrack(p)
            assert (t.samplerate, t.channels, t.frames, t.frames_declared) == (22050, ch, 700, 700)
            got, _ = t.decode_host(0, 700)
            x = np.frombuffer(back, np.uint8).reshape(-1, width)[:, ::-1]                      # big-endian -> little
            v = np.zeros((x.shape[0], 4), np.uint8)
            v[:, 4 - width:] = x
            ints = v.view("<i4").reshape(-1) >> (32 - 8 * width)
            want = ints.astype(np.int16) if width == 2 else (ints.astype(np.float64) / 2.0 ** (8 * width - 1)).astype(np.float32)
            np.testing.assert_array_equal(got.reshape(-1), want)
            t.close()


def test_files_written_by_sunau_read_back(tmp_path):
    rng = np.random.default_rng(1)
    for width, ch in ((1, 2), (2, 1), (3, 2), (4, 1)):
        frames = rng.integers(0, 256, 500 * width * ch, dtype=np.uint8).tobytes()
        p = str(tmp_path / "x.au")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            w = sunau.open(p, "wb")
            if width > 1:                                   # (sunau's default is mu-law)
                w.setcomptype("NONE", "not compressed")
            w.setnchannels(ch)
            w.setsampwidth(width)
            w.setframerate(16000)
            w.writeframes(frames)
            w.close()
            r = sunau.open(p, "rb")
            back = r.readframes(r.getnframes())
            r.close()
        t = pcmio.PcmTrack(p)
        assert (t.samplerate, t.channels, t.frames, t.frames_declared) == (16000, ch, 500, 500)
        got, _ = t.decode_host(0, 500)
        if width == 1:                                      # mu-law: sunau reads it back as int16
            assert t.fmt.codec == _lib.PCM_ULAW
            np.testing.assert_array_equal(got.reshape(-1), np.frombuffer(back, "<i2"))
            t.close()
            continue
        x = np.frombuffer(back, np.uint8).reshape(-1, width)[:, ::-1]
        v = np.zeros((x.shape[0], 4), np.uint8)
        v[:, 4 - width:] = x
        ints = v.view("<i4").reshape(-1) >> (32 - 8 * width)
        want = ints.astype(np.int16) if width == 2 else (ints.astype(np.float64) / 2.0 ** (8 * width - 1)).astype(np.float32)
        np.testing.assert_array_equal(got.reshape(-1), want)
        t.close()


def test_au_encodings_and_unknown_size(tmp_path):
    pcm = G.test_signal(3000, 2, 16, seed=3)
    for enc, data in ((1, G.g711(pcm, "ulaw")), (27, G.g711(pcm, "alaw")), (3, G.linear(pcm, 2, True)),
                      (6, G.floats(pcm / 32768.0, 4, True)), (7, G.floats(pcm / 32768.0, 8, True))):
        for unknown in (False, True):
            t = pcmio.PcmTrack(write(tmp_path, "a.au", G.au(data, 8000, 2, enc, unknown_size=unknown)))
            assert (t.samplerate, t.channels, t.frames, t.frames_declared) == (8000, 2, 3000, 3000)
            got, st = t.decode_host(0, 3000)
            assert st.samples == 3000
            if enc == 3:
                np.testing.assert_array_equal(got, pcm.astype(np.int16))
            t.close()
    full = G.au(G.linear(pcm, 2, True), 8000, 2, 3)
    t = pcmio.PcmTrack(write(tmp_path, "cut.au", full[:-4 * 100 - 2]))
    assert (t.frames, t.frames_declared) == (2899, 3000)
    t.close()
    with pytest.raises(pcmio.PcmFormatError, match="encoding 23"):
        pcmio.PcmTrack(write(tmp_path, "g721.au", G.au(b"\0" * 100, 8000, 1, 23)))


def test_w64_every_fmt_tag(tmp_path):
    pcm = G.test_signal(3000, 2, 16, seed=4)
    ima, ispb = G.ima_encode(pcm, 512)
    ms, mspb = G.ms_encode(pcm, 512)
    cases = [(G.fmt_body(1, 2, 32000, 16, 4), G.linear(pcm, 2), 3000, None),
             (G.fmt_body(1, 2, 32000, 8, 2), G.linear(pcm >> 8, 1, signed=False), 3000, None),
             (G.fmt_body(3, 2, 32000, 32, 8), G.floats(pcm / 32768.0, 4), 3000, None),
             (G.fmt_body(7, 2, 32000, 8, 2), G.g711(pcm, "ulaw"), 3000, None),
             (G.fmt_body(6, 2, 32000, 8, 2), G.g711(pcm, "alaw"), 3000, None),
             (G.fmt_ima(2, 32000, 512, ispb), ima, 3000, 3000),
             (G.fmt_ms(2, 32000, 512, mspb), ms, 3000, 3000)]
    for fmt, data, frames, fact in cases:
        t = pcmio.PcmTrack(write(tmp_path, "a.w64", G.w64(fmt, data, fact)))
        assert (t.container, t.samplerate, t.channels, t.frames, t.frames_declared) == ("w64", 32000, 2, frames, frames)
        t.close()
    t = pcmio.PcmTrack(write(tmp_path, "a.w64", G.w64(cases[0][0], cases[0][1])))
    assert t.raw_s16 and t.is_s16
    np.testing.assert_array_equal(t.decode_host(5, 100)[0], pcm[5:105].astype(np.int16))
    t.close()


def test_coded_wave_and_rf64(tmp_path):
    pcm = G.test_signal(10000, 1, 16, seed=5)
    ima, spb = G.ima_encode(pcm, 256)
    for rf64 in (False, True):
        t = pcmio.PcmTrack(write(tmp_path, "i.wav", G.wave(G.fmt_ima(1, 16000, 256, spb), ima, fact=10000, rf64=rf64)))
        assert (t.samplerate, t.channels, t.frames, t.frames_declared) == (16000, 1, 10000, 10000)
        t.close()
    # no fact: the blocks' capacity; a cut inside the last block: the frames whose codes are there
    nblk = len(ima) // 256
    t = pcmio.PcmTrack(write(tmp_path, "nofact.wav", G.wave(G.fmt_ima(1, 16000, 256, spb), ima)))
    assert t.frames == t.frames_declared == nblk * spb
    t.close()
    cut = G.wave(G.fmt_ima(1, 16000, 256, spb), ima, fact=10000)[: -256 - 100]
    t = pcmio.PcmTrack(write(tmp_path, "cut.wav", cut))
    assert t.frames == (nblk - 2) * spb + 1 + 2 * (156 - 4) and t.frames_declared == 10000
    got, st = t.decode_host(0, t.frames)
    assert st.samples == t.frames
    t.close()
    # the placeholder data size of a streaming writer: the file's length
    t = pcmio.PcmTrack(write(tmp_path, "ph.wav", G.wave(G.fmt_body(7, 1, 8000, 8, 1), G.g711(pcm, "ulaw"), data_size=0xFFFFFFFF)))
    assert (t.frames, t.frames_declared) == (10000, 10000)
    t.close()


def test_ms_fmt_coefficients_are_read_from_the_file(tmp_path):
    pcm = G.test_signal(2000, 1, 16, seed=6)
    coefs = (256, 0, 100, 20, -50, 300)
    data, spb = G.ms_encode(pcm, 200, coefs)
    t = pcmio.PcmTrack(write(tmp_path, "m.wav", G.wave(G.fmt_ms(1, 8000, 200, spb, coefs), data, fact=2000)))
    assert t.fmt.n_coefs == 3 and list(t.fmt.coefs[:6]) == list(coefs)
    got, _ = t.decode_host(0, 2000)
    np.testing.assert_array_equal(got, ms_oracle(data, 1, 200, spb, len(data) // 200, coefs)[:2000])
    t.close()


# ---------------------------------------------------------------- ranges and invalid headers
@pytest.mark.parametrize("kind", ["ima1", "ima2", "ms2", "ulaw", "be24"])
def test_ranges(lib, kind):
    ch = 2 if kind[-1] == "2" or kind in ("ulaw", "be24") else 1
    pcm = G.test_signal(20000, ch, 16, seed=7)
    if kind.startswith("ima"):
        data, spb = G.ima_encode(pcm, 256 * ch)
        f = pcmio.make_format(_lib.PCM_IMA_ADPCM, ch, block_align=256 * ch, samples_per_block=spb)
        ba = 256 * ch
    elif kind == "ms2":
        data, spb = G.ms_encode(pcm, 512)
        f = pcmio.make_format(_lib.PCM_MS_ADPCM, ch, block_align=512, samples_per_block=spb, coefs=G.MS_COEFS)
        ba = 512
    elif kind == "ulaw":
        data, spb, ba = G.g711(pcm, "ulaw"), 1, ch
        f = pcmio.make_format(_lib.PCM_ULAW, ch, 1)
    else:
        data, spb, ba = G.linear(pcm << 8, 3, True), 1, 3 * ch
        f = pcmio.make_format(_lib.PCM_LINEAR, ch, 3, big_endian=True)
    total = len(data) // ba * spb
    whole, _ = host_decode(lib, f, data, 0, total)
    for a, m in ((spb // 2 + 3, 1), (spb + 5, 3 * spb), (0, 1), (total - 1, 1), (7, total - 7), (total - spb - 9, spb + 9)):
        blk0 = a // spb
        blk1 = -(-(a + m) // spb)
        seg = data[blk0 * ba: blk1 * ba]
        got, st = host_decode(lib, f, seg, a, m, fill=77)
        assert (st.samples, st.reason, st.bad_block) == (m, 0, -1), (a, m)
        np.testing.assert_array_equal(got, whole[a: a + m])
    # the last block cut short: the frames whose codes are entirely present
    if spb > 1:
        blk = total // spb - 1
        for keep in (3, 4 * ch + 1, 4 * ch + 4 * ch, ba - 1):
            seg = data[blk * ba: blk * ba + keep]
            got, st = host_decode(lib, f, seg, blk * spb, spb, fill=77)
            k = pcmio.block_frames(f, keep)
            assert st.samples == k and st.end_sample == blk * spb + k and st.reason == (0 if k == spb else 2)
            np.testing.assert_array_equal(got[:k], whole[blk * spb: blk * spb + k])
            assert (got[k:] == 77).all()


@pytest.mark.parametrize("kind", ["ima", "ms"])
def test_invalid_block_header_ends_the_audio(lib, kind):
    ch = 2
    pcm = G.test_signal(12000, ch, 16, seed=8)
    if kind == "ima":
        data, spb = G.ima_encode(pcm, 512)
        f = pcmio.make_format(_lib.PCM_IMA_ADPCM, ch, block_align=512, samples_per_block=spb)
    else:
        data, spb = G.ms_encode(pcm, 512)
        f = pcmio.make_format(_lib.PCM_MS_ADPCM, ch, block_align=512, samples_per_block=spb, coefs=G.MS_COEFS)
    nblk = len(data) // 512
    whole, _ = host_decode(lib, f, data, 0, nblk * spb)
    bad = bytearray(data)
    if kind == "ima":
        bad[7 * 512 + 4 + 2] = 89                  # channel 1's step index of block 7
    else:
        bad[7 * 512 + 1] = 7                       # channel 1's predictor index of block 7 (7 pairs: 0-6)
    a = 2 * spb + 11
    got, st = host_decode(lib, f, bytes(bad[2 * 512:]), a, nblk * spb - a, fill=77)
    assert (st.reason, st.bad_block, st.samples, st.end_sample) == (1, 7, 7 * spb - a, 7 * spb)
    np.testing.assert_array_equal(got[: st.samples], whole[a: 7 * spb])
    assert (got[st.samples:] == 77).all()


def test_bad_formats_are_refused(lib):
    for f in (pcmio.make_format(_lib.PCM_LINEAR, 1, 5), pcmio.make_format(_lib.PCM_FLOAT, 1, 2),
              pcmio.make_format(_lib.PCM_LINEAR, 9, 2), pcmio.make_format(_lib.PCM_IMA_ADPCM, 1, block_align=3, samples_per_block=1),
              pcmio.make_format(_lib.PCM_IMA_ADPCM, 1, block_align=256, samples_per_block=600),
              pcmio.make_format(_lib.PCM_MS_ADPCM, 1, block_align=256, samples_per_block=100)):
        with pytest.raises(_lib.BuzzdetectHipError, match="BD_EINVAL"):
            host_decode(lib, f, b"\0" * 16, 0, 1)


# ---------------------------------------------------------------- routing, discovery, the host-only reader
def test_open_track_routes_by_magic(tmp_path):
    from buzzdetect_amd.flacio import FlacTrack, open_track
    from tools import flacgen as FG
    pcm = G.test_signal(3000, 1, 16, seed=9)
    ima, spb = G.ima_encode(pcm, 256)
    files = {"a.wav": (G.wav16(pcm, 8000), WavTrack), "b.wav": (G.wave(G.fmt_body(7, 1, 8000, 8, 1), G.g711(pcm, "ulaw")), pcmio.PcmTrack),
             "c.wav": (G.wave(G.fmt_ima(1, 8000, 256, spb), ima, fact=3000), pcmio.PcmTrack),
             "d.rf64": (G.wave(G.fmt_body(1, 1, 8000, 16, 2), G.linear(pcm, 2), rf64=True), WavTrack),
             "e.aiff": (G.aiff(G.linear(pcm, 2, True), 8000, 1, 3000, 16), pcmio.PcmTrack),
             "f.au": (G.au(G.linear(pcm, 2, True), 8000, 1, 3), pcmio.PcmTrack),
             "g.w64": (G.w64(G.fmt_body(1, 1, 8000, 16, 2), G.linear(pcm, 2)), pcmio.PcmTrack),
             "h.flac": (FG.encode(pcm, 8000, 16), FlacTrack),
             "misnamed.wav": (G.aiff(G.linear(pcm, 2, True), 8000, 1, 3000, 16), pcmio.PcmTrack)}
    for name, (data, cls) in files.items():
        t = open_track(write(tmp_path, name, data))
        assert type(t) is cls, name
        assert t.frames == 3000 and t.samplerate == 8000, name
        t.close()
    with pytest.raises(Exception, match="0x55"):
        open_track(write(tmp_path, "mp3.wav", G.wave(G.fmt_body(0x55, 1, 8000, 0, 1), b"\0" * 4000)))


def test_search_audio_finds_the_new_extensions(tmp_path):
    from buzzdetect_amd.analyze import search_audio
    names = ["a.wav", "b.FLAC", "c.aiff", "d.AU", "e.w64", "f.Rf64", "g.mp3", "h.aif", "i.aifc", "j.snd", "k.ogg"]
    for n in names:
        (tmp_path / n).write_bytes(b"x")
    got = sorted(os.path.basename(p) for p in search_audio(str(tmp_path)))
    assert got == ["a.wav", "b.FLAC", "c.aiff", "d.AU", "e.w64", "f.Rf64"]


def _host_tasks(tmp_path, name):
    from buzzdetect_amd import pipeline as P, results as R
    pipe = P.Pipeline(make_engine=None, classes=["a"], framehop_s=0.96, hop=15360, step=96, chunklength=7.1, framelength_s=0.96,
                      digits_time=2, digits_results=2, classes_out="all", threshold=None, readers=1, analyzers=1,
                      pin_memory=False, stream_buffer_depth=64)
    job = P.FileJob(str(tmp_path / name), name[:1], name, R.ResultFile(str(tmp_path / "out" / name)))
    pipe._plan_file(job)
    while not pipe.q_units.empty():
        pipe._read_unit(pipe.q_units.get())
    tasks = []
    while not pipe.q_analyze.empty():
        t = pipe.q_analyze.get()
        tasks.append((t.chunk, t.frames, t.nbytes, t.s16, bytes(pipe.pool.buffer(t.slot).numpy()[: t.nbytes])))
    return tasks, pipe.report


def test_host_reader_stage_gives_the_wav_chunks(tmp_path):
    """AIFF-16, mu-law WAV and IMA WAV through the planner and the host reader: the ChunkTasks and slot bytes of a 16-bit WAV
    of the decoded samples."""
    pcm = G.test_signal(16000 * 30, 1, 16, seed=10)
    ima, spb = G.ima_encode(pcm, 1024)
    files = {"a.aiff": G.aiff(G.linear(pcm, 2, True), 16000, 1, pcm.shape[0], 16),
             "b.wav": G.wave(G.fmt_body(7, 1, 16000, 8, 1), G.g711(pcm, "ulaw")),
             "c.wav": G.wave(G.fmt_ima(1, 16000, 1024, spb), ima, fact=pcm.shape[0])}
    for name, data in files.items():
        write(tmp_path, name, data)
        t = pcmio.PcmTrack(str(tmp_path / name))
        dec, _ = t.decode_host(0, t.frames)
        t.close()
        write(tmp_path, "w" + name[0] + ".wav", G.wav16(dec, 16000))
        got, _ = _host_tasks(tmp_path, name)
        want, _ = _host_tasks(tmp_path, "w" + name[0] + ".wav")
        assert got == want and len(got) == 5, name


def test_host_reader_stage_cut_short_mid_block(tmp_path, caplog):
    pcm = G.test_signal(16000 * 30, 1, 16, seed=11)
    ima, spb = G.ima_encode(pcm, 1024)
    full = G.wave(G.fmt_ima(1, 16000, 1024, spb), ima, fact=pcm.shape[0])
    write(tmp_path, "a.wav", full[: len(full) // 2 + 333])
    t = pcmio.PcmTrack(str(tmp_path / "a.wav"))
    dec, _ = t.decode_host(0, t.frames)
    t.close()
    assert 0 < dec.shape[0] < t.frames_declared and dec.shape[0] % spb not in (0, 1)
    wav = G.wav16(np.concatenate([dec, np.zeros((t.frames_declared - dec.shape[0], 1), np.int16)]), 16000)
    write(tmp_path, "w.wav", wav[: 44 + 2 * dec.shape[0]])
    msgs = {}
    for name in ("a.wav", "w.wav"):
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="buzzdetect"):
            got, _ = _host_tasks(tmp_path, name)
        msgs[name] = [r.getMessage().replace(name, "x") for r in caplog.records if "Unreadable audio" in r.getMessage()]
        msgs[name + "tasks"] = got
    assert msgs["a.wavtasks"] == msgs["w.wavtasks"]
    assert msgs["a.wav"] == msgs["w.wav"] and len(msgs["a.wav"]) == 1


def test_adpcm_with_other_than_4_bits_is_refused(tmp_path):
    pcm = G.test_signal(2000, 1, 16, seed=12)
    data, spb = G.ima_encode(pcm, 256)
    fmt = bytearray(G.fmt_ima(1, 8000, 256, spb))
    fmt[14:16] = struct.pack("<H", 3)
    with pytest.raises(pcmio.PcmFormatError, match="3-bit ADPCM"):
        pcmio.PcmTrack(write(tmp_path, "i3.wav", G.wave(bytes(fmt), data, fact=2000)))
    fmt = bytearray(G.fmt_ms(1, 8000, 256, G.ms_spb(256, 1)))
    fmt[14:16] = struct.pack("<H", 5)
    with pytest.raises(pcmio.PcmFormatError, match="5-bit ADPCM"):
        pcmio.PcmTrack(write(tmp_path, "m5.wav", G.wave(bytes(fmt), data, fact=2000)))


@pytest.mark.parametrize("kind", ["ima", "be24"])
def test_pieces_are_whole_blocks_below_the_byte_cap(tmp_path, monkeypatch, kind):
    pcm = G.test_signal(20000, 2, 16, seed=13)
    if kind == "ima":
        data, spb = G.ima_encode(pcm, 512)
        path = write(tmp_path, "i.wav", G.wave(G.fmt_ima(2, 8000, 512, spb), data, fact=20000))
    else:
        path = write(tmp_path, "a.aiff", G.aiff(G.linear(pcm << 8, 3, True), 8000, 2, 20000, 24))
    t = pcmio.PcmTrack(path)
    f = t.fmt
    monkeypatch.setattr(pcmio, "PIECE_BYTES", 3 * f.block_align + 5)
    for a, n in ((0, 20000), (1234, 5000), (19999, 1), (f.samples_per_block, 3 * f.samples_per_block)):
        ps = t.pieces(a, n)
        assert ps[0][0] == a and sum(m for _, m in ps) == n
        assert all(p + m == q for (p, m), (q, _) in zip(ps, ps[1:]))
        for p, m in ps:
            lo, hi = t.byte_range(p, m)
            assert hi - lo <= 3 * f.block_align
            if p != a:
                assert p % f.samples_per_block == 0
    t.close()


def test_host_reader_stage_in_small_pieces_gives_the_same_chunks(tmp_path, monkeypatch):
    pcm = G.test_signal(16000 * 30, 1, 16, seed=14)
    ima, spb = G.ima_encode(pcm, 1024)
    write(tmp_path, "c.wav", G.wave(G.fmt_ima(1, 16000, 1024, spb), ima, fact=pcm.shape[0]))
    write(tmp_path, "d.aiff", G.aiff(G.linear(pcm << 8, 3, True), 16000, 1, pcm.shape[0], 24))
    whole = {n: _host_tasks(tmp_path, n)[0] for n in ("c.wav", "d.aiff")}
    monkeypatch.setattr(pcmio, "PIECE_BYTES", 7 * 1024 + 3)
    for name in ("c.wav", "d.aiff"):
        assert _host_tasks(tmp_path, name)[0] == whole[name] and len(whole[name]) == 5
