"""Recordings of three to eight channels without a GPU: what the channel mean is (np.mean(axis=1) in float32, the running sum
in channel order the kernels' general paths compute), that the three decoders deliver [frames, channels] frames in the
interleaving the resamplers read, and bd_resample_any_host - which shares ar_mono with anyrate_kernel - against the float64
oracle at the channel counts tests/test_anyrate_host.py leaves out."""
import struct

import numpy as np
import pytest

from oracle import resample_oracle as RO
from tests import multichannel_cases as MC
from tools import flacgen as FG
from tools import pcmgen as PG


@pytest.mark.parametrize("channels", [3, 4, 5, 6, 7])
def test_downmix_is_the_in_order_float32_mean_below_eight_channels(channels):
    """RO.downmix is np.mean(axis=1) of float32: below eight channels NumPy adds a row's values in order, so the running
    sum in channel order divided by the count has the same bits - for float PCM and for 16-bit PCM as value / 32768."""
    for x in (MC.marked(4099, channels, channels), MC.as_float(MC.marked_s16(4099, channels, channels)),
              MC.as_float(MC.full_scale_s16(4099, channels, channels))):
        want = RO.downmix(x)
        assert want.dtype == np.float32 and want.shape == (4099,)
        assert np.array_equal(want, np.mean(x, axis=1))
        assert np.array_equal(want.view(np.uint32), MC.in_order_mean(x).view(np.uint32))


def test_downmix_of_eight_channels_is_order_free_for_16_bit_pcm_only():
    """At eight channels NumPy sums pairwise.  Every partial sum of eight 16-bit values / 32768 is a multiple of 2^-15 below
    2^3, exact in float32, so no order of additions changes the bits; for float PCM the two orders round differently: seven
    additions and a division each, every one within 2^-24 of a value no larger than S = sum |x|, so the means differ by
    less than 2 * 8 * 2^-24 * S / 8 - which, where the channels cancel, is thousands of ulps of the mean (4096 on this
    signal).  Hence the kernels restate NumPy's order (np_row_sum) and not the running sum."""
    for q in (MC.marked_s16(4099, 8, 8), MC.full_scale_s16(4099, 8, 8)):
        assert np.array_equal(RO.downmix(MC.as_float(q)).view(np.uint32), MC.in_order_mean(q).view(np.uint32))
        assert np.array_equal(RO.downmix(MC.as_float(q)).astype(np.float64), q.astype(np.float64).sum(axis=1) / 8 / 32768)
    x = MC.marked(100003, 8, 100003)
    want, got = RO.downmix(x), MC.in_order_mean(x)
    d = np.abs(want.astype(np.float64) - got.astype(np.float64))
    assert d.max() > 0 and (d <= 2.0 ** -20 * np.abs(x).astype(np.float64).sum(axis=1) / 8).all()
    assert (d / np.spacing(np.abs(want))).max() > 100


@pytest.mark.parametrize("channels", [3, 7, 8, 9, 15, 16, 17, 24, 31, 128])
def test_np_row_sum_is_the_order_numpy_adds_a_row_in(channels):
    """The restatement of np_row_sum in float32 NumPy, one operation at a time, has the bits of np.mean(axis=1) up to 128
    channels (where NumPy starts to halve the row): whole blocks of eight, a ragged tail, a frame of -0.0."""
    for x in (MC.marked(4099, channels, channels), MC.as_float(MC.marked_s16(4099, channels, channels)),
              np.full((3, channels), -0.0, np.float32)):
        assert np.array_equal(RO.downmix(x).view(np.uint32), MC.row_sum_mean(x).view(np.uint32))


def counter(frames, channels):
    """sample = 16 * frame + channel: every position of the interleaved stream holds another value."""
    assert channels <= 16 and 16 * frames + channels < 32768
    return (16 * np.arange(frames)[:, None] + np.arange(channels)[None, :]).astype(np.int16)


def test_wav_extensible_five_channels_come_back_frame_by_frame(tmp_path):
    from buzzdetect_amd.wavio import WavTrack
    pcm = counter(2000, 5)
    guid = struct.pack("<H", 1) + bytes.fromhex("000000001000800000aa00389b71")           # KSDATAFORMAT_SUBTYPE_PCM
    fmt = PG.fmt_body(0xFFFE, 5, 48000, 16, 10, ext=struct.pack("<HI", 16, 0x37) + guid)
    assert len(fmt) == 40
    (tmp_path / "e.wav").write_bytes(PG.wave(fmt, pcm.astype("<i2").tobytes()))
    t = WavTrack(str(tmp_path / "e.wav"))
    assert (t.channels, t.frames, t.samplerate, t.is_s16) == (5, 2000, 48000, True)
    got = t.read(2000, keep_s16=True)
    t.seek(0)
    as_f32 = t.read(2000)
    t.close()
    assert got.shape == (2000, 5) and np.array_equal(got, pcm)
    assert as_f32.shape == (2000, 5) and np.array_equal(as_f32, pcm.astype(np.float32) / 32768.0)


def test_aiff_six_channels_come_back_frame_by_frame(tmp_path):
    from buzzdetect_amd.pcmio import PcmTrack
    pcm = counter(2000, 6)
    (tmp_path / "s.aiff").write_bytes(PG.aiff(PG.linear(pcm, 2, True), 48000, 6, 2000, 16))
    t = PcmTrack(str(tmp_path / "s.aiff"))
    got, st = t.decode_host(0, t.frames)
    part, _ = t.decode_host(777, 100)
    t.close()
    assert st.samples == 2000 and got.dtype == np.int16 and got.shape == (2000, 6) and np.array_equal(got, pcm)
    assert np.array_equal(part, pcm[777:877])


def test_flac_eight_channels_come_back_frame_by_frame(tmp_path):
    from buzzdetect_amd.flacio import FlacTrack
    pcm = counter(2000, 8)
    (tmp_path / "o.flac").write_bytes(FG.encode(pcm, 48000, 16, blocksize=576, subframe_kind=("fixed", 2)))
    t = FlacTrack(str(tmp_path / "o.flac"))
    got, st = t.decode_host(0, t.frames)
    part, _ = t.decode_host(777, 100)
    t.close()
    assert st.samples == 2000 and got.dtype == np.int16 and got.shape == (2000, 8) and np.array_equal(got, pcm)
    assert np.array_equal(part, pcm[777:877])


def any_host(x, rate_in):
    from buzzdetect_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(x)
    n, channels = x.shape
    m = lib.bd_resample_length(n, rate_in, 16000)
    out = np.full(max(m, 1), np.nan, np.float32)
    rc = lib.bd_resample_any_host(x.ctypes.data, int(x.dtype == np.int16), n, channels, rate_in, 16000, out.ctypes.data)
    assert rc == 0, lib.bd_last_error()
    return out[:m]


@pytest.mark.parametrize("channels", [3, 5, 7, 8])
@pytest.mark.parametrize("rate_in", [47999, 768000])
def test_anyrate_host_restatement_matches_the_f64_oracle(rate_in, channels):
    """The channel counts test_host_restatement_matches_the_f64_oracle does not reach, both sample types, on channels that
    can be told apart: one frame, less than a filter span, a ragged twentieth of a second - within its 5e-6."""
    for n in (1, 97, int(0.05 * rate_in) + 37):
        for x in (MC.marked(n, channels, n + channels), MC.marked_s16(n, channels, n + channels)):
            got, want = any_host(x, rate_in), MC.oracle(x, rate_in)
            assert got.shape == want.shape == (-(-n * 16000 // rate_in),)
            err = float(np.abs(got - want).max())
            print(f"{rate_in} Hz, {channels} channels, {n} frames, {x.dtype}: max |d| = {err:.3g}")
            assert err < 5e-6, (n, x.dtype, err)
