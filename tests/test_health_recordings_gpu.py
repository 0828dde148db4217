"""health.health_recordings end to end on the GPU: a folder with a 16-bit mono WAV at 16 kHz, a 16-bit stereo WAV at 48 kHz and a
float32 WAV at 44.1 kHz, each with a clipped burst in bin 0, digital silence over the whole of bin 2 and a tone in noise
elsewhere, read in chunks of 1.92 s at bin_s = 1.0 (every second bin lies in two chunks), against HealthMeter's host path on the
same decoded samples, chunk by chunk as analyze cuts them."""
import struct
import wave

import numpy as np
import pytest

from buzzdetect_amd import calls, framing, health

pytestmark = pytest.mark.gpu

CHUNK = 1.92
BIN_S = 1.0


def write_wav(path, pcm16, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm16.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm16, "<i2").tobytes())


def write_float_wav(path, x, rate):
    data = np.asarray(x, "<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, x.shape[1], rate, rate * 4 * x.shape[1], 4 * x.shape[1], 32)
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
                + b"data" + struct.pack("<I", len(data)) + data)


def recording(seconds, rate, ch, seed):
    """float64 [n, ch] in (-0.5, 0.5): a tone in noise; full scale for 0.01 s from 0.5 s on (channel 0); zeros over bin 2."""
    n = int(seconds * rate)
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None] / rate
    x = 0.3 * np.sin(2 * np.pi * 440.0 * t + np.arange(ch)[None, :]) + 0.05 * rng.standard_normal((n, ch))
    x[int(0.5 * rate):int(0.51 * rate), 0] = 2.0
    x[2 * rate:3 * rate] = 0.0
    return x


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("health")
    audio = root / "audio"
    (audio / "site").mkdir(parents=True)
    a = (np.clip(recording(5.0, 16000, 1, 1), -1, 1 - 2.0 ** -15) * 32768.0).round().astype(np.int16)
    b = (np.clip(recording(4.0, 48000, 2, 2), -1, 1 - 2.0 ** -15) * 32768.0).round().astype(np.int16)
    c = np.clip(recording(3.5, 44100, 1, 3), -1, 1).astype(np.float32)
    write_wav(audio / "a.wav", a, 16000)
    write_wav(audio / "site" / "b.wav", b, 48000)
    write_float_wav(audio / "c.wav", c, 44100)
    return str(audio), {"a": (a, 16000), "site/b": (b, 48000), "c": (c, 44100)}, root


def host_health(engine, meter, x, rate):
    """HealthMeter's host path over analyze's chunks; the 16 kHz mono chunk is the engine's own resampling of those samples."""
    import torch
    levels, spectra = [], []
    for edge in framing.gaps_to_chunklist([(0, x.shape[0] / rate)], framing.round_chunklength(CHUNK)):
        lo, hi = framing.chunk_sample_range(edge, rate)
        hi = min(hi, x.shape[0])
        if hi <= lo:
            continue
        part = np.ascontiguousarray(x[lo:hi])
        levels.append(meter.levels_host(part, rate, lo))
        pcm = engine.resample(torch.from_numpy(part), rate, 16000).cpu().numpy()      # (what dataset._read_chunks does with these)
        spectra.append(meter.spectrum_host(pcm, float(edge[0])))
    return health.recording_health(health.merge_levels(levels), health.merge_spectrum(spectra, meter.n_bands), rate, meter.bin_ticks)


def test_health_recordings_is_the_host_path_over_analyzes_chunks(engine, folder):
    dir_audio, pcm, root = folder
    got = health.health_recordings(dir_audio, bin_s=BIN_S, engine=engine, chunklength=CHUNK)
    assert sorted(got.recordings) == sorted(pcm) and got.messages == [] and got.bin_s == BIN_S
    meter = health.HealthMeter(bin_s=BIN_S)
    for ident, (x, rate) in pcm.items():
        want, mine = host_health(engine, meter, x, rate), got.recordings[ident]
        for name in ("bin_start", "seconds", "peak_dbfs", "rms_dbfs", "dc", "samples", "full", "clipped", "clip_runs", "flat", "flat_runs",
                     "nonfinite", "frames", "bad_frames", "band_power"):
            assert np.array_equal(getattr(mine, name), getattr(want, name), equal_nan=True), (ident, name)
        burst = int(0.51 * rate) - int(0.5 * rate)
        assert mine.clipped[:, 0].tolist() == [burst] + [0] * (mine.bin_start.shape[0] - 1) and mine.clip_runs[0, 0] == 1
        assert (mine.flat[2] == rate).all() and (mine.rms_dbfs[2] == -np.inf).all() and (mine.flat_runs[2] == 1).all()
        assert mine.bin_start.tolist() == [float(b) for b in range(int(np.ceil(x.shape[0] / rate)))]
        assert mine.frames.sum() + mine.bad_frames.sum() > 25 * (x.shape[0] // rate) and not mine.bad_frames.any()
        # the tone's band (250..500 Hz holds 440 Hz) stands out of its neighbours wherever there is sound
        loud = [b for b in range(mine.bin_start.shape[0]) if b != 2 and mine.frames[b] > 4]
        assert (mine.band_db[loud, 3] > mine.band_db[loud, 2] + 10).all() and (mine.band_db[loud, 3] > mine.band_db[loud, 5] + 10).all()


def test_flags_csv_and_the_bins_of_call_recordings(engine, folder):
    dir_audio, pcm, root = folder
    got = health.health_recordings(dir_audio, bin_s=BIN_S, engine=engine, chunklength=CHUNK)
    for ident, rows in got.flags().items():
        assert [b for b, usable, _ in rows if not usable] == [0.0, 2.0], ident
        assert rows[0][2] == ("clipped",) and rows[2][2] == ("flat", "silent")
    got.to_csv(str(root / "out"))
    for ident, (x, rate) in pcm.items():
        bins = got.recordings[ident].bin_start.shape[0]
        lines = (root / "out" / (ident + health.SUFFIX_HEALTH)).read_text().splitlines()
        assert lines[0] == ",".join(health.HEALTH_COLUMNS) and len(lines) == 1 + bins * x.shape[1]
        silent = [l for l in lines[1:] if l.startswith("2.0,")]
        assert silent == [f"2.0,{c},1.0,-inf,-inf,0.000000,0,0,0,{rate},1,0" for c in range(x.shape[1])]
        assert lines[1].split(",")[:3] == ["0.0", "0", "1.0"] and lines[1].split(",")[7] == str(int(0.51 * rate) - int(0.5 * rate))
        ltsa = (root / "out" / (ident + health.SUFFIX_LTSA)).read_text().splitlines()
        assert ltsa[0].startswith("bin_start,frames,bad_frames,band_0_62.5,band_62.5_125,") and len(ltsa) == 1 + bins
        assert ltsa[0].endswith("band_4000_8000") and all(len(l.split(",")) == 11 for l in ltsa)
    called = calls.call_recordings(dir_audio, classes=["ins_buzz"], thresholds={"ins_buzz": 0.0}, bin_s=BIN_S, engine=engine, chunklength=CHUNK)
    for ident in pcm:
        # call_recordings lists the bins that hold windows; each of them is a bin of the health table, with the same start
        theirs, mine = called.bins[ident].bin_start.tolist(), got.recordings[ident].bin_start.tolist()
        assert theirs and set(theirs) <= set(mine) and theirs == mine[:len(theirs)]


def test_a_store_is_refused(tmp_path):
    (tmp_path / "store.json").write_text("{}")
    with pytest.raises(ValueError, match="holds no audio"):
        health.health_recordings(str(tmp_path))
