"""The any-ratio resampler on the device (include/buzzdetect_anyrate.h): anyrate_kernel against its host restatement bit for
bit, bd_resample's routes untouched, determinism, and analyze() on recordings whose rates bd_resample refuses."""
import functools
import wave

import numpy as np
import pytest

from oracle import resample_oracle as RO

pytestmark = pytest.mark.gpu

RATES = [47999, 44099, 22051, 7999, 250001, 768000, 1024000, 16000 * 4099]


@pytest.fixture(autouse=True)
def one_filter_design_per_ratio(monkeypatch):
    """RO.resample designs its filter on every call (seconds for an irreducible ratio); the same arrays, kept per ratio."""
    monkeypatch.setattr(RO, "taps", functools.lru_cache(maxsize=2)(RO.taps))


def host(x, rate_in, rate_out=16000):
    from buzzdetect_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(x)
    n, channels = x.shape[0], (1 if x.ndim == 1 else x.shape[1])
    m = lib.bd_resample_length(n, rate_in, rate_out)
    out = np.full(max(m, 1), np.nan, np.float32)
    assert lib.bd_resample_any_host(x.ctypes.data, int(x.dtype == np.int16), n, channels, rate_in, rate_out, out.ctypes.data) == 0, \
        lib.bd_last_error()
    return out[:m]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("rate_in", RATES + [-47999])
def test_kernel_equals_host_restatement_bit_for_bit(engine, rate_in):
    """Every rate bd_resample refuses (and 16 000 -> 47 999 Hz, listed as -47999) x {s16, f32} x {1, 2, 3, 6} channels."""
    rate_in, rate_out = (rate_in, 16000) if rate_in > 0 else (16000, -rate_in)
    rng = np.random.default_rng(rate_in)
    n = int(0.05 * rate_in) + 301 if rate_in < 10 ** 7 else 2 * 4099 * 170     # the last: 340 outputs of 774 k taps each
    for channels in (1, 2, 3, 6):
        x = rng.uniform(-1.0, 1.0, (n, channels)).astype(np.float32)
        q = np.floor(x * 32768.0).astype(np.int16)
        if channels == 1:
            x, q = x[:, 0], q[:, 0]
        for samples in (x, q):
            got = engine.resample(samples, rate_in, rate_out).cpu().numpy()
            assert same_bits(got, host(samples, rate_in, rate_out)), (rate_in, channels, samples.dtype)


@pytest.mark.parametrize("rate_in,seconds", [(47999, 600), (768000, 60)])
def test_one_long_call(engine, rate_in, seconds):
    """600 s of 47 999 Hz and 60 s of 768 kHz mono 16-bit PCM in one call (j down beyond 2^32): the whole output equals the
    host restatement bit for bit, and stretches at the start, the middle and the end are within 5e-6 of the oracle run on
    the matching piece of the input (the pattern of tests/test_resample.py:331-357)."""
    rng = np.random.default_rng(seconds)
    n = rate_in * seconds + 17
    q = rng.integers(-20000, 20000, n, dtype=np.int16)
    got = engine.resample(q, rate_in).cpu().numpy()
    up, down = RO.ratio(rate_in, 16000)
    _, half = RO.taps(up, down)
    n_out = -(-n * up // down)
    assert got.shape[0] == n_out
    reach = half // up + 2
    block = 3000
    for j0 in (0, (n_out // 2) // up * up, n_out - block):
        j1 = min(j0 + block, n_out)
        i0 = max(0, j0 * down // up - reach)
        i0 -= i0 % down                                      # keep the piece's phase: i0 a multiple of `down` = whole outputs
        i1 = min(n, j1 * down // up + reach + down)
        ref = RO.resample(q[i0:i1].astype(np.float32) / 32768.0, rate_in)
        off = i0 * up // down
        err = float(np.abs(got[j0:j1] - ref[j0 - off:j1 - off]).max())
        print(f"{rate_in} Hz, outputs [{j0}, {j1}): max |d| = {err:.3g}")
        assert err < 5e-6, (j0, j1)
    assert same_bits(got, host(q, rate_in))


@pytest.mark.parametrize("quality", ["hq", "scipy"])
def test_existing_routes_are_bd_resample_bit_for_bit(engine, quality):
    import torch
    lib, handle = engine._lib, engine._handle
    engine.set_resample_quality(quality)
    try:
        for rate_in in (16000, 32000, 44100, 48000, 96000):
            rng = np.random.default_rng(rate_in)
            n = rate_in // 2 + 13
            x = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)).to(engine.device)
            q = torch.from_numpy(rng.integers(-32768, 32767, (n, 2), dtype=np.int16)).to(engine.device)
            m = lib.bd_resample_length(n, rate_in, 16000)
            stream = torch.cuda.current_stream(engine.device).cuda_stream
            for t, old, new in ((x, lib.bd_resample, lib.bd_resample_any), (q, lib.bd_resample_s16, lib.bd_resample_any_s16)):
                a = torch.full((m,), float("nan"), device=engine.device)
                b = torch.full((m,), float("nan"), device=engine.device)
                with torch.cuda.device(engine.device):
                    assert old(handle, t.data_ptr(), n, 2, rate_in, 16000, a.data_ptr(), stream) == 0
                    assert new(handle, t.data_ptr(), n, 2, rate_in, 16000, b.data_ptr(), stream) == 0
                torch.cuda.synchronize()
                assert same_bits(a.cpu().numpy(), b.cpu().numpy()), (rate_in, quality, t.dtype)
    finally:
        engine.set_resample_quality("hq")


def test_bd_resample_still_refuses_and_scipy_has_no_anyrate_form(engine):
    import torch
    from buzzdetect_amd._lib import BuzzdetectHipError
    lib, handle = engine._lib, engine._handle
    x = torch.zeros(4800, device=engine.device)
    out = torch.zeros(1600, device=engine.device)
    stream = torch.cuda.current_stream(engine.device).cuda_stream
    assert lib.bd_resample(handle, x.data_ptr(), 4799, 1, 47999, 16000, out.data_ptr(), stream) < 0
    engine.set_resample_quality("scipy")
    try:
        with pytest.raises(BuzzdetectHipError, match="any-ratio"):
            engine.resample(np.zeros(4799, np.float32), 47999)
    finally:
        engine.set_resample_quality("hq")


def test_same_bits_alone_after_another_ratio_and_on_a_second_engine(engine):
    import torch
    from buzzdetect_amd.engine import HipEngine
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, (24000, 2)).astype(np.float32)
    first = engine.resample(x, 47999).cpu().numpy()
    engine.resample(rng.uniform(-1.0, 1.0, 40000).astype(np.float32), 768000)
    engine.resample(x, 44099)
    again = engine.resample(x, 47999).cpu().numpy()
    assert same_bits(first, again)
    other = HipEngine()
    try:
        side = torch.cuda.Stream(device=other.device)
        with torch.cuda.stream(side):
            a = other.resample(x, 47999)
            b = other.resample(x, 47999)
        side.synchronize()
        assert same_bits(first, a.cpu().numpy()) and same_bits(first, b.cpu().numpy())
    finally:
        other.close()


def _write_wav(path, x, rate):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    q = (np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(q.tobytes())
    return q if q.shape[1] > 1 else q[:, 0]


def test_analyze_reads_the_rates_bd_resample_refuses(engine, tmp_path):
    """A 47 999 Hz stereo, a 768 kHz mono and a 16 000 * 4099 Hz mono recording of a few windows: all analysed, none
    skipped, every CSV value the formatted logit engine.predict gives for the ORACLE-resampled chunk (1e-4 gate, then the
    half step of the CSV's two decimals)."""
    import pandas as pd
    from buzzdetect_amd.analyze import analyze
    audio, out = tmp_path / "audio", tmp_path / "out"
    audio.mkdir()
    rng = np.random.default_rng(11)
    pcm = {}
    for name, rate, channels, seconds in (("odd", 47999, 2, 2.5), ("ultra", 768000, 1, 2.5), ("mhz", 16000 * 4099, 1, 2.0)):
        n = int(rate * seconds)
        t = np.arange(n) / rate
        x = np.stack([0.3 * np.sin(2 * np.pi * (230.0 + 90 * c) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) for c in range(channels)], 1)
        x += 0.05 * rng.standard_normal((n // 64 + 1, channels)).repeat(64, 0)[:n]
        pcm[name] = (rate, _write_wav(audio / f"{name}.wav", x.astype(np.float32), rate))
        del x, t
    rep = analyze("model_general_v3", classes_out=["ins_buzz", "ambient_rain"], framehop_prop=1, chunklength=3,
                  dir_audio=str(audio), dir_out=str(out), engine=engine)
    assert rep.files_done == 3 and rep.files_skipped == 0
    assert not any("not supported" in m for m in rep.messages), rep.messages
    cols = {"activation_ins_buzz": engine.classes.index("ins_buzz"), "activation_ambient_rain": engine.classes.index("ambient_rain")}
    for name, (rate, q) in pcm.items():
        csv = pd.read_csv(out / f"{name}_buzzdetect.csv")
        assert len(csv) >= 2, name
        mono = RO.resample(q.astype(np.float32) / 32768.0, rate).astype(np.float32)
        ref = engine.predict(mono, 0.96).numpy()
        for col, k in cols.items():
            err = float(np.abs(csv[col].to_numpy() - ref[:len(csv), k]).max())
            print(f"{name}: {col} max |d| = {err:.4g}")
            assert err <= 0.005 + 1e-4, (name, col)
