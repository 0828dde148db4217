"""The any-ratio resampler (include/buzzdetect_anyrate.h) without a GPU: the host-only query, and bd_resample_any_host - the
kernel's coefficient rows, lane split and order of additions restated on the host - against the float64 oracle
(oracle/resample_oracle.py, quality "hq").  The bounds are those tests/test_resample.py holds the HQ device path to."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import resample_oracle as RO

HQ, SCIPY = 1, 0
# rate_in -> rate_out pairs bd_resample refuses: ratios that do not reduce to <= 4096, HQ decimations beyond ~43 : 1
PAIRS = [(47999, 16000), (44099, 16000), (22051, 16000), (7999, 16000), (250001, 16000), (768000, 16000), (1024000, 16000),
         (16000 * 4099, 16000), (16000, 47999)]


@pytest.fixture(scope="module")
def lib():
    from buzzdetect_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def one_filter_design_per_ratio(monkeypatch):
    """RO.resample designs its filter on every call (9 M taps of np.i0 for an irreducible ratio: seconds); the same arrays,
    kept for the two most recent ratios."""
    monkeypatch.setattr(RO, "taps", functools.lru_cache(maxsize=2)(RO.taps))


def host(lib, x, rate_in, rate_out=16000):
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.int16)
    n, channels = x.shape[0], (1 if x.ndim == 1 else x.shape[1])
    m = lib.bd_resample_length(n, rate_in, rate_out)
    out = np.full(max(m, 1), np.nan, np.float32)
    rc = lib.bd_resample_any_host(x.ctypes.data if n else None, int(x.dtype == np.int16), n, channels, rate_in, rate_out,
                                  out.ctypes.data)
    assert rc == 0, lib.bd_last_error()
    return out[:m]


def oracle(x, rate_in, rate_out=16000):
    x = np.asarray(x)
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768.0
    return RO.resample(x, rate_in, rate_out, dtype=np.float64, quality="hq")


def span_of(rate_in, rate_out):
    """Input samples either side of an output's centre."""
    up, down = RO.ratio(rate_in, rate_out)
    max_rate = max(up, down)
    fp, fs = (e / max_rate for e in RO.hq_band_edges())
    half = (int(np.ceil((RO.HQ_DESIGN_ATTENUATION_DB - 7.95) / (2.285 * np.pi * (fs - fp)))) + 1) // 2
    return half // up + 2


def test_query_accepts_every_rate(lib):
    for rate_in, rate_out in PAIRS:
        assert lib.bd_anyrate_supported(rate_in, rate_out, HQ) == 1, (rate_in, rate_out)
    # what tests/test_resample.py lists as supported by bd_resample, at both qualities
    for rate_in in (16000, 8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000):
        for quality in (HQ, SCIPY):
            if lib.bd_resample_supported(rate_in, 16000, quality) == 1:
                assert lib.bd_anyrate_supported(rate_in, 16000, quality) == 1, (rate_in, quality)
        assert lib.bd_anyrate_supported(rate_in, 16000, HQ) == 1, rate_in
    # every rate of the stated range, both ways (host only, no table is built): the ends, and a sweep of odd steps
    for rate in [2000, 2001, 4095999, 4096000] + list(range(2000, 4096000, 7919)):
        assert lib.bd_anyrate_supported(rate, 16000, HQ) == 1, rate
        assert lib.bd_anyrate_supported(16000, rate, HQ) == 1, rate
    assert lib.bd_anyrate_supported(768000, 16000, SCIPY) == 1          # bd_resample's own vector kernel takes it
    assert lib.bd_anyrate_supported(47999, 16000, SCIPY) == 0           # truthfully: that filter has no any-ratio form
    assert lib.bd_anyrate_supported(1 << 27, 16000, HQ) == 0            # outside the stated range
    assert lib.bd_anyrate_supported(0, 16000, HQ) < 0 and lib.bd_anyrate_supported(48000, 0, HQ) < 0
    assert lib.bd_anyrate_supported(48000, 16000, 7) < 0
    assert lib.bd_anyrate_abi_version() == 1


def test_bd_resample_keeps_its_refusals(lib):
    assert lib.bd_resample_supported(768000, 16000, HQ) == 0
    assert lib.bd_resample_supported(1024000, 16000, HQ) == 0
    assert lib.bd_resample_supported(16000 * 4099, 16000, HQ) == 0
    assert lib.bd_resample_supported(47999, 16000, HQ) == 0


def test_host_restatement_refuses_by_name(lib):
    x = np.zeros(8, np.float32)
    out = np.zeros(8, np.float32)
    assert lib.bd_resample_any_host(x.ctypes.data, 0, 8, 1, 1 << 27, 16000, out.ctypes.data) < 0
    assert b"any-ratio range" in lib.bd_last_error()
    assert lib.bd_resample_any_host(x.ctypes.data, 0, 8, 0, 47999, 16000, out.ctypes.data) < 0
    assert lib.bd_resample_any_host(None, 0, 8, 1, 47999, 16000, out.ctypes.data) < 0


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_host_restatement_matches_the_f64_oracle(lib, rate_in, rate_out):
    """Uniform noise in [-1, 1), 1 / 2 / 6 channels, float32 and 16-bit PCM; no input, one sample, less than one filter span
    and a ragged quarter of a second: within 5e-6 of the oracle (tests/test_resample.py:175)."""
    rng = np.random.default_rng(rate_in + rate_out)
    span = span_of(rate_in, rate_out)
    worst = 0.0
    for n in (0, 1, max(2, span // 3), int(0.25 * rate_in) + 37):
        for channels in (1, 2, 6):
            x = rng.uniform(-1.0, 1.0, (n, channels)).astype(np.float32)
            q = np.floor(x * 32768.0).astype(np.int16)
            if channels == 1:
                x, q = x[:, 0], q[:, 0]
            for samples in (x, q):
                got, want = host(lib, samples, rate_in, rate_out), oracle(samples, rate_in, rate_out)
                assert got.shape == want.shape == (-(-n * rate_out // rate_in),), (n, channels, samples.dtype)
                err = float(np.abs(got - want).max()) if got.size else 0.0
                print(f"{rate_in} -> {rate_out} n={n} channels={channels} {samples.dtype}: max |d| = {err:.3g}")
                worst = max(worst, err)
                assert err < 5e-6, (n, channels, samples.dtype, err)
    print(f"{rate_in} -> {rate_out}: worst {worst:.3g}")


@pytest.mark.parametrize("rate_in", [47999, 768000])
@pytest.mark.parametrize("where", [0.9, 1.1])
def test_full_scale_tones_either_side_of_nyquist(lib, rate_in, where):
    """A full-scale sine at 0.9 (kept) and 1.1 (removed) of the lower Nyquist: within 1.5e-6 of the oracle
    (tests/test_resample.py:281-291)."""
    n = int(0.25 * rate_in) + 11
    x = np.sin(2 * np.pi * where * 8000.0 * np.arange(n) / rate_in).astype(np.float32)
    got, want = host(lib, x, rate_in), oracle(x, rate_in)
    err = float(np.abs(got - want).max())
    print(f"{rate_in} Hz, tone at {where} Nyquist: max |d| = {err:.3g}, peak out {np.abs(want).max():.3g}")
    assert (np.abs(want[400:-400]).max() > 0.9) if where < 1 else (np.abs(want[400:-400]).max() < 1e-5)
    assert err < 1.5e-6


@pytest.mark.parametrize("rate_in", [47999, 768000])
@pytest.mark.parametrize("level", [1.0, 1e-2, 1e-4])
def test_quiet_input_keeps_its_relative_accuracy(lib, rate_in, level):
    """tests/test_resample.py:204: within 5e-6 * level + 1e-9."""
    rng = np.random.default_rng(7)
    x = (level * rng.uniform(-1.0, 1.0, int(0.25 * rate_in) + 5)).astype(np.float32)
    got, want = host(lib, x, rate_in), oracle(x, rate_in)
    err = float(np.abs(got - want).max())
    print(f"{rate_in} Hz at level {level}: max |d| = {err:.3g}")
    assert err < 5e-6 * level + 1e-9


def test_pipeline_planner_asks_the_anyrate_query(lib):
    """_rate_supported answers for the quality the engines run: the rates bd_resample refuses are planned at "hq", and
    skipped at "scipy", which has no any-ratio form."""
    from buzzdetect_amd.pipeline import Pipeline
    hq, scipy = Pipeline.__new__(Pipeline), Pipeline.__new__(Pipeline)
    hq.resample_quality, hq._rates = HQ, {}
    scipy.resample_quality, scipy._rates = SCIPY, {}
    for rate in (47999, 768000, 16000 * 4099):
        assert hq._rate_supported(rate)
    assert not scipy._rate_supported(47999) and scipy._rate_supported(48000)
    assert not hq._rate_supported(1 << 27)
